"""GPU tests of the merge kernels on their own (csrc/mci_static_kernels.h k_add_host_obs, k_hist_stage1, k_finalize and k_finish; the device
functions merge_stats, merge_hist_bin and merge_pa of csrc/mci_train.h), launched by the test hook Engine.merge_rows with the grids, thread
counts and dynamic LDS the product launches them with, over the made-up rows of tests/merge_cases.py: every case on both paths
(k_finalize at 256 threads; k_finish at 256 or 512, told to merge only).

Three yardsticks.  The float64 mirror of the kernels' order of operations: the SAME bits in packed, stage1, scratch, the block means and the
partial rows k_add_host_obs leaves behind -- the summation order is a contract.  The long-double reference: every entry within its own
derived bound, the "integers" cases exactly (the derivation is in merge_cases; tests/test_merge_host.py holds the mirror to it on the CPU
and shows that the bounds reject a lost row).  And what is known outright: no entry left unwritten, the status bit, the global histogram
buffers zeroed and nothing behind them touched.  Two launches per case (one per path); the outputs are computed once and shared."""
import numpy as np
import pytest

import merge_cases as M
from test_hip_parity import SEED, make
from test_merge_host import GROUPS, engine

pytestmark = pytest.mark.gpu

PATHS = ("finalize", "finish")
_OUT = {}


@pytest.fixture(scope="module")
def engines():
    """one engine per problem of merge_cases.SHAPES, for its device, its stream and its shape only"""
    engs = {name: engine(name) for name in M.SHAPES}
    for name, eng in engs.items():
        assert eng.merge_shape() == M.SHAPES[name]
    yield engs
    for eng in engs.values():
        eng.close()


def kernel(engines, c, path):
    key = (c["id"], path)
    if key not in _OUT:
        x = M.inputs(c)
        out = engines[c["problem"]].merge_rows(c["nblocks"], c["wpb"], x["part_cols"], part_hist=x["part_hist"], ghist=x["ghist"], part_pa=x["part_pa"],
                                               hold=x["hold"], obs=x["obs"], hist_no_offset=c["hist_no_offset"], block_means=c["block_means"], path=path)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _OUT[key] = out
    return _OUT[key]


def same_bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d of %d entries differ, first at %s" % (
        what, np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)), a.size, np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).ravel())[:8])


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_kernels_leave_what_the_mirror_leaves_bit_for_bit_on_both_paths(engines, group):
    for c in GROUPS[group]:
        mir = M.mirror(c)
        outs = [kernel(engines, c, path) for path in PATHS]
        for path, out in zip(PATHS, outs):
            who = "%s, %s" % (c["id"], path)
            same_bits(out["packed"], mir["packed"], who + ": packed")
            if c["hist_rows"]:
                same_bits(out["stage1"], mir["stage1"], who + ": stage1")
            else:                                   # no first stage: the hook's fill
                assert (out["stage1"].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all() and np.isnan(mir["stage1"]).all(), who
            same_bits(out["scratch"], mir["scratch"], who + ": scratch")
            same_bits(out["part_cols"], mir["part_cols"], who + ": part_cols")
            assert (out["block_means"] is None) == (mir["block_means"] is None) == (not c["block_means"])
            if c["block_means"]:
                same_bits(out["block_means"], mir["block_means"], who + ": block means")
            assert out["status"] == mir["status"], who
        for k in ("packed", "stage1", "scratch", "part_cols", "ghist"):           # k_finish (256 | 512 threads) against k_finalize (256)
            same_bits(outs[0][k], outs[1][k], c["id"] + ": the two paths' " + k)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_kernels_against_the_long_double_reference(engines, group):
    worst, at = 0.0, None
    for c in GROUPS[group]:
        for path in PATHS:
            w = M.check(c, kernel(engines, c, path), "kernel (%s)" % path)
            if w > worst:
                worst, at = w, c["id"]
    print("%-20s %3d cases x 2 paths, largest difference / derived bound %.4f (%s)" % (group, len(GROUPS[group]), worst, at))
    assert worst <= 1.0


def test_nothing_the_layout_names_is_left_unwritten(engines):
    """every output starts as 0xFF bytes (NaN): the whole reduce size of packed, every group of stage1 -- the empty ones too --, every
    block sum and block mean are written; only the "bad_norm" cases have NaN, exactly where the reference has them"""
    for c in M.cases():
        ref = M.reference(c)
        for path in PATHS:
            out = kernel(engines, c, path)
            who = (c["id"], path)
            assert np.array_equal(np.isnan(out["packed"]), np.isnan(ref["packed"])) and np.array_equal(np.isnan(out["scratch"]), np.isnan(ref["scratch"])), who
            assert c["values"] == "bad_norm" or not (np.isnan(out["packed"]).any() or np.isnan(out["scratch"]).any()), who
            assert np.isnan(out["stage1"]).all() if c["use_ghist"] else not np.isnan(out["stage1"]).any(), who
            if c["block_means"]:
                assert np.array_equal(np.isnan(out["block_means"]), np.isnan(ref["means"])), who


def test_the_normalization_bit_is_set_on_bad_norm_and_on_no_other_case(engines):
    seen = set()
    for c in M.cases():
        for path in PATHS:
            st = kernel(engines, c, path)["status"]
            assert st == (M.ST_NORMALIZATION if c["values"] == "bad_norm" else 0), (c["id"], path, st)
            seen.add(st)
    assert seen == {0, M.ST_NORMALIZATION}


def test_global_histogram_buffers_come_back_zero_and_the_row_behind_them_untouched(engines):
    n = 0
    for c in M.cases():
        if not c["use_ghist"]:
            continue
        lay, ref = M.layout(c), M.reference(c)
        for path in PATHS:
            out = kernel(engines, c, path)
            gh = out["ghist"]
            assert gh.shape == (c["use_ghist"] + 1, M.SHAPES[c["problem"]]["nbin"])
            assert not gh[:-1].any() and not np.signbit(gh[:-1]).any(), (c["id"], path)                  # zero again for the next iteration
            assert (gh[-1].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all(), (c["id"], path)                  # the guard row: the hook's fill, bit for bit
            lo, hi = lay["hist"]
            err = np.abs(out["packed"][lo:hi].astype(M.LD) - ref["packed"][lo:hi])
            assert np.all(err <= ref["bound"][lo:hi]) and (c["values"] != "integers" or not err.any()), (c["id"], path)
            n += 1
    assert n >= 2 * 2 * len(M.VALUES) * len(M.SHAPES)


def test_host_observables_change_the_first_row_of_each_block_and_nothing_else(engines):
    n = 0
    for c in M.cases():
        x, nobs = M.inputs(c), M.SHAPES[c["problem"]]["nobs"]
        for path in PATHS:
            left = kernel(engines, c, path)["part_cols"]
            want = x["part_cols"].copy()
            if c["obs"]:
                first = np.arange(c["nblocks"]) * c["wpb"]
                want[first, :nobs] = x["part_cols"][first, :nobs] + x["obs"]                         # one rounded addition each
                n += 1
            same_bits(left, want, "%s, %s: part_cols" % (c["id"], path))
    assert n >= 2 * 30


def test_the_hook_leaves_the_engine_alone(oracle):
    """mci_debug_merge takes the problem's device, stream and shape only: after hook calls on both paths -- one of them raising the hook's
    own normalization bit -- the engine's packed buffer, its status and its next iteration are those of a twin that never called it"""
    def started():
        eng = make("sphere2_padding", oracle)[2]
        eng.set_deterministic(True)                                       # (no float atomics: twins agree to the bit)
        eng.integrate("vegasmc", neval=4 * 500, niter=2, block=4, seed=SEED, nchain=4)
        eng.run("vegasmc", 500, 0, 4, 2, SEED, nchain=4)                  # ... and a merge still pending
        return eng
    eng, twin = started(), started()
    assert eng.merge_shape() == M.SHAPES["sphere2"]
    mine = [c for c in M.cases() if c["problem"] == "sphere2"]
    picks = [next(c for c in mine if c["values"] == v and bool(c["use_ghist"]) == g and c["obs"] == o)
             for v, g, o in (("uniform", False, False), ("bad_norm", False, False), ("signed", True, False), ("integers", False, True))]
    for i, c in enumerate(picks):
        x = M.inputs(c)
        out = eng.merge_rows(c["nblocks"], c["wpb"], x["part_cols"], part_hist=x["part_hist"], ghist=x["ghist"], part_pa=x["part_pa"], hold=x["hold"],
                             obs=x["obs"], hist_no_offset=c["hist_no_offset"], block_means=c["block_means"], path=PATHS[i % 2])
        assert out["status"] == M.reference(c)["status"]
    eng.check_status()                                                     # (the hook's normalization bit never reached the problem's word)
    twin.check_status()
    assert eng.get_packed(reduce_size=True).tobytes() == twin.get_packed(reduce_size=True).tobytes()
    for e in (eng, twin):
        e.finish("vegasmc", 4, adapt=True)
    assert eng.grid(0).tobytes() == twin.grid(0).tobytes() and eng.reweight().tobytes() == twin.reweight().tobytes()
    a = eng.iteration("vegasmc", 500, 0, 4, iteration=3, seed=SEED, nchain=4)
    b = twin.iteration("vegasmc", 500, 0, 4, iteration=3, seed=SEED, nchain=4)
    assert a.tobytes() == b.tobytes()
    eng.check_status()
    eng.close()
    twin.close()


@pytest.mark.parametrize("layout,solver", [("c2_gauss4_composite", "vegas"), ("discrete2_composite", "vegas"), ("sphere2_padding", "vegasmc")])
def test_merging_inside_the_refinement_launch_or_ahead_of_it_gives_the_same_bytes(oracle, layout, solver):
    """the product's two routes, no hook involved: run -> finish(adapt) takes merge and refinement as ONE launch (k_finish); run ->
    get_packed -> finish(adapt) takes k_finalize, then k_train on the merged histogram in `packed`"""
    kw = dict(nchain=4) if solver != "vegas" else {}
    twins = [make(layout, oracle)[2] for _ in range(2)]
    for eng in twins:
        eng.set_deterministic(True)                                         # (no float atomics: what differs, the routes made differ)
    looked = None
    for it in range(2):
        for k, eng in enumerate(twins):
            eng.run(solver, 2000, 0, 4, it, SEED, **kw)
            if k == 1:
                looked = eng.get_packed()
            eng.finish(solver, 4, adapt=True)
    one, two = twins
    nstat = one.merge_shape()["nstat"]
    for leaf, lf in enumerate(one.config.leaves):
        if hasattr(lf, "ninc"):
            assert one.grid(leaf).tobytes() == two.grid(leaf).tobytes(), leaf
            assert not np.array_equal(one.grid(leaf), np.linspace(lf.lower, lf.upper, lf.ninc))      # (the refinement did run)
        else:
            (d1, a1), (d2, a2) = one.distribution(leaf), two.distribution(leaf)
            assert d1.tobytes() == d2.tobytes() and a1.tobytes() == a2.tobytes(), leaf
            assert not np.array_equal(d1, np.full(d1.size, 1.0 / d1.size))
    assert one.reweight().tobytes() == two.reweight().tobytes()
    rows = [eng.iteration_log(2) for eng in twins]
    assert rows[0].tobytes() == rows[1].tobytes() and rows[0][1].tobytes() == looked[:nstat].tobytes()
    for eng in twins:                                                       # clearStatistics!: the histogram section sits at 1e-10
        sh = eng.merge_shape()
        h = eng.get_packed()[nstat:nstat + sh["nbin"]]
        assert h.tobytes() == np.full(sh["nbin"], 1.0e-10).tobytes()
        eng.check_status()
        eng.close()
