"""CPU tests of the block merge's test harness (tests/merge_cases.py): the float64 mirror of the kernels' order of operations against the
independent long-double reference over the whole case table -- which proves that the derived bounds can be met without the kernel --, three
deliberate mistakes planted into the mirror that the reference check must reject -- which proves that the bounds have teeth --, the table's
coverage, and the refusals of the test hook (csrc/mci_debug.h mci_debug_merge through Engine.merge_rows), which need no device."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import merge_cases as M
from test_sweep_leaves_host import discrete2


def engine(problem, **kw):
    """the engine of a problem of merge_cases.SHAPES (tests/test_hip_merge.py builds the same ones on a device)"""
    if problem == "discrete2":
        cfg, f = mci.Configuration(var=mci.Discrete([(1, 3), (1, 4)]), dof=[[1]]), mci.catalog.one()
    elif problem == "sphere2":
        cfg, f = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2()
    else:
        var = (mci.Continuous(0.0, 1.0, ninc=301), mci.Continuous(0.0, 2.0, ninc=41), mci.Discrete(1, 4))
        cfg, f = mci.Configuration(var=var, dof=[[1, 1, 1], [1, 1, 1]]), mci.catalog.one()
    return mci.Engine(cfg, f, **kw)


GROUPS = {}
for _c in M.cases():
    GROUPS.setdefault("%s-%s" % (_c["problem"], _c["values"]), []).append(_c)


def pick(**want):
    """the first case of the table with these properties"""
    return next(c for c in M.cases() if all(c[k] == v for k, v in want.items()))


@pytest.mark.parametrize("problem", list(M.SHAPES))
def test_the_shapes_of_the_table_are_the_engines(problem):
    eng = engine(problem, device=-1)
    assert eng.merge_shape() == M.SHAPES[problem]
    sh = M.SHAPES[problem]
    assert eng.packed_size == sh["nstat"] + sh["nbin"] + 2 * sh["npa"] and eng.reduce_size == eng.packed_size + 64
    assert discrete2().merge_shape() == M.SHAPES["discrete2"]


def test_the_table_covers_what_it_is_for():
    cs = M.cases()
    print(len(cs), "cases")
    assert 300 <= len(cs) <= 600
    sh = M.SHAPES
    assert any(s["nbin"] < 256 for s in sh.values()) and any(s["nbin"] > 256 and s["nbin"] % 256 and s["maxn"] > 256 for s in sh.values())
    assert any(len(s["leaves"]) > 2 for s in sh.values()) and all(s["nobs"] >= 1 for s in sh.values()) and any(s["nobs"] >= 2 for s in sh.values())
    assert sh["sphere2"]["ni"] == 2 and sh["sphere2"]["npa"] == 27 and (2 * sh["sphere2"]["npa"]) % 4
    for values in M.VALUES:
        mine = [c for c in cs if c["values"] == values]
        assert {c["hist_rows"] for c in mine} == set(M.HIST_ROWS) | {0} and {c["use_ghist"] for c in mine} == set(M.USE_GHIST) | {0}
        assert {c["wpb"] for c in mine} >= set(M.WG_PER_BLOCK) and {c["nblocks"] for c in mine} >= set(M.NBLOCKS) | set(M.OBS_NBLOCKS)
        assert {c["nrows"] for c in mine} >= set(M.NROWS) and {c["problem"] for c in mine} == set(sh)
        for flag in ("pa", "hold", "obs", "block_means"):
            assert {bool(c[flag]) for c in mine} == {False, True}, (values, flag)
        assert {c["hist_no_offset"] for c in mine} == ({1} if values == "integers" else {0, 1})
        assert {(c["pa"], c["hold"]) for c in mine} == {(False, False), (False, True), (True, False), (True, True)}
        assert any(c["nrows"] > c["nblocks"] * c["wpb"] for c in mine)
    for h in M.HIST_ROWS + M.USE_GHIST:
        assert {c["problem"] for c in cs if h in (c["hist_rows"], c["use_ghist"])} == set(sh)
    # the strides of merge_stats' first loop: nblocks * ncols on both sides of 32 (256 threads) and of 64 (512 threads: a leaf of > 256 bins)
    cells = {(c["nblocks"] * sh[c["problem"]]["ncols"], sh[c["problem"]]["maxn"] > 256) for c in cs}
    assert {(30, False), (35, False), (28, True), (35, True), (63, True), (70, True), (60, False), (65, False)} <= cells
    # k_add_host_obs: nblocks * nobs on both sides of its 256 threads
    assert {c["nblocks"] * sh[c["problem"]]["nobs"] for c in cs if c["obs"]} >= {254, 256, 258, 127, 128, 129}
    for c in cs:
        assert c["nrows"] >= c["nblocks"] * c["wpb"] and bool(c["hist_rows"]) != bool(c["use_ghist"]), c["id"]
        assert max(c["nrows"] * 2 * sh[c["problem"]]["npa"], max(c["hist_rows"], 1) * sh[c["problem"]]["nbin"]) <= 2049 * 999


def test_no_normalization_of_the_table_is_close_to_zero():
    """the quotient's bound needs dN < |N|: held with twenty bits to spare on every block of every case (bad_norm: on its finite blocks)"""
    for c in M.cases():
        r = M.reference(c)
        fin = np.isfinite(r["N"])
        assert fin.all() or c["values"] == "bad_norm", c["id"]
        assert np.all(r["dN"][fin] * 2.0 ** 20 < np.abs(r["N"][fin])), c["id"]
        assert (r["status"] != 0) == (c["values"] == "bad_norm"), c["id"]
        assert np.all(r["bound"] >= 0) or c["values"] == "bad_norm"


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_mirror_lies_within_the_derived_bounds_of_the_reference(group):
    worst = 0.0
    for c in GROUPS[group]:
        out = M.mirror(c)
        worst = max(worst, M.check(c, out, "mirror"))
        lay = M.layout(c)
        assert not np.isnan(out["packed"][lay["hist"][0]:]).any() and not np.isnan(out["part_cols"][:, M.SHAPES[c["problem"]]["nobs"] + 1:]).any(), c["id"]
    print("%-20s %3d cases, largest difference / bound %.3f" % (group, len(GROUPS[group]), worst))
    assert worst <= 1.0


def named(mutation, values):
    """cases on which the mistake loses a row: histogram rows that are no multiple of 32 | rows per block that are no multiple of 8"""
    if mutation == "short_row_loop":
        return [pick(values=values, wpb=w) for w in (1, 7, 9, 17)]
    if mutation == "per_floor":
        return [pick(values=values, hist_rows=h) for h in (1, 3, 31, 33, 65, 129, 2049)]
    return [pick(values=values, hist_rows=h) for h in (1, 33, 129, 160, 256, 2049)]


@pytest.mark.parametrize("values", [v for v in M.VALUES if v != "decades"])
@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_the_bounds_reject_a_mirror_that_loses_a_row(mutation, values):
    """(not "decades": a lost row thirty decades below the sum is below any honest bound)"""
    for c in named(mutation, values):
        M.check(c, M.mirror(c), "mirror")
        with pytest.raises(AssertionError, match="differs from the exact sum" if values == "integers" else "off at|differs from|is NaN at"):
            M.check(c, M.mirror(c, mutate=mutation), "mutated mirror")


def test_an_unchanged_geometry_lets_the_mistakes_through():
    """the mistakes are geometry bugs: where rows divide evenly they change nothing, which is why the table needs the odd sizes"""
    c = pick(hist_rows=64, wpb=8)
    for mutation in ("short_row_loop", "per_floor"):
        assert M.mirror(c, mutate=mutation)["packed"].tobytes() == M.mirror(c)["packed"].tobytes()


def test_the_hook_refuses_bad_arguments_without_a_device():
    eng = engine("sphere2", device=-1)
    sh = M.SHAPES["sphere2"]
    cols, hist = np.ones((6, sh["ncols"])), np.ones((3, sh["nbin"]))
    good = dict(nblocks=2, wg_per_block=3, part_cols=cols, part_hist=hist)
    for bad, match in ((dict(nblocks=0), "0 blocks"), (dict(wg_per_block=0), "of 0 rows"), (dict(nblocks=-1), "-1 blocks"),
                       (dict(nblocks=3), "6 rows for 3 blocks of 3"), (dict(part_hist=None), "one of hist_rows and use_ghist"),
                       (dict(ghist=np.ones((1, sh["nbin"]))), "exclude each other"),
                       (dict(part_hist=None, ghist=np.ones((65, sh["nbin"]))), "65 global histogram buffers"),
                       (dict(nblocks=2 ** 30, wg_per_block=4), "more than a test hook takes"),
                       (dict(nblocks=2 ** 29), "more than a test hook takes")):
        with pytest.raises(mci.MCIError, match=match):
            eng.merge_rows(**dict(good, **bad))
    for bad in (dict(part_cols=np.ones((6, sh["ncols"] + 1))), dict(part_hist=np.ones((3, sh["nbin"] - 1))), dict(part_pa=np.ones((6, 2 * sh["npa"] + 1))),
                dict(hold=np.zeros(63, dtype=np.uint64)), dict(obs=np.ones((3, sh["nobs"]))), dict(path="both")):
        with pytest.raises(ValueError):
            eng.merge_rows(**dict(good, **bad))
    for extra in (dict(), dict(path="finish"), dict(part_hist=None, ghist=np.ones((3, sh["nbin"]))), dict(part_pa=np.ones((6, 2 * sh["npa"])))):
        with pytest.raises(mci.MCIError, match="offline"):              # good arguments get as far as the device
            eng.merge_rows(**dict(good, **extra))
