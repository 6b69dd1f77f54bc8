"""GPU tests of train! on its own (csrc/mci_train.h train_leaf, do_reweight_dev, iteration_bookkeeping; launched as k_train,
csrc/mci_static_kernels.h) over the made-up histograms of tests/train_cases.py, driven through the public route of a multi-rank run:
set_grid -> set_packed -> train() (mci_set_grid, mci_set_packed, mci_train), then grid / distribution, get_packed and walk_counts.
Every other test that reaches this code feeds it a histogram the sample kernels produced: positive, smooth, 999 bins or a few more.

Every case runs under four walks -- `prefix` (scan + bisection), `serial` (the recurrence as slots with given decisions), `serial_general`
(the hand-written recurrence) and `serial_wrong_decision` (slots with one decision planted wrong) -- once; the outputs are shared.
Yardsticks: the long-double reference with bounds derived per entry (train_cases; tests/test_train_host.py holds the CPU oracle to them and
shows that they reject planted mistakes); the three serial walks against each other, bit for bit; and what is known outright: end points,
monotonicity, clearStatistics!, everything train! must not touch, the metamorphic pair lognormal | pow2, the status paths."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import train_cases as T
from test_hip_parity import SEED, make
from test_train_host import FAMILY_CASES, GAMMAS, GOALS, NOT_STRICT, START, VISITED, engine, reweight_engine

pytestmark = pytest.mark.gpu

WALKS = ("prefix", "serial", "serial_general", "serial_wrong_decision")
SERIAL = WALKS[1:]
MODE = {"prefix": "scan", "serial": "serial", "serial_general": "serial_general", "serial_wrong_decision": "serial_wrong_decision"}
_OUT = {}


class Engines:
    """one engine per problem of the table, created when first asked for"""

    def __init__(self):
        self.engs, self.shapes = {}, {}

    def get(self, name):
        if name not in self.engs:
            self.engs[name] = engine(name)
            self.shapes[name] = self.engs[name].merge_shape()
        return self.engs[name], self.shapes[name]

    def close(self):
        for eng in self.engs.values():
            eng.close()


@pytest.fixture(scope="module")
def engines():
    e = Engines()
    yield e
    e.close()


def made_up(eng, sh, hists):
    """a packed row: a made-up statistics head, the case's histograms, a recognisable fill behind them"""
    p = np.empty(eng.packed_size)
    nstat, nbin = sh["nstat"], sh["nbin"]
    p[:nstat] = 1.5 + 0.25 * np.arange(nstat)
    for (off, n), h in zip(sh["leaves"], hists):
        assert h.shape == (n,)
        p[nstat + off:nstat + off + n] = h
    p[nstat + nbin:] = 0.015625 * (1.0 + np.arange(p.size - nstat - nbin))
    return p


def start_distribution(n):
    return (1.0 + np.arange(n)) / (n * (n + 1) / 2.0)


def launch(engines, c, walk, leaves):
    eng, sh = engines.get(c["problem"])
    assert [(k == "c", n) for k, n, a, ad, g, h in leaves] == [(hasattr(lf, "ninc"), nb) for lf, (off, nb) in zip(eng.config.leaves, sh["leaves"])]
    eng.set_train_walk(MODE[walk])
    before = []
    for l, (k, n, a, ad, g, h) in enumerate(leaves):
        if k == "c":
            eng.set_grid(l, g)
            before.append(eng.grid(l))
        else:
            eng.set_distribution(l, start_distribution(n))
            before.append(eng.distribution(l))
    p = made_up(eng, sh, [lf[5] for lf in leaves])
    c0 = eng.walk_counts()
    eng.set_packed(p)
    eng.train()
    c1 = eng.walk_counts()
    out = dict(leaves=[eng.grid(l) if lf[0] == "c" else eng.distribution(l) for l, lf in enumerate(leaves)], before=before, packed_in=p,
               packed=eng.get_packed(), counts=(c1[0] - c0[0], c1[1] - c0[1]))
    return out


def kernel(engines, c, walk):
    key = (c["id"], walk)
    if key not in _OUT:
        _OUT[key] = launch(engines, c, walk, T.leaf_inputs(c))
    return _OUT[key]


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def leaf_bits(x):
    return x.tobytes() if isinstance(x, np.ndarray) else x[0].tobytes() + x[1].tobytes()


@pytest.mark.parametrize("family", sorted(FAMILY_CASES))
def test_every_walk_against_the_long_double_reference(engines, family):
    """worst |kernel - reference| / derived bound per walk, and max |kernel - reference| / (upper - lower) next to the 1e-12 x range of
    tests/test_hip_parity.py test_train_matches_oracle (which compares with the oracle on sampled histograms; on these made-up ones
    both kernel and oracle are further than that from the exact result wherever a bin of the 1e-10 fill must take a new point)"""
    worst, wrange, at = dict.fromkeys(WALKS, 0.0), dict.fromkeys(WALKS, 0.0), dict.fromkeys(WALKS)
    for c in FAMILY_CASES[family]:
        leaves = T.leaf_inputs(c)
        for walk in WALKS:
            out = kernel(engines, c, walk)
            for l, leaf in enumerate(leaves):
                if not leaf[3]:
                    continue
                w, r = T.check_leaf(leaf, out["leaves"][l], "kernel (%s), case %s leaf %d" % (walk, c["id"], l))
                wrange[walk] = max(wrange[walk], r)
                if w > worst[walk]:
                    worst[walk], at[walk] = w, c["id"]
    for walk in WALKS:
        print("%-12s %-22s %3d cases, largest difference / derived bound %.4f (%s), largest difference / range %.3g"
              % (family, walk, len(FAMILY_CASES[family]), worst[walk], at[walk], wrange[walk]))
    assert max(worst.values()) <= 1.0


def test_the_serial_walks_leave_identical_bytes_on_every_case(engines):
    n = 0
    for c in T.cases():
        outs = [kernel(engines, c, walk) for walk in SERIAL]
        for walk, out in zip(SERIAL[1:], outs[1:]):
            for l in range(len(out["leaves"])):
                assert leaf_bits(out["leaves"][l]) == leaf_bits(outs[0]["leaves"][l]), (c["id"], walk, l)
            assert same_bits(out["packed"], outs[0]["packed"]), (c["id"], walk)
            n += 1
    assert n == 2 * len(T.cases())


def expected_counts(leaves, walk):
    """(walks run as slots, walks in the general form) of one launch, from the code of train_leaf where it can be told ahead: `given`
    needs the slots' LDS (train_lds_bytes' spare, decided by the LARGEST leaf), a serial_walk other than 2 and N > 1; the planted wrong
    decision sits in bin N / 2 and is looked at only where N / 2 < N - 1, i.e. N >= 3.  None: depends on the bins (below)"""
    spare = T.has_spare(max(n for k, n, a, ad, g, h in leaves))
    slots = general = 0
    unknown = False
    for k, n, a, ad, g, h in leaves:
        if k != "c" or not ad or walk == "prefix":
            continue
        if walk == "serial_general" or not spare or n == 1:
            general += 1
        elif walk == "serial_wrong_decision" and n >= 3:
            general += 1
        else:
            unknown = True       # slots, unless a decision taken from the prefix sums does not hold (C[j] within rounding of a multiple of f_ninc)
            slots += 1
    return slots, general, unknown


def test_walk_counts_tell_which_form_ran(engines):
    """the slots form on N_fit and the general form on N_fit + 1 (the Python formula of train_lds_bytes is the device's); the planted
    wrong decision is caught every time; the prefix-scan walk counts nothing.  Whether `serial` keeps its slots depends on the bins: a
    bin that takes SEVERAL new points does not by itself leave the slots form (slots() emits c - 1 subtractions and one merged or
    plain addition); only a decision floor(C[j] / f_ninc) - floor(C[j-1] / f_ninc) that differs from the recurrence's count does, which
    needs C[j] / f_ninc within rounding of an integer.  So the spike families are expected to run as slots -- their one heavy bin takes
    hundreds of points through the slots -- except where such a tie occurs; `flat`, `ones` and `comb`, whose C[j] / f_ninc are integers
    or half-integers up to rounding, are where ties live.  Printed per family; asserted: every launch counts each trained Continuous
    leaf exactly once, in the form the code dictates where that can be told ahead."""
    fell = {}
    for c in T.cases():
        leaves = T.leaf_inputs(c)
        for walk in WALKS:
            slots, general, unknown = expected_counts(leaves, walk)
            got = kernel(engines, c, walk)["counts"]
            assert sum(got) == slots + general and got[1] >= general, (c["id"], walk, got, slots, general)
            if not unknown:
                assert got == (slots, general), (c["id"], walk, got)
            elif walk == "serial":
                f = fell.setdefault(c["family"] if c["kind"] != "m" else "mixed", [0, 0])
                f[0] += got[1] - general
                f[1] += slots
    for fam, (a, b) in sorted(fell.items()):
        print("%-12s serial: %3d of %3d walks that started as slots fell back to the general form" % (fam, a, b))
    fit = [c for c in T.cases() if c["kind"] == "c" and c["n"] in (T.N_FIT, T.N_FIT + 1)]
    assert len(fit) == 2 * len(T.FAMILIES) * len(T.GRIDS)
    for c in fit:
        assert kernel(engines, c, "serial_wrong_decision")["counts"] == (0, 1)
        if c["n"] == T.N_FIT + 1:
            assert kernel(engines, c, "serial")["counts"] == (0, 1), c["id"]
    # ... and on N_fit the slots do run (on every family without ties in it)
    assert all(kernel(engines, c, "serial")["counts"] == (1, 0) for c in fit if c["n"] == T.N_FIT and c["family"] in ("lognormal", "pow2", "ramp", "tiny"))
    spikes = [kernel(engines, c, "serial")["counts"] for c in T.cases() if c["kind"] == "c" and c["family"].startswith("spike") and 17 <= c["n"] <= T.N_FIT]
    assert spikes.count((1, 0)) > len(spikes) // 2          # a heavy bin alone does not leave the slots form


def test_what_is_known_outright(engines):
    for c in T.cases():
        leaves = T.leaf_inputs(c)
        _, sh = engines.get(c["problem"])
        nstat, nbin = sh["nstat"], sh["nbin"]
        for walk in WALKS:
            out, who = kernel(engines, c, walk), (c["id"], walk)
            pin, pout = out["packed_in"], out["packed"]
            assert same_bits(pout[:nstat], pin[:nstat]) and same_bits(pout[nstat + nbin:], pin[nstat + nbin:]), who     # head and tail untouched
            for l, ((k, n, a, ad, g, h), (off, nb)) in enumerate(zip(leaves, sh["leaves"])):
                section = pout[nstat + off:nstat + off + nb]
                if not ad:                                   # variable.jl:208 / :370 return before clearStatistics!
                    assert same_bits(section, h) and leaf_bits(out["leaves"][l]) == leaf_bits(out["before"][l]), who
                    continue
                assert same_bits(section, np.full(nb, 1.0e-10)), who                                              # clearStatistics!
                if k == "c":
                    new = out["leaves"][l]
                    assert new[0].tobytes() == g[0].tobytes() and new[-1].tobytes() == g[-1].tobytes(), who       # the old end points, bit for bit
                    w = np.diff(new)
                    assert np.all(w >= 0), who
                    if c["grid"] == "uniform" or c["id"] not in NOT_STRICT:
                        assert np.all(w > 0), (who, np.flatnonzero(w <= 0)[:8])
                    if n == 1:
                        assert same_bits(new, g), who
                else:
                    dist, acc = out["leaves"][l]
                    assert acc[0] == 0.0 and not np.signbit(acc[0]) and np.all(np.diff(acc) >= 0) and np.all(dist >= 0), who
                    if n == 1:                               # rescale leaves one bin alone (common.jl:68-70); normalised, it is 1
                        assert same_bits(dist, [1.0]) and same_bits(acc, [0.0, 1.0]), who


def test_a_power_of_two_scale_changes_no_byte(engines):
    """smoothing, the division by the sum and everything after it are exact under a power-of-two scale of the histogram"""
    n = 0
    for c in T.cases():
        if c["family"] != "pow2":
            continue
        twin = next(x for x in T.cases() if x["problem"] == c["problem"] and x["grid"] == c["grid"] and x["family"] == "lognormal")
        for walk in WALKS:
            a, b = kernel(engines, c, walk), kernel(engines, twin, walk)
            assert leaf_bits(a["leaves"][0]) == leaf_bits(b["leaves"][0]) and a["counts"] == b["counts"], (c["id"], walk)
            n += 1
    assert n >= 4 * 90


def test_one_leafs_histogram_changes_no_other_leafs_output(engines):
    mixed = [c for c in T.cases() if c["kind"] == "m"]
    for c in mixed[:4]:
        leaves = T.leaf_inputs(c)
        for walk in ("prefix", "serial"):
            base = kernel(engines, c, walk)
            for l, (k, n, a, ad, g, h) in enumerate(leaves):
                other = T.hist(n, "ramp" if c["families"][l] != "ramp" else "comb")
                changed = [lf if i != l else (k, n, a, ad, g, other) for i, lf in enumerate(leaves)]
                out = launch(engines, c, walk, changed)
                for i in range(len(leaves)):
                    if i != l:
                        assert leaf_bits(out["leaves"][i]) == leaf_bits(base["leaves"][i]), (c["id"], walk, l, i)
                    elif ad:
                        assert leaf_bits(out["leaves"][i]) != leaf_bits(base["leaves"][i]), (c["id"], walk, l)
                    else:
                        assert leaf_bits(out["leaves"][i]) == leaf_bits(out["before"][i])


def test_small_leaves_trained_by_512_threads_equal_the_same_leaves_alone(engines):
    """the 41- and 17-bin leaves of the mixed problem run on 512 threads next to a 1200-bin leaf (and meet the reference's bounds there,
    test_every_walk_against_the_long_double_reference); the serial walks, whose order of operations does not depend on the thread
    count, give the bytes a one-leaf problem of that size gives on 256 threads"""
    for c in [c for c in T.cases() if c["kind"] == "m"]:
        leaves = T.leaf_inputs(c)
        for l, (k, n, a, ad, g, h) in enumerate(leaves):
            if k != "c" or not ad or n > 256:
                continue
            alone = dict(id="alone-%s-%d" % (c["id"], l), problem=T.problem_name("c", n, a), kind="c", n=n, alpha=a, grid=c["grid"], family=c["families"][l])
            assert T.train_threads(n) == 256
            for walk in ("serial", "serial_general"):
                assert same_bits(kernel(engines, c, walk)["leaves"][l], kernel(engines, alone, walk)["leaves"][0]), (c["id"], l, walk)


def test_the_sum_of_a_long_histogram_is_split_where_julia_splits_it(engines, oracle):
    """train_cases.assoc_hist: distribution[512] follows sum(h) bit by bit, and the oracle's association of that sum (mcio_sum_julia: halves
    of 513 | 512 elements, sixteen interleaved partial sums) is sixteen ulps of the sum away from the split the other way round --
    more than 24 units of 2^-53 distribution[512] (tests/test_train_host.py; 31 by the arithmetic).  The allowance, in the same units:
    v = h[512] / sum(h) is the same double on both sides; each of the other 1024 bins is (1 - v) / (-log v), (2 + 2 L) u = 8 u from the
    device with L = 3 ulp and 4 u from the host's libm, so the two sums of d differ by at most 12 u = 6 units if every bin errs the
    same way, plus what the two left-to-right additions then round differently and the two quotients: 12 units, half of 24"""
    h = T.assoc_hist()
    leaf = ("d", T.ASSOC_K, T.ASSOC_ALPHA, True, None, h)
    c = dict(id="assoc", problem=T.problem_name("d", T.ASSOC_K, T.ASSOC_ALPHA))
    dist, acc = launch(engines, c, "serial", [leaf])["leaves"][0]
    odist, oacc = oracle.train_discrete(h, T.ASSOC_ALPHA)
    unit = 2.0 ** -53 * odist[T.ASSOC_BIN]
    print("distribution[512]: kernel - oracle = %.3g units of 2^-53 of its size" % ((dist[T.ASSOC_BIN] - odist[T.ASSOC_BIN]) / unit))
    assert abs(dist[T.ASSOC_BIN] - odist[T.ASSOC_BIN]) <= 12 * unit
    assert T.check_leaf(leaf, (dist, acc), "kernel, assoc")[0] <= 1.0


def finish_picks():
    """a dozen cases: six of the mixed problem, six of the 999-bin problem (every family once, both grids)"""
    mixed = [c for c in T.cases() if c["kind"] == "m"][:6]
    one = [c for c in T.cases() if c["kind"] == "c" and c["n"] == 999 and c["alpha"] == 2.0]
    fams = ("spike", "flat", "lognormal", "comb", "tiny", "spike_last")
    return mixed + [next(c for c in one if c["family"] == f and c["grid"] == T.GRIDS[i % 2]) for i, f in enumerate(fams)]


@pytest.mark.parametrize("walk", ["prefix", "serial", "serial_wrong_decision"])
def test_k_finish_trains_from_its_lds_copy_as_k_train_does_from_packed(engines, walk):
    """k_finish's route (merge, then train_leaf from the merged histogram in LDS: `staged`, the LDS copy, `spare` aliasing the histogram),
    through Engine.merge_rows(train=...) on the hook's own tables: the case's histograms go in as partial rows or global buffers, the
    float64 mirror of the merge (merge_cases.mirror) predicts the merged histogram, and k_train fed that histogram at the same thread
    count must leave the same bytes"""
    import merge_cases as M
    for i, c in enumerate(finish_picks()):
        eng, sh = engines.get(c["problem"])
        leaves = T.leaf_inputs(c)
        nstat, nbin = sh["nstat"], sh["nbin"]
        rng = np.random.default_rng([T.SEED, i])
        hrows, k = ((5, 0), (40, 0), (0, 3))[i % 3]
        full = np.concatenate([lf[5] for lf in leaves])
        w = rng.dirichlet(np.ones(hrows or k))[:, None] * np.ones((1, nbin))
        rows = w * full[None, :]
        mc = dict(problem=c["problem"], nblocks=3, wpb=2, nrows=6, hist_rows=hrows, use_ghist=k, hist_no_offset=i % 2, block_means=False)
        x = dict(part_cols=rng.uniform(0.5, 1.5, (6, sh["ncols"])), part_hist=rows if hrows else None, ghist=rows if k else None, part_pa=None,
                 hold=None, obs=None)
        mir = M.mirror(mc, shape=sh, x=x)
        merged = mir["packed"][nstat:nstat + nbin]
        assert np.all(merged > 0) and np.all(np.isfinite(merged))
        fed = [lf[:5] + (merged[off:off + n].copy(),) for lf, (off, n) in zip(leaves, sh["leaves"])]
        ref = launch(engines, c, walk, fed)                                            # k_train on the predicted histogram
        cont = [l for l, lf in enumerate(leaves) if lf[0] == "c"]
        disc = [l for l, lf in enumerate(leaves) if lf[0] == "d"]
        out = eng.merge_rows(3, 2, x["part_cols"], part_hist=x["part_hist"], ghist=x["ghist"], hist_no_offset=mc["hist_no_offset"], block_means=False,
                             path="finish", train=MODE[walk], grids=[leaves[l][4] for l in cont], tables=[ref["before"][l] for l in disc])
        who = (c["id"], walk)
        assert out["status"] == 0 and out["walk_counts"] == ref["counts"], (who, out["walk_counts"], ref["counts"])
        for j, l in enumerate(cont):
            assert same_bits(out["grids"][j], ref["leaves"][l]), (who, l)
        for j, l in enumerate(disc):
            assert leaf_bits(out["tables"][j]) == leaf_bits(ref["leaves"][l]), (who, l)
        assert same_bits(out["packed"][:nstat], mir["packed"][:nstat]), who                 # the merge itself: still the mirror's
        for lf, (off, n) in zip(leaves, sh["leaves"]):
            want = np.full(n, 1.0e-10) if lf[3] else merged[off:off + n]
            assert same_bits(out["packed"][nstat + off:nstat + off + n], want), who
        for l, lf in enumerate(leaves):                                                    # the engine's own tables: where k_train left them
            got = eng.grid(l) if lf[0] == "c" else eng.distribution(l)
            assert leaf_bits(got) == leaf_bits(ref["leaves"][l]), who


BAD_MESSAGE = {"nan": "histogram should be all finite", "inf": "histogram should be all finite", "zero": "all positive and non-zero",
               "minus_one": "all positive and non-zero", "minus_zero": "all positive and non-zero"}


@pytest.mark.parametrize("kind,n", [("c", T.BAD_N), ("d", 17)])
def test_a_bad_bin_raises_its_message_and_leaves_everything_as_it_was(engines, kind, n):
    """check_status orders the messages: non-finite before non-positive.  A rescale that goes non-finite cannot be had from finite
    positive bins (tests/test_train_host.py test_a_rescale_that_goes_non_finite_needs_a_bad_bin), so that path and a bad f_ninc, which
    needs the same, are not forced here"""
    c = next(c for c in T.cases() if c["kind"] == kind and c["n"] == n and c["alpha"] == 2.0 and c["family"] == "lognormal")
    eng, sh = engines.get(c["problem"])
    (leaf,) = T.leaf_inputs(c)
    places = T.bad_places(n) if kind == "c" else dict(first=0, middle=n // 2, last=n - 1)
    for walk in ("serial", "prefix"):
        good = kernel(engines, c, walk)
        for name, value in T.BAD_VALUES + (("nan_and_zero", None),):
            for where, at in places.items():
                h = leaf[5].copy()
                h[at] = np.nan if value is None else value
                if value is None:
                    h[(at + 1) % n] = 0.0
                with pytest.raises(mci.MCIError, match=BAD_MESSAGE["nan" if value is None else name]):
                    launch(engines, c, walk, [leaf[:5] + (h,)])
                after = eng.grid(0) if kind == "c" else eng.distribution(0)
                assert leaf_bits(after) == leaf_bits(good["before"][0]), (walk, name, where)               # grid | tables as they went in
                assert same_bits(eng.get_packed(), made_up(eng, sh, [h])), (walk, name, where)            # the bad bin included
                eng.check_status()                                                                     # the status word was cleared
        again = launch(engines, c, walk, [leaf])                                                       # a good train() right after
        assert leaf_bits(again["leaves"][0]) == leaf_bits(good["leaves"][0]), walk


def test_set_packed_refuses_a_wrong_length(engines):
    eng, sh = engines.get(T.problem_name("c", 17, 2.0))
    before = eng.get_packed()
    for n in (eng.packed_size - 1, eng.packed_size + 1, eng.packed_size + 63, 0):
        with pytest.raises(mci.MCIError, match="packed size is %d" % eng.packed_size):
            eng.set_packed(np.zeros(n))
    assert same_bits(eng.get_packed(), before)
    eng.set_packed(np.concatenate([before, np.zeros(64)]))                 # (the reduce size, with the 64 holding counts, is taken)


def test_do_reweight_against_the_reference():
    """set_reweight -> set_packed with made-up visited counts -> finish("vegasmc", adapt=False, gamma): k_train's bookkeeping workgroup"""
    eng = reweight_engine()
    sh = eng.merge_shape()
    nstat, nd = sh["nstat"], 3
    worst = 0.0
    rows = 0
    g0 = eng.grid(0)
    for name, vis in VISITED.items():
        for gamma in GAMMAS:
            for goal in GOALS:
                eng.set_reweight_goal(goal)
                eng.set_reweight(START)
                r0 = eng.reweight()
                p = made_up(eng, sh, [T.hist(999, "lognormal")])
                p[nstat - nd:nstat] = vis
                eng.set_packed(p)
                eng.finish("vegasmc", 4, adapt=False, gamma=gamma)
                rows += 1
                got = eng.reweight()
                ref, bound = T.ref_reweight(r0, vis, gamma, goal)
                worst = max(worst, T.ratio(got, ref, bound, "reweight %s gamma %g goal %s" % (name, gamma, goal)))
                assert abs(float(got.astype(T.LD).sum() - 1)) <= 4 * float(T.EPS), (name, gamma, goal)
                assert same_bits(eng.iteration_log(1)[0], p[:nstat])                                    # the log row: the head that went in
                assert same_bits(eng.get_packed(), p) and same_bits(eng.grid(0), g0)                    # adapt=False: nothing trained or cleared
    eng.set_reweight_goal(None)
    print("doReweight!: %d launches, largest difference / derived bound %.4f" % (rows, worst))
    assert worst <= 1.0
    eng.close()


@pytest.mark.parametrize("layout,solver", [("c2_gauss4_composite", "vegas"), ("discrete2_composite", "vegas"), ("sphere2_padding", "vegasmc")])
def test_train_on_a_packed_row_handed_back_equals_finish(oracle, layout, solver):
    """the multi-rank route after a real run: run -> get_packed -> set_packed of the same bytes -> train() (k_finalize, then k_train)
    against a twin's run -> finish(adapt=True) (k_finish), both deterministic: the same grids and tables, bit for bit"""
    kw = dict(nchain=4) if solver != "vegas" else {}
    one, two = [make(layout, oracle)[2] for _ in range(2)]
    for eng in (one, two):
        eng.set_deterministic(True)
        eng.run(solver, 2000, 0, 4, 0, SEED, **kw)
    one.finish(solver, 4, adapt=True)
    p = two.get_packed()
    two.set_packed(p)
    two.train()
    nstat, nbin = one.merge_shape()["nstat"], one.merge_shape()["nbin"]
    for leaf, lf in enumerate(one.config.leaves):
        if hasattr(lf, "ninc"):
            assert same_bits(one.grid(leaf), two.grid(leaf)), leaf
            assert not np.array_equal(one.grid(leaf), np.linspace(lf.lower, lf.upper, lf.ninc))
        else:
            assert leaf_bits(one.distribution(leaf)) == leaf_bits(two.distribution(leaf)), leaf
    for eng in (one, two):
        assert same_bits(eng.get_packed()[nstat:nstat + nbin], np.full(nbin, 1.0e-10))
        eng.check_status()
        eng.close()
