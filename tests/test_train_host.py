"""CPU tests of train!'s test harness (tests/train_cases.py): the CPU oracle (mcio_train_continuous, mcio_train_discrete,
mcio_do_reweight) against the independent long-double reference over the whole case table -- which proves that the derived bounds can be
met without the kernel --, three deliberate mistakes planted into a float64 replay that the bounds must reject -- which proves that they
have teeth --, the table's coverage and its own conditions (the reference's unguarded walk stays inside its bins on every case; strictly
increasing results where claimed), and the refusals that need no device."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import train_cases as T


def engine(problem, **kw):
    """the engine of a problem of train_cases.problems() (tests/test_hip_train.py builds the same ones on a device)"""
    var = tuple(mci.Continuous(T.LOWER, T.UPPER, ninc=n + 1, alpha=a, adapt=ad) if k == "c" else mci.Discrete(1, n, alpha=a, adapt=ad)
                for k, n, a, ad in T.problems()[problem])
    return mci.Engine(mci.Configuration(var=var, dof=[[1] * len(var)]), mci.catalog.one(), **kw)


def reweight_engine(**kw):
    """the chain-solver problem of the reweighting cases: merge_cases' sphere2 (nd = 3)"""
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2(), **kw)


ONE = np.nextafter(1.0, 2.0)
# visited counts (nd = 3): 0, 1, 1 + ulp take the `<= 1` branch or just miss it; large; all equal
VISITED = {"zero": (0.0, 5.0, 7.0), "one": (1.0, 3.0, 4.0), "one_plus_ulp": (ONE, ONE, 2.5), "large": (3.0e15, 1.0e8, 7.0e11),
           "equal": (123.0, 123.0, 123.0), "mixed": (0.5, 1.0e-8, 4.0e6)}
GAMMAS = (1.0, 0.5, 2.0)
GOALS = (None, (1.0, 2.0, 5.0))
START = (0.2, 0.5, 0.3)

# adapted-grid cases on which the CPU oracle itself leaves two equal neighbours: none on this table (the adapted grids keep every width
# twenty bits above an ulp of its position); tests/test_hip_train.py would assert non-decreasing only on a case named here
NOT_STRICT = set()

FAMILY_CASES = {}
for _c in T.cases():
    FAMILY_CASES.setdefault(_c["family"] if _c["kind"] != "m" else "mixed", []).append(_c)


def oracle_leaf(oracle, leaf):
    kind, n, alpha, adapt, g, h = leaf
    return oracle.train_continuous(g, h, alpha) if kind == "c" else oracle.train_discrete(h, alpha)


@pytest.mark.parametrize("family", sorted(FAMILY_CASES))
def test_the_oracle_lies_within_the_derived_bounds_of_the_reference(oracle, family):
    worst, wrange, at = 0.0, 0.0, None
    for c in FAMILY_CASES[family]:
        for l, leaf in enumerate(T.leaf_inputs(c)):
            if not leaf[3]:
                continue
            w, r = T.check_leaf(leaf, oracle_leaf(oracle, leaf), "oracle, case %s leaf %d" % (c["id"], l))
            wrange = max(wrange, r)
            if w > worst:
                worst, at = w, c["id"]
    print("%-12s %3d cases, oracle: largest difference / derived bound %.4f (%s), largest difference / range %.3g"
          % (family, len(FAMILY_CASES[family]), worst, at, wrange))
    assert worst <= 1.0


def test_the_oracles_reweighting_lies_within_its_bounds():
    import mci_oracle
    worst = 0.0
    for name, vis in VISITED.items():
        for gamma in GAMMAS:
            for goal in GOALS:
                r0 = np.array(START) / np.sum(START)
                ref, bound = T.ref_reweight(r0, vis, gamma, goal)
                got = mci_oracle.do_reweight(r0, vis, gamma, goal)
                worst = max(worst, T.ratio(got, ref, bound, "oracle reweight %s gamma %g" % (name, gamma)))
                assert abs(float(ref.sum()) - 1.0) < 1e-18
    print("doReweight!: oracle, largest difference / derived bound %.4f" % worst)
    assert worst <= 1.0


def named(mutation):
    """cases on which the planted mistake changes the outcome"""
    if mutation == "acc_shift":
        return [c for c in T.cases() if c["kind"] == "d" and c["n"] in (2, 3, 17, 1025) and c["family"] in ("ones", "ramp", "lognormal", "spike")]
    fams = ("flat", "ones", "ramp", "lognormal", "comb")    # (not N = 2: on a symmetric histogram both of its bins are end bins and change alike)
    return [c for c in T.cases() if c["kind"] == "c" and c["n"] in (3, 17, 257, 999) and c["alpha"] == 2.0 and c["family"] in fams]


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_the_bounds_reject_a_replay_with_a_planted_mistake(mutation):
    cs = named(mutation)
    assert len(cs) >= 16
    for c in cs:
        (leaf,) = T.leaf_inputs(c)
        kind, n, alpha, adapt, g, h = leaf
        good = T.replay_continuous(g, h, alpha) if kind == "c" else T.replay_discrete(h, alpha)
        assert T.check_leaf(leaf, good, "replay " + c["id"])[0] <= 1.0
        bad = T.replay_continuous(g, h, alpha, mutate=mutation) if kind == "c" else T.replay_discrete(h, alpha, mutate=mutation)
        assert T.check_leaf(leaf, bad, "mutated replay " + c["id"])[0] > 1.0, (mutation, c["id"])


def discrete_with_sum(h, s, alpha):
    """train!(Discrete) in float64 with sum(h) given"""
    v = h / s
    m = (v > 0) & (v <= T.THRESHOLD)
    d = v.copy()
    d[m] = (-(1.0 - v[m]) / np.log(v[m])) ** alpha
    return d / np.cumsum(d)[-1]


def test_one_histogram_tells_julias_split_of_a_long_sum_from_another(oracle):
    """train_cases.assoc_hist: the oracle's sum (Julia's halves of 513 | 512) and the halves the other way round differ by sixteen ulps,
    and distribution[512] follows by more than 24 units of 2^-53 of its size -- twice the twelve tests/test_hip_train.py allows the
    kernel against the oracle there"""
    h = T.assoc_hist()
    julia, other = T.sum_julia64(h), T.sum_julia64(h, split=lambda n: n >> 1)
    assert julia == oracle.sum_julia(h) == 2.0 ** 60 + 258048 and other == 2.0 ** 60 + 253952
    dist, acc = oracle.train_discrete(h, T.ASSOC_ALPHA)
    a, b = discrete_with_sum(h, julia, T.ASSOC_ALPHA)[T.ASSOC_BIN], discrete_with_sum(h, other, T.ASSOC_ALPHA)[T.ASSOC_BIN]
    unit = 2.0 ** -53 * dist[T.ASSOC_BIN]
    print("distribution[512]: replay - oracle = %.3g, other split - oracle = %.3g units" % ((a - dist[T.ASSOC_BIN]) / unit, (b - dist[T.ASSOC_BIN]) / unit))
    assert abs(a - dist[T.ASSOC_BIN]) <= 4 * unit and abs(b - dist[T.ASSOC_BIN]) >= 24 * unit and 0.03 < a < 0.04
    leaf = ("d", T.ASSOC_K, T.ASSOC_ALPHA, True, None, h)
    assert T.check_leaf(leaf, (dist, acc), "oracle, assoc")[0] <= 1.0


def test_the_table_covers_what_it_is_for():
    cs = T.cases()
    print(len(cs), "cases, N_fit", T.N_FIT)
    assert 900 <= len(cs) <= 1200
    assert T.has_spare(T.N_FIT) and not T.has_spare(T.N_FIT + 1) and 2700 < T.N_FIT < 2800
    assert (T.lds_doubles(T.MAX_LEAF_BINS) + T.MAX_LEAF_BINS) * 8 <= T.TRAIN_LDS_MAX       # the largest leaf's launch fits without the slots
    cont = [c for c in cs if c["kind"] == "c"]
    want = {1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 511, 512, 513, 999, 1023, 1024, 1025, 2047, 2048, 2049, T.N_FIT, T.N_FIT + 1,
            4399, 4400}
    for fam in T.FAMILIES:
        for gk in T.GRIDS:
            assert {c["n"] for c in cont if c["alpha"] == 2.0 and c["family"] == fam and c["grid"] == gk} == want, (fam, gk)
        for alpha in T.SIDE_ALPHAS:
            assert {c["n"] for c in cont if c["alpha"] == alpha and c["family"] == fam} == set(T.SIDE_SIZES), (fam, alpha)
        for alpha in T.DISCRETE_ALPHAS:
            assert {c["n"] for c in cs if c["kind"] == "d" and c["alpha"] == alpha and c["family"] == fam} == set(T.DISCRETE_K), (fam, alpha)
        for alpha in T.DISCRETE_SIDE_ALPHAS:
            assert {c["n"] for c in cs if c["kind"] == "d" and c["alpha"] == alpha and c["family"] == fam} == set(T.DISCRETE_SIDE_K), (fam, alpha)
    assert set(T.SIDE_ALPHAS) == {1.0, 3.0, 1.5, 0.5} and set(T.DISCRETE_SIDE_ALPHAS) == {1.0, 3.0}
    for alpha in T.SIDE_ALPHAS:
        assert {c["grid"] for c in cont if c["alpha"] == alpha} == set(T.GRIDS)
    mixed = [c for c in cs if c["kind"] == "m"]
    for l in range(len(T.MIXED)):
        assert {c["families"][l] for c in mixed} == set(T.FAMILIES)
    kinds = [(k, n, ad) for k, n, a, ad in T.MIXED]
    assert ("c", 1200, True) in kinds and ("c", 41, True) in kinds and ("c", 17, False) in kinds and ("d", 4, True) in kinds and ("d", 3, False) in kinds
    assert T.train_threads(max(n for k, n, a, ad in T.MIXED)) == 512
    # the histogram families are what they say, seeded, and a pure function of (N, family)
    for n in (1, 2, 17, 999):
        for fam in T.FAMILIES:
            h = T.hist(n, fam)
            assert h.shape == (n,) and np.all(np.isfinite(h)) and np.all(h > 0) and h.tobytes() == T.hist(n, fam).tobytes()
        assert T.hist(n, "pow2").tobytes() == (T.hist(n, "lognormal") * 2.0 ** 40).tobytes()
    h = T.hist(999, "spike")
    assert h[333] == 1.0e6 and np.count_nonzero(h == 1.0e-10) == 998 and T.hist(999, "spike_first")[0] == 1.0e6 and T.hist(999, "spike_last")[-1] == 1.0e6
    # the adapted grid: strictly increasing (what mci_set_grid checks), widths over several decades, none near an ulp of its position
    for n in sorted(want):
        g = T.grid(n, "adapted")
        w = np.diff(g)
        assert g[0] == T.LOWER and g[-1] == T.UPPER and np.all(w > 0) and w.min() > 2.0 ** 20 * np.spacing(4.0)
        assert n < 999 or 1.0e4 < w.max() / w.min() < 1.0e8, (n, w.max() / w.min())
    places = T.bad_places(T.BAD_N)
    assert places == dict(first=0, middle=499, last=998, second_wave=639) and len(T.BAD_VALUES) == 5


def test_no_rescaled_bin_sits_on_the_rescale_threshold():
    """rescale is discontinuous at v = 0.99999999 (by ~1e-8 alpha): the bounds assume no bin of the table is within rounding of it"""
    for c in T.cases():
        for kind, n, alpha, adapt, g, h in T.leaf_inputs(c):
            if n == 1:
                continue
            hl = np.asarray(h).astype(T.LD)
            d = hl.copy()
            if kind == "c":
                d[0], d[-1] = (7 * hl[0] + hl[1]) / 8, (7 * hl[-1] + hl[-2]) / 8
                d[1:-1] = (hl[:-2] + 6 * hl[1:-1] + hl[2:]) / 8
            v = d / d.sum()
            assert np.all(np.abs(v - T.LD(T.THRESHOLD)) > 1.0e-12), c["id"]


def test_a_rescale_that_goes_non_finite_needs_a_bad_bin():
    """the status path "distribution is not all finite" cannot be reached with finite positive bins: v = d / sum(d) lies in (0, 1], -log v
    is finite and positive for every positive double below 1, (1 - v) / (-log v) lies in (0, 1) and so does any positive power of it;
    at worst it underflows to 0, which is finite.  Shown here on the smallest and largest ratios float64 has."""
    for alpha in (0.5, 1.0, 1.5, 2.0, 3.0):
        v = np.array([5e-324, 1e-308, 1e-300, 1e-16, 0.5, np.nextafter(T.THRESHOLD, 0.0), T.THRESHOLD])
        r = (-(1.0 - v) / np.log(v)) ** alpha
        assert np.all(np.isfinite(r)) and np.all(r >= 0) and np.all(r < 1)


def test_the_reference_walk_stays_inside_its_bins_on_every_case(oracle):
    """mcio_train_continuous' `while (acc_f < f_ninc) { j += 1; acc_f += d[j-1]; }` (variable.jl:228-231) has no guard of its own: Julia
    would throw a BoundsError where rounding lets acc_f fall short at the very end.  Replayed in float64 on the oracle's own d and
    f_ninc: j <= N on every Continuous leaf of the table (a condition on the TABLE; the oracle now returns 5 instead of reading past d)"""
    n = 0
    for c in T.cases():
        for kind, nb, alpha, adapt, g, h in T.leaf_inputs(c):
            if kind != "c" or not adapt:
                continue
            d = oracle.rescale(oracle.smooth(h), alpha) if nb > 1 else np.array(h)
            j = T.walk_stays_inside(d, oracle.sum_julia(d) / nb)
            assert j <= nb, (c["id"], j, nb)
            n += 1
    assert n >= 800
    # the replay does tell: bins that fall short of (N - 1) f_ninc send j past N
    assert T.walk_stays_inside(np.array([1.0, 1.0, 0.0]), 1.0) == 2 and T.walk_stays_inside(np.array([1.0, 0.5, 0.25]), 1.0) == 4


def test_the_oracle_keeps_the_grid_strictly_increasing_on_uniform_grids(oracle):
    """... and non-decreasing everywhere; the cases where the oracle itself merges two neighbours on an adapted grid are named"""
    ties = []
    for c in T.cases():
        for l, (kind, nb, alpha, adapt, g, h) in enumerate(T.leaf_inputs(c)):
            if kind != "c" or not adapt:
                continue
            w = np.diff(oracle.train_continuous(g, h, alpha))
            assert np.all(w >= 0), c["id"]
            if c["grid"] == "uniform":
                assert np.all(w > 0), c["id"]
            elif not np.all(w > 0):
                ties.append(c["id"])
    print("adapted-grid cases on which the oracle leaves equal neighbours:", ties)
    assert set(ties) <= NOT_STRICT


def test_non_adapting_leaves_keep_everything_in_the_oracle(oracle):
    """variable.jl:208 / :370 return before clearStatistics!: mcio_train leaves grid, distribution AND histogram of an adapt=false leaf"""
    c = next(c for c in T.cases() if c["kind"] == "m")
    leaves = T.leaf_inputs(c)
    ol = [dict(kind=0 if k == "c" else 1, pool=i, lower=T.LOWER if k == "c" else 1, upper=T.UPPER if k == "c" else n, npts=n + 1, alpha=a, adapt=ad,
               grid=g) for i, (k, n, a, ad, g, h) in enumerate(leaves)]
    ocfg = oracle.Config(ol, [[1] * len(ol)])
    before = []
    for i, (k, n, a, ad, g, h) in enumerate(leaves):
        np.ctypeslib.as_array(ocfg.leaf(i).hist, shape=(n,))[:] = h
        before.append(ocfg.grid(i) if k == "c" else (ocfg.distribution(i), ocfg.accumulation(i)))
    ocfg.train()
    for i, (k, n, a, ad, g, h) in enumerate(leaves):
        if ad:
            assert ocfg.hist(i).tobytes() == np.full(n, 1.0e-10).tobytes()
            got = ocfg.grid(i) if k == "c" else (ocfg.distribution(i), ocfg.accumulation(i))
            assert T.check_leaf(leaves[i], got, "mcio_train leaf %d" % i)[0] <= 1.0
        else:
            assert ocfg.hist(i).tobytes() == h.tobytes()
            if k == "c":
                assert ocfg.grid(i).tobytes() == before[i].tobytes() == g.tobytes()
            else:
                assert ocfg.distribution(i).tobytes() == before[i][0].tobytes() and ocfg.accumulation(i).tobytes() == before[i][1].tobytes()


def test_the_hooks_train_step_refuses_bad_arguments_without_a_device():
    """Engine.merge_rows(train=...) / mci_debug_merge's do_train: path "finish" only, a known walk, one table per leaf of the right size"""
    eng = engine("mixed", device=-1)
    sh = eng.merge_shape()
    leaves = T.leaf_inputs(next(c for c in T.cases() if c["kind"] == "m"))
    grids = [lf[4] for lf in leaves if lf[0] == "c"]
    tables = [(np.full(lf[1], 1.0 / lf[1]), np.linspace(0.0, 1.0, lf[1] + 1)) for lf in leaves if lf[0] == "d"]
    good = dict(nblocks=1, wg_per_block=1, part_cols=np.ones((1, sh["ncols"])), part_hist=np.ones((2, sh["nbin"])), path="finish", train="serial",
                grids=grids, tables=tables)
    for bad in (dict(path="finalize"), dict(train="fast"), dict(grids=grids[:-1]), dict(grids=[g[:-1] for g in grids]), dict(tables=tables[:1]),
                dict(tables=[(d, a[:-1]) for d, a in tables]), dict(grids=None)):
        with pytest.raises(ValueError):
            eng.merge_rows(**dict(good, **bad))
    for walk in ("scan", "serial", "serial_general", "serial_wrong_decision"):
        with pytest.raises(mci.MCIError, match="offline"):              # good arguments get as far as the device
            eng.merge_rows(**dict(good, train=walk))
    # the C side's own refusals
    import ctypes as C
    from mcintegration_jl_amd import _lib
    pc, ph, packed = np.ones((1, sh["ncols"])), np.ones((2, sh["nbin"])), np.zeros(eng.reduce_size)
    g, d, a = np.concatenate(grids), np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])
    dp = lambda v: v.ctypes.data_as(_lib.c_double_p)

    def io(**kw):
        s = _lib.DebugMergeIO(1, 1, 1, 2, 0, 0, 1, dp(pc), dp(ph))
        s.packed, s.do_train, s.train_walk = dp(packed), 1, 1
        s.grids, s.dists, s.accs, s.grids_out, s.dists_out, s.accs_out = dp(g), dp(d), dp(a), dp(g.copy()), dp(d.copy()), dp(a.copy())
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    for kw, match in ((dict(path=0), "do_train needs path 1"), (dict(train_walk=4), "train walk 4"), (dict(train_walk=-1), "train walk -1"),
                      (dict(grids=None), "without its tables"), (dict(accs_out=None), "without its tables"), (dict(), "offline")):
        with pytest.raises(mci.MCIError, match=match):
            _lib.check(_lib.lib().mci_debug_merge(eng.p, C.byref(io(**kw))))


def test_refusals_that_need_no_device():
    eng = engine(T.problem_name("c", 17, 2.0), device=-1)
    with pytest.raises(mci.MCIError, match="offline"):
        eng.train()
    with pytest.raises(mci.MCIError, match="offline"):                    # (mci_set_packed looks at the context before the length: the
        eng.set_packed(np.zeros(eng.packed_size + 1))                     # wrong lengths are refused in tests/test_hip_train.py)
    g = T.grid(17, "adapted").copy()
    eng.set_grid(0, g)                                                    # the adapted grid passes mci_set_grid's check
    assert eng.grid(0).tobytes() == g.tobytes()
    for bad in (g[::-1], np.concatenate([g[:5], g[4:-1]]), np.where(np.arange(18) == 9, np.nan, g)):
        with pytest.raises(mci.MCIError, match="strictly increasing"):
            eng.set_grid(0, bad)
    with pytest.raises(mci.MCIError, match="18 points"):
        eng.set_grid(0, g[:-1])
    assert eng.grid(0).tobytes() == g.tobytes()                           # a refused grid changes nothing
