"""GPU tests of stratified (VEGAS+) points in :vegas parameter sweeps (mci_integrate_sweep_strat; csrc/mci_sweep_strat.h
vegas_sweep_strat): P independent stratified loops, one workgroup per point, in ONE launch -- against the oracle's plain VEGAS+ iteration
(oracle/mci_oracle.c mcio_strat_alloc / mcio_strat_iteration) on identical Philox streams, against the ordinary stratified call, and
against themselves under another assignment of points to workgroups.

`chain` runs a sweep of niter = 1 again and again, feeding `maps` and `alloc` (d) back, teacher-forced as tests/test_hip_stratified_parity.py
drives the ordinary path: before each iteration the oracle takes the engine's grids and the counts the sweep reports.  Per point and
iteration (the bounds are that module's, which derives them):

    allocation (counts_out)          mcio_strat_alloc of the ORACLE's d_h (uniform first)    check_alloc: sum = N, min >= 2, |delta n_h| <= 1 on at
                                                                                             most max(2, ncube / 1000) hypercubes
    mean per column                  oracle (long double)                                    1e-11 * sum_h V / n_h sum |f J|
    sum_k s^2 = d_out^(2 / beta)     oracle two-pass                                         sum_k 4 (n_h + 2) 2^-53 S2 / (n_h - 1) + rel 1e-12
    variance per column              oracle                                                  sum_h V^2 / n_h * that bound + rel 1e-11
    map after train!                 oracle's train! of its histogram + (m + 1) 1e-10        abs 1e-12 * range, ends equal, increasing

One launch of several iterations differs from the chain only in what the prefix-scan walk and the order of sums leave: 1e-11 / 1e-8 on
an iteration that follows no train!, 1e-4 / 1e-2 (maps 1e-4 * range) over a run, the tolerances of tests/test_hip_sweep.py."""
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_stratified import GAUSS4, LOGSQRT, WATSON, _c1_cfg, _gauss4_cfg, watson_cfg
from test_hip_stratified_parity import COMPLEX_BODY, PEAK2, SEED, U, check_alloc, ocont

pytestmark = pytest.mark.gpu

X2Y2P = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
SPHERE2P = ("w[0] = (x[0] * x[0] + x[1] * x[1] < ud[0]) ? 1.0 : 0.0; "
            "w[1] = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] < ud[0]) ? 1.0 : 0.0;")
COMPLEXP = COMPLEX_BODY + " w[0] *= ud[0]; w[3] += ud[0];"
PEAK2P = PEAK2 + " w[0] *= ud[0];"
LAYOUTS = {
    "x2y2": dict(dof=[[2]], f=X2Y2P),
    "sphere2": dict(dof=[[2], [3]], f=SPHERE2P),
    "complex": dict(dof=[[1], [1]], f=COMPLEXP, complex=True),
    "peak2": dict(dof=[[2]], f=PEAK2P),
}


def make(oracle, name, ud0):
    L = LAYOUTS[name]
    cx = L.get("complex", False)
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=L["dof"], seed=SEED, **(dict(type=complex) if cx else {}))
    eng = mci.Engine(cfg, mci.Integrand(L["f"], [ud0]))
    ocfg = oracle.Config([ocont()], L["dof"], obs_nbin=[2] * len(L["dof"]) if cx else None)
    if cx:
        ocfg.set_ncomp(2)
    return cfg, eng, ocfg, oracle.compile_c_integrand(L["f"])


def merged_blocks(eng, N, block):
    """blocks the ordinary stratified call merges its rows as (chunks of the largest of 8 | 4 | 2 | 1 trips of 256
    samples whose LDS -- the sample tables plus (nloc + 1) + 2 NW nloc + 256 + 512 NW doubles, nloc = S / 2 + 1 -- fits 64 KiB, else
    159 KiB; one workgroup per chunk up to 2048; the call's blocks when there are that many workgroups, else one)"""
    NW = eng.nobs
    S = None
    for lim in (64 * 1024, 159 * 1024):
        for k in (8, 4, 2, 1):
            nloc = k * 128 + 1
            if S is None and eng.lds_bytes + 8 * ((nloc + 1) + 2 * NW * nloc + 256 + 512 * NW) <= lim:
                S = 256 * k
    nwg = min(-(-N // S), 2048)
    return block if nwg >= block else 1


def check_point(oracle, ocfg, of, ud, r, grid_in, want, nstrat, N, k, seed, beta, m_blocks, tag):
    """one point's one iteration against the oracle on the engine's grid and counts; returns the oracle's d_h and its trained grid"""
    nc = int(np.prod(nstrat))
    V = 1.0 / nc
    assert r["status"] == 0 and r["neval"] == N, tag
    counts = r["strat_counts"]
    check_alloc(counts, want, N, tag)
    off = np.concatenate([[0], np.cumsum(counts)])
    ocfg.set_grid(0, grid_in)
    o = ocfg.strat_iteration(of, ud, seed, k, 0, nstrat, off, beta)
    n = counts.astype(np.float64)
    m, e = r["iter_mean"][0], r["iter_std"][0]
    tol_mean = 1e-11 * (V / n[:, None] * o["A1"]).sum(axis=0)
    print(tag, "mean", m, "ref", o["mean"], "tol", tol_mean)
    assert np.all(np.abs(m - o["mean"]) <= tol_mean), (tag, m, o["mean"], tol_mean)
    bound_hq = 4.0 * (n[:, None] + 2.0) * U * o["S2"] / (n[:, None] - 1.0)
    v2_ref = o["v2"].sum(axis=1)
    v2_gpu = (r["strat_d"].astype(np.longdouble) ** (np.longdouble(2.0) / np.longdouble(beta))).astype(np.float64)
    bound = bound_hq.sum(axis=1)
    err = np.abs(v2_gpu - v2_ref)
    bad = np.flatnonzero(~(err <= bound + 1e-12 * np.maximum(v2_ref, v2_gpu)))
    with np.errstate(divide="ignore", invalid="ignore"):
        print(tag, "max |v2_gpu - v2_ref| / bound = %.3g" % np.where(bound > 0, err / bound, 0.0).max())
    assert bad.size == 0, (tag, "first hypercube", bad[:1], counts[bad[:1]], v2_gpu[bad[:1]], v2_ref[bad[:1]], bound[bad[:1]], bad.size)
    tol_var = (V * V / n[:, None] * bound_hq).sum(axis=0) + 1e-11 * o["var"]
    print(tag, "var", e * e, "ref", o["var"], "tol", tol_var)
    assert np.all(np.abs(e * e - o["var"]) <= tol_var), (tag, e * e, o["var"], tol_var)
    ocfg.add_hist(0, m_blocks * 1e-10)
    ocfg.train()
    g, og = r["maps"], ocfg.grid(0)
    assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0), tag
    np.testing.assert_allclose(g, og, rtol=0, atol=1e-12, err_msg=tag)
    return o["d"].copy(), (o["mean"].copy(), np.sqrt(o["var"]))


def chain(oracle, name, nstrat, N, block, uds, niter=3, grid=2, beta=0.75, seed=SEED):
    """niter sweeps of one iteration each over the points `uds` on `grid` workgroups, maps and d fed back; everything of the module's
    table asserted per point and iteration.  Returns (engine, [per iteration: list of result dicts], [per iteration: oracle rows])"""
    cfg, eng, ocfg, of = make(oracle, name, uds[0])
    eng.set_stratification(nstrat=nstrat, beta=beta)
    eng.sweep_workgroups(grid)
    P, nc = len(uds), int(np.prod(nstrat))
    m_blocks = merged_blocks(eng, N, block)
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(nc), N, True))
    maps, d, want = None, None, [uniform] * P
    runs, rows = [], []
    for k in range(niter):
        start = [eng.grid(0)] * P if maps is None else maps
        rs = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds], neval=N, niter=1, block=block, seed=seed, ignore=0, maps=maps, d=d,
                                       first_iteration=k)
        assert eng.last_sweep_launch()[0] == min(grid, P)
        nxt, row = [], []
        for p in range(P):
            dref, mo = check_point(oracle, ocfg, of, [uds[p]], rs[p], start[p], want[p], nstrat, N, k, seed, beta, m_blocks,
                                   "%s %s N=%d point %d iteration %d" % (name, nstrat, N, p, k))
            nxt.append(np.diff(oracle.Config.strat_alloc(dref, N)))
            row.append(mo)
        want = nxt
        maps, d = np.array([r["maps"] for r in rs]), np.array([r["strat_d"] for r in rs])
        runs.append(rs)
        rows.append(row)
    return eng, runs, rows


def test_first_iteration_three_points_on_two_workgroups(oracle):
    eng, runs, _ = chain(oracle, "x2y2", [16, 16], 4096, 4, [1.0, 0.25, -2.0], niter=1)
    m = [r["iter_mean"][0, 0] for r in runs[0]]
    assert abs(m[0] - m[1]) > 0.1 and abs(m[0] - m[2]) > 0.1      # (the points ARE different integrals)
    eng.close()


@pytest.mark.parametrize("name,N,block,nstrat", [("sphere2", 30, 1, [5, 1, 3]), ("sphere2", 2048, 16, [5, 1, 3]), ("sphere2", 8193, 3, [5, 1, 3]),
                                                 ("sphere2", 4096, 2, [16, 1, 128]), ("peak2", 6000, 4, [3, 2]), ("complex", 4096, 4, [37])],
                         ids=["two_each_tiny", "more_blocks_than_chunks", "odd", "two_each_2048_cubes", "peak2_long_and_cut", "complex"])
def test_teacher_forced_chain(oracle, name, N, block, nstrat):
    """sphere2: a padding probability with two columns, at the sizes of the parity file; peak2 on six hypercubes of 6000 samples: the
    uniform hypercubes of 1000 samples are cut at the ends of chunks of 256 .. 2048 samples (no multiple of 1000 is one of 256), and once
    the samples have moved to the peak one hypercube is longer than the largest chunk; complex: four columns"""
    uds = [1.0, 0.6] if name != "complex" else [1.0, -0.5]
    eng, runs, _ = chain(oracle, name, nstrat, N, block, uds)
    counts = [r["strat_counts"] for rs in runs for r in rs]
    if N == 2 * int(np.prod(nstrat)):
        assert all(np.all(c == 2) for c in counts)      # exactly two samples per hypercube: nothing moves
    elif name == "peak2":
        assert max(c.max() for c in counts) > 2048 and np.abs(counts[-1] - counts[0]).max() > 1
    eng.close()


def _kw(N, block, niter, **more):
    return dict(neval=N, niter=niter, block=block, seed=SEED, **more)


def test_one_launch_against_the_chain(oracle):
    N, block, nstrat, uds = 8192, 4, [5, 1, 3], [1.0, 0.6, 0.8]
    eng, runs, rows = chain(oracle, "sphere2", nstrat, N, block, uds, niter=3)
    for niter, (rm, rs, ra) in ((2, (1e-11, 1e-8, None)), (3, (1e-4, 1e-2, 1e-4))):
        out = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds], **_kw(N, block, niter))
        for p, r in enumerate(out):
            # iteration 0 follows no train!: the chain's iteration 0 at the single-iteration tolerances
            np.testing.assert_allclose(r["iter_mean"][0], rows[0][p][0], rtol=1e-11, atol=1e-300)
            np.testing.assert_allclose(r["iter_std"][0], rows[0][p][1], rtol=1e-8, atol=1e-300)
            if niter == 2:   # the last allocation: made from iteration 0's d_h, which the chain's second sweep was given
                check_alloc(r["strat_counts"], runs[1][p]["strat_counts"], N, "niter 2 point %d" % p)
            else:
                for k in range(3):
                    np.testing.assert_allclose(r["iter_mean"][k], rows[k][p][0], rtol=rm, atol=1e-300)
                    np.testing.assert_allclose(r["iter_std"][k], rows[k][p][1], rtol=rs, atol=1e-300)
                g, og = r["maps"], runs[2][p]["maps"]
                assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0)
                np.testing.assert_allclose(g, og, rtol=0, atol=ra)
            assert r["neval"] == niter * N and r["status"] == 0
    eng.close()


def test_one_point_against_the_ordinary_call():
    N, block, niter, nstrat = 16384, 4, 3, [5, 1, 3]
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(SPHERE2P, [0.9]))
    eng.set_stratification(nstrat=nstrat)
    g0 = eng.grid(0).copy()
    r = eng.integrate_sweep_strat("vegas", userdata=[[0.9]], **_kw(N, block, niter))[0]
    assert eng.grid(0).tobytes() == g0.tobytes()      # the engine's own map: untouched
    res = mci.integrate(mci.Integrand(SPHERE2P, [0.9]), var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], solver="vegas", neval=N, niter=niter,
                        block=block, seed=SEED, stratify=mci.Stratify(nstrat=nstrat))
    np.testing.assert_allclose(r["iter_mean"][0], res.iter_mean[0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"][0], res.iter_std[0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["iter_mean"], res.iter_mean, rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], res.iter_std, rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], res.mean, rtol=1e-4)
    np.testing.assert_allclose(r["stdev"], res.stdev, rtol=1e-2)
    g = res.config._engine.grid(0)
    np.testing.assert_allclose(r["maps"], g, rtol=0, atol=1e-4)
    check_alloc(r["strat_counts"], res.config._engine.strat_counts(), N, "last allocation")
    eng.close()


def _sphere_engine(nstrat=(5, 1, 3)):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(SPHERE2P, [1.0]))
    eng.set_stratification(nstrat=list(nstrat))
    return eng


def _agree(a, b):
    np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(a["iter_std"][0], b["iter_std"][0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(a["iter_std"], b["iter_std"], rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(a["maps"], b["maps"], rtol=0, atol=1e-4)


def test_nothing_leaks_between_points():
    """five points on two workgroups in two orders, an all-NaN point between: its status is set, the others do not see it"""
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED), mci.Integrand(X2Y2P, [1.0]))
    eng.set_stratification(nstrat=[4, 4])
    eng.sweep_workgroups(2)
    uds = [1.0, 0.6, float("nan"), 0.8, 0.4]
    kw = _kw(8192, 4, 3)
    a = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds], **kw)
    order = [4, 2, 0, 3, 1]
    b = eng.integrate_sweep_strat("vegas", userdata=[[uds[i]] for i in order], **kw)
    eng.sweep_workgroups(0)
    alone = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds if u == u], **kw)
    assert a[2]["status"] != 0 and b[1]["status"] != 0
    assert a[2]["maps"].tobytes() == eng.grid(0).tobytes()      # train! refused: the map stayed
    good = [i for i in range(5) if i != 2]
    for j, i in enumerate(good):
        assert a[i]["status"] == 0 and np.all(np.isfinite(a[i]["iter_mean"])) and np.all(np.isfinite(a[i]["maps"]))
        _agree(a[i], b[order.index(i)])
        _agree(a[i], alone[j])
        assert a[i]["strat_counts"].sum() == 8192 and a[i]["strat_counts"].min() >= 2
    eng.close()


def test_frozen_allocation_and_maps(oracle):
    N, block, nstrat = 8192, 4, [5, 1, 3]
    uds = [[1.0], [0.6], [0.8]]
    eng = _sphere_engine(nstrat)
    trained = eng.integrate_sweep_strat("vegas", userdata=uds, **_kw(N, block, 3))
    d = np.array([r["strat_d"] for r in trained])
    maps = np.array([r["maps"] for r in trained])
    frozen = eng.integrate_sweep_strat("vegas", userdata=uds, adapt=False, d=d, maps=maps, **_kw(N, block, 3))
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(15), N, True))
    for p, r in enumerate(frozen):
        check_alloc(r["strat_counts"], np.diff(oracle.Config.strat_alloc(d[p], N)), N, "frozen point %d" % p)
        assert np.abs(r["strat_counts"] - uniform).max() > 1
        assert r["maps"].tobytes() == maps[p].tobytes()
        assert r["strat_d"].max() > 0 and not np.array_equal(r["strat_d"], d[p])      # (d_out is what the last iteration measured)
    plain = eng.integrate_sweep_strat("vegas", userdata=uds, adapt=False, **_kw(N, block, 3))
    for r in plain:
        assert np.array_equal(r["strat_counts"], uniform) and r["maps"].tobytes() == eng.grid(0).tobytes()
    eng.close()
    # through the public call: train, then freeze over the whole scan
    def kw():      # (a Configuration is built from these per call)
        return dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED, solver="vegas", neval=N, block=block, niter=3,
                    stratify=mci.Stratify(nstrat=nstrat))
    f = mci.Integrand(SPHERE2P, [1.0])
    tr = mci.integrate_sweep(f, uds, **kw())
    fz = mci.integrate_sweep(f, uds, adapt=False, alloc=[r.strat_d for r in tr], maps=[r.map for r in tr], **kw())
    for a, b in zip(tr, fz):
        assert a.stratification["carried"] == "uniform" and b.stratification["carried"] == "same plan" and b.sweep_batched
        assert b.map.tobytes() == a.map.tobytes() and b.stratification["nstrat"] == nstrat and b.stratification["ncube"] == 15
        check_alloc(b.strat_counts, np.diff(oracle.Config.strat_alloc(np.asarray(a.strat_d), N)), N, "alloc=")


def test_ragged_points_and_seeds():
    """P = 7 on 3 workgroups against 7 workgroups; per-point seeds against one-point sweeps under those seeds"""
    eng = _sphere_engine()
    uds = [[0.3 + 0.1 * k] for k in range(7)]
    seeds = [SEED + 11 * k for k in range(7)]
    kw = dict(neval=4096, niter=2, block=4)
    eng.sweep_workgroups(3)
    a = eng.integrate_sweep_strat("vegas", userdata=uds, seeds=seeds, **kw)
    assert eng.last_sweep_launch() == (3, 256)
    eng.sweep_workgroups(0)
    b = eng.integrate_sweep_strat("vegas", userdata=uds, seeds=seeds, **kw)
    assert eng.last_sweep_launch()[0] == 7
    for k in range(7):      # (the LDS histogram adds of a workgroup are not ordered: the maps, and what follows them, agree to the run tolerances)
        _agree(a[k], b[k])
        check_alloc(a[k]["strat_counts"], b[k]["strat_counts"], 4096, "point %d" % k)
    for k in (0, 6):
        _agree(eng.integrate_sweep_strat("vegas", userdata=[uds[k]], seed=seeds[k], **kw)[0], a[k])
    assert a[0]["iter_mean"][0, 0] != a[1]["iter_mean"][0, 0]
    eng.close()


def test_stratified_sweep_errors_are_honest_and_smaller():
    """the integrands and thresholds of test_hip_stratified.test_stratified_errors_are_honest_and_smaller, the 32 seeds as 32 points of
    ONE stratified sweep; the scatter is also below that of the classic sweep of the same points"""
    seeds = list(range(1, 33))
    ratios = {}
    for name, f, mk, neval in (("benchmark1", WATSON, watson_cfg, 2e5), ("benchmark4", GAUSS4, _gauss4_cfg, 1e5), ("c1", LOGSQRT, _c1_cfg, 1e5)):
        ud = np.zeros((32, 0))
        eng = mci.Engine(mk(1), mci.Integrand(f))
        classic = eng.integrate_sweep("vegas", userdata=ud, neval=int(neval), niter=10, seeds=seeds)
        eng.set_stratification()
        strat = eng.integrate_sweep_strat("vegas", userdata=ud, neval=int(neval), niter=10, seeds=seeds)
        assert eng.last_sweep_launch()[0] == 32 and all(r["status"] == 0 for r in strat)
        sc = float(np.std([r["mean"][0] for r in classic], ddof=1))
        ss, es = float(np.std([r["mean"][0] for r in strat], ddof=1)), float(np.mean([r["stdev"][0] for r in strat]))
        print(name, "scatter classic sweep %.3g stratified sweep %.3g (reported %.3g)" % (sc, ss, es))
        assert 0.6 < ss / es < 1.5, (name, ss, es)
        ratios[name] = ss / sc
        eng.close()
    print("scatter stratified sweep / classic sweep:", ratios)
    assert ratios["benchmark1"] <= 0.5, ratios
    assert ratios["benchmark4"] <= 1.25, ratios
    assert ratios["c1"] <= 0.5, ratios


class Para:
    def __init__(self, a):
        self.a = a


def closure(x, c):
    return x[0] * x[0] + c.userdata.a * x[1] * x[1]


def test_end_to_end_closure():
    """a closure through mci.integrate_sweep(stratify=True): batched, one trace, one code object; the loop of integrate(stratify=True)"""
    params = [Para(0.5 + 0.25 * k) for k in range(5)]
    def kw():
        return dict(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED, solver="vegas", neval=20000, niter=4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rs = mci.integrate_sweep(closure, params, stratify=True, **kw())
    assert len(rs) == 5 and all(r.sweep_batched and r.status == 0 for r in rs)
    eng = rs[0].config._engine
    assert all(r.config._engine is eng for r in rs)      # one trace, one engine
    assert eng.code_object("vegas_sweep_strat").endswith(".hsaco")
    for p, r in zip(params, rs):
        one = mci.integrate(closure, userdata=p, stratify=True, **kw())
        np.testing.assert_allclose(r.iter_mean, one.iter_mean, rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(r.iter_std, one.iter_std, rtol=1e-2, atol=1e-300)
        np.testing.assert_allclose(r.mean, one.mean, rtol=1e-4)
        assert r.stratification["nstrat"] == one.stratification["nstrat"] and r.stratification["ncube"] == one.stratification["ncube"]
        assert r.strat_counts.sum() == 20000 and r.strat_d.shape == (r.stratification["ncube"],)
        assert abs(r.mean[0] - (1.0 + p.a) / 3.0) < 5 * r.stdev[0]
