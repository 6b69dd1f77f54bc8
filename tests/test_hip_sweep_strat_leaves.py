"""GPU tests of stratified (VEGAS+) sweep points of problems with SEVERAL Continuous variable leaves (mci_set_sweep_strat_leaves;
csrc/mci_sweep_strat_leaves.h vegas_sweep_strat_leaves): the teacher-forced chain of tests/test_hip_sweep_strat.py generalised to leaves
-- before each iteration the oracle takes the engine's grids of EVERY leaf and the counts the sweep reports -- against the oracle's plain
VEGAS+ iteration on identical Philox streams, against the ordinary stratified call, and against itself under another assignment of points
to workgroups.

Per point and iteration the bounds are those of tests/test_hip_sweep_strat.py check_point and tests/test_hip_stratified_parity.py, which
derive them; they are applied per leaf:

    allocation (counts_out)          mcio_strat_alloc of the ORACLE's d_h (uniform first)    check_alloc
    mean per column                  oracle (long double)                                    1e-11 * sum_h V / n_h sum |f J|
    sum_k s^2 = d_out^(2 / beta)     oracle two-pass                                         sum_k 4 (n_h + 2) 2^-53 S2 / (n_h - 1) + rel 1e-12
    variance per column              oracle                                                  sum_h V^2 / n_h * that bound + rel 1e-11
    every leaf's map after train!    oracle's train! of its histogram + (m + 1) 1e-10        abs 1e-12 * (upper - lower), ends equal, increasing
    a leaf with adapt=False          its input                                               bytes

One launch of several iterations against the chain: 1e-11 / 1e-8 on an iteration that follows no train!, 1e-4 / 1e-2 (maps 1e-4 * range)
over a run."""
import math
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_stratified_parity import LAYOUTS as PARITY, PEAK2, POOLS3, SEED, U, check_alloc, ocont
from test_hip_sweep_strat import merged_blocks

pytestmark = pytest.mark.gpu
PI = math.pi

X2Y2P = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
WATSON3P = "w[0] = 1.0 / (1.0 - ud[0] * cos(x[0]) * cos(x[1]) * cos(x[2])) / (M_PI * M_PI * M_PI);"
SPHERE2P = ("w[0] = (x[0] * x[0] + x[1] * x[1] < ud[0]) ? 1.0 : 0.0; "
            "w[1] = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] < ud[0]) ? 1.0 : 0.0;")
# layout: variables, dof, C body for both sides (ud[0] is the swept parameter), oracle leaves
LAYOUTS = {
    "two_grids": dict(var=lambda: mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], f=X2Y2P, oleaves=[ocont(0), ocont(0)]),
    "pools3": dict(var=PARITY["pools3"]["var"], dof=PARITY["pools3"]["dof"], f=POOLS3 + " w[0] *= ud[0];", oleaves=PARITY["pools3"]["oleaves"]),
    "watson3": dict(var=lambda: mci.Continuous([(0.0, PI)] * 3), dof=[[1]], f=WATSON3P, oleaves=[ocont(0, 0.0, PI) for _ in range(3)]),
    "peak2_two_grids": dict(var=lambda: mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], f=PEAK2 + " w[0] *= ud[0];", oleaves=[ocont(0), ocont(0)]),
    "two_pools_ragged": dict(var=lambda: (mci.Continuous(0.0, 1.0), mci.Continuous(0.0, 1.0, ninc=300)), dof=[[2, 0], [2, 1]], f=SPHERE2P,
                             oleaves=[ocont(0), ocont(1, npts=300)]),
}
# every (layout, nstrat, N, block, points) the chain runs below; tests/test_sweep_strat_leaves_host.py holds the allocation cap on them
CHAIN_CASES = [
    ("two_grids", [16, 16], 4096, 4, [1.0, 0.25, -2.0]),
    ("pools3", [3, 2, 2, 2], 48, 1, [1.0, 0.6]),
    ("pools3", [3, 2, 2, 2], 2048, 16, [1.0, 0.6]),
    ("pools3", [3, 2, 2, 2], 8193, 3, [1.0, 0.6]),
    ("pools3", [4, 1, 16, 32], 4096, 2, [1.0, 0.6]),
    ("watson3", [6, 6, 6], 4096, 4, [0.95, 0.5]),
    ("peak2_two_grids", [3, 2], 6000, 4, [1.0, 0.6]),
    ("two_pools_ragged", [5, 1, 3], 8192, 4, [1.0, 0.6, 0.8]),
]
CHAIN_IDS = ["%s-%d-%d" % (c[0], int(np.prod(c[1])), c[2]) for c in CHAIN_CASES]


def make(oracle, name, ud0):
    L = LAYOUTS[name]
    cfg = mci.Configuration(var=L["var"](), dof=L["dof"], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(L["f"], [ud0]))
    eng.set_sweep_strat_leaves("all")
    return L, eng, oracle.Config(L["oleaves"], L["dof"]), oracle.compile_c_integrand(L["f"])


def check_point(oracle, L, ocfg, of, ud, r, grids_in, want, nstrat, N, k, seed, beta, m_blocks, tag):
    """one point's one iteration against the oracle on the engine's grids and counts (check_point of tests/test_hip_sweep_strat.py, the
    map per leaf); returns the oracle's d_h and its (mean, std)"""
    nc = int(np.prod(nstrat))
    V = 1.0 / nc
    assert r["status"] == 0 and r["neval"] == N, tag
    counts = r["strat_counts"]
    check_alloc(counts, want, N, tag)
    off = np.concatenate([[0], np.cumsum(counts)])
    for i, g in enumerate(grids_in):
        ocfg.set_grid(i, g)
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
    for i in range(len(L["oleaves"])):
        ocfg.add_hist(i, m_blocks * 1e-10)
    ocfg.train()
    assert len(r["maps_by_leaf"]) == len(L["oleaves"]) and np.array_equal(np.concatenate(r["maps_by_leaf"]), r["maps"]), tag
    for i, lf in enumerate(L["oleaves"]):
        g, og = r["maps_by_leaf"][i], ocfg.grid(i)
        assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0), (tag, i)
        np.testing.assert_allclose(g, og, rtol=0, atol=1e-12 * (lf["upper"] - lf["lower"]), err_msg="%s leaf %d" % (tag, i))
        if not lf.get("adapt", True):
            assert g.tobytes() == np.ascontiguousarray(grids_in[i], dtype=np.float64).tobytes(), (tag, i, "a leaf that does not adapt")
    return o["d"].copy(), (o["mean"].copy(), np.sqrt(o["var"]))


def chain(oracle, name, nstrat, N, block, uds, niter=3, grid=2, beta=0.75, seed=SEED):
    """niter sweeps of one iteration each over the points `uds` on `grid` workgroups, maps (the flat rows) and d fed back; everything of
    the module's table asserted per point and iteration.  Returns (engine, [per iteration: result dicts], [per iteration: oracle rows])"""
    L, eng, ocfg, of = make(oracle, name, uds[0])
    eng.set_stratification(nstrat=nstrat, beta=beta)
    eng.sweep_workgroups(grid)
    P, nc, nleaf = len(uds), int(np.prod(nstrat)), len(L["oleaves"])
    m_blocks = merged_blocks(eng, N, block)
    geo = eng.sweep_strat_geometry(N, block)
    print("GEOMETRY %s %s N=%d block=%d: chunk %d, %d bytes of LDS, map at %d" % (name, nstrat, N, block, geo["chunk"], geo["lds_bytes"], geo["map_off"]))
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(nc), N, True))
    maps, d, want = None, None, [uniform] * P
    start = [[eng.grid(i) for i in range(nleaf)]] * P
    runs, rows = [], []
    for k in range(niter):
        rs = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds], neval=N, niter=1, block=block, seed=seed, ignore=0, maps=maps, d=d,
                                       first_iteration=k)
        assert eng.last_sweep_launch()[0] == min(grid, P)
        nxt, row = [], []
        for p in range(P):
            dref, mo = check_point(oracle, L, ocfg, of, [uds[p]], rs[p], start[p], want[p], nstrat, N, k, seed, beta, m_blocks,
                                   "%s %s N=%d point %d iteration %d" % (name, nstrat, N, p, k))
            nxt.append(np.diff(oracle.Config.strat_alloc(dref, N)))
            row.append(mo)
        want = nxt
        maps, d = np.array([r["maps"] for r in rs]), np.array([r["strat_d"] for r in rs])
        start = [r["maps_by_leaf"] for r in rs]
        runs.append(rs)
        rows.append(row)
    assert eng.code_object("vegas_sweep_strat_leaves").endswith(".hsaco")
    return eng, runs, rows


def test_first_iteration_three_points_on_two_workgroups(oracle):
    name, nstrat, N, block, uds = CHAIN_CASES[0]
    eng, runs, _ = chain(oracle, name, nstrat, N, block, uds, niter=1)
    m = [r["iter_mean"][0, 0] for r in runs[0]]
    assert abs(m[0] - m[1]) > 0.1 and abs(m[0] - m[2]) > 0.1      # (the points ARE different integrals)
    eng.close()


@pytest.mark.parametrize("name,nstrat,N,block,uds", CHAIN_CASES[1:7], ids=CHAIN_IDS[1:7])
def test_teacher_forced_chain(oracle, name, nstrat, N, block, uds):
    """pools3: 17, 257 and 1000 grid points (histogram slices that start at offsets that are no multiples of 256), alphas 0.5 and 3, a
    middle leaf that does not adapt; exactly two samples per hypercube, more blocks than chunks, an odd sample count, 2048 hypercubes of
    two samples.  watson3: a composite with one grid per axis.  peak2 on six hypercubes: once the samples have moved to the peak one
    hypercube is longer than the largest chunk, so the cut hypercube is carried from chunk to chunk"""
    eng, runs, _ = chain(oracle, name, nstrat, N, block, uds)
    counts = [r["strat_counts"] for rs in runs for r in rs]
    if N == 2 * int(np.prod(nstrat)):
        assert all(np.all(c == 2) for c in counts)      # exactly two samples per hypercube: nothing moves
    elif name == "peak2_two_grids":
        assert max(c.max() for c in counts) > 2048 and np.abs(counts[-1] - counts[0]).max() > 1
    if name == "pools3" and N > 48:
        first = eng.grid(0)
        assert any(not np.array_equal(r["maps_by_leaf"][0], first) for r in runs[-1])      # (the leaves that adapt did move)
    eng.close()


def _kw(N, block, niter, **more):
    return dict(neval=N, niter=niter, block=block, seed=SEED, **more)


def _ranges(name):
    return [lf["upper"] - lf["lower"] for lf in LAYOUTS[name]["oleaves"]]


def _maps_close(name, a, b, tol=1e-4):
    assert len(a) == len(b) == len(_ranges(name))
    for g, og, w in zip(a, b, _ranges(name)):
        assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0)
        np.testing.assert_allclose(g, og, rtol=0, atol=tol * w)


def test_one_launch_against_the_chain(oracle):
    name, nstrat, N, block, uds = CHAIN_CASES[7]
    eng, runs, rows = chain(oracle, name, nstrat, N, block, uds, niter=3)
    eng.sweep_workgroups(0)
    for niter, (rm, rs) in ((2, (1e-11, 1e-8)), (3, (1e-4, 1e-2))):
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
                _maps_close(name, r["maps_by_leaf"], runs[2][p]["maps_by_leaf"])
            assert r["neval"] == niter * N and r["status"] == 0
    eng.close()


def test_one_point_against_the_ordinary_call():
    name, N, block, niter, nstrat = "two_pools_ragged", 16384, 4, 3, [5, 1, 3]
    L = LAYOUTS[name]
    eng = mci.Engine(mci.Configuration(var=L["var"](), dof=L["dof"], seed=SEED), mci.Integrand(L["f"], [0.9]))
    eng.set_sweep_strat_leaves("all")
    eng.set_stratification(nstrat=nstrat)
    g0 = [eng.grid(i).copy() for i in range(2)]
    r = eng.integrate_sweep_strat("vegas", userdata=[[0.9]], **_kw(N, block, niter))[0]
    assert all(eng.grid(i).tobytes() == g0[i].tobytes() for i in range(2))      # the engine's own map: untouched
    res = mci.integrate(mci.Integrand(L["f"], [0.9]), var=L["var"](), dof=L["dof"], solver="vegas", neval=N, niter=niter, block=block, seed=SEED,
                        stratify=mci.Stratify(nstrat=nstrat))
    np.testing.assert_allclose(r["iter_mean"][0], res.iter_mean[0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"][0], res.iter_std[0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["iter_mean"], res.iter_mean, rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], res.iter_std, rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], res.mean, rtol=1e-4)
    np.testing.assert_allclose(r["stdev"], res.stdev, rtol=1e-2)
    _maps_close(name, r["maps_by_leaf"], [res.config._engine.grid(i) for i in range(2)])
    check_alloc(r["strat_counts"], res.config._engine.strat_counts(), N, "last allocation")
    eng.close()


def _engine(name, nstrat, ud0=1.0):
    L = LAYOUTS[name]
    eng = mci.Engine(mci.Configuration(var=L["var"](), dof=L["dof"], seed=SEED), mci.Integrand(L["f"], [ud0]))
    eng.set_sweep_strat_leaves("all")
    eng.set_stratification(nstrat=list(nstrat))
    return eng


def _agree(name, a, b):
    np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(a["iter_std"][0], b["iter_std"][0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(a["iter_std"], b["iter_std"], rtol=1e-2, atol=1e-300)
    _maps_close(name, a["maps_by_leaf"], b["maps_by_leaf"])


def test_nothing_leaks_between_points():
    """five points on two workgroups in two orders, an all-NaN point between: its status is set and both of its leaves' maps stay, the
    others do not see it"""
    eng = _engine("two_grids", [4, 4])
    eng.sweep_workgroups(2)
    uds = [1.0, 0.6, float("nan"), 0.8, 0.4]
    kw = _kw(8192, 4, 3)
    a = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds], **kw)
    order = [4, 2, 0, 3, 1]
    b = eng.integrate_sweep_strat("vegas", userdata=[[uds[i]] for i in order], **kw)
    eng.sweep_workgroups(0)
    alone = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in uds if u == u], **kw)
    assert a[2]["status"] != 0 and b[1]["status"] != 0
    for i in range(2):      # train! refused leaf by leaf: the maps stayed
        assert a[2]["maps_by_leaf"][i].tobytes() == eng.grid(i).tobytes() and b[1]["maps_by_leaf"][i].tobytes() == eng.grid(i).tobytes()
    good = [i for i in range(5) if i != 2]
    for j, i in enumerate(good):
        assert a[i]["status"] == 0 and np.all(np.isfinite(a[i]["iter_mean"])) and np.all(np.isfinite(a[i]["maps"]))
        _agree("two_grids", a[i], b[order.index(i)])
        _agree("two_grids", a[i], alone[j])
        assert a[i]["strat_counts"].sum() == 8192 and a[i]["strat_counts"].min() >= 2
    eng.close()


def test_ragged_points_and_seeds():
    """P = 7 on 3 workgroups against 7 workgroups; per-point seeds against one-point sweeps under those seeds"""
    name = "two_pools_ragged"
    eng = _engine(name, [5, 1, 3])
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
        _agree(name, a[k], b[k])
        check_alloc(a[k]["strat_counts"], b[k]["strat_counts"], 4096, "point %d" % k)
    for k in (0, 6):
        _agree(name, eng.integrate_sweep_strat("vegas", userdata=[uds[k]], seed=seeds[k], **kw)[0], a[k])
    assert a[0]["iter_mean"][0, 0] != a[1]["iter_mean"][0, 0]
    eng.close()


def test_train_then_freeze(oracle):
    """alloc= + maps= + adapt=False: the maps are bytes-equal, the allocation is that of the trained d"""
    name, N, block, nstrat = "two_pools_ragged", 8192, 4, [5, 1, 3]
    L = LAYOUTS[name]
    uds = [[1.0], [0.6], [0.8]]
    eng = _engine(name, nstrat)
    trained = eng.integrate_sweep_strat("vegas", userdata=uds, **_kw(N, block, 3))
    d = np.array([r["strat_d"] for r in trained])
    maps = np.array([r["maps"] for r in trained])
    assert maps.shape == (3, eng.sweep_map_doubles()) and eng.sweep_map_doubles() == 1000 + 300
    frozen = eng.integrate_sweep_strat("vegas", userdata=uds, adapt=False, d=d, maps=maps, **_kw(N, block, 3))
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(15), N, True))
    for p, r in enumerate(frozen):
        check_alloc(r["strat_counts"], np.diff(oracle.Config.strat_alloc(d[p], N)), N, "frozen point %d" % p)
        assert np.abs(r["strat_counts"] - uniform).max() > 1
        assert r["maps"].tobytes() == maps[p].tobytes()
        assert r["strat_d"].max() > 0 and not np.array_equal(r["strat_d"], d[p])      # (d_out is what the last iteration measured)
    eng.close()
    # through the public call: train, then freeze over the whole scan
    def kw():      # (a Configuration is built from these per call)
        return dict(var=L["var"](), dof=L["dof"], seed=SEED, solver="vegas", neval=N, block=block, niter=3, stratify=mci.Stratify(nstrat=nstrat), leaves="all")
    f = mci.Integrand(L["f"], [1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = mci.integrate_sweep(f, uds, **kw())
        fz = mci.integrate_sweep(f, uds, adapt=False, alloc=[r.strat_d for r in tr], maps=[r.map for r in tr], **kw())
    for a, b in zip(tr, fz):
        assert a.stratification["carried"] == "uniform" and b.stratification["carried"] == "same plan" and a.sweep_batched and b.sweep_batched
        assert b.map.tobytes() == a.map.tobytes() and b.stratification["nstrat"] == nstrat and b.stratification["ncube"] == 15
        assert len(b.maps_by_leaf) == 2 and [len(g) for g in b.maps_by_leaf] == [1000, 300]
        check_alloc(b.strat_counts, np.diff(oracle.Config.strat_alloc(np.asarray(a.strat_d), N)), N, "alloc=")


class Para:
    def __init__(self, a):
        self.a = a


def closure(X, c):
    return X[0][0] ** 2 + c.userdata.a * X[1][0] ** 2


def test_end_to_end_closure():
    """a closure over two variable types through mci.integrate_sweep(stratify=True, leaves="all"): batched, one trace, one code object; the
    loop of integrate(stratify=True)"""
    params = [Para(0.5 + 0.25 * k) for k in range(4)]
    def kw():
        return dict(var=(mci.Continuous(0.0, 1.0), mci.Continuous(0.0, 2.0)), seed=SEED, solver="vegas", neval=20000, niter=4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rs = mci.integrate_sweep(closure, params, stratify=True, leaves="all", **kw())
    assert len(rs) == 4 and all(r.sweep_batched and r.status == 0 for r in rs)
    eng = rs[0].config._engine
    assert all(r.config._engine is eng for r in rs)      # one trace, one engine
    assert eng.code_object("vegas_sweep_strat_leaves").endswith(".hsaco")
    for p, r in zip(params, rs):
        one = mci.integrate(closure, userdata=p, stratify=True, **kw())
        np.testing.assert_allclose(r.iter_mean, one.iter_mean, rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(r.iter_std, one.iter_std, rtol=1e-2, atol=1e-300)
        np.testing.assert_allclose(r.mean, one.mean, rtol=1e-4)
        assert r.stratification["nstrat"] == one.stratification["nstrat"] and r.stratification["ncube"] == one.stratification["ncube"]
        assert r.strat_counts.sum() == 20000 and r.strat_d.shape == (r.stratification["ncube"],) and len(r.maps_by_leaf) == 2
        assert abs(r.mean[0] - (2.0 / 3.0 + 8.0 * p.a / 3.0)) < 5 * r.stdev[0]
