"""GPU tests of batched :vegas parameter sweeps (mci_integrate_sweep; csrc/mci_sweep.h vegas_sweep): P independent integrals that differ
in the userdata row, one workgroup per point, in ONE launch -- against the oracle's loop (main.jl:142-207) point by point, against the
ordinary call, and against themselves under another assignment of points to workgroups.

Tolerances are those of the persistent launch's tests (tests/test_hip_persistent.py) and of
test_hip_parity.test_full_integrate_matches_oracle[prefix]: a single iteration (no train! in between) agrees to 1e-11 (mean) / 1e-8
(error); the refinement is the prefix-scan walk, whose whole-run agreement with the reference recurrence is 1e-4 (< 0.05 sigma).

The integrand is the 4-D Genz product peak, ud = [D, a, u...]; the points differ in a (2 .. 8) and in u."""
import time
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import SEED, make, ocont

pytestmark = pytest.mark.gpu
D = 4


def point(k):
    """userdata row of scan point k: a in [2, 8], peak positions u in [0.3, 0.7]"""
    rng = np.random.default_rng(1000 + k)
    return [float(D), 2.0 + 6.0 * ((k * 0.37) % 1.0)] + list(0.3 + 0.4 * rng.random(D))


def genz(ud):
    return mci.Integrand(mci.catalog.genz_product_peak(D).body, list(ud), "genz_product_peak%d" % D)


def engine(ud=None):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[D]], seed=SEED)
    return cfg, mci.Engine(cfg, genz(point(0) if ud is None else ud))


def oracle_run(oracle, ud, **kw):
    ocfg = oracle.Config([ocont()], [[D]])
    return ocfg, ocfg.integrate(oracle.VEGAS, "genz_product_peak", list(ud), **kw)


def check_first(r, o):
    np.testing.assert_allclose(r["iter_mean"][0], o["iter_mean"][0], rtol=1e-11, atol=1e-300, equal_nan=True)
    np.testing.assert_allclose(r["iter_std"][0], o["iter_std"][0], rtol=1e-8, atol=1e-300, equal_nan=True)


def check_run(r, o):
    np.testing.assert_allclose(r["iter_mean"], o["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], o["iter_std"], rtol=1e-2, atol=1e-300)


def check_map(g, og, atol):
    assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0)
    np.testing.assert_allclose(g, og, rtol=0, atol=atol * (og[-1] - og[0]))


def test_each_point_is_the_oracles_run(oracle):
    cfg, eng = engine()
    uds = [point(k) for k in range(3)]
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED)
    rs = eng.integrate_sweep("vegas", userdata=uds, **kw)
    assert len(rs) == 3 and eng.last_sweep_launch()[0] == 3
    for ud, r in zip(uds, rs):
        ocfg, o = oracle_run(oracle, ud, **kw)
        check_first(r, o)
        check_run(r, o)
        np.testing.assert_allclose(r["mean"], o["mean"], rtol=1e-4)
        np.testing.assert_allclose(r["stdev"], o["stdev"], rtol=1e-2)
        assert np.all(np.abs(r["mean"] - o["mean"]) < 5e-2 * o["stdev"])
        assert r["neval"] == 4 * 16000 and r["status"] == 0
        check_map(r["maps"], ocfg.grid(0), 1e-4)
    assert abs(rs[0]["mean"][0] - rs[1]["mean"][0]) > 10 * rs[0]["stdev"][0]   # (the points ARE different integrals)


def test_niter_1_leaves_the_oracles_first_iteration(oracle):
    """one iteration, one train!: the statistics the log row holds -- the iteration's mean and error, neval, config.visited -- and
    the map, at the per-iteration tolerances of the launch chain (the row itself stays on the device: a sweep returns results)"""
    cfg, eng = engine()
    block, npb = 8, 4000
    uds = [point(3), point(4)]
    rs = eng.integrate_sweep("vegas", userdata=uds, neval=block * npb, niter=1, block=block, seed=SEED, ignore=0)
    for ud, r in zip(uds, rs):
        ocfg = oracle.Config([ocont()], [[D]])
        packed = ocfg.iteration(oracle.VEGAS, "genz_product_peak", ud, npb, 0, block, 0, SEED)
        ocfg.train()
        om, oe = oracle.mean_std(packed[:1], packed[1:2], block)
        np.testing.assert_allclose(r["iter_mean"][0], om, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], oe, rtol=1e-8, atol=1e-300)
        assert r["neval"] == packed[3]
        np.testing.assert_allclose(r["visited"], packed[4:6], rtol=1e-11)
        check_map(r["maps"], ocfg.grid(0), 1e-12)


def test_a_sweep_of_one_point_equals_the_ordinary_call():
    ud = point(5)
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED)
    cfg, eng = engine(ud)
    g0, p0 = eng.grid(0).copy(), eng.get_packed().copy()
    r = eng.integrate_sweep("vegas", userdata=[ud], **kw)[0]
    assert np.array_equal(eng.grid(0), g0) and eng.grid(0).tobytes() == g0.tobytes()       # the engine's own state: untouched
    assert eng.get_packed().tobytes() == p0.tobytes()
    for mode in ("on", "off"):
        cfg2, ordinary = engine(ud)
        ordinary.set_persistent(mode)
        q = ordinary.integrate("vegas", **kw)
        assert ordinary.last_integrate_persistent() == (mode == "on")
        np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-2, atol=1e-300)
        np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-4)
        g = ordinary.grid(0)
        np.testing.assert_allclose(r["maps"], g, rtol=0, atol=1e-4 * (g[-1] - g[0]))


@pytest.mark.parametrize("pathological", [False, True])
def test_nothing_leaks_from_point_to_point(pathological):
    """two workgroups, five points: workgroup 0 runs A, C, E one after the other (then E, A in the second order), workgroup 1 B, D
    (then C).  Whatever a point left in LDS or in its global rows would show in the point behind it.  pathological: B's `a` is NaN --
    every weight, the observable and the histogram with it; the ordinary call raises MCI_ERR_HISTOGRAM for it."""
    A, B, C_, D_, E = (point(k) for k in range(10, 15))
    if pathological:
        B = [float(D), float("nan")] + B[2:]
    cfg, eng = engine()
    eng.sweep_workgroups(2)
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED)
    first = eng.integrate_sweep("vegas", userdata=[A, B, C_, D_, E], **kw)
    assert eng.last_sweep_launch()[0] == 2
    second = eng.integrate_sweep("vegas", userdata=[E, C_, A], **kw)
    for a, b in ((first[0], second[2]), (first[2], second[1]), (first[4], second[0])):
        np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(a["iter_std"], b["iter_std"], rtol=1e-2, atol=1e-300)
        np.testing.assert_allclose(a["maps"], b["maps"], rtol=0, atol=1e-4)
    eng.sweep_workgroups(0)
    alone = eng.integrate_sweep("vegas", userdata=[A, C_, D_, E], **kw)    # one workgroup per point: nothing before any of them
    for a, b in zip((first[0], first[2], first[3], first[4]), alone):
        np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
        assert a["status"] == 0 and np.all(np.isfinite(a["mean"]))
    if pathological:
        assert first[1]["status"] & 2, first[1]["status"]                 # ST_HIST_NONFINITE (variable.jl:212)
        cfg2, ordinary = engine(B)
        with pytest.raises(mci.MCIError) as e:
            ordinary.integrate("vegas", **kw)
        assert e.value.code == 5
    else:
        assert first[1]["status"] == 0


@pytest.mark.parametrize("npb,block", [(100, 16), (1001, 16), (1001, 1), (100, 1)])
def test_ragged_sizes(oracle, npb, block):
    """fewer samples per block than threads, a count that is no multiple of the workgroup size; one block and sixteen"""
    cfg, eng = engine()
    uds = [point(20), point(21)]
    kw = dict(neval=npb * block, niter=2, block=block, seed=SEED)
    rs = eng.integrate_sweep("vegas", userdata=uds, **kw)
    for ud, r in zip(uds, rs):
        check_first(r, oracle_run(oracle, ud, **kw)[1])
        assert r["neval"] == 2 * npb * block


def test_more_points_than_workgroups_at_the_default_grid(oracle):
    cfg, eng = engine()
    P = 600
    uds = [point(100 + k) for k in range(P)]
    kw = dict(neval=16 * 100, niter=2, block=16, seed=SEED)
    t0 = time.time()
    rs = eng.integrate_sweep("vegas", userdata=uds, **kw)
    assert time.time() - t0 < 60.0
    assert len(rs) == P and eng.last_sweep_launch()[0] < P
    for r in rs:
        assert np.all(np.isfinite(r["iter_mean"])) and np.all(np.isfinite(r["iter_std"])) and np.all(np.isfinite(r["mean"])) and r["status"] == 0
    for k in range(0, P, 50):
        check_first(rs[k], oracle_run(oracle, uds[k], **kw)[1])


def test_resume_from_maps_out():
    cfg, eng = engine()
    uds = [point(30), point(31), point(32)]
    kw = dict(neval=16 * 1000, block=16, seed=SEED)
    whole = eng.integrate_sweep("vegas", userdata=uds, niter=5, **kw)
    head = eng.integrate_sweep("vegas", userdata=uds, niter=3, **kw)
    tail = eng.integrate_sweep("vegas", userdata=uds, niter=2, first_iteration=3, maps=[r["maps"] for r in head], ignore=0, **kw)
    for w, h, t in zip(whole, head, tail):
        np.testing.assert_allclose(h["iter_mean"], w["iter_mean"][:3], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(t["iter_mean"], w["iter_mean"][3:], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(t["maps"], w["maps"], rtol=0, atol=1e-4)
    maps = np.array([r["maps"] for r in whole])
    fixed = eng.integrate_sweep("vegas", userdata=uds, niter=2, adapt=False, maps=maps, **kw)
    for r, m in zip(fixed, maps):
        assert r["maps"].tobytes() == m.tobytes()


def test_per_point_seeds(oracle):
    cfg, eng = engine()
    ud = point(40)
    s0, s1 = SEED, 777
    kw = dict(neval=16 * 1000, niter=3, block=16)
    rs = eng.integrate_sweep("vegas", userdata=[ud, ud], seeds=[s0, s1], **kw)
    for s, r in zip((s0, s1), rs):
        o = oracle_run(oracle, ud, seed=s, **kw)[1]
        check_first(r, o)
        check_run(r, o)
    assert rs[0]["iter_mean"][0][0] != rs[1]["iter_mean"][0][0]


@pytest.mark.parametrize("name,word", [("discrete", "Discrete"), ("c2_gauss4_composite", "4 variable leaves")])
def test_layouts_a_sweep_refuses_say_why(oracle, name, word):
    c, cfg, eng, ocfg = make(name, oracle)
    why = eng.sweep_supported()
    assert why and word in why, why
    ud = np.zeros((2, len(eng.integrand.userdata)))
    with pytest.raises(mci.MCIError) as e:
        eng.integrate_sweep("vegas", userdata=ud, neval=16000, niter=2)
    assert e.value.code == 1 and why in str(e.value)


def test_measurefreq_2_is_refused_with_the_reason():
    cfg, eng = engine()
    assert eng.sweep_supported() is None
    why = eng.sweep_supported(measurefreq=2)
    assert why and "measurefreq = 2" in why
    with pytest.raises(mci.MCIError) as e:
        eng.integrate_sweep("vegas", userdata=[point(0)], neval=16000, niter=2, measurefreq=2)
    assert e.value.code == 1 and why in str(e.value)


def test_the_fallback_of_integrate_sweep_warns_once_and_loops(oracle):
    """two independent grids are no sweep layout: mci.integrate_sweep runs the points as ordinary calls, says so once, and marks them"""
    L = 50.0 ** 0.5
    f = mci.catalog.gaussian(2)
    rows = [list(f.userdata)] * 3
    kw = dict(var=mci.Continuous([(-L, L)] * 2), dof=[[1]], solver="vegas", neval=16000, niter=3, seed=SEED)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        rs = mci.integrate_sweep(f, params=rows, **kw)
    said = [w for w in rec if issubclass(w.category, RuntimeWarning) and "sweep" in str(w.message)]
    assert len(said) == 1 and "2 variable leaves" in str(said[0].message)
    assert len(rs) == 3 and all(r.sweep_batched is False for r in rs)
    for r in rs:
        q = mci.integrate(f, var=mci.Continuous([(-L, L)] * 2), dof=[[1]], solver="vegas", neval=16000, niter=3, seed=SEED)
        np.testing.assert_allclose(r.iter_mean, q.iter_mean, rtol=1e-9)
        np.testing.assert_allclose(r.mean[0], q.mean[0], rtol=1e-9)


def test_a_16d_one_leaf_layout_is_swept_or_refused_with_its_reason(oracle):
    """sixteen draws on one shared grid (c2_gauss16_shared_pool): the draw count alone is no reason to refuse"""
    c, cfg, eng, ocfg = make("c2_gauss16_shared_pool", oracle)
    why = eng.sweep_supported()
    kw = dict(neval=16 * 1000, niter=2, block=16, seed=SEED)
    if why is None:
        r = eng.integrate_sweep("vegas", userdata=[c["ud"], c["ud"]], **kw)
        o = ocfg.integrate(oracle.VEGAS, c["oname"], c["ud"], **kw)
        check_first(r[0], o)
        check_first(r[1], o)
    else:
        assert "draw" not in why
        with pytest.raises(mci.MCIError) as e:
            eng.integrate_sweep("vegas", userdata=[c["ud"]], **kw)
        assert why in str(e.value)


def test_a_traced_closure_over_a_struct_of_parameters_is_swept_on_one_code_object(monkeypatch):
    """the closure reads its parameters off config.userdata (a struct of floats, as examples/bubble_closure.py does): traced ONCE, every
    point's ud row evaluated from its object, one sweep code object, each point the ordinary call of that object"""
    import types
    from mcintegration_jl_amd import trace

    def peak(x, c):
        p = c.userdata
        q = 1.0
        for d in range(D):
            t = x[d] - p.u[d]
            q = q * (1.0 / (p.a * p.a) + t * t)
        return 1.0 / q

    objs = [types.SimpleNamespace(a=2.0 + 1.5 * k, u=np.array(point(50 + k)[2:])) for k in range(4)]
    calls = []
    real = trace.trace_integrand
    monkeypatch.setattr(trace, "trace_integrand", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    def kw():   # (a variable object per call: one that lives in an open engine hands its trained map on, docs/src/index.md:129)
        return dict(var=mci.Continuous(0.0, 1.0), dof=[[D]], solver="vegas", neval=16 * 1000, niter=4, seed=SEED)
    rs = mci.integrate_sweep(peak, params=objs, **kw())
    assert len(calls) == 1
    monkeypatch.undo()
    assert len(rs) == 4 and all(r.sweep_batched for r in rs)
    eng = rs[0].config._engine
    assert isinstance(eng.integrand, mci.Integrand) and all(r.config._engine is eng for r in rs)
    swept = eng.code_object("vegas_sweep")
    for obj, r in zip(objs, rs):
        q = mci.integrate(peak, userdata=obj, **kw())
        np.testing.assert_allclose(r.iter_mean, q.iter_mean, rtol=1e-4)
        assert abs(r.mean[0] - q.mean[0]) < 5e-2 * q.stdev[0]
        assert r.config.userdata is obj
    assert eng.code_object("vegas_sweep") == swept
