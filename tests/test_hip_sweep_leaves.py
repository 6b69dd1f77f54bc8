"""GPU tests of :vegas parameter sweeps over problems with several variable leaves (Engine.set_sweep_leaves("all"); csrc/mci_sweep_leaves.h
vegas_sweep_leaves): Continuous and Discrete leaves, composites, a histogram over a Discrete draw -- one workgroup per point, the point's
whole map in LDS -- against the oracle's loop (main.jl:142-207) point by point, against the ordinary call, and against themselves under
another assignment of points to workgroups.

Tolerances are those of tests/test_hip_sweep.py and of test_hip_parity.test_full_integrate_matches_oracle[prefix], which the ordinary
call meets on these layouts: a single iteration (no train! before it) agrees to 1e-11 (mean) / 1e-8 (error); a run through the
prefix-scan walk to 1e-4 / 1e-2, maps to 1e-4 of their range; one train! step to 1e-12 of the range (grids) and 1e-11 (Discrete
distribution and accumulation), as in test_train_matches_oracle."""
import math
import types
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from catalog_params import bubble_userdata
from test_hip_parity import CASES, SEED, make, ocont, odisc

pytestmark = pytest.mark.gpu
PI = math.pi
KW = dict(neval=16 * 1000, niter=4, block=16, seed=SEED)


def check_first(r, o):
    np.testing.assert_allclose(r["iter_mean"][0], o["iter_mean"][0], rtol=1e-11, atol=1e-300, equal_nan=True)
    np.testing.assert_allclose(r["iter_std"][0], o["iter_std"][0], rtol=1e-8, atol=1e-300, equal_nan=True)


def check_run(r, o):
    np.testing.assert_allclose(r["iter_mean"], o["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], o["iter_std"], rtol=1e-2, atol=1e-300)


def check_map(g, og, atol):
    assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0)
    np.testing.assert_allclose(g, og, rtol=0, atol=atol * (og[-1] - og[0]))


def opted_in(name, oracle):
    c, cfg, eng, ocfg = make(name, oracle)
    eng.set_sweep_leaves("all")
    assert eng.sweep_supported() is None
    return c, cfg, eng


def oracle_config(oracle, c):
    return oracle.Config(c["oleaves"], c["dof"], obs_nbin=c.get("obs_nbin"), obs_bin_draw=c.get("obs_bin_draw"))


def bubble_row(k):
    ud = list(bubble_userdata())
    ud[0] *= 1 + 0.15 * k
    for i in range(6, 10):
        ud[i] *= 1 - 0.1 * k
    return ud


def unpack(oleaves, flat):
    """a flat maps row leaf by leaf: (grid,) of a Continuous leaf, (accumulation, distribution) of a Discrete one"""
    out, o = [], 0
    for lf in oleaves:
        if lf["kind"] == 0:
            n = lf.get("npts", 1000)
            out.append((flat[o:o + n],))
            o += n
        else:
            n = int(lf["upper"] - lf["lower"]) + 1
            out.append((flat[o:o + n + 1], flat[o + n + 1:o + 2 * n + 1]))
            o += 2 * n + 1
    assert o == len(flat)
    return out


# ---- the mixed layout: per-leaf sizes, per-leaf learning rates and an ADAPTING Discrete leaf together
MIXED_BODY = "const double t = x[0] - ud[1]; w[0] = x[2] * exp(-ud[0] * x[1]) / (0.01 + t * t);"
MIXED_LEAVES = [ocont(0, 0.0, 1.0, npts=65, alpha=1.5), ocont(1, 0.0, 2.0, alpha=2.0), odisc(2, 1, 7)]


def mixed_row(k):
    return [1.0 + k, 0.3 + 0.1 * k]


def mixed_engine():
    cfg = mci.Configuration(var=(mci.Continuous(0.0, 1.0, ninc=65, alpha=1.5), mci.Continuous(0.0, 2.0, alpha=2.0), mci.Discrete(1, 7)),
                            dof=[[1, 1, 1]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(MIXED_BODY, mixed_row(0), "mixed"))
    eng.set_sweep_leaves("all")
    assert eng.sweep_supported() is None
    return cfg, eng


def mixed_oracle(oracle, ud, **kw):
    ocfg = oracle.Config(MIXED_LEAVES, [[1, 1, 1]])
    return ocfg, ocfg.integrate(oracle.VEGAS, oracle.compile_c_integrand(MIXED_BODY, 1, "mixed"), list(ud), **kw)


def check_mixed_maps(r, ocfg, atol):
    leaves = unpack(MIXED_LEAVES, r["maps"])
    for l in (0, 1):
        check_map(leaves[l][0], ocfg.grid(l), atol)
        assert r["maps_by_leaf"][l].tobytes() == leaves[l][0].tobytes()
    np.testing.assert_allclose(leaves[2][1], ocfg.distribution(2), rtol=atol)
    np.testing.assert_allclose(leaves[2][0], ocfg.accumulation(2), rtol=atol, atol=atol)
    assert r["maps_by_leaf"][2].tobytes() == leaves[2][1].tobytes()


def test_bubble_points_are_the_oracles_runs(oracle):
    c, cfg, eng = opted_in("bubble", oracle)
    uds = [bubble_row(k) for k in range(3)]
    grids0 = [eng.grid(l).copy() for l in range(4)]
    dist0, packed0 = eng.distribution(4)[0].copy(), eng.get_packed().copy()
    rs = eng.integrate_sweep("vegas", userdata=uds, **KW)
    assert len(rs) == 3 and eng.last_sweep_launch() == (3, 256)
    for l in range(4):                                            # the engine's own state: untouched
        assert eng.grid(l).tobytes() == grids0[l].tobytes()
    assert eng.distribution(4)[0].tobytes() == dist0.tobytes() and eng.get_packed().tobytes() == packed0.tobytes()
    for ud, r in zip(uds, rs):
        ocfg = oracle_config(oracle, c)
        o = ocfg.integrate(oracle.VEGAS, "bubble", ud, **KW)
        assert r["iter_mean"].shape == (4, 4)                     # four iterations of the four-bin q histogram
        check_first(r, o)
        check_run(r, o)
        np.testing.assert_allclose(r["mean"], o["mean"], rtol=1e-4)
        assert r["neval"] == 4 * 16000 and r["status"] == 0
        leaves = unpack(c["oleaves"], r["maps"])
        for l in range(4):
            check_map(r["maps_by_leaf"][l], ocfg.grid(l), 1e-4)
            assert r["maps_by_leaf"][l].tobytes() == leaves[l][0].tobytes()
        assert r["maps_by_leaf"][4].tobytes() == dist0.tobytes()  # adapt = False: the Discrete leaf is where it started, bit for bit
        assert leaves[4][0].tobytes() == eng.distribution(4)[1].tobytes()
    assert np.any(np.abs(rs[0]["mean"] - rs[1]["mean"]) > 5 * rs[0]["stdev"])   # (the points ARE different integrals)


@pytest.mark.parametrize("name", ["bubble", "c2_gauss4_composite", "discrete2_composite", "discrete"])
def test_niter_1_leaves_the_oracles_first_iteration_and_one_train_step(oracle, name):
    c, cfg, eng = opted_in(name, oracle)
    block, npb = 8, 2000
    uds = [bubble_row(1), bubble_row(2)] if name == "bubble" else [c["ud"] or [], c["ud"] or []]
    rs = eng.integrate_sweep("vegas", userdata=np.array(uds, dtype=np.float64).reshape(2, -1), neval=block * npb, niter=1, block=block,
                             seed=SEED, ignore=0)
    nobs = eng.nobs
    for ud, r in zip(uds, rs):
        ocfg = oracle_config(oracle, c)
        packed = ocfg.iteration(oracle.VEGAS, c["oname"], ud or None, npb, 0, block, 0, SEED)
        ocfg.train()
        om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
        np.testing.assert_allclose(r["iter_mean"][0], om, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], oe, rtol=1e-8, atol=1e-300)
        assert r["neval"] == packed[2 * nobs + 1] and r["status"] == 0
        np.testing.assert_allclose(r["visited"], packed[2 * nobs + 2:2 * nobs + 2 + cfg.N + 1], rtol=1e-11)
        for l, (lf, parts) in enumerate(zip(c["oleaves"], unpack(c["oleaves"], r["maps"]))):
            if lf["kind"] == 0:
                check_map(parts[0], ocfg.grid(l), 1e-12)
            else:
                np.testing.assert_allclose(parts[1], ocfg.distribution(l), rtol=1e-11)
                np.testing.assert_allclose(parts[0], ocfg.accumulation(l), rtol=1e-11)
                assert r["maps_by_leaf"][l].tobytes() == parts[1].tobytes()


def test_mixed_sizes_learning_rates_and_an_adapting_discrete_leaf(oracle):
    cfg, eng = mixed_engine()
    uds = [mixed_row(k) for k in range(3)]
    rs = eng.integrate_sweep("vegas", userdata=uds, **KW)
    for ud, r in zip(uds, rs):
        ocfg, o = mixed_oracle(oracle, ud, **KW)
        check_first(r, o)
        check_run(r, o)
        assert r["status"] == 0 and r["neval"] == 4 * 16000
        check_mixed_maps(r, ocfg, 1e-4)
    d0 = np.full(7, 1.0 / 7)
    assert np.max(np.abs(rs[0]["maps_by_leaf"][2] - d0)) > 1e-2   # (the Discrete leaf DID adapt: the weight grows with its value)
    assert abs(rs[0]["mean"][0] - rs[1]["mean"][0]) > 10 * rs[0]["stdev"][0]


def test_a_sweep_of_one_bubble_point_equals_the_ordinary_call(oracle):
    ud = bubble_row(1)
    c, cfg, eng = opted_in("bubble", oracle)
    r = eng.integrate_sweep("vegas", userdata=[ud], **KW)[0]
    cfg2 = mci.Configuration(var=c["var"](), dof=c["dof"], obs=c.get("obs"), seed=SEED)
    ordinary = mci.Engine(cfg2, mci.Integrand(c["f"].body, ud, "bubble"), measure=c.get("measure"))
    q = ordinary.integrate("vegas", **KW)
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-4)
    for l in range(4):
        g = ordinary.grid(l)
        np.testing.assert_allclose(r["maps_by_leaf"][l], g, rtol=0, atol=1e-4 * (g[-1] - g[0]))
    np.testing.assert_allclose(r["maps_by_leaf"][4], ordinary.distribution(4)[0], rtol=0, atol=1e-4)


@pytest.mark.parametrize("pathological", [False, True])
def test_nothing_leaks_from_point_to_point(oracle, pathological):
    """two workgroups, five points: workgroup 0 runs A, C, E one after the other (then E, A in the second order), workgroup 1 B, D
    (then C).  Whatever a point left in LDS -- tables, map block, verdict words -- or in its global rows would show in the point behind
    it.  pathological: B's kF is NaN -- every weight, the observable and the histograms with it."""
    A, B, C_, D_, E = (bubble_row(0.3 * k) for k in range(5))
    if pathological:
        B = [float("nan")] + B[1:]
    c, cfg, eng = opted_in("bubble", oracle)
    eng.sweep_workgroups(2)
    first = eng.integrate_sweep("vegas", userdata=[A, B, C_, D_, E], **KW)
    assert eng.last_sweep_launch()[0] == 2
    second = eng.integrate_sweep("vegas", userdata=[E, C_, A], **KW)
    for a, b in ((first[0], second[2]), (first[2], second[1]), (first[4], second[0])):
        np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(a["iter_std"], b["iter_std"], rtol=1e-2, atol=1e-300)
        for l in range(4):
            g = a["maps_by_leaf"][l]
            np.testing.assert_allclose(g, b["maps_by_leaf"][l], rtol=0, atol=1e-4 * (g[-1] - g[0]))
    eng.sweep_workgroups(0)
    alone = eng.integrate_sweep("vegas", userdata=[A, C_, D_, E], **KW)    # one workgroup per point: nothing before any of them
    for a, b in zip((first[0], first[2], first[3], first[4]), alone):
        np.testing.assert_allclose(a["iter_mean"][0], b["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(a["iter_mean"], b["iter_mean"], rtol=1e-4, atol=1e-300)
        assert a["status"] == 0 and np.all(np.isfinite(a["mean"]))
    if pathological:
        assert first[1]["status"] & 2, first[1]["status"]                 # ST_HIST_NONFINITE (variable.jl:212)
    else:
        assert first[1]["status"] == 0


@pytest.mark.parametrize("npb,block", [(1000, 3), (257, 5)])
def test_ragged_sizes(oracle, npb, block):
    """a block count that is no power of two, a sample count that is no multiple of the workgroup size"""
    cfg, eng = mixed_engine()
    uds = [mixed_row(0), mixed_row(2)]
    kw = dict(neval=npb * block, niter=3, block=block, seed=SEED)
    rs = eng.integrate_sweep("vegas", userdata=uds, **kw)
    for ud, r in zip(uds, rs):
        ocfg, o = mixed_oracle(oracle, ud, **kw)
        check_first(r, o)
        check_run(r, o)
        assert r["neval"] == 3 * npb * block and r["status"] == 0


def test_resume_from_maps_out(oracle):
    c, cfg, eng = opted_in("bubble", oracle)
    uds = [bubble_row(k) for k in range(3)]
    kw = dict(neval=16 * 1000, block=16, seed=SEED)
    whole = eng.integrate_sweep("vegas", userdata=uds, niter=5, **kw)
    head = eng.integrate_sweep("vegas", userdata=uds, niter=3, **kw)
    tail = eng.integrate_sweep("vegas", userdata=uds, niter=2, first_iteration=3, maps=[r["maps"] for r in head], ignore=0, **kw)
    for w, h, t in zip(whole, head, tail):
        np.testing.assert_allclose(h["iter_mean"], w["iter_mean"][:3], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(t["iter_mean"], w["iter_mean"][3:], rtol=1e-4, atol=1e-300)
        for l in range(4):
            g = w["maps_by_leaf"][l]
            np.testing.assert_allclose(t["maps_by_leaf"][l], g, rtol=0, atol=1e-4 * (g[-1] - g[0]))
        assert t["maps_by_leaf"][4].tobytes() == w["maps_by_leaf"][4].tobytes()
    maps = np.array([r["maps"] for r in whole])
    fixed = eng.integrate_sweep("vegas", userdata=uds, niter=2, adapt=False, maps=maps, **kw)
    for r, m in zip(fixed, maps):
        assert r["maps"].tobytes() == m.tobytes()


def test_per_point_seeds(oracle):
    cfg, eng = mixed_engine()
    ud = mixed_row(1)
    s0, s1 = SEED, 777
    kw = dict(neval=16 * 1000, niter=3, block=16)
    rs = eng.integrate_sweep("vegas", userdata=[ud, ud], seeds=[s0, s1], **kw)
    for s, r in zip((s0, s1), rs):
        ocfg, o = mixed_oracle(oracle, ud, seed=s, **kw)
        check_first(r, o)
        check_run(r, o)
    assert rs[0]["iter_mean"][0][0] != rs[1]["iter_mean"][0][0]


# ---- the bubble closures of examples/bubble_closure.py (test/bubble.jl:40-88)
def green(tau, omega, beta):
    if tau >= 0.0:
        return np.exp(-omega * tau) / (1 + np.exp(-omega * beta)) if omega > 0.0 else np.exp(omega * (beta - tau)) / (1 + np.exp(omega * beta))
    return -np.exp(-omega * (tau + beta)) / (1 + np.exp(-omega * beta)) if omega > 0.0 else -np.exp(-omega * tau) / (1 + np.exp(omega * beta))


def bubble_integrand(vars, config):
    R, Theta, Phi, T, Ext = vars
    para = config.userdata
    kF, beta, me = para.kF, para.beta, para.me
    r = R[0] / (1 - R[0])
    theta, phi = Theta[0], Phi[0]
    k = np.array([r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)])
    factor = 1.0 / (2 * PI) ** para.dim
    factor *= r ** 2 / (1 - R[0]) ** 2 * np.sin(theta)
    Tin, Tout = 0.0, T[0]
    q = para.extQ[Ext[0] - 1]
    kq = k + q
    tau = Tout - Tin
    g1 = green(tau, (np.dot(k, k) - kF ** 2) / (2 * me), beta)
    g2 = green(-tau, (np.dot(kq, kq) - kF ** 2) / (2 * me), beta)
    return g1 * g2 * para.spin * factor


def bubble_measure(vars, obs, weight, config):
    Ext = vars[-1]
    obs[0][Ext[0] - 1] += weight[0]


def test_the_bubble_closures_are_swept_on_one_code_object(monkeypatch):
    from mcintegration_jl_amd import trace
    p0 = mci.catalog.bubble_parameters()
    beta = p0["beta"]                                              # (one T domain for the three points)

    def para(k):
        kF = p0["kF"] * (1 + 0.15 * k)
        return types.SimpleNamespace(kF=kF, beta=beta, me=0.5, spin=2, dim=3, Qsize=4,
                                     extQ=[np.array([q, 0.0, 0.0]) for q in np.linspace(0.0, 1.5 * kF * (1 - 0.1 * k), 4)])
    objs = [para(k) for k in range(3)]
    calls = []
    real = trace.trace_integrand
    monkeypatch.setattr(trace, "trace_integrand", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def kw():   # (variable objects per call: one that lives in an open engine hands its trained map on)
        var = (mci.Continuous(0.0, 1.0, alpha=3.0), mci.Continuous(0.0, PI, alpha=3.0), mci.Continuous(0.0, 2 * PI, alpha=3.0),
               mci.Continuous(0.0, beta, alpha=3.0), mci.Discrete(1, 4, adapt=False))
        return dict(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)], solver="vegas", measure=bubble_measure, neval=16 * 1000, niter=4, seed=SEED)
    rs = mci.integrate_sweep(bubble_integrand, params=objs, leaves="all", **kw())
    assert len(calls) == 1
    monkeypatch.undo()
    assert len(rs) == 3 and all(r.sweep_batched for r in rs)
    eng = rs[0].config._engine
    assert isinstance(eng.integrand, mci.Integrand) and isinstance(eng.measure, mci.Measure) and all(r.config._engine is eng for r in rs)
    swept = eng.code_object("vegas_sweep_leaves")
    for obj, r in zip(objs, rs):
        q = mci.integrate(bubble_integrand, userdata=obj, **kw())
        np.testing.assert_allclose(r.iter_mean, q.iter_mean, rtol=1e-4)
        np.testing.assert_allclose(np.asarray(r.mean[0]), np.asarray(q.mean[0]), rtol=1e-4)
        assert r.config.userdata is obj and r.status == 0 and len(r.maps_by_leaf) == 5
    assert eng.code_object("vegas_sweep_leaves") == swept
    assert not np.allclose(np.asarray(rs[0].mean[0]), np.asarray(rs[1].mean[0]), rtol=1e-2)
    # without the opt-in the same call warns once and loops, as ever
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        looped = mci.integrate_sweep(bubble_integrand, params=objs, **kw())
    said = [w for w in rec if issubclass(w.category, RuntimeWarning) and "sweep" in str(w.message)]
    assert len(said) == 1 and "5 variable leaves" in str(said[0].message)
    assert all(r.sweep_batched is False for r in looped)
    for r, l in zip(rs, looped):
        np.testing.assert_allclose(r.iter_mean, l.iter_mean, rtol=1e-4)
