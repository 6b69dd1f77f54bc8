"""GPU tests of :vegasmc parameter sweeps (Engine.integrate_sweep_chains, mci.integrate_sweep(..., solver="vegasmc", chains=K);
csrc/mci_sweep_chains.h vegasmc_sweep): one workgroup per point, the blocks of a point one after another, a lane per chain -- against
the oracle's chains with set_chain_carry(0) point by point, against the ordinary call with set_chain_carry(0) and one lane per chain,
against its own restarts, and against itself under another assignment of points to workgroups.

Tolerances.  A single iteration (no train!, no doReweight! before it) runs the oracle's chains on the oracle's streams: 1e-11 (mean) /
1e-8 (error) / 1e-11 (visited, reweight factors after one doReweight!), the propose | accept counts are integers plus offsets (1e-12),
one train! step 1e-12 of the range (grids) and 1e-11 (Discrete), as in test_hip_sweep_leaves.  Later iterations of runs whose maps went
through different sums: 1e-4 / 1e-2, maps 1e-4 of their range, or -- a chain is discontinuous in its accept tests -- the reference's
7 sigma band (test/runtests.jl:4-9) where said.

Bit-for-bit comparisons use at most 64 chains per block: one wave then runs a block's chains, and the order in which its lanes'
LDS histogram and observable adds land is the hardware's lane order; several waves add in the order they happen to run."""
import math
import types
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import CASES, SEED, make
from test_hip_sweep_leaves import bubble_integrand, bubble_measure, bubble_row, check_map, oracle_config, unpack

pytestmark = pytest.mark.gpu
PI = math.pi
NAMES = ["bubble", "sphere2_padding", "discrete"]
SHAPES = [(600, 3, 1), (700, 5, 7), (1500, 3, 300)]     # (nevalperblock, block, nchain): one chain | idle lanes | the chain loop's second trip


def rows(name, c, n=2):
    """n userdata rows of a case: the bubble's differ, the others have none or one fixed row"""
    if name == "bubble":
        return [bubble_row(k + 1) for k in range(n)]
    return [list(c["ud"] or []) for _ in range(n)]


def ud_array(uds):
    return np.array(uds, dtype=np.float64).reshape(len(uds), -1)


def engine(name, oracle):
    c, cfg, eng, _ = make(name, oracle)
    return c, cfg, eng


def npa_of(cfg):
    nd = cfg.N + 1
    return 3 * nd * max(nd, len(cfg.var))


def sweep(eng, uds, **kw):
    return eng.integrate_sweep_chains("vegasmc", userdata=ud_array(uds), **kw)


@pytest.mark.parametrize("npb,block,nchain", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_first_iteration_is_the_oracles(oracle, name, npb, block, nchain):
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    rs = sweep(eng, uds, neval=npb * block, niter=1, block=block, seed=SEED, ignore=0, nchain=nchain)
    assert eng.last_sweep_launch() == (2, 256)
    nobs, nd, npa = eng.nobs, cfg.N + 1, npa_of(cfg)
    for ud, r in zip(uds, rs):
        ocfg = oracle_config(oracle, c)
        ocfg.set_chain_carry(0)
        rw0 = np.array(ocfg.reweight, dtype=np.float64)
        packed = ocfg.iteration(oracle.VEGASMC, c["oname"], ud or None, npb, 0, block, 0, SEED, nchain=nchain)
        ocfg.train()
        om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
        visited = packed[2 * nobs + 2:2 * nobs + 2 + nd]
        print(name, npb, block, nchain, "mean", r["iter_mean"][0], om, "std", r["iter_std"][0], oe, "reweight", r["reweight"])
        np.testing.assert_allclose(r["iter_mean"][0], om, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], oe, rtol=1e-8, atol=1e-300)
        assert r["neval"] == packed[2 * nobs + 1] and r["status"] == 0 and r["correlated"] is False
        np.testing.assert_allclose(r["visited"], visited, rtol=1e-11)
        np.testing.assert_allclose(r["propose"].ravel(), packed[-2 * npa:-npa], rtol=1e-12)
        np.testing.assert_allclose(r["accept"].ravel(), packed[-npa:], rtol=1e-12)
        assert r["propose"][1, 0, :len(cfg.var)].sum() > 0.5 * block * (npb // nchain) * nchain
        np.testing.assert_allclose(r["reweight"], oracle.do_reweight(rw0, visited, 1.0), rtol=1e-11)   # one doReweight! (main.jl:183)
        for l, (lf, parts) in enumerate(zip(c["oleaves"], unpack(c["oleaves"], r["maps"]))):
            if lf["kind"] == 0:
                check_map(parts[0], ocfg.grid(l), 1e-12)
            else:
                np.testing.assert_allclose(parts[1], ocfg.distribution(l), rtol=1e-11)
                np.testing.assert_allclose(parts[0], ocfg.accumulation(l), rtol=1e-11)
                assert r["maps_by_leaf"][l].tobytes() == parts[1].tobytes()


@pytest.mark.parametrize("name,nchain", [("bubble", 7), ("sphere2_padding", 16), ("discrete", 1)])
def test_a_run_equals_its_restarts_bit_for_bit(oracle, name, nchain):
    """niter = 3 in one call against three niter = 1 calls chained through maps=, reweight= and first_iteration: the same kernel on the
    same state and the same streams (one wave of chains: the module's note on bit-for-bit comparisons)."""
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    kw = dict(neval=5 * 700, block=5, seed=SEED, nchain=nchain, ignore=0)
    whole = sweep(eng, uds, niter=3, **kw)
    maps = rw = None
    nevals = np.zeros(len(uds), dtype=np.int64)
    for it in range(3):
        part = sweep(eng, uds, niter=1, first_iteration=it, maps=maps, reweight=rw, **kw)
        nevals += [r["neval"] for r in part]
        maps, rw = np.array([r["maps"] for r in part]), np.array([r["reweight"] for r in part])
        for w, q in zip(whole, part):
            assert q["iter_mean"][0].tobytes() == w["iter_mean"][it].tobytes(), (it, q["iter_mean"][0], w["iter_mean"][it])
            assert q["iter_std"][0].tobytes() == w["iter_std"][it].tobytes()
    for w, q in zip(whole, part):
        assert q["maps"].tobytes() == w["maps"].tobytes() and q["reweight"].tobytes() == w["reweight"].tobytes()
        assert q["propose"].tobytes() == w["propose"].tobytes() and q["accept"].tobytes() == w["accept"].tobytes()
        assert q["status"] == w["status"] == 0
    # (config.neval counts the integrand calls of the steps: a block's 700 steps are 700 // nchain per chain)
    assert [w["neval"] for w in whole] == list(nevals) and all(0 < w["neval"] <= 3 * 5 * (700 // nchain) * nchain for w in whole)
    assert np.any(whole[0]["reweight"] != 1.0 / (cfg.N + 1))


def ordinary_engine(c, ud, name):
    cfg2 = mci.Configuration(var=c["var"](), dof=c["dof"], obs=c.get("obs"), seed=SEED)
    f = mci.Integrand(c["f"].body, ud, name) if ud else c["f"]
    eng = mci.Engine(cfg2, f, measure=c.get("measure"))
    eng.set_chain_carry(0)
    eng.set_chain_speculation(1)        # one lane per chain
    return eng


@pytest.mark.parametrize("name,nchain", [("bubble", 16), ("sphere2_padding", 64), ("discrete", 7)])
def test_a_sweep_of_one_point_equals_the_ordinary_call(oracle, name, nchain):
    """Engine.integrate("vegasmc", nchain=K) with fresh chains in every iteration and one lane per chain, niter = 4: the first iteration
    to rounding, the later ones to the tolerances of test_a_sweep_of_one_bubble_point_equals_the_ordinary_call."""
    c, cfg, eng = engine(name, oracle)
    ud = rows(name, c, 1)[0]
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED, nchain=nchain)
    # one iteration alone: both sides run the same chains, so the tables (the last iteration's on either side) agree entry by entry
    r1 = sweep(eng, [ud], **dict(kw, niter=1, ignore=0))[0]
    once = ordinary_engine(c, ud, name)
    once.integrate("vegasmc", **dict(kw, niter=1, ignore=0))
    pr1, ac1 = once.acceptance()
    np.testing.assert_allclose(r1["propose"], pr1, rtol=1e-12)
    np.testing.assert_allclose(r1["accept"], ac1, rtol=1e-12)
    np.testing.assert_allclose(r1["reweight"], once.reweight(), rtol=1e-11)
    r = sweep(eng, [ud], **kw)[0]
    ordinary = ordinary_engine(c, ud, name)
    q = ordinary.integrate("vegasmc", **kw)
    assert ordinary.last_chain_launch() == (nchain, False) and not q["correlated"]
    print(name, nchain, "sweep", r["iter_mean"], "ordinary", q["iter_mean"], "reweight", r["reweight"], ordinary.reweight())
    np.testing.assert_allclose(r["iter_mean"][0], q["iter_mean"][0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"][0], q["iter_std"][0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-4)
    np.testing.assert_allclose(r["reweight"], ordinary.reweight(), rtol=1e-4)
    pr, ac = ordinary.acceptance()
    np.testing.assert_allclose(r["propose"], pr, rtol=1e-12)          # (which pool a step proposes for does not depend on the chain's state)
    assert np.all(r["accept"] <= r["propose"]) and ac.shape == r["accept"].shape
    for l, lf in enumerate(c["oleaves"]):
        if lf["kind"] == 0:
            g = ordinary.grid(l)
            np.testing.assert_allclose(r["maps_by_leaf"][l], g, rtol=0, atol=1e-4 * (g[-1] - g[0]))
        else:
            np.testing.assert_allclose(r["maps_by_leaf"][l], ordinary.distribution(l)[0], rtol=0, atol=1e-4)


@pytest.mark.parametrize("name,nchain", [("bubble", 16), ("sphere2_padding", 300), ("discrete", 1)])
def test_whole_runs_against_the_oracles_integrate(oracle, name, nchain):
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    kw = dict(neval=8 * 1500, niter=4, block=8, seed=SEED, nchain=nchain)
    rs = sweep(eng, uds, **kw)
    for ud, r in zip(uds, rs):
        ocfg = oracle_config(oracle, c)
        ocfg.set_chain_carry(0)
        o = ocfg.integrate(oracle.VEGASMC, c["oname"], ud or None, **kw)
        print(name, nchain, "sweep", r["mean"], r["stdev"], "oracle", o["mean"], o["stdev"])
        np.testing.assert_allclose(r["iter_mean"][0], o["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], o["iter_std"][0], rtol=1e-8, atol=1e-300)
        assert np.all(np.abs(r["mean"] - o["mean"]) <= 7 * np.hypot(r["stdev"], o["stdev"]) + 1e-300)
        assert r["status"] == 0 and r["neval"] == o["neval"] and np.all(np.isfinite(r["iter_mean"]))


def same_point(a, b):
    """two runs of one point by the same kernel on the same streams, one wave of chains: everything, bit for bit"""
    for k in ("iter_mean", "iter_std", "maps", "reweight", "propose", "accept", "visited"):
        assert a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])
    assert a["status"] == b["status"] == 0 and np.all(np.isfinite(a["mean"]))


@pytest.mark.parametrize("pathological", [False, True])
def test_nothing_leaks_from_point_to_point(oracle, pathological):
    """two workgroups, five points: workgroup 0 runs A, C, E one after the other (then E, A in the second order), workgroup 1 B, D
    (then C).  Whatever a point left in LDS -- tables, counters, map block, verdict words -- or in its global rows (partial rows,
    propose | accept rows, reweight factors) would show in the point behind it.  pathological: B's kF is NaN."""
    A, B, C_, D_, E = (bubble_row(0.3 * k) for k in range(5))
    if pathological:
        B = [float("nan")] + B[1:]
    c, cfg, eng = engine("bubble", oracle)
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED, nchain=16)
    eng.sweep_workgroups(2)
    first = sweep(eng, [A, B, C_, D_, E], **kw)
    assert eng.last_sweep_launch()[0] == 2
    second = sweep(eng, [E, C_, A], **kw)
    for a, b in ((first[0], second[2]), (first[2], second[1]), (first[4], second[0])):
        same_point(a, b)
    eng.sweep_workgroups(0)
    alone = sweep(eng, [A, C_, D_, E], **kw)     # one workgroup per point: nothing before any of them
    for a, b in zip((first[0], first[2], first[3], first[4]), alone):
        same_point(a, b)
    if pathological:
        assert first[1]["status"] & 2, first[1]["status"]                 # ST_HIST_NONFINITE (variable.jl:212)
    else:
        assert first[1]["status"] == 0
    assert first[0]["reweight"].tobytes() != first[2]["reweight"].tobytes()


def test_per_point_seeds_change_the_results(oracle):
    c, cfg, eng = engine("sphere2_padding", oracle)
    s0, s1 = SEED, 777
    kw = dict(neval=16 * 1000, niter=3, block=16, nchain=16)
    rs = sweep(eng, [[], []], seeds=[s0, s1], **kw)
    for s, r in zip((s0, s1), rs):
        same_point(r, sweep(eng, [[]], seed=s, **kw)[0])
    assert rs[0]["iter_mean"][0][0] != rs[1]["iter_mean"][0][0] and rs[0]["reweight"].tobytes() != rs[1]["reweight"].tobytes()


def test_adapt_false_keeps_the_maps_and_still_reweights(oracle):
    c, cfg, eng = engine("bubble", oracle)
    uds = rows("bubble", c)
    kw = dict(neval=16 * 1000, block=16, seed=SEED, nchain=16)
    trained = sweep(eng, uds, niter=2, **kw)
    maps = np.array([r["maps"] for r in trained])
    rw = np.array([r["reweight"] for r in trained])
    fixed = sweep(eng, uds, niter=2, adapt=False, maps=maps, reweight=rw, first_iteration=2, **kw)
    for r, m, w in zip(fixed, maps, rw):
        assert r["maps"].tobytes() == m.tobytes() and r["status"] == 0
        assert np.all(r["reweight"] != w) and abs(r["reweight"].sum() - 1.0) < 1e-12       # main.jl:183 runs whatever `adapt` says
    start = sweep(eng, uds, niter=1, adapt=False, **kw)     # ... and from the engine's own (untrained) map
    for l in range(4):
        assert start[0]["maps_by_leaf"][l].tobytes() == eng.grid(l).tobytes()
    assert np.all(start[0]["reweight"] != 0.5)


def test_the_problems_own_state_is_untouched(oracle):
    c, cfg, eng = engine("bubble", oracle)
    eng.set_chain_carry(0)
    eng.integrate("vegasmc", neval=16 * 500, niter=2, block=16, seed=SEED, nchain=4)      # (a state worth keeping: trained map, moved factors)
    grids = [eng.grid(l).copy() for l in range(4)]
    dist, rw, packed = eng.distribution(4)[0].copy(), eng.reweight().copy(), eng.get_packed().copy()
    pr, ac = (t.copy() for t in eng.acceptance())
    assert np.all(rw != 0.5)
    rs = sweep(eng, rows("bubble", c), neval=16 * 1000, niter=3, block=16, seed=SEED, nchain=16)
    for l in range(4):
        assert eng.grid(l).tobytes() == grids[l].tobytes()
    assert eng.distribution(4)[0].tobytes() == dist.tobytes() and eng.reweight().tobytes() == rw.tobytes()
    assert eng.get_packed().tobytes() == packed.tobytes()
    assert eng.acceptance()[0].tobytes() == pr.tobytes() and eng.acceptance()[1].tobytes() == ac.tobytes()
    # the points started from that state: map and factors
    again = sweep(eng, rows("bubble", c), neval=16 * 1000, niter=3, block=16, seed=SEED, nchain=16,
                  maps=[np.concatenate(grids + [eng.distribution(4)[1], dist])] * 2, reweight=[rw] * 2)
    for a, b in zip(rs, again):
        same_point(a, b)


def test_the_bubble_closures_are_swept_on_one_code_object(monkeypatch):
    from mcintegration_jl_amd import trace
    p0 = mci.catalog.bubble_parameters()
    beta = p0["beta"]

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
        return dict(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)], solver="vegasmc", measure=bubble_measure, neval=16 * 1000, niter=4, seed=SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # batched: nothing warns
        rs = mci.integrate_sweep(bubble_integrand, params=objs, chains=16, **kw())
    assert len(calls) == 1
    monkeypatch.undo()
    assert len(rs) == 3 and all(r.sweep_batched for r in rs)
    eng = rs[0].config._engine
    assert isinstance(eng.integrand, mci.Integrand) and isinstance(eng.measure, mci.Measure) and all(r.config._engine is eng for r in rs)
    swept = eng.code_object("vegasmc_sweep")
    for other in ("vegas_sweep_leaves", "vegasmc"):
        with pytest.raises(mci.MCIError, match="has not been compiled yet"):
            eng.code_object(other)
    for obj, r in zip(objs, rs):
        assert r.config.userdata is obj and r.status == 0 and len(r.maps_by_leaf) == 5 and r.correlated is False
        assert r.reweight.shape == (2,) and abs(r.reweight.sum() - 1.0) < 1e-12 and r.map.shape == (4009,)
        pr, ac = r.config.propose, r.config.accept
        assert pr.shape == ac.shape == (3, 2, 5) and pr[1, 0].sum() > 0.5 * 16000 and np.all(ac <= pr)
        assert r.config.visited.shape == (2,) and np.all(r.config.visited > 0)
    assert rs[0].config.propose.tobytes() != rs[1].config.propose.tobytes() or rs[0].config.accept.tobytes() != rs[1].config.accept.tobytes()
    assert not np.allclose(np.asarray(rs[0].mean[0]), np.asarray(rs[1].mean[0]), rtol=1e-2)
    # resumed through reweight= and maps= (on other streams): the same scan, gone on with, on the same code object
    again = dict(kw(), seed=SEED + 1)
    more = mci.integrate_sweep(bubble_integrand, params=objs, chains=16, maps=[r.map for r in rs], reweight=[r.reweight for r in rs], **again)
    assert more[0].config._engine.code_object("vegasmc_sweep") == swept and all(r.sweep_batched and r.status == 0 for r in more)
    for r, m in zip(rs, more):
        assert np.all(np.abs(np.asarray(m.mean[0]) - np.asarray(r.mean[0])) <= 7 * np.hypot(np.asarray(m.stdev[0]), np.asarray(r.stdev[0])))
    # without chains= the same call warns once and loops, as ever: other chains (automatic count, carried), the same integrals
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        looped = mci.integrate_sweep(bubble_integrand, params=objs[:2], **kw())
    said = [w for w in rec if issubclass(w.category, RuntimeWarning) and "sweep" in str(w.message)]
    assert len(said) == 1 and "chain solvers are not swept" in str(said[0].message)
    assert all(r.sweep_batched is False for r in looped)
    for r, q in zip(rs, looped):
        assert np.all(np.abs(np.asarray(r.mean[0]) - np.asarray(q.mean[0])) <= 7 * np.hypot(np.asarray(r.stdev[0]), np.asarray(q.stdev[0])))
