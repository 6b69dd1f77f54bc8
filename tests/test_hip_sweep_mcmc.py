"""GPU tests of :mcmc parameter sweeps (Engine.integrate_sweep_mcmc, mci.integrate_sweep(..., solver="mcmc", mcmc_chains=K);
csrc/mci_sweep_chains.h mcmc_sweep): one workgroup per point, the blocks of a point one after another, a lane per chain -- against
the oracle's chains with set_chain_carry(0) point by point, against the ordinary call with set_chain_carry(0) and one lane per chain,
against its own restarts, and against itself under another assignment of points to workgroups.

Tolerances: those of test_hip_sweep_chains.  A single iteration (no train!, no doReweight! before it) runs the oracle's chains on the
oracle's streams: 1e-11 (mean) / 1e-8 (error) / 1e-11 (visited, reweight factors after one doReweight!), the propose | accept counts
are integers plus offsets (1e-12), one train! step 1e-12 of the range (grids) and 1e-11 (Discrete).  Later iterations of runs whose maps
went through different sums: 1e-4 / 1e-2, maps 1e-4 of their range, or -- a chain is discontinuous in its accept tests -- the
reference's 7 sigma band (test/runtests.jl:4-9) where said.  The holding-time histograms are integer bookkeeping: equal.

Bit-for-bit comparisons use at most 64 chains per block: one wave then runs a block's chains, and the order in which its lanes'
LDS histogram and observable adds land is the hardware's lane order; several waves add in the order they happen to run."""
import io
import math
import types
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import CASES, SEED, make
from test_hip_sweep_leaves import bubble_integrand, bubble_row, check_map, oracle_config, unpack

pytestmark = pytest.mark.gpu
PI = math.pi
NAMES = ["bubble", "sphere2_padding", "discrete"]
SHAPES = [(600, 3, 1), (700, 5, 7), (1500, 3, 300)]     # (nevalperblock, block, nchain): the reference's chain | idle lanes | the chain loop's second trip
TR = 0.1                                                 # thermal_ratio
ST_MCMC_INIT = 16


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


def fresh_oracle(oracle, c):
    ocfg = oracle_config(oracle, c)
    ocfg.set_chain_carry(0)
    ocfg.set_thermal_ratio(TR)
    return ocfg


def npa_of(cfg):
    nd = cfg.N + 1
    return 3 * nd * max(nd, len(cfg.var))


def sweep(eng, uds, **kw):
    return eng.integrate_sweep_mcmc("mcmc", userdata=ud_array(uds), thermal_ratio=TR, **kw)


def hold_max(h):
    top = np.flatnonzero(h)
    return (1 << int(top[-1])) - 1 if top.size else 0


@pytest.mark.parametrize("npb,block,nchain", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_first_iteration_is_the_oracles(oracle, name, npb, block, nchain):
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    rs = sweep(eng, uds, neval=npb * block, niter=1, block=block, seed=SEED, ignore=0, nchain=nchain)
    assert eng.last_sweep_launch() == (2, 256)
    nobs, nd, npa = eng.nobs, cfg.N + 1, npa_of(cfg)
    for ud, r in zip(uds, rs):
        ocfg = fresh_oracle(oracle, c)
        rw0 = np.array(ocfg.reweight, dtype=np.float64)
        packed = ocfg.iteration(oracle.MCMC, c["oname"], ud or None, npb, 0, block, 0, SEED, nchain=nchain)
        ohold = ocfg.hold_hist
        ocfg.train()
        om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
        visited = packed[2 * nobs + 2:2 * nobs + 2 + nd]
        print(name, npb, block, nchain, "mean", r["iter_mean"][0], om, "std", r["iter_std"][0], oe, "reweight", r["reweight"],
              "holds", np.flatnonzero(r["holds"]), r["hold_max"])
        np.testing.assert_allclose(r["iter_mean"][0], om, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], oe, rtol=1e-8, atol=1e-300)
        assert r["neval"] == packed[2 * nobs + 1] and r["status"] == 0 and r["correlated"] is False
        np.testing.assert_allclose(r["visited"], visited, rtol=1e-11)
        np.testing.assert_allclose(r["propose"].ravel(), packed[-2 * npa:-npa], rtol=1e-12)
        np.testing.assert_allclose(r["accept"].ravel(), packed[-npa:], rtol=1e-12)
        np.testing.assert_allclose(r["reweight"], oracle.do_reweight(rw0, visited, 1.0), rtol=1e-11)   # one doReweight! (main.jl:183)
        np.testing.assert_array_equal(r["holds"], ohold)
        assert r["holds"].sum() == block * nchain and r["hold_max"] == hold_max(ohold)
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
    same state and the same streams (one wave of chains: the module's note on bit-for-bit comparisons).  The holds of the run are the
    sum of the three."""
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    kw = dict(neval=5 * 700, block=5, seed=SEED, nchain=nchain, ignore=0)
    whole = sweep(eng, uds, niter=3, **kw)
    maps = rw = None
    nevals = np.zeros(len(uds), dtype=np.int64)
    holds = np.zeros((len(uds), 64), dtype=np.uint64)
    for it in range(3):
        part = sweep(eng, uds, niter=1, first_iteration=it, maps=maps, reweight=rw, **kw)
        nevals += [r["neval"] for r in part]
        holds += np.array([r["holds"] for r in part])
        maps, rw = np.array([r["maps"] for r in part]), np.array([r["reweight"] for r in part])
        for w, q in zip(whole, part):
            assert q["iter_mean"][0].tobytes() == w["iter_mean"][it].tobytes(), (it, q["iter_mean"][0], w["iter_mean"][it])
            assert q["iter_std"][0].tobytes() == w["iter_std"][it].tobytes()
            assert q["holds"].sum() == 5 * nchain
    for w, q, h in zip(whole, part, holds):
        assert q["maps"].tobytes() == w["maps"].tobytes() and q["reweight"].tobytes() == w["reweight"].tobytes()
        assert q["propose"].tobytes() == w["propose"].tobytes() and q["accept"].tobytes() == w["accept"].tobytes()
        assert q["status"] == w["status"] == 0
        np.testing.assert_array_equal(w["holds"], h)
        assert w["holds"].sum() == 3 * 5 * nchain and w["hold_max"] == hold_max(h)
    assert [w["neval"] for w in whole] == list(nevals) and all(0 < w["neval"] <= 3 * 5 * (700 // nchain + 700) * nchain for w in whole)
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
    """Engine.integrate("mcmc", nchain=K) with fresh chains in every iteration and one lane per chain, niter = 4: the first iteration
    to rounding, the later ones to the tolerances of the module's docstring; the holds of one iteration are mci_get_hold_histogram's."""
    c, cfg, eng = engine(name, oracle)
    ud = rows(name, c, 1)[0]
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED, nchain=nchain)
    # one iteration alone: both sides run the same chains, so the tables (the last iteration's on either side) agree entry by entry
    r1 = sweep(eng, [ud], **dict(kw, niter=1, ignore=0))[0]
    once = ordinary_engine(c, ud, name)
    once.integrate("mcmc", thermal_ratio=TR, **dict(kw, niter=1, ignore=0))
    pr1, ac1 = once.acceptance()
    np.testing.assert_allclose(r1["propose"], pr1, rtol=1e-12)
    np.testing.assert_allclose(r1["accept"], ac1, rtol=1e-12)
    np.testing.assert_allclose(r1["reweight"], once.reweight(), rtol=1e-11)
    np.testing.assert_array_equal(r1["holds"], once.hold_histogram())
    r = sweep(eng, [ud], **kw)[0]
    ordinary = ordinary_engine(c, ud, name)
    q = ordinary.integrate("mcmc", thermal_ratio=TR, **kw)
    assert ordinary.last_chain_launch() == (nchain, False) and not q["correlated"]
    print(name, nchain, "sweep", r["iter_mean"], "ordinary", q["iter_mean"], "reweight", r["reweight"], ordinary.reweight())
    np.testing.assert_allclose(r["iter_mean"][0], q["iter_mean"][0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"][0], q["iter_std"][0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-4)
    np.testing.assert_allclose(r["reweight"], ordinary.reweight(), rtol=1e-4)
    assert np.all(r["accept"] <= r["propose"]) and ordinary.acceptance()[1].shape == r["accept"].shape
    assert r["holds"].sum() == 4 * 16 * nchain
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
        ocfg = fresh_oracle(oracle, c)
        o = ocfg.integrate(oracle.MCMC, c["oname"], ud or None, **kw)
        print(name, nchain, "sweep", r["mean"], r["stdev"], "oracle", o["mean"], o["stdev"])
        np.testing.assert_allclose(r["iter_mean"][0], o["iter_mean"][0], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"][0], o["iter_std"][0], rtol=1e-8, atol=1e-300)
        assert np.all(np.abs(r["mean"] - o["mean"]) <= 7 * np.hypot(r["stdev"], o["stdev"]) + 1e-300)
        assert r["status"] == 0 and r["neval"] == o["neval"] and np.all(np.isfinite(r["iter_mean"]))


def same_point(a, b):
    """two runs of one point by the same kernel on the same streams, one wave of chains: everything, bit for bit"""
    for k in ("iter_mean", "iter_std", "maps", "reweight", "propose", "accept", "visited", "holds"):
        assert a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])
    assert a["status"] == b["status"] == 0 and np.all(np.isfinite(a["mean"])) and a["hold_max"] == b["hold_max"]


@pytest.mark.parametrize("bad", [None, "zero", "nan"])
def test_nothing_leaks_from_point_to_point(oracle, bad):
    """two workgroups, five points: workgroup 0 runs A, C, E one after the other (then E, A in the second order), workgroup 1 B, D
    (then C).  Whatever a point left in LDS -- tables, counters, map block, verdict words -- or in its global rows (partial rows,
    propose | accept rows, reweight factors, holds) would show in the point behind it.
    bad = "zero": B's spin is 0, its integrand 0 wherever a chain starts -- after 10000 tries the chains that start on it report
    ST_MCMC_INIT in B's status word (mcmc/montecarlo.jl:109-110; a device status flag, not a fault).
    bad = "nan": B's kF is NaN, so is its integrand.  `probability ~ 0.0` (montecarlo.jl:109) is false for a NaN, in the reference, in the
    ordinary call and here: such a point raises no ST_MCMC_INIT, it shows in its own non-finite results -- and in nobody else's."""
    A, B, C_, D_, E = (bubble_row(0.3 * k) for k in range(5))
    if bad == "zero":
        B = B[:3] + [0.0] + B[4:]
    elif bad == "nan":
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
    alone = sweep(eng, [A, C_, D_, E], **kw)     # one workgroup per point: nothing before any of them, and no bad point among them
    for a, b in zip((first[0], first[2], first[3], first[4]), alone):
        same_point(a, b)
    print(bad, "status of B", first[1]["status"], "mean", first[1]["mean"])
    if bad == "zero":
        assert first[1]["status"] & ST_MCMC_INIT, first[1]["status"]
    elif bad == "nan":
        assert not (first[1]["status"] & ST_MCMC_INIT) and not np.all(np.isfinite(first[1]["iter_mean"]))
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
    eng.integrate("mcmc", neval=16 * 500, niter=2, block=16, seed=SEED, nchain=4)      # (a state worth keeping: trained map, moved factors)
    grids = [eng.grid(l).copy() for l in range(4)]
    dist, rw, packed = eng.distribution(4)[0].copy(), eng.reweight().copy(), eng.get_packed().copy()
    pr, ac = (t.copy() for t in eng.acceptance())
    hh = eng.hold_histogram().copy()
    assert np.all(rw != 0.5) and hh.sum() == 16 * 4
    rs = sweep(eng, rows("bubble", c), neval=16 * 1000, niter=3, block=16, seed=SEED, nchain=16)
    for l in range(4):
        assert eng.grid(l).tobytes() == grids[l].tobytes()
    assert eng.distribution(4)[0].tobytes() == dist.tobytes() and eng.reweight().tobytes() == rw.tobytes()
    assert eng.get_packed().tobytes() == packed.tobytes()
    assert eng.acceptance()[0].tobytes() == pr.tobytes() and eng.acceptance()[1].tobytes() == ac.tobytes()
    np.testing.assert_array_equal(eng.hold_histogram(), hh)
    # the points started from that state: map and factors
    again = sweep(eng, rows("bubble", c), neval=16 * 1000, niter=3, block=16, seed=SEED, nchain=16,
                  maps=[np.concatenate(grids + [eng.distribution(4)[1], dist])] * 2, reweight=[rw] * 2)
    for a, b in zip(rs, again):
        same_point(a, b)


def bubble_integrand_mcmc(idx, vars, config):       # integrand(idx, var, config), mcmc/montecarlo.jl:34
    return bubble_integrand(vars, config)


def bubble_measure_mcmc(idx, vars, obs, relative_weight, config):      # measure(idx, var, obs, relative_weight, config), :166-169
    Ext = vars[-1]
    obs[0][Ext[0] - 1] += relative_weight


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
        return dict(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)], solver="mcmc", measure=bubble_measure_mcmc, neval=16 * 1000, niter=4, seed=SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # batched: nothing warns
        rs = mci.integrate_sweep(bubble_integrand_mcmc, params=objs, mcmc_chains=16, **kw())
    assert len(calls) == 1
    monkeypatch.undo()
    assert len(rs) == 3 and all(r.sweep_batched for r in rs)
    eng = rs[0].config._engine
    assert isinstance(eng.integrand, mci.Integrand) and isinstance(eng.measure, mci.Measure) and all(r.config._engine is eng for r in rs)
    swept = eng.code_object("mcmc_sweep")
    for other in ("vegas_sweep_leaves", "vegasmc_sweep", "mcmc"):
        with pytest.raises(mci.MCIError, match="has not been compiled yet"):
            eng.code_object(other)
    for obj, r in zip(objs, rs):
        assert r.config.userdata is obj and r.status == 0 and len(r.maps_by_leaf) == 5 and r.correlated is False
        assert r.reweight.shape == (2,) and abs(r.reweight.sum() - 1.0) < 1e-12 and r.map.shape == (4009,)
        pr, ac = r.config.propose, r.config.accept
        assert pr.shape == ac.shape == (3, 2, 5) and pr.sum() > 0.5 * 16000 and np.all(ac <= pr)
        assert r.config.visited.shape == (2,) and np.all(r.config.visited > 0)
        assert r.holds.shape == (64,) and r.holds.sum() == 4 * 16 * 16 and r.hold_max == hold_max(r.holds) > 0 and r.chain_steps == 1000 // 16
    assert rs[0].config.propose.tobytes() != rs[1].config.propose.tobytes() or rs[0].config.accept.tobytes() != rs[1].config.accept.tobytes()
    assert not np.allclose(np.asarray(rs[0].mean[0]), np.asarray(rs[1].mean[0]), rtol=1e-2)
    # resumed through reweight= and maps= (on other streams): the same scan, gone on with, on the same code object
    again = dict(kw(), seed=SEED + 1)
    more = mci.integrate_sweep(bubble_integrand_mcmc, params=objs, mcmc_chains=16, maps=[r.map for r in rs], reweight=[r.reweight for r in rs], **again)
    assert more[0].config._engine.code_object("mcmc_sweep") == swept and all(r.sweep_batched and r.status == 0 for r in more)


def test_the_report_note_follows_the_oracles_holds(oracle):
    """(600, 3, 1) on sphere2: the oracle's chains hold up to bin 6 (63 steps: 16 x 63 > 600), a note; ten times the length, the same
    top bin (16 x 63 <= 6000), none.  Both decided by the oracle's own histogram of the same chains."""
    c = CASES["sphere2_padding"]
    said = {}
    for npb in (600, 6000):
        ocfg = fresh_oracle(oracle, c)
        ocfg.iteration(oracle.MCMC, c["oname"], None, npb, 0, 3, 0, SEED, nchain=1)
        ohold = ocfg.hold_hist
        res = mci.integrate_sweep(c["f"], params=np.zeros((1, 0)), solver="mcmc", mcmc_chains=1, thermal_ratio=TR, var=c["var"](), dof=c["dof"],
                                  neval=3 * npb, block=3, niter=1, ignore=0, seed=SEED)[0]
        np.testing.assert_array_equal(res.holds, ohold)
        assert res.hold_max == hold_max(ohold) and res.chain_steps == npb and res.status == 0 and res.sweep_batched
        out = io.StringIO()
        mci.report(res, io=out)
        said[npb] = ":mcmc sweep point" in out.getvalue()
        print(npb, "hold_max", res.hold_max, "note", said[npb])
        assert said[npb] == (16 * hold_max(ohold) > npb) == (res.hold_note is not None)
    assert said == {600: True, 6000: False}
