"""GPU tests of carried chains in the chain solvers' sweeps (Engine.set_sweep_chain_carry, integrate_sweep_chains | integrate_sweep_mcmc(...,
carry=True); csrc/mci_sweep_chains.h chain_sweep<Cfg, MCMC, true>): a point's workgroup resamples the chains its last iteration stored to
the target train! and doReweight! have moved, block by block, and goes on with them -- against the oracle's carried iterations point by
point and iteration by iteration, against the uncarried sweep where carrying must not show, against the ordinary call with
set_chain_carry(1), and against itself under another assignment of points to workgroups.

Tolerances.  Iteration `it` against the oracle's: 1e-8 * 10^it (mean; tests/layout_cases.py check_carried_iterations: every train! in
between amplifies the rounding-level difference of the two maps by an order of magnitude) and 1e-5 * 10^it (error: the same bound widened
by the 1e3 that separates mean and error in the first-iteration checks, 1e-11 / 1e-8).  Final factors and maps, and later iterations of
runs whose maps went through different sums: those of test_hip_sweep_mcmc (1e-4 / 1e-2, maps 1e-4 of their range).

Bit-for-bit comparisons use at most 64 chains per block (test_hip_sweep_mcmc's note on one wave)."""
import math

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import CASES, SEED
from test_hip_sweep_leaves import bubble_row, check_map, oracle_config, unpack
from test_hip_sweep_mcmc import NAMES, ST_MCMC_INIT, TR, engine, rows, ud_array

pytestmark = pytest.mark.gpu
SOLVERS = ["vegasmc", "mcmc"]
SHAPES = [(700, 5, 7), (1500, 3, 300)]      # (nevalperblock, block, nchain): idle lanes | more chains than threads: a thread's stretch of the
                                            # resampling is two chains, and a lane runs a second chain
KEYS = ("iter_mean", "iter_std", "mean", "stdev", "maps", "reweight", "propose", "accept", "visited")
EXACT = {"sphere2_padding": np.array([math.pi / 4, math.pi / 6]), "discrete": np.array([6.0])}


def sweep(eng, solver, uds, **kw):
    if solver == "mcmc":
        return eng.integrate_sweep_mcmc("mcmc", userdata=ud_array(uds), thermal_ratio=TR, **kw)
    return eng.integrate_sweep_chains("vegasmc", userdata=ud_array(uds), **kw)


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, a[k], b[k])
    assert a["neval"] == b["neval"] and a["status"] == b["status"] and a["correlated"] == b["correlated"]
    if "holds" in a:
        np.testing.assert_array_equal(a["holds"], b["holds"])


def carried_oracle(oracle, c):
    ocfg = oracle_config(oracle, c)
    ocfg.set_chain_carry(1)
    ocfg.set_thermal_ratio(TR)
    return ocfg


@pytest.mark.parametrize("npb,block,nchain", SHAPES)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", NAMES)
def test_every_iteration_is_the_oracles_carried_iteration(oracle, name, solver, npb, block, nchain):
    """per point a fresh oracle config with set_chain_carry(1): iteration -> doReweight! -> train!, four times (the loop of
    check_carried_iterations), against the four log rows of the point"""
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    kw = dict(neval=npb * block, niter=4, block=block, seed=SEED, nchain=nchain)
    rs = sweep(eng, solver, uds, carry=True, **kw)
    plain = sweep(eng, solver, uds, **kw)
    assert eng.last_sweep_launch() == (2, 256) and eng.sweep_chain_carry() is False
    nobs, nd = eng.nobs, cfg.N + 1
    osolver = oracle.MCMC if solver == "mcmc" else oracle.VEGASMC
    for ud, r, q in zip(uds, rs, plain):
        ocfg = carried_oracle(oracle, c)
        neval = 0
        for it in range(4):
            packed = ocfg.iteration(osolver, c["oname"], ud or None, npb, 0, block, it, SEED, nchain=nchain)
            om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
            neval += int(packed[2 * nobs + 1])
            print(name, solver, nchain, "it", it, "mean", r["iter_mean"][it], om, "std", r["iter_std"][it], oe)
            np.testing.assert_allclose(r["iter_mean"][it], om, rtol=1e-8 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            np.testing.assert_allclose(r["iter_std"][it], oe, rtol=1e-5 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            ocfg.set_reweight(oracle.do_reweight(ocfg.reweight, packed[2 * nobs + 2:2 * nobs + 2 + nd]))
            ocfg.train()
        assert r["neval"] == neval and r["status"] == 0 and r["correlated"] is True
        if solver == "mcmc":
            assert r["neval"] < q["neval"], (r["neval"], q["neval"])      # no burn-in in the three carried iterations
            assert r["holds"].sum() == 4 * block * nchain and r["carried"] is True
        assert q["correlated"] is False
        np.testing.assert_allclose(r["reweight"], ocfg.reweight, rtol=1e-4)
        for l, (lf, parts) in enumerate(zip(c["oleaves"], unpack(c["oleaves"], r["maps"]))):
            if lf["kind"] == 0:
                check_map(parts[0], ocfg.grid(l), 1e-4)
            else:
                np.testing.assert_allclose(parts[1], ocfg.distribution(l), rtol=0, atol=1e-4)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["discrete", "sphere2_padding"])
def test_both_sides_of_the_resamplers_lds_limit_are_the_oracles_carried_iterations(oracle, name, solver, side):
    """A point's workgroup resamples in the front of its LDS segment, where the chain loop's carve is dead: the running weights of a block
    of up to lds_w = map_off - 256 stored chains sit there and the bisections read them, beyond that they read W in global memory
    (resample_block).  nchain = lds_w and lds_w + 1, the limit taken from the library (Engine.sweep_resample_lds), two blocks, chains of
    two steps; the body and the tolerances of test_every_iteration_is_the_oracles_carried_iteration.  `discrete` has the smallest map
    and with it the smallest limit, 144: fewer than the resampler's 256 threads, so either side is one chain per thread there.
    sphere2_padding's 4128 puts both sides at several chains per thread, and a lane of the chain loop runs 17 chains."""
    c, cfg, eng = engine(name, oracle)
    lds_w = eng.sweep_resample_lds()
    if name == "discrete":
        assert lds_w >= 2
    else:
        assert lds_w + 1 > 256                   # a thread's stretch of the resampling is several chains on either side
    nchain, block = lds_w + side, 2
    npb = 2 * nchain
    uds = rows(name, c)
    rs = sweep(eng, solver, uds, carry=True, neval=npb * block, niter=4, block=block, seed=SEED, nchain=nchain)
    assert eng.last_sweep_launch() == (2, 256)
    nobs, nd = eng.nobs, cfg.N + 1
    osolver = oracle.MCMC if solver == "mcmc" else oracle.VEGASMC
    for ud, r in zip(uds, rs):
        ocfg = carried_oracle(oracle, c)
        neval = 0
        for it in range(4):
            packed = ocfg.iteration(osolver, c["oname"], ud or None, npb, 0, block, it, SEED, nchain=nchain)
            om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
            neval += int(packed[2 * nobs + 1])
            print(name, solver, nchain, "it", it, "mean", r["iter_mean"][it], om, "std", r["iter_std"][it], oe)
            np.testing.assert_allclose(r["iter_mean"][it], om, rtol=1e-8 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            np.testing.assert_allclose(r["iter_std"][it], oe, rtol=1e-5 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            ocfg.set_reweight(oracle.do_reweight(ocfg.reweight, packed[2 * nobs + 2:2 * nobs + 2 + nd]))
            ocfg.train()
        assert r["neval"] == neval and r["status"] == 0 and r["correlated"] is True
        if solver == "mcmc":
            assert r["holds"].sum() == 4 * block * nchain and r["carried"] is True
        np.testing.assert_allclose(r["reweight"], ocfg.reweight, rtol=1e-4)
        for l, (lf, parts) in enumerate(zip(c["oleaves"], unpack(c["oleaves"], r["maps"]))):
            if lf["kind"] == 0:
                check_map(parts[0], ocfg.grid(l), 1e-4)
            else:
                np.testing.assert_allclose(parts[1], ocfg.distribution(l), rtol=0, atol=1e-4)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", NAMES)
def test_carrying_shows_where_it_must_and_nowhere_else(oracle, name, solver):
    c, cfg, eng = engine(name, oracle)
    uds = rows(name, c)
    kw = dict(neval=5 * 700, block=5, seed=SEED, nchain=7, ignore=0)
    both = lambda **k: (sweep(eng, solver, uds, carry=True, **dict(kw, **k)), sweep(eng, solver, uds, **dict(kw, **k)))
    for a, b in zip(*both(niter=1)):                          # a call's first iteration starts afresh
        same(a, b)
        assert a["correlated"] is False
    if solver == "vegasmc":
        for a, b in zip(*both(niter=2)):                      # not out of the iteration on the map before its first refinement
            same(a, b)
            assert a["correlated"] is False
        on, off = both(niter=3, adapt=False)                  # the map stays: carried from the second iteration on
    else:
        on, off = both(niter=3)
    for a, b in zip(on, off):
        assert a["iter_mean"][0].tobytes() == b["iter_mean"][0].tobytes() and a["iter_std"][0].tobytes() == b["iter_std"][0].tobytes()
        for it in (1, 2):
            assert np.all(a["iter_mean"][it] != b["iter_mean"][it]), (it, a["iter_mean"][it], b["iter_mean"][it])
        assert a["correlated"] is True and b["correlated"] is False and a["status"] == b["status"] == 0
    for a, b in zip(*both(niter=4, nchain=1)):                # one chain per block: nothing is ever carried
        same(a, b)
        assert a["correlated"] is False


def ordinary_engine(c, ud, name):
    cfg2 = mci.Configuration(var=c["var"](), dof=c["dof"], obs=c.get("obs"), seed=SEED)
    f = mci.Integrand(c["f"].body, ud, name) if ud else c["f"]
    eng = mci.Engine(cfg2, f, measure=c.get("measure"))
    eng.set_chain_carry(1)
    eng.set_chain_speculation(1)        # one lane per chain
    return eng


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name,nchain", [("bubble", 16), ("sphere2_padding", 64), ("discrete", 7)])
def test_a_carried_sweep_of_one_point_equals_the_ordinary_call(oracle, name, nchain, solver):
    c, cfg, eng = engine(name, oracle)
    ud = rows(name, c, 1)[0]
    kw = dict(neval=16 * 1000, niter=4, block=16, seed=SEED, nchain=nchain)
    r = sweep(eng, solver, [ud], carry=True, **kw)[0]
    ordinary = ordinary_engine(c, ud, name)
    q = ordinary.integrate(solver, **dict(kw, **({"thermal_ratio": TR} if solver == "mcmc" else {})))
    assert ordinary.last_chain_launch() == (nchain, True) and q["correlated"] and r["correlated"] is True
    print(name, solver, nchain, "sweep", r["iter_mean"], r["stdev"], "ordinary", q["iter_mean"], q["stdev"])
    np.testing.assert_allclose(r["iter_mean"][0], q["iter_mean"][0], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"][0], q["iter_std"][0], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-4, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-2, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-4)
    np.testing.assert_allclose(r["stdev"], q["stdev"], rtol=1e-2)          # the block-lineage error on both sides
    np.testing.assert_allclose(r["reweight"], ordinary.reweight(), rtol=1e-4)
    assert r["neval"] == q["neval"]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("bad", [None, "zero", "nan"])
def test_nothing_leaks_from_point_to_point(oracle, solver, bad):
    """one workgroup runs A, B, C one after another, then two workgroups run A, C | B: whatever a point left in LDS or in its stored
    chains, picks and weights would show in the point behind it.  bad: B's integrand is zero (:mcmc: ST_MCMC_INIT in B's own status word)
    or NaN -- in nobody else's bytes"""
    A, B, C_ = (bubble_row(0.3 * k) for k in range(3))
    if bad == "zero":
        B = B[:3] + [0.0] + B[4:]
    elif bad == "nan":
        B = [float("nan")] + B[1:]
    c, cfg, eng = engine("bubble", oracle)
    kw = dict(neval=5 * 700, niter=4, block=5, seed=SEED, nchain=7, carry=True)
    eng.sweep_workgroups(1)
    one = sweep(eng, solver, [A, B, C_], **kw)
    assert eng.last_sweep_launch()[0] == 1
    eng.sweep_workgroups(2)
    two = sweep(eng, solver, [A, B, C_], **kw)
    assert eng.last_sweep_launch()[0] == 2
    eng.sweep_workgroups(0)
    alone = sweep(eng, solver, [A, C_], **kw)
    for k in (0, 2):
        same(one[k], two[k])
        same(one[k], alone[k // 2])
        assert one[k]["status"] == 0 and one[k]["correlated"] is True and np.all(np.isfinite(one[k]["mean"]))
    print(solver, bad, "status of B", one[1]["status"], "mean", one[1]["mean"])
    if bad is None:
        same(one[1], two[1])
        assert one[1]["status"] == 0
    elif bad == "zero" and solver == "mcmc":
        assert one[1]["status"] & ST_MCMC_INIT
    elif bad == "nan":
        assert not np.all(np.isfinite(one[1]["iter_mean"]))
    assert one[0]["reweight"].tobytes() != one[2]["reweight"].tobytes() or one[0]["maps"].tobytes() != one[2]["maps"].tobytes()


@pytest.mark.parametrize("solver", SOLVERS)
def test_seeds_are_per_point_and_the_engines_own_state_is_untouched(oracle, solver):
    c, cfg, eng = engine("sphere2_padding", oracle)
    tr = {"thermal_ratio": TR} if solver == "mcmc" else {}
    eng.set_chain_carry(1)
    eng.set_chain_speculation(1)
    eng.integrate(solver, neval=4 * 500, niter=3, block=4, seed=SEED, nchain=4, **tr)      # (a state worth keeping: map, factors, stored chains)
    grid, rw, packed, last = eng.grid(0).copy(), eng.reweight().copy(), eng.get_packed().copy(), eng.last_chain_launch()
    assert last == (4, True)
    s0, s1 = SEED, 777
    kw = dict(neval=5 * 700, niter=3, block=5, nchain=7, carry=True)
    rs = sweep(eng, solver, [[], []], seeds=[s0, s1], **kw)
    for s, r in zip((s0, s1), rs):
        same(r, sweep(eng, solver, [[]], seed=s, **kw)[0])
        assert r["correlated"] is True
    assert rs[0]["iter_mean"][0][0] != rs[1]["iter_mean"][0][0] and rs[0]["iter_mean"][2][0] != rs[1]["iter_mean"][2][0]
    assert eng.grid(0).tobytes() == grid.tobytes() and eng.reweight().tobytes() == rw.tobytes() and eng.get_packed().tobytes() == packed.tobytes()
    assert eng.last_chain_launch() == last and eng.sweep_chain_carry() is False
    # ... and the engine's own stored chains: its next iteration continues them as if no sweep had run
    twin = engine("sphere2_padding", oracle)[2]
    twin.set_chain_carry(1)
    twin.set_chain_speculation(1)
    twin.integrate(solver, neval=4 * 500, niter=3, block=4, seed=SEED, nchain=4, **tr)
    a = eng.iteration(solver, 500, 0, 4, iteration=3, seed=SEED, nchain=4, **tr)
    b = twin.iteration(solver, 500, 0, 4, iteration=3, seed=SEED, nchain=4, **tr)
    assert eng.last_chain_launch() == twin.last_chain_launch() == (4, True) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["sphere2_padding", "discrete"])
def test_known_answers_within_the_references_seven_sigma(oracle, name, solver):
    """test/runtests.jl:4-9 on the carried sweeps' final means, with the reported block-lineage error"""
    c, cfg, eng = engine(name, oracle)
    rs = sweep(eng, solver, [[], []], seeds=[SEED, SEED + 1], neval=16 * 1000, niter=4, block=16, nchain=16, carry=True)
    for r in rs:
        print(name, solver, r["mean"], "+-", r["stdev"], "exact", EXACT[name])
        assert r["correlated"] is True and r["status"] == 0 and np.all(r["stdev"] > 0)
        assert np.all(np.abs(r["mean"] - EXACT[name]) < 7.0 * r["stdev"]), (r["mean"], r["stdev"])
