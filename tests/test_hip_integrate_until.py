"""GPU tests of integrate() with a target error (mci_integrate_until): the persistent :vegas launch that stops itself
(csrc/mci_persist_until.h) and the launch chain with the host's rule between its launches (csrc/mci_host_integrate.h), for all three
solvers and stratified :vegas.

Where a call must stop is formed on the CPU: the oracle's loop for plain :vegas (tests/until_cases.py oracle_heads / reference_stops,
with the recorded inputs that keep every decision 5 % from its threshold), the oracle's VEGAS+ iteration for the stratified call, the
oracle's chain iterations for the chain solvers while they are uncorrelated.  For a correlated call the rule reads the block-lineage
error, which is made of every block's mean of every iteration; the oracle hands out an iteration's merged head only, so there the
lineage formula of include/mci.h is written out in numpy over the block means of the FIXED call on a fresh engine -- whose rows are held
to the oracle's carried iterations first.  Every expected stop asserts its own margin (no decision within 5 % of its threshold) before
anything is compared; nothing is skipped.

A stopped call is held to the fixed call with niter = niter_run on a fresh engine.  Tolerances: two calls of the same path differ by the
order of the histogram atomics alone -- 1e-6 on the means, what tests/test_hip_persistent.py holds two persistent runs to, 1e-4 on the
errors (its factor 100 between the two), maps 1e-6 of their range; the persistent launch against the launch chain 1e-4 / 1e-2 / 1e-4 of
the range (test_persistent_launch_and_launch_chain_give_the_same_run); chain solvers 1e-4 / 1e-2 (tests/test_hip_sweep_carry.py, runs
whose maps went through different sums); deterministic mode bit for bit."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
from until_cases import CASES, KW, MARGIN, SEED, TWO_BODY, oracle_heads, reference_stops, row, two_row

pytestmark = pytest.mark.gpu
NITER = KW["niter"]


def genz_engine(ud, **kw):
    from test_hip_sweep import engine
    cfg, eng = engine(ud)
    return eng if not kw else mci.Engine(cfg, eng.integrand, **kw)


def two_engine(ud, **kw):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [2]], seed=SEED)
    return mci.Engine(cfg, mci.Integrand(TWO_BODY, list(ud), "until_two"), **kw)


def mixed_engine(ud, **kw):
    from test_hip_sweep_leaves import MIXED_BODY
    cfg = mci.Configuration(var=(mci.Continuous(0.0, 1.0, ninc=65, alpha=1.5), mci.Continuous(0.0, 2.0, alpha=2.0), mci.Discrete(1, 7)),
                            dof=[[1, 1, 1]], seed=SEED)
    return mci.Engine(cfg, mci.Integrand(MIXED_BODY, list(ud), "mixed"), **kw)


ENGINES = {"genz": genz_engine, "two_columns": two_engine, "mixed": mixed_engine}


def oracle_stop(oracle, case, k):
    """(stop, margin) of scan point k as an ordinary call: an ordinary call on a fresh configuration IS the sweep point's call"""
    c = CASES[case]
    heads = oracle_heads(oracle, case, k)
    nobs = heads.shape[1] // 2
    ms = [oracle.mean_std(h[:nobs], h[nobs:], KW["block"]) for h in heads]
    stop, margin = reference_stops(oracle, np.array([m for m, _ in ms]), np.array([e for _, e in ms]), c["rtol"], c["atol"], ignore=1)
    print("%s k = %d: oracle stop %s, nearest decision %.1f %% from its threshold" % (case, k, stop or "none", 100 * margin))
    assert margin >= MARGIN, (case, k, margin)
    return stop


def grids(eng):
    return [eng.grid(i) if hasattr(lf, "ninc") else eng.distribution(i)[0] for i, lf in enumerate(eng.config.leaves)]


def check_same_run(r, q, maps_r, maps_q, n, mean=1e-6, std=1e-4, grid=1e-6):
    assert r["iter_mean"].shape[0] == n == q["iter_mean"].shape[0]
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=mean, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=std, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=mean)
    np.testing.assert_allclose(r["stdev"], q["stdev"], rtol=std)
    assert r["neval"] == q["neval"] and r["correlated"] == q["correlated"]
    np.testing.assert_array_equal(r["visited"], q["visited"])
    for g, og in zip(maps_r, maps_q):
        np.testing.assert_allclose(g, og, rtol=0, atol=grid * max(og[-1] - og[0], 1.0))


# ---- 1. the persistent launch ------------------------------------------------------------------------------------------------------------

def persistent_point(oracle, case, k, want, niter=NITER):
    c = CASES[case]
    stop = oracle_stop(oracle, case, k)
    assert stop == want
    if stop > niter:
        stop = 0
    kw = dict(KW, niter=niter, seed=SEED)
    eng = ENGINES[case](row(case, k))
    eng.set_persistent("on")
    r = eng.integrate("vegas", target=(c["rtol"], c["atol"], 0), **kw)
    assert eng.last_integrate_persistent()
    n = r["niter_run"]
    print("%s k = %d: niter_run %d converged %s discarded %d" % (case, k, n, r["converged"], r["neval_discarded"]))
    assert n == (stop or niter) and r["converged"] == (stop != 0)
    assert r["neval"] == n * KW["neval"] and r["neval_discarded"] == (KW["neval"] if n < niter else 0)
    assert eng.code_object("vegas_persistent_until") != ""
    fixed = ENGINES[case](row(case, k))
    fixed.set_persistent("on")
    q = fixed.integrate("vegas", **dict(kw, niter=n))
    assert fixed.last_integrate_persistent()
    check_same_run(r, q, grids(eng), grids(fixed), n)
    np.testing.assert_allclose(eng.iteration_log(n), fixed.iteration_log(n), rtol=1e-4, atol=1e-300)     # the log holds n rows, the last of them row n
    # the counters: the next persistent launch on the SAME engine neither stalls nor fails, and continues like the launch chain does
    r2 = eng.integrate("vegas", first_iteration=n, **dict(kw, niter=3))
    assert eng.last_integrate_persistent()
    eng.check_status()
    chain = ENGINES[case](row(case, k))
    chain.set_persistent("off")
    chain.integrate("vegas", **dict(kw, niter=n))
    q2 = chain.integrate("vegas", first_iteration=n, **dict(kw, niter=3))
    assert not chain.last_integrate_persistent()
    check_same_run(r2, q2, grids(eng), grids(chain), 3, mean=1e-4, std=1e-2, grid=1e-4)


@pytest.mark.parametrize("k,want", list(zip(CASES["genz"]["ks"], CASES["genz"]["stops"])))
def test_persistent_genz_points_stop_where_the_oracle_says(oracle, k, want):
    """stops 3 (the first checkable turn, ignore + 2), 0 (never: niter_run = niter, not converged), 3, 5, 4"""
    persistent_point(oracle, "genz", k, want)


@pytest.mark.parametrize("k,want", list(zip(CASES["two_columns"]["ks"], CASES["two_columns"]["stops"])))
def test_persistent_two_column_points_stop_where_the_oracle_says(oracle, k, want):
    persistent_point(oracle, "two_columns", k, want)


def test_a_persistent_call_that_converges_in_its_last_turn(oracle):
    """genz k = 4 stops at 5: with niter = 5 that is the last turn -- nothing is discarded, converged is true, the counters are the fixed
    launch's; with niter = 4 it is not reached"""
    persistent_point(oracle, "genz", 4, 5, niter=5)
    persistent_point(oracle, "genz", 4, 5, niter=4)


def test_a_zero_target_on_the_persistent_launch_is_the_fixed_call(oracle):
    eng, fixed = genz_engine(row("genz", 0)), genz_engine(row("genz", 0))
    for e in (eng, fixed):
        e.set_persistent("on")
    r = eng.integrate("vegas", seed=SEED, target=(0.0, 0.0, 0), **KW)
    q = fixed.integrate("vegas", seed=SEED, **KW)
    assert eng.last_integrate_persistent() and r["niter_run"] == NITER and r["converged"] is False and r["neval_discarded"] == 0
    check_same_run(r, q, grids(eng), grids(fixed), NITER)
    r = eng.integrate("vegas", seed=SEED, first_iteration=NITER, target=(1.0, 0.0, 7), **KW)        # min_niter holds a loose target back
    assert eng.last_integrate_persistent() and r["niter_run"] == 7 and r["converged"] is True


# ---- 2. the launch chain, :vegas -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,want", list(zip(CASES["mixed"]["ks"], CASES["mixed"]["stops"])))
def test_launch_chain_points_of_several_leaves_stop_where_the_oracle_says(oracle, k, want):
    c = CASES["mixed"]
    assert oracle_stop(oracle, "mixed", k) == want
    eng, fixed = mixed_engine(row("mixed", k)), mixed_engine(row("mixed", k))
    eng.set_persistent("on")                                     # (several leaves: never persistent, whatever is asked)
    r = eng.integrate("vegas", seed=SEED, target=(c["rtol"], c["atol"], 0), **KW)
    assert not eng.last_integrate_persistent()
    assert r["niter_run"] == want and r["converged"] is True and r["neval"] == want * KW["neval"] and r["neval_discarded"] == 0
    q = fixed.integrate("vegas", seed=SEED, **dict(KW, niter=want))
    check_same_run(r, q, grids(eng), grids(fixed), want)


def test_a_deterministic_call_stops_on_the_fixed_calls_bytes(oracle):
    c = CASES["genz"]
    k, want = 6, 4
    assert oracle_stop(oracle, "genz", k) == want
    eng, fixed = genz_engine(row("genz", k), deterministic=True), genz_engine(row("genz", k), deterministic=True)
    r = eng.integrate("vegas", seed=SEED, target=(c["rtol"], c["atol"], 0), **KW)
    assert not eng.last_integrate_persistent() and r["niter_run"] == want and r["converged"] is True
    q = fixed.integrate("vegas", seed=SEED, **dict(KW, niter=want))
    for key in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited"):
        assert np.asarray(r[key]).tobytes() == np.asarray(q[key]).tobytes(), key
    assert eng.grid(0).tobytes() == fixed.grid(0).tobytes()
    assert eng.iteration_log(want).tobytes() == fixed.iteration_log(want).tobytes()


STRAT = dict(k=0, nstrat=[4, 4, 4, 4], beta=0.75, rtol=4.6e-4)


def test_a_stratified_call_stops_where_the_vegas_plus_oracle_says(oracle):
    """genz k = 0 on 4^4 hypercubes: the CPU oracle's free-running VEGAS+ loop (allocation from its own d_h, its own train!) gives the
    rows; rtol was chosen on them so that iteration 3 is 17 % above the threshold and iteration 4 15 % below"""
    from test_hip_sweep import ocont
    ud, N, nstrat = row("genz", STRAT["k"]), KW["neval"], STRAT["nstrat"]
    ocfg = oracle.Config([ocont()], [[4]])
    off = oracle.Config.strat_alloc(np.ones(int(np.prod(nstrat))), N, True)
    im, ie = [], []
    for it in range(NITER):
        o = ocfg.strat_iteration("genz_product_peak", ud, SEED, it, 0, nstrat, off, STRAT["beta"])
        ocfg.train()
        im.append(o["mean"].copy())
        ie.append(np.sqrt(o["var"]))
        off = oracle.Config.strat_alloc(o["d"], N)
    want, margin = reference_stops(oracle, np.array(im), np.array(ie), STRAT["rtol"], 0.0, ignore=1)
    print("stratified: oracle stop %s, nearest decision %.1f %% from its threshold" % (want or "none", 100 * margin))
    assert margin >= MARGIN and 3 <= want < NITER, (want, margin)
    eng, fixed = genz_engine(ud), genz_engine(ud)
    for e in (eng, fixed):
        e.set_stratification(nstrat=nstrat, beta=STRAT["beta"])
    r = eng.integrate("vegas", seed=SEED, target=(STRAT["rtol"], 0.0, 0), **KW)
    print("stratified: niter_run %d, rows" % r["niter_run"], r["iter_mean"].ravel(), r["iter_std"].ravel(), "oracle", np.ravel(im), np.ravel(ie))
    assert r["niter_run"] == want and r["converged"] is True and not eng.last_integrate_persistent()
    q = fixed.integrate("vegas", seed=SEED, **dict(KW, niter=want))
    check_same_run(r, q, grids(eng), grids(fixed), want)
    np.testing.assert_array_equal(eng.strat_counts(), fixed.strat_counts())      # the allocation is left as the fixed call leaves it


# ---- 3. the chain solvers ------------------------------------------------------------------------------------------------------------------

CHAIN_K = 1
# nchain = 1 (uncorrelated: the plain rule), chosen on the oracle's rows: :vegasmc -- column 0's relative error is 10 % above rtol at n = 4
# and 11 % below at n = 5, column 1's absolute error 12 % above atol at n = 4 and 9 % below at n = 5; :mcmc -- column 0 12 % above at
# n = 3, 10 % below at n = 4, column 1 34 % above and 24 % below.
# nchain = 4 (correlated: the lineage rule), chosen on the fixed call's block means (the test prints both error sequences): :vegasmc --
# column 0 decides: its lineage error is 15 % above rtol at n = 3 and 8 % below at n = 4, where the plain error is still 8 % above (6.5 %
# below at n = 5); :mcmc -- column 1 decides: its lineage error is 52 % above atol at n = 3 and 11 % below at n = 4, where the plain
# error is still 12 % above (10 % below at n = 5); the other column is through from n = 3 on either way
CHAIN_TARGETS = {("vegasmc", 1): (2.8e-3, 9.7e-4), ("mcmc", 1): (3.7e-2, 4.3e-3), ("vegasmc", 4): (3.1e-3, 1.3e-3), ("mcmc", 4): (5.0e-2, 3.75e-3)}


def lineage_errors(block_mean, iter_std, ignore, block):
    """E [niter][nobs] of the block-lineage formula (include/mci.h mci_lineage_sums -> mci_mean_std), written out: block b's lineage is
    its weighted average over iterations ignore + 1 .. n with the weights 1 / (s_i + 1e-10)^2 of average(); E = the scatter of the
    lineages' mean, sqrt((sum m_b^2 / B - mean^2) / (B - 1))"""
    bm, ie = np.asarray(block_mean), np.asarray(iter_std)
    niter, B, nobs = bm.shape
    assert B == block
    E = np.full((niter, nobs), np.nan)
    for n in range(ignore + 2, niter + 1):
        w = 1.0 / (ie[ignore:n] + 1.0e-10) ** 2                  # [n - ignore][nobs]
        mb = (bm[ignore:n] * (w / w.sum(0))[:, None, :]).sum(0)   # [B][nobs]
        m = mb.sum(0) / B
        v = ((mb * mb).sum(0) / B - m * m) / (B - 1)
        E[n - 1] = np.sqrt(np.maximum(v, 0.0))
    return E


def stops_of(oracle, im, ie, E, rtol, atol, ignore=1):
    """(stop, margin) with the errors E [niter][nobs] in the place of average()'s (None: average()'s own)"""
    niter, nobs = im.shape
    margin, stop = np.inf, 0
    for n in range(ignore + 2, niter + 1):
        done = True
        for o in range(nobs):
            M, e, _ = oracle.average(im[:, o], ie[:, o], init=ignore + 1, max=n)
            if E is not None:
                e = E[n - 1, o]
            bound = max(atol, rtol * abs(M))
            margin = min(margin, abs(e / bound - 1.0))
            done = done and e <= bound
        if done:
            stop = n
            break
    return stop, margin


def oracle_chain_rows(oracle, solver, nchain, ud):
    from test_hip_sweep import ocont
    f = oracle.compile_c_integrand(TWO_BODY, 2, "until_two")
    ocfg = oracle.Config([ocont()], [[2], [2]])
    ocfg.set_thermal_ratio(0.1)
    nobs, nd, block = int(ocfg.c.nobs), 3, KW["block"]
    im, ie = [], []
    for it in range(NITER):
        packed = ocfg.iteration(oracle.MCMC if solver == "mcmc" else oracle.VEGASMC, f, ud, KW["neval"] // block, 0, block, it, SEED, nchain=nchain)
        m, e = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
        im.append(m)
        ie.append(e)
        ocfg.set_reweight(oracle.do_reweight(ocfg.reweight, packed[2 * nobs + 2:2 * nobs + 2 + nd]))
        ocfg.train()
    return np.array(im), np.array(ie)


@pytest.mark.parametrize("nchain", [1, 4])
@pytest.mark.parametrize("solver", ["vegasmc", "mcmc"])
def test_chain_solvers_stop_by_the_error_their_result_reports(oracle, solver, nchain):
    ud = two_row(CHAIN_K)
    rtol, atol = CHAIN_TARGETS[(solver, nchain)]
    kw = dict(KW, seed=SEED, nchain=nchain)
    om, oe = oracle_chain_rows(oracle, solver, nchain, ud)
    fixed10 = two_engine(ud)
    q10 = fixed10.integrate(solver, **kw)
    # the fixed call's rows are the oracle's carried (nchain = 4) | afresh (nchain = 1) iterations
    for it in range(4):
        np.testing.assert_allclose(q10["iter_mean"][it], om[it], rtol=1e-8 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
        np.testing.assert_allclose(q10["iter_std"][it], oe[it], rtol=1e-5 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
    plain, pmargin = stops_of(oracle, om, oe, None, rtol, atol)
    assert q10["correlated"] == (nchain > 1)
    if nchain == 1:
        want, margin = plain, pmargin
        print("%s nchain 1: plain rule stops at %s, margin %.1f %%" % (solver, want or "none", 100 * margin))
    else:
        E = lineage_errors(q10["block_mean"], q10["iter_std"], 1, KW["block"])
        np.testing.assert_allclose(E[-1], q10["stdev"], rtol=1e-10)                 # (the formula as written IS what the library reports)
        want, margin = stops_of(oracle, q10["iter_mean"], q10["iter_std"], E, rtol, atol)
        plain, pmargin = stops_of(oracle, q10["iter_mean"], q10["iter_std"], None, rtol, atol)
        P = np.array([[oracle.average(q10["iter_mean"][:, o], q10["iter_std"][:, o], init=2, max=n)[:2] for o in range(2)] for n in range(3, NITER + 1)])
        print("%s nchain 4, n = 3 ..: lineage E / |M| of column 0" % solver, E[2:, 0] / np.abs(P[:, 0, 0]), "plain", P[:, 0, 1] / np.abs(P[:, 0, 0]))
        print("%s nchain 4, n = 3 ..: lineage E of column 1" % solver, E[2:, 1], "plain", P[:, 1, 1])
        print("%s nchain 4: lineage rule stops at %s (margin %.1f %%), the plain rule would at %s (margin %.1f %%)"
              % (solver, want or "none", 100 * margin, plain or "none", 100 * pmargin))
        assert pmargin >= MARGIN and want != plain                                  # the proof of which error the rule reads
    assert margin >= MARGIN and 3 <= want < NITER, (want, margin)
    eng = two_engine(ud)
    r = eng.integrate(solver, target=(rtol, atol, 0), **kw)
    print("%s nchain %d: niter_run %d correlated %s" % (solver, nchain, r["niter_run"], r["correlated"]))
    assert r["niter_run"] == want and r["converged"] is True and r["correlated"] == (nchain > 1)
    fixed = two_engine(ud)
    q = fixed.integrate(solver, **dict(kw, niter=want))
    check_same_run(r, q, grids(eng), grids(fixed), want, mean=1e-4, std=1e-2, grid=1e-4)
    np.testing.assert_allclose(eng.reweight(), fixed.reweight(), rtol=1e-4)
    if nchain > 1:
        np.testing.assert_allclose(r["block_mean"], q["block_mean"], rtol=1e-4, atol=1e-12)


# ---- 4. continuation, through the public call ------------------------------------------------------------------------------------------------

def test_a_stopped_call_is_continued_on_the_next_iteration_indices(oracle):
    from test_hip_sweep import genz
    c, k, want = CASES["genz"], 6, 4
    assert oracle_stop(oracle, "genz", k) == want
    mk = lambda: mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]], seed=SEED)
    cfg = mk()
    kw = dict(solver="vegas", neval=KW["neval"], block=KW["block"])
    res = mci.integrate(genz(row("genz", k)), config=cfg, niter=NITER, rtol=c["rtol"], atol=c["atol"], **kw)
    assert res.niter_run == want and res.converged is True and cfg.iterations_done == want
    assert res.neval == want * KW["neval"] and len(res.iterations) == want
    more = mci.integrate(genz(row("genz", k)), config=res.config, niter=2, **kw)
    assert cfg.iterations_done == want + 2 and more.niter_run is None and more.converged is None
    whole = mci.integrate(genz(row("genz", k)), config=mk(), niter=want + 2, **kw)
    assert np.asarray(res.iter_mean).shape[0] == want and np.asarray(more.iter_mean).shape[0] == 2
    np.testing.assert_allclose(np.concatenate([res.iter_mean, more.iter_mean]), whole.iter_mean, rtol=1e-6)
    np.testing.assert_allclose(np.concatenate([res.iter_std, more.iter_std]), whole.iter_std, rtol=1e-4)
    never = mci.integrate(genz(row("genz", 1)), config=mk(), niter=NITER, rtol=c["rtol"], **kw)          # k = 1 never gets there
    assert never.niter_run == NITER and never.converged is False and never.config.iterations_done == NITER
    import io
    out = io.StringIO()
    mci.report(never, io=out)
    assert "ran all 10 iterations it was given without reaching its target error" in out.getvalue()


# ---- 5. a stalled persistent launch --------------------------------------------------------------------------------------------------------

def test_a_stalled_persistent_launch_with_a_target_falls_back_to_the_launch_chain(oracle):
    """the spin-tick hook of csrc/mci_debug.h, as tests/test_hip_persistent.py uses it: the launch gives up, the map is restored, and the
    call -- target and all -- runs through the launch chain, with the launch chain's answer"""
    from mcintegration_jl_amd._lib import check, lib
    c, k, want = CASES["genz"], 6, 4
    assert oracle_stop(oracle, "genz", k) == want
    eng = genz_engine(row("genz", k))
    eng.set_persistent("on")
    check(lib().mci_debug_persist_spin_ticks(eng.p, 1))
    r = eng.integrate("vegas", seed=SEED, target=(c["rtol"], c["atol"], 0), **KW)
    assert not eng.last_integrate_persistent() and r["niter_run"] == want and r["converged"] is True and r["neval_discarded"] == 0
    chain = genz_engine(row("genz", k))
    chain.set_persistent("off")
    q = chain.integrate("vegas", seed=SEED, target=(c["rtol"], c["atol"], 0), **KW)
    assert q["niter_run"] == want
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-9)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-6)
    np.testing.assert_allclose(eng.grid(0), chain.grid(0), rtol=0, atol=1e-9)
    check(lib().mci_debug_persist_spin_ticks(eng.p, 200000000))
    r2 = eng.integrate("vegas", seed=SEED, first_iteration=want, target=(0.0, 0.0, 0), **dict(KW, niter=3))   # later calls: the launch chain
    assert not eng.last_integrate_persistent() and r2["niter_run"] == 3
    eng.check_status()
