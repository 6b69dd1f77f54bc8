"""GPU tests of the carried VEGAS+ allocation (mci_set_stratification_carry, k_strat_remap, MCISTATE version 2): a call that starts
from the d_h the last one measured -- on the same plan, at another N, on another plan or beta (remapped), frozen with adapt=False,
across a state file --, that carry off is the behaviour it was, determinism, and what it buys on the Watson integral.

Expected allocations are the oracle's (mcio_strat_alloc) of the d_h the run started from; they are compared under the rule of
tests/test_hip_stratified_parity.py (restated here): sum = N, min >= 2, |delta n_h| <= 1 on at most max(2, ncube / 1000) hypercubes --
the kernel's prefix sums are formed in another order than the oracle's, so a floor() may land one sample to either side."""
import math
import os
import struct

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_stratified import WATSON, watson_cfg
from test_strat_carry_host import PAIRS_3D, remap_numpy

pytestmark = pytest.mark.gpu
SEED = 20240229
N0, BLOCK = 16384, 4
PLAN = (5, 1, 3)
HOW_UNIFORM, HOW_SAME, HOW_REMAPPED = 0, 1, 2


def check_alloc(counts, want, N, what):
    nc = counts.size
    assert counts.sum() == N and counts.min() >= 2, what
    delta = np.abs(counts - want)
    bad = np.flatnonzero(delta)
    assert delta.max() <= 1 and bad.size <= max(2, nc // 1000), (what, "first hypercube that differs", bad[:1], counts[bad[:5]], want[bad[:5]], bad.size)


def sphere_cfg():
    return mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED)


def sphere_engine(nstrat=PLAN, beta=0.75, carry=True, **kw):
    eng = mci.Engine(sphere_cfg(), mci.catalog.sphere2(), **kw)
    eng.set_stratification(nstrat=list(nstrat), beta=beta, carry=carry)
    return eng


def x2y2_engine(nstrat, carry=True):
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED), mci.catalog.x2y2())
    eng.set_stratification(nstrat=list(nstrat), carry=carry)
    return eng


def alloc(oracle, d, N):
    return np.diff(oracle.Config.strat_alloc(d, N, False))


def uniform(oracle, ncube, N):
    return np.diff(oracle.Config.strat_alloc(np.ones(ncube), N, True))


def train(eng, N=N0, niter=3, block=BLOCK):
    """a training call; the d_h its last iteration measured"""
    eng.integrate("vegas", N, niter=niter, block=block, seed=SEED)
    d = eng.strat_d()
    assert d.max() > 0
    return d


# ---- 1, 2: the same plan ------------------------------------------------------------------------------------------------------------

def test_same_plan_same_n(oracle):
    eng = sphere_engine()
    d = train(eng)
    assert eng.strat_carry() == (True, HOW_UNIFORM)          # the training call itself had nothing to start from
    start = eng.strat_start_d_next(15)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    counts = eng.strat_counts()
    assert np.array_equal(start, d)                          # the values the allocation was made from: the carried ones, bit for bit
    check_alloc(counts, alloc(oracle, d, N0), N0, "same plan, same N")
    assert np.abs(counts - uniform(oracle, 15, N0)).max() > 1
    assert eng.strat_carry() == (True, HOW_SAME)
    info = eng.stratification()
    assert info["carry"] is True and info["carried"] == "same plan" and info["nstrat"] == list(PLAN)
    eng.close()


def test_same_plan_other_n(oracle):
    eng = sphere_engine()
    d = train(eng)
    eng.integrate("vegas", 4 * N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    counts = eng.strat_counts()
    check_alloc(counts, alloc(oracle, d, 4 * N0), 4 * N0, "same plan, 4 N")
    assert np.abs(counts - uniform(oracle, 15, 4 * N0)).max() > 1 and eng.strat_carry() == (True, HOW_SAME)
    # N = 2 ncube: two samples each, nothing left to move
    eng.integrate("vegas", 30, niter=1, block=1, seed=SEED, first_iteration=4)
    assert np.array_equal(eng.strat_counts(), np.full(15, 2)) and eng.strat_carry() == (True, HOW_SAME)
    d30 = eng.strat_d()
    with pytest.raises(mci.MCIError, match="need at least"):
        eng.integrate("vegas", 28, niter=1, block=1, seed=SEED, first_iteration=5)
    # (the refusal took nothing away: the next call starts from the d_h of the N = 30 iteration)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=5)
    check_alloc(eng.strat_counts(), alloc(oracle, d30, N0), N0, "after the refusal")
    eng.close()


# ---- 3: another plan, another beta ---------------------------------------------------------------------------------------------------

def remap_case(oracle, eng, plan_a, plan_b, N, what):
    d_a = train(eng, N)
    nb = int(np.prod(plan_b))
    eng.set_stratification(nstrat=list(plan_b), carry=True)
    start = eng.strat_start_d_next(nb)
    eng.integrate("vegas", N, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    want_d = remap_numpy(d_a, plan_a, plan_b)
    assert np.array_equal(start, want_d), what               # e = 1: the old values, bit for bit
    counts = eng.strat_counts()
    assert counts.size == nb
    check_alloc(counts, alloc(oracle, want_d, N), N, what)
    return counts


@pytest.mark.parametrize("plan_a,plan_b", PAIRS_3D, ids=["refine", "coarsen", "non_nested", "identity"])
def test_remap_three_draws(oracle, plan_a, plan_b):
    eng = sphere_engine(plan_a)
    remap_case(oracle, eng, plan_a, plan_b, N0, "%s -> %s" % (plan_a, plan_b))
    # (the identity pair under the same beta is no remap: it is the carried d_h on its own plan, and the kernel does not run)
    assert eng.strat_carry() == (True, HOW_SAME if plan_a == plan_b else HOW_REMAPPED)
    assert eng.stratification()["nstrat"] == list(plan_b)
    eng.close()


def test_remap_two_draws_several_tiles(oracle):
    """(40, 40) -> (64, 50): 3200 new hypercubes -- several tiles of k_strat_alloc, more than one workgroup of k_strat_remap"""
    eng = x2y2_engine((40, 40))
    counts = remap_case(oracle, eng, (40, 40), (64, 50), N0, "(40, 40) -> (64, 50)")
    assert counts.size == 3200 > 256 and eng.strat_carry() == (True, HOW_REMAPPED)
    eng.close()


def test_beta_change_on_the_identity_plan(oracle):
    eng = sphere_engine(beta=0.75)
    d = train(eng)
    eng.set_stratification(nstrat=list(PLAN), beta=0.5, carry=True)
    start = eng.strat_start_d_next(15)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    want_d = d ** (0.5 / 0.75)
    np.testing.assert_allclose(start, want_d, rtol=1e-14, atol=0)
    check_alloc(eng.strat_counts(), alloc(oracle, start, N0), N0, "beta 0.75 -> 0.5")
    check_alloc(eng.strat_counts(), alloc(oracle, want_d, N0), N0, "beta 0.75 -> 0.5 (numpy's powers)")
    assert eng.strat_carry() == (True, HOW_REMAPPED) and eng.stratification()["beta"] == 0.5
    # beta = 0 on either side starts uniform: an even allocation is asked for | nothing was learned
    eng.set_stratification(nstrat=list(PLAN), beta=0.0, carry=True)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=4)
    assert np.array_equal(eng.strat_counts(), uniform(oracle, 15, N0)) and eng.strat_carry() == (True, HOW_UNIFORM)
    eng.set_stratification(nstrat=list(PLAN), beta=0.75, carry=True)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=5)
    assert np.array_equal(eng.strat_counts(), uniform(oracle, 15, N0)) and eng.strat_carry() == (True, HOW_UNIFORM)
    eng.close()


def test_default_plans_through_integrate(oracle):
    """the README's resume idiom: config=res.config at a larger neval -- another default plan, the carried d_h moved onto it"""
    f = mci.catalog.sphere2()
    res = mci.integrate(f, config=sphere_cfg(), solver="vegas", neval=16384, niter=3, stratify=mci.Stratify(carry=True))
    eng = res.config._engine
    plan_a, d_a = res.stratification["nstrat"], eng.strat_d()
    assert res.stratification["carry"] is True and res.stratification["carried"] == "uniform"
    res2 = mci.integrate(f, config=res.config, solver="vegas", neval=131072, niter=1, stratify=mci.Stratify(carry=True))
    assert res2.config._engine is eng
    plan_b = res2.stratification["nstrat"]
    assert plan_a != plan_b and res2.stratification["carried"] == "remapped" and eng.strat_carry() == (True, HOW_REMAPPED)
    counts = eng.strat_counts()
    assert counts.size == int(np.prod(plan_b)) == res2.stratification["ncube"]
    check_alloc(counts, alloc(oracle, remap_numpy(d_a, plan_a, plan_b), 131072), 131072, "%s -> %s" % (plan_a, plan_b))
    lines = []

    class IO:
        def write(self, s):
            lines.append(s)
    mci.report(res2, io=IO())
    assert "moved onto this plan" in "".join(lines)


# ---- 4: frozen production -----------------------------------------------------------------------------------------------------------

def test_frozen_production_keeps_the_carried_allocation(oracle):
    eng = sphere_engine()
    d = train(eng)
    g = eng.grid(0).copy()
    eng.integrate("vegas", N0, niter=3, block=BLOCK, seed=SEED, first_iteration=3, adapt=False)
    counts = eng.strat_counts()                               # (of the call's LAST iteration)
    check_alloc(counts, alloc(oracle, d, N0), N0, "adapt = False")
    assert np.abs(counts - uniform(oracle, 15, N0)).max() > 1
    assert np.array_equal(eng.grid(0), g) and eng.strat_carry() == (True, HOW_SAME)
    assert not np.array_equal(eng.strat_d(), d)               # d_d goes on holding the last finished iteration's values
    eng.close()


# ---- 5: state files -----------------------------------------------------------------------------------------------------------------

def v1_length(nleaf, ni, npts):
    """ "MCISTATE" | u32 version, nleaf, ni | per leaf u32 kind, n | f64 reweight[ni + 1] | per leaf f64 grid[n] """
    return 8 + 3 * 4 + nleaf * 2 * 4 + (ni + 1) * 8 + sum(npts) * 8


def test_state_file_carries_the_allocation(tmp_path):
    path = str(tmp_path / "a.mcistate")
    a = sphere_engine(deterministic=True)
    a.integrate("vegas", N0, niter=3, block=BLOCK, seed=SEED)
    a.save_state(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"MCISTATE" and struct.unpack("<I", raw[8:12])[0] == 2
    body = v1_length(1, 2, [1000])
    assert len(raw) == body + 4 + 3 * 4 + 8 + 8 + 15 * 8
    ndim, n0, n1, n2, ncube, beta = struct.unpack("<IIIIQd", raw[body:body + 32])
    assert (ndim, n0, n1, n2, ncube, beta) == (3, 5, 1, 3, 15, 0.75)
    assert np.array_equal(np.frombuffer(raw[body + 32:], dtype=np.float64), a.strat_d())
    b = sphere_engine(deterministic=True)
    b.load_state(path)
    ra = a.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    rb = b.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    assert np.array_equal(a.strat_counts(), b.strat_counts()) and np.abs(np.diff(b.strat_counts())).max() > 1
    assert np.array_equal(ra["iter_mean"], rb["iter_mean"]) and np.array_equal(ra["iter_std"], rb["iter_std"])
    assert b.strat_carry() == (True, HOW_SAME)
    # ... loaded before the problem is stratified at all, and onto another plan
    c = mci.Engine(sphere_cfg(), mci.catalog.sphere2())
    c.load_state(path)
    c.set_stratification(nstrat=[7, 2, 4], carry=True)
    c.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED)
    assert c.strat_carry() == (True, HOW_REMAPPED) and np.abs(np.diff(c.strat_counts())).max() > 1
    # a problem that does not carry ignores the section
    e = sphere_engine(carry=False)
    e.load_state(path)
    e.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED)
    assert e.strat_carry() == (False, HOW_UNIFORM) and np.abs(np.diff(e.strat_counts())).max() <= 1
    for eng in (a, b, c, e):
        eng.close()


def test_state_file_versions_and_refusals(tmp_path):
    p1, p2, p3 = (str(tmp_path / n) for n in ("plain.mcistate", "carried.mcistate", "offcarry.mcistate"))
    plain = mci.Engine(sphere_cfg(), mci.catalog.sphere2())
    plain.integrate("vegas", N0, niter=2, block=BLOCK, seed=SEED)
    plain.save_state(p1)
    raw = open(p1, "rb").read()
    assert raw[:8] == b"MCISTATE" and struct.unpack("<I", raw[8:12])[0] == 1 and len(raw) == v1_length(1, 2, [1000])
    # a stratified problem that does not carry writes version 1 too
    off = sphere_engine(carry=False)
    train(off)
    off.save_state(p3)
    assert struct.unpack("<I", open(p3, "rb").read()[8:12])[0] == 1 and os.path.getsize(p3) == v1_length(1, 2, [1000])
    # a version-1 file leaves a carrying problem nothing to start from
    eng = sphere_engine()
    train(eng)
    eng.save_state(p2)
    eng.load_state(p1)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    assert eng.strat_carry() == (True, HOW_UNIFORM) and np.abs(np.diff(eng.strat_counts())).max() <= 1
    # a carried allocation over three draws does not fit a problem whose samples have two
    two = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1], [2]], seed=SEED), mci.Integrand("w[0] = x[0]; w[1] = x[0] * x[1];"))
    with pytest.raises(mci.MCIError, match="ndim"):
        two.load_state(p2)
    # ... and a plan that does not multiply up to its ncube is refused
    raw = bytearray(open(p2, "rb").read())
    body = v1_length(1, 2, [1000])
    raw[body + 4:body + 8] = struct.pack("<I", 4)            # nstrat[0]: 5 -> 4
    bad = str(tmp_path / "bad.mcistate")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(mci.MCIError, match="ncube"):
        eng.load_state(bad)
    for e in (plain, off, eng, two):
        e.close()


# ---- 6: carry off -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("explicit", [True, False], ids=["carry_false", "keyword_absent"])
def test_carry_off_starts_every_call_uniform(oracle, explicit):
    eng = mci.Engine(sphere_cfg(), mci.catalog.sphere2())
    kw = dict(carry=False) if explicit else {}
    eng.set_stratification(nstrat=list(PLAN), **kw)
    even = uniform(oracle, 15, N0)
    assert even.min() >= N0 // 15 and even.max() <= N0 // 15 + 1
    eng.integrate("vegas", N0, niter=3, block=BLOCK, seed=SEED)
    assert np.abs(eng.strat_counts() - even).max() > 1       # the call did learn an allocation ...
    assert set(eng.stratification()) == {"nstrat", "ncube", "beta"}
    for k in range(2):
        if k == 1:                                           # ... which neither the next call nor the setter in between keeps
            eng.set_stratification(nstrat=list(PLAN), **kw)
        eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3 + k)
        assert np.array_equal(eng.strat_counts(), even) and eng.strat_carry() == (False, HOW_UNIFORM)
    # switching carry off drops what a carrying problem held
    eng.set_stratification(nstrat=list(PLAN), carry=True)
    train(eng)
    eng.set_stratification(nstrat=list(PLAN), **kw)
    eng.integrate("vegas", N0, niter=1, block=BLOCK, seed=SEED, first_iteration=3)
    assert np.array_equal(eng.strat_counts(), even) and eng.strat_carry() == (False, HOW_UNIFORM)
    eng.close()


# ---- 7: determinism -----------------------------------------------------------------------------------------------------------------

def test_two_call_sequence_is_bit_identical():
    out = []
    for _ in range(2):
        eng = sphere_engine(deterministic=True)
        r1 = eng.integrate("vegas", N0, niter=3, block=BLOCK, seed=SEED)
        eng.set_stratification(nstrat=[7, 2, 4], carry=True)
        r2 = eng.integrate("vegas", N0, niter=2, block=BLOCK, seed=SEED, first_iteration=3)
        assert eng.strat_carry() == (True, HOW_REMAPPED)
        out.append((r1["iter_mean"].copy(), r2["iter_mean"].copy(), r2["iter_std"].copy(), eng.strat_counts()))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 8: what it buys ----------------------------------------------------------------------------------------------------------------

WATSON_EXACT = 1.3932039297
# production error carried / not carried, pooled over the eight seeds, as measured on an MI355X with the not-carried run of the same
# script as the yardstick (profiles/r09_strat_carry.txt: 0.427 over seeds 1 .. 8, 0.426 over 32; per seed 0.40 .. 0.50); the test's bound
# lies halfway between it and 1, so that seed-to-seed spread does not flip it
MEASURED_RATIO = 0.427
RATIO_BOUND = 0.5 * (MEASURED_RATIO + 1.0)


def watson_train_then_freeze(seed, carry):
    st = mci.Stratify(carry=carry)
    res = mci.integrate(WATSON, config=watson_cfg(seed), solver="vegas", neval=2e5, niter=10, stratify=st)
    return mci.integrate(WATSON, config=res.config, solver="vegas", neval=2e5, niter=10, adapt=False, stratify=st)


def test_carried_production_pays_and_its_errors_are_honest():
    """Train at neval = 2e5 x 10, then measure at 2e5 x 10 with adapt=False: carried, the production call runs on the allocation the
    training learned; not carried, on an even one.  Eight seeds; `error` is the pooled reported error of the production call.
    (Measured: scatter of the eight carried means 0.65 x their mean reported error, 0.89 x over 32 seeds; the rms deviation from the
    exact value falls by more than the reported error does, x 0.26 | 0.34 -- profiles/r09_strat_carry.txt.)"""
    rows = {}
    for carry in (True, False):
        rows[carry] = [(r.mean[0], r.stdev[0], r.stratification["carried"]) for r in (watson_train_then_freeze(s, carry) for s in range(1, 9))]
    for s in range(8):
        print("seed %d  carried %.8f +- %.3g (%s)   not carried %.8f +- %.3g (%s)" % ((s + 1,) + rows[True][s] + rows[False][s]))
    assert all(r[2] == "same plan" for r in rows[True]) and all(r[2] == "uniform" for r in rows[False])
    m, e = (np.array([r[k] for r in rows[True]]) for k in (0, 1))
    m0, e0 = (np.array([r[k] for r in rows[False]]) for k in (0, 1))
    pooled, pooled0 = math.sqrt(np.mean(e * e)), math.sqrt(np.mean(e0 * e0))
    ss, es = float(np.std(m, ddof=1)), float(np.mean(e))
    print("pooled error carried %.4g  not carried %.4g  ratio %.3f | carried: scatter %.4g reported %.4g ratio %.2f | rms deviation from the exact "
          "value carried %.4g not carried %.4g" % (pooled, pooled0, pooled / pooled0, ss, es, ss / es,
                                                   math.sqrt(np.mean((m - WATSON_EXACT) ** 2)), math.sqrt(np.mean((m0 - WATSON_EXACT) ** 2))))
    assert pooled / pooled0 < RATIO_BOUND, (pooled, pooled0, MEASURED_RATIO)
    assert 0.6 < ss / es < 1.5, (ss, es)                     # the rule of test_stratified_errors_are_honest_and_smaller
