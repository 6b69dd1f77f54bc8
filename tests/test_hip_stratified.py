"""GPU tests of stratified :vegas (VEGAS+ adaptive stratified sampling, csrc/mci_strat.h): one hypercube is classic :vegas, the
allocation / strata / statistics of an iteration against numpy recomputed from the samples it dumped, known answers, the error it
buys, determinism, refusals, and that switching it off gives the plain kernels' numbers back."""
import math

import numpy as np
import pytest

import mcintegration_jl_amd as mci

pytestmark = pytest.mark.gpu

WATSON = "w[0] = 1.0 / (1.0 - cos(x[0]) * cos(x[1]) * cos(x[2])) / (M_PI * M_PI * M_PI);"   # benchmark1.jl: 1.3932039297 on [0, pi]^3
GAUSS4 = ("double s = 0.0; for (int d = 0; d < 4; ++d) { const double t = x[d] - 0.5; s += t * t; } "
          "w[0] = exp(-100.0 * s) * 1013.2118364296088;")                                       # benchmark4.jl: 1 on [0, 1]^4
LOGSQRT = "w[0] = log(x[0]) / sqrt(x[0]);"


def watson_cfg(seed=None):
    kw = {} if seed is None else dict(seed=seed)
    return mci.Configuration(var=mci.Continuous(0.0, math.pi, alpha=3.0), dof=[[3]], **kw)


def alloc_rule(d, N):
    """step 2: cumulative rounding of the damped weights d_h (uniform where sum d is 0 or not finite)"""
    d = np.asarray(d, dtype=np.float64)
    nc = d.size
    M = N - 2 * nc
    tot = d.sum()
    if not (tot > 0 and np.isfinite(tot)):
        C = M * np.arange(1, nc + 1, dtype=np.float64) / nc
    else:
        C = M * np.cumsum(d) / tot
    C = np.minimum(C, M)
    C[-1] = M
    fl = np.floor(C).astype(np.int64)
    return 2 + np.diff(np.concatenate([[0], fl]))


def strat_stats(fj, h, counts, beta):
    """steps 4-6 from the samples: (mean, var) of the iteration and d_h of the next allocation"""
    nc = counts.size
    V = 1.0 / nc
    s1 = np.bincount(h, weights=fj, minlength=nc)
    s2 = np.bincount(h, weights=fj * fj, minlength=nc)
    n = counts.astype(np.float64)
    v2 = np.maximum((s2 - s1 * s1 / n) / (n - 1.0), 0.0)
    return (V / n * s1).sum(), (V * V * v2 / n).sum(), v2 ** (beta / 2)


@pytest.mark.parametrize("layout", ["c1", "3d"])
def test_one_hypercube_is_classic_vegas(layout):
    if layout == "c1":
        cfg_args, f, N, block = dict(var=mci.Continuous(0.0, 1.0), dof=[[1]]), mci.Integrand(LOGSQRT), 16384, 4
    else:
        cfg_args, f, N, block = dict(var=mci.Continuous(0.0, math.pi, alpha=3.0), dof=[[3]]), mci.Integrand(WATSON), 24576, 4
    seed, npb = 77, N // block
    classic = mci.Engine(mci.Configuration(**cfg_args), f)
    strat = mci.Engine(mci.Configuration(**cfg_args), f)
    D = strat.ndraw
    strat.set_stratification(nstrat=[1] * D)
    parts = [classic.sample_dump(npb, nevalperblock=npb, block_index=b, iteration=0, seed=seed) for b in range(block)]
    x0, jac0, w0 = (np.concatenate([p[i] for p in parts]) for i in range(3))
    dump = strat.strat_dump_next(N)
    pk_s = strat.iteration("vegas", npb, 0, block, 0, seed)
    pk_c = classic.iteration("vegas", npb, 0, block, 0, seed)
    assert np.array_equal(dump["x"], x0) and np.array_equal(dump["jac"], jac0) and np.array_equal(dump["w"], w0)
    assert np.all(dump["h"] == 0)
    nstat = 2 * strat.nobs + 2 + 2
    np.testing.assert_allclose(pk_s[nstat:nstat + 999], pk_c[nstat:nstat + 999], rtol=1e-9, atol=1e-9)   # the histogram (merge orders and offsets differ)
    ms, es = strat.finish("vegas", block)
    mc, ec = classic.finish("vegas", block)
    np.testing.assert_allclose(ms, mc, rtol=1e-11)
    np.testing.assert_allclose(strat.grid(0), classic.grid(0), rtol=1e-11, atol=1e-11)
    assert np.array_equal(strat.strat_counts(), [N])
    classic.close()
    strat.close()


def test_allocation_strata_and_statistics():
    N, block, seed, beta = 8192, 4, 5, 0.75
    eng = mci.Engine(watson_cfg(), mci.Integrand(WATSON))
    eng.set_stratification(nstrat=[4, 4, 4], beta=beta)
    assert eng.stratification() == dict(nstrat=[4, 4, 4], ncube=0, beta=beta)
    counts = []
    for it in range(2):
        dump = eng.strat_dump_next(N)
        pk = eng.iteration("vegas", N // block, 0, block, it, seed)
        m, e = eng.finish("vegas", block)
        c = eng.strat_counts()
        counts.append(c)
        assert c.size == 64 and c.min() >= 2 and c.sum() == N
        off = np.concatenate([[0], np.cumsum(c)])
        h = dump["h"]
        np.testing.assert_array_equal(h, np.searchsorted(off, np.arange(N), side="right") - 1)
        y = dump["y"]
        cell = np.stack([h % 4, (h // 4) % 4, h // 16], axis=1)
        assert np.all(y < 1.0) and np.all(y >= cell / 4.0) and np.all(y < (cell + 1) / 4.0)
        fj = dump["w"][:, 0] * dump["jac"]
        mean, var, d = strat_stats(fj, h, c, beta)
        np.testing.assert_allclose(m[0], mean, rtol=1e-11)
        np.testing.assert_allclose(e[0], math.sqrt(var), rtol=1e-11)
        r = N / (64.0 * c[h])
        wh = (np.abs(dump["w"][:, 0]) * dump["jac"]) ** 2 * r
        iy = (y * 999).astype(np.int64)   # (1000 grid points: 999 increments)
        hist = sum(np.bincount(iy[:, k], weights=wh, minlength=999) for k in range(3)) + (block + 1) * 1e-10   # (clearStatistics! offsets)
        nstat = 2 * eng.nobs + 2 + 2
        np.testing.assert_allclose(pk[nstat:nstat + 999], hist, rtol=1e-9)
        if it == 0:
            np.testing.assert_array_equal(c, alloc_rule(np.ones(64), N))   # the first iteration is uniform
            d_next = d
    # (the kernel sums each hypercube in its own order: a floor() of the cumulative rounding may land one sample to either side)
    want = alloc_rule(d_next, N)
    assert counts[1].sum() == want.sum() and np.abs(counts[1] - want).max() <= 1
    assert np.abs(counts[1] - counts[0]).max() > 1
    eng.close()


PEAK = "const double t = x[0] - 0.3; w[0] = exp(-t * t * 1.0e6) * 564.18958354775628;"   # sqrt(1e6 / pi): exact 1 on [0, 1]


def test_skewed_allocation_spans_chunks():
    # a sharply peaked 1-D integrand: after one iteration a few hypercubes hold far more samples than one chunk of the kernel
    res = mci.integrate(PEAK, var=mci.Continuous(0.0, 1.0), dof=[[1]], solver="vegas", neval=2e5, niter=2, seed=3,
                        stratify=mci.Stratify(nstrat=[64], beta=1.0))
    c = res.config._engine.strat_counts()
    assert c.max() > 2048 and c.sum() == 2e5 and c.min() >= 2
    assert abs(res.mean[0] - 1.0) < 5 * res.stdev[0]


@pytest.mark.parametrize("case", ["watson", "gauss4", "c2"])
def test_known_answers(case):
    L = math.sqrt(50.0)
    for seed in (1, 2, 3, 4):
        if case == "watson":
            res = mci.integrate(WATSON, config=watson_cfg(seed), solver="vegas", neval=2e5, niter=10, stratify=True)
            exact = 1.3932039297
        elif case == "gauss4":
            res = mci.integrate(GAUSS4, var=mci.Continuous(0.0, 1.0), dof=[[4]], solver="vegas", neval=1e5, niter=10, seed=seed, stratify=True)
            exact = 1.0
        else:
            # (the 16-D map needs ~6 iterations at this size, classic :vegas too -- profiles/r07_stratified.txt --, so those are ignored)
            res = mci.integrate(mci.catalog.gaussian(16), var=mci.Continuous(-L, L), dof=[[16]], solver="vegas", neval=1e6, niter=12, ignore=6,
                                seed=seed, stratify=True)
            exact = math.erf(5.0) ** 16
        z = (res.mean[0] - exact) / res.stdev[0]
        assert abs(z) < 5, (case, seed, res.mean[0], res.stdev[0])
        assert res.stratification and res.stratification["ncube"] > 1


def test_log_over_sqrt_closure_and_source():
    # the default plan on C1's heavy tail (hypercubes of ~8 samples: their variance estimates see the tail, profiles/r07_stratified.txt)
    for seed in (11, 12, 13, 14):
        for f in (LOGSQRT, lambda x, c: np.log(x[0]) / np.sqrt(x[0])):
            res = mci.integrate(f, var=mci.Continuous(0.0, 1.0), dof=[[1]], solver="vegas", neval=1e5, niter=10, seed=seed, stratify=True)
            assert abs(res.mean[0] + 4.0) < 7 * res.stdev[0], (seed, res.mean[0], res.stdev[0])


def _scatter(f, mk, neval, stratify, seeds=16):
    """(scatter of the final means over seeds, mean reported error)"""
    m, e = [], []
    for seed in range(1, seeds + 1):
        res = mci.integrate(f, config=mk(seed), solver="vegas", neval=neval, niter=10, stratify=stratify)
        m.append(res.mean[0])
        e.append(res.stdev[0])
    return float(np.std(m, ddof=1)), float(np.mean(e))


def _gauss4_cfg(seed):
    return mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]], seed=seed)


def _c1_cfg(seed):
    return mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]], seed=seed)


def test_stratified_errors_are_honest_and_smaller():
    """Over 16 seeds: the scatter of the stratified means is what the stratified errors say (the default plan, on benchmark1's
    integrable singularity, benchmark4's peak and C1's heavy tail), and the gain is stated from the scatter, not from reported errors."""
    ratios = {}
    for name, f, mk, neval in (("benchmark1", WATSON, watson_cfg, 2e5), ("benchmark4", GAUSS4, _gauss4_cfg, 1e5), ("c1", LOGSQRT, _c1_cfg, 1e5)):
        sc, _ = _scatter(f, mk, neval, None)
        ss, es = _scatter(f, mk, neval, True)
        print(name, "scatter classic %.3g stratified %.3g (reported %.3g)" % (sc, ss, es))
        assert 0.6 < ss / es < 1.5, (name, ss, es)
        ratios[name] = ss / sc
    print("scatter stratified / classic:", ratios)
    # benchmark1 meets the 0.5 the issue asked for (measured 0.17 over 32 seeds).  benchmark4 does not (0.87 over 32 seeds): its
    # integrand is a product of 1-D Gaussians, which the separable VEGAS map already samples near-ideally, so hypercubes add little --
    # pinned as "no worse than classic by more than 25 %", not as a gain (profiles/r07_stratified.txt).
    assert ratios["benchmark1"] <= 0.5, ratios
    assert ratios["benchmark4"] <= 1.25, ratios
    assert ratios["c1"] <= 0.5, ratios


def test_deterministic_bit_identical():
    out = []
    for _ in range(2):
        res = mci.integrate(WATSON, config=watson_cfg(9), solver="vegas", neval=1e5, niter=4, deterministic=True, stratify=True)
        out.append((res.mean[0], res.iter_std.copy(), res.config._engine.strat_counts()))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_refusals_name_their_reason():
    eng = mci.Engine(mci.Configuration(var=(mci.Continuous(0.0, 1.0), mci.Discrete(1, 4)), dof=[[1, 1]]), mci.Integrand("w[0] = x[0];"))
    with pytest.raises(mci.MCIError, match="Discrete"):
        eng.set_stratification()
    eng.close()
    eng = mci.Engine(watson_cfg(), mci.Integrand(WATSON), measure=mci.Measure("obs_add(0, rw[0]);"))
    with pytest.raises(mci.MCIError, match="measure"):
        eng.set_stratification()
    eng.close()
    eng = mci.Engine(watson_cfg(), lambda x, c: 1.0)
    with pytest.raises(mci.MCIError, match="host integrand"):
        eng.set_stratification()
    eng.close()
    eng = mci.Engine(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 32), dof=[[1]]), mci.catalog.genz_product_peak(32))
    with pytest.raises(mci.MCIError, match="tiles"):
        eng.set_stratification()
    eng.close()
    eng = mci.Engine(watson_cfg(), mci.Integrand(WATSON))
    eng.set_stratification()
    with pytest.raises(mci.MCIError, match="measurefreq"):
        eng.run("vegas", 1000, 0, 4, 0, 1, measurefreq=2)
    with pytest.raises(mci.MCIError, match="solver"):
        eng.run("vegasmc", 1000, 0, 4, 0, 1)
    eng.set_stratification(nstrat=[40, 40, 40])
    with pytest.raises(mci.MCIError, match="hypercubes"):
        eng.run("vegas", 1000, 0, 4, 0, 1)
    eng.close()
    with pytest.raises(ValueError, match="closure did not trace"):
        mci.integrate(lambda x, c: float(hash(str(x[0])) % 2), config=watson_cfg(), solver="vegas", neval=1e4, stratify=True)


def test_off_gives_plain_vegas_back():
    seed = 21
    eng = mci.Engine(watson_cfg(), mci.Integrand(WATSON), deterministic=True)
    g0 = eng.grid(0).copy()
    eng.set_stratification()
    eng.integrate("vegas", 1e5, niter=3, seed=seed)
    eng.set_stratification(on=False)
    eng.set_grid(0, g0)
    a = eng.integrate("vegas", 1e5, niter=3, seed=seed)
    fresh = mci.Engine(watson_cfg(), mci.Integrand(WATSON), deterministic=True)
    b = fresh.integrate("vegas", 1e5, niter=3, seed=seed)
    assert np.array_equal(a["iter_mean"], b["iter_mean"]) and np.array_equal(a["iter_std"], b["iter_std"])
    assert eng.stratification() is None
    eng.close()
    fresh.close()
