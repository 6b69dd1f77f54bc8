"""GPU parity of stratified :vegas (VEGAS+; csrc/mci_strat.h, k_strat_alloc / k_strat_reduce) against the oracle's plain VEGAS+
iteration (oracle/mci_oracle.c mcio_strat_alloc / mcio_strat_iteration) on identical Philox streams, sample by sample.

`drive` runs engine and oracle through `niter` iterations, teacher-forced: before iteration k the oracle takes the engine's grids and
the engine's offsets, after both have been compared with its own -- a one-sample rounding difference of iteration k cannot turn into
an unrelated iteration k + 1, and nothing of an iteration stays unchecked.  Per iteration:

    h of every sample                  the walk over the offsets                     equal
    y, x of every sample               oracle replay                                 bit-equal
    common jac, weights w              oracle                                        rel 1e-13
    mean per column                    oracle (long double)                          1e-11 * sum_h V / n_h sum |f J|
    sum_k s^2_{h,k} = d_h^(2 / beta)   oracle two-pass                               sum_k 4 (n_h + 2) 2^-53 S2_{h,k} / (n_h - 1)  (the forward
                                                                                     error of the one-pass formula, Chan, Golub, LeVeque
                                                                                     1983, x 4 for the lane-order sums) + rel 1e-12 (pow)
    variance per column                oracle                                        sum_h V^2 / n_h * that bound + rel 1e-11
    merged histogram                   oracle leaf histograms + (m + 1) 1e-10        rel 1e-9 per bin
    next allocation                    mcio_strat_alloc of the ORACLE's d_h          sum = N, min >= 2, |delta n_h| <= 1 on at most
                                                                                     max(2, ncube / 1000) hypercubes
    grids after finish(adapt = True)   the oracle's train!                           abs 1e-12 * range, ends equal, increasing

(tests/test_oracle_stratified.py counts, for the kernel's documented summation order, how many hypercubes the last but one row can
differ on: none at the sizes used here.)"""
import math

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import COMPLEX_BODY
from test_hip_stratified import PEAK

pytestmark = pytest.mark.gpu
PI = math.pi
SEED = 20240229
U = 2.0 ** -53


def ocont(pool=0, lo=0.0, hi=1.0, **kw):
    return dict(kind=0, pool=pool, lower=lo, upper=hi, **kw)


EIGHT = " ".join("w[%d] = cos(%d.0 * x[0]) * (x[1] - %.1f);" % (k, k + 1, 0.1 * k) for k in range(8))
NINE = EIGHT + " w[8] = x[0];"
POOLS3 = "w[0] = exp(-3.0 * x[0]) * (1.0 + x[1] * x[1]) * sin(x[2] + 2.0 * x[3]);"
PEAK2 = "const double a = x[0] - 0.3, b = x[1] - 0.6; w[0] = exp(-(a * a + b * b) * 400.0) * 127.32395447351628;"   # 400 / pi: ~1 on [0, 1]^2
SUM8 = "double s = 0.0; for (int d = 0; d < 8; ++d) s += (d + 1) * x[d]; w[0] = s * s - 20.0;"

# layout: product variables, dof, integrand (catalog twin: (Integrand, oracle builtin) | C text for both sides), oracle leaves
LAYOUTS = {
    "sphere2": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[2], [3]], f=(mci.catalog.sphere2, "sphere2"), oleaves=[ocont()]),
    "complex": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[1], [1]], f=COMPLEX_BODY, oleaves=[ocont()], complex=True),
    "eight": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[2]] * 8, f=EIGHT, oleaves=[ocont()]),
    "pools3": dict(var=lambda: (mci.Continuous(0.0, 1.0, ninc=17, alpha=0.5), mci.Continuous(-2.0, 3.0, ninc=257, alpha=3.0, adapt=False),
                                mci.Continuous(0.0, 2.0, ninc=1000, alpha=3.0)),
                   dof=[[1, 1, 2]], f=POOLS3,
                   oleaves=[ocont(0, 0.0, 1.0, npts=17, alpha=0.5), ocont(1, -2.0, 3.0, npts=257, alpha=3.0, adapt=False),
                            ocont(2, 0.0, 2.0, npts=1000, alpha=3.0)]),
    "composite": dict(var=lambda: mci.Continuous([(0.0, PI)] * 3), dof=[[1]], f=(mci.catalog.singular2, "singular2"),
                      oleaves=[ocont(0, 0.0, PI) for _ in range(3)]),
    "x2y2": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[2]], f=(mci.catalog.x2y2, "x2y2"), oleaves=[ocont()]),
    "sum8": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[8]], f=SUM8, oleaves=[ocont()]),
    "three": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[3]], f="w[0] = x[0] + x[1] * x[2] - 0.5;", oleaves=[ocont()]),
    "peak1": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[1]], f=PEAK, oleaves=[ocont()]),
    "peak2": dict(var=lambda: mci.Continuous(0.0, 1.0), dof=[[2]], f=PEAK2, oleaves=[ocont()]),
}


def make(oracle, name, **engine_kw):
    L = LAYOUTS[name]
    cx = L.get("complex", False)
    cfg = mci.Configuration(var=L["var"](), dof=L["dof"], seed=SEED, **(dict(type=complex) if cx else {}))
    if isinstance(L["f"], tuple):
        f, of = L["f"][0](), L["f"][1]
    else:
        f, of = mci.Integrand(L["f"]), oracle.compile_c_integrand(L["f"])
    eng = mci.Engine(cfg, f, **engine_kw)
    ocfg = oracle.Config(L["oleaves"], L["dof"], obs_nbin=[2] * len(L["dof"]) if cx else None)
    if cx:
        ocfg.set_ncomp(2)
    return L, cfg, eng, ocfg, of


def merged_blocks(N, block):
    """blocks the launch's rows are merged as (strat_run: mblocks): the call's, or one when it has fewer chunks than blocks.  A chunk
    is 256 .. 2048 samples, whichever the LDS budget gives: the sizes used here decide the question for every chunk size."""
    if -(-N // 256) < block:
        return 1
    assert -(-N // 2048) >= block, "choose N so that the chunk size does not decide how the rows are merged"
    return block


def check_alloc(counts, want, N, what):
    nc = counts.size
    assert counts.sum() == N and counts.min() >= 2, what
    delta = np.abs(counts - want)
    bad = np.flatnonzero(delta)
    assert delta.max() <= 1 and bad.size <= max(2, nc // 1000), (what, "first hypercube that differs", bad[:1], counts[bad[:5]], want[bad[:5]], bad.size)


def drive(oracle, name, nstrat, N, niter, block=4, lo=0, beta=0.75, seed=SEED, setup=None, report=None, **engine_kw):
    """engine and oracle through niter stratified iterations of N samples, everything of the module's table asserted at every one;
    returns (engine, oracle config, [(oracle mean, oracle std)], [counts], worst |v2_gpu - v2_ref| / bound)"""
    L, cfg, eng, ocfg, of = make(oracle, name, **engine_kw)
    if setup:
        setup(eng, ocfg)
    eng.set_stratification(nstrat=nstrat, beta=beta)
    assert N % block == 0
    npb, D, NI = N // block, eng.ndraw, cfg.N
    nc = int(np.prod(nstrat))
    NW, nstat = eng.nobs, 2 * eng.nobs + 2 + NI + 1
    V = 1.0 / nc
    m_blocks = merged_blocks(N, block)
    rows, all_counts, worst = [], [], 0.0
    want = np.diff(oracle.Config.strat_alloc(np.ones(nc), N, True))     # every plan starts uniform
    for k in range(niter):
        tag = "%s %s iteration %d" % (name, nstrat, k)
        for i in range(len(L["oleaves"])):                               # teacher forcing: the engine's grids (compared after the last train!)
            ocfg.set_grid(i, eng.grid(i))
        dump = eng.strat_dump_next(N)
        pk = eng.iteration("vegas", npb, lo, lo + block, k, seed)
        m, e = eng.finish("vegas", block, adapt=True)
        counts = eng.strat_counts()
        all_counts.append(counts)
        check_alloc(counts, want, N, tag)
        off = np.concatenate([[0], np.cumsum(counts)])                   # teacher forcing: the engine's offsets
        r = ocfg.strat_iteration(of, None, seed, k, lo * npb, nstrat, off, beta, samples=True)
        n = counts.astype(np.float64)
        # samples
        h = np.searchsorted(off, np.arange(N), side="right") - 1
        bad = np.flatnonzero(dump["h"] != h)
        assert bad.size == 0, (tag, "first sample in another hypercube", bad[0], dump["h"][bad[0]], h[bad[0]])
        for key in ("y", "x"):
            bad = np.flatnonzero(np.any(dump[key] != r[key], axis=1))
            assert bad.size == 0, (tag, key, "first differing sample", bad[0], "hypercube", h[bad[0]], dump[key][bad[0]], r[key][bad[0]], bad.size)
        np.testing.assert_allclose(dump["jac"], r["jac"], rtol=1e-13, atol=0, err_msg=tag)
        np.testing.assert_allclose(dump["w"], r["w"], rtol=1e-13, atol=1e-300, err_msg=tag)
        # mean
        tol_mean = 1e-11 * (V / n[:, None] * r["A1"]).sum(axis=0)
        print(tag, "mean", m, "ref", r["mean"], "tol", tol_mean)
        assert np.all(np.abs(m - r["mean"]) <= tol_mean), (tag, m, r["mean"], tol_mean)
        # per-hypercube variance sums through d_h
        bound_hq = 4.0 * (n[:, None] + 2.0) * U * r["S2"] / (n[:, None] - 1.0)
        v2_ref = r["v2"].sum(axis=1)
        # (d_h ** (2 / beta) in long double: in double the rounding of the exponent 2 / beta alone, times |ln d_h| of a hypercube in the far
        # tail of a peak, is several times the bound -- 9.3 x at d_h ~ 1e-98 -- and would hide what the kernel's formula does)
        v2_gpu = (eng.strat_d().astype(np.longdouble) ** (np.longdouble(2.0) / np.longdouble(beta))).astype(np.float64) if beta > 0 else None
        if v2_gpu is not None:
            bound = bound_hq.sum(axis=1)
            err = np.abs(v2_gpu - v2_ref)
            tol = bound + 1e-12 * np.maximum(v2_ref, v2_gpu)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / bound, 0.0)
            worst = max(worst, float(ratio.max()))
            print(tag, "max |v2_gpu - v2_ref| / bound = %.3g" % ratio.max())
            bad = np.flatnonzero(~(err <= tol))
            assert bad.size == 0, (tag, "first hypercube", bad[0], "n_h", counts[bad[0]], v2_gpu[bad[0]], v2_ref[bad[0]], bound[bad[0]], bad.size)
        # variance
        tol_var = (V * V / n[:, None] * bound_hq).sum(axis=0) + 1e-11 * r["var"]
        print(tag, "var", e * e, "ref", r["var"], "tol", tol_var)
        assert np.all(np.abs(e * e - r["var"]) <= tol_var), (tag, e * e, r["var"], tol_var)
        # histogram (the oracle's holds one clearStatistics! offset; the merge adds one per block it merges the rows as)
        for i in range(len(L["oleaves"])):
            ocfg.add_hist(i, m_blocks * 1e-10)
        ref_h = np.concatenate([ocfg.hist(i) for i in range(len(L["oleaves"]))])
        got_h = pk[nstat:nstat + ref_h.size]
        bad = np.flatnonzero(~np.isclose(got_h, ref_h, rtol=1e-9, atol=0))
        assert bad.size == 0, (tag, "first bin", bad[0], got_h[bad[0]], ref_h[bad[0]], bad.size)
        # train!
        ocfg.train()
        for i, lf in enumerate(L["oleaves"]):
            g, og = eng.grid(i), ocfg.grid(i)
            assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0), (tag, i)
            np.testing.assert_allclose(g, og, rtol=0, atol=1e-12 * (lf["upper"] - lf["lower"]), err_msg=tag)
        rows.append((r["mean"].copy(), np.sqrt(r["var"])))
        want = np.diff(oracle.Config.strat_alloc(r["d"], N))             # the next allocation, from the ORACLE's d_h
    if report is not None:
        report[name + str(nstrat)] = worst
    print("RATIO %s %s N=%d: largest |v2_gpu - v2_ref| / bound over %d iterations = %.3g" % (name, nstrat, N, niter, worst))
    return eng, ocfg, rows, all_counts, worst


# ---- layouts ------------------------------------------------------------------------------------------------------------------------

def test_ragged_dof_two_columns(oracle):
    """layout 1: jaci != jac (a padding probability), NW = 2, a draw that is not cut"""
    eng, _, _, counts, _ = drive(oracle, "sphere2", [5, 1, 3], 32768, 3)
    assert np.abs(counts[1] - counts[0]).max() > 1     # the allocation did move
    eng.close()


def test_complex_weights(oracle):
    """layout 2: four columns, two integrands, the modulus in the histogram"""
    drive(oracle, "complex", [37], 16384, 2)[0].close()


def test_eight_columns_and_the_ninth_refused(oracle):
    """layout 3: kStratMaxCols"""
    drive(oracle, "eight", [7, 9], 16384, 2)[0].close()
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]] * 9), mci.Integrand(NINE))
    with pytest.raises(mci.MCIError, match="columns"):
        eng.set_stratification(nstrat=[7, 9])
    eng.close()


def test_three_pools_own_grids(oracle):
    """layout 4a: ninc 17 / 257 / 1000, alpha 0.5 / 3, one pool that does not adapt"""
    eng, ocfg, _, _, _ = drive(oracle, "pools3", [3, 2, 1, 5], 16384, 3)
    assert np.array_equal(eng.grid(1), np.linspace(-2.0, 3.0, 257))
    eng.close()


def test_composite_variable(oracle):
    """layout 4b: a composite Continuous variable, one grid per draw"""
    drive(oracle, "composite", [6, 6, 6], 16384, 2)[0].close()


def test_table_mode_3_is_refused(overrides):
    """layout 12 cannot run: mci_problem_create gives every one-tile problem in table mode 3 an LDS cache of the leading grids' edges
    (ec_doubles > 0), which the stratified kernel does not read (t.EC = nullptr) and strat_layout_check therefore refuses together with
    the tiled layouts -- although its list names mode 3 as allowed.  Pinned as the refusal it is."""
    overrides.set("table_mode", 3)
    eng = mci.Engine(mci.Configuration(var=mci.Continuous([(0.0, PI)] * 3), dof=[[1]]), mci.catalog.singular2())
    with pytest.raises(mci.MCIError, match="tiles"):
        eng.set_stratification(nstrat=[6, 6, 6])
    eng.close()


@pytest.mark.parametrize("name,nstrat,N", [("x2y2", [251, 3], 16384), ("sum8", [2] * 8, 16384), ("three", [1, 1, 1021], 16384)])
def test_cell_decode_around_the_magic_division(oracle, name, nstrat, N):
    """layout 5: a prime that is not near a power of two, eight binary digits, a prime behind two ones"""
    drive(oracle, name, nstrat, N, 2)[0].close()


@pytest.mark.parametrize("bits,rounds", [(32, 10), (52, 7), (32, 7)])
def test_streams(oracle, bits, rounds):
    """layout 6: the 32-bit stream (four draws per Philox block), the seven-round generator, both"""
    def setup(eng, ocfg):
        if bits == 32:
            eng.set_rng_bits(32)
            ocfg.set_rng_bits(32)
        if rounds == 7:
            eng.set_rng_rounds(7)
    oracle.set_rng_rounds(rounds)
    try:
        drive(oracle, "sphere2", [5, 1, 3], 16384, 2, setup=setup)[0].close()
    finally:
        oracle.set_rng_rounds(10)


def test_block_range(oracle):
    """layout 7: blocks 3 .. 6 of the call: the Philox counter of sample 0 is 3 npb"""
    drive(oracle, "sphere2", [5, 1, 3], 16384, 2, block=4, lo=3)[0].close()


@pytest.mark.parametrize("N,block,nstrat", [(30, 1, [5, 1, 3]), (200, 4, [5, 1, 3]), (8193, 3, [5, 1, 3]), (2048, 16, [5, 1, 3]), (4096, 2, [16, 1, 128])],
                         ids=["two_each_tiny", "below_one_trip", "odd", "more_blocks_than_chunks", "two_each_2048_cubes"])
def test_sizes(oracle, N, block, nstrat):
    """layout 8: N = 2 ncube (every n_h = 2: nothing left to move, no hypercube cut), N below one trip of 256 lanes, N odd and no
    multiple of 256, more blocks than chunks"""
    eng, _, _, counts, _ = drive(oracle, "sphere2", nstrat, N, 2, block=block)
    if N == 2 * int(np.prod(nstrat)):
        assert all(np.all(c == 2) for c in counts)
    eng.close()


def test_skewed_allocation_cut_and_long_hypercubes(oracle):
    """layout 9: hypercubes longer than several chunks next to hypercubes of two samples: the boundary records of k_strat_reduce"""
    eng, _, _, counts, _ = drive(oracle, "peak1", [64], 200000, 3, beta=1.0)
    assert max(c.max() for c in counts) > 4 * 2048 and min(c.min() for c in counts) == 2, [(c.max(), c.min()) for c in counts]
    eng.close()


def test_large_plan_above_2_18_hypercubes(oracle):
    """layout 10: 727^2 = 528529 hypercubes -- stretches of k_strat_alloc longer than one element, the 1024-tile cap, an empty trailing
    tile -- and every one of the 2^22 + 5 samples compared"""
    N = 2 ** 22 + 5
    eng, _, _, counts, _ = drive(oracle, "peak2", [727, 727], N, 2, block=1)
    assert counts[0].size == 528529 > 2 ** 18 and 528529 % 1024 != 0
    assert counts[1].max() > counts[1].min()     # the second allocation came from d_h
    eng.close()


def test_deterministic_mode(oracle):
    """layout 11: one histogram copy per wave"""
    drive(oracle, "sphere2", [5, 1, 3], 16384, 2, deterministic=True)[0].close()


# ---- whole calls --------------------------------------------------------------------------------------------------------------------

def _layout1_engine(nstrat=(5, 1, 3), beta=0.75):
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED), mci.catalog.sphere2())
    eng.set_stratification(nstrat=list(nstrat), beta=beta)
    return eng


def test_adapt_false_keeps_allocation_and_grids(oracle):
    N, block = 16384, 4
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(15), N, True))
    eng = _layout1_engine()
    g0 = eng.grid(0).copy()
    for k in range(3):
        eng.run("vegas", N // block, 0, block, k, SEED)
        eng.finish("vegas", block, adapt=False)
        assert np.array_equal(eng.strat_counts(), uniform), k
        assert np.array_equal(eng.grid(0), g0)
    assert eng.strat_d().max() > 0       # there was something to adapt to
    eng.integrate("vegas", N, niter=3, block=block, adapt=False, seed=SEED)
    assert np.array_equal(eng.strat_counts(), uniform) and np.array_equal(eng.grid(0), g0)
    eng.close()


def test_second_call_starts_uniform_again(oracle):
    N, block = 16384, 4
    uniform = np.diff(oracle.Config.strat_alloc(np.ones(15), N, True))
    eng = _layout1_engine()
    eng.integrate("vegas", N, niter=3, block=block, seed=SEED)
    assert np.abs(eng.strat_counts() - uniform).max() > 1 and eng.strat_d().max() > 0
    eng.integrate("vegas", N, niter=1, block=block, seed=SEED)
    assert np.array_equal(eng.strat_counts(), uniform)
    eng.close()


def test_constant_integrand_whole_call():
    """w = 0.7 on a map that stays untrained (the variable does not adapt; the allocation does): every sample carries the same f J up to
    the rounding of the bin widths, the clamped one-pass variance is rounding noise, and the allocations made from it must be valid.
    And on a map that trains: the bin widths then differ, f J with them, and the mean is 0.7 within its reported error."""
    res = mci.integrate("w[0] = 0.7;", var=mci.Continuous(0.0, 1.0, adapt=False), dof=[[2]], solver="vegas", neval=1e5, niter=3, seed=SEED,
                        stratify=True)
    print("constant integrand, untrained map:", res.mean[0], res.stdev[0], res.iter_mean[:, 0], res.iter_std[:, 0])
    assert res.mean[0] == pytest.approx(0.7, rel=1e-13)
    assert np.all(np.abs(res.iter_mean[:, 0] - 0.7) <= 0.7e-13)
    assert res.stdev[0] <= 1e-6 * abs(res.mean[0])
    c = res.config._engine.strat_counts()
    assert c.sum() == 1e5 and c.min() >= 2 and res.stratification["ncube"] == c.size > 1
    res = mci.integrate("w[0] = 0.7;", var=mci.Continuous(0.0, 1.0), dof=[[2]], solver="vegas", neval=1e5, niter=3, seed=SEED, stratify=True)
    print("constant integrand, trained map:", res.mean[0], res.stdev[0], res.iter_mean[:, 0], res.iter_std[:, 0])
    assert res.iter_mean[0, 0] == pytest.approx(0.7, rel=1e-13)          # (the first iteration runs on the untrained map)
    assert abs(res.mean[0] - 0.7) < 5 * res.stdev[0]
    c = res.config._engine.strat_counts()
    assert c.sum() == 1e5 and c.min() >= 2


def test_integrate_iterations_are_the_oracle_iterations(oracle):
    """mci.integrate(stratify = ...) logs, iteration by iteration, what the teacher-forced helper's oracle computes for the same seed,
    and weights the iterations as the reference does (statistics.jl:186-220 through oracle.average)"""
    N, block, niter = 65536, 16, 4
    _, _, rows, _, _ = drive(oracle, "sphere2", [5, 1, 3], N, niter, block=block)
    res = mci.integrate(mci.catalog.sphere2(), var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], solver="vegas", neval=N, niter=niter, block=block,
                        seed=SEED, stratify=mci.Stratify(nstrat=[5, 1, 3]))
    im, ie = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    np.testing.assert_allclose(res.iter_mean, im, rtol=1e-9)
    np.testing.assert_allclose(res.iter_std, ie, rtol=1e-6)
    for q in range(2):
        mean, err, chi2 = oracle.average(im[:, q], ie[:, q], init=2)      # ignore = 1 (adapt = True)
        assert res.mean[q] == pytest.approx(mean, rel=1e-9) and res.stdev[q] == pytest.approx(err, rel=1e-6)
        assert res.chi2[q] == pytest.approx(chi2, rel=1e-5)
