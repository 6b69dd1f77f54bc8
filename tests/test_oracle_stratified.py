"""The oracle's VEGAS+ iteration (oracle/mci_oracle.c mcio_strat_alloc / mcio_strat_iteration: the plain definition the stratified
:vegas kernels are compared with in tests/test_hip_stratified_parity.py) pinned on what can be known without a GPU, and the count
behind the cap of that module's allocation comparison."""
import math

import numpy as np
import pytest

from strat_cases import kernel_order_alloc

SEED = 20240229


def ocont(pool=0, lo=0.0, hi=1.0, **kw):
    return dict(kind=0, pool=pool, lower=lo, upper=hi, **kw)


def test_one_hypercube_is_the_classic_block(oracle):
    """nstrat = 1 everywhere: the samples, the weighted sums and the histograms of mcio_vegas_block (ragged dof: a padding probability)"""
    N, blk, it = 3000, 2, 3
    classic = oracle.Config([ocont()], [[2], [3]])
    classic.clear_statistics()
    assert classic.vegas_block("sphere2", None, SEED, it, blk, N) == 0
    strat = oracle.Config([ocont()], [[2], [3]])
    r = strat.strat_iteration("sphere2", None, SEED, it, blk * N, [1, 1, 1], [0, N], samples=True)
    # (the block's observable is sum w pad jac in double, S1 the same sum in long double)
    np.testing.assert_allclose(r["S1"][0], classic.observable, rtol=1e-13)
    np.testing.assert_allclose(r["mean"], classic.observable / N, rtol=1e-13)
    np.testing.assert_allclose(strat.hist(0), classic.hist(0), rtol=1e-14)   # (r_h = 1; the 1e-10 offset is added last here, first there)
    assert strat.c.neval == N
    for s in range(0, N, 211):
        us = [oracle.uniform(SEED, it * 8, blk * N + s, k) for k in range(3)]
        assert np.array_equal(r["y"][s], us)
        jac = 1.0
        for idx in range(1, 4):
            classic.pool_create(0, idx, [us[idx - 1]])
            jac /= classic.pool_prob(0)[idx - 1]
        assert np.array_equal(r["x"][s], classic.pool_data(0)[:3])
        assert r["jac"][s] == jac
        assert r["jaci"][s, 1] == jac and r["jaci"][s, 0] == classic.padding_probability(0) * jac


def test_32_bit_stream_and_round_count_reach_the_stratified_draws(oracle):
    cfg = oracle.Config([ocont()], [[2]])
    cfg.set_rng_bits(32)
    oracle.set_rng_rounds(7)
    try:
        r = cfg.strat_iteration("one", None, 5, 1, 40, [2, 3], oracle.Config.strat_alloc(np.ones(6), 60, True), samples=True)
        u = np.array([[oracle.uniform(5, 8, 40 + s, k, bits=32) for k in range(2)] for s in range(60)])
    finally:
        oracle.set_rng_rounds(10)
    h = np.repeat(np.arange(6), 10)
    np.testing.assert_array_equal(r["y"], np.minimum((np.stack([h % 2, h // 2], axis=1) + u) * (1.0 / np.array([2.0, 3.0])), 1 - 2.0 ** -53))


def test_constant_integrand(oracle):
    """w = 0.7 on an untrained map: every sample carries 0.7 x volume up to the rounding of the bin widths"""
    cfg = oracle.Config([ocont(0, -1.0, 2.0)], [[2]])
    f = oracle.compile_c_integrand("w[0] = 0.7;")
    off = oracle.Config.strat_alloc(np.ones(12), 5000, True)
    r = cfg.strat_iteration(f, None, SEED, 0, 0, [4, 3], off)
    assert r["mean"][0] == pytest.approx(0.7 * 9.0, rel=1e-13)
    assert math.sqrt(r["var"][0]) <= 1e-14 * r["mean"][0]
    # (a bin of width 3 / 999 between grid points of magnitude <= 2: its width, and 1 / prob with it, is rounded at ulp(2) / 3e-3 = 1.5e-13)
    assert np.all(r["d"] <= (1e-12 * 6.3) ** 0.75)


def test_allocation_rule(oracle):
    rng = np.random.default_rng(1)
    for nc, N in ((1, 2), (1, 77), (15, 30), (15, 31), (64, 8192), (1000, 2003), (24389, 200000)):
        for variant in range(4):
            d = rng.lognormal(0.0, 3.0, nc) ** 0.375
            if variant == 1:
                d[rng.random(nc) < 0.5] = 0.0
            if variant == 2:
                d[:] = 0.0          # no information: uniform
            if variant == 3:
                d[nc // 2] = np.inf  # not finite: uniform
            off = oracle.Config.strat_alloc(d, N)
            n = np.diff(off)
            assert off[0] == 0 and off[-1] == N and n.min() >= 2, (nc, N, variant)
            if variant >= 2:
                np.testing.assert_array_equal(off, oracle.Config.strat_alloc(np.ones(nc), N, True))
                assert n.max() - n.min() <= 1
            elif N > 2 * nc:
                # the definition, in exact rational arithmetic on the doubles
                from fractions import Fraction
                if nc <= 1000:
                    P = sum(Fraction(v) for v in d)
                    run, prev = Fraction(0), 0
                    for h in range(nc):
                        run += Fraction(d[h])
                        fl = (N - 2 * nc) if h == nc - 1 else math.floor((N - 2 * nc) * run / P)
                        assert abs(n[h] - (2 + fl - prev)) <= 1   # (long double against exact: a floor may land on the other side)
                        prev += n[h] - 2
    with pytest.raises(ValueError):
        oracle.Config.strat_alloc(np.ones(8), 15)


def test_hypercube_means_of_a_separable_polynomial(oracle):
    """f = x0^2 (1 + x1) on the untrained map of [0, 1]^2 (x = y, J = 1): the mean over the cell [a, b] x [c, e] is
    (b^3 - a^3) / (3 (b - a)) * (1 + (c + e) / 2)"""
    cfg = oracle.Config([ocont()], [[2]])
    f = oracle.compile_c_integrand("w[0] = x[0] * x[0] * (1.0 + x[1]);")
    ns, N = [5, 4], 40000
    off = oracle.Config.strat_alloc(np.ones(20), N, True)
    r = cfg.strat_iteration(f, None, SEED, 0, 0, ns, off)
    n = np.diff(off)
    h = np.arange(20)
    i0, i1 = h % 5, h // 5
    a, b, c, e = i0 / 5.0, (i0 + 1) / 5.0, i1 / 4.0, (i1 + 1) / 4.0
    exact = (b ** 3 - a ** 3) / (3 * (b - a)) * (1 + (c + e) / 2)
    err = np.sqrt(r["v2"][:, 0] / n)
    assert np.all(np.abs(r["S1"][:, 0] / n - exact) < 5 * err), (r["S1"][:, 0] / n - exact) / err
    assert abs(r["mean"][0] - 0.5) < 5 * math.sqrt(r["var"][0])     # int x0^2 (1 + x1) = 1/3 * 3/2
    # the two-pass variance against numpy's on the recomputed samples of one hypercube
    rs = cfg.strat_iteration(f, None, SEED, 0, 0, ns, off, samples=True)
    fj = rs["w"][off[7]:off[8], 0] * rs["jac"][off[7]:off[8]]
    assert rs["v2"][7, 0] == pytest.approx(np.var(fj, ddof=1), rel=1e-12)
    assert rs["d"][7] == pytest.approx(np.var(fj, ddof=1) ** 0.375, rel=1e-12)


@pytest.mark.parametrize("nstrat", [[5, 1, 3], [2, 2, 2, 2], [251, 3], [1, 1, 7], [37]])
def test_cell_decode(oracle, nstrat):
    D, nc = len(nstrat), int(np.prod(nstrat))
    cfg = oracle.Config([ocont()], [[D]])
    f = oracle.compile_c_integrand("w[0] = 1.0;")
    off = oracle.Config.strat_alloc(np.ones(nc), 3 * nc, True)
    r = cfg.strat_iteration(f, None, 3, 0, 0, nstrat, off, samples=True)
    h = np.repeat(np.arange(nc), 3)
    cell = np.stack(np.unravel_index(h, nstrat, order="F"), axis=1)
    np.testing.assert_array_equal(np.floor(r["y"] * np.array(nstrat, dtype=np.float64)).astype(np.int64), cell)
    assert np.all(r["y"] < 1.0)


CAP_CASES = [(64, 8192), (24389, 200000), (528529, 2 ** 22 + 5)]


@pytest.mark.parametrize("nc,N", CAP_CASES)
@pytest.mark.parametrize("zeros", [False, True])
def test_cap_of_the_allocation_comparison(oracle, nc, N, zeros):
    """The kernel adds d_h in tile / stretch order in double, the oracle in index order in long double: a floor() of C_h can land one
    sample to either side.  The GPU comparison allows |delta n_h| <= 1 on at most max(2, ncube / 1000) hypercubes; here the kernel's
    order is emulated in numpy and the differences are counted (printed: run with -s)."""
    rng = np.random.default_rng(nc + (7 if zeros else 0))
    d = rng.lognormal(0.0, 3.0, nc) ** 0.375
    if zeros:
        d[rng.random(nc) < 0.5] = 0.0
    ref = np.diff(oracle.Config.strat_alloc(d, N))
    emu = np.diff(kernel_order_alloc(d, N))
    ndiff = int(np.count_nonzero(ref != emu))
    print("cap: ncube %d N %d zeros %s: %d hypercubes differ, max |delta| %d" % (nc, N, zeros, ndiff, int(np.abs(ref - emu).max())))
    assert emu.sum() == N and emu.min() >= 2
    assert np.abs(ref - emu).max() <= 1 and ndiff <= max(2, nc // 1000)
