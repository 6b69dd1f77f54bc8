"""The cases tests/test_sweep_until_host.py (CPU) and tests/test_hip_sweep_until.py (GPU) hold sweep points with a target error to, and
the reference side of both: a point's stop derived from per-iteration means and errors with the oracle's own average(), together with
the margin the nearest decision keeps from its threshold.

Every case: neval = 16000, niter = 10, block = 16, ignore = 1, seed 20240229.  The inputs were chosen with the CPU oracle's loop so that
no decision "converged at n or not yet" sits within 5 % of its threshold -- the sweep follows the oracle's loop to 1e-4 (mean) and 1e-2
(error) over a run (check_run of tests/test_hip_sweep.py), so a decision that close could go either way.  Points that break the margin
are left out by name below; run the CPU test with -s after changing a case: it prints every point's margin."""
import numpy as np

SEED = 20240229
KW = dict(neval=16 * 1000, niter=10, block=16)
MARGIN = 0.05

TWO_BODY = "w[0] = x[0]*x[0] + ud[0]*x[1]*x[1]; w[1] = exp(-ud[1]*(x[0] + x[1])) - ud[2];"


def two_row(k):
    return [1.0 + k, 2.0 + 3.0 * k, 0.0]


# ks: the scan points; stops: the iteration each stops at (0: not within niter = 10)
CASES = {
    # point(k) of tests/test_hip_sweep.py (4-D Genz product peak); k = 2 is left out: 4.6 % from the threshold
    "genz": dict(ks=[0, 1, 3, 4, 6], rtol=1.75e-3, atol=0.0, stops=[3, 0, 3, 5, 4]),
    # MIXED_BODY / MIXED_LEAVES / mixed_row(k) of tests/test_hip_sweep_leaves.py; k = 4 is left out: 4.8 %
    "mixed": dict(ks=[0, 1, 2, 3, 5], rtol=1e-3, atol=0.0, stops=[4, 5, 5, 4, 5]),
    # two integrands over one Continuous pool: at k = 0 column 1's relative bound decides, at k = 1, 2, 3 its absolute one
    "two_columns": dict(ks=[0, 1, 2, 3, 4], rtol=2.2e-3, atol=3.2e-4, stops=[0, 0, 5, 3, 3]),
}


def row(case, k):
    if case == "genz":
        from test_hip_sweep import point
        return point(k)
    if case == "mixed":
        from test_hip_sweep_leaves import mixed_row
        return mixed_row(k)
    return two_row(k)


def _oracle_problem(oracle, case):
    cont = dict(kind=0, pool=0, lower=0.0, upper=1.0)
    if case == "genz":
        return oracle.Config([cont], [[4]]), "genz_product_peak"
    if case == "mixed":
        from test_hip_sweep_leaves import MIXED_BODY, MIXED_LEAVES
        return oracle.Config(MIXED_LEAVES, [[1, 1, 1]]), oracle.compile_c_integrand(MIXED_BODY, 1, "mixed")
    return oracle.Config([cont], [[2], [2]]), oracle.compile_c_integrand(TWO_BODY, 2, "until_two")


_heads = {}


def oracle_heads(oracle, case, k):
    """[niter][2 nobs]: the statistics head (sum | sum of squares of the blocks' means) of every iteration of the oracle's loop
    (main.jl:142-207: iteration, train!) for scan point k -- what the kernel's rule reads of `packed`.  Computed once per point."""
    if (case, k) not in _heads:
        ocfg, f = _oracle_problem(oracle, case)
        ud, block, niter = row(case, k), KW["block"], KW["niter"]
        rows = []
        for it in range(niter):
            packed = ocfg.iteration(oracle.VEGAS, f, ud, KW["neval"] // block, 0, block, it, SEED)
            ocfg.train()
            rows.append(packed)
        nobs = int(ocfg.c.nobs)
        heads = np.array([r[:2 * nobs] for r in rows])
        # (the loop above IS the oracle's integrate(): the same means and errors, bit for bit)
        ocfg2, f2 = _oracle_problem(oracle, case)
        o = ocfg2.integrate(oracle.VEGAS, f2, ud, seed=SEED, **KW)
        im = np.array([oracle.mean_std(h[:nobs], h[nobs:], block)[0] for h in heads])
        ie = np.array([oracle.mean_std(h[:nobs], h[nobs:], block)[1] for h in heads])
        assert im.tobytes() == o["iter_mean"].tobytes() and ie.tobytes() == o["iter_std"].tobytes(), (case, k)
        heads.setflags(write=False)
        _heads[(case, k)] = heads
    return _heads[(case, k)]


def reference_stops(oracle, iter_mean, iter_std, rtol, atol, ignore=1, min_niter=0):
    """(stop, margin) of one point from its per-iteration means and errors [niter][nobs]: the first n >= max(ignore + 2, min_niter) at
    which E_o <= max(atol, rtol |M_o|) for every column, (M, E) = oracle.average(..., init = ignore + 1, max = n), or 0; and the smallest
    |E_o / max(atol, rtol |M_o|) - 1| over every column and n >= ignore + 2 up to the stop (a bound of zero counts as infinitely far)"""
    im, ie = np.asarray(iter_mean), np.asarray(iter_std)
    niter, nobs = im.shape
    margin, stop = np.inf, 0
    for n in range(ignore + 2, niter + 1):
        done = True
        for o in range(nobs):
            M, E, _ = oracle.average(im[:, o], ie[:, o], init=ignore + 1, max=n)
            bound = max(atol, rtol * abs(M))
            if not (np.isfinite(M) and np.isfinite(E)):
                done = False
                continue
            if bound > 0.0:
                margin = min(margin, abs(E / bound - 1.0))
            done = done and E <= bound
        if done and n >= min_niter:
            stop = n
            break
    return stop, margin
