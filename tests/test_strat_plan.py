"""CPU tests of stratified :vegas (VEGAS+): the default plan of mci_strat_plan against its rule written out in numpy, and the
refusals of integrate(stratify=...) that come before any engine (and any device) exists."""
import ctypes as C
import math

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import _lib


def plan_rule(neval, ndim, max_nhcube):
    """the default plan: s = floor(min(N/8, max_nhcube)^(1/D)) (at least 1) strata per draw, then the leading draws raised to s + 1 one
    at a time while the hypercube count stays within min(N/8, max_nhcube) -- eight samples per hypercube on average"""
    cap = min(neval // 8, max_nhcube)
    s = max(1, int(math.floor(cap ** (1.0 / ndim))))
    while s > 1 and s ** ndim > cap:     # (the floating-point root may land one off)
        s -= 1
    while (s + 1) ** ndim <= cap:
        s += 1
    ns = np.full(ndim, s, dtype=np.int64)
    for d in range(ndim):
        trial = ns.copy()
        trial[d] = s + 1
        if np.prod(trial) > cap:
            break
        ns = trial
    return ns


def lib_plan(neval, ndim, max_nhcube):
    out = (C.c_int32 * ndim)()
    _lib.check(mci.lib().mci_strat_plan(int(neval), int(ndim), int(max_nhcube), out))
    return np.array(list(out), dtype=np.int64)


@pytest.mark.parametrize("neval", [10 ** 4, 10 ** 6, 10 ** 8, 8192, 12345])
@pytest.mark.parametrize("ndim", [1, 2, 3, 4, 7, 16, 32])
@pytest.mark.parametrize("max_nhcube", [2 ** 24, 1000, 1])
def test_default_plan_matches_rule(neval, ndim, max_nhcube):
    got = lib_plan(neval, ndim, max_nhcube)
    want = plan_rule(neval, ndim, max_nhcube)
    np.testing.assert_array_equal(got, want)
    assert np.prod(got) <= min(neval // 8, max_nhcube)
    assert got.min() >= 1 and got.max() - got.min() <= 1
    assert np.all(np.diff(got) <= 0)   # the leading draws carry the extra stratum


def test_plan_examples():
    np.testing.assert_array_equal(lib_plan(10 ** 4, 1, 2 ** 24), [1250])
    np.testing.assert_array_equal(lib_plan(10 ** 4, 3, 2 ** 24), [11, 11, 10])
    np.testing.assert_array_equal(lib_plan(2 * 10 ** 5, 3, 2 ** 24), [29, 29, 29])           # benchmark1: 24389 hypercubes
    np.testing.assert_array_equal(lib_plan(10 ** 8, 16, 2 ** 24), [3] * 12 + [2] * 4)   # C2: 3^12 * 2^4 = 8503056 hypercubes


def test_plan_refuses_too_few_samples():
    with pytest.raises(mci.MCIError):
        lib_plan(7, 3, 2 ** 24)
    with pytest.raises(mci.MCIError):
        lib_plan(100, 0, 2 ** 24)


class _NoEngine:
    """engine_factory that fails the test if integrate() gets as far as building an engine"""

    def __call__(self, *a, **k):
        raise AssertionError("an engine was created before the refusal")


@pytest.mark.parametrize("case", ["mcmc", "vegasmc", "discrete", "measurefreq", "measure", "host", "bad"])
def test_stratify_refusals_before_any_engine(case):
    kw = dict(solver="vegas", var=mci.Continuous(0.0, 1.0), dof=[[2]], neval=1e4, niter=2, stratify=True, engine_factory=_NoEngine())
    f = "w[0] = x[0] * x[1];"
    if case in ("mcmc", "vegasmc"):
        kw["solver"] = case
        match = "solver"
    elif case == "discrete":
        kw["var"] = (mci.Continuous(0.0, 1.0), mci.Discrete(1, 4))
        kw["dof"] = [[1, 1]]
        match = "Discrete"
    elif case == "measurefreq":
        kw["measurefreq"] = 2
        match = "measurefreq"
    elif case == "measure":
        kw["measure"] = mci.Measure("obs_add(0, rw[0]);")
        match = "measure"
    elif case == "host":
        f = lambda x, c: x[0] * x[1]   # noqa: E731
        kw["trace"] = False
        match = "host integrand"
    else:
        kw["stratify"] = "yes"
        match = "Stratify"
    with pytest.raises(ValueError, match=match):
        mci.integrate(f, **kw)


def test_stratify_object():
    s = mci.Stratify(beta=0.5, nstrat=[2, 3], max_nhcube=100)
    assert (s.beta, s.nstrat, s.max_nhcube) == (0.5, [2, 3], 100)
    d = mci.Stratify()
    assert (d.beta, d.nstrat, d.max_nhcube) == (0.75, None, 2 ** 24)


def test_stratify_takes_the_solver_constant():
    # solver given as its constant (integrate() takes both): accepted for :vegas -- the call gets as far as building the engine --,
    # refused for the chain solvers
    kw = dict(var=mci.Continuous(0.0, 1.0), dof=[[2]], neval=1e4, niter=2, stratify=True, engine_factory=_NoEngine())
    with pytest.raises(AssertionError, match="engine was created"):
        mci.integrate("w[0] = x[0] * x[1];", solver=_lib.VEGAS, **kw)
    with pytest.raises(ValueError, match="solver"):
        mci.integrate("w[0] = x[0] * x[1];", solver=_lib.VEGASMC, **kw)
