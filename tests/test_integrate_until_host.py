"""CPU tests of integrate() with a target error (mci_integrate_until; csrc/mci_host_integrate.h, the lines between the `integrate until
rule` markers): the host's stop rule compiled for the host next to the rule text of csrc/mci_sweep_common.h and held, on made-up rows and
block means, to the arithmetic a Result is made of -- the oracle's average() while the call is uncorrelated, mci_lineage_sums +
mci_mean_std through the library's host exports once it is correlated --; every ValueError of the new keywords on offline engines; the
refusals of the new query by name; the entry point on an offline context; the declarations in include/mci.h; the new translation unit
cross-compiled for gfx950 through the library's own JIT."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import _lib
from mcintegration_jl_amd.statistics import lineage_sums, mean_std

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
F = "return x[0] * x[0] + x[1] * x[1];"

WRAP = r"""
#include <cmath>
#include <cstddef>
#include <math.h>
#include "mci.h"
using std::isfinite;
#define __host__
#define __device__
namespace mci {
%s
}
%s
// the loop of mci_integrate_until over rows that are already there: after every n the caller's (mean, stdev, correlated) for niter = n
// stand in res (hook), then the rule; returns the n it stops at, 0 when it never does
extern "C" int stop_at(const mci_sweep_target *t, mci_result *res, int nobs, int niter, int ignore, const double *M, const double *E, const int *corr) {
    double ws[64] = {0.0};
    int added = 0;
    for (int n = 1; n <= niter; ++n) {
        for (int o = 0; o < nobs; ++o) res->mean[o] = M[(n - 1) * nobs + o], res->stdev[o] = E[(n - 1) * nobs + o];
        res->correlated = corr[n - 1];
        if (integrate_until_met(t, res, nobs, n, ignore, ws, &added)) return n;
    }
    return 0;
}
"""


def between(path, begin, end):
    text = open(path).read()
    assert text.count(begin) == 1 and text.count(end) == 1, (path, begin)
    return text[text.index(begin):text.index(end)]


@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    rule = between(os.path.join(CSRC, "mci_sweep_common.h"), "// >>> sweep until rule", "// <<< sweep until rule")
    met = between(os.path.join(CSRC, "mci_host_integrate.h"), "// >>> integrate until rule", "// <<< integrate until rule")
    assert "mci::sweep_until_add(" in met and "static bool integrate_until_met(" in met
    d = tmp_path_factory.mktemp("integrate_until")
    src, so = os.path.join(d, "until_host.cpp"), os.path.join(d, "until_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % (rule, met))
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.stop_at.restype = C.c_int

    def stop(im, ie, M, E, corr, rtol, atol, ignore=1, min_niter=0):
        im, ie, M, E = (np.ascontiguousarray(v, dtype=np.float64) for v in (im, ie, M, E))
        niter, nobs = im.shape
        corr = np.ascontiguousarray(corr, dtype=np.int32)
        m, s, c2 = np.zeros(nobs), np.zeros(nobs), np.zeros(nobs)
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
        res = _lib.ResultC(niter, nobs, dp(im), dp(ie), dp(m), dp(s), dp(c2), 0, 0.0, None, 0, 0)
        t = _lib.SweepTarget(float(rtol), float(atol), int(min_niter))
        return lib.stop_at(C.byref(t), C.byref(res), nobs, niter, int(ignore), dp(M), dp(E), corr.ctypes.data_as(_lib.c_int32_p))
    return stop


def made_up(seed, niter=12, nobs=3, nblocks=16):
    """rows and block means of a run that narrows: column o's block means scatter around o + 1 with a width that shrinks with n"""
    rng = np.random.default_rng(seed)
    bm = np.empty((niter, nblocks, nobs))
    for n in range(niter):
        bm[n] = (np.arange(nobs) + 1.0) + rng.normal(size=(nblocks, nobs)) * 0.3 / (1.0 + n) * (1.0 + np.arange(nobs))
    s, q = bm.sum(1), (bm * bm).sum(1)
    im = np.array([mean_std(s[n], q[n], nblocks)[0] for n in range(niter)])
    ie = np.array([mean_std(s[n], q[n], nblocks)[1] for n in range(niter)])
    return bm, im, ie


def reference(oracle, bm, im, ie, ignore, correlated_from):
    """(M, E) [niter][nobs] as mci_integrate reports them with niter = n: the oracle's average(); from n = correlated_from on (0: never)
    E is the block-lineage error, through the library's own host exports"""
    niter, nobs = im.shape
    M, E, corr = np.zeros((niter, nobs)), np.zeros((niter, nobs)), np.zeros(niter, dtype=np.int32)
    for n in range(1, niter + 1):
        for o in range(nobs):
            M[n - 1, o], E[n - 1, o], _ = oracle.average(im[:, o], ie[:, o], init=ignore + 1, max=n)
        if correlated_from and n >= correlated_from and n > ignore + 1:
            s1, s2 = lineage_sums(bm[:n], ie[:n], init=ignore + 1, max=n)
            le = mean_std(s1, s2, bm.shape[1])[1]
            E[n - 1] = np.where(le > 0.0, le, E[n - 1])
            corr[n - 1] = 1
    return M, E, corr


def first_stop(M, E, rtol, atol, ignore, min_niter):
    for n in range(max(ignore + 2, min_niter), M.shape[0] + 1):
        m, e = M[n - 1], E[n - 1]
        if np.all(np.isfinite(m) & np.isfinite(e) & (e <= np.maximum(atol, rtol * np.abs(m)))):
            return n
    return 0


@pytest.mark.parametrize("correlated_from", [0, 1, 5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_hosts_rule_reads_what_a_result_reports(oracle, host_rule, seed, correlated_from):
    """at every n the rule's (M, E) are the reference's: uncorrelated -- the running sums against oracle.average, 1e-12 --, correlated --
    the lineage error the library's host exports give; thresholds are put in the middle of the gap between two consecutive n so that no
    decision is near one, and the stop must be the reference's"""
    bm, im, ie = made_up(seed)
    for ignore in (0, 1, 3):
        M, E, corr = reference(oracle, bm, im, ie, ignore, correlated_from)
        # (running sums W | S as sweep_until_add forms them, against average(): what the uncorrelated branch divides)
        w = 1.0 / (ie + 1.0e-10) ** 2
        for n in range(ignore + 2, im.shape[0] + 1):
            W, S = w[ignore:n].sum(0), (w[ignore:n] * im[ignore:n]).sum(0)
            ref = np.array([oracle.average(im[:, o], ie[:, o], init=ignore + 1, max=n)[:2] for o in range(im.shape[1])])
            np.testing.assert_allclose(S / W, ref[:, 0], rtol=1e-12)
            np.testing.assert_allclose(1.0 / np.sqrt(W), ref[:, 1], rtol=1e-12)
        rel = (E / np.abs(M)).max(1)                       # the rtol at which n converges exactly
        stops = set()
        for n in range(ignore + 2, im.shape[0]):
            lo, hi = sorted((rel[n - 1], rel[n]))
            if hi / lo < 1.2:
                continue                                   # (two consecutive n too close to put a threshold between them with 5 % to spare)
            rtol = np.sqrt(lo * hi)
            want = first_stop(M, E, rtol, 0.0, ignore, 0)
            assert host_rule(im, ie, M, E, corr, rtol, 0.0, ignore=ignore) == want, (seed, ignore, n, rtol)
            stops.add(want)
            k = want + 2                                   # min_niter holds the call back
            assert host_rule(im, ie, M, E, corr, rtol, 0.0, ignore=ignore, min_niter=k) == first_stop(M, E, rtol, 0.0, ignore, k)
        assert len(stops) >= 3, stops                      # (the thresholds did move the stop)
        assert host_rule(im, ie, M, E, corr, 0.0, 0.0, ignore=ignore) == 0                    # a zero target never stops
        assert host_rule(im, ie, M, E, corr, 0.0, 1e9, ignore=ignore) == ignore + 2           # atol alone, at the first checkable n
        assert host_rule(im, ie, M, E, corr, 1e9, 0.0, ignore=ignore, min_niter=7) == max(7, ignore + 2)


def test_a_column_that_is_not_finite_never_converges(oracle, host_rule):
    bm, im, ie = made_up(4)
    for corr_from in (0, 1):
        for bad in (np.nan, np.inf):
            im2 = im.copy()
            im2[2, 1] = bad
            M, E, corr = reference(oracle, bm, im2, ie, 1, corr_from)
            assert host_rule(im2, ie, M, E, corr, 1e9, 1e9) == 0
            ie2 = ie.copy()
            ie2[2, 1] = bad
            M, E, corr = reference(oracle, bm, im, ie2, 1, corr_from)
            if not np.all(np.isfinite(E[2:])) or not np.all(np.isfinite(M[2:])):
                assert host_rule(im, ie2, M, E, corr, 1e9, 1e9) == 0


# ---- the keywords ----------------------------------------------------------------------------------------------------------------------

def offline_engine():
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]])
    return cfg, mci.Engine(cfg, mci.Integrand(F), device=-1)


@pytest.mark.parametrize("kw,words", [
    (dict(min_niter=3), "min_niter = 3 without a tolerance"),
    (dict(rtol=1e-3, min_niter=2.5), "min_niter = 2.5: an int >= 0"),
    (dict(rtol=1e-3, min_niter=True), "min_niter = True: an int >= 0"),
    (dict(rtol=1e-3, min_niter=-1), "min_niter < 0"),
    (dict(rtol=-1e-3), "rtol is negative or not finite"),
    (dict(rtol=float("nan")), "rtol is negative or not finite"),
    (dict(atol=float("inf")), "atol is negative or not finite"),
    (dict(rtol=1e-3, atol=-1.0), "atol is negative or not finite"),
])
def test_bad_targets_raise_by_name_before_anything_runs(kw, words):
    cfg, eng = offline_engine()
    cfg._engine = eng
    with pytest.raises(ValueError, match=re.escape(words)):
        mci.integrate(F, config=cfg, solver="vegas", **kw)
    assert cfg.iterations_done == 0


def test_a_target_is_refused_where_the_librarys_loop_does_not_run():
    class Two:
        size, rank = 2, 0

    cfg, _ = offline_engine()
    with pytest.raises(ValueError, match="more than one rank"):
        mci.integrate(F, config=cfg, solver="vegas", rtol=1e-3, comm=Two())
    with pytest.raises(ValueError, match="refused with an engine_factory"):
        mci.integrate(F, config=cfg, solver="vegas", atol=1e-3, engine_factory=lambda *a, **k: None)

    class Bare:      # an engine without the library's loop: integrate() would run its own, host-side one
        integrand = None

        def __init__(self):
            self.ran = 0

        def run(self, *a, **k):
            self.ran += 1

    cfg2 = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]])
    bare = Bare()
    cfg2._engine = bare
    import sys
    mod = sys.modules[mci.integrate.__module__]
    real = mod._bind
    mod._bind = lambda *a, **k: bare
    try:
        with pytest.raises(ValueError, match="refused on the host-loop path"):
            mci.integrate(F, config=cfg2, solver="vegas", rtol=1e-3)
    finally:
        mod._bind = real
    assert bare.ran == 0 and cfg2.iterations_done == 0          # nothing ran un-stopped in the target's place


def test_the_keywords_no_longer_reach_configuration(monkeypatch):
    """integrate(f, rtol=1e-3) used to hand rtol to Configuration(**kwargs) and run all niter iterations"""
    seen = []
    real = mci.Configuration.__init__

    def spy(self, *a, **kw):
        seen.append(sorted(kw))
        real(self, *a, **kw)

    monkeypatch.setattr(mci.Configuration, "__init__", spy)
    calls = []

    class Engine(mci.Engine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, device=-1))

        def integrate(self, *a, **kw):
            calls.append(kw.get("target"))
            raise _lib.MCIError(7, "offline")

        def comm_ranks(self):
            return 1

    import sys
    mod = sys.modules[mci.integrate.__module__]
    monkeypatch.setattr(mod, "Engine", Engine)
    with pytest.raises(_lib.MCIError):
        mci.integrate(F, solver="vegas", var=mci.Continuous(0.0, 1.0), dof=[[2]], rtol=1e-3, min_niter=4)
    assert seen == [["dof", "var"]] and calls == [(1e-3, 0.0, 4)]
    with pytest.raises(_lib.MCIError):
        mci.integrate(F, solver="vegas", var=mci.Continuous(0.0, 1.0), dof=[[2]])
    assert calls[-1] is None                                     # without the keywords: the call it always was


# ---- the library -----------------------------------------------------------------------------------------------------------------------

def test_the_query_names_each_refusal_and_an_offline_context_has_no_device():
    cfg, eng = offline_engine()
    assert eng.integrate_until_supported(rtol=1e-3) is None
    assert eng.integrate_until_supported() is None                                  # rtol = atol = 0 is legal (and never stops a call)
    for solver in ("vegasmc", "mcmc"):
        assert eng.integrate_until_supported(solver=solver, atol=1e-3) is None      # all three solvers
    assert eng.integrate_until_supported(rtol=-1.0) == "rtol is negative or not finite"
    assert eng.integrate_until_supported(rtol=float("inf")) == "rtol is negative or not finite"
    assert eng.integrate_until_supported(atol=float("nan")) == "atol is negative or not finite"
    assert eng.integrate_until_supported(rtol=1e-3, min_niter=-2) == "min_niter < 0"
    assert "should be larger than nblock" in eng.integrate_until_supported(rtol=1e-3, neval=8, block=16)
    eng.set_stratification(nstrat=[2, 2])
    assert eng.integrate_until_supported(rtol=1e-3) is None                         # stratified :vegas too
    assert "solver = :vegas only" in eng.integrate_until_supported(solver="vegasmc", rtol=1e-3)
    assert "measurefreq" in eng.integrate_until_supported(rtol=1e-3, measurefreq=2)
    eng.set_stratification(on=False)
    L = mci.lib()
    a = eng._integrate_args("vegas", 16000, 10, 16, -1, True, 1.0, 1, 1, 0)
    why = C.create_string_buffer(256)
    assert L.mci_integrate_until_supported(eng.p, C.byref(a), None, why, len(why)) == 1 and why.value == b"the target is NULL"
    assert b"cannot run to a target error: the target is NULL" in L.mci_last_error()
    # the entry point: a refusal comes first (the same with and without a device), then MCI_ERR_NO_DEVICE
    n = eng.nobs
    arr = [np.zeros((10, n)), np.zeros((10, n)), np.zeros(n), np.zeros(n), np.zeros(n)]
    dp = lambda v: v.ctypes.data_as(_lib.c_double_p)
    r = _lib.ResultC(10, n, *[dp(v) for v in arr], 0, 0.0, None, 0, 0)
    nrun = C.c_int32(-1)
    bad = _lib.SweepTarget(-1.0, 0.0, 0)
    assert L.mci_integrate_until(eng.p, C.byref(a), C.byref(bad), C.byref(r), C.byref(nrun)) == 1
    good = _lib.SweepTarget(1e-3, 0.0, 0)
    assert L.mci_integrate_until(eng.p, C.byref(a), C.byref(good), C.byref(r), C.byref(nrun)) == 7
    assert b"offline context" in L.mci_last_error() and nrun.value == -1
    with pytest.raises(_lib.MCIError, match="NO_DEVICE"):
        eng.integrate("vegas", 16000, target=(1e-3, None, None))


def test_the_header_declares_the_entry_points_and_keeps_the_abi():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"int mci_integrate_until\(mci_problem \*prob, const mci_integrate_args \*args, const mci_sweep_target \*target, mci_result \*result, int32_t \*niter_run\);", hdr)
    assert re.search(r"int mci_integrate_until_supported\(const mci_problem \*prob, const mci_integrate_args \*args, const mci_sweep_target \*target, char \*why, int32_t n\);", hdr)
    assert "#define MCI_ABI_VERSION 5" in hdr and "enum { MCI_VEGAS_PERSISTENT_UNTIL = 21 };" in hdr
    assert mci.lib().mci_abi_version() == 5
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {"mci_integrate_until", "mci_integrate_until_supported"} <= bound


def test_the_persistent_unit_with_a_target_is_a_code_object_of_its_own():
    """cross-compiled for gfx950 through the library's JIT on an offline engine; the fixed unit's header text is not touched by it (its
    kernel-cache key is made of mci_train.h's text, which the new unit only includes)"""
    cfg, eng = offline_engine()
    eng.compile("vegas_persistent")
    eng.compile("vegas_persistent_until")
    a, b = eng.code_object("vegas_persistent"), eng.code_object("vegas_persistent_until")
    assert a != b and os.path.getsize(b) > 0
    blob = open(b, "rb").read()
    assert b"mci_vegas_persist_until" in blob and b"mci_vegas_persist_until" not in open(a, "rb").read()
    train = open(os.path.join(CSRC, "mci_train.h")).read()
    assert "UNTIL" not in train and "persist_until" not in train
    text = open(os.path.join(CSRC, "mci_persist_until.h")).read()
    assert '#include "mci_sweep_common.h"' in text and "sweep_until_columns(" in text
    jit = open(os.path.join(CSRC, "mci_jit.h")).read()
    assert jit.index("kUnitSweepMcmcResume   */") < jit.index("kUnitVegasPersistUntil */")      # registered behind the standing ones
    cfg2 = mci.Configuration(var=(mci.Continuous(0.0, 1.0), mci.Discrete(1, 4)), dof=[[1, 1]])
    eng2 = mci.Engine(cfg2, mci.Integrand("return x[0] * x[1];"), device=-1)
    with pytest.raises(_lib.MCIError, match="no persistent :vegas kernel"):
        eng2.compile("vegas_persistent_until")


def test_report_says_when_a_call_did_not_reach_its_target():
    import io
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]])
    res = mci.Result(np.array([[1.0], [1.1], [0.9], [1.0]]), np.array([[0.1]] * 4), cfg, 1)
    assert res.niter_run is None and res.converged is None
    res.niter_run, res.converged = 4, False
    out = io.StringIO()
    mci.report(res, io=out)
    assert "ran all 4 iterations it was given without reaching its target error" in out.getvalue()
    res.converged = True
    out = io.StringIO()
    mci.report(res, io=out)
    assert "without reaching" not in out.getvalue()
