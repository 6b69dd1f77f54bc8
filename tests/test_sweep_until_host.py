"""CPU tests of :vegas sweep points that stop at a target error (mci_integrate_sweep_until; csrc/mci_sweep_common.h, the lines between the
`sweep until rule` markers): the stop rule compiled for the host and held to the oracle's own mean_std / average on the statistics heads
of oracle runs, case by case with the margin every decision keeps from its threshold; a NaN column, the first legal iteration and
min_niter; every refusal of the new query on offline engines; the declarations in include/mci.h and their comments; the two new
translation units cross-compiled for gfx950 through the library's own JIT; the ValueErrors of mci.integrate_sweep."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from until_cases import CASES, MARGIN, SEED, KW, oracle_heads, reference_stops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mcintegration.jl_amd", "csrc", "mci_sweep_common.h")
BEGIN, END = "// >>> sweep until rule", "// <<< sweep until rule"

WRAP = r"""
#include <cmath>
#include <math.h>
using std::isfinite;
#define __host__
#define __device__
%s
// mci_mean_std of a statistics head's columns
extern "C" void head_mean_std(const double *sum, const double *sq, int nobs, int nblocks, double *m, double *s) {
    for (int o = 0; o < nobs; ++o) sweep_until_mean_std(sum[o], sq[o], nblocks, m[o], s[o]);
}
// a point's loop as the kernel runs it: heads [niter][2 nobs] (sum | sum of squares), sums [2 nobs] zeroed by the caller; returns the
// iteration (1-based) the point stops at, 0 when it never does
extern "C" int stop_at(const double *heads, int niter, int nobs, int nblocks, int ignore, int min_niter, double rtol, double atol, double *sums) {
    for (int n = 1; n <= niter; ++n) {
        const double *h = heads + (long)(n - 1) * 2 * nobs;
        int wait = 0;
        for (int o = 0; o < nobs; ++o) {
            double m, s;
            sweep_until_mean_std(h[o], h[nobs + o], nblocks, m, s);
            sweep_until_add(m, s, n, ignore, sums[o], sums[nobs + o]);
            if (!sweep_until_done(sums[o], sums[nobs + o], n, ignore, min_niter, rtol, atol)) wait = 1;
        }
        if (!wait) return n;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_sweep_common.h: the marker lines around the stop rule are gone"
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi
    for fn in ("sweep_until_mean_std(", "sweep_until_add(", "sweep_until_done("):
        assert fn in text[lo:hi] and fn in text[hi:], fn            # the kernels' sweep_until_columns goes through the rule
    for name in ("mci_sweep.h", "mci_sweep_leaves.h"):
        assert "sweep_until_columns(" in open(os.path.join(os.path.dirname(HEADER), name)).read(), name
    d = tmp_path_factory.mktemp("until_rule")
    src, so = os.path.join(d, "until_host.cpp"), os.path.join(d, "until_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % text[lo:hi])
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.head_mean_std.restype, lib.head_mean_std.argtypes = None, [dp, dp, C.c_int, C.c_int, dp, dp]
    lib.stop_at.restype = C.c_int
    lib.stop_at.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, dp]

    class Rule:
        @staticmethod
        def mean_std(sum_, sq, nblocks):
            s, q = np.ascontiguousarray(sum_, dtype=np.float64), np.ascontiguousarray(sq, dtype=np.float64)
            m, e = np.empty_like(s), np.empty_like(s)
            lib.head_mean_std(s.ctypes.data_as(dp), q.ctypes.data_as(dp), s.size, int(nblocks), m.ctypes.data_as(dp), e.ctypes.data_as(dp))
            return m, e

        @staticmethod
        def stop(heads, nblocks, ignore=1, min_niter=0, rtol=0.0, atol=0.0):
            h = np.ascontiguousarray(heads, dtype=np.float64)
            niter, two = h.shape
            sums = np.zeros(two)
            return lib.stop_at(h.ctypes.data_as(dp), niter, two // 2, int(nblocks), int(ignore), int(min_niter), float(rtol), float(atol),
                               sums.ctypes.data_as(dp))
    return Rule


# ---- the rule against the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(CASES))
def test_the_rule_decides_as_the_oracles_average_does(oracle, rule, case):
    c = CASES[case]
    for k, want in zip(c["ks"], c["stops"]):
        heads = oracle_heads(oracle, case, k)
        nobs = heads.shape[1] // 2
        im = np.array([oracle.mean_std(h[:nobs], h[nobs:], KW["block"])[0] for h in heads])
        ie = np.array([oracle.mean_std(h[:nobs], h[nobs:], KW["block"])[1] for h in heads])
        for h, m, e in zip(heads, im, ie):         # mci_mean_std itself: bit for bit
            rm, re_ = rule.mean_std(h[:nobs], h[nobs:], KW["block"])
            assert rm.tobytes() == m.tobytes() and re_.tobytes() == e.tobytes()
        stop, margin = reference_stops(oracle, im, ie, c["rtol"], c["atol"], ignore=1)
        print("%s k = %d: oracle stop %s, nearest decision %.1f %% from its threshold" % (case, k, stop or "none", 100 * margin))
        assert margin >= MARGIN, (case, k, margin)
        assert stop == want, (case, k, stop, want)
        assert rule.stop(heads, KW["block"], ignore=1, rtol=c["rtol"], atol=c["atol"]) == stop


def test_the_two_column_case_is_decided_by_the_bounds_it_was_chosen_for(oracle):
    """k = 0: column 1's relative bound is the larger one; k = 1, 2, 3: its absolute bound"""
    c = CASES["two_columns"]
    for k in (0, 1, 2, 3):
        heads = oracle_heads(oracle, "two_columns", k)
        m, e = oracle.mean_std(heads[:, 1], heads[:, 3], KW["block"])
        M = oracle.average(m, e, init=2, max=10)[0]
        assert (c["rtol"] * abs(M) > c["atol"]) == (k == 0), (k, M)


def test_a_nan_column_never_converges(oracle, rule):
    heads = oracle_heads(oracle, "two_columns", 3).copy()
    assert rule.stop(heads, 16, rtol=1e9) == 3
    bad = heads.copy()
    bad[:, 1] = np.nan                              # column 1's sum in every iteration
    assert rule.stop(bad, 16, rtol=1e9, atol=1e9) == 0
    late = heads.copy()
    late[4, 3] = np.inf                             # one iteration's sum of squares: infinite error, weight 0 -- the others still count
    assert rule.stop(late, 16, rtol=1e9) == 3
    poisoned = heads.copy()
    poisoned[1, 0] = np.inf                         # an infinite mean in the first counted iteration stays in M for good
    assert rule.stop(poisoned, 16, rtol=1e9, atol=1e9) == 0
    zero = np.zeros_like(heads)                     # an identically-zero integrand: E = 1e-10 / sqrt(n), M = 0 -- atol decides
    assert rule.stop(zero, 16, rtol=1.0, atol=0.0) == 0 and rule.stop(zero, 16, rtol=0.0, atol=1e-9) == 3


def test_the_first_legal_iteration_and_min_niter(oracle, rule):
    heads = oracle_heads(oracle, "two_columns", 4)
    huge = dict(rtol=1e9, atol=0.0)
    assert rule.stop(heads, 16, ignore=1, **huge) == 3             # ignore + 2
    assert rule.stop(heads, 16, ignore=0, **huge) == 2
    assert rule.stop(heads, 16, ignore=4, **huge) == 6
    assert rule.stop(heads, 16, ignore=9, **huge) == 0             # fewer than two averaged iterations within niter = 10
    assert rule.stop(heads[:2], 16, ignore=1, **huge) == 0
    assert rule.stop(heads, 16, ignore=1, min_niter=6, **huge) == 6
    assert rule.stop(heads, 16, ignore=1, min_niter=2, **huge) == 3  # (never below ignore + 2)
    assert rule.stop(heads, 16, ignore=1, min_niter=11, **huge) == 0
    assert rule.stop(heads, 16, ignore=1, rtol=0.0, atol=0.0) == 0   # a zero target stops nothing
    c = CASES["two_columns"]
    assert rule.stop(heads, 16, ignore=1, min_niter=5, rtol=c["rtol"], atol=c["atol"]) == 5      # (converged at 3: held back)


# ---- the query -----------------------------------------------------------------------------------------------------------------------

def genz4():
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]]), mci.catalog.genz_product_peak(4), device=-1)


def mixed():
    from test_hip_sweep_leaves import MIXED_BODY, mixed_row
    cfg = mci.Configuration(var=(mci.Continuous(0.0, 1.0, ninc=65, alpha=1.5), mci.Continuous(0.0, 2.0, alpha=2.0), mci.Discrete(1, 7)), dof=[[1, 1, 1]])
    return mci.Engine(cfg, mci.Integrand(MIXED_BODY, mixed_row(0), "mixed"), device=-1)


def test_every_refusal_of_the_new_query():
    from mcintegration_jl_amd._lib import IntegrateArgs, lib
    eng = genz4()
    assert eng.sweep_until_supported() is None                                  # rtol = atol = 0: legal
    assert eng.sweep_until_supported(rtol=1e-3, atol=1e-6, min_niter=4) is None
    for kw, words in ((dict(rtol=-1e-3), "rtol is negative or not finite"), (dict(rtol=float("nan")), "rtol is negative or not finite"),
                      (dict(rtol=float("inf")), "rtol is negative or not finite"), (dict(atol=-1.0), "atol is negative or not finite"),
                      (dict(atol=float("nan")), "atol is negative or not finite"), (dict(atol=float("inf")), "atol is negative or not finite"),
                      (dict(min_niter=-1), "min_niter < 0")):
        assert eng.sweep_until_supported(**kw) == words, kw
    # a NULL target
    a = eng._integrate_args("vegas", 10000, 10, 16, -1, True, 1.0, 1, 0, 0)
    why = C.create_string_buffer(256)
    assert lib().mci_sweep_until_supported(eng.p, C.byref(a), None, why, len(why)) == 1 and why.value == b"the target is NULL"
    assert b"cannot run to a target error: the target is NULL" in lib().mci_last_error()
    # whatever mci_sweep_supported refuses, with that reason -- and before the target is looked at
    for kw in (dict(solver="vegasmc"), dict(measurefreq=2), dict(niter=0)):
        assert eng.sweep_until_supported(rtol=-1.0, **kw) == eng.sweep_supported(**kw) != None, kw
    eng.set_stratification()
    assert eng.sweep_until_supported(rtol=1e-3) == "the problem is stratified (mci_set_stratification_off first)"
    eng.set_stratification(on=False)
    m = mixed()
    assert m.sweep_until_supported(rtol=1e-3) == m.sweep_supported() and "3 variable leaves" in m.sweep_supported()
    m.set_sweep_leaves("all")
    assert m.sweep_until_supported(rtol=1e-3) is None
    # the per-wave histogram copies that make a point's bytes independent of the waves' schedule take LDS: named where they do not fit
    big = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0, ninc=1500), dof=[[2]]), mci.catalog.x2y2(), device=-1)
    assert big.sweep_supported() is None
    why = re.search(r"one histogram copy per wave .* take (\d+) bytes of LDS \((\d+) at most\)", big.sweep_until_supported(rtol=1e-3))
    assert why and int(why.group(1)) > big.sweep_lds_bytes() and int(why.group(1)) > int(why.group(2)) == 64 * 1024
    with pytest.raises(mci.MCIError, match="one histogram copy per wave"):
        big.compile("vegas_sweep_until")             # the unit's own query, not the loader, says why
    big.compile("vegas_sweep")
    with pytest.raises(mci.MCIError, match="one histogram copy per wave"):
        big.integrate_sweep_until("vegas", userdata=np.ones((2, len(big.integrand.userdata))), rtol=1e-3)
    from test_sweep_leaves_host import bubble
    b = bubble()
    b.set_sweep_leaves("all")
    assert b.sweep_supported() is None
    why = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", b.sweep_until_supported(rtol=1e-3))
    assert why and int(why.group(1)) > int(why.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="one histogram copy per wave"):
        b.compile("vegas_sweep_leaves_until")
    # the entry point: the same refusals, then the missing device
    ud = np.ones((2, len(eng.integrand.userdata)))
    with pytest.raises(mci.MCIError, match="rtol is negative"):
        eng.integrate_sweep_until("vegas", userdata=ud, rtol=-1.0)
    with pytest.raises(mci.MCIError, match="solver is not :vegas"):
        eng.integrate_sweep_until("vegasmc", userdata=ud, rtol=1e-3)
    with pytest.raises(mci.MCIError) as e:              # eligible: only the device is missing
        eng.integrate_sweep_until("vegas", userdata=ud, rtol=1e-3)
    assert e.value.code == 7
    # nothing about the fixed sweep's query moved
    assert eng.sweep_supported() is None and ":vegas" in eng.sweep_supported(solver="mcmc")


def test_header_entries_and_their_comments():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGAS_SWEEP_UNTIL = 17, MCI_VEGAS_SWEEP_LEAVES_UNTIL = 18 \};", hdr)
    assert re.search(r"typedef struct \{\s*double rtol, atol;[^}]*int32_t min_niter;[^}]*\} mci_sweep_target;", hdr)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_integrate_sweep_until\(mci_problem \*prob, const mci_integrate_args \*args, const mci_sweep_target \*target, "
                  r"int32_t npoint,\s*const double \*userdata, const uint64_t \*seeds, const double \*maps_in, double \*maps_out, mci_result \*results,\s*"
                  r"double \*iter_mean, double \*iter_std, int32_t \*status, int32_t \*niter_run\);", hdr, re.S)
    assert m
    for needle in ("statistics.jl:186-204", "statistics.jl:189-191", "main.jl:297-317", "ignore + 2", "min_niter", "max(atol, rtol |M|)", "NaN or infinite",
                   "never converges", "niter = n_p", "are zero", "capacity", "niter_run", "train!", "MCI_VEGAS_SWEEP_UNTIL", "MCI_VEGAS_SWEEP_LEAVES_UNTIL"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_until_supported\(const mci_problem \*prob, const mci_integrate_args \*args, "
                  r"const mci_sweep_target \*target, char \*why, int32_t n\);", hdr, re.S)
    assert m
    for needle in ("mci_sweep_supported", "NULL target", "negative", "not finite", "min_niter < 0", "rtol = atol = 0", "never stops"):
        assert needle in m.group(1), needle
    from mcintegration_jl_amd import _lib
    for name in ("mci_integrate_sweep_until", "mci_sweep_until_supported"):
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().mci_abi_version() == _lib.ABI_VERSION     # (two functions and one structure more, none changed)
    common = open(HEADER).read()
    assert "no counter anybody waits for" in common and "no grid-wide counters" not in common
    jit = open(os.path.join(ROOT, "mcintegration.jl_amd", "csrc", "mci_jit.h")).read()
    assert re.search(r'kUnitSweepUntil\s*\*/ \{"mci_sweep.h",.*"mci_vegas_sweep_until", "SweepUntilArgs", "f", "vegas_sweep_until", 1, true, 1, true, true, true\}', jit)
    assert re.search(r'kUnitSweepLeavesUntil\s*\*/ \{"mci_sweep_leaves.h",.*"mci_vegas_sweep_leaves_until", "SweepUntilArgs", "f", "vegas_sweep_leaves_until", 1, false, 2, true, false, true\}', jit)


# ---- the two new translation units ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("unit", ["vegas_sweep_until", "vegas_sweep_leaves_until"])
def test_the_units_cross_compile_for_gfx950(unit):
    leaves = unit == "vegas_sweep_leaves_until"
    eng = mixed() if leaves else genz4()
    fixed = "vegas_sweep_leaves" if leaves else "vegas_sweep"
    if leaves:
        with pytest.raises(mci.MCIError, match="variable leaves"):
            eng.compile(unit)                    # not opted in: what mci_sweep_supported says
        eng.set_sweep_leaves("all")
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object(unit)
    eng.compile(unit)                            # (the library refuses a unit that comes out with static LDS or scratch)
    path = eng.code_object(unit)
    blob = open(path, "rb").read()
    kernel = b"mci_" + unit.encode()
    assert blob[:4] == b"\x7fELF" and kernel + b"\0" in blob and b"gfx950" in blob
    for other in (b"mci_vegas_sweep\0", b"mci_vegas_sweep_leaves\0", b"mci_vegas_sweep_strat", b"mci_vegas_batch", b"mci_vegas_persist"):
        assert other not in blob, other
    at = blob.index(b".name\xbc" + kernel if leaves else b".name\xb5" + kernel)     # (msgpack str8 / fixstr headers of the two names' lengths)
    for key in (b".private_segment_fixed_size", b".group_segment_fixed_size"):
        k = blob.rindex(key, 0, at) if key == b".group_segment_fixed_size" else blob.index(key, at)
        assert blob[k + len(key)] == 0, key
    with pytest.raises(mci.MCIError):
        eng.code_object(fixed)                   # compiling the new unit compiles no other
    eng.compile(fixed)
    was = open(eng.code_object(fixed), "rb").read()
    assert eng.code_object(fixed) != path and kernel not in was
    with pytest.raises(mci.MCIError, match="mci_set_sweep_leaves"):
        eng.compile("vegas_sweep_until" if leaves else "vegas_sweep_leaves_until")      # the other layout's unit
    eng.close()


# ---- mci.integrate_sweep(rtol=..., atol=..., min_niter=...) --------------------------------------------------------------------------

X2Y2P = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
ROWS = [[1.0], [0.5], [0.25]]


def kw2():
    return dict(var=mci.Continuous(0.0, 1.0), dof=[[2]], device=-1)


def test_the_keywords_of_integrate_sweep_raise_where_they_do_not_apply():
    f = mci.Integrand(X2Y2P, [1.0])
    with pytest.raises(ValueError, match="min_niter= belongs to a target error"):
        mci.integrate_sweep(f, ROWS, min_niter=4, **kw2())
    for solver in ("vegasmc", "mcmc"):
        with pytest.raises(ValueError, match=r"solver is not :vegas \(chain solvers are not swept\)"):
            mci.integrate_sweep(f, ROWS, solver=solver, rtol=1e-3, **kw2())
    with pytest.raises(ValueError, match="stratify= do not go together"):
        mci.integrate_sweep(f, ROWS, rtol=1e-3, stratify=True, **kw2())
    with pytest.raises(ValueError, match="solver is not :vegas"):
        mci.integrate_sweep(f, ROWS, solver="vegasmc", atol=1e-3, chains=4, **kw2())
    with pytest.raises(ValueError, match="solver is not :vegas"):
        mci.integrate_sweep(f, ROWS, solver="mcmc", atol=1e-3, mcmc_chains=4, **kw2())
    # the target itself: in the words of mci_sweep_until_supported
    with pytest.raises(ValueError, match="rtol is negative or not finite"):
        mci.integrate_sweep(f, ROWS, rtol=-1e-3, **kw2())
    with pytest.raises(ValueError, match="atol is negative or not finite"):
        mci.integrate_sweep(f, ROWS, atol=float("nan"), **kw2())
    with pytest.raises(ValueError, match="min_niter < 0"):
        mci.integrate_sweep(f, ROWS, rtol=1e-3, min_niter=-2, **kw2())
    with pytest.raises(ValueError, match="min_niter must be an int"):
        mci.integrate_sweep(f, ROWS, rtol=1e-3, min_niter=2.5, **kw2())
    with pytest.raises(mci.MCIError) as e:            # checked, bound, eligible: only the device is missing
        mci.integrate_sweep(f, ROWS, rtol=1e-3, atol=1e-6, min_niter=4, **kw2())
    assert e.value.code == 7


def test_a_refused_sweep_raises_instead_of_looping_without_the_target(monkeypatch):
    """two Continuous leaves without leaves="all", measurefreq = 2: integrate_sweep would loop over integrate(), which has no such stop"""
    import sys
    I = sys.modules[mci.integrate.__module__]
    monkeypatch.setattr(I, "integrate", lambda *a, **k: pytest.fail("the loop of integrate() calls ran in the sweep's place"))
    f = mci.Integrand(X2Y2P, [1.0])
    def two():      # (a variable object per call: one that lives in an open engine is not copied)
        return dict(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], device=-1)
    with pytest.raises(ValueError, match=r"does not run as a sweep \(2 variable leaves.*rtol= / atol= need the batched form"):
        mci.integrate_sweep(f, ROWS, rtol=1e-3, **two())
    with pytest.raises(ValueError, match=r"does not run as a sweep \(measurefreq = 2.*need the batched form"):
        mci.integrate_sweep(f, ROWS, atol=1e-3, measurefreq=2, **kw2())
    with pytest.raises(mci.MCIError) as e:            # opted in: eligible
        mci.integrate_sweep(f, ROWS, rtol=1e-3, leaves="all", **two())
    assert e.value.code == 7


def test_report_prints_the_rows_it_has_and_says_when_the_target_was_missed():
    import io
    from mcintegration_jl_amd.statistics import Result, report
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]])
    im, ie = np.array([[1.0], [1.1], [1.05], [1.02]]), np.array([[0.1], [0.05], [0.04], [0.03]])
    r = Result(im, ie, cfg, 1)
    assert r.niter_run is None and r.converged is None
    r.niter_run, r.converged = 4, False
    out = io.StringIO()
    report(r, io=out)
    text = out.getvalue()
    assert len(re.findall(r"^\s*(?:ignore|\d+)\s+\S+ ± ", text, re.M)) == 4
    assert "ran all 4 iterations it was given without reaching its target error" in text
    assert r.with_ignore(0).converged is False and r.with_ignore(0).niter_run == 4
    r.converged = True
    out = io.StringIO()
    report(r, io=out)
    assert "target error" not in out.getvalue()
