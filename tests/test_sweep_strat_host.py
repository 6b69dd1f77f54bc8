"""CPU tests of stratified (VEGAS+) points in :vegas parameter sweeps (mci_integrate_sweep_strat, csrc/mci_sweep_strat.h): the exports
and their comments, the refusals of the classic sweep left as they are, every refusal of the new query on offline engines, the new
translation unit cross-compiled for gfx950 through the library's own JIT, the allocation rule k_strat_alloc and the sweep share compiled
for the host and held bit for bit to the documented order, the cap of the GPU tests' allocation comparison for the reference alone, and
the `stratify` / `alloc` keywords of mci.integrate_sweep."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from strat_cases import kernel_order_alloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mcintegration.jl_amd", "csrc", "mci_strat.h")
BEGIN, END = "// >>> strat alloc rule", "// <<< strat alloc rule"
SEED = 20240229

X2Y2P = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
SUM8 = "double s = 0.0; for (int d = 0; d < 8; ++d) s += (d + 1) * x[d]; w[0] = s * s - 20.0;"
COMPLEX_BODY = "w[0] = x[0]; w[1] = 0.0; w[2] = 0.5 * x[0]; w[3] = x[0] * x[0];"


def offline(cfg, f, **kw):
    return mci.Engine(cfg, f, device=-1, **kw)


def unit(dof, f, **cfgkw):
    return offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=dof, **cfgkw), f)


LAYOUTS = {
    "x2y2": lambda: unit([[2]], mci.catalog.x2y2()),
    "three": lambda: unit([[3]], mci.Integrand("w[0] = x[0] + x[1] * x[2] - 0.5;")),
    "sphere2": lambda: unit([[2], [3]], mci.catalog.sphere2()),
    "sum8": lambda: unit([[8]], mci.Integrand(SUM8)),
    "complex": lambda: unit([[1], [1]], mci.Integrand(COMPLEX_BODY), type=complex),
}


def genz4():
    return unit([[4]], mci.catalog.genz_product_peak(4))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_entries_and_their_comments():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGAS_SWEEP_STRAT = 10 \};", hdr)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_integrate_sweep_strat\(mci_problem \*prob, const mci_integrate_args \*args, int32_t npoint, "
                  r"const double \*userdata, const uint64_t \*seeds,\s*const double \*maps_in, double \*maps_out, const double \*d_in, double \*d_out, "
                  r"int64_t \*counts_out,\s*mci_result \*results, double \*iter_mean, double \*iter_std, int32_t \*status\);", hdr, re.S)
    assert m
    for needle in ("mci_set_stratification", "mci_strat_plan", "d_in", "d_out", "counts_out", "no remap", "not touched", "65536", "4 GiB", "adapt = 0"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_strat_supported\(const mci_problem \*prob, const mci_integrate_args \*args, char \*why, int32_t n\);",
                  hdr, re.S)
    assert m
    for needle in ("not stratified", "measurefreq", "ranks", "host integrand", "user measure", "deterministic", "Continuous", "32 draws", "8 weight columns",
                   "159 KiB"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_strat_doubles\(const mci_problem \*prob, const mci_integrate_args \*args, int64_t \*ncube\);", hdr, re.S)
    assert m and "d_in" in m.group(1)
    from mcintegration_jl_amd._lib import lib
    for name in ("mci_integrate_sweep_strat", "mci_sweep_strat_supported", "mci_sweep_strat_doubles"):
        assert getattr(lib(), name).argtypes is not None


def test_the_classic_sweep_refuses_a_stratified_problem_as_before():
    eng = genz4()
    assert eng.sweep_supported() is None
    eng.set_stratification()
    assert eng.sweep_supported() == "the problem is stratified (mci_set_stratification_off first)"
    with pytest.raises(mci.MCIError, match="stratified"):
        eng.integrate_sweep("vegas", userdata=np.ones((2, len(eng.integrand.userdata))))
    with pytest.raises(mci.MCIError, match="stratified"):
        eng.compile("vegas_sweep")
    assert eng.sweep_strat_supported() is None
    eng.set_stratification(on=False)
    assert eng.sweep_supported() is None and "not stratified" in eng.sweep_strat_supported()


def test_every_refusal_of_the_new_query():
    eng = genz4()
    assert "the problem is not stratified" in eng.sweep_strat_supported()
    with pytest.raises(mci.MCIError, match="not stratified"):
        eng.compile("vegas_sweep_strat")
    with pytest.raises(mci.MCIError, match="not stratified"):
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, len(eng.integrand.userdata))))
    eng.set_stratification()
    assert eng.sweep_strat_supported() is None
    assert ":vegas" in eng.sweep_strat_supported(solver="vegasmc")
    assert "measurefreq = 2" in eng.sweep_strat_supported(measurefreq=2)
    assert "niter" in eng.sweep_strat_supported(niter=0)
    # several Continuous leaves: named as the follow-up it is
    two = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]]), mci.catalog.x2y2())
    two.set_stratification()
    why = two.sweep_strat_supported()
    assert "2 variable leaves" in why and "follow-up" in why
    two.set_sweep_leaves("all")                     # (the opt-in of the classic sweep does not reach this one)
    assert "2 variable leaves" in two.sweep_strat_supported()
    # deterministic mode
    det = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]]), mci.catalog.x2y2(), deterministic=True)
    det.set_stratification()
    assert det.sweep_strat_supported() == "deterministic mode"
    # more hypercubes than neval / 2, with the counts
    eng.set_stratification(nstrat=[10, 10, 10, 10])
    why = eng.sweep_strat_supported(neval=16000)
    assert "10000 hypercubes need at least 20000 samples" in why and "16000" in why
    assert eng.sweep_strat_supported(neval=20000) is None
    assert eng.sweep_strat_plan(20000) == dict(nstrat=[10, 10, 10, 10], ncube=10000, beta=0.75)
    # what a stratified problem cannot have to begin with is refused where it is switched on: a Discrete leaf, a user measure, a host
    # integrand, tiles (tests/test_hip_stratified.py test_refusals_name_their_reason); the query repeats those checks for a problem
    # that changes afterwards
    eng.set_stratification()
    plan = eng.sweep_strat_plan(10000)
    assert plan["nstrat"] == [6, 6, 6, 5] and plan["ncube"] == 1080        # mci_strat_plan for neval = 1e4
    with pytest.raises(mci.MCIError) as e:                                   # eligible: only the device is missing
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, len(eng.integrand.userdata))))
    assert e.value.code == 7
    with pytest.raises(ValueError, match=r"d must be \[points = 2\]\[hypercubes = 1080\]"):
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, len(eng.integrand.userdata))), d=np.ones((2, 1000)))


def test_lds_refusal_names_the_byte_count():
    """a grid of 4400 increments (the most train! takes): the refinement scratch (3 x 4400 + 130 doubles), the merged histogram, the scan
    scratch and the map copy alone are 22 000 doubles"""
    eng = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0, ninc=4400), dof=[[2]]), mci.catalog.x2y2())
    eng.set_stratification()
    why = eng.sweep_strat_supported()
    m = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", why)
    assert m, why
    assert int(m.group(1)) > 22000 * 8 > int(m.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="bytes of LDS"):
        eng.compile("vegas_sweep_strat")
    ok = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0, ninc=3500), dof=[[2]]), mci.catalog.x2y2())
    ok.set_stratification()
    assert ok.sweep_strat_supported() is None          # (above 64 KiB: the launch raises the kernel's dynamic LDS limit)


# ---- the new translation unit --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_unit_cross_compiles_for_gfx950(name):
    eng = LAYOUTS[name]()
    eng.set_stratification()
    with pytest.raises(mci.MCIError):
        eng.code_object("vegas_sweep_strat")     # not compiled yet
    eng.compile("vegas_sweep_strat")             # (the library refuses a unit that comes out with static LDS or scratch)
    path = eng.code_object("vegas_sweep_strat")
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"mci_vegas_sweep_strat" in blob and b"gfx950" in blob
    for other in (b"mci_vegas_sweep\0", b"mci_vegas_sweep_leaves", b"mci_vegas_batch", b"mci_vegas_persist", b"mci_vegas_strat\0", b"k_strat_alloc"):
        assert other not in blob, other
    # the AMDGPU metadata note: no scratch, no static LDS
    at = blob.index(b".name\xb5mci_vegas_sweep_strat")
    for key in (b".private_segment_fixed_size", b".group_segment_fixed_size"):
        k = blob.rindex(key, 0, at) if key == b".group_segment_fixed_size" else blob.index(key, at)
        assert blob[k + len(key)] == 0, key
    eng.compile("vegas_strat")                   # the ordinary stratified unit: another file
    assert eng.code_object("vegas_strat") != path


def test_the_one_grid_sweep_unit_is_what_it_was():
    one = genz4()
    one.compile("vegas_sweep")
    before = one.code_object("vegas_sweep")
    was = open(before, "rb").read()
    strat = genz4()
    strat.set_stratification()
    strat.compile("vegas_sweep_strat")
    assert strat.code_object("vegas_sweep_strat") != before
    strat.set_stratification(on=False)
    strat.compile("vegas_sweep")
    assert strat.code_object("vegas_sweep") == before and open(before, "rb").read() == was
    assert b"mci_vegas_sweep\0" in was and b"mci_vegas_sweep_strat" not in was


# ---- the allocation rule, compiled for the host --------------------------------------------------------------------------------------

WRAP = r"""
#include <cmath>
#define __host__
#define __device__
%s
// k_strat_alloc / sweep_strat_alloc on one thread: the tiles in order, 256 "threads" per tile; returns the uniform verdict
extern "C" int alloc(const double *d, long long *off, long long ncube, long long nsamp, int ask_uniform) {
    const int ntile = strat_alloc_ntile(ncube);
    double part[256], tbase[1024], base = 0.0;
    long long lo, hi;
    off[0] = 0;
    if (!ask_uniform)
        for (int g = 0; g < ntile; ++g) {
            for (int t = 0; t < 256; ++t) {
                strat_alloc_stretch(ncube, ntile, g, t, lo, hi);
                part[t] = strat_alloc_stretch_sum(d, lo, hi);
            }
            tbase[g] = base;
            base += strat_alloc_base(part, 256);
        }
    const int uniform = strat_alloc_uniform(ask_uniform, base);
    for (int g = 0; g < ntile; ++g) {
        if (!uniform)
            for (int t = 0; t < 256; ++t) {
                strat_alloc_stretch(ncube, ntile, g, t, lo, hi);
                part[t] = strat_alloc_stretch_sum(d, lo, hi);
            }
        for (int t = 0; t < 256; ++t) {
            strat_alloc_stretch(ncube, ntile, g, t, lo, hi);
            strat_alloc_offsets(d, off, ncube, nsamp, lo, hi, uniform, uniform ? 0.0 : strat_alloc_base(part, t), uniform ? 0.0 : tbase[g], base);
        }
    }
    return uniform;
}
extern "C" int ntile(long long ncube) { return strat_alloc_ntile(ncube); }
"""


@pytest.fixture(scope="module")
def host_alloc(tmp_path_factory):
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_strat.h: the marker lines around the allocation rule are gone"
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi and "strat_alloc_offsets" in text[lo:hi]
    static = open(os.path.join(ROOT, "mcintegration.jl_amd", "csrc", "mci_static_kernels.h")).read()
    sweep = open(os.path.join(ROOT, "mcintegration.jl_amd", "csrc", "mci_sweep_strat.h")).read()
    for fn in ("strat_alloc_stretch(", "strat_alloc_stretch_sum(", "strat_alloc_base(", "strat_alloc_uniform(", "strat_alloc_offsets("):
        assert fn in static[static.index("void __launch_bounds__(256) k_strat_alloc"):] and fn in sweep, fn      # both callers go through the rule
    d = tmp_path_factory.mktemp("strat_alloc")
    src, so = os.path.join(d, "alloc_host.cpp"), os.path.join(d, "alloc_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % text[lo:hi])
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.alloc.restype = C.c_int
    lib.alloc.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_longlong, C.c_longlong, C.c_int]
    lib.ntile.restype, lib.ntile.argtypes = C.c_int, [C.c_longlong]

    def run(d, N, uniform=False):
        d = np.ascontiguousarray(d, dtype=np.float64)
        off = np.full(d.size + 1, -1, dtype=np.int64)
        u = lib.alloc(d.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_longlong)), d.size, int(N), 1 if uniform else 0)
        return off, bool(u)
    run.ntile = lib.ntile
    return run


def uniform_offsets(nc, N):
    h = np.arange(1, nc + 1, dtype=np.float64)
    M = float(N - 2 * nc)
    c = np.minimum(M * h / float(nc), M)
    c[-1] = M
    return np.concatenate([[0], 2 * np.arange(1, nc + 1) + np.floor(c).astype(np.int64)])


@pytest.mark.parametrize("nc", [1, 15, 256, 257, 2048, 70000])
def test_allocation_rule_is_the_documented_order_bit_for_bit(host_alloc, nc):
    assert host_alloc.ntile(nc) == min(-(-nc // 256), 1024)
    rng = np.random.default_rng(nc)
    for N in (2 * nc, 2 * nc + 1, 8 * nc + 3):
        d = rng.lognormal(0.0, 3.0, nc) ** 0.375
        zeros = d.copy()
        zeros[rng.random(nc) < 0.5] = 0.0
        for what, v in (("dense", d), ("zeros", zeros)):
            if not v.sum() > 0:
                continue
            off, uni = host_alloc(v, N)
            assert not uni
            np.testing.assert_array_equal(off, kernel_order_alloc(v, N), err_msg="%s ncube %d N %d" % (what, nc, N))
            assert off[0] == 0 and off[-1] == N and np.diff(off).min() >= 2
        # no information, a total that is not finite, or a start that asks for it: uniform
        bad_inf, bad_nan = d.copy(), d.copy()
        bad_inf[nc // 2], bad_nan[nc // 3] = np.inf, np.nan
        want = uniform_offsets(nc, N)
        for v, ask in ((np.zeros(nc), False), (bad_inf, False), (bad_nan, False), (d, True)):
            off, uni = host_alloc(v, N, ask)
            assert uni
            np.testing.assert_array_equal(off, want)
        n = np.diff(want)
        assert n.sum() == N and n.min() >= 2 and n.max() - n.min() <= 1


# the (layout, nstrat, N) of tests/test_hip_sweep_strat.py, at that module's first parameter value
GPU_CASES = [("x2y2", [16, 16], 4096), ("sphere2", [5, 1, 3], 30), ("sphere2", [5, 1, 3], 2048), ("sphere2", [5, 1, 3], 8193),
             ("sphere2", [16, 1, 128], 4096), ("sphere2", [5, 1, 3], 8192), ("sphere2", [5, 1, 3], 16384), ("peak2", [3, 2], 6000), ("complex", [37], 4096)]


@pytest.mark.parametrize("name,nstrat,N", GPU_CASES, ids=["%s-%d-%d" % (c[0], len(c[1]) and int(np.prod(c[1])), c[2]) for c in GPU_CASES])
def test_the_cap_of_the_gpu_comparison_holds_for_the_reference_alone(oracle, name, nstrat, N):
    """d_h of the oracle's own first iteration (uniform allocation, untrained map): the kernel's order of the prefix sum against the
    oracle's long double one differs by at most 1 on at most max(2, ncube // 1000) hypercubes -- what check_alloc allows on the GPU"""
    from test_hip_sweep_strat import LAYOUTS as GPU_LAYOUTS
    L = GPU_LAYOUTS[name]
    cx = L.get("complex", False)
    ocfg = oracle.Config([dict(kind=0, pool=0, lower=0.0, upper=1.0)], L["dof"], obs_nbin=[2] * len(L["dof"]) if cx else None)
    if cx:
        ocfg.set_ncomp(2)
    of = oracle.compile_c_integrand(L["f"])
    nc = int(np.prod(nstrat))
    r = ocfg.strat_iteration(of, [1.0], SEED, 0, 0, nstrat, oracle.Config.strat_alloc(np.ones(nc), N, True))
    ref = np.diff(oracle.Config.strat_alloc(r["d"], N))
    emu = np.diff(kernel_order_alloc(r["d"], N)) if r["d"].sum() > 0 else np.diff(uniform_offsets(nc, N))
    ndiff = int(np.count_nonzero(ref != emu))
    print("cap: %s ncube %d N %d: %d hypercubes differ" % (name, nc, N, ndiff))
    assert emu.sum() == N and emu.min() >= 2
    assert np.abs(ref - emu).max() <= 1 and ndiff <= max(2, nc // 1000)


# ---- mci.integrate_sweep(stratify=..., alloc=...) -------------------------------------------------------------------------------------

def kw2():
    return dict(var=mci.Continuous(0.0, 1.0), dof=[[2]], device=-1)


ROWS = [[1.0], [0.5], [0.25]]


def test_stratify_under_a_chain_solver_raises():
    for solver in ("vegasmc", "mcmc"):
        with pytest.raises(ValueError, match="stratify: refused for solver"):
            mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, solver=solver, stratify=True, **kw2())
    with pytest.raises(ValueError, match="stratify = 3"):
        mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, stratify=3, **kw2())
    with pytest.raises(ValueError, match="measurefreq"):
        mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, stratify=True, measurefreq=2, **kw2())
    with pytest.raises(ValueError, match="alloc="):
        mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, stratify=mci.Stratify(carry=True), **kw2())


def test_alloc_of_the_wrong_length_shape_or_plan_raises():
    from mcintegration_jl_amd.integrate import StratD
    f = mci.Integrand(X2Y2P, [1.0])
    st = mci.Stratify(nstrat=[4, 3])
    with pytest.raises(ValueError, match="alloc= belongs to a stratified sweep"):
        mci.integrate_sweep(f, ROWS, alloc=[np.ones(12)] * 3, **kw2())
    with pytest.raises(ValueError, match=r"one strat_d array per point \(3\), got 2"):
        mci.integrate_sweep(f, ROWS, stratify=st, alloc=[np.ones(12)] * 2, **kw2())
    with pytest.raises(ValueError, match=r"alloc\[1\] has shape \(11,\), the plan nstrat = \[4, 3\] has 12 hypercubes"):
        mci.integrate_sweep(f, ROWS, stratify=st, alloc=[np.ones(12), np.ones(11), np.ones(12)], **kw2())
    other = StratD(np.ones(12), [3, 4], 0.75)
    with pytest.raises(ValueError, match=r"alloc\[0\] was measured on nstrat = \[3, 4\] under beta = 0.75, this call runs nstrat = \[4, 3\] under beta = 0.75"):
        mci.integrate_sweep(f, ROWS, stratify=st, alloc=[other] * 3, **kw2())
    beta = StratD(np.ones(12), [4, 3], 0.5)
    with pytest.raises(ValueError, match=r"under beta = 0.5, this call runs nstrat = \[4, 3\] under beta = 0.75"):
        mci.integrate_sweep(f, ROWS, stratify=st, alloc=[beta] * 3, **kw2())
    assert other[2:5].nstrat == [3, 4] and np.asarray(other).sum() == 12.0
    same = StratD(np.ones(12), [4, 3], 0.75)
    with pytest.raises(mci.MCIError) as e:            # checked, bound, eligible: only the device is missing
        mci.integrate_sweep(f, ROWS, stratify=st, alloc=[same] * 3, **kw2())
    assert e.value.code == 7


def test_the_fallback_warns_once_and_passes_stratify_on(monkeypatch):
    """two Continuous leaves: refused by the stratified sweep, so the points run as integrate(..., stratify=...) calls"""
    import sys
    I = sys.modules[mci.integrate.__module__]
    seen = []

    def fake(f, **kw):
        seen.append(kw)
        return I.Result(np.zeros((1, 1)), np.ones((1, 1)), kw["config"], 0, neval=1, seconds=0.0, block=16)
    monkeypatch.setattr(I, "integrate", fake)
    st = mci.Stratify(nstrat=[4, 3])
    def kw():
        return dict(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], device=-1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rs = mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, stratify=st, **kw())
    mine = [x for x in w if issubclass(x.category, RuntimeWarning) and "does not run as a sweep" in str(x.message)]
    assert len(mine) == 1 and "2 variable leaves" in str(mine[0].message) and "follow-up" in str(mine[0].message)
    assert len(rs) == 3 == len(seen) and all(k["stratify"] is st for k in seen) and not any(r.sweep_batched for r in rs)
    with pytest.raises(ValueError, match="alloc= needs the batched form"):
        mci.integrate_sweep(mci.Integrand(X2Y2P, [1.0]), ROWS, stratify=st, alloc=[np.ones(12)] * 3, **kw())
