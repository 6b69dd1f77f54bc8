"""CPU tests of the harness of the stratified static kernels (tests/strat_cases.py): the float64 mirror of k_strat_alloc, k_strat_reduce and
k_strat_remap against the long-double reference within the derived bounds over the whole table, six planted mistakes that the bounds
reject, the table's coverage, strat_magic (csrc/mci_host_strat.h, the section between its marker lines compiled for the HOST) against
integer division, and the refusals of the three test hooks (csrc/mci_debug.h mci_debug_strat_alloc, mci_debug_strat_reduce,
mci_debug_strat_remap through Engine.strat_alloc_rows, strat_reduce_rows, strat_remap_rows), which need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcintegration_jl_amd as mci
import strat_cases as S
from mcintegration_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")


def alloc_groups():
    groups = {}
    for c in S.ALLOC_CASES:
        groups.setdefault(c["family"], []).append(c)
    return groups


def run_alloc(c, mutate=None):
    """-> (problems of the mirror against the reference, ratio)"""
    d, ask = S.alloc_input(c)
    ref = S.alloc_reference(d, c["nsamp"], ask)
    off, tsum = S.kernel_order_alloc(d, c["nsamp"], ask, full=True, mutate=mutate)
    bad, ratio = S.alloc_check(off, ref, c["nsamp"])
    if S.alloc_is_exact(c, d) and not np.array_equal(off[1:], 2 * np.arange(1, d.size + 1) + ref["fl"]):
        bad.append("an exact family differs from floor(C_ref)")
    if bool(tsum[-1]) != ref["uniform"] or (c["family"] in S.UNIFORM_FAMILIES) != ref["uniform"]:
        bad.append("uniform verdict %r, reference %r" % (tsum[-1], ref["uniform"]))
    return bad, ratio, ref


# ---- the table --------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_what_it_claims():
    a = S.ALLOC_CASES
    assert len({c["id"] for c in a + S.REDUCE_CASES + S.REMAP_CASES}) == len(a) + len(S.REDUCE_CASES) + len(S.REMAP_CASES)
    for nc in S.ALLOC_NCUBE:
        assert {c["nsamp"] for c in a if c["ncube"] == nc and c["family"] == "lognormal"} == set(S.alloc_nsamp(nc))
        assert {c["family"] for c in a if c["ncube"] == nc} - {"huge"} == set(S.ALLOC_FAMILIES)
    assert {(c["ncube"], c["nsamp"]) for c in a if c["family"] == "huge"} == {(15, 8192), (257, 8192)}
    for fam in S.ALLOC_FAMILIES[1:]:       # N takes turns: every family meets M = 0, M = 1, 8 ncube + 3 and 2^40 + 7
        kinds = {S.alloc_nsamp(c["ncube"]).index(c["nsamp"]) for c in a if c["family"] == fam}
        assert kinds == {0, 1, 2, 3}, fam
    assert {(c["nchunk"], c["nw"], c["values"]) for c in S.REDUCE_CASES} == {(n, w, v) for n in S.REDUCE_NCHUNK for w in S.REDUCE_NW for v in S.REDUCE_VALUES}
    assert {(c["n_old"], c["n_new"], c["e"]) for c in S.REMAP_CASES} == {(tuple(o), tuple(n), e) for o, n in S.REMAP_PLANS for e in S.REMAP_E}
    from test_strat_carry_host import PAIRS_3D
    assert [tuple(map(tuple, p)) for p in S.REMAP_PLANS[:4]] == [tuple(map(tuple, p)) for p in PAIRS_3D]
    assert int(np.prod(S.REMAP_PLANS[5][1])) > 4096 * 256 and len(S.REMAP_PLANS[6][0]) == 32
    # the tile geometry the sizes are chosen for (csrc/mci_strat.h strat_alloc_ntile, strat_alloc_stretch)
    ntile = lambda nc: min(-(-nc // 256), 1024)
    assert (ntile(256), ntile(257), ntile(262144), ntile(262145)) == (1, 2, 1024, 1024)
    tl = -(-262145 // 1024)
    assert tl == 257 and -(-tl // 256) == 2 and 262145 - 1020 * tl == 5 and 1024 - 1021 == 3     # per = 2, a 5-element tile, three empty ones


@pytest.mark.parametrize("c", [c for c in S.REDUCE_CASES if c["nw"] == 2], ids=lambda c: c["id"])
def test_the_reduce_offsets_exercise_the_ownership_rule(c):
    x = S.reduce_input(c)
    off, rec_h = x["off"], x["rec_h"]
    assert off.size - 1 <= 2000 and np.diff(off).min() >= 2
    f = S.reduce_features(x)
    if c["nchunk"] == 1:
        assert rec_h.max() == -1
    elif c["nchunk"] == 2:
        assert f["cut_first"] and f["cut_last"]
    else:
        assert all(f.values()), f
    used = rec_h >= 0
    assert np.all(np.isnan(x["rec_s"][~used])) and np.all(np.isfinite(x["rec_s"][used]))     # (a record that is not there is never to be read)
    if c["values"] == "exact":
        nc = off.size - 1
        assert nc & (nc - 1) == 0
        for h in np.unique(rec_h[used]):
            n = int(off[h + 1] - off[h])
            assert n & (n - 1) == 0
    if c["values"] == "cancel" and c["nchunk"] > 2:     # the clamp at 0 is reached from both sides
        ref = S.reduce_reference(x)
        lows = [float(lo) for v, lo, hi in ref["cut"].values()]
        assert any(v == 0 for v, lo, hi in ref["cut"].values()) and any(v > 0 for v, lo, hi in ref["cut"].values()) and min(lows) < 0


# ---- the mirror within the reference's bounds -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", sorted(alloc_groups()))
def test_alloc_mirror_within_the_window(family):
    worst, ambiguous, total = 0.0, 0, 0
    for c in alloc_groups()[family]:
        bad, ratio, ref = run_alloc(c)
        assert not bad, (c["id"], bad)
        worst = max(worst, ratio)
        ambiguous += int(np.count_nonzero(ref["lo"] != ref["hi"]))
        total += c["ncube"]
    print("alloc %-12s %3d cases: %d of %d hypercubes have a window of two integers, largest distance / bound %.3g" % (family, len(alloc_groups()[family]), ambiguous, total, worst))
    assert worst <= 1.0


def test_alloc_mirror_tsum_layout():
    c = next(c for c in S.ALLOC_CASES if c["family"] == "lognormal" and c["ncube"] == 262145)
    d, ask = S.alloc_input(c)
    off, tsum = S.kernel_order_alloc(d, c["nsamp"], ask, full=True)
    assert tsum.size == 2 * 1024 + 2 and np.all(tsum[1021:1024] == 0.0) and tsum[1020] == ((d[262140] + d[262141]) + d[262142] + d[262143]) + d[262144]
    assert tsum[1024] == 0.0 and tsum[1025] == tsum[0] and tsum[2048] == tsum[2047] + tsum[1023] and tsum[2049] == 0.0
    assert abs(tsum[2048] - float(d.astype(S.LD).sum())) <= 262145 * 2.0 ** -52 * tsum[2048]


def test_the_four_uniform_families_give_the_uniform_offsets():
    for nc in S.ALLOC_NCUBE:
        for N in S.alloc_nsamp(nc):
            want = S.kernel_order_alloc(np.ones(nc), N, True)
            n = np.diff(want)
            assert n.sum() == N and n.min() >= 2 and n.max() - n.min() <= 1
            if (N - 2 * nc) * nc < 2 ** 53:
                assert np.array_equal(want[1:], 2 * np.arange(1, nc + 1) + S.alloc_reference(np.ones(nc), N, True)["fl"])
            for fam in S.UNIFORM_FAMILIES:
                d, ask = S.alloc_input(dict(ncube=nc, family=fam, seed=nc))
                off, tsum = S.kernel_order_alloc(d, N, ask, full=True)
                assert tsum[-1] == 1.0 and np.array_equal(off, want), (fam, nc, N)


def test_huge_weights_allocate_in_proportion():
    """d_h = 1e305 with one 3e305: P is finite, M P is not.  The product form alone gives inf, clamped to M: the first hypercube would
    take every movable sample (n = [8164, 2, 2, ...]); the quotient form gives 480 each and 1440 for the heavier one."""
    c = next(c for c in S.ALLOC_CASES if c["family"] == "huge" and c["ncube"] == 15)
    d, ask = S.alloc_input(c)
    n = np.diff(S.kernel_order_alloc(d, c["nsamp"]))
    assert n.sum() == 8192 and abs(int(n[7]) - 1442) <= 1 and np.all(np.abs(np.delete(n, 7) - 482) <= 1), n
    with np.errstate(over="ignore"):
        assert not np.isfinite(float(c["nsamp"] - 30) * d.sum())
    # an input whose products are finite keeps its bits: the quotient form is not what the rule computes there
    dd = np.random.default_rng(5).lognormal(0.0, 3.0, 4000) ** 0.375
    M, P, tot = 8.0 * 4000 + 3, np.cumsum(dd), dd.sum()
    assert np.count_nonzero(M * P / tot != M * (P / tot)) > 0


@pytest.mark.parametrize("values", S.REDUCE_VALUES)
def test_reduce_mirror_within_the_bounds(values):
    worst = 0.0
    for c in S.REDUCE_CASES:
        if c["values"] != values:
            continue
        x = S.reduce_input(c)
        bad, ratio = S.reduce_check(S.kernel_order_reduce(x), x, S.reduce_reference(x), values == "exact")
        assert not bad, (c["id"], bad)
        worst = max(worst, ratio)
    print("reduce %-7s largest |mirror - reference| / bound %.3g" % (values, worst))
    assert worst <= 1.0 and (values != "exact" or worst == 0.0)


def test_remap_mirror_within_the_bounds():
    worst, ulps = 0.0, 0.0
    for c in S.REMAP_CASES:
        d = S.remap_input(c)
        ref, bound = S.remap_reference(d, c["n_old"], c["n_new"], c["e"])
        got = S.kernel_order_remap(d, c["n_old"], c["n_new"], c["e"])
        bad, ratio, u = S.remap_check(got, ref, bound)
        assert not bad, (c["id"], bad)
        if c["e"] == 1.0:
            assert np.array_equal(got.view(np.uint64), ref.astype(np.float64).view(np.uint64)), c["id"]
        assert {0.0, 3 * 5e-324, 1.0, np.inf} <= set(d.tolist())
        worst, ulps = max(worst, ratio), max(ulps, u)
    print("remap: largest |mirror - reference| / bound %.3g, %.3g ulps" % (worst, ulps))
    assert worst <= 1.0


# ---- the bounds have teeth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutate", S.MUTATIONS)
def test_a_planted_mistake_is_rejected(mutate):
    caught = []
    if mutate in ("no_last_clamp", "tile_base_late"):
        for c in S.ALLOC_CASES:
            if c["ncube"] <= 65537 and c["family"] in ("lognormal", "zeros", "integers", "spike_last", "huge"):
                d, ask = S.alloc_input(c)
                bad, _ = S.alloc_check(S.kernel_order_alloc(d, c["nsamp"], ask, mutate=mutate), S.alloc_reference(d, c["nsamp"], ask), c["nsamp"])
                if bad:
                    caught.append(c["id"])
    elif mutate == "stride_from_new":
        for c in S.REMAP_CASES:
            d = S.remap_input(c)
            ref, bound = S.remap_reference(d, c["n_old"], c["n_new"], c["e"])
            if S.remap_check(S.kernel_order_remap(d, c["n_old"], c["n_new"], c["e"], mutate=mutate), ref, bound)[0]:
                caught.append(c["id"])
    else:
        for c in S.REDUCE_CASES:
            if c["nw"] == 2:
                x = S.reduce_input(c)
                if S.reduce_check(S.kernel_order_reduce(x, mutate=mutate), x, S.reduce_reference(x), c["values"] == "exact")[0]:
                    caught.append(c["id"])
    print("%s: rejected by %d cases, e.g. %s" % (mutate, len(caught), caught[:3]))
    assert caught, mutate


def test_another_order_of_the_total_alone_stays_inside_the_window():
    """what "no_last_clamp" is planted on (strat_cases: in the kernel's own order the last P_h is the total bit for bit, and dropping
    C_last := M changes nothing): the pairwise total by itself is no mistake"""
    for c in S.ALLOC_CASES:
        if c["ncube"] <= 65537 and c["family"] in ("lognormal", "zeros", "integers", "spike_last", "huge"):
            d, ask = S.alloc_input(c)
            own, other = S.kernel_order_alloc(d, c["nsamp"], ask, full=True), S.kernel_order_alloc(d, c["nsamp"], ask, full=True, mutate="total_pairwise")
            assert not S.alloc_check(other[0], S.alloc_reference(d, c["nsamp"], ask), c["nsamp"])[0], c["id"]
            nt = (own[1].size - 2) // 2
            last = max(g for g in range(nt) if g == 0 or own[1][g] != 0.0 or g * -(-d.size // nt) < d.size)
            assert own[1][2 * nt] == own[1][nt + last] + own[1][last]          # total = the last tile's base + its sum, exactly


# ---- strat_magic, compiled for the host -----------------------------------------------------------------------------------------------------

BEGIN, END = "// >>> strat magic", "// <<< strat magic"
WRAP = r"""
#include <cstdint>
%s
// h[i] / n by the reciprocal, as the sample kernel and k_strat_remap decode: -> entries that differ from the division
extern "C" long long check(uint32_t n, const uint32_t *h, long long count, uint32_t *magic_out, int *shift_out) {
    uint32_t magic;
    int shift;
    strat_magic(n, &magic, &shift);
    *magic_out = magic;
    *shift_out = shift;
    long long bad = 0;
    for (long long i = 0; i < count; ++i) bad += (uint32_t)(((uint64_t)h[i] * magic) >> shift) != h[i] / n;
    return bad;
}
"""


@pytest.fixture(scope="module")
def host_magic(tmp_path_factory):
    text = open(os.path.join(CSRC, "mci_host_strat.h")).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_host_strat.h: the marker lines around strat_magic are gone"
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi and "void strat_magic(uint32_t n, uint32_t *magic, int *shift)" in text[lo:hi]
    d = tmp_path_factory.mktemp("strat_magic")
    src, so = os.path.join(d, "magic_host.cpp"), os.path.join(d, "magic_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % text[lo:hi])
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    lib.check.restype, lib.check.argtypes = C.c_longlong, [C.c_uint32, u32p, C.c_longlong, u32p, C.POINTER(C.c_int)]

    def run(n, h):
        h = np.ascontiguousarray(h, dtype=np.uint32)
        magic, shift = C.c_uint32(), C.c_int()
        return lib.check(int(n), h.ctypes.data_as(u32p), h.size, C.byref(magic), C.byref(shift)), magic.value, shift.value
    return run


def magic_divisors():
    ns = set(range(1, 4097))
    for k in range(1, 32):
        ns.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
    ns.update((65521, 1000003, 16777213, 2147483629, 2147483647))       # primes
    return sorted(n for n in ns if 1 <= n <= 2 ** 31 - 1)


def test_strat_magic_divides_exactly(host_magic):
    top = 2 ** 31 - 1
    rng = np.random.default_rng(S.SEED)
    for n in magic_divisors():
        kmax = top // n
        ks = np.unique(np.concatenate([np.arange(0, min(kmax, 64) + 1), rng.integers(0, kmax + 1, 64), [kmax, kmax // 2, max(kmax - 1, 0)]]))
        h = np.concatenate([ks * n - 1, ks * n, ks * n + 1, [top, top - 1, 0]])
        h = h[(h >= 0) & (h <= top)]
        bad, magic, shift = host_magic(n, h)
        assert bad == 0 and 31 <= shift <= 62 and magic > 0, (n, bad, magic, shift)
    assert host_magic(1, [0, 1, top])[1:] == (0x80000000, 31)
    assert host_magic(3, np.arange(0, 3000))[0] == 0


# ---- the hooks ------------------------------------------------------------------------------------------------------------------------------

def offline():
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]]), mci.catalog.x2y2(), device=-1)


def test_the_hooks_are_declared_and_bound():
    hdr = open(os.path.join(CSRC, "mci_debug.h")).read()
    declared = set(re.findall(r"\bint (mci_debug_[a-z_0-9]+)\(", hdr))
    bound = {name for name, _, _ in _lib.DEBUG_SIGNATURES}
    assert declared == bound, declared ^ bound
    sigs = {name: args for name, _, args in _lib.DEBUG_SIGNATURES}
    i64p = C.POINTER(C.c_int64)
    assert sigs["mci_debug_strat_alloc"] == [C.c_void_p, _lib.c_double_p, C.c_int64, C.c_int64, C.c_int32, i64p, _lib.c_double_p]
    assert sigs["mci_debug_strat_reduce"] == [C.c_void_p, C.POINTER(_lib.DebugStratReduceIO)]
    assert sigs["mci_debug_strat_remap"] == [C.c_void_p, C.c_int32, _lib.c_int32_p, _lib.c_int32_p, C.c_double, _lib.c_double_p, _lib.c_double_p]
    m = re.search(r"typedef struct mci_debug_strat_reduce_io \{(.*?)\} mci_debug_strat_reduce_io;", hdr, re.S)
    fields = re.findall(r"\b(\w+)(?:,\s*(\w+))?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert [n for pair in fields for n in pair if n] == [n for n, _ in _lib.DebugStratReduceIO._fields_]
    L = mci.lib()
    for name in ("mci_debug_strat_alloc", "mci_debug_strat_reduce", "mci_debug_strat_remap"):
        assert hasattr(L, name) and name in hdr
    host = open(os.path.join(CSRC, "mci_host_strat.h")).read()
    for helper, n in (("strat_alloc_launches(", 3), ("strat_reduce_launch(", 3), ("strat_remap_launch(", 3)):      # defined once, called by product and hook
        assert host.count(helper) == n, helper
    assert host.count("hipLaunchKernelGGL(mci::k_strat_") == 3


def test_the_hooks_refuse_bad_arguments_without_a_device():
    eng = offline()
    for d, N, match in ((np.zeros(0), 10, "0 hypercubes"), (np.ones(4), 7, "7 samples for 4 hypercubes"), (np.ones(4), 2 ** 53, "samples for 4 hypercubes")):
        with pytest.raises(mci.MCIError, match=match):
            eng.strat_alloc_rows(d, N)
    with pytest.raises(ValueError):
        eng.strat_alloc_rows(np.ones((2, 2)), 8)
    with pytest.raises(mci.MCIError, match="offline"):
        eng.strat_alloc_rows(np.ones(4), 8)
    x = S.reduce_input(next(c for c in S.REDUCE_CASES if c["nchunk"] == 2 and c["nw"] == 2))
    good = dict(off=x["off"], part=x["part"], rec_h=x["rec_h"], rec_s=x["rec_s"], dnext=x["dnext"], beta=0.75)
    nc = x["off"].size - 1
    rh_hi, rh_lo = x["rec_h"].copy(), x["rec_h"].copy()
    rh_hi[1, 0], rh_lo[0, 1] = nc, -2
    for bad, match in ((dict(part=np.ones((2, 18)), rec_s=np.ones((2, 2, 18))), "9 weight columns"), (dict(part=np.ones((2, 0)), rec_s=np.ones((2, 2, 0))), "0 weight columns"),
                       (dict(part=np.ones((0, 4)), rec_h=np.ones((0, 2)), rec_s=np.ones((0, 2, 4))), "0 chunks"), (dict(beta=-1.0), "beta"), (dict(beta=np.inf), "beta"),
                       (dict(rec_h=rh_hi), r"rec_h\[2\] = %d" % nc), (dict(rec_h=rh_lo), r"rec_h\[1\] = -2"),
                       (dict(off=np.zeros(1), dnext=np.zeros(0)), "0 hypercubes")):
        with pytest.raises(mci.MCIError, match=match):
            eng.strat_reduce_rows(**dict(good, **bad))
    for bad in (dict(part=np.ones((2, 3))), dict(rec_h=np.ones((3, 2))), dict(rec_s=np.ones((2, 2, 6))), dict(dnext=np.ones(nc + 1))):
        with pytest.raises(ValueError):
            eng.strat_reduce_rows(**dict(good, **bad))
    for kw in (dict(), dict(log_row=False)):
        with pytest.raises(mci.MCIError, match="offline"):
            eng.strat_reduce_rows(**dict(good, **kw))
    for n_old, n_new, e, d, match in (([], [], 1.0, np.ones(1), "0 draws"), ([2] * 33, [2] * 33, 1.0, np.ones(1), "33 draws"), ([2, 0], [2, 2], 1.0, np.ones(1), "draw 1 is cut into 0 -> 2"),
                                      ([2, 2], [2, -1], 1.0, np.ones(4), "draw 1 is cut into 2 -> -1"), ([2, 2], [65536, 32768], 1.0, np.ones(4), "more than 2\\^31 - 1"),
                                      ([2, 2], [3, 3], np.nan, np.ones(4), "exponent"), ([2, 2], [3, 3], np.inf, np.ones(4), "exponent")):
        with pytest.raises(mci.MCIError, match=match):
            eng.strat_remap_rows(n_old, n_new, e, d)
    for n_old, n_new, d in (([2, 2], [3], np.ones(4)), ([2, 2], [3, 3], np.ones(5))):
        with pytest.raises(ValueError):
            eng.strat_remap_rows(n_old, n_new, 1.0, d)
    with pytest.raises(mci.MCIError, match="offline"):
        eng.strat_remap_rows([2, 2], [3, 3], 0.5, np.ones(4))
