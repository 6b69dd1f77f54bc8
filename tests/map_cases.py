"""The case table, the replay and the derived bounds of the :vegas map draw on its own (csrc/mci_device.h draw_leaf, draw_sample,
draw_sample_pipe, the gather and edge-cache phases, pack_bin / tdraw_extract and the tiled replay), shared by tests/test_map_host.py (the CPU
oracle against the replay, planted mistakes, the table's own conditions) and tests/test_hip_map.py (the kernels through Engine.set_grid /
set_distribution -> sample_dump and iteration("vegas")).  Data and plain numpy only: no GPU code.  Everything is a pure function of its
arguments; the uniforms come in from outside (the oracle's generator, which tests/golden pins, or numbers a test makes up).

The replay.  In float64 with exactly the reference's operations and order (sampler.jl:293-305, :13-22, common.jl:16-25):
    Continuous   yn = y N, rounded once;  iy = floor(yn);  dy = yn - iy;  x = g[iy] + dy (g[iy+1] - g[iy]), the product and the sum each rounded
    Discrete     locate: jl = 1, ju = K + 2;  while ju - jl > 1: jm = (jl + ju) / 2;  y < acc[jm]  ?  ju = jm  :  jl = jm;   x = lower + jl - 1
so x and the bin of every draw come out as they must, bit for bit.  In long double (64-bit mantissa) on top of those:
    1 / prob     N dx with dx = g[iy+1] - g[iy] AS ROUNDED ABOVE (the reference and every kernel form that same float64 difference; it is
                 data to the product), 1 / distribution[bin] for a Discrete draw
    jac          the product of 1 / prob over all draws;  jac_i over integrand i's own draws (= weights * padding_probability * jac of
                 vegas/montecarlo.jl:152)
    packed row   per block b:  S_i = sum_s w_i(x_s) jac_i,s,  norm_b = 1e-10 + n,  m_i = S_i / norm_b;   sum_b m_i | sum_b m_i^2 |
                 1e-10 + sum_b norm_b | blocks * n | ... | per leaf and bin  (blocks + 1) 1e-10 + sum over the integrands i that own the
                 draw and the samples that drew the bin of (|w_i| jac)^2        (mcio_vegas_block, run_blocks, pack; merge_cases.mirror
                 has the same columns)

The bounds are derived, not measured; nothing in them comes from a kernel.  u = 2^-53, eps = 2 u.
    jac          per draw at most JAC_OPS = 3 rounded operations: the reference rounds N dx, 1 / (N dx) and jac / prob (sampler.jl:303,
                 vegas/montecarlo.jl:126); the kernels round raw N (or one factor of a group's N^8) and jac raw.  Products only, so the
                 relative errors add:  |jac - ref| <= JAC_OPS ndraw u ref          (16 draws: 5.3e-15, against the suite's standing 1e-13)
    a term       w_i jac_i: the Jacobian, the integrand's own W_OPS operations on positive numbers (stated per integrand below), the
                 products w pad jac:  t = (JAC_OPS ndraw + W_OPS + 2) u
    a block sum  n positive terms in any association: n eps sum, plus t;  the normalisation 1e-10 + 1 + 1 + ..: n u;  the division: u
    sums         over blocks: blocks eps more; the squares: twice the mean's bound, the square u, blocks eps
    NORM, NEVAL  NORM within (n + blocks) u of the long-double value (the reference adds 1.0 n times to 1e-10), NEVAL exactly
    a bin        c samples in it: each (|w| jac)^2 within 2 t + 2 u, their sum and the blocks + 1 offsets of 1e-10 within
                 (c + blocks + 1) eps.  A bin NO sample landed in carries bound 0 against what such a bin holds in the oracle's row,
                 1e-10 added blocks + 1 times in float64: nothing else may have touched it.
Where these come out looser than the suite's standing figures (jac 1e-13, sums 1e-11, histogram 1e-9) the tests assert the tighter.

`replay(..., mutate=)` plants one of five deliberate mistakes (tests/test_map_host.py: the bounds have teeth)."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
EPS = LD(2.0) ** -52
SEED = 20261021
JAC_OPS = 3
STANDING = dict(jac=1e-13, sums=1e-11, hist=1e-9)
SIZES = (1, 2, 3, 63, 64, 65, 999, 1024, 1025, 2500)
L16 = 50.0 ** 0.5

GRID_FAMILIES = ("uniform", "geometric", "spike_first", "spike_middle", "spike_last", "ulp_run", "offset", "straddle", "small_range",
                 "small_range_lossy")
RANGES = {"offset": (2.0 ** 40, 2.0 ** 40 + 1.0), "straddle": (-3.0, 5.0), "small_range": (0.0, 2.0 ** -125), "small_range_lossy": (0.0, 2.0 ** -119)}
ULP_RUN = 32
TABLE_FAMILIES = ("uniform", "dominant", "tiny", "zeros_first", "zeros_middle", "zeros_last")
DISCRETE_K = (1, 2, 17, 1025)


def grid(family, n, lower=0.0, upper=1.0):
    """n increments on [lower, upper], strictly increasing, the end points bit for bit"""
    lo, hi = LD(lower), LD(upper)
    i = np.arange(n + 1).astype(LD)
    if family in ("uniform", "offset", "straddle", "small_range", "small_range_lossy", "ulp_run") or n == 1:
        g = (lo + (hi - lo) * i / n).astype(np.float64)
        if family == "straddle":
            g[np.argmin(np.abs(g))] = 0.0                                  # an edge exactly at 0.0
        if family == "ulp_run":                                            # 32 neighbours, each one ulp of its left edge wide
            assert n >= 2 * ULP_RUN - 1
            s = n // 2 - ULP_RUN // 2
            for j in range(ULP_RUN):
                g[s + j + 1] = np.nextafter(g[s + j], np.inf)
    elif family == "geometric":                                            # widths falling by a constant ratio, 2^40 from first to last
        w = LD(2.0) ** (-LD(40.0) * np.arange(n).astype(LD) / (n - 1))
        g = (lo + (hi - lo) * np.concatenate([[LD(0.0)], np.cumsum(w)]) / w.sum()).astype(np.float64)
    elif family in ("spike_first", "spike_middle", "spike_last"):          # one increment holds 1 - 2^-30 of the range
        at = {"spike_first": 0, "spike_middle": n // 2, "spike_last": n - 1}[family]
        w = np.full(n, LD(2.0) ** -30 / (n - 1))
        w[at] = 1 - LD(2.0) ** -30
        g = (lo + (hi - lo) * np.concatenate([[LD(0.0)], np.cumsum(w)])).astype(np.float64)
    else:
        raise KeyError(family)
    g[0], g[-1] = lower, upper
    assert g.shape == (n + 1,) and np.all(np.diff(g) > 0), (family, n)      # what mci_set_grid checks
    g.setflags(write=False)
    return g


def ulp_run_edges(n):
    s = n // 2 - ULP_RUN // 2
    return s, s + ULP_RUN


def table(family, k):
    """the unnormalised distribution handed to set_distribution; exact 0.0 entries make ties in the accumulation"""
    d = np.ones(k)
    if k == 1 or family == "uniform":
        pass
    elif family == "dominant":
        d[:] = 2.0 ** -40 / (k - 1)
        d[k // 3] = 1.0 - 2.0 ** -40
    elif family == "tiny":
        d[k // 2] = 2.0 ** -60 * k
    elif family == "zeros_first":
        d[:max(1, k // 3)] = 0.0
    elif family == "zeros_middle":
        if k == 2:
            d[0] = 0.0
        else:
            d[k // 3:k // 3 + max(1, k // 4)] = 0.0
    elif family == "zeros_last":
        d[k - max(1, k // 3):] = 0.0
    else:
        raise KeyError(family)
    d.setflags(write=False)
    return d


def normalised(d):
    """(distribution, accumulation) as Discrete(...; distribution = d) forms them (variable.jl:306-315): left to right in float64"""
    d = np.asarray(d, dtype=np.float64)
    s = 0.0
    for v in d:
        s += float(v)
    dist = d / s
    acc = np.zeros(d.size + 1)
    run = 0.0
    for i, v in enumerate(dist):
        run += float(v)
        acc[i + 1] = run
    return dist, acc


# ------------------------------------------------------------------------------------------------------------------------------------
# integrands: (source text, the same in long double, W_OPS = rounded operations on positive numbers per weight)
# ------------------------------------------------------------------------------------------------------------------------------------
def _sumsq(d):
    return ("double r = 0.0;\nfor (int d = 0; d < %d; ++d) r += x[d] * x[d];\nw[0] = r;" % d,
            lambda x: (x[:, :d] * x[:, :d]).sum(axis=1)[:, None], d + 1)


INTEGRANDS = {
    "one": ("w[0] = 1.0;", lambda x: np.ones((x.shape[0], 1), dtype=LD), 0),
    "x2y2": ("w[0] = x[0] * x[0] + x[1] * x[1];", lambda x: (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])[:, None], 3),
    "sumsq3": _sumsq(3), "sumsq8": _sumsq(8), "sumsq16": _sumsq(16),
    "pow1000": ("w[0] = 0x1p+1000;", lambda x: np.full((x.shape[0], 1), LD(2.0) ** 1000), 0),      # exact: the integral over [0, 2^-125]^8 is 1
    "pow952": ("w[0] = 0x1p+952;", lambda x: np.full((x.shape[0], 1), LD(2.0) ** 952), 0),         # ... over [0, 2^-119]^8
    "mixed2": ("w[0] = x[0] * x[0] + x[1] * x[1] + x[2];\nw[1] = x[0] * x[0] + x[2];",
               lambda x: np.stack([x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2], x[:, 0] * x[:, 0] + x[:, 2]], axis=1), 5),
}

# ------------------------------------------------------------------------------------------------------------------------------------
# layouts: leaves ("c", lower, upper, increments) | ("d", lower, upper), one pool per leaf, dof per integrand and pool
# ------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    "sizes": dict(leaves=[("c", 0.0, 1.0, n) for n in SIZES], dof=[[1] * len(SIZES)], f="one"),
    "sizes_scaled": dict(leaves=[("c", 0.0, 2.0 ** -20, n) for n in SIZES], dof=[[1] * len(SIZES)], f="one"),
    "ranges": dict(leaves=[("c",) + RANGES["offset"] + (999,), ("c",) + RANGES["offset"] + (2500,), ("c",) + RANGES["straddle"] + (1024,),
                           ("c",) + RANGES["straddle"] + (999,)] + [("d", 1, k) for k in DISCRETE_K], dof=[[1] * 8], f="one"),
    # The two small ranges.  Continuous(0, 2^-125) itself cannot be made: the reference asserts upper > lower + 2 eps(1.0) (variable.jl:140)
    # and so do the front end and mci_problem_create.  The leaf is declared on [0, 1] and handed the uniform grid of [0, 2^-125]: the
    # map, its increments and every product of the draw are those of the range that cannot be declared.
    "small": dict(leaves=[("c", 0.0, 1.0, 999)], dof=[[8]], f="pow1000", own=["small_range"]),
    "lossy": dict(leaves=[("c", 0.0, 1.0, 999)], dof=[[8]], f="pow952", own=["small_range_lossy"]),
    "pair2": dict(leaves=[("c", 0.0, 1.0, 999)], dof=[[2]], f="x2y2"),
    "pair8": dict(leaves=[("c",) + RANGES["straddle"] + (1024,)], dof=[[8]], f="sumsq8"),
    "pair16": dict(leaves=[("c", -L16, L16, 999)], dof=[[16]], f="sumsq16"),
    "tiles": dict(leaves=[("c", 0.0, 1.0, 999), ("c", 0.0, 1.0, 1025), ("c", 0.0, 1.0, 2500)], dof=[[1, 1, 1]], f="sumsq3"),
    "tiles11": dict(leaves=[("c", 0.0, 1.0, 999), ("c", 0.0, 1.0, 1025), ("c", 0.0, 1.0, 1025)], dof=[[1, 1, 1]], f="sumsq3"),
    "mixed": dict(leaves=[("c", 0.0, 1.0, 65), ("c",) + RANGES["straddle"] + (64,), ("d", 1, 17)], dof=[[1, 1, 1], [1, 0, 1]], f="mixed2"),
}


def nbin(leaf):
    return leaf[3] if leaf[0] == "c" else leaf[2] - leaf[1] + 1


def draws(layout):
    """flat draw order (pool, slot; one leaf per pool): [(leaf, slot)]"""
    lay = LAYOUTS[layout]
    maxdof = np.max(np.asarray(lay["dof"]), axis=0)
    return [(l, s) for l in range(len(lay["leaves"])) for s in range(int(maxdof[l]))]


def owns(layout):
    """[integrand][draw]: the draw is one of the integrand's own"""
    lay = LAYOUTS[layout]
    return np.array([[s < row[l] for l, s in draws(layout)] for row in lay["dof"]])


def tables(layout, grids="uniform", dists="uniform"):
    """per leaf: the grid, or the unnormalised distribution.  `grids` / `dists`: one family for every leaf or one per leaf; a leaf whose
    range belongs to a family (offset, straddle, the small ranges) keeps that family unless another is named for it"""
    lay = LAYOUTS[layout]
    out = []
    for l, lf in enumerate(lay["leaves"]):
        if lf[0] == "c":
            fam = grids if isinstance(grids, str) else grids[l]
            own = [lay["own"][l]] if lay.get("own") else [k for k, r in RANGES.items() if r == (lf[1], lf[2])]
            if fam == "uniform" and own:
                fam = own[0]
            if fam == "ulp_run" and lf[3] < 2 * ULP_RUN - 1:
                fam = "uniform"
            out.append(grid(fam, lf[3], *(RANGES[fam] if fam in RANGES else (lf[1], lf[2]))))
        else:
            out.append(table(dists if isinstance(dists, str) else dists[l], nbin(lf)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the replay
# ------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("x_one_rounding", "bin_from_exact_product", "scale_after_eight", "bisection_le", "bin_ten_bits")


def _locate(acc, y, le=False):
    """common.jl:16-25, every y at once; 1-based jl with acc[jl] <= y < acc[jl + 1] in the reference's 1-based terms"""
    jl = np.ones(y.shape, dtype=np.int64)
    ju = np.full(y.shape, acc.size + 1, dtype=np.int64)
    while np.any(ju - jl > 1):
        go = ju - jl > 1
        jm = (jl + ju) // 2
        below = (y <= acc[jm - 1]) if le else (y < acc[jm - 1])
        ju = np.where(go & below, jm, ju)
        jl = np.where(go & ~below, jm, jl)
    return jl


def _fma(a, b, c):
    """a + b c rounded once, exactly (rationals)"""
    return np.array([float(Fraction(float(p)) + Fraction(float(q)) * Fraction(float(r))) for p, q, r in zip(a, b, c)])


def replay(layout, tabs, y, mutate=None):
    """y[n][ndraw] uniforms in [0, 1)  ->  dict(x float64 [n][ndraw], bin int [n][ndraw], inv long double [n][ndraw] = 1 / prob per draw,
    jac, jaci [n][ni] long double, located: every Discrete y lies below accumulation[end] (where not, the reference raises)).
    With `mutate`, jac / jaci come from the float64 arithmetic of the mistake."""
    assert mutate in (None,) + MUTATIONS
    lay = LAYOUTS[layout]
    dr = draws(layout)
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    assert y.shape == (n, len(dr)) and np.all((y >= 0) & (y < 1))
    x, bins, inv = np.zeros((n, len(dr))), np.zeros((n, len(dr)), dtype=np.int64), np.zeros((n, len(dr)), dtype=LD)
    raw, scale = np.zeros((n, len(dr))), np.ones(len(dr))
    located = True
    for k, (l, slot) in enumerate(dr):
        lf, yk = lay["leaves"][l], y[:, k]
        if lf[0] == "c":
            N, g = lf[3], tabs[l]
            yn = yk * float(N)                                                           # rounded once
            iy = np.floor(yn).astype(np.int64)
            if mutate == "bin_from_exact_product":
                iy = np.array([int(Fraction(float(v)) * N // 1) for v in yk], dtype=np.int64)
            dy = yn - iy
            dx = g[iy + 1] - g[iy]
            x[:, k] = _fma(g[iy], dy, dx) if mutate == "x_one_rounding" else g[iy] + dy * dx        # two roundings
            bins[:, k], raw[:, k], scale[k] = iy, dx, float(N)
            inv[:, k] = LD(N) * dx.astype(LD)
        else:
            dist, acc = normalised(tabs[l])
            located = located and bool(np.all(yk < acc[-1]))
            jl = np.minimum(_locate(acc, yk, le=mutate == "bisection_le"), dist.size)
            x[:, k] = lf[1] + (jl - 1)
            bins[:, k] = jl - 1
            with np.errstate(divide="ignore"):
                raw[:, k] = 1.0 / dist[jl - 1]
                inv[:, k] = LD(1.0) / dist[jl - 1].astype(LD)
    own = owns(layout)
    if mutate == "scale_after_eight":                                                    # float64: eight bare increments, then their N factors
        def prod(mask):
            j = np.ones(n)
            with np.errstate(under="ignore"):
                for lo in range(0, len(dr), 8):
                    sc = 1.0
                    for k in range(lo, min(lo + 8, len(dr))):
                        if mask[k]:
                            j = j * raw[:, k]
                            sc *= scale[k]
                    j = j * sc
            return j.astype(LD)
        jac, jaci = prod(np.ones(len(dr), dtype=bool)), np.stack([prod(m) for m in own], axis=1)
    else:
        jac = np.prod(inv, axis=1)
        jaci = np.stack([np.prod(np.where(m[None, :], inv, LD(1.0)), axis=1) for m in own], axis=1)
    if mutate == "bin_ten_bits":
        bins = bins & 1023
    return dict(x=x, bin=bins, inv=inv, jac=jac, jaci=jaci, located=located)


def jac_bound(layout):
    return JAC_OPS * len(draws(layout)) * U


def offset_of_an_empty_bin(nblocks):
    """what a bin no sample lands in holds after clearStatistics! of the sum and of every block and the blocks' addition (float64)"""
    v = 1.0e-10
    for _ in range(nblocks):
        v += 1.0e-10
    return v


def packed_row(layout, reps, dtype=LD):
    """the packed row of one :vegas iteration from its blocks' replays (`reps`: one replay() per block), measurefreq 1, in long double:
    dict(sums [ni], squares [ni], norm, neval, hist per leaf, count per leaf = samples per bin, and a relative bound for each)"""
    lay = LAYOUTS[layout]
    body, f, wops = INTEGRANDS[lay["f"]]
    dr, own = draws(layout), owns(layout)
    ni, nb = len(lay["dof"]), len(reps)
    t = (JAC_OPS * len(dr) + wops + 2) * U
    sums, squares, norm = np.zeros(ni, dtype=dtype), np.zeros(ni, dtype=dtype), dtype(1.0e-10)
    hist = [np.full(nbin(lf), dtype(offset_of_an_empty_bin(nb))) for lf in lay["leaves"]]
    count = [np.zeros(nbin(lf), dtype=np.int64) for lf in lay["leaves"]]
    npb = reps[0]["x"].shape[0]
    for r in reps:
        n = r["x"].shape[0]
        assert n == npb
        w = f(r["x"].astype(LD))
        nrm = dtype(1.0e-10) + dtype(n)
        m = ((w * r["jaci"]).astype(dtype).sum(axis=0) / nrm).astype(dtype)
        sums, squares, norm = sums + m, squares + m * m, norm + nrm
        for i in range(ni):
            wj2 = ((np.abs(w[:, i]) * r["jac"]) ** 2).astype(dtype)
            for k, (l, slot) in enumerate(dr):
                if own[i][k]:
                    np.add.at(hist[l], r["bin"][:, k], wj2)
                    if i == int(np.argmax(own[:, k])):
                        np.add.at(count[l], r["bin"][:, k], 1)
    b_sum = t + (npb * EPS + npb * U + U) + nb * EPS
    b_sq = 2 * (t + npb * EPS + npb * U + U) + U + nb * EPS
    b_hist = [np.where(c > 0, 2 * t + 2 * U + (c + nb + 1) * EPS, LD(0.0)) for c in count]
    return dict(sums=sums, squares=squares, norm=norm, neval=nb * npb, hist=hist, count=count, b_sum=b_sum, b_sq=b_sq, b_norm=(npb + nb) * U,
                b_hist=b_hist, nblocks=nb)


def split(packed, layout):
    """(sums, squares, norm, neval, [hist per leaf]) of a packed row: obsSum | obsSqSum | normalization | neval | visited | histograms"""
    lay = LAYOUTS[layout]
    ni = len(lay["dof"])
    p = np.asarray(packed, dtype=np.float64)
    off, hs = 2 * ni + 2 + ni + 1, []
    for lf in lay["leaves"]:
        hs.append(p[off:off + nbin(lf)])
        off += nbin(lf)
    return p[:ni], p[ni:2 * ni], p[2 * ni], p[2 * ni + 1], hs


def check_samples(x, jac, rep, layout, who):
    """x bit for bit; returns the largest |jac - ref| / bound"""
    x, jac = np.asarray(x, dtype=np.float64), np.asarray(jac, dtype=np.float64)
    bad = np.argwhere(x.view(np.uint64) != rep["x"].view(np.uint64))
    assert bad.size == 0, "%s: %d x differ from the replay, first at (sample, draw) %s: %r against %r" % (
        who, len(bad), tuple(bad[0]), x[tuple(bad[0])], rep["x"][tuple(bad[0])])
    assert np.all(np.isfinite(jac)), "%s: a Jacobian is not finite" % who
    return float((np.abs(jac.astype(LD) - rep["jac"]) / (jac_bound(layout) * rep["jac"])).max())


def check_packed(packed, ref, layout, who):
    """the largest ratio of a difference to its derived bound over (sums and squares and NORM, histogram); NEVAL and the bins no sample
    landed in exactly"""
    s, q, norm, neval, hs = split(packed, layout)
    assert neval == ref["neval"], (who, neval, ref["neval"])
    assert np.all(np.isfinite(np.asarray(packed, dtype=np.float64))), who

    def rel(got, want, bound):
        return float(np.max(np.abs(np.asarray(got).astype(LD) - want) / (bound * np.abs(want))))
    r_stat = max(rel(s, ref["sums"], ref["b_sum"]), rel(q, ref["squares"], ref["b_sq"]), rel(norm, ref["norm"], ref["b_norm"]))
    r_hist, empty = 0.0, offset_of_an_empty_bin(ref["nblocks"])
    for l, (h, want, bound, c) in enumerate(zip(hs, ref["hist"], ref["b_hist"], ref["count"])):
        untouched = c == 0
        wrong = np.flatnonzero(untouched & (h != empty))
        assert wrong.size == 0, "%s: leaf %d bin %s holds %r although no sample landed there (such a bin holds %r)" % (who, l, wrong[:8], h[wrong[:8]], empty)
        if np.any(~untouched):
            r_hist = max(r_hist, rel(h[~untouched], want[~untouched], bound[~untouched]))
    return r_stat, r_hist


def tightest(layout, npb, nblocks, count_max):
    """(jac, sums, hist): the smaller of the derived bound and the suite's standing figure, for the printout"""
    lay = LAYOUTS[layout]
    t = float((JAC_OPS * len(draws(layout)) + INTEGRANDS[lay["f"]][2] + 2) * U)
    return (min(float(jac_bound(layout)), STANDING["jac"]), min(2 * (t + float(npb * EPS + npb * U + U)) + float(U + nblocks * EPS), STANDING["sums"]),
            min(2 * t + float(2 * U + (count_max + nblocks + 1) * EPS), STANDING["hist"]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
def sample_cases():
    """per-sample cases: (id, layout, grids, dists): every grid family and every Discrete table"""
    out = [("sizes-%s" % fam, "sizes", fam, "uniform") for fam in ("uniform", "geometric", "spike_first", "spike_middle", "spike_last", "ulp_run")]
    out += [("ranges-%s" % fam, "ranges", "uniform", fam) for fam in TABLE_FAMILIES]            # (offset and straddle: the leaves' own families)
    # (the straddling leaves once more, on a geometric and a spike grid; next to 2^40 only the uniform grid is strictly increasing)
    out += [("ranges-straddle", "ranges", ("uniform", "uniform", "geometric", "spike_middle") + (None,) * 4, "zeros_middle"), ("small-small_range", "small", "uniform", "uniform"),
            ("lossy-small_range_lossy", "lossy", "uniform", "uniform")]
    return out


def family_of(case_id):
    return case_id.split("-", 1)[1]


# sample indices of the 32-bit stream (seed SEED, iteration 0) at which draw 7 of layout "sizes" (1024 increments) has y N an exact
# integer, dy == 0: the first three, found by a search on the CPU (one draw in 2^22); tests/test_map_host.py checks them
DY0_DRAW = 7
DY0_INDICES = (1422359, 3958668, 17701320)


def uniforms(oracle, layout, npb, block_lo, nblocks, iteration=0, bits=52, seed=SEED, _cache={}):
    """y[block][sample][draw] of the :vegas stream (stream = 8 iteration, index = block * npb + sample), from the oracle's generator"""
    key = (len(draws(layout)), npb, block_lo, nblocks, iteration, bits, seed)
    if key not in _cache:
        nd = key[0]
        y = np.array([[[oracle.uniform(seed, iteration * 8, (block_lo + b) * npb + s, k, bits=bits) for k in range(nd)] for s in range(npb)]
                      for b in range(nblocks)])
        y.setflags(write=False)
        _cache[key] = y
    return _cache[key]


# per-launch cases: name -> (layout, grids, dists, samples per block); two blocks each; 2003 samples where a ragged chunk matters
LAUNCHES = {
    "pair2": ("pair2", "geometric", "uniform", 512),
    "pair8": ("pair8", "uniform", "uniform", 512),
    "pair8-spike": ("pair8", "spike_middle", "uniform", 512),
    "pair16": ("pair16", "geometric", "uniform", 512),
    "pair16-ulp_run": ("pair16", "ulp_run", "uniform", 512),
    "tiles": ("tiles", ("geometric", "spike_last", "ulp_run"), "uniform", 2003),
    "tiles11": ("tiles11", ("spike_first", "geometric", "ulp_run"), "uniform", 2003),
    "mixed-zeros_first": ("mixed", ("spike_first", "uniform", None), (None, None, "zeros_first"), 512),
    "mixed-zeros_middle": ("mixed", ("geometric", "uniform", None), (None, None, "zeros_middle"), 2003),
    "mixed-zeros_last": ("mixed", ("ulp_run", "geometric", None), (None, None, "zeros_last"), 512),
    "small": ("small", "uniform", "uniform", 512),
    "lossy": ("lossy", "uniform", "uniform", 512),
}
NBLOCKS = 2


def launch_reference(oracle, name, bits=52, iteration=0, block_lo=0, _cache={}):
    """(tables, the blocks' replays, the long-double packed row with its bounds) of a per-launch case"""
    key = (name, bits, iteration, block_lo)
    if key not in _cache:
        layout, grids, dists, npb = LAUNCHES[name]
        tabs = tables(layout, grids, dists)
        y = uniforms(oracle, layout, npb, block_lo, NBLOCKS, iteration=iteration, bits=bits)
        reps = [replay(layout, tabs, y[b]) for b in range(NBLOCKS)]
        _cache[key] = tabs, reps, packed_row(layout, reps)
    return _cache[key]


def flat(row, layout):
    """a packed row (float64) out of packed_row()'s columns, visited left at zero"""
    ni = len(LAYOUTS[layout]["dof"])
    return np.concatenate([np.asarray(row["sums"], dtype=np.float64), np.asarray(row["squares"], dtype=np.float64), [float(row["norm"]), float(row["neval"])],
                           np.zeros(ni + 1)] + [np.asarray(h, dtype=np.float64) for h in row["hist"]])
