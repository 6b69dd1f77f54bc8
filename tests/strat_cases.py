"""The case table, the independent reference and the float64 mirror of the three static kernels of stratified :vegas (csrc/
mci_static_kernels.h k_strat_alloc, k_strat_reduce, k_strat_remap; the allocation rule strat_alloc_* of csrc/mci_strat.h, which the
stratified sweep's one workgroup walks too), shared by tests/test_strat_kernels_host.py (the mirror against the reference, on the CPU) and
tests/test_hip_strat_kernels.py (the kernels through Engine.strat_alloc_rows, strat_reduce_rows and strat_remap_rows).  Data and plain
numpy only: no GPU code, and reference and mirror share no helper.

The reference.  In long double, from the formulas in the comments of mci_strat.h and mci_static_kernels.h.
  allocation   M = N - 2 ncube, P_h = sum_{j <= h} d_j, P = P_{ncube - 1}: C_h = M P_h / P, off[h + 1] = 2 (h + 1) + floor(C_h), C_last = M;
               uniform (d_h = 1: C_h = M (h + 1) / ncube, in integers) if asked for or if P is 0 or not finite
  reduce       a cut hypercube h of n = off[h + 1] - off[h] samples: S = the sum of its pieces (the records that name h),
               v2_q = max(0, (S2_q - S1_q^2 / n) / (n - 1));  with V = 1 / ncube
               mean_q = sum_c part[c][q] + sum_h V / n S1_q,  var_q = sum_c part[c][nw + q] + sum_h V^2 v2_q / n,  d_h = (sum_q v2_q)^(beta / 2)
  remap        d'[h'] = d[h]^e, h the old hypercube that holds the centre of h': per draw, new cell j of n' -> old cell (2 j + 1) n // (2 n')

The bounds are derived, not measured; nothing in them comes from a kernel, no entry is excused and there is no cap.  eps = 2^-52; a
float64 sum of n terms lies, in ANY association, within n eps sum|x_i| of the exact sum (tests/merge_cases.py).
  allocation   P_h and P are sums of at most ncube non-negative terms (relative error ncube eps each), then one product and one quotient:
               C lies within b_h = (2 ncube + 4) eps C_ref of C_ref, so the kernel's floor must lie in
               [floor(max(C_ref - b_h, 0)), floor(min(C_ref + b_h, M))]; besides off[0] = 0, off[ncube] = N and every n_h >= 2.
               (The long double prefix sum itself is within ncube 2^-63 C_ref, 2^-11 of b_h.)  Where the window holds one integer the kernel
               is pinned; at N = 2^40 + 7 nearly every hypercube is ambiguous and the mirror carries the comparison.
               A uniform allocation is held to the integer rule exactly where M ncube < 2^53 (the product is then exact in float64 and a
               quotient that is no integer lies further than one rounding from the next one), else to the window with b_h = 4 eps C_ref.
  reduce       a cut hypercube of p pieces: dS = p eps sum|pieces|;  with A = |S2| + S1^2 / n
                   t = S1^2       dt = dS1 (2 |S1| + dS1) + eps (|S1| + dS1)^2
                   u = t / n      du = dt / n + eps (S1^2 + dt) / n
                   w = S2 - u     dw = dS2 + du + eps (A + dS2 + du)            <- the one-pass variance's bound, in |S2| + S1^2 / n
                   v = w / (n-1)  dv = dw / (n - 1) + eps (|w| + dw) / (n - 1);  the clamp at 0 is 1-Lipschitz: |v2 - v2_ref| <= dv,
               so an entry whose reference is clamped at 0 may be anything in [0, dv].
               V / n S1: three roundings (1 / ncube, / n, * S1): (V / n) (dS1 + 4 eps (|S1| + dS1));
               V V v2 / n: four roundings: (V^2 / n) (dv + 6 eps (v2 + dv));
               a column is the sum of nchunk partial rows and one term per cut hypercube (the idle threads' zeros cost nothing):
               sum of the terms' bounds + (nchunk + cuts) eps sum(|term| + its bound).
               d_h: x = sum_q v2_q lies within dx = sum dv + nw eps sum(v2 + dv); x -> x^a is monotone, so d_h lies between
               max(x - dx, 0)^a and (x + dx)^a, widened by pow's own error (below).
  pow          ROCm's documentation of the double pow's error is not among the files of the installation the suite is built against, so the
               project's rel 1e-12 (tests/test_hip_stratified_parity.py) stays: POW_REL; results below the normal range add one spacing of
               the subnormals, 2^-1074.  The GPU tests print the largest observed |kernel - reference| in ulps.
Exact families: the kernel must EQUAL the reference, so that a lost or doubled term cannot hide in rounding.
  allocation   "integers": d_h small integers whose total is a power of two, where M P < 2^53 (every P_h, the product and the quotient are
               then exact); "spike_*": a single 1.0 among zeros, first, in the middle, last.
  reduce       "exact": ncube and the n of every cut hypercube are powers of two, every S1, S2 and part entry is a small integer multiple
               of a power of two with S2 - S1^2 / n = k (n - 1), k a small integer, and beta = 2 (d_h = sum_q v2_q = sum_q k_q).

The mirror.  A float64 restatement of each kernel's order of operations (the library is built with -ffp-contract=off, so everything but
pow is expected to match it bit for bit):
  allocation   kernel_order_alloc: tiles of ceil(ncube / ntile) hypercubes, ntile = min(ceil(ncube / 256), 1024), 256 stretches each;
               P_h = tile base + (stretch base + running sum), every base the sequential sum of what lies before it; C = M * P_h / total,
               recomputed as M * (P_h / total) where the first form is not finite; min(C, M); the last one M; tsum = tile sums | tile
               bases | total | uniform flag
  reduce       thread t of 1024 takes the chunks [t per, min((t + 1) per, nchunk)), per = ceil(nchunk / 1024); per chunk first the partial
               row, then the records rr = 0, 1 under the ownership rule (a leading record that continues the record before it -- rec_h[2c - 1],
               or rec_h[2c - 2] where that is -1 -- was folded there; an owner folds the leading records of the following chunks while they
               name its hypercube); d_h = the sum itself where beta / 2 == 1, else pow; then the tree s = 512 .. 1 per column
  remap        the mixed-radix decode (draw 0 fastest), the gather, then v if e == 1 else pow(v, e)
These orders are a contract: a change to one changes the mirror in the same commit, or fails the tests.  `mutate` plants one of six
deliberate mistakes into the mirror (tests/test_strat_kernels_host.py: the bounds have teeth).  One of them needs a word: in the kernel's
own order the last P_h is the total bit for bit (the last tile's base plus its sum IS the total's last addition) and fl(fl(M t) / t) = M,
so there "C_last := M dropped" changes no bit and nothing can reject it.  The assignment protects every order in which the two differ;
"no_last_clamp" therefore drops it from a mirror whose total is added up pairwise -- an order that by itself ("total_pairwise") stays
inside every window -- and off[ncube] = N rejects that."""
import numpy as np

LD = np.longdouble
EPS = LD(2.0) ** -52
SEED = 20261021
POW_REL = 1e-12
TINY = 2.0 ** -1074
CHUNK = 256
REDUCE_THREADS = 1024
MUTATIONS = ("fold_twice", "fold_stops_at_stretch", "n_for_n_minus_1", "no_last_clamp", "tile_base_late", "stride_from_new")


# ---- allocation: the case table ---------------------------------------------------------------------------------------------------------

ALLOC_NCUBE = (1, 2, 255, 256, 257, 513, 65537, 262144, 262145, 1048876)
ALLOC_FAMILIES = ("lognormal", "zeros", "spike_first", "spike_mid", "spike_last", "integers", "subnormal", "all_zero", "one_inf", "one_nan", "ask_uniform")
UNIFORM_FAMILIES = ("all_zero", "one_inf", "one_nan", "ask_uniform")


def alloc_nsamp(nc):
    """M = 0 | M = 1 | a few samples to move per hypercube | offsets beyond 32 bits"""
    return (2 * nc, 2 * nc + 1, 8 * nc + 3, 2 ** 40 + 7)


def alloc_cases():
    cases = []

    def add(family, nc, N):
        cases.append(dict(kind="alloc", family=family, ncube=nc, nsamp=N, seed=SEED + len(cases), id="alloc-%s-%d-%d" % (family, nc, N)))
    for i, nc in enumerate(ALLOC_NCUBE):
        for N in alloc_nsamp(nc):                  # every size at every N
            add("lognormal", nc, N)
        for j, fam in enumerate(ALLOC_FAMILIES[1:]):   # every other family at every size, N taking turns
            add(fam, nc, alloc_nsamp(nc)[(i + j) % 4])
        add("integers", nc, 8 * nc + 3)            # (M P < 2^53 at every size: the exact comparison)
    for nc in (15, 257):                           # d_h finite, P finite, M P not
        add("huge", nc, 8192)
    seen, out = set(), []
    for c in cases:
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def alloc_input(c):
    """-> d [ncube] float64, asked-for uniform flag"""
    rng = np.random.default_rng(c["seed"])
    nc, fam = c["ncube"], c["family"]
    d = rng.lognormal(0.0, 3.0, nc) ** 0.375
    if fam == "zeros":
        d[rng.random(nc) < 0.5] = 0.0
        d[rng.integers(nc)] = 1.5                  # (never all of them)
    elif fam.startswith("spike_"):
        d = np.zeros(nc)
        d[{"spike_first": 0, "spike_mid": nc // 2, "spike_last": nc - 1}[fam]] = 1.0
    elif fam == "integers":
        d = rng.integers(0, 8, nc).astype(np.float64)
        d[0] += 1.0
        s = int(d.sum())
        d += np.bincount(rng.integers(0, nc, (1 << (s - 1).bit_length()) - s), minlength=nc)   # total: the next power of two
    elif fam == "subnormal":
        d = rng.integers(1, 4, nc) * 5e-324        # total positive and subnormal (at most 3 ncube spacings)
    elif fam == "all_zero":
        d = np.zeros(nc)
    elif fam == "one_inf":
        d[nc // 2] = np.inf
    elif fam == "one_nan":
        d[nc // 3] = np.nan
    elif fam == "huge":
        d = np.full(nc, 1e305)
        d[nc // 2] = 3e305
    return d, fam == "ask_uniform"


# ---- allocation: the reference ----------------------------------------------------------------------------------------------------------

def alloc_reference(d, N, ask_uniform):
    """-> dict of uniform, lo and hi [ncube] (the window of floor(C_h)), fl [ncube] = floor(C_ref), C [ncube] and b [ncube] in long
    double, M"""
    d = np.asarray(d, dtype=np.float64)
    nc = d.size
    M = N - 2 * nc
    with np.errstate(all="ignore"):
        P = np.cumsum(d.astype(LD))
        total = P[-1]
        uniform = bool(ask_uniform or not total > 0 or not np.isfinite(total))
        if uniform:
            fl = (np.int64(M) * np.arange(1, nc + 1, dtype=np.int64)) // np.int64(nc)      # M ncube < 2^63
            C = fl.astype(LD) + ((np.int64(M) * np.arange(1, nc + 1, dtype=np.int64)) % np.int64(nc)).astype(LD) / LD(nc)
            b = LD(0) * C if M * nc < 2 ** 53 else 4 * EPS * C
        else:
            C = LD(M) * P / total
            b = LD(2 * nc + 4) * EPS * C
    lo = np.floor(np.maximum(C - b, 0)).astype(np.int64)
    hi = np.floor(np.minimum(C + b, LD(M))).astype(np.int64)
    lo[-1] = hi[-1] = M
    C[-1], b[-1] = LD(M), LD(0)
    fl = np.floor(C).astype(np.int64)                   # (what the exact families are held to: there C itself is exact)
    return dict(uniform=uniform, lo=lo, hi=hi, C=C, b=b, M=M, fl=fl)


def alloc_is_exact(c, d):
    """the families in which C_ref is exact in float64 whatever the order: the offsets must be 2 (h + 1) + floor(C_ref)"""
    M = c["nsamp"] - 2 * c["ncube"]
    return c["family"].startswith("spike_") or (c["family"] == "integers" and M * float(np.sum(d)) < 2.0 ** 53) or \
        (c["family"] in UNIFORM_FAMILIES and M * c["ncube"] < 2 ** 53)


def alloc_check(off, ref, N):
    """the kernel's (or the mirror's) offsets against the reference -> (problems, largest distance of C_ref from the kernel's [floor,
    floor + 1) over b_h)"""
    off = np.asarray(off, dtype=np.int64)
    nc = off.size - 1
    bad = []
    if off[0] != 0 or off[nc] != N:
        bad.append("off[0] = %d, off[ncube] = %d (0, %d)" % (off[0], off[nc], N))
    if np.diff(off).min() < 2:
        bad.append("n_h = %d at hypercube %d" % (np.diff(off).min(), int(np.argmin(np.diff(off)))))
    fl = off[1:] - 2 * np.arange(1, nc + 1, dtype=np.int64)
    out = np.nonzero((fl < ref["lo"]) | (fl > ref["hi"]))[0]
    if out.size:
        h = int(out[0])
        bad.append("%d floors outside their window, first: hypercube %d has %d, window [%d, %d]" % (out.size, h, fl[h], ref["lo"][h], ref["hi"][h]))
    C, b = ref["C"], ref["b"]
    dist = np.maximum(np.maximum(fl.astype(LD) - C, C - (fl.astype(LD) + 1)), 0)
    with np.errstate(all="ignore"):
        ratio = np.where(dist > 0, dist / b, LD(0))
    return bad, float(np.max(ratio))


# ---- allocation: the mirror -------------------------------------------------------------------------------------------------------------

def kernel_order_alloc(d, N, ask_uniform=False, full=False, mutate=None):
    """k_strat_alloc's documented order of the prefix sum in double: tiles of ceil(ncube / min(ceil(ncube / 256),
    1024)) hypercubes, 256 stretches each; P_h = tile base + (stretch base + running sum), every base the sequential sum of what lies
    before it; then C_h = M P_h / P (M (P_h / P) where the product is not finite), floor, the last one M.  -> off [ncube + 1]; full: (off,
    tsum [2 ntile + 2] = tile sums | tile bases | total | uniform flag)"""
    d = np.asarray(d, dtype=np.float64)
    nc = d.size
    M = N - 2 * nc
    ntile = min(-(-nc // 256), 1024)
    tl = -(-nc // ntile)
    Ppre = np.zeros(nc)
    tsum = np.zeros(ntile)
    inner = []
    with np.errstate(all="ignore"):
        for g in range(ntile):
            t0, t1 = min(g * tl, nc), min(g * tl + tl, nc)
            if t1 <= t0:
                inner.append(None)
                continue
            per = -(-(t1 - t0) // 256)
            pad = np.zeros(256 * per)
            pad[:t1 - t0] = d[t0:t1]
            run = np.cumsum(pad.reshape(256, per), axis=1)          # sequential along a stretch
            sbase = np.concatenate([[0.0], np.cumsum(run[:, -1])])  # sequential over the stretches
            tsum[g] = sbase[256]
            inner.append((t0, t1, (sbase[:256, None] + run).reshape(-1)[:t1 - t0]))
        tbase = np.concatenate([[0.0], np.cumsum(tsum)])
        total = tbase[ntile]
        if mutate in ("no_last_clamp", "total_pairwise"):    # (planted: the total added up in another order, numpy's pairwise one)
            total = float(np.sum(d))
        uniform = bool(ask_uniform or not total > 0.0 or not total - total == 0.0)
        if uniform:
            C = float(M) * np.arange(1, nc + 1, dtype=np.float64) / float(nc)
        else:
            use = tbase if mutate != "tile_base_late" else np.concatenate([[0.0], tbase])      # (planted: the base of the tile before)
            for g, it in enumerate(inner):
                if it is not None:
                    Ppre[it[0]:it[1]] = use[g] + it[2]
            C = float(M) * Ppre / total
            again = ~(C - C == 0.0)
            C[again] = float(M) * (Ppre[again] / total)
        C = np.minimum(C, float(M))
        if mutate != "no_last_clamp":
            C[-1] = M
    fl = np.floor(C).astype(np.int64)
    off = np.concatenate([[0], 2 * np.arange(1, nc + 1) + fl])
    if not full:
        return off
    return off, np.concatenate([tsum, tbase[:ntile], [total, 1.0 if uniform else 0.0]])


# ---- reduce: the case table -------------------------------------------------------------------------------------------------------------

REDUCE_NCHUNK = (1, 2, 1023, 1024, 1025, 2049, 3000)
REDUCE_NW = (1, 2, 8)
REDUCE_VALUES = ("smooth", "cancel", "exact")
DNEXT_FILL = 12345.0      # dnext[h] = DNEXT_FILL + h before the launch


def reduce_cases():
    cases = []
    for nchunk in REDUCE_NCHUNK:
        for nw in REDUCE_NW:
            for values in REDUCE_VALUES:
                cases.append(dict(kind="reduce", nchunk=nchunk, nw=nw, values=values, seed=SEED + 1000 + len(cases),
                                  beta={"smooth": 0.75, "cancel": 1.0, "exact": 2.0}[values], id="reduce-%s-c%d-w%d" % (values, nchunk, nw)))
    return cases


def _sizes(nchunk, exact, rng):
    """hypercube sizes (each >= 2, 2000 at most) over nchunk chunks of 256 samples; the features of the issue for nchunk > 2: 2-sample
    hypercubes next to one longer than 2 per + 1 chunks, one that ends exactly on a chunk boundary, a cut in the first chunk"""
    N = CHUNK * nchunk - (0 if exact else 37)
    per = -(-nchunk // REDUCE_THREADS)
    if nchunk == 1:
        head = []
    elif nchunk == 2:
        head = [2] * 64 + [256] if exact else [2] * 100 + [100, 75]
    else:
        big = 4096 if exact else CHUNK * (2 * per + 2) + 50
        # [0, 128) twos | [128, 384) cut by the first boundary | [384, 512) ends on a boundary | twos | the long one | twos
        head = ([2] * 64 + [256, 128] if exact else [2] * 100 + [100, 212]) + [2] * 32 + [big] + [2] * 16
    R = N - sum(head)
    fill = []
    if exact:
        unit = 512 if N // 512 + 130 <= 1024 else 1024
        while R >= unit and nchunk > 2:
            fill.append(unit)
            R -= unit
        b = 1
        while R:
            b <<= 1
            if R & b:
                fill.append(b)
                R -= b
        want = max(1 << (len(head) + len(fill) - 1).bit_length(), 32)
        while len(head) + len(fill) < want:            # a split keeps the sum and the powers of two
            ok = [i for i, v in enumerate(fill) if v >= 4]
            i = ok[rng.integers(len(ok))]
            fill[i] //= 2
            fill.insert(i, fill[i])
        fill = [fill[i] for i in rng.permutation(len(fill))]
    else:
        avg = max(R // max(1800 - len(head), 1), 3)
        while R > 0:
            v = int(rng.integers(2, 2 * avg))
            if R - v < 2:
                v = R
            fill.append(v)
            R -= v
    sizes = np.array(head + fill, dtype=np.int64)
    assert sizes.min() >= 2 and sizes.sum() == N and sizes.size <= 2000
    return sizes


def reduce_records(off, nchunk):
    """rec_h [nchunk, 2] by the rule of vegas_strat (mci_strat.h): chunk c holds the samples [256 c, min(256 (c + 1), N)); its leading
    record names its first hypercube where the chunk cuts it, its trailing record its last one where that starts inside and is cut"""
    N, nc = int(off[-1]), off.size - 1
    rec = np.full((nchunk, 2), -1, dtype=np.int64)
    for c in range(nchunk):
        c0, c1 = CHUNK * c, min(CHUNK * c + CHUNK, N)
        first = int(np.searchsorted(off[:nc], c0, side="right")) - 1
        last = int(np.searchsorted(off[:nc], c1 - 1, side="right")) - 1
        if off[first] < c0 or off[first + 1] > c1:
            rec[c, 0] = first
        if last > first and off[last + 1] > c1:
            rec[c, 1] = last
    return rec


def reduce_input(c):
    """-> dict of off [ncube + 1], part [nchunk, 2 nw], rec_h [nchunk, 2], rec_s [nchunk, 2, 2 nw] (NaN where there is no record: never
    to be read), dnext [ncube], beta"""
    rng = np.random.default_rng(c["seed"])
    nchunk, nw, values = c["nchunk"], c["nw"], c["values"]
    exact = values == "exact"
    while True:                                         # (the fill is random: until the last chunk boundary cuts a hypercube too)
        sizes = _sizes(nchunk, exact, rng)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        nc = sizes.size
        rec_h = reduce_records(off, nchunk)
        if nchunk <= 2 or all(reduce_features(dict(off=off, rec_h=rec_h)).values()):
            break
    rec_s = np.full((nchunk, 2, 2 * nw), np.nan)
    if exact:
        assert nc & (nc - 1) == 0
        part = np.concatenate([rng.integers(-1024, 1025, (nchunk, nw)), rng.integers(0, 1025, (nchunk, nw))], axis=1) * 2.0 ** -30
    else:
        part = np.concatenate([rng.normal(0.0, 1.0, (nchunk, nw)), rng.random((nchunk, nw)) ** 2], axis=1) / nchunk
    where = {}
    for cc in range(nchunk):
        for rr in range(2):
            if rec_h[cc, rr] >= 0:
                where.setdefault(int(rec_h[cc, rr]), []).append((cc, rr))
    for h, pieces in where.items():
        n, p = int(sizes[h]), len(pieces)
        if exact:
            assert n & (n - 1) == 0
            s1 = rng.integers(-8, 9, (p, nw)) / 8.0
            tot = s1.sum(axis=0)
            k = rng.integers(0, 6, nw)
            units = np.round((tot * tot / n + k * (n - 1.0)) * 2.0 ** 18).astype(np.int64)       # S2 in units of 2^-18: exact
            cuts = np.sort(rng.integers(0, units + 1, (p - 1, nw)), axis=0) if p > 1 else np.zeros((0, nw), dtype=np.int64)
            edges = np.concatenate([np.zeros((1, nw), dtype=np.int64), cuts, units[None, :]], axis=0)
            s2 = np.diff(edges, axis=0) * 2.0 ** -18
        else:
            m = np.array([min(CHUNK * (cc + 1), off[h + 1]) - max(CHUNK * cc, off[h]) for cc, rr in pieces], dtype=np.float64)[:, None]
            mu, a = rng.normal(0.0, 1.0, nw), rng.lognormal(0.0, 2.0, nw)
            sig = 1e-7 if values == "cancel" else 1.0
            s1 = a * m * (mu + sig * rng.normal(0.0, 1.0, (p, nw)) / np.sqrt(m))
            s2 = a * a * m * (mu * mu + sig * sig * (0.5 + rng.random((p, nw))))
            if values == "cancel" and h % 3 == 0:       # no spread at all: S2 = S1^2 / n up to rounding, on either side of the clamp
                s1 = a * m * mu
                s2 = a * a * m * mu * mu
        for (cc, rr), x1, x2 in zip(pieces, s1, s2):
            rec_s[cc, rr, :nw], rec_s[cc, rr, nw:] = x1, x2
    return dict(off=off, part=part, rec_h=rec_h, rec_s=rec_s, dnext=DNEXT_FILL + np.arange(nc, dtype=np.float64), beta=c["beta"], nw=nw)


def reduce_features(x):
    """what the offsets of a case exercise -> dict of booleans (tests/test_strat_kernels_host.py asserts them for nchunk >= 1023)"""
    off, rec_h = x["off"], x["rec_h"]
    nchunk = rec_h.shape[0]
    per = -(-nchunk // REDUCE_THREADS)
    n = np.diff(off)
    long_ = np.nonzero(n > CHUNK * (2 * per + 1))[0]
    bounds = CHUNK * np.arange(1, nchunk)
    return dict(cut_first=rec_h[0].max() >= 0, cut_last=rec_h[nchunk - 1, 0] >= 0,
                ends_on_boundary=bool(np.isin(off[1:-1], bounds).any()),
                chunk_inside=bool(((rec_h[1:-1, 0] >= 0) & (rec_h[1:-1, 0] == rec_h[:-2].max(axis=1)) & (rec_h[1:-1, 0] == rec_h[2:, 0])).any()) if nchunk > 2 else False,
                long_next_to_twos=bool(any(h > 0 and h + 1 < n.size and n[h - 1] == 2 and n[h + 1] == 2 for h in long_)),
                crosses_stretch=bool(long_.size > 0))


# ---- reduce: the reference --------------------------------------------------------------------------------------------------------------

def pow_bounds(x, dx, a):
    """x^a for x within dx of the long double x >= 0, a > 0 -> (value, lowest, highest) with pow's own error on both"""
    x, dx, a = LD(x), LD(dx), LD(a)
    with np.errstate(all="ignore"):
        v = np.power(x, a)
        lo = np.power(np.maximum(x - dx, LD(0)), a)
        hi = np.power(x + dx, a)
    return v, lo - LD(POW_REL) * lo - LD(TINY), hi + LD(POW_REL) * hi + LD(TINY)


def reduce_reference(x):
    """-> dict of out, dout [2 nw] (value, bound), cut (hypercube -> (d_h, lowest, highest)), ncut"""
    off, part, rec_h, rec_s, nw, beta = x["off"], x["part"], x["rec_h"], x["rec_s"], x["nw"], x["beta"]
    nchunk, nc = part.shape[0], off.size - 1
    V = LD(1) / LD(nc)
    pieces = {}
    for c in range(nchunk):
        for rr in range(2):
            if rec_h[c, rr] >= 0:
                pieces.setdefault(int(rec_h[c, rr]), []).append(rec_s[c, rr].astype(LD))
    terms = [part.astype(LD)]
    dterms = [np.zeros(part.shape, dtype=LD)]
    cut = {}
    for h, ps in pieces.items():
        ps = np.array(ps, dtype=LD)
        p = ps.shape[0]
        n = LD(int(off[h + 1] - off[h]))
        S = ps.sum(axis=0)
        dS = (0 if p == 1 else p) * EPS * np.abs(ps).sum(axis=0)
        S1, S2, dS1, dS2 = S[:nw], S[nw:], dS[:nw], dS[nw:]
        A = np.abs(S2) + S1 * S1 / n
        dt = dS1 * (2 * np.abs(S1) + dS1) + EPS * (np.abs(S1) + dS1) ** 2
        du = dt / n + EPS * (S1 * S1 + dt) / n
        dw = dS2 + du + EPS * (A + dS2 + du)
        w = S2 - S1 * S1 / n
        dv = dw / (n - 1) + EPS * (np.abs(w) + dw) / (n - 1)
        v2 = np.maximum(w / (n - 1), LD(0))
        m = V / n * S1
        dm = V / n * (dS1 + 4 * EPS * (np.abs(S1) + dS1))
        q = V * V * v2 / n
        dq = V * V / n * (dv + 6 * EPS * (v2 + dv))
        terms.append(np.concatenate([m, q])[None, :])
        dterms.append(np.concatenate([dm, dq])[None, :])
        xs = v2.sum()
        dxs = dv.sum() + (0 if nw == 1 else nw) * EPS * (v2 + dv).sum()
        cut[h] = pow_bounds(xs, dxs, LD(beta) / 2)
    T, dT = np.concatenate(terms, axis=0), np.concatenate(dterms, axis=0)
    nadd = T.shape[0]
    out = T.sum(axis=0)
    dout = dT.sum(axis=0) + (0 if nadd == 1 else nadd) * EPS * (np.abs(T) + dT).sum(axis=0)
    return dict(out=out, dout=dout, cut=cut, ncut=len(pieces))


def reduce_check(got, x, ref, exact):
    """out [2 nw] and dnext [ncube] of the kernel (or the mirror) against the reference -> (problems, largest |difference| / bound)"""
    bad, worst = [], 0.0
    out, dn = np.asarray(got["out"], dtype=np.float64), np.asarray(got["dnext"], dtype=np.float64)
    nc = dn.size
    if exact:
        if not np.array_equal(out, ref["out"].astype(np.float64)) or not np.array_equal(out.astype(LD), ref["out"]):
            bad.append("out %r is not the reference's %r" % (out, ref["out"]))
    else:
        diff = np.abs(out.astype(LD) - ref["out"])
        if not np.all(diff <= ref["dout"]):
            q = int(np.argmax(diff / ref["dout"]))
            bad.append("out[%d] = %r, reference %r +- %r" % (q, out[q], ref["out"][q], ref["dout"][q]))
        worst = max(worst, float(np.max(np.where(diff > 0, diff / np.where(ref["dout"] > 0, ref["dout"], LD(TINY)), LD(0)))))
    fill = DNEXT_FILL + np.arange(nc, dtype=np.float64)
    keep = np.ones(nc, dtype=bool)
    keep[list(ref["cut"])] = False
    if not np.array_equal(dn[keep].view(np.uint64), fill[keep].view(np.uint64)):
        bad.append("dnext of %d hypercubes that are not cut was touched" % int(np.count_nonzero(dn[keep].view(np.uint64) != fill[keep].view(np.uint64))))
    if np.any(dn.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)):
        bad.append("0xFF bytes came back in dnext")
    for h, (v, lo, hi) in ref["cut"].items():
        k = LD(dn[h])
        if exact:
            if not k == v:
                bad.append("d_h[%d] = %r, the reference has %r exactly" % (h, dn[h], v))
        else:
            if not lo <= k <= hi:
                bad.append("d_h[%d] = %r outside [%r, %r] (reference %r)" % (h, dn[h], lo, hi, v))
            if k != v and np.isfinite(k):
                worst = max(worst, float(abs(k - v) / max(hi - v, v - lo)))
    return bad, worst


# ---- reduce: the mirror -----------------------------------------------------------------------------------------------------------------

def kernel_order_reduce(x, mutate=None):
    """k_strat_reduce in float64, in its order -> dict of out [2 nw] and dnext [ncube]"""
    off, part, rec_h, rec_s, nw, beta = x["off"], x["part"], x["rec_h"], x["rec_s"], x["nw"], x["beta"]
    nchunk, nc = part.shape[0], off.size - 1
    T = REDUCE_THREADS
    dnext = np.array(x["dnext"], dtype=np.float64)
    acc = np.zeros((T, 2 * nw))
    V = 1.0 / float(nc)
    per = -(-nchunk // T)
    flat_h = rec_h.reshape(-1)
    for t in range(T):
        c0 = min(t * per, nchunk)
        c1 = min(c0 + per, nchunk)
        a = acc[t]
        for c in range(c0, c1):
            a += part[c]
            for rr in range(2):
                h = int(flat_h[2 * c + rr])
                if h < 0:
                    continue
                if rr == 0 and c > 0 and mutate != "fold_twice":
                    ph = flat_h[2 * c - 1] if flat_h[2 * c - 1] >= 0 else flat_h[2 * c - 2]
                    if ph == h:
                        continue
                S = rec_s[c, rr].copy()
                stop = c1 if mutate == "fold_stops_at_stretch" else nchunk
                d = c + 1
                while d < stop and flat_h[2 * d] == h:
                    S += rec_s[d, 0]
                    d += 1
                n = float(off[h + 1] - off[h])
                ssum = 0.0
                for q in range(nw):
                    v2 = (S[nw + q] - S[q] * S[q] / n) / (n if mutate == "n_for_n_minus_1" else n - 1.0)
                    v2 = v2 if v2 > 0.0 else 0.0
                    a[q] += V / n * S[q]
                    a[nw + q] += V * V * v2 / n
                    ssum += v2
                dnext[h] = ssum if 0.5 * beta == 1.0 else np.power(ssum, 0.5 * beta)
    s = T // 2
    while s > 0:
        acc[:s] += acc[s:2 * s]
        s //= 2
    return dict(out=acc[0].copy(), dnext=dnext)


# ---- remap ------------------------------------------------------------------------------------------------------------------------------

REMAP_PLANS = [((5, 1, 3), (7, 2, 4)), ((5, 1, 3), (2, 1, 2)), ((5, 1, 3), (3, 3, 3)), ((5, 1, 3), (5, 1, 3)),   # tests/test_strat_carry_host.py PAIRS_3D
               ((40, 40), (64, 50)),
               ((3, 2), (1031, 1019)),                  # 1 050 589 new hypercubes: the grid of 4096 x 256 strides a second time
               ((1, 2) * 16, (2, 1) * 16)]              # 32 draws of ones and twos
REMAP_E = (1.0, 2.0 / 3.0, 2.0, 1.0 / 3.0)


def remap_cases():
    cases = []
    for old, new in REMAP_PLANS:
        for e in REMAP_E:
            cases.append(dict(kind="remap", n_old=tuple(old), n_new=tuple(new), e=e, seed=SEED + 2000 + len(cases),
                              id="remap-%dto%d-d%d-e%.3g" % (int(np.prod(old)), int(np.prod(new)), len(old), e)))
    return cases


def remap_input(c):
    """d_old [prod n_old]: lognormal, with 0, a subnormal, 1 and inf among the first entries"""
    rng = np.random.default_rng(c["seed"])
    d = rng.lognormal(0.0, 3.0, int(np.prod(c["n_old"])))
    d[:4] = [0.0, 3 * 5e-324, 1.0, np.inf]
    return d


def remap_reference(d_old, n_old, n_new, e):
    """-> (value [prod n_new] long double, bound): the centre rule in integers on the unravelled cells, then the power"""
    cells = np.unravel_index(np.arange(int(np.prod(n_new)), dtype=np.int64), tuple(int(v) for v in n_new), order="F")
    src = tuple((2 * j + 1) * int(n) // (2 * int(m)) for j, n, m in zip(cells, n_old, n_new))
    v = np.asarray(d_old, dtype=np.float64)[np.ravel_multi_index(src, tuple(int(v) for v in n_old), order="F")].astype(LD)
    if e == 1.0:
        return v, np.zeros(v.shape, dtype=LD)
    with np.errstate(all="ignore"):
        r = np.power(v, LD(e))
        return r, np.where(np.isfinite(r), LD(POW_REL) * r + LD(TINY), LD(0))


def remap_check(got, ref, bound):
    """-> (problems, largest |difference| / bound, largest |difference| in ulps of the reference as a double)"""
    got = np.asarray(got, dtype=np.float64)
    bad = []
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(got[~fin], ref[~fin].astype(np.float64)):
        bad.append("entries that are not finite differ from the reference's")
    diff = np.abs(got[fin].astype(LD) - ref[fin])
    if not np.all(diff <= bound[fin]):
        i = int(np.argmax(diff - bound[fin]))
        bad.append("%d entries beyond their bound, worst: %r against %r +- %r" % (int(np.count_nonzero(diff > bound[fin])), got[fin][i], ref[fin][i], bound[fin][i]))
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(diff > 0, diff / np.where(bound[fin] > 0, bound[fin], LD(TINY)), LD(0)), initial=0.0))
        ulps = float(np.max(diff / np.spacing(np.maximum(np.abs(ref[fin].astype(np.float64)), 2.0 ** -1022)).astype(LD), initial=0.0))
    return bad, ratio, ulps


def kernel_order_remap(d_old, n_old, n_new, e, mutate=None):
    """k_strat_remap in float64: per new hypercube the mixed-radix decode (draw 0 fastest), the old index, the gather, then v | pow(v, e)"""
    q = np.arange(int(np.prod(n_new)), dtype=np.int64)
    h, stride = np.zeros_like(q), 1
    for n, m in zip(n_old, n_new):
        qn = q // int(m)
        j = q - qn * int(m)
        q = qn
        h += (2 * j + 1) * int(n) // (2 * int(m)) * stride
        stride *= int(m) if mutate == "stride_from_new" else int(n)
    v = np.asarray(d_old, dtype=np.float64)[h % len(d_old)] if mutate else np.asarray(d_old, dtype=np.float64)[h]
    with np.errstate(all="ignore"):
        return v if e == 1.0 else np.power(v, e)


# ---- the sweep's twin (tests/test_hip_strat_kernels.py: Engine.integrate_sweep_strat(adapt=False, niter=1, d=...)) --------------------------

SWEEP_PLANS = [((5, 1, 3), 8192), ((16, 16), 4096), ((40, 40), 16384)]      # 1 tile | 1 tile, full | 7 tiles
SWEEP_FAMILIES = ("lognormal", "zeros", "spike_mid", "all_zero", "huge")


def sweep_rows(nstrat, family, seed):
    """three points' d [3, ncube] of one family; the rows differ (but for all zeros)"""
    nc = int(np.prod(nstrat))
    rows = []
    for k in range(3):
        d, _ = alloc_input(dict(ncube=nc, family=family, seed=seed + k))
        rows.append(np.roll(d, 5 * k) if family in ("spike_mid", "huge") else d)
    return np.stack(rows)


ALLOC_CASES = alloc_cases()
REDUCE_CASES = reduce_cases()
REMAP_CASES = remap_cases()
