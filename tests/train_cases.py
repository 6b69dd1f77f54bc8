"""The case table, the independent reference and the derived bounds of train! on its own (csrc/mci_train.h train_leaf, do_reweight_dev and
iteration_bookkeeping; their kernels k_train and k_finish in csrc/mci_static_kernels.h), shared by tests/test_train_host.py (the CPU oracle
against the reference, planted mistakes, the table's own conditions) and tests/test_hip_train.py (the kernels through Engine.set_grid ->
set_packed -> train).  Data and plain numpy only: no GPU code.  Everything is seeded and a pure function of its arguments.

The reference.  In long double (64-bit mantissa), written as the operation and not in any kernel's order (reference variable.jl:206-239,
:369-382, common.jl:43-82, main.jl:322-346):
    Continuous   d = smooth(h): (7 h[0] + h[1]) / 8 and (7 h[N-1] + h[N-2]) / 8 at the ends, (h[i-1] + 6 h[i] + h[i+1]) / 8 inside (N = 1: h)
                 v = d / sum(d);  d = ((1 - v) / (-log v)) ^ alpha where 0 < v <= 0.99999999, else v            (N = 1: left alone)
                 C[j] = d[0] + .. + d[j];  F = the piecewise-linear cumulative of d over the old grid, F(g[j+1]) = C[j]
                 new point i = F^-1(i C[N-1] / N) for 0 < i < N; both end points copied
    Discrete     v = h / sum(h), the same rescale without smoothing (K = 1: left alone), dist = d / sum(d), acc[0] = 0, acc[i+1] = acc[i] + dist[i]
    doReweight!  w[i] = r[i] (A / visited[i]) ^ gamma  (visited[i] <= 1: r[i] A ^ gamma),  A = sum(visited);  w[i] *= goal[i] / sum(goal);  w / sum(w)

The bounds are derived, not measured; nothing in them comes from a kernel.  u = 2^-53, eps = 2 u.  Every quantity below is positive, so a
float64 sum of n terms lies within n u of the exact sum RELATIVELY, in any association, and a product / quotient / rounded constant costs u.
    smoothing                 two products, two additions, one division:                                   4 u
    v = d / sum(d)            the sum N u, the division u:                                                 (N + 5) u
    b = (1 - v) / (-log v)    the subtraction u, the logarithm L ulp = 2 L u OF ITS RESULT, the division u: (2 + 2 L) u of its own, and
                              |dlog b / dlog v| = |1 / (-log v) - v / (1 - v)| <= 1/2 < 1 on (0, 1) carries v's error over at most once
    b ^ alpha                 alpha times b's relative error, plus P ulp = 2 P u of pow() (b b: u; b b b: 2 u; both below 2 P u)
    => every rescaled bin     rho = [alpha (N + 5) + alpha (2 + 2 L) + 2 P + 2] u          relatively  (N -> K and no smoothing for Discrete: the same form holds)
L and P are the limits the OpenCL C specification sets for double-precision log (3 ulp) and pow (16 ulp): the device's math library is
written to that specification, and the host's libm (the oracle's) is well inside it.  The same two constants serve oracle and kernel.
Continuous.  Both walks compare partial sums of d with multiples of f_ninc = C / N.  The prefix-scan form: C[j] and the total within N u C
each, the target i f_ninc within 2 u more.  The serial recurrence: at most 2 N rounded additions / subtractions on an acc_f <= max d + f_ninc
<= C (1 + 1/N), and the error of f_ninc (N u) times i <= N.  Either way the computed F differs from the reference's by no more than
    dC = eps C [(2 + alpha) N + alpha (7 + 2 L) + 2 P + 4]            (the walk's 2 N u C twice over, rho C, and the small change)
UNIFORMLY over the grid, the interpolation inside a bin included (it divides by the same d[j]).  F^-1 is monotone, so the point the code
finds for target t lies in [F^-1(t - dC), F^-1(t + dC)] -- evaluated with the reference's own F, over however many bins that interval
crosses (a decision that flips at a tie moves the point continuously; in a bin of the 1e-10 fill the interval is wide because the point
really is that ill-determined).  On top: the interpolation g[j+1] - (acc_f / d[j]) (g[j+1] - g[j]) rounds four times on numbers no larger
than max|g|:  4 eps max|g|  (generous by 2).  The end points carry bound 0: they are copies.
Discrete.  dist = d / sum(d): 2 rho + (K + 2) u relatively; acc[i]: i more additions, (i + K + 2) u + 2 rho relatively; acc[0] = 0 exactly.
doReweight!.  A: nd u; the quotient u; pow: gamma (nd + 1) u + 2 P u; the product u; the goal factor (nd + 2) u:  rw = [(gamma + 1)(nd + 1) + 2 P + 3] u
before the normalisation, 2 rw + (nd + 1) u after it.

`replay` is a float64 restatement of train! in the plainest order (not the kernels'), into which `mutate` plants one of three deliberate
mistakes (tests/test_train_host.py: the bounds have teeth)."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
EPS = LD(2.0) ** -52
SEED = 20261020
ULP_LOG, ULP_POW = 3, 16
THRESHOLD = 0.99999999
LOWER, UPPER = -1.0, 3.0

# csrc/mci_train.h train_lds_doubles, train_spare_doubles, kWalkPad; csrc/mci_host_types.h kTrainLdsMax, kMaxLeafBins, train_threads
WALK_PAD = 64
TRAIN_LDS_MAX = 160 * 1024 - 4096
MAX_LEAF_BINS = 4400


def lds_doubles(n):
    return (n + WALK_PAD) + (n + 2) + (n + WALK_PAD) + 2


def spare_doubles(n):
    return 2 * (2 * n + WALK_PAD) + (2 * n + WALK_PAD) // 16 + 2


def has_spare(n):
    """train_lds_bytes' *spare: the serial walk's slots fit next to the refinement's scratch"""
    return (lds_doubles(n) + spare_doubles(n)) * 8 <= TRAIN_LDS_MAX


N_FIT = max(n for n in range(1, MAX_LEAF_BINS + 1) if has_spare(n))


def train_threads(maxn):
    return 512 if maxn > 256 else 256


SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 511, 512, 513, 999, 1023, 1024, 1025, 2047, 2048, 2049, N_FIT, N_FIT + 1,
         4399, 4400)
SIDE_ALPHAS = (1.0, 3.0, 1.5, 0.5)
SIDE_SIZES = (17, 257, 999, 1025)
DISCRETE_K = (1, 2, 3, 4, 17, 1024, 1025, 4400)
DISCRETE_ALPHAS = (2.0, 1.5)
DISCRETE_SIDE_ALPHAS = (3.0, 1.0)          # rescale_pow's other two fast paths (a Continuous leaf takes its power from a lambda of its own)
DISCRETE_SIDE_K = (3, 17, 1025)
FAMILIES = ("flat", "ones", "spike", "spike_first", "spike_last", "comb", "ramp", "lognormal", "tiny", "pow2")
GRIDS = ("uniform", "adapted")
# the mixed problem's leaves: (kind, bins, alpha, adapt); train_threads(1200) = 512 for every leaf
MIXED = (("c", 1200, 2.0, True), ("c", 41, 2.0, True), ("c", 17, 2.0, False), ("d", 4, 2.0, True), ("d", 3, 2.0, False), ("c", 17, 2.0, True))
BAD_VALUES = (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("minus_one", -1.0), ("minus_zero", -0.0))
BAD_N = 999


def bad_places(n, threads=None):
    """first, middle, last, and the last bin a thread of the second wave owns (train_leaf's check strides the bins by the thread count)"""
    t = threads or train_threads(n)
    return dict(first=0, middle=n // 2, last=n - 1, second_wave=127 + t * ((n - 1 - 127) // t))


def problem_name(kind, n, alpha):
    return "%s%d-a%g" % (kind, n, alpha)


def hist(n, family):
    """the made-up histogram of n bins"""
    rng = np.random.default_rng([SEED, n, FAMILIES.index("lognormal" if family == "pow2" else family)])
    if family == "flat":
        h = np.full(n, 1.0e-10)
    elif family == "ones":
        h = np.ones(n)
    elif family in ("spike", "spike_first", "spike_last"):
        h = np.full(n, 1.0e-10)
        h[{"spike": n // 3, "spike_first": 0, "spike_last": n - 1}[family]] = 1.0e6
    elif family == "comb":
        h = np.where(np.arange(n) % 2 == 0, 1.0, 1.0e-10)
    elif family == "ramp":
        h = 1.0 + np.arange(n, dtype=np.float64)
    elif family in ("lognormal", "pow2"):
        h = np.exp(8.0 * rng.standard_normal(n))
        if family == "pow2":
            h = h * 2.0 ** 40
    elif family == "tiny":
        h = 1.0e-300 * rng.uniform(0.5, 1.5, n)
    else:
        raise KeyError(family)
    h.setflags(write=False)
    return h


ASSOC_K, ASSOC_ALPHA, ASSOC_BIN = 1025, 1.0, 512


def assoc_hist():
    """A Discrete histogram of 1025 bins on which the ASSOCIATION of Julia's sum() (sum_julia: halves of 513 | 512 elements, sixteen
    interleaved partial sums each) shows far above rounding.  Bin 512 holds 2^60 (one ulp: 256), bins 528, 544, .. 1024 hold 127, every
    other bin 256.  Split 513 | 512: bin 512 closes the first half's partial 0 and every partial sum is exact; the 32 bins of 127 meet in
    the second half's partial 15, 4064 together, and the total is 2^60 + 258016, rounded once: 2^60 + 258048.  Split 512 | 513 instead:
    bin 512 OPENS the second half's partial 0 and the 32 bins of 127 are added to it one by one, each below half an ulp and lost:
    2^60 + 253952, sixteen ulps less.  Bin 512 is the one bin the rescale leaves alone (v = h / sum(h) > 0.99999999) and with alpha = 1 the
    other bins, 1 / (-log v) ~ 1 / 36 each, make up 97 % of sum(d): distribution[512] = v / sum(d) follows sum(h) at 0.97 of its relative
    change, 31 units of 2^-53, while the logarithms of the other bins move it by a few."""
    h = np.full(ASSOC_K, 256.0)
    h[ASSOC_BIN] = 2.0 ** 60
    h[ASSOC_BIN + 16::16] = 127.0
    h.setflags(write=False)
    return h


def sum_julia64(v, split=lambda n: ((n - 1) >> 1) + 1):
    """mcio_sum_julia / sum_julia in float64 with the split left open (tests/test_train_host.py: the histogram above tells two splits apart)"""
    v = np.asarray(v, dtype=np.float64)
    if v.size > 1024:
        h = split(v.size)
        return sum_julia64(v[:h], split) + sum_julia64(v[h:], split)
    p = np.zeros(16)
    for i in range(0, v.size, 16):
        blk = v[i:i + 16]
        p[:blk.size] = p[:blk.size] + blk
    for h in (8, 4, 2, 1):
        p[:h] = p[:h] + p[h:2 * h]
    return float(p[0])


def grid(n, kind):
    """the old grid of n bins on [LOWER, UPPER]: uniform, or strictly increasing with widths spread over about six decades"""
    if kind == "uniform":
        g = np.linspace(LOWER, UPPER, n + 1)
    else:
        w = np.exp(2.0 * np.random.default_rng([SEED, n, 99]).standard_normal(n)).astype(LD)
        g = (LD(LOWER) + np.concatenate([[LD(0.0)], np.cumsum(w)]) / w.sum() * LD(UPPER - LOWER)).astype(np.float64)
        g[0], g[-1] = LOWER, UPPER
    assert g.shape == (n + 1,) and np.all(np.diff(g) > 0), (n, kind)          # what mci_set_grid checks
    g.setflags(write=False)
    return g


def build_cases():
    cases = []

    def add(**c):
        c["id"] = "%04d-%s-%s-%s" % (len(cases), c["problem"], c["grid"], c["family"])
        cases.append(c)

    for n in SIZES:
        for gk in GRIDS:
            for fam in FAMILIES:
                add(problem=problem_name("c", n, 2.0), kind="c", n=n, alpha=2.0, grid=gk, family=fam)
    for alpha in SIDE_ALPHAS:
        for n in SIDE_SIZES:
            for a, gk in enumerate(GRIDS):
                for b, fam in enumerate(FAMILIES):
                    if (a + b) % 2 == 0 or fam in ("spike", "lognormal"):     # (thinned: every family on one of the grids, two on both)
                        add(problem=problem_name("c", n, alpha), kind="c", n=n, alpha=alpha, grid=gk, family=fam)
    for alpha in DISCRETE_ALPHAS:
        for k in DISCRETE_K:
            for fam in FAMILIES:
                add(problem=problem_name("d", k, alpha), kind="d", n=k, alpha=alpha, grid="none", family=fam)
    for alpha in DISCRETE_SIDE_ALPHAS:
        for k in DISCRETE_SIDE_K:
            for fam in FAMILIES:
                add(problem=problem_name("d", k, alpha), kind="d", n=k, alpha=alpha, grid="none", family=fam)
    for i in range(len(FAMILIES)):                                            # leaf l takes family i + l: every family on every leaf
        add(problem="mixed", kind="m", n=0, alpha=2.0, grid=GRIDS[i % 2], family="rot%d" % i,
            families=tuple(FAMILIES[(i + l) % len(FAMILIES)] for l in range(len(MIXED))))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def problems():
    """name -> the leaves [(kind, bins, alpha, adapt)] of every problem the table needs, in the table's order"""
    out = {}
    for c in cases():
        out.setdefault(c["problem"], list(MIXED) if c["kind"] == "m" else [(c["kind"], c["n"], c["alpha"], True)])
    for k, n, a, ad in MIXED:                      # ... and every adapting leaf of the mixed problem as a problem of its own
        if ad:
            out.setdefault(problem_name(k, n, a), [(k, n, a, True)])
    return out


def leaf_inputs(c):
    """per leaf of the case's problem: (kind, bins, alpha, adapt, old grid | None, histogram)"""
    if c["kind"] == "m":
        return [(k, n, a, ad, grid(n, c["grid"]) if k == "c" else None, hist(n, fam)) for (k, n, a, ad), fam in zip(MIXED, c["families"])]
    return [(c["kind"], c["n"], c["alpha"], True, grid(c["n"], c["grid"]) if c["kind"] == "c" else None, hist(c["n"], c["family"]))]


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference (long double) and the derived bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _rho(n, alpha):
    return (LD(alpha) * (n + 5) + LD(alpha) * (2 + 2 * ULP_LOG) + 2 * ULP_POW + 2) * U


def _rescale(v, alpha):
    m = (v > 0) & (v <= LD(THRESHOLD))
    out = v.copy()
    with np.errstate(all="ignore"):
        out[m] = np.power((1 - v[m]) / (-np.log(v[m])), LD(alpha))
    return out


def rescaled(h, alpha, smooth=True):
    """the rescaled distribution d of a histogram, in long double"""
    h = np.asarray(h).astype(LD)
    n = h.size
    if n == 1:
        return h.copy()
    d = h.copy()
    if smooth:
        d[0], d[-1] = (7 * h[0] + h[1]) / 8, (7 * h[-1] + h[-2]) / 8
        d[1:-1] = (h[:-2] + 6 * h[1:-1] + h[2:]) / 8
    return _rescale(d / d.sum(), alpha)


def _finv(g, d, C, c):
    """F^-1 of the piecewise-linear cumulative: F(g[j]) = C[j-1], slope d[j] / (g[j+1] - g[j]) inside bin j"""
    n = d.size
    c = np.clip(c, LD(0.0), C[-1])
    j = np.clip(np.searchsorted(C, c, side="left"), 0, n - 1)
    before = np.where(j > 0, C[np.maximum(j - 1, 0)], LD(0.0))
    return g[j] + (c - before) / d[j] * (g[j + 1] - g[j])


_REF = {}


def ref_continuous(g, h, alpha):
    """(new grid, bound per point) in long double; computed once per distinct input"""
    key = ("c", g.tobytes(), h.tobytes(), alpha)
    if key in _REF:
        return _REF[key]
    n = h.size
    gl, d = g.astype(LD), rescaled(h, alpha)
    C = np.cumsum(d)
    t = np.arange(n + 1).astype(LD) * C[-1] / n
    new = _finv(gl, d, C, t)
    dC = EPS * C[-1] * ((2 + LD(alpha)) * n + LD(alpha) * (7 + 2 * ULP_LOG) + 2 * ULP_POW + 4)
    bound = np.maximum(_finv(gl, d, C, t + dC) - new, new - _finv(gl, d, C, t - dC)) + 4 * EPS * np.abs(gl).max()
    new[0], new[-1], bound[0], bound[-1] = gl[0], gl[-1], 0, 0
    for a in (new, bound):
        a.setflags(write=False)
    _REF[key] = new, bound
    return new, bound


def ref_discrete(h, alpha):
    """(distribution, its bound, accumulation, its bound) in long double"""
    key = ("d", h.tobytes(), alpha)
    if key in _REF:
        return _REF[key]
    k = h.size
    d = rescaled(h, alpha, smooth=False)
    dist = d / d.sum()
    acc = np.concatenate([[LD(0.0)], np.cumsum(dist)])
    rho = _rho(k, alpha)
    dd = (2 * rho + (k + 2) * U) * dist
    da = (2 * rho + (np.arange(k + 1) + k + 2) * U) * acc
    da[0] = 0
    for a in (dist, dd, acc, da):
        a.setflags(write=False)
    _REF[key] = dist, dd, acc, da
    return _REF[key]


def ref_reweight(r, visited, gamma, goal=None):
    """(reweight, bound) of doReweight! in long double"""
    r, v = np.asarray(r).astype(LD), np.asarray(visited).astype(LD)
    nd, A = r.size, v.sum()
    with np.errstate(all="ignore"):
        w = r * np.where(v <= 1, np.power(A, LD(gamma)), np.power(A / np.where(v <= 1, LD(1.0), v), LD(gamma)))
    if goal is not None:
        gl = np.asarray(goal).astype(LD)
        w = w * (gl / gl.sum())
    out = w / w.sum()
    rw = ((LD(gamma) + 1) * (nd + 1) + 2 * ULP_POW + 3) * U
    return out, (2 * rw + (nd + 1) * U) * out


def ratio(got, ref, bound, who):
    """largest |got - ref| / bound; where the bound is 0 the entry must equal the reference"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (who, got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    zero = bound == 0
    assert not np.any(err[zero] != 0), "%s: an entry that is a plain copy differs at %s" % (who, np.flatnonzero(zero & (err != 0))[:8])
    with np.errstate(all="ignore"):
        q = np.where(zero, LD(0.0), err / np.where(zero, LD(1.0), bound))
    return float(q.max())


def check_leaf(leaf, out, who):
    """what train! left for one ADAPTING leaf -- the new grid, or (distribution, accumulation) -- against the reference; returns (the
    largest ratio of a difference to its bound, max |difference| / (upper - lower) for a grid, else 0)"""
    kind, n, alpha, adapt, g, h = leaf
    if kind == "c":
        ref, bound = ref_continuous(g, h, alpha)
        return ratio(out, ref, bound, who), float(np.abs(np.asarray(out).astype(LD) - ref).max() / LD(g[-1] - g[0]))
    dist, dd, acc, da = ref_discrete(h, alpha)
    return max(ratio(out[0], dist, dd, who + " distribution"), ratio(out[1], acc, da, who + " accumulation")), 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# a float64 restatement in the plainest order, with room for a planted mistake
# ------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("end_weight_6", "target_plus_one", "acc_shift")


def _rescale64(d, alpha):
    if d.size == 1:
        return d.copy()
    v = d / d.sum()
    m = (v > 0) & (v <= THRESHOLD)
    out = v.copy()
    out[m] = (-(1.0 - v[m]) / np.log(v[m])) ** alpha
    return out


def replay_continuous(g, h, alpha, mutate=None):
    """train!(Continuous) in float64: smooth, rescale, cumulative, one interpolation per new point"""
    assert mutate in (None,) + MUTATIONS
    n = h.size
    w = 6.0 if mutate == "end_weight_6" else 7.0
    d = np.array(h, dtype=np.float64)
    if n > 1:
        d[0], d[-1] = (h[0] * w + h[1]) / 8.0, (h[-1] * w + h[-2]) / 8.0
        d[1:-1] = (h[:-2] + h[1:-1] * 6.0 + h[2:]) / 8.0
    d = _rescale64(d, alpha)
    C = np.cumsum(d)
    f = C[-1] / n
    i = np.arange(n + 1)
    t = np.minimum((i + 1 if mutate == "target_plus_one" else i) * f, C[-1])
    j = np.clip(np.searchsorted(C, t, side="left"), 0, n - 1)
    new = g[j + 1] - ((C[j] - t) / d[j]) * (g[j + 1] - g[j])
    new[0], new[-1] = g[0], g[-1]
    return new


def replay_discrete(h, alpha, mutate=None):
    assert mutate in (None,) + MUTATIONS
    d = _rescale64(np.array(h, dtype=np.float64), alpha)
    dist = d / d.sum()
    acc = np.concatenate([[0.0], np.cumsum(dist)])
    if mutate == "acc_shift":                      # acc[i + 1] written ahead of the addition
        acc = np.concatenate([[0.0], acc[:-1]])
    return dist, acc


def walk_stays_inside(d, f_ninc):
    """the reference's recurrence (variable.jl:227-232) on the float64 d and f_ninc the oracle has: the largest j it reaches"""
    n, j, acc = len(d), 0, 0.0
    d = [float(x) for x in d]
    for _ in range(2, n + 1):
        while acc < f_ninc:
            if j >= n:
                return j + 1
            acc += d[j]
            j += 1
        acc -= f_ninc
    return j
