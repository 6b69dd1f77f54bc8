"""The case table, the independent reference and the float64 mirror of the block merge (csrc/mci_train.h merge_stats, merge_hist_bin,
merge_pa; their kernels k_add_host_obs, k_hist_stage1, k_finalize and k_finish in csrc/mci_static_kernels.h), shared by
tests/test_merge_host.py (the mirror against the reference, on the CPU) and tests/test_hip_merge.py (the kernels through
Engine.merge_rows).  Data and plain numpy only: no GPU code, and reference and mirror share no helper.

The reference.  In long double, from the formulas in the comments of mci_train.h (reference main.jl:273-287, configuration.jl:238-250 and
:297-298), with S[b][c] the sum of block b's rows of column c (and of the host observable, where k_add_host_obs runs first):
    m[b][o]         = S[b][o] / (S[b][norm] + 1e-10)
    packed[o]       = sum_b m          packed[nobs + o] = sum_b m^2
    normalization   = 1e-10 + sum_b (S[b][norm] + 1e-10)              neval = sum_b S[b][neval]
    visited[i]      = 1e-8 + sum_b (S[b][vis + i] + 1e-8)
    hist[bin]       = (nblocks + 1) 1e-10 (1 - hist_no_offset) + sum over the histogram rows (or the k global buffers)
    propose, accept = sum over ALL nrows rows + (nblocks + 1) {1e-8, 1e-10}
    then the 64 holding counts as doubles, or zeros
and ST_NORMALIZATION exactly when some block's S[b][norm] + 1e-10 is not > 0.

The tolerance is derived, not measured; nothing in it comes from a kernel.  With eps = 2^-52: a float64 sum of n terms x_i lies, in ANY
association, within n eps sum|x_i| of the exact sum (n - 1 additions of relative error 2^-53 each on partial sums bounded by sum|x_i|; the
factor two covers the second-order terms for every n of the table; additions of an exact zero -- idle lanes, empty groups -- cost
nothing).  The sum of absolute values, A, stands in the bound because observable columns change sign.  Carried through, per entry:
    dS[b][c]   = n eps A[b][c]                                  n = wg_per_block (+ 1 where a host observable was added)
    N = S[norm] + 1e-10:       dN = dS[norm] + eps (|N| + dS[norm])                            (the sum's bound, then one rounded add)
    m = S / N:                 dq = (dS |N| + |S| dN) / (|N| (|N| - dN)),   dm = dq + eps (|m| + dq)     (needs dN < |N|, below)
    sum_b m:                   sum_b dm + nblocks eps sum_b (|m| + dm)
    m^2:                       dm2 = dm (2 |m| + dm) + eps (|m| + dm)^2;    sum_b m^2:  sum_b dm2 + nblocks eps sum_b (m^2 + dm2)
    normalization:             sum_b dN + (nblocks + 1) eps (1e-10 + sum_b (|N| + dN))
    neval:                     sum_b dS + nblocks eps sum_b (A + dS)
    visited:                   t = S + 1e-8, dt = dS + eps (A + 1e-8 + dS);  sum_b dt + (nblocks + 1) eps (1e-8 + sum_b (A + 1e-8 + dt))
    hist, propose, accept:     (n + 2) eps (offset + sum|x|), n the rows (or buffers) summed: n + 1 terms with the offset, and one eps of
                               the offset for its own rounded product (nblocks + 1) * 1e-10
    holding counts:            exact (counts up to 2^40)
No entry is excused and there is no cap.  The inputs keep every block's normalization far from zero relative to dN (the table asserts
dN < |N| / 2^20), except in the value set "bad_norm", whose blocks of normalization -1 (still far from zero) and NaN test the status bit;
there an entry the reference has as NaN must be NaN, every other entry is held to its bound.
In the value set "integers" every addend is an integer below 2^20 and the histogram carries no offset: the block sums, neval, the
histogram and the holding counts are exact in float64 in any order and must EQUAL the reference, and propose | accept must equal
float64(exact sum) + float64 offset -- one correctly rounded addition --, so a lost or doubled row cannot hide behind rounding.

The mirror.  A float64 restatement of the kernels' order of operations (the library is built with -ffp-contract=off, so the kernels are
expected to match it bit for bit):
    k_add_host_obs  the block's first row += obs
    k_hist_stage1   per = ceil(rows / 32); group g sums rows [g per, min(rows, (g + 1) per)): four accumulators over w, w + 1, w + 2, w + 3
                    while w + 3 is in range, the tail into the first, then (s0 + s1) + (s2 + s3)
    merge_hist_bin  the offset (or 0.0) first, then the 32 groups (or the k buffers) in order
    merge_stats     eight partial sums over rows part, part + 8, ...; the butterfly xor 1, xor 2, xor 4; then the serial loops over blocks
    merge_pa        64 lanes over rows lane, lane + 64, ...; the shift-down tree 32, 16, .. 1; + float64(nblocks + 1) * offset
This order is a contract (deterministic mode rests on it): a change to it changes the mirror in the same commit, or fails the tests.
`mutate` plants one of three deliberate mistakes into the mirror (tests/test_merge_host.py: the bounds have teeth)."""
import numpy as np

LD = np.longdouble
EPS = LD(2.0) ** -52
SEED = 20261020
GROUPS = 32
ST_NORMALIZATION = 1

# nobs, ni, ncols, nbin, npa, nstat, maxn, leaves: what Engine.merge_shape() says of the engines tests build under these names
# (tests/test_merge_host.py holds offline engines to this table)
SHAPES = {
    # two Discrete leaves: nbin < 256, k_finish at 256 threads; 2 npa = 24: six full merge_pa workgroups
    "discrete2": dict(nobs=1, ni=1, ncols=5, nbin=7, npa=12, nstat=6, maxn=4, leaves=[(0, 3), (3, 4)]),
    # the chain solvers' smoke shape: ni = 2 on one pool, npa = 27 (2 npa = 54: the last merge_pa workgroup is ragged), one 999-bin leaf:
    # nbin > 256 and no multiple of it, k_finish at 512 threads
    "sphere2": dict(nobs=2, ni=2, ncols=7, nbin=999, npa=27, nstat=9, maxn=999, leaves=[(0, 999)]),
    # two Continuous leaves (300 and 40 bins) and a Discrete one: nbin = 344, k_finish at 512 threads with leaves shorter than that
    "mixed": dict(nobs=2, ni=2, ncols=7, nbin=344, npa=27, nstat=9, maxn=300, leaves=[(0, 300), (300, 40), (340, 4)]),
}
VALUES = ("uniform", "signed", "decades", "integers", "bad_norm")
HIST_ROWS = (1, 3, 31, 32, 33, 64, 65, 129, 160, 256, 2049)
USE_GHIST = (1, 3)
WG_PER_BLOCK = (1, 7, 8, 9, 17)
# 1, 2, 9, 16, 40 and one value each side of nblocks * ncols = 32 | 64, the strides of merge_stats' first loop at 256 | 512 threads:
# ncols = 5: 6 | 7 and 12 | 13; ncols = 7: 4 | 5 and 9 | 10
NBLOCKS = (1, 2, 9, 16, 40, 6, 7, 12, 13, 4, 5, 10)
NROWS = (1, 63, 64, 65, 130)          # rows of the propose | accept tables (merge_pa's 64-lane stride)
OBS_NBLOCKS = (127, 128, 129)         # k_add_host_obs: nblocks * nobs on both sides of 256 (nobs = 2) and of 128 (nobs = 1)


def _geometries():
    """(nblocks, wg_per_block, nrows): every nblocks, every wg_per_block, every table size of NROWS; nrows >= nblocks * wg_per_block,
    the rows behind the blocks' own belong to merge_pa alone (merge_stats must not read them)"""
    out = [(1, 1, 1), (9, 7, 63), (7, 9, 63), (2, 17, 64), (1, 64, 64), (16, 1, 64), (9, 7, 65), (13, 1, 65), (2, 17, 130), (16, 8, 130), (1, 130, 130)]
    for i, nb in enumerate(NBLOCKS):
        for j, wpb in enumerate(WG_PER_BLOCK):
            if (i + j) % 2 == 0 or nb in (6, 7, 12, 13, 4, 5, 10) and wpb in (1, 9):
                out.append((nb, wpb, nb * wpb + (3 if (i + j) % 3 == 0 else 0)))
    return out


GEOMETRIES = _geometries()


def build_cases():
    cases = []

    def add(problem, values, geo, hist_rows=0, use_ghist=0, obs=None, **force):
        i = len(cases)
        nblocks, wpb, nrows = geo
        c = dict(problem=problem, values=values, nblocks=nblocks, wpb=wpb, nrows=nrows, hist_rows=hist_rows, use_ghist=use_ghist, seed=SEED + i,
                 pa=i % 2 == 0, hold=(i // 2) % 2 == 0, hist_no_offset=1 if values == "integers" else (i // 3) % 2, block_means=(i // 5) % 2 == 0,
                 obs=(i % 7 == 0) if obs is None else obs)
        c.update(force)
        c["id"] = "%03d-%s-%s-b%dx%d-r%d-%s%d%s%s%s%s%s" % (i, problem, values, nblocks, wpb, nrows, "g" if use_ghist else "h", use_ghist or hist_rows,
                                                  "-pa" if c["pa"] else "", "-hold" if c["hold"] else "", "-obs" if c["obs"] else "",
                                                  "-nooff" if c["hist_no_offset"] else "", "-bm" if c["block_means"] else "")
        cases.append(c)

    problems = list(SHAPES)
    modes = [dict(hist_rows=h) for h in HIST_ROWS] + [dict(use_ghist=k) for k in USE_GHIST]
    # every histogram mode x every value set x every problem; the geometries take turns
    for a, mode in enumerate(modes):
        for b, values in enumerate(VALUES):
            for d, problem in enumerate(problems):
                add(problem, values, GEOMETRIES[(7 * a + 3 * b + d) % len(GEOMETRIES)], **mode)
    # every geometry x every value set; problems and histogram modes take turns
    for a, geo in enumerate(GEOMETRIES):
        for b, values in enumerate(VALUES):
            add(problems[(a + b) % 3], values, geo, **modes[(5 * a + b) % len(modes)])
    # host observables on both sides of one k_add_host_obs workgroup
    for a, nb in enumerate(OBS_NBLOCKS):
        for b, values in enumerate(VALUES):
            for problem in ("sphere2", "discrete2"):
                add(problem, values, (nb, WG_PER_BLOCK[(a + b) % 5], nb * WG_PER_BLOCK[(a + b) % 5]), obs=True, **modes[(3 * a + b) % len(modes)])
    # holding counts and tables present | absent in every combination, block means wanted | not wanted, on the small problems
    for values in VALUES:
        for pa in (False, True):
            for hold in (False, True):
                add("mixed" if pa else "discrete2", values, (9, 7, 65), hist_rows=33, pa=pa, hold=hold, block_means=pa != hold)
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


_CASES = None


def cases():
    """the table, built once"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def _draw(rng, values, shape):
    if values == "integers":
        return rng.integers(0, 2 ** 20, size=shape).astype(np.float64)
    if values == "decades":                        # ~30 decades between the smallest and the largest addend
        return np.exp(8.0 * rng.standard_normal(shape))
    return rng.uniform(0.5, 1.5, size=shape)       # uniform | signed | bad_norm: positive and of similar size, unless changed below


_INPUTS = {}


def inputs(c):
    """the case's made-up rows, rebuilt from its seed when they are too large to keep: dict of part_cols [nrows, ncols], part_hist
    [hist_rows, nbin] | ghist [k, nbin], part_pa [nrows, 2 npa] | None, hold [64] uint64 | None, obs [nblocks, nobs] | None"""
    if c["id"] in _INPUTS:
        return _INPUTS[c["id"]]
    sh, rng, values = SHAPES[c["problem"]], np.random.default_rng(c["seed"]), c["values"]
    nobs, nblocks, wpb, nrows = sh["nobs"], c["nblocks"], c["wpb"], c["nrows"]
    cols = _draw(rng, values, (nrows, sh["ncols"]))
    own = cols[:nblocks * wpb].reshape(nblocks, wpb, sh["ncols"])        # (a view: the blocks' own rows)
    if values == "signed":                         # observables of both signs that cancel within a block to ~1e-6 of their size
        own[:, :, :nobs] = 1.0e6 * rng.standard_normal((nblocks, wpb, nobs))
        if wpb > 1:
            own[:, -1, :nobs] = rng.standard_normal((nblocks, nobs)) - own[:, :-1, :nobs].sum(axis=1)
    if values == "decades":
        own[:, :, :nobs] *= rng.choice([-1.0, 1.0], size=(nblocks, wpb, nobs))
    if values == "bad_norm":                       # block 0: a normalization of exactly -1; the last block (or the only one, every
        kind = ("neg", "nan") if nblocks > 1 else (("neg",) if c["seed"] % 2 else ("nan",))   # other case): NaN
        if "neg" in kind:
            own[0, :, nobs] = 0.0
            own[0, wpb // 2, nobs] = -1.0
        if "nan" in kind:
            own[-1, wpb - 1, nobs] = np.nan
    out = dict(part_cols=cols, part_hist=None, ghist=None, part_pa=None, hold=None, obs=None)
    if c["hist_rows"]:
        out["part_hist"] = _draw(rng, values, (c["hist_rows"], sh["nbin"]))
    else:
        out["ghist"] = _draw(rng, values, (c["use_ghist"], sh["nbin"]))
    if c["pa"]:
        out["part_pa"] = _draw(rng, values, (nrows, 2 * sh["npa"]))
    if c["hold"]:
        out["hold"] = rng.integers(0, 2 ** 40, size=64, dtype=np.uint64)
        out["hold"][:2] = (0, 2 ** 40)
    if c["obs"]:
        out["obs"] = _draw(rng, values, (nblocks, nobs)) * (rng.choice([-1.0, 1.0], size=(nblocks, nobs)) if values in ("signed", "decades") else 1.0)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    if sum(v.nbytes for v in out.values() if v is not None) <= 1 << 20:
        _INPUTS[c["id"]] = out
    return out


def layout(c):
    """where the sections of `packed` lie: dict of (lo, hi)"""
    sh = SHAPES[c["problem"]]
    nobs, ni, nbin, npa = sh["nobs"], sh["ni"], sh["nbin"], sh["npa"]
    n = 2 * nobs + 2 + ni + 1
    assert n == sh["nstat"]
    return dict(sum=(0, nobs), sq=(nobs, 2 * nobs), norm=(2 * nobs, 2 * nobs + 1), neval=(2 * nobs + 1, 2 * nobs + 2), visited=(2 * nobs + 2, n),
                hist=(n, n + nbin), propose=(n + nbin, n + nbin + npa), accept=(n + nbin + npa, n + nbin + 2 * npa),
                hold=(n + nbin + 2 * npa, n + nbin + 2 * npa + 64))


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference (long double) and the derived bounds
# ------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(c):
    """dict of packed, bound [reduce size], scratch, dscratch [nblocks, ncols], means, dmeans [nblocks, nobs] (long double), status, and
    `exact` (None, or for "integers" a boolean mask over packed of the entries float64 must reproduce exactly); computed once per case"""
    if c["id"] in _REF:
        return _REF[c["id"]]
    sh, x, lay = SHAPES[c["problem"]], inputs(c), layout(c)
    nobs, ni, ncols, nblocks, wpb, nrows = sh["nobs"], sh["ni"], sh["ncols"], c["nblocks"], c["wpb"], c["nrows"]
    with np.errstate(all="ignore"):
        own = x["part_cols"][:nblocks * wpb].astype(LD).reshape(nblocks, wpb, ncols)
        S, A, n = own.sum(axis=1), np.abs(own).sum(axis=1), np.full(ncols, wpb, dtype=LD)
        if x["obs"] is not None:
            S[:, :nobs] += x["obs"].astype(LD)
            A[:, :nobs] += np.abs(x["obs"]).astype(LD)
            n[:nobs] += 1
        dS = n[None, :] * EPS * A
        tiny, small = LD(1.0e-10), LD(1.0e-8)
        N = S[:, nobs] + tiny
        dN = dS[:, nobs] + EPS * (np.abs(N) + dS[:, nobs])
        m = S[:, :nobs] / N[:, None]
        aN, am = np.abs(N)[:, None], np.abs(m)
        dq = (dS[:, :nobs] * aN + np.abs(S[:, :nobs]) * dN[:, None]) / (aN * (aN - dN[:, None]))
        dm = dq + EPS * (am + dq)
        dm2 = dm * (2 * am + dm) + EPS * (am + dm) ** 2
        packed = np.zeros(lay["hold"][1], dtype=LD)
        bound = np.zeros(lay["hold"][1], dtype=LD)
        packed[0:nobs], bound[0:nobs] = m.sum(axis=0), dm.sum(axis=0) + nblocks * EPS * (am + dm).sum(axis=0)
        packed[nobs:2 * nobs], bound[nobs:2 * nobs] = (m * m).sum(axis=0), dm2.sum(axis=0) + nblocks * EPS * (m * m + dm2).sum(axis=0)
        packed[2 * nobs], bound[2 * nobs] = tiny + N.sum(), dN.sum() + (nblocks + 1) * EPS * (tiny + (np.abs(N) + dN).sum())
        packed[2 * nobs + 1] = S[:, nobs + 1].sum()
        bound[2 * nobs + 1] = dS[:, nobs + 1].sum() + nblocks * EPS * (A[:, nobs + 1] + dS[:, nobs + 1]).sum()
        vis = slice(nobs + 2, nobs + 3 + ni)
        dt = dS[:, vis] + EPS * (A[:, vis] + small + dS[:, vis])
        lo, hi = lay["visited"]
        packed[lo:hi] = small + (S[:, vis] + small).sum(axis=0)
        bound[lo:hi] = dt.sum(axis=0) + (nblocks + 1) * EPS * (small + (A[:, vis] + small + dt).sum(axis=0))
        rows = x["part_hist"] if x["part_hist"] is not None else x["ghist"]
        off = LD(0.0) if c["hist_no_offset"] else LD(nblocks + 1) * tiny
        lo, hi = lay["hist"]
        packed[lo:hi] = off + rows.astype(LD).sum(axis=0)
        bound[lo:hi] = (rows.shape[0] + 2) * EPS * (off + np.abs(rows).astype(LD).sum(axis=0))
        for name, o in (("propose", small), ("accept", tiny)):
            lo, hi = lay[name]
            tab = np.zeros((1, 2 * sh["npa"])) if x["part_pa"] is None else x["part_pa"]
            tab = tab[:, lo - lay["propose"][0]:hi - lay["propose"][0]].astype(LD)
            packed[lo:hi] = tab.sum(axis=0) + LD(nblocks + 1) * o
            if c["values"] == "integers":           # one correctly rounded float64 addition to an exact sum
                packed[lo:hi] = (tab.sum(axis=0).astype(np.float64) + np.float64(nblocks + 1) * np.float64(o)).astype(LD)
            bound[lo:hi] = (nrows + 2) * EPS * (np.abs(tab).sum(axis=0) + LD(nblocks + 1) * o)
        lo, hi = lay["hold"]
        if x["hold"] is not None:
            packed[lo:hi] = x["hold"].astype(LD)
        exact = None
        if c["values"] == "integers":
            exact = np.zeros(packed.size, dtype=bool)
            exact[2 * nobs + 1] = True
            exact[slice(*lay["hist"])] = exact[slice(*lay["hold"])] = exact[lay["propose"][0]:lay["accept"][1]] = True
        status = ST_NORMALIZATION if not np.all(N > 0) else 0
    out = dict(packed=packed, bound=bound, scratch=S, dscratch=dS, means=m, dmeans=dm, status=status, exact=exact, N=N, dN=dN)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REF[c["id"]] = out
    return out


def _held(got, ref, bound, exact, who, what):
    """got within bound of ref entry by entry (NaN where and only where ref is NaN; equal where `exact`); returns the largest ratio
    of a difference to its bound"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (who, what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: %s is NaN at %s, the reference at %s" % (who, what, np.flatnonzero(np.isnan(got).ravel())[:8],
                                                                                           np.flatnonzero(nan.ravel())[:8])
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - ref)
    if exact is not None:
        bad = np.flatnonzero((exact & ~nan & (err != 0)).ravel())
        assert bad.size == 0, "%s: %s differs from the exact sum at %s: %r, exact %r" % (who, what, bad[:8], got.ravel()[bad[:8]],
                                                                                        ref.ravel()[bad[:8]].astype(np.float64))
    ok = nan | (err <= bound)
    bad = np.flatnonzero(~ok.ravel())
    assert bad.size == 0, "%s: %s off at %s by %r, the derived bounds are %r" % (who, what, bad[:8], err.ravel()[bad[:8]].astype(np.float64),
                                                                             bound.ravel()[bad[:8]].astype(np.float64))
    with np.errstate(all="ignore"):
        ratio = np.where(nan | (err == 0), LD(0.0), err / bound)          # (err != 0 implies bound >= err > 0 here)
    return float(ratio.max()) if ratio.size else 0.0


def check(c, out, who):
    """what a merge left -- dict of packed, scratch, block_means (or None), status -- against the reference under the rules of the
    module's docstring; returns the largest ratio of an observed difference to its derived bound"""
    r = reference(c)
    who = "%s, case %s" % (who, c["id"])
    ex = c["values"] == "integers"
    worst = _held(out["packed"], r["packed"], r["bound"], r["exact"], who, "packed")
    worst = max(worst, _held(out["scratch"], r["scratch"], r["dscratch"], np.ones(r["scratch"].shape, dtype=bool) if ex else None, who, "scratch"))
    if out.get("block_means") is not None:
        worst = max(worst, _held(out["block_means"], r["means"], r["dmeans"], None, who, "block means"))
    assert out["status"] == r["status"], "%s: status %d, the reference %d" % (who, out["status"], r["status"])
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# the mirror (float64, the kernels' order of operations)
# ------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_row", "short_row_loop", "per_floor")


def mirror(c, mutate=None, shape=None, x=None):
    """dict of packed [reduce size], stage1 [32, nbin] (NaN without a first stage), scratch [nblocks, ncols], block_means [nblocks, nobs]
    (None if the case does not want them), status, part_cols [nrows, ncols] as k_add_host_obs leaves them.
    shape, x: a problem shape (Engine.merge_shape) and rows (as `inputs` returns them) of the caller's own instead of the table's.
    mutate: None | "drop_last_row" (the first stage loses the last row of its last non-empty group) | "short_row_loop" (merge_stats' row
    loop stops at wg_per_block - wg_per_block % 8) | "per_floor" (the first stage takes per = rows // 32)"""
    assert mutate is None or mutate in MUTATIONS
    sh, x = shape or SHAPES[c["problem"]], x or inputs(c)
    nobs, ni, ncols, nbin, npa = sh["nobs"], sh["ni"], sh["ncols"], sh["nbin"], sh["npa"]
    nblocks, wpb, nrows = c["nblocks"], c["wpb"], c["nrows"]
    nstat = 2 * nobs + 2 + ni + 1
    packed = np.full(nstat + nbin + 2 * npa + 64, np.nan)
    f8 = np.float64
    with np.errstate(all="ignore"):
        # k_add_host_obs
        cols = x["part_cols"].copy()
        if x["obs"] is not None:
            for b in range(nblocks):
                cols[b * wpb, :nobs] += x["obs"][b]
        # k_hist_stage1
        stage1 = np.full((GROUPS, nbin), np.nan)
        if x["part_hist"] is not None:
            ph, nwg = x["part_hist"], c["hist_rows"]
            per = nwg // GROUPS if mutate == "per_floor" else (nwg + GROUPS - 1) // GROUPS
            last = max(g for g in range(GROUPS) if g * per < nwg) if per else 0
            for g in range(GROUPS):
                w0 = g * per
                w1 = min(nwg, w0 + per)
                if mutate == "drop_last_row" and g == last:
                    w1 -= 1
                s = [np.zeros(nbin) for _ in range(4)]
                w = w0
                while w + 3 < w1:
                    for k in range(4):
                        s[k] = s[k] + ph[w + k]
                    w += 4
                while w < w1:
                    s[0] = s[0] + ph[w]
                    w += 1
                stage1[g] = (s[0] + s[1]) + (s[2] + s[3])
        # merge_hist_bin
        h = np.zeros(nbin) if c["hist_no_offset"] else np.full(nbin, f8(nblocks + 1) * f8(1.0e-10))
        for row in (stage1 if x["part_hist"] is not None else x["ghist"]):
            h = h + row
        packed[nstat:nstat + nbin] = h
        # merge_stats: the block sums
        own = cols[:nblocks * wpb].reshape(nblocks, wpb, ncols)
        stop = wpb - wpb % 8 if mutate == "short_row_loop" else wpb
        part = []
        for p in range(8):
            s = np.zeros((nblocks, ncols))
            for w in range(p, stop, 8):
                s = s + own[:, w, :]
            part.append(s)
        scratch = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))
        # ... and the serial loops over the blocks
        means = np.empty((nblocks, nobs))
        tot, sq, norm, neval, vis = np.zeros(nobs), np.zeros(nobs), f8(1.0e-10), f8(0.0), np.full(ni + 1, 1.0e-8)
        bad = False
        for b in range(nblocks):
            nb = scratch[b, nobs] + f8(1.0e-10)
            m = scratch[b, :nobs] / nb
            tot = tot + m
            sq = sq + m * m
            means[b] = m
            bad = bad or not nb > 0.0
            norm = norm + nb
            neval = neval + scratch[b, nobs + 1]
            vis = vis + (scratch[b, nobs + 2:] + f8(1.0e-8))
        packed[:nobs], packed[nobs:2 * nobs], packed[2 * nobs], packed[2 * nobs + 1], packed[2 * nobs + 2:nstat] = tot, sq, norm, neval, vis
        # merge_pa
        lanes = np.zeros((64, 2 * npa))
        if x["part_pa"] is not None:
            for r in range(nrows):
                lanes[r % 64] = lanes[r % 64] + x["part_pa"][r]
        width = 32
        while width:
            lanes[:width] = lanes[:width] + lanes[width:2 * width]
            width //= 2
        offs = np.where(np.arange(2 * npa) < npa, 1.0e-8, 1.0e-10)
        packed[nstat + nbin:nstat + nbin + 2 * npa] = lanes[0] + f8(nblocks + 1) * offs
        packed[nstat + nbin + 2 * npa:] = 0.0 if x["hold"] is None else x["hold"].astype(np.float64)
    return dict(packed=packed, stage1=stage1, scratch=scratch, block_means=means if c["block_means"] else None,
                status=ST_NORMALIZATION if bad else 0, part_cols=cols)
