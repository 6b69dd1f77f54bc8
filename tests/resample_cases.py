"""The case table and the independent reference of the carried chains' resampler (csrc/mci_train.h resample_block; its callers
k_resample_chains and a carried sweep point's workgroup; the oracle's mirrors mcio_resample_chains | mcio_resample_weighted), shared by
tests/test_resample_host.py (the mirrors, on the CPU) and tests/test_hip_resample.py (the kernel through Engine.resample).  Data and
plain numpy only: no GPU code, nothing of the kernel's or the mirrors' arithmetic.

The reference.  In long double,
    W_ref   = cumsum(w)                   (:mcmc: w[j] = rw_now[curr[j]] / rw_used[curr[j]])
    t_ref   = (arange(n_new) + 0.6180339887498949) * (W_ref[-1] / n_new)
    src_ref = minimum(searchsorted(W_ref, t_ref, side="right"), n_old - 1)
and src_ref[c] = c % n_old where W_ref[-1] is not > 0 (every weight zero, or a total that is not a number).

The tolerance is derived, not measured.  A float64 running sum of n non-negative terms lies, in any association, within n 2^-52 total of
the exact sum (n - 1 additions, each within 2^-53 relative of a partial sum that is at most the total, and the slack of the factor two
covers the second-order terms for every n of the table); the :mcmc form, a sum of nd products of a rounded quotient and an exact count,
within (nd + 1) 2^-52 total.  So with gamma = max(n_old, nd + 1) 2^-52 W_ref[-1]:
  * W of the kernel lies within gamma of W_ref, and does not decrease;
  * a pick a = src[c] may differ from b = src_ref[c] only if every W_ref[j], j in [min(a, b), max(a, b)), lies within 2 gamma of t_ref[c]
    (those are the running weights the two sides put on different sides of the target: one gamma for W, one for the target, which is
    the total times a factor below one, rounded twice).  Differing by one is NOT the criterion: chains of weight zero in between are
    skipped by either side;
  * per case at most 1e-3 of the picks may be let through by that clause (CAP), which keeps it from hiding a broken bisection.
tests/test_resample_host.py holds the mirrors to these rules over the whole table, so the table is proven to fit within the cap
without the kernel."""
import numpy as np

U = 0.6180339887498949
CAP = 1e-3
SEED = 20261020
N_OLD = (1, 2, 7, 255, 256, 257, 300, 513, 8192, 8193, 20000)    # stretch edges (per = ceil(n_old / 256) changes at 256 | 257 | 513: empty
                                                                 # stretches, two-chain stretches), the static kernel's LDS limit 8192 | 8193
N_NEW = ("one", "same", "twice+1", "third")
ND = (2, 5, 16, 17, 33, 64)                                       # counts in registers up to 16, the pass per integrand beyond
WEIGHTS = ("ones", "uniform", "lognormal", "sparse", "ends")


def n_new_of(kind, n_old):
    return {"one": 1, "same": n_old, "twice+1": 2 * n_old + 1, "third": max(1, n_old // 3)}[kind]


def _weights(rng, kind, shape):
    nblocks, n_old = shape
    if kind == "ones":
        return np.ones(shape)
    if kind == "uniform":
        return rng.random(shape)
    if kind == "lognormal":                       # ~30 decades between the smallest and the largest weight
        return np.exp(8.0 * rng.standard_normal(shape))
    if kind == "sparse":                          # 95 % exact zeros, at least one positive weight per block
        w = np.where(rng.random(shape) < 0.95, 0.0, rng.random(shape) + 0.01)
        w[np.arange(nblocks), rng.integers(0, n_old, size=nblocks)] = rng.random(nblocks) + 0.01
        return w
    if kind == "ends":                            # one positive weight on the first stored chain, one on the last
        w = np.zeros(shape)
        w[:, 0] = rng.random(nblocks) + 0.01
        w[:, -1] += rng.random(nblocks) + 0.01
        return w
    raise KeyError(kind)


def _case(cid, expect, nblocks, n_old, n_new, nd=1, w_chain=None, curr=None, rw_now=None, rw_used=None):
    c = dict(id=cid, expect=expect, nblocks=nblocks, n_old=n_old, n_new=n_new, nd=nd, w_chain=w_chain)
    c["curr"] = np.zeros((nblocks, n_old), dtype=np.int32) if curr is None else np.ascontiguousarray(curr, dtype=np.int32)
    c["rw_now"] = np.ones(nd) if rw_now is None else np.asarray(rw_now, dtype=np.float64)
    c["rw_used"] = np.ones(nd) if rw_used is None else np.asarray(rw_used, dtype=np.float64)
    return c


def _mcmc_factors(rng, nd):
    used = rng.uniform(0.1, 1.1, size=nd)
    return used * np.exp(rng.standard_normal(nd)), used


def build_cases():
    """expect: "ref" (the long-double reference under the rules above) | "fallback" (c % n_old, exactly) | "mirror" (a total of +inf:
    kernel and mirror are compared with each other only)"""
    cases = []

    def rng():
        return np.random.default_rng(SEED + len(cases))

    # a weight per stored chain (:vegasmc): every n_old x every n_new x every kind of weights; one and three blocks take turns
    for i, n_old in enumerate(N_OLD):
        for j, nn in enumerate(N_NEW):
            for k, kind in enumerate(WEIGHTS):
                nblocks = 3 if (i + j + k) % 2 else 1
                cases.append(_case("w-%s-%d-%s-b%d" % (kind, n_old, nn, nblocks), "ref", nblocks, n_old, n_new_of(nn, n_old),
                                   w_chain=_weights(rng(), kind, (nblocks, n_old))))
    # a weight per integrand (:mcmc): every nd x every n_old, once with one block and once with three, the n_new taking turns
    for i, nd in enumerate(ND):
        for j, n_old in enumerate(N_OLD):
            for nblocks, nn in ((1, N_NEW[(i + j) % 4]), (3, N_NEW[(i + j + 2) % 4])):
                r = rng()
                now, used = _mcmc_factors(r, nd)
                cases.append(_case("m-nd%d-%d-%s-b%d" % (nd, n_old, nn, nblocks), "ref", nblocks, n_old, n_new_of(nn, n_old), nd=nd,
                                   curr=r.integers(0, nd, size=(nblocks, n_old)), rw_now=now, rw_used=used))
    for nd in ND:
        for n_old in (7, 256, 300, 513, 8193):
            # the exact-tie contract: every stored chain of every block on the last integrand, W[j] = w (j + 1)
            for nn in ("same", "twice+1", "third"):
                r = rng()
                now, used = _mcmc_factors(r, nd)
                cases.append(_case("m-tie-nd%d-%d-%s" % (nd, n_old, nn), "ref", 3, n_old, n_new_of(nn, n_old), nd=nd,
                                   curr=np.full((3, n_old), nd - 1), rw_now=now, rw_used=used))
            # some integrands have fallen to rw_now = 0: their chains are never continued
            r = rng()
            now, used = _mcmc_factors(r, nd)
            now[r.permutation(nd)[:nd // 2]] = 0.0
            cases.append(_case("m-zeros-nd%d-%d" % (nd, n_old), "ref", 3, n_old, 2 * n_old + 1, nd=nd,
                               curr=r.integers(0, nd, size=(3, n_old)), rw_now=now, rw_used=used))
    # exact ties, pinned: u 2^53 is an integer m, so with one new chain and a total of 2^53 the target IS m, in float64 as in long
    # double, and a running weight of exactly m (every sum here is a sum of integers below 2^53) is NOT above it: the chain continues the
    # stored chain that carries the rest of the weight, past every chain of weight zero in between
    m, rest = U * 2.0 ** 53, 2.0 ** 53 - U * 2.0 ** 53
    assert m == int(m) and m + rest == 2.0 ** 53
    cases.append(_case("x-w-2", "ref", 3, 2, 1, w_chain=np.tile([m, rest], (3, 1))))
    for n_old, first, second in ((300, 10, 200), (8193, 100, 8000)):
        w = np.zeros((3, n_old))
        w[np.arange(3), first + np.arange(3)], w[np.arange(3), second + np.arange(3)] = m, rest
        cases.append(_case("x-w-%d" % n_old, "ref", 3, n_old, 1, w_chain=w))
        for nd in (5, 17):
            curr = np.full((3, n_old), 2)
            curr[np.arange(3), first + np.arange(3)], curr[np.arange(3), second + np.arange(3)] = 0, 1
            cases.append(_case("x-m-nd%d-%d" % (nd, n_old), "ref", 3, n_old, 1, nd=nd, curr=curr, rw_now=[m, rest] + [0.0] * (nd - 2)))
    # nothing to resample by: n_new > n_old, three blocks
    for n_old in (1, 7, 257, 8193):
        n_new = 2 * n_old + 1
        r = rng()
        cases.append(_case("f-wzero-%d" % n_old, "fallback", 3, n_old, n_new, w_chain=np.zeros((3, n_old))))
        w = r.random((3, n_old))
        w[np.arange(3), r.integers(0, n_old, size=3)] = np.nan
        cases.append(_case("f-wnan-%d" % n_old, "fallback", 3, n_old, n_new, w_chain=w))
        for nd in (5, 17):
            r = rng()
            now, used = _mcmc_factors(r, nd)
            now[:2] = 0.0                         # every integrand a stored chain sits on
            cases.append(_case("f-present-nd%d-%d" % (nd, n_old), "fallback", 3, n_old, n_new, nd=nd, curr=r.integers(0, 2, size=(3, n_old)),
                               rw_now=now, rw_used=used))
            now, used = _mcmc_factors(r, nd)
            now[1] = used[1] = 0.0                # 0 / 0, on an integrand some stored chain of every block sits on
            curr = r.integers(0, nd, size=(3, n_old))
            curr[:, 0] = 1
            cases.append(_case("f-0over0-nd%d-%d" % (nd, n_old), "fallback", 3, n_old, n_new, nd=nd, curr=curr, rw_now=now, rw_used=used))
    # a total of +inf
    for n_old in (7, 300, 8193):
        r = rng()
        w = r.random((3, n_old))
        w[:, n_old // 2] = np.inf
        cases.append(_case("i-w-%d" % n_old, "mirror", 3, n_old, 2 * n_old + 1, w_chain=w))
        for nd in (5, 17):
            r = rng()
            now, used = _mcmc_factors(r, nd)
            used[1] = 0.0                         # rw_used = 0 < rw_now
            curr = r.integers(0, nd, size=(3, n_old))
            curr[:, -1] = 1
            cases.append(_case("i-m-nd%d-%d" % (nd, n_old), "mirror", 3, n_old, 2 * n_old + 1, nd=nd, curr=curr, rw_now=now, rw_used=used))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


_CASES = None


def cases():
    """the table, built once (the arrays are shared: nobody writes to them)"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
        for c in _CASES:
            for k in ("w_chain", "curr", "rw_now", "rw_used"):
                if c[k] is not None:
                    c[k].setflags(write=False)
    return _CASES


def block_weights(case, b):
    """long-double weights of block b's stored chains"""
    with np.errstate(all="ignore"):
        if case["w_chain"] is not None:
            return case["w_chain"][b].astype(np.longdouble)
        w = case["rw_now"].astype(np.longdouble) / case["rw_used"].astype(np.longdouble)
        return w[case["curr"][b]]


_REF = {}


def reference(case):
    """(W_ref [nblocks, n_old], t_ref [nblocks, n_new], src_ref [nblocks, n_new], gamma [nblocks]) in long double, computed once per case"""
    if case["id"] not in _REF:
        nb, n_old, n_new = case["nblocks"], case["n_old"], case["n_new"]
        W = np.empty((nb, n_old), dtype=np.longdouble)
        t = np.empty((nb, n_new), dtype=np.longdouble)
        src = np.empty((nb, n_new), dtype=np.int64)
        gamma = np.empty(nb, dtype=np.longdouble)
        with np.errstate(all="ignore"):
            for b in range(nb):
                W[b] = np.cumsum(block_weights(case, b))
                if W[b, -1] > 0:
                    t[b] = (np.arange(n_new).astype(np.longdouble) + np.longdouble(U)) * (W[b, -1] / np.longdouble(n_new))
                    src[b] = np.minimum(np.searchsorted(W[b], t[b], side="right"), n_old - 1)
                else:
                    t[b] = np.nan
                    src[b] = np.arange(n_new) % n_old
                gamma[b] = np.longdouble(max(n_old, case["nd"] + 1)) * np.longdouble(2.0) ** -52 * W[b, -1]
        for a in (W, t, src, gamma):
            a.setflags(write=False)
        _REF[case["id"]] = (W, t, src, gamma)
    return _REF[case["id"]]


def fallback_picks(case):
    return np.tile(np.arange(case["n_new"]) % case["n_old"], (case["nblocks"], 1))


def check_picks(case, src, who):
    """src [nblocks, n_new] against the reference under the rules of the module's docstring; returns the picks the clause let through"""
    W, t, ref, gamma = reference(case)
    src = np.asarray(src)
    assert src.shape == ref.shape, (who, case["id"], src.shape)
    assert src.min() >= 0 and src.max() < case["n_old"], (who, case["id"], src.min(), src.max())
    excused = 0
    for b, c in zip(*np.nonzero(src != ref)):
        lo, hi = sorted((int(src[b, c]), int(ref[b, c])))
        off = np.abs(W[b, lo:hi] - t[b, c])
        assert np.all(off <= 2 * gamma[b]), "%s, case %s: block %d chain %d continues %d, the reference %d; |W_ref - t_ref| up to %g, 2 gamma %g" % (
            who, case["id"], b, c, src[b, c], ref[b, c], float(off.max()), float(2 * gamma[b]))
        excused += 1
    assert excused <= CAP * src.size, "%s, case %s: %d of %d picks differ from the reference within 2 gamma (at most %g of them may)" % (
        who, case["id"], excused, src.size, CAP)
    return excused


def check_running_weights(case, Wk, who):
    """the kernel's W [nblocks, n_old] against W_ref: within gamma, never decreasing"""
    W, _, _, gamma = reference(case)
    Wk = np.asarray(Wk)
    assert Wk.shape == W.shape, (who, case["id"], Wk.shape)
    err = np.abs(Wk.astype(np.longdouble) - W)
    assert np.all(err <= gamma[:, None]), "%s, case %s: W off by %g of the total, gamma is %g of it" % (
        who, case["id"], float((err / W[:, -1:]).max()), float((gamma / W[:, -1]).max()))
    assert np.all(np.diff(Wk, axis=1) >= 0), (who, case["id"])


def mirror(oracle, case):
    """the oracle's picks, block by block -> [nblocks, n_new]"""
    out = np.empty((case["nblocks"], case["n_new"]), dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(case["nblocks"]):
            if case["w_chain"] is not None:
                out[b] = oracle.resample_weighted(case["w_chain"][b], case["n_new"])
            else:
                out[b] = oracle.resample_chains(case["curr"][b], case["rw_now"], case["rw_used"], case["n_new"])
    return out
