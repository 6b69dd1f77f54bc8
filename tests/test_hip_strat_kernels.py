"""GPU tests of the three static kernels of stratified :vegas on their own (csrc/mci_static_kernels.h k_strat_alloc, k_strat_reduce,
k_strat_remap), through the test hooks Engine.strat_alloc_rows, strat_reduce_rows and strat_remap_rows (csrc/mci_debug.h), which launch
them by the helpers the product launches them with, over the made-up inputs of tests/strat_cases.py: every case against the bounds of the
long-double reference (derived there; tests/test_strat_kernels_host.py holds the mirror to them on the CPU), against the float64 mirror
bit for bit -- offsets, tsum, out, log_row and the e == 1 remap; everything but pow --, and the exact families EQUAL to the reference.
The allocation rule's other caller, the stratified sweep's one workgroup (csrc/mci_sweep_strat.h), is held to the same mirror through
the public route: Engine.integrate_sweep_strat(adapt=False, niter=1, d=made_up) must report the mirror's counts bit for bit.

Run with -s for the figures: per family the largest difference over the derived bound (asserted <= 1), and the largest |kernel -
reference| of pow in ulps."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import strat_cases as S

pytestmark = pytest.mark.gpu

WORST = {}      # family -> largest difference / bound seen (printed by the module's last test)
POW_ULPS = {}


@pytest.fixture(scope="module")
def eng():
    """one engine, NOT stratified, for its device and its stream only"""
    e = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]]), mci.catalog.x2y2())
    yield e
    e.close()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %d of %d entries differ, first at %s" % (
        what, np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)), a.size, np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))[:8])


def note(table, key, value):
    table[key] = max(table.get(key, 0.0), value)


# ---- k_strat_alloc --------------------------------------------------------------------------------------------------------------------------

ALLOC_GROUPS = {}
for _c in S.ALLOC_CASES:
    ALLOC_GROUPS.setdefault("%s-%d" % (_c["family"], _c["ncube"]), []).append(_c)


@pytest.mark.parametrize("group", list(ALLOC_GROUPS))
def test_alloc_against_reference_and_mirror(eng, group):
    for c in ALLOC_GROUPS[group]:
        d, ask = S.alloc_input(c)
        N, nc = c["nsamp"], c["ncube"]
        off, tsum = eng.strat_alloc_rows(d, N, uniform=ask)
        assert off.min() >= 0 and not np.any(tsum.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)), c["id"] + ": the hook's fill came back"
        ref = S.alloc_reference(d, N, ask)
        bad, ratio = S.alloc_check(off, ref, N)
        print("%s: %d of %d hypercubes have a window of two integers, largest distance / bound %.3g" % (c["id"], np.count_nonzero(ref["lo"] != ref["hi"]), nc, ratio))
        assert not bad, (c["id"], bad)
        assert ratio <= 1.0, c["id"]
        note(WORST, "alloc " + c["family"], ratio)
        assert bool(tsum[-1]) == ref["uniform"] == (c["family"] in S.UNIFORM_FAMILIES), c["id"]
        if S.alloc_is_exact(c, d):
            assert np.array_equal(off[1:], 2 * np.arange(1, nc + 1) + ref["fl"]), c["id"] + ": an exact family differs from floor(C_ref)"
        m_off, m_tsum = S.kernel_order_alloc(d, N, ask, full=True)
        same_bits(off, m_off, c["id"] + ": offsets")
        same_bits(tsum, m_tsum, c["id"] + ": tsum")


def test_the_uniform_families_agree(eng):
    """all zeros, one inf, one NaN and uniform = 1 give the same offsets, those of d_h = 1"""
    for nc, N in ((257, 2059), (65537, 8 * 65537 + 3), (262145, 2 ** 40 + 7)):
        want, tsum = eng.strat_alloc_rows(np.ones(nc), N, uniform=True)
        same_bits(want, S.kernel_order_alloc(np.ones(nc), N, True), "uniform %d %d" % (nc, N))
        assert want[nc] == N and np.diff(want).min() >= 2 and np.diff(want).max() - np.diff(want).min() <= 1
        for fam in S.UNIFORM_FAMILIES:
            d, ask = S.alloc_input(dict(ncube=nc, family=fam, seed=nc))
            off, tsum = eng.strat_alloc_rows(d, N, uniform=ask)
            assert tsum[-1] == 1.0
            same_bits(off, want, "%s %d %d" % (fam, nc, N))


# ---- k_strat_reduce -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nchunk", S.REDUCE_NCHUNK)
@pytest.mark.parametrize("values", S.REDUCE_VALUES)
def test_reduce_against_reference_and_mirror(eng, values, nchunk):
    for c in S.REDUCE_CASES:
        if c["values"] != values or c["nchunk"] != nchunk:
            continue
        x = S.reduce_input(c)
        args = (x["off"], x["part"], x["rec_h"], x["rec_s"], x["dnext"], x["beta"])
        got, bare = eng.strat_reduce_rows(*args), eng.strat_reduce_rows(*args, log_row=False)
        assert bare["log_row"] is None
        same_bits(got["log_row"], got["out"], c["id"] + ": log_row against out")
        same_bits(bare["out"], got["out"], c["id"] + ": out without a log row")
        same_bits(bare["dnext"], got["dnext"], c["id"] + ": dnext without a log row")
        ref = S.reduce_reference(x)
        bad, ratio = S.reduce_check(got, x, ref, values == "exact")
        print("%s: %d cut hypercubes, largest |kernel - reference| / bound %.3g" % (c["id"], ref["ncut"], ratio))
        assert not bad, (c["id"], bad)
        assert ratio <= 1.0 and (values != "exact" or ratio == 0.0), c["id"]
        note(WORST, "reduce " + values, ratio)
        mir = S.kernel_order_reduce(x)
        same_bits(got["out"], mir["out"], c["id"] + ": out against the mirror")
        cut = sorted(ref["cut"])
        if cut:         # pow: the kernel's against numpy's, in ulps (a figure, not a check: the check is the reference's interval above)
            k, m = got["dnext"][cut], mir["dnext"][cut]
            fin = np.isfinite(m) & (m > 0)
            note(POW_ULPS, "reduce d_h", float(np.max(np.abs(k[fin] - m[fin]) / np.spacing(m[fin]), initial=0.0)))


# ---- k_strat_remap --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", S.REMAP_CASES, ids=lambda c: c["id"])
def test_remap_against_reference_and_mirror(eng, c):
    d = S.remap_input(c)
    got = eng.strat_remap_rows(c["n_old"], c["n_new"], c["e"], d)
    assert not np.any(got.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)), "the hook's fill came back: a new hypercube was not written"
    ref, bound = S.remap_reference(d, c["n_old"], c["n_new"], c["e"])
    bad, ratio, ulps = S.remap_check(got, ref, bound)
    print("%s: largest |kernel - reference| / bound %.3g, %.3g ulps" % (c["id"], ratio, ulps))
    assert not bad, (c["id"], bad)
    assert ratio <= 1.0
    note(WORST, "remap e=%.3g" % c["e"], ratio)
    if c["e"] == 1.0:
        same_bits(got, S.kernel_order_remap(d, c["n_old"], c["n_new"], c["e"]), c["id"] + ": e == 1 copies bits")
        same_bits(got, ref.astype(np.float64), c["id"] + ": e == 1 against the reference")
    else:
        note(POW_ULPS, "remap", ulps)


# ---- the sweep's twin: the same rule walked by one workgroup, through the public route ---------------------------------------------------------

SWEEP_LAYOUTS = {3: dict(dof=[[2], [3]], f="w[0] = x[0] + ud[0] * x[1]; w[1] = x[0] * x[1] * x[2];"), 2: dict(dof=[[2]], f="w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];")}


@pytest.fixture(scope="module")
def sweep_engines():
    engs = {D: mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=L["dof"]), mci.Integrand(L["f"], [1.0])) for D, L in SWEEP_LAYOUTS.items()}
    yield engs
    for e in engs.values():
        e.close()


@pytest.mark.parametrize("family", S.SWEEP_FAMILIES)
@pytest.mark.parametrize("plan", S.SWEEP_PLANS, ids=lambda p: "x".join(map(str, p[0])) + "-%d" % p[1])
def test_the_sweeps_allocation_is_the_mirrors_bit_for_bit(sweep_engines, plan, family):
    nstrat, N = plan
    e = sweep_engines[len(nstrat)]
    e.set_stratification(nstrat=list(nstrat))
    rows = S.sweep_rows(nstrat, family, S.SEED + 7)
    rs = e.integrate_sweep_strat("vegas", userdata=[[1.0], [0.5], [0.25]], neval=N, niter=1, block=16, adapt=False, d=rows, seed=S.SEED)
    assert len(rs) == 3
    for k, r in enumerate(rs):
        assert r["status"] == 0 and r["neval"] == N
        want = np.diff(S.kernel_order_alloc(rows[k], N))
        assert want.sum() == N and want.min() >= 2
        same_bits(np.ascontiguousarray(r["strat_counts"], dtype=np.int64), want, "%s %s point %d" % (plan, family, k))
        ref = S.alloc_reference(rows[k], N, False)
        assert ref["uniform"] == (family == "all_zero")
        bad, ratio = S.alloc_check(np.concatenate([[0], np.cumsum(r["strat_counts"])]), ref, N)
        assert not bad and ratio <= 1.0, (plan, family, k, bad)
        note(WORST, "sweep " + family, ratio)
    if family not in ("all_zero",):
        assert not np.array_equal(rs[0]["strat_counts"], rs[1]["strat_counts"])      # (the points' rows differ, and so do their allocations)


# ---- the hooks leave the problem alone ---------------------------------------------------------------------------------------------------------

def test_the_hooks_take_the_device_and_the_stream_only():
    """the three hooks called between two iterations of a stratified run: its counts and its d_h come out as they do without the calls"""
    N, block = 8192, 16

    def two_iterations(calls):
        # (deterministic: the histogram adds, and with them the map the second iteration samples on, are bit-identical run to run)
        e = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]]), mci.catalog.x2y2(), deterministic=True)
        e.set_stratification(nstrat=[16, 16])
        e.run("vegas", N // block, 0, block, 0, S.SEED)
        e.finish("vegas", block, adapt=True)
        first = (e.strat_counts(), e.strat_d())
        if calls:
            rng = np.random.default_rng(3)
            e.strat_alloc_rows(rng.random(256), N)                       # the run's own plan and N, other d_h
            e.strat_alloc_rows(rng.random(1000), 5000, uniform=True)
            x = S.reduce_input(next(c for c in S.REDUCE_CASES if c["nchunk"] == 1025 and c["nw"] == 1 and c["values"] == "smooth"))
            e.strat_reduce_rows(x["off"], x["part"], x["rec_h"], x["rec_s"], x["dnext"], x["beta"])
            e.strat_remap_rows([16, 16], [20, 13], 0.5, rng.random(256))
            with pytest.raises(mci.MCIError, match="hypercubes"):
                e.strat_alloc_rows(np.ones(4), 7)
        e.run("vegas", N // block, 0, block, 1, S.SEED)
        e.finish("vegas", block, adapt=True)
        out = first + (e.strat_counts(), e.strat_d(), e.grid(0))
        e.close()
        return out
    plain, hooked = two_iterations(False), two_iterations(True)
    for a, b, what in zip(plain, hooked, ("counts 0", "d_h 0", "counts 1", "d_h 1", "grid")):
        same_bits(a, b, what)
    assert np.abs(plain[2] - plain[0]).max() > 1        # (the second allocation did follow the first iteration's d_h)


def test_print_the_figures():
    """per family the largest difference over the derived bound seen by the tests above (each asserted <= 1 where it was seen), and pow's
    largest |kernel - reference| in ulps; run the module with -s"""
    for k in sorted(WORST):
        print("largest difference / bound  %-22s %.3g" % (k, WORST[k]))
    for k in sorted(POW_ULPS):
        print("pow, largest difference in ulps  %-12s %.3g" % (k, POW_ULPS[k]))
    assert all(v <= 1.0 for v in WORST.values())
