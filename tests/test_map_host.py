"""CPU tests of the map draw's test harness (tests/map_cases.py): the CPU oracle (mcio_create through pool_create, mcio_vegas_block through
iteration) against the replay over the whole case table, sample by sample and iteration by iteration -- which proves that the derived
bounds can be met without the kernel --, five deliberate mistakes planted into the replay that the bounds must reject, each on a named
case -- which proves that they have teeth --, and the table's own conditions: every case leaves the replay's Jacobians and sums finite
and normal, every grid is strictly increasing with the leaf's end points, every Discrete draw lies below accumulation[end], and the
recorded sample indices with dy == 0 are what they are said to be."""
import numpy as np
import pytest

import map_cases as M

BITS = (52, 32)
NSAMPLE = 256
TINY = np.finfo(np.float64).tiny


def oracle_config(oracle, layout, tabs, bits=52):
    lay = M.LAYOUTS[layout]
    leaves = [dict(kind=0, pool=l, lower=lf[1], upper=lf[2], npts=lf[3] + 1) if lf[0] == "c" else dict(kind=1, pool=l, lower=lf[1], upper=lf[2])
              for l, lf in enumerate(lay["leaves"])]
    ocfg = oracle.Config(leaves, lay["dof"])
    for l, lf in enumerate(lay["leaves"]):
        if lf[0] == "c":
            ocfg.set_grid(l, tabs[l])
        else:
            d = np.ascontiguousarray(tabs[l], dtype=np.float64)
            assert oracle.lib().mcio_set_distribution(ocfg.p, l, d.ctypes.data_as(oracle.c_double_p)) == 0
    ocfg.set_rng_bits(bits)
    return ocfg


def oracle_samples(oracle, ocfg, indices, iteration=0, bits=52):
    """x[n][ndraw], jac[n] as the ORACLE draws the samples `indices` of the :vegas stream (tests/test_hip_vegas_check.py oracle_samples)"""
    oc = ocfg.c
    x, jac = np.zeros((len(indices), oc.ndraw)), np.zeros(len(indices))
    for s, gs in enumerate(indices):
        k, jaco = 0, 1.0
        for vi in range(oc.npool):
            for idx in range(1, oc.maxdof[vi] + 1):
                ocfg.pool_create(vi, idx, [oracle.uniform(M.SEED, iteration * 8, int(gs), k, bits=bits)])
                jaco /= np.ctypeslib.as_array(oc.pool_prob[vi], shape=(idx + 1,))[idx]
                x[s, k] = ocfg.pool_data(oc.pool_leaf0[vi])[idx - 1]
                k += 1
        jac[s] = jaco
    return x, jac


def stream(oracle, layout, indices, bits):
    nd = len(M.draws(layout))
    return np.array([[oracle.uniform(M.SEED, 0, int(i), k, bits=bits) for k in range(nd)] for i in indices])


FAMILIES = {}
for _c in M.sample_cases():
    FAMILIES.setdefault(M.family_of(_c[0]), []).append(_c)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_oracle_draws_what_the_replay_draws_sample_by_sample(oracle, family):
    worst = 0.0
    for cid, layout, grids, dists in FAMILIES[family]:
        tabs = M.tables(layout, grids, dists)
        for bits in BITS:
            idx = list(range(NSAMPLE)) + (list(M.DY0_INDICES) if layout == "sizes" and bits == 32 else [])
            rep = M.replay(layout, tabs, stream(oracle, layout, idx, bits))
            x, jac = oracle_samples(oracle, oracle_config(oracle, layout, tabs, bits), idx, bits=bits)
            worst = max(worst, M.check_samples(x, jac, rep, layout, "oracle, %s, %d bits" % (cid, bits)))
    print("%-18s oracle - replay: every x bit for bit, jac: largest difference / derived bound %.4f (bound %.3g, standing %.3g)"
          % (family, worst, min(float(M.jac_bound(c[1])) for c in FAMILIES[family]), M.STANDING["jac"]))
    assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(M.LAUNCHES))
def test_the_oracles_iteration_lies_within_the_derived_bounds(oracle, name):
    layout, grids, dists, npb = M.LAUNCHES[name]
    body = M.INTEGRANDS[M.LAYOUTS[layout]["f"]][0]
    fn = oracle.compile_c_integrand(body)
    for bits in BITS:
        tabs, reps, ref = M.launch_reference(oracle, name, bits)
        got = oracle_config(oracle, layout, tabs, bits).iteration(oracle.VEGAS, fn, None, npb, 0, M.NBLOCKS, 0, M.SEED)
        r_stat, r_hist = M.check_packed(got, ref, layout, "oracle, %s, %d bits" % (name, bits))
        tj, ts, th = M.tightest(layout, npb, M.NBLOCKS, max(int(c.max()) for c in ref["count"]))
        print("%-18s %d bits, oracle - replay over the derived bound: sums %.4f, histogram %.4f   (bounds asserted: jac %.3g sums %.3g histogram %.3g; "
              "standing 1e-13 / 1e-11 / 1e-9)" % (name, bits, r_stat, r_hist, tj, ts, th))
        assert r_stat <= 1.0 and r_hist <= 1.0
        assert float(ref["b_sum"]) < M.STANDING["sums"] and all(float(b.max()) < M.STANDING["hist"] for b in ref["b_hist"])     # the derived bounds ARE the tighter


# ---- planted mistakes ------------------------------------------------------------------------------------------------------------------
def rejected_per_sample(layout, tabs, y, mutation):
    """the mutated replay's samples against the replay's: does an x differ, or a jac leave its bound?"""
    good, bad = M.replay(layout, tabs, y), M.replay(layout, tabs, y, mutate=mutation)
    assert M.check_samples(good["x"], good["jac"].astype(np.float64), good, layout, "replay") <= 1.0
    try:
        return M.check_samples(bad["x"], bad["jac"].astype(np.float64), good, layout, mutation) > 1.0
    except AssertionError:
        return True


def rejected_per_launch(layout, tabs, ys, mutation):
    """... the mutated replay's packed row against the replay's"""
    good = [M.replay(layout, tabs, y) for y in ys]
    ref = M.packed_row(layout, good)
    assert max(M.check_packed(M.flat(M.packed_row(layout, good, dtype=np.float64), layout), ref, layout, "replay")) <= 1.0
    bad = M.flat(M.packed_row(layout, [M.replay(layout, tabs, y, mutate=mutation) for y in ys], dtype=np.float64), layout)
    try:
        return max(M.check_packed(bad, ref, layout, mutation)) > 1.0
    except AssertionError:
        return True


def test_x_formed_with_one_rounding_is_rejected(oracle):
    """named cases: sizes-uniform (the 3-increment leaf: one x in twelve), sizes-spike_middle and pair16.  One rounding and two differ
    only where the product's own rounding error decides the sum's rounding, about dx / |g[iy]| of the draws: rarely on a fine grid, never
    where an increment is one ulp wide (dy ulp is exact) -- a contracted x = fma(dy, dx, g) would pass most samples and still fail these"""
    for layout, grids in (("sizes", "uniform"), ("sizes", "spike_middle"), ("pair16", "uniform")):
        tabs = M.tables(layout, grids)
        y = stream(oracle, layout, range(NSAMPLE), 52)
        print("%s %s: x differs at %d of %d draws" % (layout, grids, int(np.sum(M.replay(layout, tabs, y)["x"] != M.replay(layout, tabs, y, mutate="x_one_rounding")["x"])), y.size))
        assert rejected_per_sample(layout, tabs, y, "x_one_rounding"), layout


def rounds_up_to_an_integer(n):
    """uniforms y < j / n whose product y n rounds UP to the integer j: the exact product lies in increment j - 1, the rounded one in j"""
    out = []
    for j in range(1, n):
        y = np.nextafter(j / n, 0.0)
        while y * n >= j and y > 0:                       # walk down to the largest y whose exact product is below j
            from fractions import Fraction
            if Fraction(float(y)) * n < j:
                out.append(float(y))
                break
            y = np.nextafter(y, 0.0)
    return np.array(out)


def test_the_bin_taken_from_the_exact_product_is_rejected():
    """named case: pair2 (999 increments) on the spike_middle grid, fed uniforms just below j / 999 whose rounded product is the integer j
    (no generator gives them in a test's lifetime: about one draw in 2^43)"""
    ys = rounds_up_to_an_integer(999)
    assert ys.size >= 8
    ys = ys[:ys.size // 2 * 2].reshape(-1, 2)
    tabs = M.tables("pair2", "spike_middle")
    good, bad = M.replay("pair2", tabs, ys), M.replay("pair2", tabs, ys, mutate="bin_from_exact_product")
    assert np.all(bad["bin"] == good["bin"] - 1) and np.all(good["x"] == tabs[0][good["bin"]])      # dy == 0: x is the left edge
    assert rejected_per_launch("pair2", tabs, [ys, ys], "bin_from_exact_product")


def test_the_scale_applied_after_eight_bare_increments_is_rejected(oracle):
    """named cases: small (the bare product underflows to 0) and lossy (it passes through the denormals and loses bits)"""
    for layout in ("small", "lossy"):
        tabs = M.tables(layout)
        y = stream(oracle, layout, range(64), 52)
        bad = M.replay(layout, tabs, y, mutate="scale_after_eight")
        if layout == "small":
            assert np.all(bad["jac"] == 0)
        else:
            err = np.abs(bad["jac"] - M.replay(layout, tabs, y)["jac"]) / M.replay(layout, tabs, y)["jac"]
            print("lossy: planted mistake, relative error of jac %.3g .. %.3g" % (float(err.min()), float(err.max())))
            assert float(err.max()) > 16 * float(M.jac_bound(layout))         # (ten bits lost below 2^-1022: up to 2^-43, next to the standing 1e-13)
        assert rejected_per_sample(layout, tabs, y, "scale_after_eight"), layout
    tabs = M.tables("pair8")                                   # ... and on a tame range it is no mistake at all
    assert not rejected_per_sample("pair8", tabs, stream(oracle, "pair8", range(64), 52), "scale_after_eight")


def test_le_in_the_discrete_bisection_is_rejected():
    """named cases: mixed-zeros_first and mixed-zeros_middle, fed uniforms that ARE entries of the accumulation (0.0 among them: with
    `<=` a draw of y = 0 lands in the first bin, of probability zero, and 1 / prob is infinite)"""
    for name in ("mixed-zeros_first", "mixed-zeros_middle"):
        layout, grids, dists, npb = M.LAUNCHES[name]
        tabs = M.tables(layout, grids, dists)
        dist, acc = M.normalised(tabs[2])
        ties = np.unique(acc[:-1])
        y = np.stack([np.full(ties.size, 0.25), np.full(ties.size, 0.75), ties], axis=1)
        good = M.replay(layout, tabs, y)
        assert np.all(dist[good["bin"][:, 2]] > 0)            # the reference never lands in a bin of probability zero
        assert rejected_per_sample(layout, tabs, y, "bisection_le"), name


def test_a_packed_bin_truncated_to_ten_bits_is_rejected(oracle):
    """named case: tiles (1025 and 2500 increments: bins beyond 1023)"""
    layout, grids, dists, npb = M.LAUNCHES["tiles"]
    tabs = M.tables(layout, grids, dists)
    ys = M.uniforms(oracle, layout, 512, 0, 2)
    assert rejected_per_launch(layout, tabs, list(ys), "bin_ten_bits")
    assert not rejected_per_launch("pair2", M.tables("pair2"), list(M.uniforms(oracle, "pair2", 512, 0, 2)), "bin_ten_bits")   # 999 bins fit


# ---- the table's own conditions ----------------------------------------------------------------------------------------------------------
def test_every_case_leaves_the_replays_jacobians_and_sums_finite_and_normal(oracle):
    for cid, layout, grids, dists in M.sample_cases():
        tabs = M.tables(layout, grids, dists)
        for bits in BITS:
            rep = M.replay(layout, tabs, stream(oracle, layout, range(NSAMPLE), bits))
            j = rep["jac"].astype(np.float64)
            assert rep["located"] and np.all(np.isfinite(j)) and np.all(j >= TINY), (cid, bits)
            run = np.cumprod(rep["inv"], axis=1).astype(np.float64)                 # ... and so is every partial product, draw by draw
            assert np.all(np.isfinite(run)) and np.all(run >= TINY), (cid, bits)
    for name in M.LAUNCHES:
        for bits in BITS:
            tabs, reps, ref = M.launch_reference(oracle, name, bits)
            cols = np.concatenate([ref["sums"], ref["squares"], [ref["norm"]]] + ref["hist"]).astype(np.float64)
            assert all(r["located"] for r in reps) and np.all(np.isfinite(cols)) and np.all(cols >= TINY), (name, bits)
            for r in reps:
                assert np.all(r["jac"].astype(np.float64) >= TINY) and np.all(np.isfinite(r["jaci"].astype(np.float64))), (name, bits)
    # the small ranges are where they are for this reason: the true Jacobians are ordinary doubles, the bare products of eight increments are not
    assert float(M.replay("small", M.tables("small"), np.full((1, 8), 0.5))["jac"][0]) == pytest.approx(2.0 ** -1000, rel=1e-12)
    assert (2.0 ** -125 / 999) ** 8 == 0.0 and 0.0 < (2.0 ** -119 / 999) ** 8 < TINY


def test_the_table_covers_what_it_is_for():
    for fam in ("uniform", "geometric", "spike_first"):
        for n in M.SIZES:
            g = M.grid(fam, n)
            assert g[0] == 0.0 and g[-1] == 1.0 and g.size == n + 1
    assert {n for k, lo, hi, n in M.LAYOUTS["sizes"]["leaves"]} == set(M.SIZES)
    g = M.grid("geometric", 999)
    w = np.diff(g)
    assert 2.0 ** 39 < w[0] / w[-1] < 2.0 ** 41
    for fam in ("spike_first", "spike_middle", "spike_last"):
        w = np.diff(M.grid(fam, 999))
        assert abs(w.max() - (1 - 2.0 ** -30)) < 1e-12 and np.sum(w > 0.5) == 1
    for n in (63, 64, 65, 999, 1024, 2500):
        g = M.grid("ulp_run", n)
        a, b = M.ulp_run_edges(n)
        assert all(g[j + 1] == np.nextafter(g[j], np.inf) for j in range(a, b)) and b - a == 32
    g = M.grid("offset", 2500, *M.RANGES["offset"])
    assert g[0] == 2.0 ** 40 and g[-1] == 2.0 ** 40 + 1 and np.all(g * 4096 == np.round(g * 4096))       # 12 fraction bits
    for n in (64, 999, 1024):
        g = M.grid("straddle", n, *M.RANGES["straddle"])
        assert (g[0], g[-1]) == (-3.0, 5.0) and np.sum(g == 0.0) == 1
    assert M.grid("small_range", 999, *M.RANGES["small_range"])[-1] == 2.0 ** -125
    assert M.grid("small_range_lossy", 999, *M.RANGES["small_range_lossy"])[-1] == 2.0 ** -119
    for fam in M.TABLE_FAMILIES:
        for k in M.DISCRETE_K:
            dist, acc = M.normalised(M.table(fam, k))
            assert dist.size == k and abs(acc[-1] - 1.0) < 1e-12 and np.all(np.diff(acc) >= 0)
            if fam.startswith("zeros") and k > 1:
                assert np.any(dist == 0.0) and np.any(np.diff(acc) == 0.0)                                  # ties in the accumulation
    assert M.normalised(M.table("dominant", 17))[0].max() == pytest.approx(1 - 2.0 ** -40, rel=1e-15)
    assert M.normalised(M.table("tiny", 1025))[0].min() == pytest.approx(2.0 ** -60, rel=1e-2)
    assert M.normalised(M.table("zeros_last", 17))[0][-1] == 0.0
    covered = {M.family_of(c[0]) for c in M.sample_cases()} | set(M.RANGES)
    assert covered >= set(M.GRID_FAMILIES) | set(M.TABLE_FAMILIES)
    assert len(M.LAYOUTS) <= 12


def test_the_recorded_indices_have_dy_zero(oracle):
    """32-bit stream: draw 7 of layout `sizes` (1024 increments) at the recorded sample indices has y N an exact integer"""
    assert M.LAYOUTS["sizes"]["leaves"][M.DY0_DRAW][3] == 1024 and len(M.DY0_INDICES) >= 3
    for i in M.DY0_INDICES:
        y = oracle.uniform(M.SEED, 0, i, M.DY0_DRAW, bits=32)
        assert y * 1024.0 == np.floor(y * 1024.0) and 0 < y < 1, (i, y)
    rep = M.replay("sizes", M.tables("sizes", "geometric"), stream(oracle, "sizes", M.DY0_INDICES, 32))
    g = M.tables("sizes", "geometric")[M.DY0_DRAW]
    assert np.all(rep["x"][:, M.DY0_DRAW] == g[rep["bin"][:, M.DY0_DRAW]])                                  # x is the left edge itself
