"""GPU tests of the :vegas map draw on its own (csrc/mci_device.h draw_leaf, draw_sample with its batched pair-table reads, draw_sample_pipe,
the gather and edge-cache phases, pack_bin / tdraw_extract and the tiled replay, the Discrete bisection) over the made-up maps of
tests/map_cases.py, handed in through Engine.set_grid / set_distribution.  Every other test that reaches this code feeds it the uniform
start or a map train! produced: smooth, on [0, 1] or [-sqrt 50, sqrt 50], 999 increments or so.

Yardsticks: the float64 replay of the reference's draw (x bit for bit) and its long-double Jacobians, sums and histograms with bounds
derived per entry (map_cases; tests/test_map_host.py holds the CPU oracle to them and shows that they reject planted mistakes), and what
is known outright.  Per sample through sample_dump on both streams; per launch through iteration("vegas"), plan by plan, each plan forced
with the suite's own switches and checked to have run.  One engine per (layout, stream, plan), outputs shared between the tests."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import map_cases as M
from test_map_host import FAMILIES, stream

pytestmark = pytest.mark.gpu
NSAMPLE = 1024
_OUT = {}


def engine(layout, bits=52, **kw):
    lay = M.LAYOUTS[layout]
    var = tuple(mci.Continuous(lf[1], lf[2], ninc=lf[3] + 1) if lf[0] == "c" else mci.Discrete(lf[1], lf[2]) for lf in lay["leaves"])
    return mci.Engine(mci.Configuration(var=var, dof=lay["dof"], seed=M.SEED), mci.Integrand(M.INTEGRANDS[lay["f"]][0]), rng_bits=bits, **kw)


def set_tables(eng, layout, tabs):
    for l, lf in enumerate(M.LAYOUTS[layout]["leaves"]):
        if lf[0] == "c":
            eng.set_grid(l, tabs[l])
        else:
            eng.set_distribution(l, tabs[l])


class Engines:
    """one engine per (layout, stream bits) for the dumps, created when first asked for"""

    def __init__(self):
        self.engs = {}

    def get(self, layout, bits):
        if (layout, bits) not in self.engs:
            self.engs[layout, bits] = engine(layout, bits)
        return self.engs[layout, bits]

    def close(self):
        for eng in self.engs.values():
            eng.close()


@pytest.fixture(scope="module")
def engines():
    e = Engines()
    yield e
    e.close()


def dump(engines, oracle, cid, layout, grids, dists, bits):
    """(x, jac, the replay) of samples 0 .. NSAMPLE - 1 of the case, and of the recorded dy == 0 samples on the 32-bit stream"""
    key = (cid, bits)
    if key not in _OUT:
        eng = engines.get(layout, bits)
        tabs = M.tables(layout, grids, dists)
        set_tables(eng, layout, tabs)
        x, jac, w = eng.sample_dump(NSAMPLE, iteration=0, seed=M.SEED)
        idx = list(range(NSAMPLE))
        if layout == "sizes" and bits == 32:
            for i in M.DY0_INDICES:                                      # exactly that sample: a block of one sample, block index i
                xi, ji, wi = eng.sample_dump(1, nevalperblock=1, block_index=i, iteration=0, seed=M.SEED)
                x, jac, idx = np.concatenate([x, xi]), np.concatenate([jac, ji]), idx + [i]
        _OUT[key] = x, jac, M.replay(layout, tabs, stream(oracle, layout, idx, bits)), tabs
    return _OUT[key]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_sample_is_the_replays(engines, oracle, family):
    """every x bit for bit, every jac within JAC_OPS ndraw u, on both streams, the dy == 0 samples included"""
    worst = 0.0
    for cid, layout, grids, dists in FAMILIES[family]:
        for bits in (52, 32):
            x, jac, rep, tabs = dump(engines, oracle, cid, layout, grids, dists, bits)
            worst = max(worst, M.check_samples(x, jac, rep, layout, "kernel, %s, %d bits" % (cid, bits)))
    print("%-18s sample_dump - replay: every x bit for bit, jac: largest difference / derived bound %.4f (bound %.3g, standing %.3g)"
          % (family, worst, min(float(M.jac_bound(c[1])) for c in FAMILIES[family]), M.STANDING["jac"]))
    assert worst <= 1.0


# ---- per launch ----------------------------------------------------------------------------------------------------------------------
# plan -> (case of map_cases.LAUNCHES, stream bits, overrides, Engine keywords, (threads, wg_per_block) | None, what must have run)
RAGGED = 2 * 668          # split_chunk: 668 samples of each of the two blocks at a time -> 2003 = 668 + 668 + 667


def pair(eng, r):
    """the pair table in LDS (table modes 0 / 1; it takes 16 bytes per increment), one tile, no cursor"""
    return eng.table_mode <= 1 and eng.lds_bytes >= 16 * 999 and r["chunks"] == 0 and not r["cursor"]


PLANS = {
    "pair-2-draws": ("pair2", 52, {}, {}, None, pair),
    "pair-8-draws": ("pair8", 52, {}, {}, None, pair),                                   # batched reads, the FMA bin form
    "pair-8-draws-32-bits": ("pair8-spike", 32, {}, {}, None, pair),
    "pair-16-draws": ("pair16", 52, {"vegas_cursor": 0}, {}, None, lambda eng, r: pair(eng, r) and r["copies"] >= 8),
    "pair-16-draws-32-bits-deterministic": ("pair16-ulp_run", 32, {}, dict(deterministic=True), None, pair),
    "cursor-16-draws": ("pair16", 52, {"vegas_cursor": 1, "vegas_big_unit": 0}, {}, (0, 1),
                        lambda eng, r: (r["copies"], r["threads"], r["wgs"], r["cursor"]) == (8, 512, M.NBLOCKS, True)),
    "big-unit-16-draws": ("pair16-ulp_run", 52, {"vegas_cursor": 1, "vegas_big_unit": 1}, {}, (0, 1),
                          lambda eng, r: (r["copies"], r["threads"], r["wgs"], r["cursor"]) == (16, 1024, M.NBLOCKS, True)),
    "table-mode-1": ("mixed-zeros_first", 52, {"table_mode": 1}, {}, None, lambda eng, r: eng.table_mode == 1),
    "table-mode-2": ("mixed-zeros_middle", 52, {"table_mode": 2}, {}, None, lambda eng, r: eng.table_mode == 2),
    "table-mode-3": ("mixed-zeros_last", 32, {"table_mode": 3}, {}, None, lambda eng, r: eng.table_mode == 3),
    "table-mode-3-no-l1-phase": ("tiles", 52, {"table_mode": 3, "l1_phase": 0}, {}, None, lambda eng, r: eng.table_mode == 3),
    # leaves of 999, 1025 and 2500 increments in tiles of 2500 bins: {999, 1025} | {2500}; every tile replayed: three fields of 12 bits, the third across two words
    "tiles-split-all": ("tiles", 52, {"table_mode": 3, "hist_tile_bins": 2500, "split_chunk": RAGGED}, {}, None,
                        lambda eng, r: eng.table_mode == 3 and r["tiles"] and r["chunks"] == 3),
    "tiles-keep-tile-0": ("tiles", 32, {"table_mode": 3, "hist_tile_bins": 2500, "split_chunk": RAGGED, "no_split_all": 1}, {}, None,
                          lambda eng, r: eng.table_mode == 3 and r["tiles"] and r["chunks"] == 3),
    # 999 | 1025 | 1025 increments in tiles of 1100 bins, one leaf each: three fields of 11 bits, the third across two words
    "tiles-11-bits": ("tiles11", 52, {"table_mode": 3, "hist_tile_bins": 1100, "split_chunk": RAGGED}, {}, None,
                      lambda eng, r: eng.table_mode == 3 and r["tiles"] and r["chunks"] == 3),
    "small-range-pair": ("small", 52, {}, {}, None, pair),
    "small-range-lossy-pair-32-bits": ("lossy", 32, {}, {}, None, pair),
    # (the big unit itself is out of reach of 8 draws: vegas_big_rule takes a launch only where the standing unit runs the eight-copy
    # plan, which 16 draws get and 8 do not -- asserted here: one copy --, and 16 such draws take the Jacobian itself out of the doubles;
    # forced the same way, the launch goes through the same pipelined loop by cursor)
    "small-range-cursor": ("small", 52, {"vegas_cursor": 1, "vegas_big_unit": 1}, {}, (0, 1),
                           lambda eng, r: r["cursor"] and r["wgs"] == M.NBLOCKS and r["copies"] == 1),
}


def plan_engine(plan, overrides, **kw):
    """the engine of a plan under its overrides (the layout decisions are taken when the engine is made, the launch's when it runs)"""
    name, bits, over, ekw, launch, expect = PLANS[plan]
    for k, v in over.items():
        overrides.set(k, v)
    eng = engine(M.LAUNCHES[name][0], bits, **dict(ekw, **kw))
    if launch:
        eng.set_launch(*launch)
    return eng


def run_plan(oracle, overrides, plan):
    if plan not in _OUT:
        from mcintegration_jl_amd import isa_mix
        name, bits, over, ekw, launch, expect = PLANS[plan]
        layout, grids, dists, npb = M.LAUNCHES[name]
        tabs, reps, ref = M.launch_reference(oracle, name, bits)
        eng = plan_engine(plan, overrides)
        set_tables(eng, layout, tabs)
        packed = eng.iteration("vegas", npb, 0, M.NBLOCKS, iteration=0, seed=M.SEED)
        eng.check_status()
        wgs, threads = eng.kernel_times_ms(1)[1:]
        kernels = sorted(isa_mix.resources(eng.code_object("vegas")))
        r = dict(wgs=wgs, threads=threads, cursor=eng.last_launch_cursor()[0], copies=eng.histogram_copies(), chunks=eng.split_chunks()[0],
                 table_mode=eng.table_mode, tiles="mci_vegas_tiles" in kernels, check=eng.vegas_check_status())
        ok = bool(expect(eng, r))
        again = eng.iteration("vegas", npb, 0, M.NBLOCKS, iteration=0, seed=M.SEED)      # the same launch once more: nothing carried over
        eng.close()
        overrides.clear()
        _OUT[plan] = packed, again, r, ok, ref, layout, npb
    return _OUT[plan]


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_every_plan_leaves_the_replays_row(oracle, overrides, plan):
    """the packed row of one iteration (block sums, squares, NORM, NEVAL) and every histogram bin against the long-double replay, within
    the derived bounds; a bin no sample landed in holds what it held before; the intended plan ran"""
    packed, again, r, ok, ref, layout, npb = run_plan(oracle, overrides, plan)
    r_stat, r_hist = M.check_packed(packed, ref, layout, "kernel, %s" % plan)
    tj, ts, th = M.tightest(layout, npb, M.NBLOCKS, max(int(c.max()) for c in ref["count"]))
    print("%-36s %-18s ran %r\n%36s kernel - replay over the derived bound: sums %.4f, histogram %.4f   (bounds asserted: sums %.3g histogram %.3g; standing 1e-11 / 1e-9)"
          % (plan, PLANS[plan][0], r, "", r_stat, r_hist, ts, th))
    assert ok, (plan, r)
    assert r_stat <= 1.0 and r_hist <= 1.0
    assert max(M.check_packed(again, ref, layout, "kernel, %s, second launch" % plan)) <= 1.0


# ---- known outright ------------------------------------------------------------------------------------------------------------------
def test_on_a_run_of_increments_one_ulp_wide_every_x_is_an_edge(engines, oracle):
    seen = 0
    for bits in (52, 32):
        x, jac, rep, tabs = dump(engines, oracle, "sizes-ulp_run", "sizes", "ulp_run", "uniform", bits)
        for k, (l, slot) in enumerate(M.draws("sizes")):
            n = M.LAYOUTS["sizes"]["leaves"][l][3]
            if n < 2 * M.ULP_RUN - 1:
                continue
            a, b = M.ulp_run_edges(n)
            g = tabs[l]
            inside = (rep["bin"][:, k] >= a) & (rep["bin"][:, k] < b)
            xs, bs = x[inside, k], rep["bin"][inside, k]
            assert np.all((xs == g[bs]) | (xs == g[bs + 1])), (bits, n)
            seen += int(inside.sum())
    print("ulp_run: %d draws landed in a run" % seen)
    assert seen >= 100


def test_bins_of_probability_zero_receive_nothing(engines, oracle, overrides):
    for fam in ("zeros_first", "zeros_middle", "zeros_last"):
        for bits in (52, 32):
            x, jac, rep, tabs = dump(engines, oracle, "ranges-" + fam, "ranges", "uniform", fam, bits)
            assert np.all(np.isfinite(jac)) and np.all(jac > 0), (fam, bits)                     # zeros_last: no 1 / 0 through the clamp
            for k, (l, slot) in enumerate(M.draws("ranges")):
                lf = M.LAYOUTS["ranges"]["leaves"][l]
                if lf[0] == "d":
                    dist = M.normalised(tabs[l])[0]
                    assert np.all(dist[(x[:, k] - lf[1]).astype(int)] > 0), (fam, bits, l)
    for plan in ("table-mode-1", "table-mode-2", "table-mode-3"):
        packed, again, r, ok, ref, layout, npb = run_plan(oracle, overrides, plan)
        name = PLANS[plan][0]
        dist = M.normalised(M.tables(layout, M.LAUNCHES[name][1], M.LAUNCHES[name][2])[2])[0]
        h = M.split(packed, layout)[4][2]
        assert np.any(dist == 0) and np.all(h[dist == 0] == M.offset_of_an_empty_bin(M.NBLOCKS)), plan
        assert np.all(h[dist > 0] > M.offset_of_an_empty_bin(M.NBLOCKS)), plan                 # (1024 draws over at most 17 bins: every other bin is hit)


def test_a_power_of_two_scale_of_grid_and_range_scales_every_x_and_changes_no_bin(engines, oracle):
    """... and the Jacobian by the power's tenth power, exactly: every operation of the draw is exact under the scale"""
    for fam in ("geometric", "spike_middle", "ulp_run"):
        for bits in (52, 32):
            x, jac, rep, tabs = dump(engines, oracle, "sizes-" + fam, "sizes", fam, "uniform", bits)
            eng = engines.get("sizes_scaled", bits)
            scaled = [g * 2.0 ** -20 for g in tabs]
            set_tables(eng, "sizes_scaled", scaled)
            xs, js, ws = eng.sample_dump(NSAMPLE, iteration=0, seed=M.SEED)
            assert np.array_equal(xs, x[:NSAMPLE] * 2.0 ** -20) and np.array_equal(js, jac[:NSAMPLE] * 2.0 ** -200), (fam, bits)
            srep = M.replay("sizes_scaled", scaled, stream(oracle, "sizes", range(NSAMPLE), bits))
            assert np.array_equal(srep["bin"], rep["bin"][:NSAMPLE]) and np.array_equal(srep["x"], xs)

