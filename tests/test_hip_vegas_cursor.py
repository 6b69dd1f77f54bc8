"""Cursor hand-out of the pipelined :vegas loop (csrc/mci_device.h, the cursor section; csrc/mci_host_iteration.h): the waves of a block's
workgroups take ranges of 128-sample units from the block's cursor word instead of walking a fixed share of the block.  Only the order
of the partial sums may change: the set of samples, their Philox indices and the measurement cadence are the fixed partition's.

Every case forces the path on (override vegas_cursor = 1) on the headline layout with 2 blocks and 3 workgroups per block (24 waves per
block) and holds the launch to the CPU oracle AND to the fixed partition of the same engine, at the tolerances of
tests/test_hip_parity.py (packed sums 1e-11, histogram 1e-9); the NEVAL and NORM columns, exact integers counted per range here and per
sample there, must be equal.  Every case also asserts that the launch did go through the cursor and through the 8-copy pipelined unit
that passed its self-check (a unit that fails it is replaced by the plain loop, which has no cursor and would pass everything here)."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import SEED, hist_split, make

pytestmark = pytest.mark.gpu
NAME = "c2_gauss16_shared_pool"
NBLOCK, WPB, WAVES = 2, 3, 3 * 8
LOG2_BIG, ONES = 4, 4   # the defaults (csrc/mci_host_types.h kCursorLog2Big, kCursorOnes)


def tickets(units, waves=WAVES, k=LOG2_BIG, ones=ONES):
    """ranges of a block of `units` units, restated from the rule's description: from the block's end `ones * waves` single units, then
    `waves` ranges each of 2, 4, ... 2^(k-1) units, then ranges of 2^k; the first range is what is left"""
    n, rem = 0, units
    for size, count in [(1, ones * waves)] + [(2 ** l, waves) for l in range(1, k)]:
        take = min(rem, size * count)
        n += -(-take // size)
        rem -= take
    return n + -(-rem // 2 ** k)


def launch(eng, overrides, cursor, npb, lo, it, mf=1):
    overrides.set("vegas_cursor", 1 if cursor else 0)
    got = eng.iteration("vegas", npb, lo, lo + NBLOCK, iteration=it, seed=SEED, measurefreq=mf)
    assert eng.last_launch_cursor()[0] == cursor
    return got


def check(oracle, overrides, eng, ocfg, cfg, c, npb, lo=0, it=1, mf=1):
    base0 = eng.last_launch_cursor()[1]
    got = launch(eng, overrides, True, npb, lo, it, mf)
    assert eng.last_launch_cursor()[1] == base0 + tickets(-(-npb // 128)) + WAVES
    static = launch(eng, overrides, False, npb, lo, it, mf)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], npb, lo, lo + NBLOCK, it, SEED, measurefreq=mf)
    nobs = eng.nobs
    for other in (ref, static):
        gs, gh = hist_split(got, nobs, cfg.N)
        rs, rh = hist_split(other, nobs, cfg.N)
        np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(gh, rh, rtol=1e-9)
    assert got[2 * nobs + 1] == static[2 * nobs + 1] == NBLOCK * npb       # NEVAL
    assert got[2 * nobs] == static[2 * nobs]                               # NORM (+ the 1e-10 offsets of the merge, the same in both)
    assert eng.vegas_check_status()[0] == 1, eng.vegas_check_status()
    assert eng.histogram_copies() == 8 and eng.kernel_times_ms(1)[1:] == (NBLOCK * WPB, 512)
    return got


def engine(oracle):
    c, cfg, eng, ocfg = make(NAME, oracle)
    eng.set_launch(0, WPB)
    return c, cfg, eng, ocfg


# 100: less than one unit -- one wave works, 23 idle; 677: a ragged last unit, lanes with one and with two samples in it, an odd count
# per lane; 70 000: 547 units, more than the taper's 24 x 18 -- big ranges, every taper level, single units
@pytest.mark.parametrize("mf", [1, 3])
@pytest.mark.parametrize("npb", [100, 677, 70000])
def test_cursor_launch_matches_oracle_and_fixed_partition(oracle, overrides, npb, mf):
    c, cfg, eng, ocfg = engine(oracle)
    check(oracle, overrides, eng, ocfg, cfg, c, npb, mf=mf)
    eng.close()


def test_seven_round_stream(oracle, overrides):
    c, cfg, eng, ocfg = engine(oracle)
    eng.set_rng_rounds(7)
    eng.set_launch(0, WPB)
    oracle.set_rng_rounds(7)
    try:
        check(oracle, overrides, eng, ocfg, cfg, c, 677)
    finally:
        oracle.set_rng_rounds(10)
    eng.close()


def test_32_bit_stream(oracle, overrides):
    c, cfg, eng, ocfg = engine(oracle)
    eng.set_rng_bits(32)
    eng.set_launch(0, WPB)
    ocfg.set_rng_bits(32)
    check(oracle, overrides, eng, ocfg, cfg, c, 677)
    eng.close()


def test_blocks_across_and_above_the_32_bit_index_boundary(oracle, overrides):
    """the per-workgroup choice between the loop with the hoisted Philox head and the generic one (tests/test_hip_philox_hoist.py): the
    first block's index range holds 2^32 (generic rounds), the second lies above it (high word 1)"""
    npb = 5000
    edge = 2 ** 32 // npb
    assert edge * npb < 2 ** 32 <= edge * npb + npb - 1
    c, cfg, eng, ocfg = engine(oracle)
    check(oracle, overrides, eng, ocfg, cfg, c, npb, lo=edge)
    eng.close()


def test_cursor_base_carries_across_launches_of_different_length(oracle, overrides):
    """three consecutive iterations on one engine, nothing cleared in between: each launch starts from the value the one before it left
    in the words (the fixed-partition launches in between leave them alone)"""
    c, cfg, eng, ocfg = engine(oracle)
    for it, npb in enumerate((677, 70000, 100), start=1):
        check(oracle, overrides, eng, ocfg, cfg, c, npb, it=it)
    assert eng.last_launch_cursor()[1] == sum(tickets(-(-n // 128)) + WAVES for n in (677, 70000, 100))
    eng.close()


def test_deterministic_mode_and_other_layouts_keep_the_fixed_partition(oracle, overrides):
    overrides.set("vegas_cursor", 1)
    c, cfg, eng, ocfg = engine(oracle)
    eng.set_deterministic(True)
    got = eng.iteration("vegas", 677, 0, NBLOCK, iteration=1, seed=SEED)
    assert eng.last_launch_cursor() == (False, 0)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 677, 0, NBLOCK, 1, SEED)
    np.testing.assert_allclose(hist_split(got, eng.nobs, cfg.N)[0], hist_split(ref, eng.nobs, cfg.N)[0], rtol=1e-11, atol=1e-300)
    eng.close()
    c, cfg, eng, ocfg = make("sphere2_padding", oracle)   # 2 + 3 draws on one grid: the plain loop
    got = eng.iteration("vegas", 677, 0, NBLOCK, iteration=1, seed=SEED)
    assert eng.last_launch_cursor() == (False, 0)
    np.testing.assert_allclose(got, ocfg.iteration(oracle.VEGAS, "sphere2", None, 677, 0, NBLOCK, 1, SEED), rtol=1e-9)
    eng.close()


def test_self_check_of_the_unit_still_passes_and_runs_without_the_cursor(oracle, overrides):
    """the first-use check of the code object (run here although the cache holds its marker) makes its small launches on the fixed
    partition and passes; the launch it precedes takes the cursor"""
    overrides.set("vegas_self_check", 1)
    c, cfg, eng, ocfg = engine(oracle)
    assert eng.vegas_check_status()[0] == 0 and eng.last_launch_cursor() == (False, 0)
    check(oracle, overrides, eng, ocfg, cfg, c, 677)
    assert eng.vegas_check_status()[0] == 1 and eng.vegas_check_launches() == 3
    eng.close()


def test_big_launch_takes_the_cursor_on_a_resident_grid_by_itself(overrides):
    """2^25 samples and no forced geometry: the launch rule picks the cursor on as many workgroups as the runtime's occupancy query says
    are resident -- a whole number per block, at most two per CU -- and the sums are the fixed partition's"""
    L = 50.0 ** 0.5
    cfg = mci.Configuration(var=mci.Continuous(-L, L), dof=[[16]], seed=SEED)
    eng = mci.Engine(cfg, mci.catalog.gaussian(16))
    npb, nb = 2 ** 21, 16
    got = eng.iteration("vegas", npb, 0, nb, iteration=1, seed=SEED)
    assert eng.last_launch_cursor()[0]
    wgs, threads = eng.kernel_times_ms(1)[1:]
    assert threads == 512 and wgs % nb == 0 and nb <= wgs <= 2 * 256
    waves = wgs // nb * 8
    assert eng.last_launch_cursor()[1] == tickets(npb // 128, waves=waves) + waves
    overrides.set("vegas_cursor", 0)
    static = eng.iteration("vegas", npb, 0, nb, iteration=1, seed=SEED)
    assert not eng.last_launch_cursor()[0] and eng.kernel_times_ms(1)[1] > wgs   # (the fixed partition's several rounds)
    gs, gh = hist_split(got, eng.nobs, cfg.N)
    rs, rh = hist_split(static, eng.nobs, cfg.N)
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(gh, rh, rtol=1e-9)
    assert got[2 * eng.nobs + 1] == static[2 * eng.nobs + 1] == nb * npb and got[2 * eng.nobs] == static[2 * eng.nobs]
    eng.close()
