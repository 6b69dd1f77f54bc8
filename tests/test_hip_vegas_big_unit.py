"""The big :vegas unit on the device (csrc/mci_host_vegas_plan.h vegas_big_rule, csrc/mci_host_iteration.h select_vegas_big): the
measurefreq == 1 kernel with sixteen histogram copies in 1024-thread workgroups, which big cursor launches of eight-copy layouts run
instead of the standing 8 x 512 unit.  Only the order of the partial sums may differ from the standing unit's: same samples, same Philox
indices, same cursor ranges.

Setup: the headline layout, 2 blocks, the unit forced on at any size with the overrides vegas_big_unit = 1 and vegas_cursor = 1, one and
two workgroups per block (16 and 32 waves per block).  Every launch is held to the CPU oracle and to the standing unit on the same engine
at the tolerances of tests/test_hip_parity.py (packed sums 1e-11, histogram 1e-9) with NEVAL and NORM exactly equal, and must have run
1024 threads and 16 copies by cursor through a unit that passed its self-check."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import CASES, SEED, hist_split, make
from test_hip_vegas_cursor import tickets

pytestmark = pytest.mark.gpu
NAME = "c2_gauss16_shared_pool"
NBLOCK = 2
L = 50.0 ** 0.5


def same(got, other, nobs, ni):
    gs, gh = hist_split(got, nobs, ni)
    rs, rh = hist_split(other, nobs, ni)
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(gh, rh, rtol=1e-9)


def ran(eng):
    """(histogram copies, threads, workgroups, by cursor, threads the reported code object is bound to) of the last :vegas launch"""
    from mcintegration_jl_amd import isa_mix
    wgs, threads = eng.kernel_times_ms(1)[1:]
    bound = isa_mix.resources(eng.code_object("vegas"))["mci_vegas_batch"]["max_threads"]
    return eng.histogram_copies(), threads, wgs, eng.last_launch_cursor()[0], bound


def launch(eng, overrides, big, npb, lo, it, mf=1):
    overrides.set("vegas_cursor", 1)
    overrides.set("vegas_big_unit", 1 if big else 0)
    return eng.iteration("vegas", npb, lo, lo + NBLOCK, iteration=it, seed=SEED, measurefreq=mf)


def check(oracle, overrides, eng, ocfg, cfg, c, wpb, npb, lo=0, it=1):
    base0 = eng.last_launch_cursor()[1]
    got = launch(eng, overrides, True, npb, lo, it)
    assert ran(eng) == (16, 1024, NBLOCK * wpb, True, 1024)
    base1 = eng.last_launch_cursor()[1]
    assert base1 == base0 + tickets(-(-npb // 128), waves=16 * wpb) + 16 * wpb
    standing = launch(eng, overrides, False, npb, lo, it)
    assert ran(eng) == (8, 512, NBLOCK * wpb, True, 512)
    assert eng.last_launch_cursor()[1] == base1 + tickets(-(-npb // 128), waves=8 * wpb) + 8 * wpb
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], npb, lo, lo + NBLOCK, it, SEED)
    nobs = eng.nobs
    same(got, ref, nobs, cfg.N)
    same(got, standing, nobs, cfg.N)
    assert got[2 * nobs + 1] == standing[2 * nobs + 1] == NBLOCK * npb     # NEVAL
    assert got[2 * nobs] == standing[2 * nobs]                             # NORM
    status, flags = eng.vegas_check_status()
    assert status == 1 and not flags & 8, (status, flags)
    return got


def engine(oracle, wpb):
    c, cfg, eng, ocfg = make(NAME, oracle)
    eng.set_launch(0, wpb)
    return c, cfg, eng, ocfg


# 100: less than one unit -- one wave works, 15 (31) idle; 677: a ragged last unit, an odd count per lane; 70 000: 547 units, more than
# the taper's waves x 18 at one workgroup per block (288) and two (576 > 547: the taper alone) -- big ranges, every taper level, single units
@pytest.mark.parametrize("wpb", [1, 2])
@pytest.mark.parametrize("npb", [100, 677, 70000])
def test_big_unit_matches_oracle_and_standing_unit(oracle, overrides, npb, wpb):
    c, cfg, eng, ocfg = engine(oracle, wpb)
    check(oracle, overrides, eng, ocfg, cfg, c, wpb, npb)
    eng.close()


@pytest.fixture(scope="module")
def trained_grid(oracle):
    """eight training iterations of the oracle: narrow increments around the peak, a wave's adds pile onto a few bins"""
    c = CASES[NAME]
    ocfg = oracle.Config(c["oleaves"], c["dof"])
    ocfg.integrate(oracle.VEGAS, c["oname"], c["ud"], neval=800000, niter=8, block=16, seed=SEED, nthreads=8)
    grid = np.array(ocfg.grid(0))
    inc = np.diff(grid)
    assert inc.min() < 0.3 * (2 * L / 999) and inc.max() > 3.0 * (2 * L / 999)     # the map has adapted
    return grid


@pytest.mark.parametrize("wpb", [1, 2])
def test_trained_map(oracle, overrides, trained_grid, wpb):
    c, cfg, eng, ocfg = engine(oracle, wpb)
    eng.set_grid(0, trained_grid)
    ocfg.set_grid(0, trained_grid)
    check(oracle, overrides, eng, ocfg, cfg, c, wpb, 70000, it=7)
    eng.close()


def test_blocks_across_and_above_the_32_bit_index_boundary(oracle, overrides):
    """the first block's index range holds 2^32 (the generic Philox rounds), the second lies above it (the hoisted head, high word 1)"""
    npb = 5000
    edge = 2 ** 32 // npb
    assert edge * npb < 2 ** 32 <= edge * npb + npb - 1
    c, cfg, eng, ocfg = engine(oracle, 2)
    check(oracle, overrides, eng, ocfg, cfg, c, 2, npb, lo=edge)
    eng.close()


def test_other_cadence_keeps_the_standing_unit(oracle, overrides):
    c, cfg, eng, ocfg = engine(oracle, 2)
    got = launch(eng, overrides, True, 677, 0, 1, mf=3)
    assert ran(eng) == (8, 512, NBLOCK * 2, True, 512)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 677, 0, NBLOCK, 1, SEED, measurefreq=3)
    same(got, ref, eng.nobs, cfg.N)
    eng.close()


def test_alternating_units_share_the_cursor_words(oracle, overrides):
    """big and standing launches of different lengths on one engine, nothing cleared in between: a word moves by the tickets + waves of
    whichever unit ran (check() asserts the base after each launch), every result is the oracle's, and the reporting calls follow the
    unit of the last launch"""
    c, cfg, eng, ocfg = engine(oracle, 2)
    assert eng.histogram_copies() == 8                                     # before any launch: the standing plan
    total = 0
    for it, npb in enumerate((677, 70000, 100), start=1):
        check(oracle, overrides, eng, ocfg, cfg, c, 2, npb, it=it)
        total += tickets(-(-npb // 128), waves=32) + 32 + tickets(-(-npb // 128), waves=16) + 16
    assert eng.last_launch_cursor()[1] == total
    eng.close()


def test_launch_rule_picks_the_unit_by_size(overrides):
    """no overrides, no forced geometry: 16 x 2^22 samples run the big unit by cursor on the grid the runtime reports as resident -- one
    1024-thread workgroup per CU, a whole number per block, its partial rows kept --, 16 x 2^21 the standing (512 workgroups x 512
    threads, cursor) geometry; the reporting calls follow"""
    cfg = mci.Configuration(var=mci.Continuous(-L, L), dof=[[16]], seed=SEED)
    eng = mci.Engine(cfg, mci.catalog.gaussian(16))
    nb = 16
    big = eng.iteration("vegas", 2 ** 22, 0, nb, iteration=1, seed=SEED)
    copies, threads, wgs, cursor, bound = ran(eng)
    assert (copies, threads, cursor, bound) == (16, 1024, True, 1024) and wgs % nb == 0 and nb <= wgs <= 256
    waves = wgs // nb * 16
    assert eng.last_launch_cursor()[1] == tickets(2 ** 22 // 128, waves=waves) + waves
    assert eng.vegas_check_status()[0] == 1 and not eng.vegas_check_status()[1] & 8
    overrides.set("vegas_big_unit", 0)
    standing = eng.iteration("vegas", 2 ** 22, 0, nb, iteration=1, seed=SEED)
    assert ran(eng)[:2] == (8, 512) and ran(eng)[3]
    overrides.clear("vegas_big_unit")
    same(big, standing, eng.nobs, cfg.N)
    assert big[2 * eng.nobs + 1] == standing[2 * eng.nobs + 1] == nb * 2 ** 22 and big[2 * eng.nobs] == standing[2 * eng.nobs]
    eng.iteration("vegas", 2 ** 21, 0, nb, iteration=2, seed=SEED)
    assert ran(eng) == (8, 512, 512, True, 512)
    eng.close()


def test_perturbed_units_are_replaced_and_the_histogram_is_the_oracles(oracle, overrides, tmp_path, monkeypatch, capfd):
    """MCI_CHECK_PERTURB_HIST=1 shifts the pipelined adds of every unit compiled under it.  From the start: the standing unit fails its check
    first and the problem falls back to the plain layout as before -- which has no big unit.  Set after the standing unit has passed:
    only the big unit is compiled under it, fails, and is never selected again; the standing unit and its status stay."""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=1")
    c, cfg, eng, ocfg = engine(oracle, 2)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 4000, 0, NBLOCK, 0, SEED)
    got = launch(eng, overrides, True, 4000, 0, 0)
    same(got, ref, eng.nobs, cfg.N)
    assert eng.vegas_check_status()[0] == -1 and not eng.vegas_check_status()[1] & 8
    assert ran(eng)[:2] == (1, 256) and not eng.last_launch_cursor()[0]
    eng.close()

    monkeypatch.delenv("MCI_JIT_FLAGS")
    c, cfg, eng, ocfg = engine(oracle, 2)
    first = launch(eng, overrides, False, 4000, 0, 0)
    assert eng.vegas_check_status() == (1, 0) and ran(eng)[:2] == (8, 512)
    same(first, ref, eng.nobs, cfg.N)
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=1")
    capfd.readouterr()
    launches = eng.vegas_check_launches()
    for _ in range(2):
        got = launch(eng, overrides, True, 4000, 0, 0)
        same(got, ref, eng.nobs, cfg.N)
        assert ran(eng) == (8, 512, NBLOCK * 2, True, 512)
        assert eng.vegas_check_status() == (1, 8)
        assert eng.vegas_check_launches() == launches + 3          # (one check of the big unit: its launch, the dump, the static kernel)
    assert capfd.readouterr().err.count("the big :vegas unit of this problem") == 1
    eng.close()
