"""The pipelined :vegas sample loop computes the lane-invariant part of Philox rounds 0-1 once per workgroup when the high word of the
sample index is the same for the whole statistical block (csrc/mci_device.h PhiloxHead), and runs the generic rounds when the block's
index range crosses a multiple of 2^32.  Either way the stream is the oracle's: draws bit-exact, packed sums at the tolerances of
tests/test_hip_parity.py -- below 2^32, above it (high word 1), and across it; on the opt-in 7-round and 32-bit streams too.
The sample dump draws with the generic rounds, so it is the packed sums of the iteration that judge the hoisted loop -- and only while the
engine still runs it: a code object that fails its first-use self-check is replaced by the plain layout with the generic rounds
(csrc/mci_host_check.h), which would pass everything here.  So every case asserts afterwards that the check passed and that the launch
was the 8-copy pipelined one."""
import numpy as np
import pytest

from test_hip_parity import SEED, hist_split, make

pytestmark = pytest.mark.gpu
NAME = "c2_gauss16_shared_pool"   # 16 draws on one grid: the pipelined loop, two samples per trip
NPB, NBLOCK = 5000, 8             # 40000 samples per case
EDGE = 2 ** 32 // NPB             # the block whose index range [EDGE * NPB, EDGE * NPB + NPB) holds 2^32
assert EDGE * NPB < 2 ** 32 <= EDGE * NPB + NPB - 1
# first block of the launch: every block below 2^32 | every block above | blocks on both sides of the one that straddles it
BLOCK_LO = {"below": 0, "above": EDGE + 1, "straddle": EDGE - 2}


def oracle_draws(oracle, ocfg, stream, gs, bits):
    oc = ocfg.c
    k = 0
    xo = np.zeros(oc.ndraw)
    for vi in range(oc.npool):
        nl = oc.pool_nleaf[vi]
        for idx in range(1, oc.maxdof[vi] + 1):
            us = [oracle.uniform(SEED, stream, gs, k + l, bits=bits) for l in range(nl)]
            ocfg.pool_create(vi, idx, us)
            for l in range(nl):
                xo[k + l] = ocfg.pool_data(oc.pool_leaf0[vi] + l)[idx - 1]
            k += nl
    return xo


def check(oracle, eng, ocfg, cfg, c, block_lo, bits=52):
    it = 1
    # draws of a block of the launch -- the straddling one where there is one -- sample for sample around its middle and its ends
    b = EDGE if block_lo <= EDGE < block_lo + NBLOCK else block_lo
    x, jac, w = eng.sample_dump(NPB, nevalperblock=NPB, block_index=b, iteration=it, seed=SEED)
    cross = 2 ** 32 - b * NPB   # the sample whose index is 2^32 (inside the block only when it straddles)
    for s in sorted({0, 1, 63, 64, 511, 512, 2500, NPB - 1} | ({cross - 1, cross, cross + 1} if 0 < cross < NPB - 1 else set())):
        assert np.array_equal(x[s], oracle_draws(oracle, ocfg, it * 8 + 0, b * NPB + s, bits)), (block_lo, s)
    got = eng.iteration("vegas", NPB, block_lo, block_lo + NBLOCK, iteration=it, seed=SEED)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], NPB, block_lo, block_lo + NBLOCK, it, SEED)
    gs, gh = hist_split(got, eng.nobs, cfg.N)
    rs, rh = hist_split(ref, eng.nobs, cfg.N)
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(gh, rh, rtol=1e-9)
    assert got[2 * eng.nobs + 1] == NBLOCK * NPB  # neval
    # the numbers above came out of the pipelined loop with the hoisted head, not out of the fallback a failed self-check installs
    assert eng.vegas_check_status()[0] == 1, eng.vegas_check_status()
    assert eng.histogram_copies() == 8 and eng.kernel_times_ms(1)[2] == 512
    return got


@pytest.mark.parametrize("where", list(BLOCK_LO))
def test_vegas_iteration_matches_oracle_around_the_32_bit_index_boundary(oracle, where):
    c, cfg, eng, ocfg = make(NAME, oracle)
    assert eng.histogram_copies() == 8   # the headline plan
    check(oracle, eng, ocfg, cfg, c, BLOCK_LO[where])


@pytest.mark.parametrize("where", ["above", "straddle"])
def test_seven_round_stream_with_the_hoisted_head(oracle, where):
    c, cfg, eng, ocfg = make(NAME, oracle)
    eng.set_rng_rounds(7)
    oracle.set_rng_rounds(7)
    try:
        check(oracle, eng, ocfg, cfg, c, BLOCK_LO[where])
    finally:
        oracle.set_rng_rounds(10)


@pytest.mark.parametrize("where", ["above", "straddle"])
def test_32_bit_stream_with_the_hoisted_head(oracle, where):
    """four draws per Philox block: four blocks per sample"""
    c, cfg, eng, ocfg = make(NAME, oracle)
    eng.set_rng_bits(32)
    ocfg.set_rng_bits(32)
    check(oracle, eng, ocfg, cfg, c, BLOCK_LO[where], bits=32)
