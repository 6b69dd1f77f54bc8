"""GPU tests of the carried chains' resampler kernel on its own (csrc/mci_train.h resample_block through k_resample_chains, launched by the
test hook Engine.resample exactly as an ordinary carried launch launches it), path by path over the case table of
tests/resample_cases.py: a weight per stored chain (:vegasmc), per-integrand counts in registers (:mcmc, up to 16 integrands), one pass
per integrand over W in global memory (more), bisections in LDS (up to 8192 stored chains per block) and in global memory (more), and
the spread c % n_old where the total weight is zero or not a number.

Three yardsticks.  The oracle's mirrors: the SAME picks, element for element, no tolerance ("same operations in the same order").  The
long-double reference of resample_cases: W within gamma and never decreasing, picks equal except within 2 gamma of a tie, at most 1e-3 of
a case's picks excused (the derivation is in that module; tests/test_resample_host.py holds the mirrors to it on the CPU).  And the
cases whose answer is known outright.  One launch per case; the kernel's output is computed once and shared by the tests."""
import numpy as np
import pytest

import resample_cases as R
from test_hip_parity import SEED, make
from test_resample_host import GROUPS

pytestmark = pytest.mark.gpu

_OUT = {}


@pytest.fixture(scope="module")
def device(oracle):
    """one small engine, for its device and stream only"""
    eng = make("sphere2_padding", oracle)[2]
    yield eng
    eng.close()


def kernel(eng, c):
    if c["id"] not in _OUT:
        src, W = eng.resample(c["curr"], c["rw_now"], c["rw_used"], c["n_new"], w_chain=c["w_chain"])
        src.setflags(write=False)
        W.setflags(write=False)
        _OUT[c["id"]] = (src, W)
    return _OUT[c["id"]]


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_kernel_picks_what_the_mirror_picks(oracle, device, group):
    for c in GROUPS[group]:
        src, _ = kernel(device, c)
        assert src.min() >= 0 and src.max() < c["n_old"], (c["id"], src.min(), src.max())
        np.testing.assert_array_equal(src, R.mirror(oracle, c), err_msg=c["id"])


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g not in ("f", "i")))
def test_the_kernel_against_the_long_double_reference(device, group):
    for c in GROUPS[group]:
        src, W = kernel(device, c)
        R.check_running_weights(c, W, "kernel")
        excused = R.check_picks(c, src, "kernel")
        print("%-28s %8d picks, %d within 2 gamma of a tie" % (c["id"], src.size, excused))


def test_a_total_of_zero_or_nan_spreads_the_new_chains_over_the_stored_ones(device):
    for c in GROUPS["f"]:
        np.testing.assert_array_equal(kernel(device, c)[0], R.fallback_picks(c), err_msg=c["id"])


def test_equal_weights_continue_every_stored_chain_equally_often(device):
    for n_old in R.N_OLD:
        for nd, w_chain in ((1, np.ones((3, n_old))), (5, None), (17, None)):
            curr = np.random.default_rng(SEED + n_old).integers(0, nd, size=(3, n_old))
            rw = np.full(nd, 0.75)
            src, _ = device.resample(curr, rw, rw, n_old, w_chain=w_chain)
            np.testing.assert_array_equal(src, np.tile(np.arange(n_old), (3, 1)), err_msg="%d stored chains, nd %d" % (n_old, nd))
            src, _ = device.resample(curr, rw, rw, 2 * n_old, w_chain=w_chain)
            np.testing.assert_array_equal(src, np.tile(np.repeat(np.arange(n_old), 2), (3, 1)), err_msg="%d stored chains, nd %d" % (n_old, nd))


@pytest.mark.parametrize("solver", ["vegasmc", "mcmc"])
def test_the_hook_leaves_the_engines_own_chains_alone(oracle, solver):
    """mci_debug_resample takes the problem's device and stream only: the record of its last chain launch and the bytes of its next
    carried iteration are those of a twin that never called the hook"""
    kw = {"thermal_ratio": 0.1} if solver == "mcmc" else {}

    def started():
        eng = make("sphere2_padding", oracle)[2]
        eng.set_chain_carry(1)
        eng.set_chain_speculation(1)
        eng.integrate(solver, neval=4 * 500, niter=3, block=4, seed=SEED, nchain=4, **kw)
        return eng
    eng, twin = started(), started()
    last, rw, packed = eng.last_chain_launch(), eng.reweight().copy(), eng.get_packed().copy()
    assert last == (4, True)
    for c in (GROUPS["w-uniform"][5], GROUPS["m-nd5"][3], GROUPS["m-nd17"][3], GROUPS["f"][0]):
        eng.resample(c["curr"], c["rw_now"], c["rw_used"], c["n_new"], w_chain=c["w_chain"])
    assert eng.last_chain_launch() == last and eng.reweight().tobytes() == rw.tobytes() and eng.get_packed().tobytes() == packed.tobytes()
    a = eng.iteration(solver, 500, 0, 4, iteration=3, seed=SEED, nchain=4, **kw)
    b = twin.iteration(solver, 500, 0, 4, iteration=3, seed=SEED, nchain=4, **kw)
    assert eng.last_chain_launch() == twin.last_chain_launch() == (4, True) and a.tobytes() == b.tobytes()
    eng.close()
    twin.close()
