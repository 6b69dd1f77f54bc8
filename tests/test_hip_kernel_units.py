"""GPU test of the life cycle of a problem's kernel units (csrc/mci_host_types.h KernelUnit): every JIT unit is compiled, loaded and run
once, all modules are dropped twice (set_rng_rounds(7), then back to 10), and everything is compiled -- now from the kernel cache -- loaded
and run again.  The second run of a unit goes through the same code object on the same inputs, so only the order of the atomic adds can
differ: packed sums agree to 1e-11 and histograms (and what lies behind them) to 1e-9, the tolerances tests/test_hip_parity.py holds HIP
to against the oracle; the sweep units to those of tests/test_hip_sweep_units.py.  code_object(...) names the same files before and after,
and closing the engines leaves the context clean for the next one.

x2y2 (2-D, one Continuous leaf) at 2 blocks x 512 samples: the :vegas units of both cadences, the sample dump, the persistent unit, the
stratified unit, the one-grid sweep unit with 2 points.  The bubble layout (four Continuous leaves and a Discrete one): :vegasmc and
:mcmc, both several-lanes-per-chain units, the sweep unit for several leaves.  Only the Engine API: the test does not know how the
library keeps its modules."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import SEED, hist_split, make as make_case
from test_hip_sweep_leaves import bubble_row
from test_hip_sweep_strat import make as make_x2y2
from test_hip_sweep_units import same_sweep

pytestmark = pytest.mark.gpu

NPB, BLOCK = 512, 2


def x2y2_round(eng):
    """-> ({name: packed-like array}, {name: sweep results}, {unit: code object})"""
    grid0 = eng.grid(0).copy()
    out, obj = {}, {}
    out["vegas any cadence"] = eng.iteration("vegas", NPB, 0, BLOCK, iteration=0, seed=SEED, measurefreq=3)
    obj["vegas any cadence"] = eng.code_object("vegas")       # (the only :vegas unit so far)
    out["vegas"] = eng.iteration("vegas", NPB, 0, BLOCK, iteration=0, seed=SEED)
    obj["vegas"] = eng.code_object("vegas")
    assert obj["vegas"] != obj["vegas any cadence"]
    x, jac, w = eng.sample_dump(256, nevalperblock=NPB, block_index=1, iteration=0, seed=SEED)
    out["dump"] = np.concatenate([x.ravel(), jac, w.ravel()])
    eng.set_persistent("on")
    r = eng.integrate("vegas", neval=NPB * BLOCK, niter=2, block=BLOCK, seed=SEED)
    assert eng.last_integrate_persistent()
    eng.set_persistent("auto")
    out["persistent"] = np.concatenate([r["iter_mean"].ravel(), r["iter_std"].ravel()])
    obj["vegas_persistent"] = eng.code_object("vegas_persistent")
    eng.set_grid(0, grid0)                                      # (the two iterations trained the map)
    eng.set_stratification()
    out["stratified"] = eng.iteration("vegas", NPB, 0, BLOCK, iteration=0, seed=SEED)
    obj["vegas_strat"] = eng.code_object("vegas_strat")
    eng.set_stratification(on=False)
    sweep = eng.integrate_sweep("vegas", userdata=[[1.0], [0.25]], neval=NPB * BLOCK, niter=1, block=BLOCK, seed=SEED)
    obj["vegas_sweep"] = eng.code_object("vegas_sweep")
    return out, {"sweep": sweep}, obj


def bubble_round(eng):
    out, obj = {}, {}
    eng.set_chain_speculation(lanes=1)
    for solver in ("vegasmc", "mcmc"):
        out[solver] = eng.iteration(solver, NPB, 0, BLOCK, iteration=0, seed=SEED, nchain=8)
        assert eng.last_chain_speculation()[0] == 1
        obj[solver] = eng.code_object(solver)
    eng.set_chain_speculation(lanes=16)
    for solver in ("vegasmc", "mcmc"):
        out[solver + " lanes"] = eng.iteration(solver, NPB, 0, BLOCK, iteration=0, seed=SEED, nchain=1)
        assert eng.last_chain_speculation()[0] == 16 and eng.chain_speculation_status(solver) == 1
        obj[solver + "_lanes"] = eng.code_object(solver + "_lanes")
    eng.set_sweep_leaves("all")
    sweep = eng.integrate_sweep("vegas", userdata=[bubble_row(0), bubble_row(1)], neval=NPB * BLOCK, niter=1, block=BLOCK, seed=SEED)
    obj["vegas_sweep_leaves"] = eng.code_object("vegas_sweep_leaves")
    return out, {"sweep leaves": sweep}, obj


def same(first, second, nhead):
    for name in first[0]:
        a, b = first[0][name], second[0][name]
        n = nhead if len(a) > nhead and name not in ("dump", "persistent") else len(a)
        print(name, "largest relative difference, sums:", np.max(np.abs(a[:n] - b[:n]) / np.maximum(np.abs(a[:n]), 1e-300)),
              "behind them:", np.max(np.abs(a[n:] - b[n:]) / np.maximum(np.abs(a[n:]), 1e-300)) if len(a) > n else 0.0)
    for name in first[0]:
        a, b = first[0][name], second[0][name]
        n = nhead if len(a) > nhead and name not in ("dump", "persistent") else len(a)
        np.testing.assert_allclose(b[:n], a[:n], rtol=1e-11, atol=1e-300, err_msg=name)
        np.testing.assert_allclose(b[n:], a[n:], rtol=1e-9, atol=1e-300, err_msg=name)
    for name in first[1]:
        same_sweep(first[1][name], second[1][name])
    assert first[2] == second[2]                              # the same files, before and after


def test_every_unit_runs_again_after_its_modules_were_dropped(oracle):
    _, a, _, _ = make_x2y2(oracle, "x2y2", 1.0)
    _, cfg_b, b, _ = make_case("bubble", oracle)
    rounds = []
    for k in range(2):
        rounds.append((x2y2_round(a), bubble_round(b)))
        if k == 0:
            for eng in (a, b):                                 # every module goes, twice; the streams end where they were
                eng.set_rng_rounds(7)
                eng.set_rng_rounds(10)
                with pytest.raises(mci.MCIError, match="has not been compiled yet"):
                    eng.code_object("vegas")
    same(rounds[0][0], rounds[1][0], len(hist_split(rounds[0][0][0]["vegas"], a.nobs, a.config.N)[0]))
    same(rounds[0][1], rounds[1][1], len(hist_split(rounds[0][1][0]["vegasmc"], b.nobs, cfg_b.N)[0]))
    assert len(set(rounds[0][0][2].values()) | set(rounds[0][1][2].values())) == 10      # ten named units (the sample dump has no name), ten code objects
    a.check_status()
    b.check_status()
    a.close()
    b.close()
    _, c, _, _ = make_x2y2(oracle, "x2y2", 1.0)              # a second engine of the same context
    c.check_status()
    c.iteration("vegas", NPB, 0, BLOCK, iteration=0, seed=SEED)
    c.check_status()
    c.close()
