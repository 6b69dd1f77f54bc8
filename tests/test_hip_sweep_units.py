"""GPU tests of what the three sweep units share on the host (csrc/mci_host_sweep.h: one descriptor table, compile_sweep_unit, sweep_run): ONE
problem and ONE context running different units in turn, and the one-grid unit loaded again for another workgroup size.  The layout is
x2y2 of tests/test_hip_sweep_strat.py (2-D, one Continuous leaf, default increments) at neval = 2000, niter = 2, block = 4: three points on
two workgroups, so that one workgroup runs two points.  Tolerances between two classic sweeps of the same inputs are those of
tests/test_hip_sweep.py: 1e-11 / 1e-8 on an iteration that follows no train!, 1e-4 / 1e-2 over a run, maps 1e-4."""
import numpy as np
import pytest

from test_hip_stratified_parity import SEED
from test_hip_sweep_strat import check_point, make, merged_blocks

pytestmark = pytest.mark.gpu

UDS = [1.0, 0.25, -2.0]
N, NITER, BLOCK = 2000, 2, 4


def classic(eng):
    return eng.integrate_sweep("vegas", userdata=[[u] for u in UDS], neval=N, niter=NITER, block=BLOCK, seed=SEED)


def same_sweep(a, b):
    for p, (x, y) in enumerate(zip(a, b)):
        assert x["status"] == 0 and y["status"] == 0, p
        np.testing.assert_allclose(y["iter_mean"][0], x["iter_mean"][0], rtol=1e-11, atol=1e-300, err_msg="point %d" % p)
        np.testing.assert_allclose(y["iter_std"][0], x["iter_std"][0], rtol=1e-8, atol=1e-300, err_msg="point %d" % p)
        np.testing.assert_allclose(y["iter_mean"], x["iter_mean"], rtol=1e-4, atol=1e-300, err_msg="point %d" % p)
        np.testing.assert_allclose(y["iter_std"], x["iter_std"], rtol=1e-2, atol=1e-300, err_msg="point %d" % p)
        np.testing.assert_allclose(y["maps"], x["maps"], rtol=0, atol=1e-4, err_msg="point %d" % p)


def test_classic_stratified_classic_on_one_engine(oracle):
    _, eng, ocfg, of = make(oracle, "x2y2", UDS[0])
    eng.sweep_workgroups(2)
    first = classic(eng)
    assert eng.last_sweep_launch() == (2, 256)
    path = eng.code_object("vegas_sweep")
    m = [r["iter_mean"][0, 0] for r in first]
    assert abs(m[0] - m[1]) > 0.1 and abs(m[0] - m[2]) > 0.1      # (the points ARE different integrals)
    # the stratified unit, teacher-forced as test_hip_sweep_strat.chain drives it: NITER sweeps of one iteration, maps and d fed back
    eng.set_stratification()
    plan = eng.sweep_strat_plan(neval=N, block=BLOCK)
    nstrat, beta, nc = plan["nstrat"], plan["beta"], plan["ncube"]
    m_blocks = merged_blocks(eng, N, BLOCK)
    want = [np.diff(oracle.Config.strat_alloc(np.ones(nc), N, True))] * len(UDS)
    maps, d = None, None
    for k in range(NITER):
        start = [eng.grid(0)] * len(UDS) if maps is None else maps
        rs = eng.integrate_sweep_strat("vegas", userdata=[[u] for u in UDS], neval=N, niter=1, block=BLOCK, seed=SEED, ignore=0, maps=maps, d=d,
                                       first_iteration=k)
        assert eng.last_sweep_launch() == (2, 256)
        nxt = []
        for p, u in enumerate(UDS):
            dref, _ = check_point(oracle, ocfg, of, [u], rs[p], start[p], want[p], nstrat, N, k, SEED, beta, m_blocks, "x2y2 point %d iteration %d" % (p, k))
            nxt.append(np.diff(oracle.Config.strat_alloc(dref, N)))
        want = nxt
        maps, d = np.array([r["maps"] for r in rs]), np.array([r["strat_d"] for r in rs])
    assert eng.code_object("vegas_sweep_strat") != path
    # ... and the one-grid unit again: what it was, where it was
    eng.set_stratification(on=False)
    again = classic(eng)
    assert eng.last_sweep_launch() == (2, 256)
    same_sweep(first, again)
    assert eng.code_object("vegas_sweep") == path
    eng.close()


def test_the_one_grid_unit_is_loaded_again_for_another_workgroup_size(oracle):
    _, eng, _, _ = make(oracle, "x2y2", UDS[0])
    eng.sweep_workgroups(2)
    eng.sweep_threads(512)
    wide = classic(eng)
    assert eng.last_sweep_launch() == (2, 512)
    eng.sweep_threads(0)
    narrow = classic(eng)
    assert eng.last_sweep_launch() == (2, 256)
    same_sweep(wide, narrow)
    eng.close()
