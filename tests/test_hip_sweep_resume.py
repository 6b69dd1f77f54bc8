"""GPU tests of carried chain sweeps that go on from the chains of the call before (Engine.integrate_sweep_chains | integrate_sweep_mcmc(...,
carry=True, state=[r["chain_state"] ...]); mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume; csrc/mci_sweep_chains.h
chain_sweep<Cfg, MCMC, true, true>): a run split in two calls against the unsplit run bit for bit, every iteration of two joined calls
with different chain counts against the oracle's carried iterations, the :mcmc burn-in that is no longer paid, the C ABI itself, and
another assignment of points to workgroups.

Helpers, layouts and tolerances are those of test_hip_sweep_carry and test_hip_sweep_mcmc: iteration `it` of a point's lineage against
the oracle's 1e-8 * 10^it (mean) and 1e-5 * 10^it (error), final factors 1e-4, maps 1e-4 of their range.  Bit-for-bit comparisons use 7
chains per block (that module's note on one wave)."""
import ctypes as C

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import _lib
from test_hip_parity import SEED
from test_hip_sweep_carry import carried_oracle, same, sweep
from test_hip_sweep_leaves import check_map, unpack
from test_hip_sweep_mcmc import TR, engine, rows, ud_array

pytestmark = pytest.mark.gpu
SOLVERS = ["vegasmc", "mcmc"]
LAYOUTS = ["discrete", "sphere2_padding"]
SEEDS = [SEED, SEED + 1, SEED + 2]          # (these layouts have no userdata to tell the points apart)
NPB, BLOCK, K = 700, 5, 7                   # idle lanes, one wave of chains per block


def three_points(name, oracle):
    """(case, configuration, engine, userdata rows): three points on two workgroups"""
    c, cfg, eng = engine(name, oracle)
    eng.sweep_workgroups(2)
    return c, cfg, eng, rows(name, c, 3)


def joined(rs):
    """what the next call takes from the results of the one before"""
    assert all(r["chain_state"] is not None for r in rs)
    return dict(maps=[r["maps"] for r in rs], reweight=[r["reweight"] for r in rs], state=[r["chain_state"] for r in rs])


def same_state(a, b):
    assert a.record() == b.record(), (a, b)
    assert a.data.tobytes() == b.data.tobytes()


@pytest.mark.parametrize("adapt", [True, False])
@pytest.mark.parametrize("n1", [1, 2, 3])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_a_split_run_equals_the_whole_bit_for_bit(oracle, name, solver, n1, adapt):
    """niter = 4 in one carried call against n1 and 4 - n1 iterations joined through maps, reweight, chain_state and first_iteration = n1:
    rows n1..3 of iter_mean and iter_std, the final maps and factors and the bytes of the final chain state.  :vegasmc with adapt = True
    split after its first iteration starts the second call afresh and carries from that call's second iteration on (carry_first = 1);
    every other split continues the stored chains in its first iteration."""
    c, cfg, eng, uds = three_points(name, oracle)
    kw = dict(neval=NPB * BLOCK, block=BLOCK, seeds=SEEDS, nchain=K, adapt=adapt, ignore=0, carry=True)
    whole = sweep(eng, solver, uds, niter=4, **kw)
    assert eng.last_sweep_launch() == (2, 256)
    head = sweep(eng, solver, uds, niter=n1, **kw)
    tail = sweep(eng, solver, uds, niter=4 - n1, first_iteration=n1, **dict(kw, **joined(head)))
    continues = solver == "mcmc" or not adapt or n1 >= 2
    for w, h, t in zip(whole, head, tail):
        print(name, solver, n1, adapt, "whole", w["iter_mean"][:, 0], "head", h["iter_mean"][:, 0], "tail", t["iter_mean"][:, 0])
        assert w["iter_mean"][:n1].tobytes() == h["iter_mean"].tobytes() and w["iter_std"][:n1].tobytes() == h["iter_std"].tobytes()
        assert w["iter_mean"][n1:].tobytes() == t["iter_mean"].tobytes()
        assert w["iter_std"][n1:].tobytes() == t["iter_std"].tobytes()
        for k in ("maps", "reweight", "propose", "accept", "visited"):
            assert np.asarray(w[k]).tobytes() == np.asarray(t[k]).tobytes(), k
        same_state(w["chain_state"], t["chain_state"])
        assert w["neval"] == h["neval"] + t["neval"] and t["status"] == 0
        assert t["continued"] is continues and h["continued"] is False
        assert t["correlated"] is (continues or 4 - n1 > 1)
        st = t["chain_state"]
        assert (st.solver, st.blocks, st.nchain, st.iteration, st.adapted) == (solver, BLOCK, K, 3, adapt) and st.ntrain == (3 if adapt else 0)


@pytest.fixture(scope="module")
def lds_limit(oracle):
    return engine("discrete", oracle)[2].sweep_resample_lds()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name,case", [("discrete", "few->many"), ("sphere2_padding", "few->many"), ("discrete", "many->few"),
                                       ("sphere2_padding", "many->few"), ("discrete", "lds")])
def test_every_iteration_of_two_joined_calls_is_the_oracles(oracle, lds_limit, name, solver, case):
    """per point a fresh oracle config with set_chain_carry(1) runs iterations 0..3, the first two with nchain = K1, the last two with K2;
    the engine runs two calls of two iterations joined through the chain state.  few->many: (7, 300) -- more new chains than stored
    ones, a lane runs a second chain and a resampler thread owns two chains; many->few: (300, 7); lds: (lds_w + 1, 7) on two blocks with
    stored chains of two steps -- the stored side crosses the resampler's LDS limit at the continued call's iteration 0."""
    c, cfg, eng, uds = three_points(name, oracle)
    if case == "lds":
        k1, k2, block = lds_limit + 1, 7, 2
        npb = 2 * k1
    else:
        (k1, k2), block, npb = ((7, 300) if case == "few->many" else (300, 7)), 3, 1500
    kw = dict(neval=npb * block, niter=2, block=block, seeds=SEEDS, carry=True)
    head = sweep(eng, solver, uds, nchain=k1, **kw)
    tail = sweep(eng, solver, uds, nchain=k2, first_iteration=2, **dict(kw, **joined(head)))
    nobs, nd = eng.nobs, cfg.N + 1
    osolver = oracle.MCMC if solver == "mcmc" else oracle.VEGASMC
    for seed, ud, h, t in zip(SEEDS, uds, head, tail):
        ocfg = carried_oracle(oracle, c)
        neval = [0, 0]
        for it in range(4):
            r, row = (h, it) if it < 2 else (t, it - 2)
            packed = ocfg.iteration(osolver, c["oname"], ud or None, npb, 0, block, it, seed, nchain=k1 if it < 2 else k2)
            om, oe = oracle.mean_std(packed[:nobs], packed[nobs:2 * nobs], block)
            neval[it // 2] += int(packed[2 * nobs + 1])
            print(name, solver, case, "it", it, "mean", r["iter_mean"][row], om, "std", r["iter_std"][row], oe)
            np.testing.assert_allclose(r["iter_mean"][row], om, rtol=1e-8 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            np.testing.assert_allclose(r["iter_std"][row], oe, rtol=1e-5 * 10 ** it, atol=1e-300, err_msg="iteration %d" % it)
            ocfg.set_reweight(oracle.do_reweight(ocfg.reweight, packed[2 * nobs + 2:2 * nobs + 2 + nd]))
            ocfg.train()
        assert [h["neval"], t["neval"]] == neval and t["status"] == 0
        assert t["continued"] is True and t["correlated"] is True and t["chain_state"].nchain == k2 and t["chain_state"].iteration == 3
        np.testing.assert_allclose(t["reweight"], ocfg.reweight, rtol=1e-4)
        for l, (lf, parts) in enumerate(zip(c["oleaves"], unpack(c["oleaves"], t["maps"]))):
            if lf["kind"] == 0:
                check_map(parts[0], ocfg.grid(l), 1e-4)
            else:
                np.testing.assert_allclose(parts[1], ocfg.distribution(l), rtol=0, atol=1e-4)


@pytest.mark.parametrize("niter", [1, 3])
@pytest.mark.parametrize("name", LAYOUTS)
def test_a_continued_mcmc_call_holds_no_burn_in(oracle, name, niter):
    c, cfg, eng, uds = three_points(name, oracle)
    kw = dict(neval=NPB * BLOCK, block=BLOCK, seeds=SEEDS, nchain=K, carry=True)
    head = sweep(eng, "mcmc", uds, niter=2, **kw)
    j = joined(head)
    on = sweep(eng, "mcmc", uds, niter=niter, first_iteration=2, **dict(kw, **j))
    off = sweep(eng, "mcmc", uds, niter=niter, first_iteration=2, **dict(kw, maps=j["maps"], reweight=j["reweight"]))
    for a, b in zip(on, off):
        print(name, niter, "neval with the state", a["neval"], "without", b["neval"])
        assert a["neval"] < b["neval"]                               # the first iteration burns in without the state, none with it
        assert a["holds"].sum() == niter * BLOCK * K                 # one longest hold per chain and iteration: the measured steps alone
        assert a["correlated"] is True and a["carried"] is True and a["continued"] is True and a["status"] == 0
        assert b["continued"] is False and b["correlated"] is (niter > 1)


def c_sweep(eng, solver, a, P, niter, ud, state_in=None, state_out=None, resume=True, maps=None, rw=None):
    """the C entry points themselves on ctypes structures; -> (rc, result dicts | None)"""
    from mcintegration_jl_amd.engine import _dp
    mcmc = solver == "mcmc"
    lib = mci.lib()
    fn = ((lib.mci_integrate_sweep_mcmc_resume if mcmc else lib.mci_integrate_sweep_chains_resume) if resume
          else (lib.mci_integrate_sweep_mcmc if mcmc else lib.mci_integrate_sweep_chains))
    nd = eng.config.N + 1
    m = max(nd, len(eng.config.var))

    def extra(P):
        ro, pa = np.zeros((P, nd)), np.zeros((P, 2, 3, nd, m))
        own = (_dp(rw) if rw is not None else None, _dp(ro), _dp(pa))
        keys = dict(reweight=ro, pa=pa)
        if mcmc:
            ho = np.zeros((P, 64), dtype=np.uint64)
            own += (ho.ctypes.data_as(C.POINTER(C.c_uint64)),)
            keys["holds"] = ho
        if resume:
            own += (C.byref(state_in) if state_in is not None else None, C.byref(state_out) if state_out is not None else None)
        return own, keys
    try:
        return 0, eng._sweep_call(fn, a, P, niter, (ud, None, maps), extra)
    except mci.MCIError as e:
        return e, None


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_c_abi_hands_the_states_out_and_takes_them_in(oracle, solver):
    c, cfg, eng, uds = three_points("discrete", oracle)
    ud, P = ud_array(uds), 3
    args = lambda niter, first, s=solver: eng._integrate_args(s, NPB * BLOCK, niter, BLOCK, 0, True, 1.0, 1, SEED, first, K, TR)
    eng.set_sweep_chain_carry(True)
    try:
        n, info = eng.sweep_chain_state_doubles(solver, NPB * BLOCK, 2, BLOCK, nchain=K, thermal_ratio=TR)
        cap = BLOCK * K
        assert n == eng.ndraw * cap + ((cap + 1) // 2 + cfg.N + 1 if solver == "mcmc" else cap)
        assert (info["blocks"], info["nchain"], info["iteration"], info["ntrain"], info["adapted"]) == (BLOCK, K, 1, 1, 1)
        # NULL for both: the carried sweep's bytes
        rc, plain = c_sweep(eng, solver, args(4, 0), P, 4, ud, resume=False)
        rc2, nulls = c_sweep(eng, solver, args(4, 0), P, 4, ud)
        assert rc == 0 and rc2 == 0
        for a, b in zip(plain, nulls):
            same(a, b, keys=("iter_mean", "iter_std", "mean", "stdev", "maps", "reweight", "pa", "visited"))
        # state_out of one call as state_in of the next: the whole run
        rows_out = np.zeros((P, n))
        s1 = _lib.SweepChainState(_lib.SweepChainInfo(), rows_out.ctypes.data_as(_lib.c_double_p))
        rc, head = c_sweep(eng, solver, args(2, 0), P, 2, ud, state_out=s1)
        assert rc == 0 and (s1.info.solver, s1.info.blocks, s1.info.nchain, s1.info.iteration, s1.info.ntrain, s1.info.adapted) == \
            (_lib.SOLVERS[solver], BLOCK, K, 1, 1, 1)
        maps = np.ascontiguousarray([r["maps"] for r in head])
        rw = np.ascontiguousarray([r["reweight"] for r in head])
        rows2 = np.zeros((P, n))
        s2 = _lib.SweepChainState(_lib.SweepChainInfo(), rows2.ctypes.data_as(_lib.c_double_p))
        rc, tail = c_sweep(eng, solver, args(2, 2), P, 2, ud, state_in=s1, state_out=s2, maps=maps, rw=rw)
        assert rc == 0 and s2.info.iteration == 3 and s2.info.ntrain == 3
        for w, t in zip(plain, tail):
            assert w["iter_mean"][2:].tobytes() == t["iter_mean"].tobytes() and w["iter_std"][2:].tobytes() == t["iter_std"].tobytes()
            assert w["maps"].tobytes() == t["maps"].tobytes() and w["reweight"].tobytes() == t["reweight"].tobytes() and t["correlated"] is True
        # a gap in the iteration numbers, the other solver: refused by name, nothing runs
        rc, none = c_sweep(eng, solver, args(2, 3), P, 2, ud, state_in=s1, maps=maps, rw=rw)
        assert none is None and rc.code == 1 and "a gap in the iteration numbers" in str(rc) and "first_iteration = 3" in str(rc)
        other = "vegasmc" if solver == "mcmc" else "mcmc"
        rc, none = c_sweep(eng, other, args(2, 2, other), P, 2, ud, state_in=s1, maps=maps, rw=rw)
        assert none is None and rc.code == 1 and "the state is another solver's" in str(rc)
    finally:
        eng.set_sweep_chain_carry(False)


@pytest.mark.parametrize("solver", SOLVERS)
def test_another_assignment_of_points_to_workgroups_leaves_every_point_alone(oracle, solver):
    c, cfg, eng, uds = three_points("sphere2_padding", oracle)
    kw = dict(neval=NPB * BLOCK, block=BLOCK, seeds=SEEDS, nchain=K, adapt=False, carry=True)
    head = sweep(eng, solver, uds, niter=2, **kw)
    runs = []
    for g in (1, 2):
        eng.sweep_workgroups(g)
        runs.append(sweep(eng, solver, uds, niter=2, first_iteration=2, **dict(kw, **joined(head))))
        assert eng.last_sweep_launch()[0] == g
    for a, b in zip(*runs):
        same(a, b)
        same_state(a["chain_state"], b["chain_state"])
        assert a["continued"] is True and a["status"] == 0
    assert runs[0][0]["chain_state"].data.tobytes() != runs[0][1]["chain_state"].data.tobytes()
