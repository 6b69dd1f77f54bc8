"""The geometry of a sample launch (csrc/mci_host_iteration.h, the launch plan): workgroups, workgroup size, chains, lanes per chain,
cursor, chunks.  One iteration per case, on both sides of every threshold of the grid rule at the smallest sizes that reach it, and the
launch's record is compared with the table below.  The table was recorded by running this file on an MI355X before the launch path was
split into a plan and stages; the rule is not supposed to move, so a case that fails names a decision that changed.

Every case prints its figures before it asserts (pytest -s)."""
import math

import numpy as np
import pytest

import mcintegration_jl_amd as mci

pytestmark = pytest.mark.gpu
SEED = 20240229
L16 = 50.0 ** 0.5


def x2y2(**kw):
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED), mci.catalog.x2y2(), **kw)


def gauss16(**kw):
    return mci.Engine(mci.Configuration(var=mci.Continuous(-L16, L16), dof=[[16]], seed=SEED), mci.catalog.gaussian(16), **kw)


def sphere2(**kw):
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], seed=SEED), mci.catalog.sphere2(), **kw)


def vegas(eng, nblocks, npb, it=1):
    """(workgroups, threads, by cursor?) of one :vegas iteration"""
    eng.run("vegas", npb, 0, nblocks, iteration=it, seed=SEED)
    _, wgs, threads = eng.kernel_times_ms(1)
    return wgs, threads, eng.last_launch_cursor()[0]


def chains(eng, solver, nblocks, npb, it=0, nchain=0):
    """(workgroups, threads, chains per block, carried?, lanes per chain, accept levels) of one chain-solver iteration.  run + reduce, as
    the loop goes: on a context that holds a communicator (one that an earlier test of the process created stays) the :mcmc holding
    times reach the host behind the all-reduce and not behind the launch, and the next launch is sized from them either way"""
    eng.run(solver, npb, 0, nblocks, iteration=it, seed=SEED, nchain=nchain)
    eng.reduce()
    _, wgs, threads = eng.kernel_times_ms(1)
    return (wgs, threads) + eng.last_chain_launch() + eng.last_chain_speculation()


# ---- :vegas, x^2 + y^2 (2 draws): samples x draws around 2^19, samples around 2^22, one block and 16 ---------------------------------
def vegas_2d(nblocks, samples):
    def run(overrides):
        eng = x2y2()
        out = vegas(eng, nblocks, samples // nblocks)
        eng.close()
        return out
    return run


def vegas_2d_one_sample_short(nblocks, samples):
    """... one sample per block fewer: just below the threshold"""
    def run(overrides):
        eng = x2y2()
        out = vegas(eng, nblocks, samples // nblocks - 1)
        eng.close()
        return out
    return run


def vegas_2d_forced_wpb(overrides):
    eng = x2y2()
    eng.set_launch(0, 3)
    out = vegas(eng, 16, 2 ** 14)
    eng.close()
    return out


def vegas_2d_threads(overrides):
    eng = x2y2()
    eng.set_launch(128)
    out = vegas(eng, 16, 2 ** 14)
    eng.close()
    return out


def vegas_2d_deterministic(overrides):
    eng = x2y2(deterministic=True)
    out = vegas(eng, 16, 2 ** 14)
    eng.close()
    return out


def vegas_2d_integrate(overrides):
    """a launch-bound mci_integrate call through the launch chain: (ran as one persistent launch?, workgroups, threads).  (The persistent
    launch is switched off: in its automatic mode it is taken or not by what the kernel cache holds; tests/test_hip_persistent.py is
    about that launch)"""
    eng = x2y2()
    eng.set_persistent("off")
    eng.integrate("vegas", neval=10000, niter=3, block=16, seed=SEED)
    out = (eng.last_integrate_persistent(),) + tuple(eng.kernel_times_ms(1)[1:])
    eng.close()
    return out


# ---- :vegas, 16-D Gaussian: the fixed partition at 2^22, the cursor at 2^25 --------------------------------------------------------
def vegas_16d(log2, wpb=0, cursor=None):
    def run(overrides):
        if cursor is not None:
            overrides.set("vegas_cursor", cursor)
        eng = gauss16()
        if wpb:
            eng.set_launch(0, wpb)
        out = vegas(eng, 16, 2 ** (log2 - 4)) + (eng.last_launch_cursor()[1],)
        eng.close()
        return out
    return run


# ---- tiled :vegas: three 999-bin leaves in three tiles, 4 blocks x 2003 samples in 3 chunks of 668 ---------------------------------
def vegas_tiled(keep_tile0):
    def run(overrides):
        overrides.set("table_mode", 3)
        overrides.set("hist_tile_bins", 1000)
        overrides.set("split_chunk", 4 * 668)
        if keep_tile0:
            overrides.set("no_split_all", 1)
        cfg = mci.Configuration(var=mci.Continuous([(0.0, math.pi)] * 3), dof=[[1]], seed=SEED)
        eng = mci.Engine(cfg, mci.catalog.singular2())
        out = vegas(eng, 4, 2003) + eng.split_chunks()
        eng.close()
        return out
    return run


# ---- chain solvers (two integrands, dof [[2], [3]]) ---------------------------------------------------------------------------------
def chain_auto(solver, neval, nblocks):
    def run(overrides):
        eng = sphere2()
        out = chains(eng, solver, nblocks, neval // nblocks)
        eng.close()
        return out
    return run


def chain_explicit(solver):
    def run(overrides):
        eng = sphere2()
        out = chains(eng, solver, 16, 625, nchain=5)
        eng.close()
        return out
    return run


def chain_lanes(solver, lanes):
    def run(overrides):
        eng = sphere2()
        eng.set_chain_speculation(lanes)
        out = chains(eng, solver, 16, 625, nchain=1)
        eng.close()
        return out
    return run


def chain_carried(solver):
    """three consecutive iterations over the same blocks: the second and third continue the chains of the one before (and an :mcmc
    launch sizes its chains from the holds the one before it measured)"""
    def run(overrides):
        eng = sphere2()
        out = tuple(chains(eng, solver, 16, 62500, it=it) for it in range(3))
        eng.close()
        return out
    return run


# ---- host closures -----------------------------------------------------------------------------------------------------------------------
def vegas_host_integrand(overrides):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED)
    eng = mci.Engine(cfg, lambda x, c: x[0] * x[0] + x[1] * x[1])
    out = vegas(eng, 2, 150)
    eng.close()
    return out


def mcmc_host_measure(overrides):
    """the measure counts its records: blocks x chains x the measured-step window of a chain (BatchArgs::hm_first, hm_count)"""
    seen = []

    def m(x, obs, weights, config):
        seen.append(len(weights[0]))
        obs[0][0] += weights[0].sum()
    cfg = mci.Configuration(var=mci.Continuous([(0.0, math.pi)] * 3), dof=[[1]], seed=SEED)
    eng = mci.Engine(cfg, mci.catalog.singular2(), measure=m)
    eng.set_chain_speculation(1)
    out = chains(eng, "mcmc", 2, 300, nchain=4)
    eng.get_packed()
    eng.close()
    return out + (len(seen), int(np.sum(seen)))


CASES = {
    "vegas-2d-16blocks-below-2^19": vegas_2d_one_sample_short(16, 2 ** 18),
    "vegas-2d-16blocks-at-2^19": vegas_2d(16, 2 ** 18),
    "vegas-2d-1block-below-2^19": vegas_2d_one_sample_short(1, 2 ** 18),
    "vegas-2d-1block-at-2^19": vegas_2d(1, 2 ** 18),
    "vegas-2d-16blocks-below-2^22": vegas_2d_one_sample_short(16, 2 ** 22),
    "vegas-2d-16blocks-at-2^22": vegas_2d(16, 2 ** 22),
    "vegas-2d-1block-below-2^22": vegas_2d_one_sample_short(1, 2 ** 22),
    "vegas-2d-1block-at-2^22": vegas_2d(1, 2 ** 22),
    "vegas-2d-forced-wg-per-block": vegas_2d_forced_wpb,
    "vegas-2d-explicit-threads": vegas_2d_threads,
    "vegas-2d-deterministic": vegas_2d_deterministic,
    "vegas-2d-integrate-launch-chain": vegas_2d_integrate,
    "vegas-16d-2^22": vegas_16d(22),
    "vegas-16d-2^25": vegas_16d(25),
    "vegas-16d-2^25-forced-wg-per-block": vegas_16d(25, wpb=8),
    "vegas-16d-2^25-cursor-off": vegas_16d(25, cursor=0),
    "vegas-tiled-3-chunks": vegas_tiled(False),
    "vegas-tiled-3-chunks-keep-tile0": vegas_tiled(True),
    "vegas-host-integrand": vegas_host_integrand,
    "mcmc-host-measure": mcmc_host_measure,
}
for _solver in ("vegasmc", "mcmc"):
    for _neval in (10 ** 4, 10 ** 6):
        for _nb in (1, 16):
            CASES["%s-auto-1e%d-%dblocks" % (_solver, round(math.log10(_neval)), _nb)] = chain_auto(_solver, _neval, _nb)
    CASES["%s-explicit-nchain" % _solver] = chain_explicit(_solver)
    for _lanes in (1, 16, -1):
        CASES["%s-lanes-%s" % (_solver, "auto" if _lanes < 0 else _lanes)] = chain_lanes(_solver, _lanes)
    CASES["%s-three-iterations" % _solver] = chain_carried(_solver)

# recorded on an MI355X (256 CUs) at the commit before the split; see the module docstring
EXPECTED = {
    'mcmc-auto-1e4-16blocks': (16, 64, 1, False, 64, 3),
    'mcmc-auto-1e4-1blocks': (1, 128, 2, False, 64, 3),
    'mcmc-auto-1e6-16blocks': (64, 256, 15, False, 64, 3),
    'mcmc-auto-1e6-1blocks': (61, 256, 244, False, 64, 3),
    'mcmc-explicit-nchain': (32, 256, 5, False, 64, 3),
    'mcmc-host-measure': (2, 256, 4, False, 1, 0, 2, 608),
    'mcmc-lanes-1': (16, 256, 1, False, 1, 0),
    'mcmc-lanes-16': (16, 64, 1, False, 16, 3),
    'mcmc-lanes-auto': (16, 64, 1, False, 64, 3),
    'mcmc-three-iterations': ((64, 256, 15, False, 64, 3), (256, 256, 122, True, 32, 3), (256, 256, 122, True, 32, 3)),
    'vegas-16d-2^22': (2048, 512, False, 0),
    'vegas-16d-2^25': (512, 512, True, 2784),
    'vegas-16d-2^25-cursor-off': (2048, 512, False, 0),
    'vegas-16d-2^25-forced-wg-per-block': (128, 512, False, 0),
    'vegas-2d-16blocks-at-2^19': (256, 512, False),
    'vegas-2d-16blocks-at-2^22': (2048, 256, False),
    'vegas-2d-16blocks-below-2^19': (64, 256, False),
    'vegas-2d-16blocks-below-2^22': (256, 512, False),
    'vegas-2d-1block-at-2^19': (256, 512, False),
    'vegas-2d-1block-at-2^22': (2048, 256, False),
    'vegas-2d-1block-below-2^19': (64, 256, False),
    'vegas-2d-1block-below-2^22': (256, 512, False),
    'vegas-2d-deterministic': (256, 512, False),
    'vegas-2d-explicit-threads': (256, 128, False),
    'vegas-2d-forced-wg-per-block': (48, 256, False),
    'vegas-2d-integrate-launch-chain': (False, 48, 256),
    'vegas-host-integrand': (2, 256, False),
    'vegas-tiled-3-chunks': (32, 256, False, 3, 32064),
    'vegas-tiled-3-chunks-keep-tile0': (32, 256, False, 3, 32064),
    'vegasmc-auto-1e4-16blocks': (16, 64, 1, False, 64, 12),
    'vegasmc-auto-1e4-1blocks': (2, 256, 6, False, 64, 12),
    'vegasmc-auto-1e6-16blocks': (160, 256, 40, False, 64, 12),
    'vegasmc-auto-1e6-1blocks': (163, 256, 651, False, 64, 12),
    'vegasmc-explicit-nchain': (32, 256, 5, False, 64, 12),
    'vegasmc-lanes-1': (16, 256, 1, False, 1, 0),
    'vegasmc-lanes-16': (16, 64, 1, False, 16, 12),
    'vegasmc-lanes-auto': (16, 64, 1, False, 64, 12),
    'vegasmc-three-iterations': ((160, 256, 40, False, 64, 12), (176, 256, 162, True, 16, 12), (176, 256, 162, True, 16, 12)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_geometry(case, overrides):
    got = CASES[case](overrides)
    print("\nPLAN %r: %r," % (case, got))
    assert got == EXPECTED[case]
