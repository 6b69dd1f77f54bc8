"""CPU tests of :vegasmc parameter sweeps (mci_integrate_sweep_chains, csrc/mci_sweep_chains.h): the fourth sweep unit cross-compiled for
gfx950 through the library's own JIT into a code object of its own, what mci_sweep_chains_supported refuses and by which name, the
Python argument errors of mci.integrate_sweep(..., chains=K), and that without chains= a chain solver loops and warns as before."""
import os
import re
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import isa_mix
from test_sweep_leaves_host import bubble, discrete, gauss4, offline, one_leaf, two_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("mci_vegas_sweep", "mci_vegas_sweep_leaves", "mci_vegas_sweep_strat")


def sphere2():
    return offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2())


def test_the_unit_compiles_to_a_code_object_of_its_own():
    eng = bubble()
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object("vegasmc_sweep")
    eng.compile("vegasmc_sweep")
    path = eng.code_object("vegasmc_sweep")
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and b"mci_vegasmc_sweep\0" in blob
    for other in OTHERS + ("mci_vegasmc_chains", "mci_vegas_batch"):
        assert other.encode() + b"\0" not in blob, other
    for other in ("vegas_sweep", "vegas_sweep_leaves", "vegas_sweep_strat", "vegasmc", "vegas"):
        with pytest.raises(mci.MCIError):
            eng.code_object(other)                  # compiling this unit compiles no other
    eng.compile("vegasmc_sweep")                    # again: the same file
    assert eng.code_object("vegasmc_sweep") == path
    res = isa_mix.resources(path)["mci_vegasmc_sweep"]
    assert res["scratch"] == 0 and res["lds"] == 0 and res["vgpr_spill"] == 0     # (compile_sweep_unit's rule: no scratch, no static LDS)
    for make in (sphere2, discrete, gauss4, one_leaf):     # the other layouts of the GPU tests, each a code object of its own
        e2 = make()
        e2.compile("vegasmc_sweep")
        assert e2.code_object("vegasmc_sweep") != path
    # the opt-in of the :vegas sweeps has no say here, and this unit none there
    eng.set_sweep_leaves("all")
    eng.compile("vegasmc_sweep")
    assert eng.code_object("vegasmc_sweep") == path


def test_the_sweep_header_goes_through_the_common_one():
    csrc = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
    text = open(os.path.join(csrc, "mci_sweep_chains.h")).read()
    assert '#include "mci_sweep_common.h"' in text and '#include "mci_sweep_leaves.h"' not in text
    assert "__hip_atomic_load(" not in text and "s_waitcnt" not in text and "atomicAdd" not in text
    assert "sweep_round_trip();" in text and "sweep_take_hist(" in text
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '("kSweepChainsHeader", "mci_sweep_chains.h")' in entry


def test_sweep_chains_supported_names_each_refusal():
    eng = bubble()
    assert eng.sweep_chains_supported() is None and eng.sweep_chains_supported(nchain=300, neval=16 * 1500) is None
    assert eng.sweep_chains_supported(solver="vegas") == "solver is not :vegasmc (mci_integrate_sweep runs :vegas)"
    assert "a follow-up" in eng.sweep_chains_supported(solver="mcmc") and ":mcmc" in eng.sweep_chains_supported(solver="mcmc")
    assert "nchain = 0" in eng.sweep_chains_supported(nchain=0) and "automatic" in eng.sweep_chains_supported(nchain=0)
    assert eng.sweep_chains_supported(nchain=626, neval=10000, block=16) == "nchain = 626 exceeds the 625 steps of a block"
    assert eng.sweep_chains_supported(nchain=625, neval=10000, block=16) is None
    assert "measurefreq = 2" in eng.sweep_chains_supported(measurefreq=2)
    # a chain's streams are keyed by (block < 4096, iteration < 131072), as in the ordinary chain launch: beyond them blocks would repeat
    assert eng.sweep_chains_supported(neval=4096 * 4, block=4096) is None
    assert eng.sweep_chains_supported(neval=8192 * 4, block=8192) == "block = 8192 (chain solvers address a chain by block < 4096)"
    assert eng.sweep_chains_supported(niter=10, first_iteration=131062) is None
    assert "first_iteration = 131063, niter = 10" in eng.sweep_chains_supported(niter=10, first_iteration=131063)
    assert "0 <= iteration < 131072" in eng.sweep_chains_supported(first_iteration=-1)
    assert "niter < 1" in eng.sweep_chains_supported(niter=0)
    eng.set_reweight_goal([1.0, 2.0])
    assert "a reweight goal" in eng.sweep_chains_supported()
    eng.set_reweight_goal(None)
    assert eng.sweep_chains_supported() is None
    fk = offline(mci.Configuration(var=(mci.FermiK(3, 1.0, 0.5, 10.0), mci.Continuous(0.0, 1.0)), dof=[[1, 1]]),
                 mci.Integrand("w[0] = x[0] * x[0] + x[3];", None, "fermik"))
    assert "FermiK" in fk.sweep_chains_supported()
    det = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]]), mci.catalog.x2y2(), deterministic=True)
    assert "deterministic" in det.sweep_chains_supported()
    strat = two_leaves()
    strat.set_stratification(4)
    assert "stratified" in strat.sweep_chains_supported()
    strat.set_stratification(on=False)
    assert strat.sweep_chains_supported() is None
    host = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]]), mci.HostIntegrand(lambda x: x[0]))
    assert "a host integrand" in host.sweep_chains_supported()
    big = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 24), dof=[[1]]), mci.catalog.gaussian(24))
    m = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", big.sweep_chains_supported())
    assert m and int(m.group(1)) > 24 * 1000 * 8 > int(m.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="bytes of LDS"):
        big.compile("vegasmc_sweep")
    with pytest.raises(mci.MCIError, match="cannot run as a sweep of :vegasmc points: .*FermiK"):
        fk.compile("vegasmc_sweep")


def test_the_vegas_queries_still_refuse_chain_solvers():
    for make in (bubble, one_leaf, sphere2):
        eng = make()
        assert eng.sweep_supported(solver="vegasmc") == "solver is not :vegas (chain solvers are not swept)"
        assert eng.sweep_supported(solver="mcmc") == "solver is not :vegas (chain solvers are not swept)"
    eng = one_leaf()
    eng.set_stratification()
    assert ":vegas" in eng.sweep_strat_supported(solver="vegasmc")


def test_the_two_exports_and_the_units_name():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGASMC_SWEEP = 11 \};", hdr)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_integrate_sweep_chains\(", hdr, re.S)
    assert m
    for needle in ("vegas_mc/montecarlo.jl:112-241", "main.jl:183", ":322-346", "reweight_in", "reweight_out", "pa_out", "nchain >= 1"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_chains_supported\(", hdr, re.S)
    assert m and ":mcmc" in m.group(1) and "FermiK" in m.group(1) and "159 KiB" in m.group(1)


def test_engine_integrate_sweep_chains_validates_its_arrays():
    eng = bubble()
    nud = len(eng.integrand.userdata)
    ud = np.ones((2, nud))
    with pytest.raises(ValueError, match=r"reweight must be \[points = 2\]\[integrands \+ 1 = 2\]"):
        eng.integrate_sweep_chains(userdata=ud, reweight=np.ones((2, 3)))
    with pytest.raises(ValueError, match=r"maps must be \[points = 2\]\[grid points = 4009\]"):
        eng.integrate_sweep_chains(userdata=ud, maps=np.zeros((2, 4000)))
    with pytest.raises(ValueError, match="one seed per point"):
        eng.integrate_sweep_chains(userdata=ud, seeds=[1, 2, 3])
    with pytest.raises(mci.MCIError, match="nchain = 0"):
        eng.integrate_sweep_chains(userdata=ud, nchain=0)
    with pytest.raises(mci.MCIError, match=":vegasmc"):
        eng.integrate_sweep_chains("vegas", userdata=ud)
    with pytest.raises(mci.MCIError) as e:          # eligible: only the device is missing
        eng.integrate_sweep_chains(userdata=ud, nchain=4)
    assert e.value.code == 7


def test_integrate_sweep_argument_errors():
    f = mci.catalog.sphere2()
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)    # (variable objects per call: a bound one belongs to its engine)
    rows = np.zeros((2, 0))
    for bad in (0, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="chains must be an int >= 1"):
            mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=bad, **kw())
    with pytest.raises(ValueError, match='chains= belongs to solver="vegasmc".*swept without it'):
        mci.integrate_sweep(f, params=rows, solver="vegas", chains=4, **kw())
    with pytest.raises(ValueError, match='chains= belongs to solver="vegasmc".*follow-up'):
        mci.integrate_sweep(f, params=rows, solver="mcmc", chains=4, **kw())
    with pytest.raises(ValueError, match="chains= and stratify="):
        mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, stratify=True, **kw())
    with pytest.raises(ValueError, match="reweight= belongs to a chain sweep"):
        mci.integrate_sweep(f, params=rows, solver="vegasmc", reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
    with pytest.raises(ValueError, match=r"one vector per point \(2\), got 1"):
        mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, reweight=[[0.3, 0.3, 0.4]], **kw())
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # eligible: no warning, no loop; only the device is missing
        with pytest.raises(mci.MCIError) as e:
            mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, **kw())
        assert e.value.code == 7
        # refused (measurefreq): reweight= needs the batched form, said before anything warns
        with pytest.raises(ValueError, match=r"measurefreq = 2.*reweight= needs the batched form"):
            mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, measurefreq=2, reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
    # ... and without reweight= the refused chain sweep loops with the usual warning
    with pytest.warns(RuntimeWarning, match=r"does not run as a sweep \(measurefreq = 2.*2 ordinary integrate\(\) calls"):
        with pytest.raises(mci.MCIError) as e:
            mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, measurefreq=2, **kw())
    assert e.value.code == 7


def test_without_chains_a_chain_solver_loops_and_warns_as_before():
    f = mci.catalog.sphere2()
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)    # (variable objects per call: a bound one belongs to its engine)
    for solver in ("vegasmc", "mcmc"):
        with pytest.warns(RuntimeWarning) as rec:
            with pytest.raises(mci.MCIError) as e:  # (the first ordinary call finds no device)
                mci.integrate_sweep(f, params=np.zeros((3, 0)), solver=solver, **kw())
        assert e.value.code == 7
        said = [str(w.message) for w in rec if "sweep" in str(w.message)]
        assert said == ["integrate_sweep: this problem does not run as a sweep (solver is not :vegas (chain solvers are not swept)): "
                        "3 ordinary integrate() calls, one after another"]
