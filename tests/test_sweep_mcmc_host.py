"""CPU tests of :mcmc parameter sweeps (mci_integrate_sweep_mcmc, csrc/mci_sweep_chains.h mcmc_sweep): the fifth sweep unit cross-compiled
for gfx950 through the library's own JIT into a code object of its own, what mci_sweep_mcmc_supported refuses and by which name, the
Python argument errors of mci.integrate_sweep(..., solver="mcmc", mcmc_chains=K), and that without mcmc_chains= an :mcmc scan loops and
warns as before."""
import io
import os
import re
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import isa_mix
from test_sweep_leaves_host import bubble, discrete, offline, two_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("mci_vegas_sweep", "mci_vegas_sweep_leaves", "mci_vegas_sweep_strat", "mci_vegasmc_sweep")


def sphere2():
    return offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2())


def test_the_unit_compiles_to_a_code_object_of_its_own():
    eng = bubble()
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object("mcmc_sweep")
    eng.compile("mcmc_sweep")
    path = eng.code_object("mcmc_sweep")
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and b"mci_mcmc_sweep\0" in blob
    for other in OTHERS + ("mci_mcmc_chains", "mci_vegasmc_chains", "mci_vegas_batch"):
        assert other.encode() + b"\0" not in blob, other
    for other in ("vegas_sweep", "vegas_sweep_leaves", "vegas_sweep_strat", "vegasmc_sweep", "mcmc", "vegasmc", "vegas"):
        with pytest.raises(mci.MCIError):
            eng.code_object(other)                  # compiling this unit compiles no other
    eng.compile("mcmc_sweep")                       # again: the same file
    assert eng.code_object("mcmc_sweep") == path
    res = isa_mix.resources(path)["mci_mcmc_sweep"]
    print("mci_mcmc_sweep, bubble:", res)
    assert res["scratch"] == 0 and res["lds"] == 0 and res["vgpr_spill"] == 0     # (compile_sweep_unit's rule: no scratch, no static LDS)
    assert res["max_threads"] == 256 and res["vgpr"] <= 512
    eng.compile("vegasmc_sweep")                    # the same header's other instantiation: another kernel in another object
    assert eng.code_object("vegasmc_sweep") != path
    assert b"mci_mcmc_sweep\0" not in open(eng.code_object("vegasmc_sweep"), "rb").read()
    for make in (sphere2, discrete):                # the other layouts of the GPU tests, each a code object of its own
        e2 = make()
        e2.compile("mcmc_sweep")
        assert e2.code_object("mcmc_sweep") != path
    eng.set_sweep_leaves("all")                     # the opt-in of the :vegas sweeps has no say here
    eng.compile("mcmc_sweep")
    assert eng.code_object("mcmc_sweep") == path


def test_one_header_two_instantiations():
    csrc = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
    text = open(os.path.join(csrc, "mci_sweep_chains.h")).read()
    assert "if constexpr (MCMC) mcmc_chains<Cfg>(a); else vegasmc_chains<Cfg>(a);" in text
    assert text.count("chain_sweep<Cfg, false>(a0, fc)") == 1 and text.count("chain_sweep<Cfg, true>(a0, fc)") == 1
    assert "__hip_atomic_load(" not in text and "atomicAdd" not in text
    assert "sweep_round_trip();" in text and "sweep_take_hist(" in text
    head = text[:text.index("#pragma once")]
    assert "the round trip of the first leaf's histogram slice stands in between" in head and "mcmc_chains" in head
    jit = open(os.path.join(csrc, "mci_jit.h")).read()
    assert re.search(r'kUnitSweepMcmc\s*\*/ \{"mci_sweep_chains.h",.*"mci_mcmc_sweep", "SweepChainArgs", "f", "mcmc_sweep", -1, false, 2, true, false, true\}', jit)


def test_sweep_mcmc_supported_names_each_refusal():
    eng = bubble()
    assert eng.sweep_mcmc_supported() is None and eng.sweep_mcmc_supported(nchain=300, neval=16 * 1500) is None
    assert eng.sweep_mcmc_supported(solver="vegas") == "solver is not :mcmc (mci_integrate_sweep runs :vegas, mci_integrate_sweep_chains :vegasmc)"
    assert eng.sweep_mcmc_supported(solver="vegasmc") == eng.sweep_mcmc_supported(solver="vegas")
    assert eng.sweep_mcmc_supported(nchain=0) == eng.sweep_chains_supported(nchain=0) and "automatic" in eng.sweep_mcmc_supported(nchain=0)
    assert eng.sweep_mcmc_supported(nchain=-2) == "nchain < 0"
    assert eng.sweep_mcmc_supported(nchain=626, neval=10000, block=16) == "nchain = 626 exceeds the 625 steps of a block"
    assert eng.sweep_mcmc_supported(nchain=625, neval=10000, block=16) is None
    assert eng.sweep_mcmc_supported(neval=4096 * 4, block=4096) is None
    assert eng.sweep_mcmc_supported(neval=8192 * 4, block=8192) == "block = 8192 (chain solvers address a chain by block < 4096)"
    assert eng.sweep_mcmc_supported(niter=10, first_iteration=131062) is None
    assert "first_iteration = 131063, niter = 10" in eng.sweep_mcmc_supported(niter=10, first_iteration=131063)
    assert "0 <= iteration < 131072" in eng.sweep_mcmc_supported(first_iteration=-1)
    assert "niter < 1" in eng.sweep_mcmc_supported(niter=0)
    assert eng.sweep_mcmc_supported(thermal_ratio=0.0) is None
    for bad in (-0.1, float("nan"), float("inf")):
        assert "thermal_ratio = " in eng.sweep_mcmc_supported(thermal_ratio=bad) and "finite and >= 0" in eng.sweep_mcmc_supported(thermal_ratio=bad)
    # steps + nburn of a chain stay below 2^31 - 1: 2^31 / 1.1 steps and a tenth of them burnt in is past it, a little fewer is not
    assert eng.sweep_mcmc_supported(neval=1900000000, block=1) is None
    m = re.match(r"steps \+ nburn = (\d+) \+ (\d+) per chain", eng.sweep_mcmc_supported(neval=1960000000, block=1))
    assert m and int(m.group(1)) == 1960000000 and int(m.group(1)) + int(m.group(2)) >= 2 ** 31 - 1
    assert "steps + nburn" in eng.sweep_mcmc_supported(neval=10 ** 9, block=1, thermal_ratio=1.2)
    assert "steps + nburn" in eng.sweep_mcmc_supported(neval=10 ** 9, block=1, thermal_ratio=1e300)
    assert "measurefreq = 2" in eng.sweep_mcmc_supported(measurefreq=2)
    eng.set_reweight_goal([1.0, 2.0])
    assert "a reweight goal" in eng.sweep_mcmc_supported()
    eng.set_reweight_goal(None)
    assert eng.sweep_mcmc_supported() is None
    fk = offline(mci.Configuration(var=(mci.FermiK(3, 1.0, 0.5, 10.0), mci.Continuous(0.0, 1.0)), dof=[[1, 1]]),
                 mci.Integrand("w[0] = x[0] * x[0] + x[3];", None, "fermik"))
    assert "FermiK" in fk.sweep_mcmc_supported() and "a follow-up" in fk.sweep_mcmc_supported() and "vegas doesn't" not in fk.sweep_mcmc_supported()
    det = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]]), mci.catalog.x2y2(), deterministic=True)
    assert "deterministic" in det.sweep_mcmc_supported()
    strat = two_leaves()
    strat.set_stratification(4)
    assert "stratified" in strat.sweep_mcmc_supported()
    strat.set_stratification(on=False)
    assert strat.sweep_mcmc_supported() is None
    host = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]]), mci.HostIntegrand(lambda x: x[0]))
    assert "a host integrand" in host.sweep_mcmc_supported()
    big = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 24), dof=[[1]]), mci.catalog.gaussian(24))
    m = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", big.sweep_mcmc_supported())
    assert m and int(m.group(1)) > 24 * 1000 * 8 > int(m.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="bytes of LDS"):
        big.compile("mcmc_sweep")
    with pytest.raises(mci.MCIError, match="cannot run as a sweep of :mcmc points: .*FermiK"):
        fk.compile("mcmc_sweep")


def test_the_older_queries_keep_their_strings():
    for make in (bubble, sphere2):
        eng = make()
        assert eng.sweep_supported(solver="mcmc") == "solver is not :vegas (chain solvers are not swept)"
        assert eng.sweep_chains_supported(solver="mcmc") == "solver is :mcmc (a sweep of :mcmc points is a follow-up)"
        assert eng.sweep_chains_supported() is None


def test_the_two_exports_and_the_units_name():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_MCMC_SWEEP = 12 \};", hdr)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_integrate_sweep_mcmc\(", hdr, re.S)
    assert m
    for needle in ("mcmc/montecarlo.jl:72-187", "mcmc/updates.jl", "main.jl:183", ":322-346", "holds_out", "mci_mcmc_burnin", "10000"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_mcmc_supported\(", hdr, re.S)
    assert m
    for needle in ("mcmc/montecarlo.jl:72-187", "mcmc/updates.jl", "main.jl:183", ":322-346", "FermiK", "a follow-up", "159 KiB", "thermal_ratio", "2^31 - 1"):
        assert needle in m.group(1), needle
    # next to both older queries: which entry point runs :mcmc points
    for fn in ("mci_sweep_supported", "mci_sweep_chains_supported"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % fn, hdr, re.S)
        assert m and "mci_integrate_sweep_mcmc runs :mcmc" in " ".join(m.group(1).replace("*", " ").split()), fn


def test_engine_integrate_sweep_mcmc_validates_its_arrays():
    eng = bubble()
    nud = len(eng.integrand.userdata)
    ud = np.ones((2, nud))
    with pytest.raises(ValueError, match=r"integrate_sweep_mcmc: reweight must be \[points = 2\]\[integrands \+ 1 = 2\]"):
        eng.integrate_sweep_mcmc(userdata=ud, reweight=np.ones((2, 3)))
    with pytest.raises(ValueError, match=r"integrate_sweep_mcmc: maps must be \[points = 2\]\[grid points = 4009\]"):
        eng.integrate_sweep_mcmc(userdata=ud, maps=np.zeros((2, 4000)))
    with pytest.raises(ValueError, match="one seed per point"):
        eng.integrate_sweep_mcmc(userdata=ud, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match=r"userdata must be a 2-D array"):
        eng.integrate_sweep_mcmc(userdata=np.ones((2, nud + 1)))
    with pytest.raises(mci.MCIError, match="nchain = 0"):
        eng.integrate_sweep_mcmc(userdata=ud, nchain=0)
    with pytest.raises(mci.MCIError, match="thermal_ratio"):
        eng.integrate_sweep_mcmc(userdata=ud, thermal_ratio=-1.0)
    with pytest.raises(mci.MCIError, match="solver is not :mcmc"):
        eng.integrate_sweep_mcmc("vegasmc", userdata=ud)
    with pytest.raises(mci.MCIError) as e:          # eligible: only the device is missing
        eng.integrate_sweep_mcmc(userdata=ud, nchain=4)
    assert e.value.code == 7
    assert mci.Engine.hold_max_of(np.zeros(64)) == 0 and mci.Engine.hold_max_of([3, 0, 1] + [0] * 61) == 3
    assert mci.Engine.hold_max_of([0] * 63 + [1]) == 2 ** 63 - 1


def test_integrate_sweep_argument_errors():
    f = mci.catalog.sphere2()
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)    # (variable objects per call: a bound one belongs to its engine)
    rows = np.zeros((2, 0))
    for bad in (0, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="mcmc_chains must be an int >= 1"):
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=bad, **kw())
    with pytest.raises(ValueError, match='mcmc_chains= belongs to solver="mcmc".*swept without it'):
        mci.integrate_sweep(f, params=rows, solver="vegas", mcmc_chains=4, **kw())
    with pytest.raises(ValueError, match='mcmc_chains= belongs to solver="mcmc".*takes chains='):
        mci.integrate_sweep(f, params=rows, solver="vegasmc", mcmc_chains=4, **kw())
    with pytest.raises(ValueError, match="chains= .* and mcmc_chains= .* do not go together"):
        mci.integrate_sweep(f, params=rows, solver="mcmc", chains=4, mcmc_chains=4, **kw())
    with pytest.raises(ValueError, match='chains= belongs to solver="vegasmc".*follow-up'):     # (the older keyword keeps its pinned error)
        mci.integrate_sweep(f, params=rows, solver="mcmc", chains=4, **kw())
    with pytest.raises(ValueError, match="mcmc_chains= and stratify="):
        mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, stratify=True, **kw())
    with pytest.raises(ValueError, match="reweight= belongs to a chain sweep"):
        mci.integrate_sweep(f, params=rows, solver="mcmc", reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
    with pytest.raises(ValueError, match=r"one vector per point \(2\), got 1"):
        mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, reweight=[[0.3, 0.3, 0.4]], **kw())
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # eligible: no warning, no loop; only the device is missing
        with pytest.raises(mci.MCIError) as e:
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
        assert e.value.code == 7
        # refused (measurefreq, thermal_ratio): reweight= needs the batched form, said before anything warns
        with pytest.raises(ValueError, match=r"measurefreq = 2.*reweight= needs the batched form"):
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, measurefreq=2, reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
        with pytest.raises(ValueError, match=r"thermal_ratio = .*reweight= needs the batched form"):
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, thermal_ratio=-0.5, reweight=[[0.3, 0.3, 0.4]] * 2, **kw())
    # ... and without reweight= the refused sweep loops with the usual single warning
    with pytest.warns(RuntimeWarning) as rec:
        with pytest.raises(mci.MCIError) as e:      # (the first ordinary call finds no device)
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, measurefreq=2, **kw())
    assert e.value.code == 7
    said = [str(w.message) for w in rec if "sweep" in str(w.message)]
    assert said == ["integrate_sweep: this problem does not run as a sweep (measurefreq = 2 (a sweep measures every sample)): "
                    "2 ordinary integrate() calls, one after another"]


def test_without_mcmc_chains_an_mcmc_scan_loops_and_warns_as_before():
    f = mci.catalog.sphere2()
    with pytest.warns(RuntimeWarning) as rec:
        with pytest.raises(mci.MCIError) as e:      # (the first ordinary call finds no device)
            mci.integrate_sweep(f, params=np.zeros((3, 0)), solver="mcmc", var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)
    assert e.value.code == 7
    said = [str(w.message) for w in rec if "sweep" in str(w.message)]
    assert said == ["integrate_sweep: this problem does not run as a sweep (solver is not :vegas (chain solvers are not swept)): "
                    "3 ordinary integrate() calls, one after another"]


def test_the_report_note_follows_the_holds():
    """Result.hold_note / report(): 16 x the longest hold against the measured steps of a chain (mci_mcmc_launch_valid's rule)"""
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]])
    res = mci.Result(np.array([[1.0], [1.1]]), np.array([[0.1], [0.1]]), cfg, 0)
    assert res.holds is None and res.hold_max is None and res.hold_note is None
    holds = np.zeros(64, dtype=np.uint64)
    holds[5], holds[6] = 2, 1
    res.holds, res.hold_max, res.chain_steps = holds, mci.Engine.hold_max_of(holds), 600
    assert res.hold_max == 63 and "63 steps" in res.hold_note and "600 steps" in res.hold_note and "1008" in res.hold_note
    out = io.StringIO()
    mci.report(res, io=out)
    assert out.getvalue().count("note: some chain of this :mcmc sweep point") == 1
    res.chain_steps = 1008                          # 16 x 63: long enough
    assert res.hold_note is None
    out = io.StringIO()
    mci.report(res, io=out)
    assert ":mcmc sweep point" not in out.getvalue()
    assert res.with_ignore(1).hold_max == 63
