"""CPU tests of carried chains in the chain solvers' sweeps (mci_set_sweep_chain_carry; csrc/mci_sweep_chains.h chain_sweep<Cfg, MCMC, true>):
the two new units cross-compiled for gfx950 through the library's own JIT into code objects of their own, the setter and its default, what
include/mci.h says next to it, the Python keyword errors of mci.integrate_sweep(..., carry=True), and the factor of report()'s hold note."""
import io
import os
import re

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import isa_mix
from test_sweep_leaves_host import bubble, discrete, offline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("mci_vegas_sweep", "mci_vegas_sweep_leaves", "mci_vegas_sweep_strat", "mci_vegasmc_sweep", "mci_mcmc_sweep", "mci_vegasmc_sweep_carry",
           "mci_mcmc_sweep_carry", "mci_mcmc_chains", "mci_vegasmc_chains", "mci_vegas_batch", "mci_vegasmc_carry_weights")
UNITS = ("vegas_sweep", "vegas_sweep_leaves", "vegas_sweep_strat", "vegasmc_sweep", "mcmc_sweep", "vegasmc_sweep_carry", "mcmc_sweep_carry", "mcmc", "vegasmc", "vegas")


def sphere2():
    return offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2())


@pytest.mark.parametrize("unit", ["vegasmc_sweep_carry", "mcmc_sweep_carry"])
def test_the_carried_unit_compiles_to_a_code_object_of_its_own(unit):
    kernel = "mci_" + unit
    eng = bubble()
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object(unit)
    eng.compile(unit)
    path = eng.code_object(unit)
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and kernel.encode() + b"\0" in blob
    for other in KERNELS:
        if other != kernel:
            assert other.encode() + b"\0" not in blob, other
    for other in UNITS:
        if other != unit:
            with pytest.raises(mci.MCIError):
                eng.code_object(other)              # compiling this unit compiles no other
    eng.compile(unit)                               # again: the same file
    assert eng.code_object(unit) == path
    res = isa_mix.resources(path)[kernel]
    print(kernel, "bubble:", res)
    assert res["scratch"] == 0 and res["lds"] == 0 and res["vgpr_spill"] == 0     # (compile_sweep_unit's rule: no scratch, no static LDS)
    assert res["max_threads"] == 256 and res["vgpr"] <= 512
    plain = unit[:-len("_carry")]
    eng.compile(plain)                              # the uncarried unit: another kernel in another object
    assert eng.code_object(plain) != path and kernel.encode() + b"\0" not in open(eng.code_object(plain), "rb").read()
    for make in (sphere2, discrete):                # the other layouts of the GPU tests, each a code object of its own
        e2 = make()
        e2.compile(unit)
        r2 = isa_mix.resources(e2.code_object(unit))[kernel]
        assert e2.code_object(unit) != path and r2["scratch"] == 0 and r2["lds"] == 0 and r2["vgpr_spill"] == 0 and r2["max_threads"] == 256


def test_one_header_four_instantiations_and_one_resampler():
    csrc = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
    text = open(os.path.join(csrc, "mci_sweep_chains.h")).read()
    assert text.count("chain_sweep<Cfg, false, true>(a0, f.c, &f.k)") == 1 and text.count("chain_sweep<Cfg, true, true>(a0, f.c, &f.k)") == 1
    assert text.count("resample_block(") >= 1 and "vegasmc_carry_weight<Cfg>(" in text
    head = text[:text.index("#pragma once")]
    assert "The first iteration\n// of every call starts afresh: chain state does not travel between calls." in head
    static = open(os.path.join(csrc, "mci_static_kernels.h")).read()
    body = static[static.index("k_resample_chains(ResampleArgs a) {"):]
    body = body[:body.index("\n}\n")]
    assert "resample_block(a, (long long)blockIdx.x, scratch, kLdsW);" in body and "for (" not in body     # the kernel is a call to the shared body
    device = open(os.path.join(csrc, "mci_device.h")).read()
    assert device.count("vegasmc_carry_weight<Cfg>(a, t, rw, j)") == 1                                      # ... and so is the grid-strided weights loop
    jit = open(os.path.join(csrc, "mci_jit.h")).read()
    assert re.search(r'kUnitSweepChainsCarry\s*\*/ \{"mci_sweep_chains.h",.*"mci_vegasmc_sweep_carry", "SweepChainCarryArgs", "f", "vegasmc_sweep_carry", -1, false, 2, true, false, true\}', jit)
    assert re.search(r'kUnitSweepMcmcCarry\s*\*/ \{"mci_sweep_chains.h",.*"mci_mcmc_sweep_carry", "SweepChainCarryArgs", "f", "mcmc_sweep_carry", -1, false, 2, true, false, true\}', jit)


def test_the_setter_defaults_to_off_and_adds_no_refusal():
    eng = bubble()
    assert eng.sweep_chain_carry() is False
    before = [eng.sweep_chains_supported(), eng.sweep_mcmc_supported(), eng.sweep_chains_supported(solver="mcmc"), eng.sweep_mcmc_supported(nchain=0),
              eng.sweep_chains_supported(nchain=626, neval=10000, block=16)]
    eng.set_sweep_chain_carry(True)
    assert eng.sweep_chain_carry() is True
    assert [eng.sweep_chains_supported(), eng.sweep_mcmc_supported(), eng.sweep_chains_supported(solver="mcmc"), eng.sweep_mcmc_supported(nchain=0),
            eng.sweep_chains_supported(nchain=626, neval=10000, block=16)] == before
    eng.set_sweep_chain_carry(False)
    assert eng.sweep_chain_carry() is False
    assert mci.lib().mci_set_sweep_chain_carry(eng.p, 2) != 0 and b"sweep chain carry" in mci.lib().mci_last_error()
    # eligible with the setting on: only the device is missing
    ud = np.ones((2, len(eng.integrand.userdata)))
    for call in (eng.integrate_sweep_chains, eng.integrate_sweep_mcmc):
        with pytest.raises(mci.MCIError) as e:
            call(userdata=ud, nchain=4, carry=True)
        assert e.value.code == 7
        assert eng.sweep_chain_carry() is False     # carry=True is the call's: the engine's own setting is back


def test_the_header_documents_the_setter_and_the_two_units():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGASMC_SWEEP_CARRY = 13, MCI_MCMC_SWEEP_CARRY = 14 \};", hdr)
    assert hdr.index("int mci_set_sweep_leaves(") < hdr.index("int mci_set_sweep_chain_carry(") < hdr.index("int mci_get_sweep_chain_carry(") < hdr.index("int mci_sweep_map_doubles(")
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_set_sweep_chain_carry\(", hdr, re.S)
    assert m
    said = " ".join(m.group(1).replace("*", " ").split())
    for needle in ("mci_set_chain_carry", "mci_integrate_sweep_chains", "mci_integrate_sweep_mcmc", "reweight_now[curr] / reweight_used[curr]", "pi_new / pi_old",
                   "nburn = 0", "mci_chain_burnin(steps, 1, nslots)", "chain state does not travel between calls", "mci_lineage_sums", "correlated = 1",
                   "MCI_VEGASMC_SWEEP_CARRY", "4 GiB", "adds no refusal"):
        assert needle in said, needle
    for fn in ("mci_integrate_sweep_chains", "mci_integrate_sweep_mcmc"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % fn, hdr, re.S)
        assert m and "mci_set_sweep_chain_carry" in m.group(1), fn


def test_integrate_sweep_carry_argument_errors():
    f = mci.catalog.sphere2()
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)    # (variable objects per call: a bound one belongs to its engine)
    rows = np.zeros((2, 0))
    for solver in ("vegasmc", "mcmc"):
        with pytest.raises(ValueError, match=r"carry= belongs to a chain sweep: give chains=K .* or mcmc_chains=K"):
            mci.integrate_sweep(f, params=rows, solver=solver, carry=True, **kw())
    with pytest.raises(ValueError, match='carry= belongs to a chain sweep .*"vegas" has no chains'):
        mci.integrate_sweep(f, params=rows, solver="vegas", carry=True, **kw())
    with pytest.raises(ValueError, match="carry= and stratify= do not go together"):
        mci.integrate_sweep(f, params=rows, solver="vegasmc", chains=4, carry=True, stratify=True, **kw())
    with pytest.raises(ValueError, match="carry= and stratify= do not go together"):
        mci.integrate_sweep(f, params=rows, solver="vegas", carry=True, stratify=True, **kw())
    for bad in (1.5, "yes", None, 2):
        with pytest.raises(ValueError, match="carry must be True or False"):
            mci.integrate_sweep(f, params=rows, solver="mcmc", mcmc_chains=4, carry=bad, **kw())
    for extra in (dict(solver="vegasmc", chains=4), dict(solver="mcmc", mcmc_chains=4)):
        with pytest.raises(mci.MCIError) as e:      # eligible: only the device is missing
            mci.integrate_sweep(f, params=rows, carry=True, **extra, **kw())
        assert e.value.code == 7


def test_the_report_note_of_a_carried_point_asks_for_four_holds():
    """Result.hold_note: 4 x the longest hold against the measured steps of a chain where the iterations were carried (plan_mcmc_chains'
    factor for chains that start stationary), 16 x otherwise"""
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]])
    res = mci.Result(np.array([[1.0], [1.1]]), np.array([[0.1], [0.1]]), cfg, 0)
    assert res.chains_carried is False
    holds = np.zeros(64, dtype=np.uint64)
    holds[6] = 1
    res.holds, res.hold_max, res.chain_steps = holds, mci.Engine.hold_max_of(holds), 600
    assert res.hold_max == 63 and "fresh chains want at least 16 x" in res.hold_note and "1008" in res.hold_note
    res.chains_carried = True                        # 4 x 63 = 252 <= 600: long enough for carried chains
    assert res.hold_note is None and res.with_ignore(1).chains_carried is True
    res.chain_steps = 200
    assert "carried chains want at least 4 x their longest hold (252)" in res.hold_note
    out = io.StringIO()
    mci.report(res, io=out)
    assert out.getvalue().count("note: some chain of this :mcmc sweep point") == 1
