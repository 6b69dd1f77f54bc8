"""CPU tests of chain sweeps that continue the chains of the call before (mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume;
csrc/mci_sweep_chains.h chain_sweep<Cfg, MCMC, true, true>): the two new units cross-compiled for gfx950 through the library's own JIT into
code objects of their own, the size query, every refusal in words on offline engines, the keyword errors of mci.integrate_sweep(...,
chain_state=...), what include/mci.h says, and an eligible call that fails only for want of a device."""
import os
import re

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import isa_mix
from test_sweep_carry_host import KERNELS, UNITS, sphere2
from test_sweep_leaves_host import bubble, discrete

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vegasmc_sweep_resume", "mcmc_sweep_resume")


def state(solver="vegasmc", blocks=16, nchain=4, ndraw=5, nd=2, iteration=9, ntrain=9, adapted=True):
    s = mci.ChainState(solver, blocks, nchain, ndraw, nd, iteration, ntrain, adapted, np.zeros(0))
    s.data = np.zeros(s.row_doubles())
    return s


@pytest.mark.parametrize("unit", NEW)
def test_the_resume_unit_compiles_to_a_code_object_of_its_own(unit):
    kernel = "mci_" + unit
    eng = bubble()
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object(unit)
    eng.compile(unit)
    path = eng.code_object(unit)
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and kernel.encode() + b"\0" in blob
    for other in KERNELS + tuple("mci_" + u for u in NEW):
        if other != kernel:
            assert other.encode() + b"\0" not in blob, other
    for other in UNITS + NEW:
        if other != unit:
            with pytest.raises(mci.MCIError):
                eng.code_object(other)              # compiling this unit compiles no other
    res = isa_mix.resources(path)[kernel]
    print(kernel, "bubble:", res)
    assert res["scratch"] == 0 and res["lds"] == 0 and res["vgpr_spill"] == 0 and res["max_threads"] == 256 and res["vgpr"] <= 512
    carried = unit.replace("_resume", "_carry")
    eng.compile(carried)                            # the carried unit: another kernel in another object
    assert eng.code_object(carried) != path and kernel.encode() + b"\0" not in open(eng.code_object(carried), "rb").read()
    for make in (sphere2, discrete):                # the layouts of the GPU tests, each a code object of its own
        e2 = make()
        e2.compile(unit)
        r2 = isa_mix.resources(e2.code_object(unit))[kernel]
        assert e2.code_object(unit) != path and r2["scratch"] == 0 and r2["lds"] == 0 and r2["vgpr_spill"] == 0 and r2["max_threads"] == 256


def test_one_header_six_instantiations():
    csrc = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
    text = open(os.path.join(csrc, "mci_sweep_chains.h")).read()
    assert text.count("chain_sweep<Cfg, false, true, true>(a0, f.c, &f.k, &f.r)") == 1 and text.count("chain_sweep<Cfg, true, true, true>(a0, f.c, &f.k, &f.r)") == 1
    assert "template <class Cfg, bool MCMC, bool CARRY = false, bool RESUME = false>" in text and text.count("if constexpr (RESUME)") >= 3
    head = text[:text.index("#pragma once")]
    assert "chain state does not travel between calls" in head and "mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume" in head
    jit = open(os.path.join(csrc, "mci_jit.h")).read()
    assert re.search(r'kUnitSweepChainsResume \*/ \{"mci_sweep_chains.h",.*"mci_vegasmc_sweep_resume", "SweepChainResumeArgs", "f", "vegasmc_sweep_resume", -1, false, 2, true, false, true\}', jit)
    assert re.search(r'kUnitSweepMcmcResume\s*\*/ \{"mci_sweep_chains.h",.*"mci_mcmc_sweep_resume", "SweepChainResumeArgs", "f", "mcmc_sweep_resume", -1, false, 2, true, false, true\}', jit)
    assert jit.index("kUnitSweepLeavesUntil */") < jit.index("kUnitSweepChainsResume */") < jit.index("kUnitSweepMcmcResume   */")   # after the standing ones


def test_the_size_query():
    eng = bubble()                                  # 5 draws, one integrand
    assert eng.ndraw == 5 and eng.config.N == 1
    n, info = eng.sweep_chain_state_doubles("vegasmc", neval=10000, niter=3, block=16, nchain=7, first_iteration=4)
    assert n == 5 * 16 * 7 + 16 * 7                 # x [ndraw][cap] | P [cap]
    assert info == dict(solver=1, nd=2, ndraw=5, iteration=6, ntrain=2, adapted=1, blocks=16, nchain=7)
    n, info = eng.sweep_chain_state_doubles("mcmc", neval=10000, niter=3, block=3, nchain=7, adapt=False)
    assert n == 5 * 21 + 11 + 2                     # x | 21 indices on 11 doubles | reweight_used [nd]
    assert info == dict(solver=2, nd=2, ndraw=5, iteration=2, ntrain=0, adapted=0, blocks=3, nchain=7)
    assert state("mcmc", 3, 7).row_doubles() == n   # (the Python object counts the same)
    with pytest.raises(mci.MCIError, match="nothing is carried with one chain per block"):
        eng.sweep_chain_state_doubles("vegasmc", nchain=1)
    with pytest.raises(mci.MCIError, match="solver is not :vegasmc"):
        eng.sweep_chain_state_doubles("vegas", nchain=4)


def test_every_refusal_in_words():
    eng = bubble()
    ask = lambda st, solver="vegasmc", **kw: eng.sweep_chain_state_supported(st, solver, **dict(dict(nchain=4, first_iteration=10), **kw))
    assert "the sweep chain carry is off (mci_set_sweep_chain_carry(prob, 1) first" in ask(state())[0]
    assert "the sweep chain carry is off" in ask(None)[0]
    eng.set_sweep_chain_carry(True)
    assert ask(None) == (None, False)               # states only go out: nothing to continue
    assert ask(state()) == (None, True)
    assert ask(state(nchain=300)) == (None, True)   # another chain count is the resampler's business
    assert ask(state("mcmc"), "mcmc") == (None, True)
    # :vegasmc: not out of the iteration on the never-refined map onto a refined one -- no refusal, the call starts afresh
    assert ask(state(iteration=0, ntrain=0, adapted=True), first_iteration=1) == (None, False)
    assert ask(state(iteration=0, ntrain=0, adapted=False), first_iteration=1) == (None, True)
    assert ask(state("mcmc", iteration=0, ntrain=0, adapted=True), "mcmc", first_iteration=1) == (None, True)
    for st, kw, words in (
            (state("mcmc"), {}, "the state is another solver's (stored under :mcmc, the call runs :vegasmc)"),
            (state(blocks=8), {}, "the state holds another block count (8 blocks stored, the call runs 16)"),
            (state(ndraw=4), {}, "the state is another layout's (nd = 2, ndraw = 4 stored, the problem has nd = 2, ndraw = 5)"),
            (state(nd=3), {}, "the state is another layout's (nd = 3, ndraw = 5 stored"),
            (state(nchain=1), {}, "the state holds 1 chains per block (nothing is carried with fewer than two)"),
            (state(iteration=7), {}, "a gap in the iteration numbers (the state was stored by iteration 7, the call starts at first_iteration = 10: 8 continues it)"),
            (state(), dict(first_iteration=9), "a gap in the iteration numbers"),
            (state(), dict(nchain=1), "nchain = 1 together with a chain state (nothing is carried with one chain per block)"),
            (state(), dict(nchain=0), "nchain = 0"),
            (state(), dict(measurefreq=2), "measurefreq = 2")):
        why, cont = ask(st, **kw)
        assert why is not None and words in why and cont is False, (why, words)
    assert "the state is another solver's (stored under :vegasmc, the call runs :mcmc)" in ask(state(), "mcmc")[0]
    assert b"this chain sweep cannot go on from a chain state: " in mci.lib().mci_last_error()
    # the entry points say the same, before they look for a device
    ud = np.ones((2, len(eng.integrand.userdata)))
    with pytest.raises(mci.MCIError, match="a gap in the iteration numbers") as e:
        eng.integrate_sweep_chains(userdata=ud, nchain=4, state=[state(iteration=7)] * 2, first_iteration=10)
    assert e.value.code == 1
    with pytest.raises(mci.MCIError, match="the state is another solver's"):
        eng.integrate_sweep_mcmc(userdata=ud, nchain=4, state=[state()] * 2, first_iteration=10)
    with pytest.raises(mci.MCIError, match="nchain = 1 together with a chain state"):
        eng.integrate_sweep_chains(userdata=ud, nchain=1, state=[state()] * 2, first_iteration=10)
    eng.set_sweep_chain_carry(False)
    with pytest.raises(mci.MCIError, match="the sweep chain carry is off"):
        eng.integrate_sweep_chains(userdata=ud, nchain=4, state=[state()] * 2, first_iteration=10)
    # what Python checks itself: the list and the arrays
    eng.set_sweep_chain_carry(True)
    with pytest.raises(ValueError, match="state must hold one ChainState per point"):
        eng.integrate_sweep_chains(userdata=ud, nchain=4, state=[state()], first_iteration=10)
    with pytest.raises(ValueError, match="chain states disagree with each other"):
        eng.integrate_sweep_chains(userdata=ud, nchain=4, state=[state(), state(nchain=5)], first_iteration=10)
    short = state()
    short.data = short.data[:-1]
    with pytest.raises(ValueError, match="does not hold the 384 doubles of its record"):
        eng.integrate_sweep_chains(userdata=ud, nchain=4, state=[short, short], first_iteration=10)


def test_an_eligible_call_fails_only_for_want_of_a_device():
    eng = bubble()
    ud = np.ones((2, len(eng.integrand.userdata)))
    for call, solver in ((eng.integrate_sweep_chains, "vegasmc"), (eng.integrate_sweep_mcmc, "mcmc")):
        with pytest.raises(mci.MCIError) as e:
            call(userdata=ud, nchain=4, carry=True, state=[state(solver)] * 2, first_iteration=10)
        assert e.value.code == 7 and eng.sweep_chain_carry() is False
    assert mci.lib().mci_integrate_sweep_chains_resume(eng.p, None, 2, None, None, None, None, None, None, None, None, None, None, None, None, None) == 1


def test_integrate_sweep_chain_state_argument_errors():
    f = mci.catalog.sphere2()
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]], device=-1)    # (variable objects per call: a bound one belongs to its engine)
    rows = np.zeros((2, 0))
    st = lambda **k: state(**dict(dict(blocks=16, nchain=4, ndraw=3, nd=3, iteration=9), **k))
    call = lambda states, **k: mci.integrate_sweep(f, params=rows, chain_state=states, **dict(dict(solver="vegasmc", chains=4, carry=True), **k), **kw())
    with pytest.raises(ValueError, match="chain_state= belongs to a chain sweep with carried chains: give carry=True"):
        call([st(), st()], carry=False)
    with pytest.raises(ValueError, match=r"chain_state must hold one ChainState per point \(2\), got 3"):
        call([st()] * 3)
    with pytest.raises(ValueError, match="chain_state must be a list with one ChainState per point"):
        call(7)
    with pytest.raises(ValueError, match="chain_state must hold ChainState objects"):
        call([None, None])
    with pytest.raises(ValueError, match="the chain states disagree with each other: they were stored by iterations 8, 9"):
        call([st(), st(iteration=8)])
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]])
    cfg.iterations_done = 4
    with pytest.raises(ValueError, match=r"stored by iteration 9, and config.iterations_done = 4: .* \(10\)"):
        mci.integrate_sweep(f, params=rows, chain_state=[st(), st()], solver="vegasmc", chains=4, carry=True, config=cfg, device=-1)
    with pytest.raises(ValueError, match="does not run as a sweep .*chain_state= needs the batched form"):
        call([st(), st()], measurefreq=2)
    with pytest.raises(mci.MCIError, match="the state is another solver's"):       # the library's refusals keep their words
        call([st(solver="mcmc")] * 2)
    with pytest.raises(mci.MCIError, match="the state holds another block count"):
        call([st(blocks=8)] * 2)
    for extra, solver in ((dict(solver="vegasmc", chains=4), "vegasmc"), (dict(solver="mcmc", chains=None, mcmc_chains=4), "mcmc")):
        with pytest.raises(mci.MCIError) as e:      # eligible, first_iteration taken from the states: only the device is missing
            call([st(solver=solver)] * 2, **extra)
        assert e.value.code == 7


def test_the_header_documents_the_states_and_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGASMC_SWEEP_RESUME = 19, MCI_MCMC_SWEEP_RESUME = 20 \};", hdr)
    assert re.search(r"#define MCI_ABI_VERSION 5\b", hdr)
    order = [hdr.index(s) for s in ("int mci_sweep_mcmc_supported(", "} mci_sweep_chain_info;", "} mci_sweep_chain_state;", "int mci_sweep_chain_state_doubles(",
                                    "int mci_sweep_chain_state_supported(", "int mci_integrate_sweep_chains_resume(", "int mci_integrate_sweep_mcmc_resume(")]
    assert order == sorted(order)
    said = lambda fn: " ".join(re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % fn, hdr, re.S).group(1).replace("*", " ").split())
    for needle in ("mci_set_sweep_chain_carry(prob, 1) is required", "K_old and K may differ", "pi_new / pi_old", "mci_chain_burnin(steps, 1, nslots)",
                   "state_out -> state_in", "byte for byte", "correlated = 1 whenever iteration 0 continued", "MCI_VEGASMC_SWEEP_RESUME", "4 GiB",
                   "mci_integrate_sweep_chains itself"):
        assert needle in said("mci_integrate_sweep_chains_resume"), needle
    for needle in ("MCI_MCMC_SWEEP_RESUME", "reweight_now[curr] / reweight_used[curr]", "nburn = 0", "always continues"):
        assert needle in said("mci_integrate_sweep_mcmc_resume"), needle
    for needle in ("another solver", "another block count", "another layout", "a gap in the iteration numbers", "never dropped silently", "nchain = 1",
                   "mci_set_sweep_chain_carry", "ntrain = 0 and adapted = 1"):
        assert needle in said("mci_sweep_chain_state_supported"), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_set_sweep_chain_carry\(", hdr, re.S)
    assert "chain state does not travel between calls" in m.group(1) and "mci_integrate_sweep_chains_resume" in m.group(1)
    names = [s[0] for s in mci._lib.SIGNATURES]
    for fn in ("mci_sweep_chain_state_doubles", "mci_sweep_chain_state_supported", "mci_integrate_sweep_chains_resume", "mci_integrate_sweep_mcmc_resume"):
        assert fn in names, fn
