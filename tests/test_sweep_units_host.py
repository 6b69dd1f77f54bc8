"""CPU test of the three sweep units as ONE family (csrc/mci_host_types.h kSweepUnits, csrc/mci_host_sweep.h compile_sweep_unit, csrc/mci_jit.h
kUnits): each compiles through the same path into a gfx950 code object of its own that holds its kernel and neither of the other two.
What is particular to a unit stays with tests/test_sweep_host.py, tests/test_sweep_leaves_host.py and tests/test_sweep_strat_host.py."""
import os

import pytest

import mcintegration_jl_amd as mci
from test_sweep_leaves_host import bubble
from test_sweep_strat_host import genz4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opted_in_bubble():
    eng = bubble()
    eng.set_sweep_leaves("all")
    return eng


def stratified_genz4():
    eng = genz4()
    eng.set_stratification()
    return eng


UNITS = {"vegas_sweep": genz4, "vegas_sweep_leaves": opted_in_bubble, "vegas_sweep_strat": stratified_genz4}


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_each_sweep_unit_compiles_to_a_code_object_of_its_own(unit):
    eng = UNITS[unit]()
    with pytest.raises(mci.MCIError, match="has not been compiled yet"):
        eng.code_object(unit)
    eng.compile(unit)
    path = eng.code_object(unit)
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob
    for other in UNITS:     # (the one-grid kernel's name is a prefix of the other two: the symbol table ends every name with a NUL)
        assert (b"mci_" + other.encode() + b"\0" in blob) == (other == unit), other
    for other in UNITS:
        if other != unit:
            with pytest.raises(mci.MCIError):
                eng.code_object(other)      # compiling one unit compiles no other
    eng.compile(unit)                       # again: the same file
    assert eng.code_object(unit) == path
    eng.close()


def test_the_three_units_share_one_device_header_and_one_driver():
    csrc = os.path.join(ROOT, "mcintegration.jl_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    for name in ("mci_sweep.h", "mci_sweep_leaves.h", "mci_sweep_strat.h"):
        text = read(name)
        assert '#include "mci_sweep_common.h"' in text and "__hip_atomic_load(&gh[" not in text and "s_waitcnt" not in text, name
    common = read("mci_sweep_common.h")
    assert common.count("__hip_atomic_load(&gh[") == 1 and common.count("__builtin_amdgcn_s_waitcnt(0x0F70)") == 1
    host = read("mci_host_sweep.h")
    assert host.count("hipModuleLaunchKernel(") == 1 and host.count(".build()") == 1     # (Candidate::build, csrc/mci_host_jit.h: the one hiprtc job)
