"""The big :vegas unit (csrc/mci_host_vegas_plan.h, the section behind vegas_kernel_rule; csrc/mci_host_jit.h compile_vegas_big) without a GPU:
the headline layout's "vegas_big" code object cross-compiled in an offline context and read with llvm-readelf / llvm-objdump, what compiling
it leaves of the standing plan, and the selection rule vegas_big_rule compiled for the host with g++ and walked refusal by refusal -- every
condition of the rule has a case on each side of it."""
import ctypes as C
import math
import os
import subprocess

import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import isa_mix

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "mcintegration.jl_amd", "csrc", "mci_host_vegas_plan.h")
BEGIN, END = "// >>> vegas kernel rule", "// <<< vegas kernel rule"
L = math.sqrt(50.0)


def headline(device=-1):
    return mci.Engine(mci.Configuration(var=mci.Continuous(-L, L), dof=[[16]]), mci.catalog.gaussian(16), device=device)


@pytest.fixture(scope="module")
def objects():
    """(standing code object compiled alone, its bytes) and (standing, big) of an engine that compiled both, with what it reported"""
    eng = headline()
    eng.compile("vegas")
    alone = eng.code_object("vegas")
    alone_bytes = open(alone, "rb").read()
    eng.close()
    eng = headline()
    assert eng.histogram_copies() == 8
    eng.compile("vegas_big")                         # (before the standing unit: nothing of the standing plan is needed or touched)
    before = eng.histogram_copies()
    eng.compile("vegas")
    out = dict(alone=alone, alone_bytes=alone_bytes, standing=eng.code_object("vegas"), big=eng.code_object("vegas_big"),
               copies=(before, eng.histogram_copies()))
    eng.compile("vegas_big")                         # (a second call is a no-op)
    assert eng.code_object("vegas_big") == out["big"]
    eng.close()
    return out


def test_big_unit_resources_and_loop_mix(objects):
    res = isa_mix.resources(objects["big"])["mci_vegas_batch"]
    assert res["max_threads"] == 1024 and res["vgpr"] <= 128 and res["vgpr_spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0, res
    big = isa_mix.loop_mix(objects["big"], "mci_vegas_batch", draws_per_sample=16)
    std = isa_mix.loop_mix(objects["standing"], "mci_vegas_batch", draws_per_sample=16)
    m = big["mnemonics"]
    assert big["samples_per_trip"] == 2 and big["inner_backward_branches"] == 0
    assert m["ds_read_b128"] == 16 and m["ds_add_f64"] == 16 and big["pipes"]["lds"] == 32 and big["pipes"].get("vmem", 0) == 0
    assert abs(big["pipes"]["valu"] - std["pipes"]["valu"]) <= 1, (big["pipes"], std["pipes"])


def test_compiling_the_big_unit_leaves_the_standing_plan_alone(objects):
    assert objects["copies"] == (8, 8)
    assert objects["big"] != objects["standing"] and objects["standing"] == objects["alone"]
    assert open(objects["standing"], "rb").read() == objects["alone_bytes"]
    assert isa_mix.resources(objects["standing"])["mci_vegas_batch"]["max_threads"] == 512


def test_layouts_without_the_eight_copy_plan_refuse_the_name():
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]]), mci.catalog.log_over_sqrt(), device=-1)
    with pytest.raises(Exception, match="no big :vegas unit"):
        eng.compile("vegas_big")
    eng.close()
    eng = headline()
    eng.set_launch(256, -1)                          # an explicit workgroup size: no copy plan
    with pytest.raises(Exception, match="no big :vegas unit"):
        eng.compile("vegas_big")
    eng.close()


# ---- the rule, on the host ------------------------------------------------------------------------------------------------------------
FIELDS = ("vegas", "mf1", "pipe_unit", "forced_grid", "deterministic", "override_big", "cursor_forced", "copy_plan", "conservative",
          "copies_forced", "threads_explicit", "copies", "threads", "sixteen_fit_lds", "samples", "threshold", "adds", "adds_floor", "nblocks",
          "resident", "state")
WRAP = r"""
#include <functional>
#include <vector>
%s
extern "C" int big_rule(const long long *q) {
    VegasBigIn in{};
    in.vegas = q[0]; in.mf1 = q[1]; in.pipe_unit = q[2]; in.forced_grid = q[3]; in.deterministic = q[4]; in.override_big = (int)q[5];
    in.cursor_forced = q[6]; in.copy_plan = q[7]; in.conservative = q[8]; in.copies_forced = q[9]; in.threads_explicit = q[10];
    in.copies = (int)q[11]; in.threads = (int)q[12]; in.sixteen_fit_lds = q[13]; in.samples = q[14]; in.threshold = q[15];
    in.adds = (int)q[16]; in.adds_floor = (int)q[17]; in.nblocks = q[18]; in.resident = q[19]; in.state = (int)q[20];
    return (int)vegas_big_rule(in);
}
// -> 1 (VGPR keys) | 2 (SGPR keys) | the over-budget state
extern "C" int big_budget(long v0, long s0, int have1, long v1, long s1) {
    const VegasBuilt a = {v0, s0, true}, b = {v1, s1, true};
    bool keys = false;
    const int r = vegas_big_budget(a, have1 ? &b : nullptr, &keys);
    return r == 1 ? (keys ? 1 : 2) : r;
}
extern "C" int big_const(int which) {
    const int v[6] = {kBigCopies, kBigThreads, VegasBigUnit::kOverBudget, VegasBigUnit::kFailedCheck, VegasBigUnit::kNoCompile, (int)kBigTake};
    return v[which];
}
"""
REFUSALS = ("take", "not_mf1", "no_cursor", "forced_grid", "deterministic", "override_off", "standing_plan", "lds", "small", "few_adds",
            "not_resident", "over_budget", "failed_check", "no_compile")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    text = open(HEADER).read()
    section = text[text.index(BEGIN):text.index(END)]
    assert "vegas_big_rule" in section and "struct VegasBigIn" in section
    d = tmp_path_factory.mktemp("vegas_big_rule")
    src, so = os.path.join(d, "big_rule_host.cpp"), os.path.join(d, "big_rule_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % section)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so], check=True)
    return C.CDLL(so)


THRESHOLD = 2 ** 26
# the headline launch: 16 blocks, 1e8 samples, the unit loaded, 256 workgroups resident
HEADLINE = dict(vegas=1, mf1=1, pipe_unit=1, forced_grid=0, deterministic=0, override_big=-1, cursor_forced=0, copy_plan=1, conservative=0,
                copies_forced=0, threads_explicit=0, copies=8, threads=512, sixteen_fit_lds=1, samples=10 ** 8, threshold=THRESHOLD, adds=16,
                adds_floor=8, nblocks=16, resident=256, state=1)


def rule(lib, **kw):
    v = dict(HEADLINE, **kw)
    q = (C.c_longlong * len(FIELDS))(*[int(v[k]) for k in FIELDS])
    return REFUSALS[lib.big_rule(q)]


def test_constants(lib):
    assert [lib.big_const(i) for i in range(6)] == [16, 1024, -1, -2, -3, 0]


def test_headline_launch_takes_the_big_unit(lib):
    assert rule(lib) == "take"


@pytest.mark.parametrize("kw,want", [
    (dict(vegas=0), "not_mf1"),                                   # a chain solver's launch
    (dict(mf1=0), "not_mf1"),                                     # cadence
    (dict(pipe_unit=0), "no_cursor"),                             # no pipelined loop, a self-check launch, vegas_cursor = 0
    (dict(forced_grid=1), "forced_grid"),
    (dict(forced_grid=1, override_big=1), "forced_grid"),         # (the override needs vegas_cursor = 1 next to it)
    (dict(deterministic=1), "deterministic"),
    (dict(deterministic=1, override_big=1, cursor_forced=1), "deterministic"),
    (dict(override_big=0), "override_off"),
    (dict(override_big=0, cursor_forced=1), "override_off"),
    (dict(conservative=1), "standing_plan"),
    (dict(copy_plan=0), "standing_plan"),
    (dict(copies_forced=1), "standing_plan"),                     # the hist_copies override
    (dict(threads_explicit=1), "standing_plan"),
    (dict(copies=4), "standing_plan"),                            # copies < 8
    (dict(copies=1, threads=256), "standing_plan"),               # the plain layout the kernel rule fell back to
    (dict(copies=16, threads=1024), "standing_plan"),             # both opt-in streams: the standing unit is 16 x 1024 already
    (dict(sixteen_fit_lds=0), "lds"),
    (dict(samples=THRESHOLD - 1), "small"),
    (dict(adds=7), "few_adds"),
    (dict(resident=15), "not_resident"),
    (dict(resident=0, state=0), "not_resident"),                  # (asked before the unit is there, without the assumption)
    (dict(state=-1), "over_budget"),
    (dict(state=-2), "failed_check"),
    (dict(state=-3), "no_compile"),
])
def test_refusals(lib, kw, want):
    assert rule(lib, **kw) == want


@pytest.mark.parametrize("kw", [
    dict(samples=THRESHOLD),                                      # the threshold itself
    dict(adds=8),                                                 # the floor itself
    dict(resident=16),                                            # one workgroup per block
    dict(override_big=1),                                         # the override without vegas_cursor = 1 changes nothing
    dict(override_big=1, cursor_forced=1, samples=200, forced_grid=1, resident=1, adds=1),   # tests: any size, any grid
    dict(cursor_forced=1),                                        # vegas_cursor = 1 alone: the size rule holds
])
def test_other_side_of_each_condition_takes_it(lib, kw):
    assert rule(lib, **kw) == "take"


def test_forced_on_still_needs_a_usable_unit_and_the_copy_plan(lib):
    on = dict(override_big=1, cursor_forced=1, samples=200, forced_grid=1)
    assert rule(lib, state=-2, **on) == "failed_check" and rule(lib, state=-1, **on) == "over_budget"
    assert rule(lib, conservative=1, **on) == "standing_plan" and rule(lib, mf1=0, **on) == "not_mf1" and rule(lib, sixteen_fit_lds=0, **on) == "lds"
    assert rule(lib, cursor_forced=1, samples=200) == "small" and rule(lib, override_big=1, samples=200) == "small"


def test_register_budget(lib):
    assert lib.big_budget(123, 0, 0, 0, 0) == 1 and lib.big_budget(128, 0, 0, 0, 0) == 1     # VGPR keys within 128 registers, no scratch
    assert lib.big_budget(129, 0, 1, 101, 0) == 2 and lib.big_budget(128, 8, 1, 128, 0) == 2  # else SGPR keys
    assert lib.big_budget(140, 0, 1, 130, 0) == -1 and lib.big_budget(140, 0, 1, 120, 16) == -1 and lib.big_budget(140, 0, 0, 0, 0) == -1
