"""The :vegas kernel rule (csrc/mci_host_vegas_plan.h, between its marker lines) compiled for the HOST with g++ and walked arm by arm:
which variants -- {histogram copies, VGPR round keys, launch bound} -- it asks the builder for, in which batches (a batch compiles
side by side; every further batch is another compile latency of a cold start), which one it chooses and what it leaves in the plan.
The builder is a table of (VGPRs, scratch bytes) per variant, so the arms no integrand at hand reaches are walked too.  The expected
outcomes are read off compile_solver as it stood before the rule was split from its driver; the arms the BASELINE configurations take
agree with what their code objects show (profiles/r14_kernel_units.txt: c1 wide 512, c2 8 copies + keys at 512, c2_16grids rung 768, c4
rung 1024, the 6-D light kernel plain and wide, the 16-D fat one plain at 256, set_launch(128), the 16-copy stream, hist_copies = 4)."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "mcintegration.jl_amd", "csrc", "mci_host_vegas_plan.h")
BEGIN, END = "// >>> vegas kernel rule", "// <<< vegas kernel rule"

WRAP = r"""
#include <functional>
#include <vector>
%s
static VegasKernelPlan unpack(const int *q) {
    VegasKernelPlan p;
    p.planned = q[0]; p.keys = q[1]; p.wide = q[2]; p.threads_vegas = q[3]; p.ladder = q[4];
    p.hcopy_auto = q[5]; p.hcopy_rule = q[6]; p.hcopy_plan = q[7]; p.conservative = q[8];
    return p;
}
static void pack(const VegasKernelPlan &p, int *q) {
    const int v[9] = {p.planned, p.keys, p.wide, p.threads_vegas, p.ladder, p.hcopy_auto, p.hcopy_rule, p.hcopy_plan, p.conservative};
    for (int i = 0; i < 9; ++i) q[i] = v[i];
}
// which: 0 created(a, b) | 1 modules_dropped() | 2 explicit_threads(a, b) | 3 make_conservative(a)
extern "C" void transition(int *plan, int which, int a, int b) {
    VegasKernelPlan p = unpack(plan);
    if (which == 0) p.created(a, b != 0);
    if (which == 1) p.modules_dropped();
    if (which == 2) p.explicit_threads(a, b != 0);
    if (which == 3) p.make_conservative(a != 0);
    pack(p, plan);
}
extern "C" int planned_copies(const int *plan, int sixteen_fit, int *threads) { return unpack(plan).planned_copies(sixteen_fit != 0, threads); }
// in: threads, threads_explicit, ndraw, host_integrand, deterministic, copies_forced, sixteen_fit, copies
// table: rows of (copies, keys, threads, vgprs, scratch, ok); asked: rows of (batch, copies, keys, threads), at most max_asked
extern "C" int rule(int *plan, const int *in, const long *table, int nrows, int *chosen, int *asked, int max_asked, int *nasked) {
    VegasKernelPlan p = unpack(plan);
    const VegasRuleIn ri = {in[0], in[1] != 0, in[2], in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, in[7]};
    int batch = 0, n = 0, unknown = 0;
    VegasBuild build = [&](const std::vector<VegasVariant> &vs, std::vector<VegasBuilt> &out) {
        out.clear();
        for (const VegasVariant &v : vs) {
            if (n < max_asked) { asked[4 * n] = batch; asked[4 * n + 1] = v.copies; asked[4 * n + 2] = v.keys; asked[4 * n + 3] = v.threads; }
            ++n;
            VegasBuilt b = {0, 0, false};
            bool found = false;
            for (int r = 0; r < nrows && !found; ++r)
                if (table[6 * r] == v.copies && table[6 * r + 1] == (long)v.keys && table[6 * r + 2] == v.threads) {
                    b = {table[6 * r + 3], table[6 * r + 4], table[6 * r + 5] != 0};
                    found = true;
                }
            if (!found) ++unknown;
            out.push_back(b);
        }
        ++batch;
    };
    VegasVariant v = {0, false, 0};
    const int rc = vegas_kernel_rule(p, ri, build, &v);
    pack(p, plan);
    chosen[0] = v.copies; chosen[1] = v.keys; chosen[2] = v.threads;
    *nasked = n;
    return unknown ? -1000 - unknown : rc;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_host_vegas_plan.h: the marker lines %r ... %r are gone" % (BEGIN, END)
    section = text[text.index(BEGIN):text.index(END)]
    assert "vegas_kernel_rule" in section and "struct VegasKernelPlan" in section
    d = tmp_path_factory.mktemp("vegas_rule")
    src, so = os.path.join(d, "rule_host.cpp"), os.path.join(d, "rule_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % section)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so], check=True)
    return C.CDLL(so)


FIELDS = ("planned", "keys", "wide", "threads_vegas", "ladder", "hcopy_auto", "hcopy_rule", "hcopy_plan", "conservative")
CREATED, DROPPED, EXPLICIT, CONSERVATIVE = 0, 1, 2, 3


class Plan:
    def __init__(self, lib, **kw):
        self.lib = lib
        self.q = (C.c_int * 9)(0, 0, 0, 0, 0, 1, 1, 0, 0)
        for k, v in kw.items():
            self.q[FIELDS.index(k)] = int(v)

    def go(self, which, a=0, b=0):
        self.lib.transition(self.q, which, int(a), int(b))
        return self

    def __getattr__(self, name):
        return self.q[FIELDS.index(name)]

    def dict(self):
        return dict(zip(FIELDS, list(self.q)))


def run(lib, plan, table, threads=256, explicit=False, ndraw=16, host=False, det=False, forced=False, sixteen=False, copies=1):
    """-> (rc, chosen (copies, keys, threads), batches [[(copies, keys, threads), ...], ...]); table: {(copies, keys, threads): (vgprs, scratch) | None}"""
    rows = []
    for (c, k, t), r in table.items():
        rows += [c, int(k), t] + ([r[0], r[1], 1] if r else [0, 0, 0])
    tab = (C.c_long * max(len(rows), 1))(*rows)
    inp = (C.c_int * 8)(threads, explicit, ndraw, host, det, forced, sixteen, copies)
    chosen, asked, n = (C.c_int * 3)(), (C.c_int * (4 * 16))(), C.c_int()
    rc = lib.rule(plan.q, inp, tab, len(table), chosen, asked, 16, C.byref(n))
    assert rc > -1000, "the rule asked for a variant the table does not hold: %s" % [tuple(asked[4 * i + 1:4 * i + 4]) for i in range(n.value)]
    batches = []
    for i in range(n.value):
        b, v = asked[4 * i], (asked[4 * i + 1], bool(asked[4 * i + 2]), asked[4 * i + 3])
        while len(batches) <= b:
            batches.append([])
        batches[b].append(v)
    return rc, (chosen[0], bool(chosen[1]), chosen[2]), batches


def copy_plan(lib, copies=8):
    p = Plan(lib).go(CREATED, copies, 0)
    assert (p.hcopy_plan, p.threads_vegas, p.hcopy_auto, p.hcopy_rule, p.ladder) == (1, 512, copies, copies, 0)
    return p


KEYS, NOKEYS, PLAIN256, PLAIN512 = (8, True, 512), (8, False, 512), (1, False, 256), (1, False, 512)


def test_copies_rule_keys_variant_within_budget(lib):
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (120, 0), PLAIN256: (100, 0)})
    assert rc == 0 and chosen == KEYS and batches == [[KEYS, PLAIN256]]
    assert p.dict() == dict(planned=1, keys=1, wide=0, threads_vegas=512, ladder=0, hcopy_auto=8, hcopy_rule=8, hcopy_plan=1, conservative=0)


def test_copies_rule_keys_too_fat_sgpr_keys_fit(lib):
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (132, 0), NOKEYS: (124, 0), PLAIN256: (100, 0)})
    assert rc == 0 and chosen == NOKEYS and batches == [[KEYS, PLAIN256], [NOKEYS]]
    assert (p.planned, p.keys, p.threads_vegas) == (1, 0, 512)
    # ... scratch counts like registers
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (128, 8), NOKEYS: (110, 0), PLAIN256: (100, 0)})
    assert chosen == NOKEYS and batches == [[KEYS, PLAIN256], [NOKEYS]] and p.keys == 0


@pytest.mark.parametrize("vgprs", [78, 80])
def test_copies_rule_light_kernel_takes_the_plain_layout(lib, vgprs):
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (vgprs, 0), PLAIN256: (60, 0)})
    assert rc == 0 and chosen == PLAIN256 and batches == [[KEYS, PLAIN256]]
    assert (p.planned, p.keys, p.wide, p.threads_vegas) == (1, 0, 0, 0)
    # at most eight draws: the plain layout was built for 512 threads next to the copies, and keeps that bound when it is clean
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (vgprs, 0), PLAIN512: (57, 0)}, ndraw=6)
    assert rc == 0 and chosen == PLAIN512 and batches == [[KEYS, PLAIN512]]
    assert (p.planned, p.keys, p.wide, p.threads_vegas) == (1, 0, 1, 0)
    p = copy_plan(lib)
    assert run(lib, p, {KEYS: (81, 0), PLAIN256: (60, 0)})[1] == KEYS           # (81 .. 128: the copies)


def test_copies_rule_fat_kernel_takes_the_plain_layout(lib):
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (140, 0), NOKEYS: (140, 0), PLAIN256: (148, 352)})
    assert rc == 0 and chosen == PLAIN256 and batches == [[KEYS, PLAIN256], [NOKEYS]]
    assert (p.planned, p.keys, p.wide, p.threads_vegas) == (1, 0, 0, 0)


@pytest.mark.parametrize("wide_built", [(100, 16), (130, 0)])
def test_wide_attempt_that_does_not_fit_is_built_again_at_the_default_size(lib, wide_built):
    # the default arm (no copies, no ladder)
    p = Plan(lib).go(CREATED, 1, 0)
    rc, chosen, batches = run(lib, p, {PLAIN512: wide_built, PLAIN256: (90, 0)}, ndraw=2)
    assert rc == 0 and chosen == PLAIN256 and batches == [[PLAIN512], [PLAIN256]] and (p.planned, p.wide, p.threads_vegas) == (1, 0, 0)
    # ... and the plain layout of the copies rule
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: (70, 0), PLAIN512: wide_built, PLAIN256: (90, 0)}, ndraw=6)
    assert rc == 0 and chosen == PLAIN256 and batches == [[KEYS, PLAIN512], [PLAIN256]] and (p.planned, p.wide, p.threads_vegas) == (1, 0, 0)
    # a clean one stays
    p = Plan(lib).go(CREATED, 1, 0)
    rc, chosen, batches = run(lib, p, {PLAIN512: (128, 0)}, ndraw=2)
    assert rc == 0 and chosen == PLAIN512 and batches == [[PLAIN512]] and (p.planned, p.wide, p.threads_vegas) == (1, 1, 0)
    # no attempt: more than eight draws | a host integrand | an explicit or another workgroup size
    for kw in (dict(ndraw=9), dict(ndraw=2, host=True), dict(ndraw=2, explicit=True)):
        p = Plan(lib).go(CREATED, 1, 0)
        assert run(lib, p, {PLAIN256: (90, 0)}, **kw)[2] == [[PLAIN256]] and p.wide == 0


def rung(t):
    return (1, False, t)


@pytest.mark.parametrize("scratch,want", [((0, 0, 0), 1024), ((40, 0, 0), 768), ((40, 40, 0), 512), ((40, 40, 40), 512)])
def test_ladder_picks_the_first_rung_without_scratch_or_the_last(lib, scratch, want):
    p = Plan(lib).go(CREATED, 1, 1)
    assert (p.ladder, p.threads_vegas, p.hcopy_plan) == (1, 1024, 0)
    table = {rung(t): (128, s) for t, s in zip((1024, 768, 512), scratch)}
    rc, chosen, batches = run(lib, p, table, threads=512)
    assert rc == 0 and chosen == rung(want) and batches == [[rung(1024), rung(768), rung(512)]]
    assert (p.planned, p.threads_vegas, p.keys, p.wide) == (1, want, 0, 0)


def test_ladder_skips_the_rungs_above_where_it_starts(lib):
    p = Plan(lib, ladder=1, threads_vegas=768)
    rc, chosen, batches = run(lib, p, {rung(768): (168, 8), rung(512): (200, 0)}, threads=512)
    assert rc == 0 and chosen == rung(512) and batches == [[rung(768), rung(512)]] and p.threads_vegas == 512
    p = Plan(lib).go(CREATED, 1, 1).go(CONSERVATIVE, 0)     # (the conservative layout starts from `threads`)
    rc, chosen, batches = run(lib, p, {rung(512): (200, 0)}, threads=512)
    assert rc == 0 and chosen == rung(512) and batches == [[rung(512)]] and p.threads_vegas == 512
    # a rung that did not compile below a clean one is not looked at; above it, it fails the call
    p = Plan(lib).go(CREATED, 1, 1)
    assert run(lib, p, {rung(1024): (128, 0), rung(768): None, rung(512): None}, threads=512)[:2] == (0, rung(1024))
    p = Plan(lib).go(CREATED, 1, 1)
    assert run(lib, p, {rung(1024): (128, 8), rung(768): None, rung(512): (128, 0)}, threads=512)[0] != 0 and p.planned == 0


def test_second_variant_of_a_plan_with_keys_that_is_too_fat_is_rebuilt_without(lib):
    p = Plan(lib, planned=1, keys=1, threads_vegas=512, hcopy_auto=8, hcopy_rule=8, hcopy_plan=1)
    rc, chosen, batches = run(lib, p, {KEYS: (133, 0), NOKEYS: (126, 0)}, copies=8)
    assert rc == 0 and chosen == NOKEYS and batches == [[KEYS], [NOKEYS]]
    assert p.dict() == dict(planned=1, keys=1, wide=0, threads_vegas=512, ladder=0, hcopy_auto=8, hcopy_rule=8, hcopy_plan=1, conservative=0)   # (keys stays: as before)
    p = Plan(lib, planned=1, keys=1, threads_vegas=512, hcopy_auto=8, hcopy_rule=8, hcopy_plan=1)
    assert run(lib, p, {KEYS: (125, 0)}, copies=8)[1:] == (KEYS, [[KEYS]])


def test_second_variant_of_a_wide_plan_that_is_too_fat_goes_back_to_the_default_size(lib):
    p = Plan(lib, planned=1, wide=1)
    rc, chosen, batches = run(lib, p, {PLAIN512: (131, 0), PLAIN256: (131, 0)}, ndraw=2)
    assert rc == 0 and chosen == PLAIN256 and batches == [[PLAIN512], [PLAIN256]] and (p.planned, p.wide) == (1, 0)
    p = Plan(lib, planned=1, wide=1)
    assert run(lib, p, {PLAIN512: (100, 0)}, ndraw=2)[1:] == (PLAIN512, [[PLAIN512]]) and p.wide == 1
    # a standing ladder plan keeps its rung whatever the variant needs
    p = Plan(lib, planned=1, ladder=1, threads_vegas=768)
    assert run(lib, p, {rung(768): (168, 64)}, threads=512)[1:] == (rung(768), [[rung(768)]])


@pytest.mark.parametrize("ndraw", [2, 16])
def test_conservative_plan_asks_for_one_copy_sgpr_keys_and_the_default_size(lib, ndraw):
    p = copy_plan(lib).go(CONSERVATIVE, 0)
    assert p.dict() == dict(planned=0, keys=0, wide=0, threads_vegas=0, ladder=0, hcopy_auto=1, hcopy_rule=8, hcopy_plan=0, conservative=1)
    for _ in range(2):    # the first variant, then the other one of the standing plan
        rc, chosen, batches = run(lib, p, {PLAIN256: (90, 0)}, ndraw=ndraw)
        assert rc == 0 and chosen == PLAIN256 and batches == [[PLAIN256]] and (p.planned, p.keys, p.wide, p.threads_vegas) == (1, 0, 0, 0)
    # the deterministic mode keeps its copies; only the flag is set
    d = copy_plan(lib).go(CONSERVATIVE, 1)
    assert (d.conservative, d.hcopy_auto, d.hcopy_plan, d.threads_vegas) == (1, 8, 1, 512)


def test_explicit_thread_count_means_no_ladder_and_no_copies_rule(lib):
    p = copy_plan(lib).go(EXPLICIT, 128, 0)
    assert p.dict() == dict(planned=0, keys=0, wide=0, threads_vegas=0, ladder=0, hcopy_auto=1, hcopy_rule=8, hcopy_plan=0, conservative=0)
    rc, chosen, batches = run(lib, p, {(1, False, 128): (97, 0)}, threads=128, explicit=True)
    assert rc == 0 and chosen == (1, False, 128) and batches == [[(1, False, 128)]] and (p.planned, p.threads_vegas) == (1, 0)
    p = copy_plan(lib).go(EXPLICIT, 512, 0)            # 512 threads and more keep the copies, without the rule around them
    assert (p.hcopy_auto, p.hcopy_plan) == (8, 0)
    assert run(lib, p, {NOKEYS: (70, 0)}, threads=512, explicit=True)[1:] == (NOKEYS, [[NOKEYS]])
    p = Plan(lib).go(CREATED, 1, 1).go(EXPLICIT, 256, 0)
    assert (p.ladder, p.threads_vegas) == (0, 0)
    assert run(lib, p, {PLAIN256: (200, 100)}, explicit=True)[1:] == (PLAIN256, [[PLAIN256]])
    assert copy_plan(lib).go(EXPLICIT, 128, 1).hcopy_auto == 8    # (the hist_copies override holds at any size)


def test_forced_copies_the_sixteen_copy_stream_and_a_failed_build(lib):
    p = copy_plan(lib, 4)                              # the hist_copies override: the count as it is, no rule around it
    rc, chosen, batches = run(lib, p, {(4, False, 512): (101, 0)}, forced=True)
    assert rc == 0 and chosen == (4, False, 512) and batches == [[(4, False, 512)]] and (p.keys, p.threads_vegas) == (0, 512)
    p = copy_plan(lib)                                 # both opt-in streams: sixteen copies in one 1024-thread workgroup
    t = C.c_int()
    assert lib.planned_copies(p.q, 1, C.byref(t)) == 16 and t.value == 1024 and lib.planned_copies(p.q, 0, C.byref(t)) == 8 and t.value == 512
    rc, chosen, batches = run(lib, p, {(16, True, 1024): (115, 0), PLAIN256: (100, 0)}, sixteen=True)
    assert rc == 0 and chosen == (16, True, 1024) and batches == [[(16, True, 1024), PLAIN256]] and (p.keys, p.threads_vegas) == (1, 1024)
    p = copy_plan(lib)
    rc, chosen, batches = run(lib, p, {KEYS: None, PLAIN256: (100, 0)})
    assert rc != 0 and batches == [[KEYS, PLAIN256]] and (p.planned, p.keys) == (0, 0)
    # drop_modules: the next unit plans afresh from where this plan left the workgroup size
    p = Plan(lib, planned=1, keys=1, wide=1, threads_vegas=768, ladder=1).go(DROPPED)
    assert p.dict() == dict(planned=0, keys=0, wide=0, threads_vegas=768, ladder=1, hcopy_auto=1, hcopy_rule=1, hcopy_plan=0, conservative=0)
