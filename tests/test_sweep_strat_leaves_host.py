"""CPU tests of stratified (VEGAS+) sweep points of problems with several Continuous variable leaves (mci_set_sweep_strat_leaves,
csrc/mci_sweep_strat_leaves.h): the export, its comment and the unit's id, the default answers of the stratified query left as they
are, the answers of an opted-in problem on offline engines, the new translation unit cross-compiled for gfx950 through the library's own
JIT, the one-grid stratified unit left byte for byte what it was, the `leaves="all"` keyword of mci.integrate_sweep together with
`stratify=`, and the cap of the GPU tests' allocation comparison for the reference alone."""
import os
import re
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_sweep_strat_leaves import CHAIN_CASES, CHAIN_IDS, LAYOUTS
from strat_cases import kernel_order_alloc
from test_sweep_strat_host import uniform_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240229
X2Y2P = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
TODAY = "2 variable leaves (a stratified sweep point refines ONE Continuous grid; several Continuous leaves are a follow-up)"
# the plan every layout is compiled and laid out under below (its first GPU case)
PLANS = {"two_grids": ([16, 16], 4096, 4), "pools3": ([3, 2, 2, 2], 2048, 16), "watson3": ([6, 6, 6], 4096, 4), "two_pools_ragged": ([5, 1, 3], 8192, 4),
         "peak2_two_grids": ([3, 2], 6000, 4)}


def offline(name, ud0=1.0):
    L = LAYOUTS[name]
    return mci.Engine(mci.Configuration(var=L["var"](), dof=L["dof"]), mci.Integrand(L["f"], [ud0]), device=-1)


def genz4():
    return mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]]), mci.catalog.genz_product_peak(4), device=-1)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_entry_its_comment_and_the_unit_id():
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    assert re.search(r"enum \{ MCI_VEGAS_SWEEP_STRAT_LEAVES = 16 \};", hdr)
    assert re.search(r"enum \{ MCI_SWEEP_ONE_GRID = 0, MCI_SWEEP_ALL_LEAVES = 1 \};", hdr)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_set_sweep_strat_leaves\(mci_problem \*prob, int32_t mode\);", hdr, re.S)
    assert m
    for needle in ("MCI_SWEEP_ONE_GRID", "MCI_SWEEP_ALL_LEAVES", "Continuous", "mci_set_sweep_leaves", "159 KiB", "MCI_VEGAS_SWEEP_STRAT_LEAVES",
                   "mci_sweep_map_doubles", "MCI_VEGAS_SWEEP_STRAT)"):
        assert needle in m.group(1), needle
    from mcintegration_jl_amd._lib import lib
    assert lib().mci_set_sweep_strat_leaves.argtypes is not None
    eng = offline("two_grids")
    with pytest.raises(ValueError, match='"one" or "all"'):
        eng.set_sweep_strat_leaves("some")
    assert lib().mci_set_sweep_strat_leaves(eng.p, 2) == 1      # MCI_ERR_INVALID


# ---- the query ------------------------------------------------------------------------------------------------------------------------

def test_default_mode_answers_as_before():
    two = offline("two_grids")
    two.set_stratification()
    assert two.sweep_strat_supported() == TODAY
    two.set_sweep_leaves("all")                     # (the opt-in of the classic sweep does not reach this one)
    assert two.sweep_strat_supported() == TODAY
    with pytest.raises(mci.MCIError, match="2 variable leaves"):
        two.compile("vegas_sweep_strat_leaves")
    two.set_sweep_strat_leaves("all")
    assert two.sweep_strat_supported() is None
    two.set_sweep_strat_leaves("one")
    assert two.sweep_strat_supported() == TODAY
    three = offline("pools3")
    three.set_stratification()
    assert three.sweep_strat_supported() == TODAY.replace("2 variable", "3 variable")


def test_opted_in_answers():
    two = offline("two_grids")
    two.set_sweep_strat_leaves("all")
    assert "not stratified" in two.sweep_strat_supported()      # (the common refusals stay)
    two.set_stratification()
    assert two.sweep_strat_supported() is None
    assert two.sweep_supported() == "the problem is stratified (mci_set_stratification_off first)"      # (and this opt-in does not reach the classic query)
    assert ":vegas" in two.sweep_strat_supported(solver="vegasmc") and "measurefreq = 2" in two.sweep_strat_supported(measurefreq=2)
    two.set_stratification(nstrat=[100, 100])
    why = two.sweep_strat_supported(neval=16000)
    assert "10000 hypercubes need at least 20000 samples" in why and "16000" in why
    assert two.sweep_strat_supported(neval=20000) is None
    assert two.sweep_strat_plan(20000) == dict(nstrat=[100, 100], ncube=10000, beta=0.75)
    with pytest.raises(mci.MCIError, match="several leaves"):      # which of the two units such a problem runs
        two.compile("vegas_sweep_strat")
    det = mci.Engine(mci.Configuration(var=LAYOUTS["two_grids"]["var"](), dof=[[1]]), mci.Integrand(X2Y2P, [1.0]), device=-1, deterministic=True)
    det.set_sweep_strat_leaves("all")
    det.set_stratification()
    assert det.sweep_strat_supported() == "deterministic mode"
    # a Discrete leaf is still refused where stratification is switched on
    disc = mci.Engine(mci.Configuration(var=(mci.Continuous(0.0, 1.0), mci.Discrete(1, 4)), dof=[[1, 1]]), mci.Integrand("w[0] = x[0] * x[1];"), device=-1)
    disc.set_sweep_strat_leaves("all")
    with pytest.raises(mci.MCIError, match="Discrete"):
        disc.set_stratification()


def test_one_grid_problem_opted_in_runs_the_one_grid_unit():
    plain, opted = genz4(), genz4()
    for eng in (plain, opted):
        eng.set_stratification()
    opted.set_sweep_strat_leaves("all")
    assert opted.sweep_strat_supported() is None
    plain.compile("vegas_sweep_strat")
    opted.compile("vegas_sweep_strat")
    assert opted.code_object("vegas_sweep_strat") == plain.code_object("vegas_sweep_strat")
    with pytest.raises(mci.MCIError, match="one-grid"):
        opted.compile("vegas_sweep_strat_leaves")
    assert opted.sweep_strat_geometry() == plain.sweep_strat_geometry()


def test_lds_refusal_names_the_byte_count():
    """three grids of 3000 points: the map block alone is 9000 doubles next to a histogram tile of 8997 and tables of 9000 more"""
    big = mci.Engine(mci.Configuration(var=tuple(mci.Continuous(0.0, 1.0, ninc=3000) for _ in range(3)), dof=[[1, 1, 1]]),
                     mci.Integrand("w[0] = x[0] * x[1] * x[2];"), device=-1)
    big.set_stratification(nstrat=[2, 2, 2])
    assert "3 variable leaves" in big.sweep_strat_supported()
    big.set_sweep_strat_leaves("all")
    why = big.sweep_strat_supported()
    m = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", why)
    assert m, why
    assert int(m.group(1)) > 3 * 9000 * 8 > int(m.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="bytes of LDS"):
        big.compile("vegas_sweep_strat_leaves")


@pytest.mark.parametrize("name", sorted(PLANS))
def test_lds_layout_of_the_test_layouts(name):
    """the one host function that makes the byte count: the map block, the sums and the broadcast pair behind the larger of the sample
    carve with the chunk's hypercubes and the refinement scratch of the largest leaf; within a CU's LDS at a chunk of whole trips"""
    nstrat, N, block = PLANS[name]
    eng = offline(name)
    eng.set_sweep_strat_leaves("all")
    eng.set_stratification(nstrat=nstrat)
    g = eng.sweep_strat_geometry(N, block)
    print("GEOMETRY %s: chunk %d, %d bytes of LDS, map at %d doubles" % (name, g["chunk"], g["lds_bytes"], g["map_off"]))
    nbins = [lf.ninc - 1 for lf in eng.config.leaves]
    nedge, maxn, NW = sum(n + 1 for n in nbins), max(nbins), eng.nobs
    nloc = g["chunk"] // 2 + 1
    carve = (eng.lds_bytes + 7) // 8 + (nloc + 1) + 2 * NW * nloc + 256 + 512 * NW      # Lds<Cfg> + strat_lds_doubles(nloc, 256)
    # (the refinement scratch: train_lds_doubles(maxn) >= 3 maxn, the merged slice maxn, the scan's partial sums 256)
    assert g["chunk"] in (256, 512, 1024, 2048) and g["map_off"] % 2 == 0 and g["map_off"] >= carve and g["map_off"] >= 4 * maxn + 256
    even = lambda n: (n + 1) & ~1
    assert g["lds_bytes"] == 8 * (g["map_off"] + even(nedge) + even(0) + even(0) + 4 + 4 * 8 + 2) <= 159 * 1024
    assert eng.sweep_map_doubles() == nedge


# ---- the new translation unit --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_grids", "pools3", "watson3", "two_pools_ragged"])
def test_the_unit_cross_compiles_for_gfx950(name):
    eng = offline(name)
    eng.set_sweep_strat_leaves("all")
    eng.set_stratification(nstrat=PLANS[name][0])
    with pytest.raises(mci.MCIError):
        eng.code_object("vegas_sweep_strat_leaves")     # not compiled yet
    eng.compile("vegas_sweep_strat_leaves")             # (the library refuses a unit that comes out with static LDS or scratch)
    path = eng.code_object("vegas_sweep_strat_leaves")
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"mci_vegas_sweep_strat_leaves" in blob and b"gfx950" in blob
    for other in (b"mci_vegas_sweep\0", b"mci_vegas_sweep_leaves", b"mci_vegas_sweep_strat\0", b"mci_vegas_batch", b"mci_vegas_persist", b"mci_vegas_strat\0",
                  b"k_strat_alloc", b"mci_vegasmc_sweep", b"mci_mcmc_sweep"):
        assert other not in blob, other
    # the AMDGPU metadata note: no scratch, no static LDS
    at = blob.index(b".name\xbcmci_vegas_sweep_strat_leaves")      # (0xa0 | 28: the fixstr of the kernel's name)
    for key in (b".private_segment_fixed_size", b".group_segment_fixed_size"):
        k = blob.rindex(key, 0, at) if key == b".group_segment_fixed_size" else blob.index(key, at)
        assert blob[k + len(key)] == 0, key
    assert blob.count(b".group_segment_fixed_size") == 1      # (one kernel in the code object)


def test_the_one_grid_stratified_unit_is_what_it_was():
    one = genz4()
    one.set_stratification()
    one.compile("vegas_sweep_strat")
    before = one.code_object("vegas_sweep_strat")
    was = open(before, "rb").read()
    two = offline("two_grids")
    two.set_sweep_strat_leaves("all")
    two.set_stratification()
    two.compile("vegas_sweep_strat_leaves")
    assert two.code_object("vegas_sweep_strat_leaves") != before
    again = genz4()
    again.set_stratification()
    again.compile("vegas_sweep_strat")
    assert again.code_object("vegas_sweep_strat") == before and open(before, "rb").read() == was
    assert b"mci_vegas_sweep_strat\0" in was and b"mci_vegas_sweep_strat_leaves" not in was


# ---- mci.integrate_sweep(stratify=..., leaves="all") ------------------------------------------------------------------------------------

ROWS = [[1.0], [0.5], [0.25]]


def kw2():
    return dict(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], device=-1)


def test_leaves_all_with_stratify_is_batched_and_the_default_falls_back_as_before(monkeypatch):
    f, st = mci.Integrand(X2Y2P, [1.0]), mci.Stratify(nstrat=[4, 3])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # (no fallback warning)
        with pytest.raises(mci.MCIError) as e:            # checked, bound, eligible: only the device is missing
            mci.integrate_sweep(f, ROWS, stratify=st, leaves="all", **kw2())
    assert e.value.code == 7
    # without leaves="all": today's fallback and its warning text
    import sys
    I = sys.modules[mci.integrate.__module__]
    seen = []

    def fake(f, **kw):
        seen.append(kw)
        return I.Result(np.zeros((1, 1)), np.ones((1, 1)), kw["config"], 0, neval=1, seconds=0.0, block=16)
    monkeypatch.setattr(I, "integrate", fake)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rs = mci.integrate_sweep(f, ROWS, stratify=st, **kw2())
    mine = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning) and "does not run as a sweep" in str(x.message)]
    assert len(mine) == 1 and TODAY in mine[0]
    assert len(rs) == 3 == len(seen) and all(k["stratify"] is st for k in seen) and not any(r.sweep_batched for r in rs)


def test_alloc_and_maps_of_the_wrong_length_raise():
    f, st = mci.Integrand(X2Y2P, [1.0]), mci.Stratify(nstrat=[4, 3])
    with pytest.raises(ValueError, match=r"alloc\[1\] has shape \(11,\), the plan nstrat = \[4, 3\] has 12 hypercubes"):
        mci.integrate_sweep(f, ROWS, stratify=st, leaves="all", alloc=[np.ones(12), np.ones(11), np.ones(12)], **kw2())
    with pytest.raises(ValueError, match=r"maps must be \[points = 3\]\[grid points = 2000\] \(sweep_map_doubles\(\)"):
        mci.integrate_sweep(f, ROWS, stratify=st, leaves="all", maps=[np.linspace(0.0, 1.0, 1000)] * 3, **kw2())
    eng = offline("two_pools_ragged")
    eng.set_sweep_strat_leaves("all")
    eng.set_stratification(nstrat=[5, 1, 3])
    assert eng.sweep_map_doubles() == 1300
    with pytest.raises(ValueError, match=r"integrate_sweep_strat: maps must be \[points = 2\]\[grid points = 1300\] \(sweep_map_doubles\(\)"):
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, 1)), maps=np.ones((2, 1000)))
    with pytest.raises(ValueError, match=r"d must be \[points = 2\]\[hypercubes = 15\]"):
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, 1)), d=np.ones((2, 14)))
    with pytest.raises(mci.MCIError) as e:                # right lengths: only the device is missing
        eng.integrate_sweep_strat("vegas", userdata=np.ones((2, 1)), maps=np.ones((2, 1300)), d=np.ones((2, 15)))
    assert e.value.code == 7


# ---- the allocation cap of the GPU comparison, for the reference alone ----------------------------------------------------------------

@pytest.mark.parametrize("name,nstrat,N,block,uds", CHAIN_CASES + [("two_pools_ragged", [5, 1, 3], 16384, 4, [0.9])], ids=CHAIN_IDS + ["two_pools_ragged-15-16384"])
def test_the_cap_of_the_gpu_comparison_holds_for_the_reference_alone(oracle, name, nstrat, N, block, uds):
    """d_h of three oracle iterations (uniform allocation first, the oracle's own train! and re-allocation between them): the kernel's
    order of the prefix sum against the oracle's long double one differs by at most 1 on at most max(2, ncube // 1000) hypercubes -- what
    check_alloc allows on the GPU"""
    L = LAYOUTS[name]
    ocfg = oracle.Config(L["oleaves"], L["dof"])
    of = oracle.compile_c_integrand(L["f"])
    nc = int(np.prod(nstrat))
    off = oracle.Config.strat_alloc(np.ones(nc), N, True)
    for k in range(3):
        r = ocfg.strat_iteration(of, [uds[0]], SEED, k, 0, nstrat, off)
        off = oracle.Config.strat_alloc(r["d"], N)
        ref = np.diff(off)
        emu = np.diff(kernel_order_alloc(r["d"], N)) if r["d"].sum() > 0 else np.diff(uniform_offsets(nc, N))
        ndiff = int(np.count_nonzero(ref != emu))
        print("cap: %s ncube %d N %d iteration %d: %d hypercubes differ" % (name, nc, N, k, ndiff))
        assert emu.sum() == N and emu.min() >= 2
        assert np.abs(ref - emu).max() <= 1 and ndiff <= max(2, nc // 1000)
        for i in range(len(L["oleaves"])):
            ocfg.add_hist(i, 1e-10)
        ocfg.train()
