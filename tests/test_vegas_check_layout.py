"""CPU: the run-time layout table the library's static :vegas kernel is given (csrc/mci_host_check.h vegas_check_layout, read back through
csrc/mci_debug.h mci_debug_vegas_check_layout on an offline context) says what configuration.py says about the same Configuration --
draws per pool and slot, own-draw masks from dof, observable offsets -- and mci_vegas_check_status is bound everywhere a binding lives."""
import math
import os
import re

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi


def shapes():
    C, D = mci.Continuous, mci.Discrete
    return {
        "c1": dict(var=C(0.0, 1.0), dof=[[1]]),
        "shared_pool_16": dict(var=C(-7.0, 7.0), dof=[[16]]),
        "composite_4": dict(var=C([(-7.0, 7.0)] * 4), dof=[[1]]),
        "mixed_dof": dict(var=C(0.0, 1.0), dof=[[2], [3]]),
        "nested": dict(var=C(0.0, 1.0), dof=[[3], [6], [9], [12]]),
        "bubble": dict(var=(C(0.0, 1.0, alpha=3.0), C(0.0, PI, alpha=3.0), C(0.0, 2 * PI, alpha=3.0), C(0.0, 25.0, alpha=3.0), D(1, 4, adapt=False)),
                       dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)], measure=mci.bin_by(4)),
        "two_pools_unused": dict(var=(C(0.0, 1.0), D(1, 5)), dof=[[2, 0], [1, 1]]),
        "complex": dict(var=C(0.0, 1.0), dof=[[1], [1]], type=complex),
    }


@pytest.mark.parametrize("name", list(shapes()))
def test_layout_table_is_the_configurations(name):
    s = shapes()[name]
    cfg = mci.Configuration(var=s["var"], dof=s["dof"], obs=s.get("obs"), **({"type": s["type"]} if "type" in s else {}))
    body = " ".join("w[%d] = 1.0;" % q for q in range(cfg.N * cfg.ncomp))
    eng = mci.Engine(cfg, mci.Integrand(body), measure=s.get("measure"), device=-1)
    L = eng.vegas_check_layout()
    assert L["covered"] and L["with_obs"]
    assert (L["ndraw"], L["ni"], L["ncomp"]) == (cfg.ndraw, cfg.N, cfg.ncomp)
    assert L["nobs"] == sum(cfg.obs_nbin) and L["ncols"] == L["nobs"] + 2 + cfg.N + 1
    # draws: pool after pool, slot after slot, leaf after leaf (configuration.py pool_layout / draw_index)
    k, boff = 0, {}
    nbins = [(lf.ninc - 1 if hasattr(lf, "ninc") else int(lf.upper - lf.lower) + 1) for lf in cfg.leaves]
    for i in range(len(cfg.leaves)):
        boff[i] = sum(nbins[:i])
    assert L["nbin"] == sum(nbins)
    for vi in range(len(cfg.maxdof)):
        width = cfg.pool_width(vi)
        leaves = [i for i, p in enumerate(cfg.leaf_pool) if p == vi]
        assert len(leaves) == width
        for slot in range(cfg.maxdof[vi]):
            for l, leaf in enumerate(leaves):
                assert k == cfg.draw_index(vi, slot, l)
                d, lf = L["draws"][k], cfg.leaves[leaf]
                cont = hasattr(lf, "ninc")
                assert d["kind"] == (0 if cont else 1) and d["nbin"] == nbins[leaf] and d["boff"] == boff[leaf]
                assert d["scale"] == (float(nbins[leaf]) if cont else 1.0)
                covered = any(cfg.dof[i][vi] > slot for i in range(cfg.N))
                assert d["hist"] == (1 if (lf.adapt and covered) else 0), (name, k)
                k += 1
    assert k == cfg.ndraw
    # own masks: integrand i owns the first dof[i][v] slots of every pool v (vegas/montecarlo.jl:82, variable.jl:628-641)
    off = 0
    for i in range(cfg.N):
        own = 0
        for vi in range(len(cfg.maxdof)):
            for slot in range(cfg.dof[i][vi]):
                for l in range(cfg.pool_width(vi)):
                    own |= 1 << cfg.draw_index(vi, slot, l)
        g = L["integrands"][i]
        assert g["own"] == own, (name, i, bin(g["own"]), bin(own))
        assert (g["obs_off"], g["obs_nbin"]) == (off, cfg.obs_nbin[i])
        off += cfg.obs_nbin[i]
    bd = cfg.obs_bin_draw(s.get("measure"))
    assert [g["obs_bin_draw"] for g in L["integrands"]] == [int(b) for b in bd]
    assert eng.vegas_check_status() == (0, 0)          # offline: nothing is ever looked at
    eng.close()


def test_a_user_measure_and_uncovered_layouts_are_marked():
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]])
    eng = mci.Engine(cfg, mci.Integrand("w[0] = x[0];"), measure=mci.Measure("obs_add(0, rw[0]);"), device=-1)
    L = eng.vegas_check_layout()
    assert L["covered"] and not L["with_obs"]
    eng.close()
    cfg = mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 32), dof=[[1]])
    eng = mci.Engine(cfg, mci.catalog.genz_product_peak(32), device=-1)          # 32 grids: two histogram tiles
    assert not eng.vegas_check_layout()["covered"]
    eng.close()


def test_the_status_entry_point_is_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mci.h")).read(), flags=re.S)
    assert re.search(r"int\s+mci_vegas_check_status\(const mci_problem \*prob, int32_t \*status, int32_t \*flags\);", hdr)
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["mci_vegas_check_status"]
    assert len(sig[1]) == 3
    assert hasattr(mci.lib(), "mci_vegas_check_status") and hasattr(mci.Engine, "vegas_check_status")
    jl = open(os.path.join(ROOT, "mcintegration.jl_amd", "julia", "MCIntegrationHIP.jl")).read()
    assert re.search(r"ccall\(\(:mci_vegas_check_status, libmci\), Cint, \(Ptr\{Cvoid\}, Ptr\{Int32\}, Ptr\{Int32\}\)", jl)
    dbg = {n for n, _r, _a in _lib.DEBUG_SIGNATURES}
    assert {"mci_debug_vegas_check", "mci_debug_vegas_check_launches", "mci_debug_vegas_check_layout"} <= dbg
    for n in dbg:
        assert hasattr(mci.lib(), n), n
