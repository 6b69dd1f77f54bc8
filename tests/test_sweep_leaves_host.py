"""CPU tests of :vegas parameter sweeps over problems with several variable leaves (mci_set_sweep_leaves, csrc/mci_sweep_leaves.h): the
opt-in and what it leaves alone, eligibility on an offline engine, the new translation unit cross-compiled for gfx950 through the
library's own JIT, the two exports in include/mci.h, and the tracer's per-object userdata rows for closures that look a value up in a
table by a Discrete draw."""
import math
import os
import re
import types

import numpy as np
import pytest

import mcintegration_jl_amd as mci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
L = 50.0 ** 0.5


def offline(cfg, f, **kw):
    return mci.Engine(cfg, f, device=-1, **kw)


def one_leaf():
    return offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]]), mci.catalog.genz_product_peak(4))


def two_leaves():
    return offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]]), mci.catalog.x2y2())


def discrete():
    return offline(mci.Configuration(var=mci.Discrete(1, 3), dof=[[1]]), mci.catalog.discrete_id())


def discrete2():
    return offline(mci.Configuration(var=mci.Discrete([(1, 3), (1, 4)]), dof=[[1]]), mci.catalog.one())


def gauss4():
    return offline(mci.Configuration(var=mci.Continuous([(-L, L)] * 4), dof=[[1]]), mci.catalog.gaussian(4))


def bubble():
    beta = mci.catalog.bubble_parameters()["beta"]
    var = (mci.Continuous(0.0, 1.0, alpha=3.0), mci.Continuous(0.0, PI, alpha=3.0), mci.Continuous(0.0, 2 * PI, alpha=3.0),
           mci.Continuous(0.0, beta, alpha=3.0), mci.Discrete(1, 4, adapt=False))
    cfg = mci.Configuration(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)])
    return offline(cfg, mci.catalog.bubble(), measure=mci.bin_by(4))


def test_without_opting_in_the_refusals_are_todays():
    assert "2 variable leaves (a sweep point refines ONE Continuous grid)" in two_leaves().sweep_supported()
    assert discrete().sweep_supported() == "a Discrete or FermiK variable (a sweep point refines ONE Continuous grid)"
    assert "5 variable leaves" in bubble().sweep_supported()
    back = two_leaves()
    back.set_sweep_leaves("all")
    assert back.sweep_supported() is None
    back.set_sweep_leaves("one")                 # ... and out again
    assert "2 variable leaves" in back.sweep_supported()
    with pytest.raises(ValueError, match='"one" or "all"'):
        back.set_sweep_leaves("some")
    assert one_leaf().sweep_supported() is None


@pytest.mark.parametrize("make", [bubble, gauss4, discrete, discrete2, two_leaves, one_leaf])
def test_opted_in_layouts_are_eligible(make):
    eng = make()
    eng.set_sweep_leaves("all")
    assert eng.sweep_supported() is None


def test_opted_in_problems_are_still_refused_for_what_a_sweep_does_not_do():
    eng = bubble()
    eng.set_sweep_leaves("all")
    assert "measurefreq = 2" in eng.sweep_supported(measurefreq=2)
    assert ":vegas" in eng.sweep_supported(solver="vegasmc")
    fk = offline(mci.Configuration(var=(mci.FermiK(3, 1.0, 0.5, 10.0), mci.Continuous(0.0, 1.0)), dof=[[1, 1]]),
                 mci.Integrand("w[0] = x[0] * x[0] + x[3];", None, "fermik"))
    fk.set_sweep_leaves("all")
    assert "vegas doesn't work with FermiK" in fk.sweep_supported()
    det = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]]), mci.catalog.x2y2(), deterministic=True)
    det.set_sweep_leaves("all")
    assert "deterministic" in det.sweep_supported()
    strat = two_leaves()
    strat.set_sweep_leaves("all")
    strat.set_stratification(4)
    assert "stratified" in strat.sweep_supported()
    strat.set_stratification(on=False)
    assert strat.sweep_supported() is None


def test_a_map_that_does_not_fit_the_lds_is_refused_with_the_byte_count():
    big = offline(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 24), dof=[[1]]), mci.catalog.gaussian(24))
    big.set_sweep_leaves("all")
    why = big.sweep_supported()
    m = re.search(r"take (\d+) bytes of LDS \((\d+) at most\)", why)
    assert m, why
    # at least the map block itself: 24 grids of 1000 points
    assert int(m.group(1)) > 24 * 1000 * 8 > int(m.group(2)) == 159 * 1024
    with pytest.raises(mci.MCIError, match="bytes of LDS"):
        big.compile("vegas_sweep_leaves")


def test_the_new_unit_cross_compiles_for_gfx950_and_the_one_grid_unit_is_what_it_was():
    eng = bubble()
    with pytest.raises(mci.MCIError, match="5 variable leaves"):
        eng.compile("vegas_sweep_leaves")       # not opted in
    eng.set_sweep_leaves("all")
    with pytest.raises(mci.MCIError):
        eng.code_object("vegas_sweep_leaves")    # not compiled yet
    with pytest.raises(mci.MCIError, match="several leaves"):
        eng.compile("vegas_sweep")               # (the one-grid unit is not this problem's)
    eng.compile("vegas_sweep_leaves")
    path = eng.code_object("vegas_sweep_leaves")
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and b"mci_vegas_sweep_leaves" in blob and b"gfx950" in blob
    assert b"mci_vegas_sweep\0" not in blob and b"mci_vegas_batch" not in blob and b"mci_vegas_persist" not in blob
    for make in (gauss4, discrete, discrete2):   # the other layouts of the GPU tests compile too, each to a code object of its own
        other = make()
        other.set_sweep_leaves("all")
        other.compile("vegas_sweep_leaves")
        assert other.code_object("vegas_sweep_leaves") != path
    # one Continuous leaf: the same unit, the same file, the same bytes, opted in or not
    one = one_leaf()
    one.compile("vegas_sweep")
    before = one.code_object("vegas_sweep")
    was = open(before, "rb").read()
    assert b"mci_vegas_sweep\0" in was and b"mci_vegas_sweep_leaves" not in was
    one.set_sweep_leaves("all")
    one.compile("vegas_sweep")
    assert one.code_object("vegas_sweep") == before and open(before, "rb").read() == was
    with pytest.raises(mci.MCIError, match="one-grid"):
        one.compile("vegas_sweep_leaves")
    again = one_leaf()
    again.set_sweep_leaves("all")
    again.compile("vegas_sweep")
    assert again.code_object("vegas_sweep") == before


def test_map_rows_and_the_two_new_exports():
    assert one_leaf().sweep_map_doubles() == 1000                 # nbin + 1
    assert bubble().sweep_map_doubles() == 4 * 1000 + (5 + 4)
    assert discrete2().sweep_map_doubles() == (4 + 3) + (5 + 4)
    hdr = open(os.path.join(ROOT, "include", "mci.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_set_sweep_leaves\(mci_problem \*prob, int32_t mode\);", hdr, re.S)
    assert m
    for needle in ("MCI_SWEEP_ONE_GRID", "MCI_SWEEP_ALL_LEAVES", "FermiK", "159 KiB", "Discrete"):
        assert needle in m.group(1), needle
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_sweep_map_doubles\(const mci_problem \*prob, int32_t \*n\);", hdr, re.S)
    assert m and "nbin + 1" in m.group(1)
    assert re.search(r"enum \{ MCI_SWEEP_ONE_GRID = 0, MCI_SWEEP_ALL_LEAVES = 1 \};", hdr)
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mci_integrate_sweep\(", hdr, re.S).group(1)
    assert "mci_sweep_map_doubles" in doc and "accumulation" in doc and "distribution" in doc
    eng = bubble()
    eng.set_sweep_leaves("all")
    with pytest.raises(ValueError, match=r"maps must be \[points = 2\]\[grid points = 4009\]"):
        eng.integrate_sweep("vegas", userdata=np.ones((2, len(eng.integrand.userdata))), maps=np.zeros((2, 4000)))


def lookup(var, c):
    x, ext = var
    p = c.userdata
    return x[0] * p.kF * p.extQ[ext[0] - 1]


def para(k, n=3):
    return types.SimpleNamespace(kF=1.0 + 0.5 * k, extQ=np.linspace(0.1, 0.9, n) * (1.0 + k))


def lookup_config(obj=None):
    return dict(var=(mci.Continuous(0.0, 1.0), mci.Discrete(1, 3)), dof=[[1, 1]], **({} if obj is None else {"userdata": obj}))


def test_one_trace_gives_every_objects_row_with_its_table():
    from mcintegration_jl_amd import trace
    objs = [para(k) for k in range(3)]
    traced = [trace.trace_integrand(lookup, mci.Configuration(**lookup_config(o))) for o in objs]
    first = traced[0]
    assert "(int)" in first.body and first.body == traced[1].body == traced[2].body
    assert getattr(first, "userdata_for", None) is not None
    n = len(objs[0].extQ)
    for o, t in zip(objs, traced):
        row = first.userdata_for(o)
        np.testing.assert_array_equal(row, t.userdata)            # the first trace alone knows every row
        np.testing.assert_array_equal(row[-n:], o.extQ)          # ... whose table section is that object's extQ
    with pytest.raises(ValueError, match="different bodies.*extQ"):
        first.userdata_for(para(1, n=4))
    # a table the closure captured instead of reading it off userdata keeps its traced values at every point
    table = np.array([0.25, 0.5, 0.75])

    def captured(var, c):
        x, ext = var
        return x[0] * c.userdata.kF * table[ext[0] - 1]
    tc = trace.trace_integrand(captured, mci.Configuration(**lookup_config(objs[0])))
    row = tc.userdata_for(objs[2])
    np.testing.assert_array_equal(row[-3:], table)
    assert objs[2].kF in row and objs[0].kF not in row


def test_a_measure_that_reads_a_value_off_userdata_is_refused_and_one_that_only_touches_it_is_not():
    objs = [para(k) for k in range(2)]

    def reads_a_float(var, obs, weights, c):
        obs[0][0] += weights[0] * c.userdata.kF

    def reads_a_table(var, obs, weights, c):
        obs[0][0] += weights[0] * c.userdata.extQ[0]

    def touches(var, obs, weights, c):
        p = c.userdata                                             # (the reference's bubble measure does as much: test/bubble.jl:84-88)
        assert p is not None
        obs[0][var[1][0] - 1] += weights[0]

    kw = dict(obs=[np.zeros(3)], device=-1, leaves="all", **lookup_config())
    with pytest.raises(ValueError, match=r"the measure reads userdata\.kF"):
        mci.integrate_sweep(lookup, params=objs, measure=reads_a_float, **kw)
    with pytest.raises(ValueError, match=r"the measure reads userdata\.extQ"):
        mci.integrate_sweep(lookup, params=objs, measure=reads_a_table, **kw)
    with pytest.raises(mci.MCIError) as e:                         # traced, bound, eligible: only the device is missing
        mci.integrate_sweep(lookup, params=objs, measure=touches, **kw)
    assert e.value.code == 7
    with pytest.raises(ValueError, match='leaves must be "one" or "all"'):
        mci.integrate_sweep(lookup, params=objs, leaves="some", **lookup_config(), device=-1)
