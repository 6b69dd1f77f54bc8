"""GPU tests of :vegas sweep points that stop at a target error (mci_integrate_sweep_until; csrc/mci_sweep.h vegas_sweep<Cfg, true>,
csrc/mci_sweep_leaves.h vegas_sweep_leaves<Cfg, true>; the stop rule of csrc/mci_sweep_common.h).

The reference of every case is the FIXED sweep (Engine.integrate_sweep, the standing units): the stops are derived from its niter = 10
log with the oracle's average() (tests/until_cases.py reference_stops), after the margin condition has been asserted on that log -- no
decision within 5 % of its threshold --, and a point that stopped at n_p must equal the fixed sweep run with niter = n_p at the
per-iteration tolerances of test_hip_sweep.test_niter_1_leaves_the_oracles_first_iteration (the two units run the same device
functions; the tests print whether the match was bit for bit).  chi2 is held to 1e-6: it is made of (m_i - M)^2 / s_i^2 with
|m_i - M| ~ 1e-3 |M| here, so 1e-11 on the means and 1e-8 on the errors bound it by a few 1e-8.

Byte equality.  A point of the FIXED sweep with adapt = True is not byte-reproducible from call to call: the waves of its workgroup add
to one LDS histogram in the order they happen to be scheduled in, so the map behind the first train! differs in its last bits and the
later iterations follow (measured on an MI355X, eight Genz points, identical arguments and grid: two calls at niter = 10 are byte-equal
in 0 of 8 points, iter_mean to 1.1e-14, iter_std to 1.9e-11, maps to 6.5e-14; with adapt = False in 8 of 8).  The `until` units are
therefore compiled in the deterministic histogram layout (csrc/mci_device.h hslot, Cfg::DET: a histogram and an observable copy per wave,
summed in a fixed order): which workgroup runs a point, and what ran before it, never shows in its results -- three calls of the `until`
sweep are byte-equal in 8 of 8 points, every array.  Against the fixed sweep the per-iteration tolerances hold, not the bytes: that side
changes from call to call."""
import ctypes as C
import io
import re

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from until_cases import CASES, KW, MARGIN, SEED, TWO_BODY, reference_stops, row, two_row

pytestmark = pytest.mark.gpu


def genz_engine():
    from test_hip_sweep import engine
    return engine()[1]


def mixed_engine():
    from test_hip_sweep_leaves import mixed_engine as make
    return make()[1]


def two_engine():
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [2]], seed=SEED)
    return mci.Engine(cfg, mci.Integrand(TWO_BODY, two_row(0), "until_two"))


ENGINES = {"genz": genz_engine, "mixed": mixed_engine, "two_columns": two_engine}
_fixed = {}


def fixed(eng, case, uds, niter, **kw):
    """the fixed sweep of these points at this niter: computed once per (case, points, niter, arguments), never modified"""
    key = (case, repr(uds), niter, repr(sorted(kw.items())))
    if key not in _fixed:
        args = dict(KW, seed=SEED, **kw)
        args["niter"] = niter
        _fixed[key] = eng.integrate_sweep("vegas", userdata=uds, **args)
    return _fixed[key]


def expected(oracle, ref10, rtol, atol, ignore=1, min_niter=0):
    """stops (0: none) of the points of a fixed niter = 10 sweep, the margin condition asserted on its log first"""
    stops = []
    for k, r in enumerate(ref10):
        stop, margin = reference_stops(oracle, r["iter_mean"], r["iter_std"], rtol, atol, ignore=ignore, min_niter=min_niter)
        print("point %d: stop %s, nearest decision %.2f %% from its threshold" % (k, stop or "none", 100 * margin))
        assert margin >= MARGIN, (k, margin)
        stops.append(stop)
    return stops


def split_map(eng, flat):
    """a flat maps row leaf by leaf: [grid] of a Continuous leaf, [accumulation, distribution] of a Discrete one"""
    out, o = [], 0
    for lf in eng.config.leaves:
        if hasattr(lf, "ninc"):
            out.append([flat[o:o + lf.ninc]])
            o += lf.ninc
        else:
            n = lf.upper - lf.lower + 1
            out.append([flat[o:o + n + 1], flat[o + n + 1:o + 2 * n + 1]])
            o += 2 * n + 1
    assert o == len(flat)
    return out


def check_equals_fixed(eng, r, q, n):
    """point result r of the `until` call == q, the same point of the fixed sweep with niter = n; returns whether bit for bit"""
    assert r["niter_run"] == n and r["iter_mean"].shape[0] == n == r["iter_std"].shape[0] == q["iter_mean"].shape[0]
    np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["mean"], q["mean"], rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["stdev"], q["stdev"], rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(r["chi2"], q["chi2"], rtol=1e-6, atol=1e-12)
    assert r["neval"] == q["neval"] == n * KW["neval"] and r["status"] == q["status"] and np.array_equal(r["visited"], q["visited"])
    for lr, lq in zip(split_map(eng, r["maps"]), split_map(eng, q["maps"])):
        if len(lr) == 1:                    # a grid: 1e-12 of its range, equal ends
            g, og = lr[0], lq[0]
            assert g[0] == og[0] and g[-1] == og[-1] and np.all(np.diff(g) > 0)
            np.testing.assert_allclose(g, og, rtol=0, atol=1e-12 * (og[-1] - og[0]))
        else:                               # a Discrete leaf: its accumulation and its distribution
            np.testing.assert_allclose(lr[0], lq[0], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(lr[1], lq[1], rtol=1e-12)
    return all(np.asarray(r[k]).tobytes() == np.asarray(q[k]).tobytes() for k in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited", "maps"))


def run_case(oracle, case, **target):
    c = CASES[case]
    eng = ENGINES[case]()
    uds = [row(case, k) for k in c["ks"]]
    ref10 = fixed(eng, case, uds, 10)
    stops = expected(oracle, ref10, c["rtol"], c["atol"])
    assert stops == c["stops"], stops
    rs = eng.integrate_sweep_until("vegas", userdata=uds, seed=SEED, rtol=c["rtol"], atol=c["atol"], **dict(KW, **target))
    got = [r["niter_run"] for r in rs]
    print("%s: niter_run %s" % (case, got))
    assert got == [s or 10 for s in stops]
    assert [r["converged"] for r in rs] == [s != 0 for s in stops]
    exact = [check_equals_fixed(eng, r, fixed(eng, case, uds, n)[p], n) for p, (r, n) in enumerate(zip(rs, got))]
    print("%s: equal to the fixed sweep with niter = n_p bit for bit: %s" % (case, exact))
    return eng, uds, rs


def test_genz_points_stop_where_the_fixed_sweeps_log_says(oracle):
    eng, uds, rs = run_case(oracle, "genz")
    assert eng.code_object("vegas_sweep_until") != eng.code_object("vegas_sweep")
    assert eng.last_sweep_launch() == (5, 256)


def test_a_zero_target_runs_every_iteration_and_equals_the_fixed_sweep():
    eng = genz_engine()
    uds = [row("genz", k) for k in CASES["genz"]["ks"]]
    rs = eng.integrate_sweep_until("vegas", userdata=uds, seed=SEED, rtol=0.0, atol=0.0, **KW)
    assert [r["niter_run"] for r in rs] == [10] * 5 and not any(r["converged"] for r in rs)
    exact = [check_equals_fixed(eng, r, q, 10) for r, q in zip(rs, fixed(eng, "genz", uds, 10))]
    print("zero target: equal to the fixed sweep bit for bit: %s" % exact)


def test_a_huge_target_stops_at_the_first_legal_iteration():
    eng = genz_engine()
    uds = [row("genz", k) for k in (0, 1, 3)]
    rs = eng.integrate_sweep_until("vegas", userdata=uds, seed=SEED, rtol=1e9, **KW)
    assert [r["niter_run"] for r in rs] == [3] * 3 and all(r["converged"] for r in rs)              # ignore + 2, adapt = True
    for p, r in enumerate(rs):
        check_equals_fixed(eng, r, fixed(eng, "genz", uds, 3)[p], 3)
    rs = eng.integrate_sweep_until("vegas", userdata=uds, seed=SEED, rtol=1e9, adapt=False, ignore=0, **KW)
    assert [r["niter_run"] for r in rs] == [2] * 3 and all(r["converged"] for r in rs)
    for p, r in enumerate(rs):
        check_equals_fixed(eng, r, fixed(eng, "genz", uds, 2, adapt=False, ignore=0)[p], 2)
    rs = eng.integrate_sweep_until("vegas", userdata=uds, seed=SEED, rtol=1e9, min_niter=6, **KW)
    assert [r["niter_run"] for r in rs] == [6] * 3 and all(r["converged"] for r in rs)
    for p, r in enumerate(rs):
        check_equals_fixed(eng, r, fixed(eng, "genz", uds, 6)[p], 6)


def test_more_points_than_workgroups_take_their_points_from_the_cursor(oracle):
    """two workgroups, eight points of unequal length: which workgroup ran a point never shows in its results."""
    c = CASES["genz"]
    eng = genz_engine()
    ks = list(range(9))
    ref10 = fixed(eng, "genz", [row("genz", k) for k in ks], 10)
    keep = [k for k, r in zip(ks, ref10) if reference_stops(oracle, r["iter_mean"], r["iter_std"], c["rtol"], c["atol"])[1] >= MARGIN]
    print("points within the margin: %s" % keep)
    assert len(keep) >= 7 and set(c["ks"]) <= set(keep)
    uds = [row("genz", k) for k in keep]
    stops = expected(oracle, [ref10[k] for k in keep], c["rtol"], c["atol"])
    assert len(set(stops)) >= 4                              # (points of unequal length: the cursor hands them out in an order of its own)
    kw = dict(KW, seed=SEED, rtol=c["rtol"], atol=c["atol"])
    eng.sweep_workgroups(2)
    two = eng.integrate_sweep_until("vegas", userdata=uds, **kw)
    assert eng.last_sweep_launch()[0] == 2
    eng.sweep_workgroups(0)
    wide = eng.integrate_sweep_until("vegas", userdata=uds, **kw)
    assert eng.last_sweep_launch()[0] == len(keep)
    eng.sweep_workgroups(1)                                  # one workgroup runs them all, one after the other
    one = eng.integrate_sweep_until("vegas", userdata=uds, **kw)
    assert eng.last_sweep_launch()[0] == 1
    eng.sweep_workgroups(0)
    assert [r["niter_run"] for r in two] == [r["niter_run"] for r in wide] == [r["niter_run"] for r in one] == [s or 10 for s in stops]
    assert all(r["niter_run"] >= 1 for r in two)
    for a, b, c1 in zip(two, wide, one):
        assert a["neval"] == b["neval"] == c1["neval"] and a["status"] == b["status"] == c1["status"] == 0 and a["converged"] == b["converged"]
        for x in (a, c1):
            np.testing.assert_allclose(x["iter_mean"], b["iter_mean"], rtol=1e-11, atol=1e-300)
            np.testing.assert_allclose(x["iter_std"], b["iter_std"], rtol=1e-8, atol=1e-300)
            np.testing.assert_allclose(x["maps"], b["maps"], rtol=0, atol=1e-12)
    # every result array byte-equal between the grids (the until units' histograms do not depend on the waves' schedule)
    for a, b in zip(two, wide):
        for key in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited", "maps"):
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def test_which_workgroup_runs_a_point_never_shows_on_a_frozen_map(oracle):
    """adapt = False: no histogram is read, so the FIXED sweep is reproducible bit for bit as well (the module docstring) -- two workgroups,
    one workgroup and one workgroup per point return the same bytes, and those are the fixed sweep's with niter = n_p: the per-wave
    observable copies of the `until` units sum to the same bits here"""
    eng = genz_engine()
    ks, rtol = [0, 1, 3, 4, 6, 8], 7e-3                      # (chosen with the CPU oracle's loop at adapt = False: stops 2, 3, 2, 2, 2, none)
    uds = [row("genz", k) for k in ks]
    frozen = dict(adapt=False, ignore=0)
    stops = expected(oracle, fixed(eng, "genz", uds, 10, **frozen), rtol, 0.0, ignore=0)
    assert len(set(stops)) >= 3, stops
    kw = dict(KW, seed=SEED, rtol=rtol, **frozen)
    runs = []
    for g in (2, 1, 0):
        eng.sweep_workgroups(g)
        runs.append(eng.integrate_sweep_until("vegas", userdata=uds, **kw))
        assert eng.last_sweep_launch()[0] == (g or len(ks))
    two, one, wide = runs
    assert [r["niter_run"] for r in two] == [r["niter_run"] for r in one] == [r["niter_run"] for r in wide] == [s or 10 for s in stops]
    for p, (a, b, c1) in enumerate(zip(two, one, wide)):
        q = fixed(eng, "genz", uds, c1["niter_run"], **frozen)[p]
        assert check_equals_fixed(eng, c1, q, c1["niter_run"])                 # bit for bit
        for key in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited", "maps"):
            assert np.asarray(a[key]).tobytes() == np.asarray(c1[key]).tobytes() == np.asarray(b[key]).tobytes(), key
        assert a["neval"] == b["neval"] == c1["neval"] and a["status"] == b["status"] == c1["status"] == 0


def test_several_leaves_stop_under_the_unit_for_all_leaves(oracle):
    eng, uds, rs = run_case(oracle, "mixed")
    assert eng.code_object("vegas_sweep_leaves_until") != eng.code_object("vegas_sweep_leaves")
    with pytest.raises(mci.MCIError):
        eng.code_object("vegas_sweep_until")
    assert len(rs[0]["maps_by_leaf"]) == 3 and abs(rs[0]["maps_by_leaf"][2].sum() - 1.0) < 1e-12      # the Discrete distribution


def raw_until(eng, uds, target, niter, want_niter_run, **kw):
    """mci_integrate_sweep_until through the C ABI's own arrays, pre-filled with NaN: (iter_mean, iter_std [P][niter][nobs], niter_run | None)"""
    from mcintegration_jl_amd import _lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ud = np.ascontiguousarray(uds, dtype=np.float64)
    P, n = ud.shape[0], eng.nobs
    im, ie = np.full((P, niter, n), np.nan), np.full((P, niter, n), np.nan)
    m, s, c2, vis = np.zeros((P, n)), np.zeros((P, n)), np.zeros((P, n)), np.zeros((P, eng.config.N + 1))
    mo = np.zeros((P, eng.sweep_map_doubles()))
    st = np.zeros(P, dtype=np.int32)
    nrun = np.full(P, -1, dtype=np.int32)
    res = (_lib.ResultC * P)()
    for q in range(P):
        res[q] = _lib.ResultC(niter, n, None, None, dp(m[q]), dp(s[q]), dp(c2[q]), 0, 0.0, dp(vis[q]), 0, 0)
    a = eng._integrate_args("vegas", KW["neval"], niter, KW["block"], -1, True, 1.0, 1, SEED, 0)
    t = _lib.SweepTarget(*target)
    _lib.check(_lib.lib().mci_integrate_sweep_until(eng.p, C.byref(a), C.byref(t), P, dp(ud), None, None, dp(mo), res, dp(im), dp(ie),
                                                     st.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     nrun.ctypes.data_as(C.POINTER(C.c_int32)) if want_niter_run else None))
    return im, ie, (nrun if want_niter_run else None), m, [int(res[q].niter) for q in range(P)]


def test_two_columns_and_the_rows_behind_a_points_stop(oracle):
    """every column has to meet its bound (column 1: the relative one at k = 0, the absolute one at k = 1, 2, 3); through the C ABI the
    rows from n_p on are zero, results[p].niter stays the capacity, and niter_run = NULL is accepted"""
    eng, uds, rs = run_case(oracle, "two_columns")
    c = CASES["two_columns"]
    want = [s or 10 for s in c["stops"]]
    im, ie, nrun, mean, cap = raw_until(eng, uds, (c["rtol"], c["atol"], 0), 10, True)
    assert list(nrun) == want and cap == [10] * 5
    im2, ie2, none, mean2, _ = raw_until(eng, uds, (c["rtol"], c["atol"], 0), 10, False)
    assert none is None
    for p, n in enumerate(want):
        for a, e, m in ((im, ie, mean), (im2, ie2, mean2)):
            assert np.all(np.isfinite(a[p, :n])) and np.all(e[p, :n] > 0)
            assert np.all(a[p, n:] == 0.0) and np.all(e[p, n:] == 0.0)        # (the arrays came in as NaN)
            # (another call of the same sweep: what two adapting calls agree to, the module docstring)
            np.testing.assert_allclose(a[p, :n], rs[p]["iter_mean"], rtol=1e-11, atol=1e-300)
            np.testing.assert_allclose(e[p, :n], rs[p]["iter_std"], rtol=1e-8, atol=1e-300)
            np.testing.assert_allclose(m[p], rs[p]["mean"], rtol=1e-11, atol=1e-300)


def test_a_pathological_point_runs_every_iteration_and_its_neighbours_never_see_it():
    """the `pathological` row of test_hip_sweep.test_nothing_leaks_from_point_to_point between two good points, all three on ONE workgroup"""
    from test_hip_sweep import D, point
    eng = genz_engine()
    A, C_ = point(14), point(11)
    B = [float(D), float("nan")] + point(11)[2:]        # the `pathological` row of test_nothing_leaks_from_point_to_point
    kw = dict(KW, seed=SEED, rtol=CASES["genz"]["rtol"])
    eng.sweep_workgroups(1)                              # one workgroup: A, then B, then C in the LDS B left
    with_b = eng.integrate_sweep_until("vegas", userdata=[A, B, C_], **kw)
    eng.sweep_workgroups(0)
    without = eng.integrate_sweep_until("vegas", userdata=[A, C_], **kw)
    b = with_b[1]
    print("pathological: niter_run %s, status %s" % ([r["niter_run"] for r in with_b], [r["status"] for r in with_b]))
    assert b["niter_run"] == 10 and not b["converged"] and b["status"] & 2 and b["neval"] == 10 * KW["neval"]
    assert not np.all(np.isfinite(b["iter_mean"]))
    for r, q in zip((with_b[0], with_b[2]), without):
        assert r["niter_run"] == q["niter_run"] < 10 and r["converged"] and q["converged"] and r["status"] == q["status"] == 0
        np.testing.assert_allclose(r["iter_mean"], q["iter_mean"], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(r["iter_std"], q["iter_std"], rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(r["maps"], q["maps"], rtol=0, atol=1e-12)
    # ... and byte-equal to a call without the pathological point
    for r, q in zip((with_b[0], with_b[2]), without):
        for key in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited", "maps"):
            assert np.asarray(r[key]).tobytes() == np.asarray(q[key]).tobytes(), key


def test_a_pathological_points_neighbours_never_see_it_on_a_frozen_map():
    """the same with adapt = False, ignore = 0"""
    from test_hip_sweep import D, point
    eng = genz_engine()
    A, C_ = point(1), point(0)                           # (on the frozen map at rtol = 7e-3: stops 3 and 2)
    B = [float(D), float("nan")] + point(11)[2:]
    kw = dict(KW, seed=SEED, rtol=7e-3, adapt=False, ignore=0)
    eng.sweep_workgroups(1)
    with_b = eng.integrate_sweep_until("vegas", userdata=[A, B, C_], **kw)
    eng.sweep_workgroups(0)
    without = eng.integrate_sweep_until("vegas", userdata=[A, C_], **kw)
    b = with_b[1]
    assert b["niter_run"] == 10 and not b["converged"] and not np.all(np.isfinite(b["iter_mean"]))
    for r, q in zip((with_b[0], with_b[2]), without):
        assert r["niter_run"] == q["niter_run"] < 10 and r["converged"] and r["status"] == q["status"] == 0
        for key in ("iter_mean", "iter_std", "mean", "stdev", "chi2", "visited", "maps"):
            assert np.asarray(r[key]).tobytes() == np.asarray(q[key]).tobytes(), key


def test_integrate_sweep_with_a_tolerance_on_a_traced_closure():
    import types
    from test_hip_sweep import D, point

    def peak(x, c):
        p = c.userdata
        q = 1.0
        for d in range(D):
            t = x[d] - p.u[d]
            q = q * (1.0 / (p.a * p.a) + t * t)
        return 1.0 / q

    ks = CASES["genz"]["ks"]
    objs = [types.SimpleNamespace(a=point(k)[1], u=np.array(point(k)[2:])) for k in ks]
    rs = mci.integrate_sweep(peak, params=objs, var=mci.Continuous(0.0, 1.0), dof=[[D]], solver="vegas", neval=KW["neval"], niter=10, block=16,
                             seed=SEED, rtol=1e9, min_niter=4)
    assert len(rs) == 5 and all(r.sweep_batched for r in rs)
    eng = rs[0].config._engine
    assert all(r.config._engine is eng for r in rs) and eng.code_object("vegas_sweep_until")
    with pytest.raises(mci.MCIError):
        eng.code_object("vegas_sweep")                 # one code object: the fixed unit was never compiled
    assert [r.niter_run for r in rs] == [4] * 5 and all(r.converged is True for r in rs)
    for obj, r in zip(objs, rs):
        assert r.iter_mean.shape == (4, 1) and len(r.iterations) == 4 and r.neval == 4 * KW["neval"] and r.config.userdata is obj
        out = io.StringIO()
        mci.report(r, io=out)
        text = out.getvalue()
        assert len(re.findall(r"^\s*(?:ignore|\d+)\s+\S+ ± ", text, re.M)) == 4 and "target error" not in text
    tight = mci.integrate_sweep(peak, params=objs[:2], var=mci.Continuous(0.0, 1.0), dof=[[D]], solver="vegas", neval=KW["neval"], niter=4, block=16,
                                seed=SEED, rtol=1e-9)
    assert [r.niter_run for r in tight] == [4, 4] and all(r.converged is False for r in tight)
    out = io.StringIO()
    mci.report(tight[0], io=out)
    assert "ran all 4 iterations it was given without reaching its target error" in out.getvalue()
    for r, q in zip(tight, rs):
        np.testing.assert_allclose(r.iter_mean, q.iter_mean, rtol=1e-11, atol=1e-300)      # (the same four iterations, another call)
