"""The self-check of a new :vegas code object (csrc/mci_host_check.h vegas_self_check, mci_vegas_check_status).

Every user integrand is a new hiprtc translation unit.  The first launch through a classic single-tile :vegas sample kernel that has no
marker in the kernel cache is preceded by <= 2 blocks x <= 512 samples through it, and its packed buffer is compared with what the
library's STATIC kernel k_check_vegas (csrc/mci_check.h: the iteration defined plainly, compiled ahead of time) makes of the same samples.

Bounds.  The static kernel against the CPU oracle: those tests/test_hip_parity.py holds the engine to (packed sums 1e-11, histogram 1e-9,
x bit for bit, jac 1e-13).  The check itself: spec_self_check's rule (statistics 1e-9, histogram 1e-8), inside the library.
A "miscompile" is stood in for by MCI_JIT_FLAGS=-DMCI_CHECK_PERTURB_HIST=1|2 (csrc/mci_device.h perturbed_bin): histogram adds go to the
next bin of the same leaf -- wrong arithmetic at valid addresses -- in the pipelined layout only (1) or in every :vegas layout (2)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from test_hip_parity import CASES, COMPLEX_BODY, SEED, hist_split, make, ocont

pytestmark = pytest.mark.gpu
PI = math.pi
WARNING = "does not reproduce the library's static :vegas kernel"


def oracle_samples(oracle, ocfg, fn, ud, nw, npb, block_lo, nblocks, iteration, bits=52, seed=SEED):
    """x[n][ndraw], jac[n], w[n][nw] of blocks [block_lo, block_lo + nblocks) as the ORACLE draws and evaluates them (the loop of
    tests/test_hip_parity.py test_map_draw_and_integrand_match_oracle over every sample)"""
    oc = ocfg.c
    n = npb * nblocks
    x, jac, w = np.zeros((n, oc.ndraw)), np.zeros(n), np.zeros((n, nw))
    call = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)(fn)
    udv = np.ascontiguousarray(ud if ud is not None else [0.0], dtype=np.float64)
    wo = np.zeros(nw)
    for s in range(n):
        gs = block_lo * npb + s
        k, jaco = 0, 1.0
        for vi in range(oc.npool):
            nl = oc.pool_nleaf[vi]
            for idx in range(1, oc.maxdof[vi] + 1):
                us = [oracle.uniform(seed, iteration * 8 + 0, gs, k + l, bits=bits) for l in range(nl)]
                ocfg.pool_create(vi, idx, us)
                jaco /= np.ctypeslib.as_array(oc.pool_prob[vi], shape=(idx + 1,))[idx]
                for l in range(nl):
                    x[s, k + l] = ocfg.pool_data(oc.pool_leaf0[vi] + l)[idx - 1]
                k += nl
        jac[s] = jaco
        call(x[s].ctypes.data, wo.ctypes.data, udv.ctypes.data)
        w[s] = wo
    return x, jac, w


STATIC_CASES = ["c1_log_over_sqrt", "c2_gauss16_shared_pool", "discrete", "c2_gauss4_composite", "sphere2_padding", "bubble", "complex"]


@pytest.mark.parametrize("name", STATIC_CASES)
def test_the_static_kernel_is_the_oracles_iteration(oracle, name):
    """k_check_vegas on its own (csrc/mci_debug.h mci_debug_vegas_check), fed the ORACLE's draws and weights -- no JIT kernel takes part --
    against the oracle's vegas_block: it reproduces every x bit for bit and every jac to 1e-13, and its packed buffer is the oracle's
    (statistics 1e-11, histogram 1e-9).  This pins the yardstick to the oracle, not to the code it will judge."""
    npb, lo, nb, it = 500, 1, 2, 1
    if name == "complex":
        cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1], [1]], type=complex, seed=SEED)
        eng = mci.Engine(cfg, mci.Integrand(COMPLEX_BODY))
        ocfg = oracle.Config([ocont()], [[1], [1]], obs_nbin=[2, 2])
        ocfg.set_ncomp(2)
        fn, ud, nw, ni = oracle.compile_c_integrand(COMPLEX_BODY), None, 4, 2
    else:
        c, cfg, eng, ocfg = make(name, oracle)
        fn, ud, ni = oracle.builtin(c["oname"]), c["ud"], cfg.N
        nw = ni
    x, jac, w = oracle_samples(oracle, ocfg, fn, ud, nw, npb, lo, nb, it)
    for mf in (1, 3):
        got, bad = eng.vegas_check_reference(npb, lo, nb, iteration=it, seed=SEED, measurefreq=mf, x=x, jac=jac, w=w)
        assert bad == (0, 0), (name, bad)
        ref = ocfg.iteration(oracle.VEGAS, fn, ud, npb, lo, lo + nb, it, SEED, measurefreq=mf)
        gs, gh = hist_split(got, eng.nobs, ni)
        rs, rh = hist_split(ref, eng.nobs, ni)
        np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300, err_msg=name)
        np.testing.assert_allclose(gh[:len(rh)], rh, rtol=1e-9, err_msg=name)
        assert got[2 * eng.nobs + 1] == nb * npb
    assert eng.vegas_check_status() == (0, 0)          # (the hook is not the self-check: nothing was launched through a :vegas unit)
    # ... and it sees a sample that is not the stream's: one x moved by an ulp, one jac by 1e-12
    x2, j2 = x.copy(), jac.copy()
    x2[7, 0] = np.nextafter(x2[7, 0], 10.0)
    j2[11] *= 1.0 + 1e-12
    assert eng.vegas_check_reference(npb, lo, nb, iteration=it, seed=SEED, x=x2, jac=j2, w=w)[1] == (1, 1)
    eng.close()


@pytest.mark.parametrize("name,copies", [("c1_log_over_sqrt", False), ("c2_gauss16_shared_pool", True)], ids=["plain", "pipelined"])
def test_status_life_cycle_and_marker(oracle, tmp_path, monkeypatch, name, copies):
    """cold private cache: 0 before the first launch, 1 after it with the marker next to the code object; a second engine on the same cache
    is verified FROM the marker (flag bit 1), which is not written again.  The plain layout (C1) and the pipelined one with its
    histogram copies (C2)."""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    c, cfg, eng, ocfg = make(name, oracle)
    assert eng.vegas_check_status() == (0, 0) and eng.vegas_check_launches() == 0
    got = eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    assert (eng.histogram_copies() > 1) == copies
    assert eng.vegas_check_status() == (1, 0) and eng.vegas_check_launches() == 3      # the unit, the sample dump, the static kernel
    marker = eng.code_object("vegas") + ".ok"
    assert os.path.exists(marker) and "hiprtc" in open(marker).read()
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 4000, 0, 8, 0, SEED)
    np.testing.assert_allclose(hist_split(got, eng.nobs, cfg.N)[1], hist_split(ref, eng.nobs, cfg.N)[1], rtol=1e-9)
    eng.iteration("vegas", 4000, 0, 8, iteration=1, seed=SEED)
    assert eng.vegas_check_launches() == 3                                               # once per code object
    eng.close()
    t = os.path.getmtime(marker)
    c, cfg, eng, ocfg = make(name, oracle)
    eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    assert eng.vegas_check_status() == (1, 2) and eng.vegas_check_launches() == 0 and os.path.getmtime(marker) == t
    eng.close()


@pytest.mark.parametrize("name", ["c1_log_over_sqrt", "c2_gauss16_shared_pool"])
def test_the_check_is_invisible(overrides, name):
    """integrate(..., deterministic=True) with the check switched off and with the check forced: bit-identical iterations and grids, the
    same launch records and status words afterwards"""
    c = CASES[name]

    def run(mode):
        overrides.set("vegas_self_check", mode)
        cfg = mci.Configuration(var=c["var"](), dof=c["dof"], seed=SEED)
        res = mci.integrate(c["f"], config=cfg, neval=40000, niter=3, block=8, solver="vegas", seed=SEED, deterministic=True, print=-1)
        eng = cfg._engine
        ms, wg, threads = eng.kernel_times_ms(8)
        rec = (len(ms), wg, threads, eng.split_chunks(), eng.last_chain_launch(), eng.check_status())
        return res, eng.grid(0).copy(), rec, eng.vegas_check_status(), eng.vegas_check_launches()
    r0, g0, rec0, st0, n0 = run(0)
    r1, g1, rec1, st1, n1 = run(1)
    assert st0 == (0, 0) and n0 == 0 and st1 == (1, 0) and n1 == 3
    assert np.array_equal(r0.iter_mean, r1.iter_mean) and np.array_equal(r0.iter_std, r1.iter_std) and np.array_equal(g0, g1)
    assert rec0 == rec1
    assert r1.vegas_check == (1, 0) and r1.vegas_check_note is None


def test_a_perturbed_pipelined_unit_trips_the_check_and_the_user_gets_the_right_histogram(oracle, overrides, tmp_path, monkeypatch, capfd):
    """C2's pipelined unit compiled with its histogram adds one bin off: one warning, status -1, and the iteration the user asked for
    comes from the unit compiled again in the conservative layout -- the oracle's histogram at 1e-9.  With the check switched off the same
    unit returns the shifted histogram silently: that is what the check stands in front of, and it shows that this test can see the
    defect."""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=1")
    name = "c2_gauss16_shared_pool"
    c, cfg, eng, ocfg = make(name, oracle)
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 4000, 0, 8, 0, SEED)
    rs, rh = hist_split(ref, 1, 1)
    capfd.readouterr()
    got = eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    err = capfd.readouterr().err
    assert eng.vegas_check_status() == (-1, 0) and err.count(WARNING) == 1 and "histogram" in err, err[-2000:]
    assert eng.histogram_copies() == 1
    gs, gh = hist_split(got, eng.nobs, cfg.N)
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(gh, rh, rtol=1e-9)
    got = eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED, measurefreq=3)      # the other cadence variant: conservative too, and verified
    ref3 = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 4000, 0, 8, 0, SEED, measurefreq=3)
    np.testing.assert_allclose(hist_split(got, 1, 1)[1], hist_split(ref3, 1, 1)[1], rtol=1e-9)
    assert eng.vegas_check_status()[0] == -1 and WARNING not in capfd.readouterr().err
    eng.close()
    overrides.set("vegas_self_check", 0)                                                 # what the check stands in front of
    c, cfg, eng, ocfg = make(name, oracle)
    got = eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    gs, gh = hist_split(got, eng.nobs, cfg.N)
    assert eng.vegas_check_status() == (0, 0) and WARNING not in capfd.readouterr().err
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-300)                          # right estimates ...
    assert not np.allclose(gh, rh, rtol=1e-9) and np.sum(~np.isclose(gh, rh, rtol=1e-9)) > 100    # ... the histogram in the wrong bins
    np.testing.assert_allclose(np.roll(gh[:999], -1), rh[:999], rtol=1e-9)               # (the leaf's 999 bins exactly one off: the stand-in, nothing else)
    eng.close()


def test_when_no_layout_agrees_the_status_is_minus_two_and_the_call_still_returns(oracle, tmp_path, monkeypatch, capfd):
    """every :vegas layout perturbed (=2): the conservative unit disagrees too -- two warnings, status -2, MCI_OK; report() says so"""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=2")
    c = CASES["c1_log_over_sqrt"]
    cfg = mci.Configuration(var=c["var"](), dof=c["dof"], seed=SEED)
    capfd.readouterr()
    res = mci.integrate(c["f"], config=cfg, neval=40000, niter=2, block=8, solver="vegas", seed=SEED, print=-1)
    err = capfd.readouterr().err
    assert cfg._engine.vegas_check_status() == (-2, 0) and err.count(WARNING) == 2, err[-2000:]
    assert res.vegas_check == (-2, 0) and "do not trust" in res.vegas_check_note
    import io
    out = io.StringIO()
    mci.report(res, io=out)
    assert "mci_vegas_check_status = -2" in out.getvalue()
    assert not os.path.exists(cfg._engine.code_object("vegas") + ".ok")


def test_a_user_measure_is_left_out_of_the_comparison_and_said_so(oracle, tmp_path, monkeypatch, capfd):
    """Measure("obs_add(0, rw[0]);"): the static kernel cannot run the body -- status 1 with flag bit 0; a perturbed unit still trips,
    through the histogram"""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    c = CASES["c1_log_over_sqrt"]
    eng = mci.Engine(mci.Configuration(var=c["var"](), dof=c["dof"], seed=SEED), c["f"], measure=mci.Measure("obs_add(0, rw[0]);"))
    eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    assert eng.vegas_check_status() == (1, 1)
    eng.close()
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=2")
    capfd.readouterr()
    eng = mci.Engine(mci.Configuration(var=c["var"](), dof=c["dof"], seed=SEED), c["f"], measure=mci.Measure("obs_add(0, rw[0]);"))
    eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    st, fl = eng.vegas_check_status()
    assert st < 0 and fl & 1 and WARNING in capfd.readouterr().err
    eng.close()


def test_paths_the_check_cannot_cover_report_zero_and_launch_nothing(overrides):
    """a host integrand (the closure runs on the host) and the many-tile path (32 grids: sample pass + mci_vegas_tiles): status 0, no
    check launch -- never 1"""
    overrides.set("vegas_self_check", 1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=SEED), lambda x, c: x[0] + x[1])
        eng.iteration("vegas", 2000, 0, 4, iteration=0, seed=SEED)
    assert eng.vegas_check_status() == (0, 0) and eng.vegas_check_launches() == 0
    eng.close()
    eng = mci.Engine(mci.Configuration(var=mci.Continuous([(0.0, 1.0)] * 32), dof=[[1]], seed=SEED), mci.catalog.genz_product_peak(32))
    eng.iteration("vegas", 2000, 0, 4, iteration=0, seed=SEED)
    assert eng.vegas_check_status() == (0, 0) and eng.vegas_check_launches() == 0
    eng.close()


def closure_layouts():
    """EVERY :vegas call of tests/test_hip_closure_battery.py, in its order: the same closure, var, dof, config, measure, type and seed
    (neval is not part of a layout: 40000 here, except where the battery itself runs its default 1e4).  {name: () -> (f, keywords)}."""
    from mcintegration_jl_amd import CompositeVar, Configuration, Continuous, Discrete

    def sphere2(offset):
        def integrand(X, config):
            i1 = 1.0 if X[0 + offset] ** 2 + X[1 + offset] ** 2 < 1.0 else 0.0
            i2 = 1.0 if X[0 + offset] ** 2 + X[1 + offset] ** 2 + X[2 + offset] ** 2 < 1.0 else 0.0
            return i1, i2

        def measure(X, obs, relative_weights, config):          # obs .+= relativeWeights
            for i in range(2):
                obs[i][0] += relative_weights[i]
        T = Continuous(0.0, 1.0, 2 + offset, offset=offset)
        return integrand, dict(config=Configuration(var=(T,), dof=[[2], [3]], neighbor=[(1, 3), (1, 2)], seed=102 + offset), measure=measure, debug=True)

    def sphere3():
        def measure3(X, obs, relative_weights, config):
            obs[0][0] += relative_weights[0]
            obs[1][0] += relative_weights[1]
            obs[1][1] += relative_weights[1] * 2.0
        config = Configuration(var=(Continuous(0.0, 1.0),), dof=[[2], [3]], neighbor=[(1, 3), (1, 2)], obs=[0.0, [0.0, 0.0]], seed=112)
        return sphere2(0)[0], dict(config=config, measure=measure3, debug=True)
    s2 = lambda x: 1.0 / (1.0 - np.cos(x[0]) * np.cos(x[1]) * np.cos(x[2])) / PI ** 3

    def leaves(cvars):
        x, y, z = cvars
        return 1.0 / (1.0 - np.cos(x[0]) * np.cos(y[0]) * np.cos(z[0])) / PI ** 3

    def two_pools():
        N, alpha = 8, 3.0
        x1 = Continuous(-1.0, 1.0, grid=np.linspace(-1.0, 1.0, N), alpha=alpha)
        x2 = Continuous(0.0, 1.0, grid=np.linspace(0.0, 1.0, N), alpha=alpha)

        def gauss(X):
            x = [X[0][0], X[1][0], X[1][1], X[1][2]]
            dx2 = 0.0
            for d in range(4):
                dx2 += (x[d] - 0.5) ** 2
            return np.exp(-dx2 * 100.0) * 1013.2118364296088
        return (lambda X, c: gauss(X)), dict(config=Configuration(var=(x1, x2), dof=[[1, 3]], seed=130), block=16, niter=10, neval=1e4)
    return {
        "sphere1": lambda: (lambda x, c: 1.0 if x[0] ** 2 + x[1] ** 2 < 1.0 else 0.0, dict(var=(Continuous(0.0, 1.0),), dof=[[2]], seed=101)),
        "sphere2_offset0": lambda: sphere2(0),
        "sphere2_offset2": lambda: sphere2(2),
        "sphere3_mixed_observables": sphere3,
        "discrete": lambda: (lambda x, c: x[0], dict(config=Configuration(var=(Discrete(1, 3, adapt=True),), dof=[[1]], seed=103), niter=10)),
        "discrete2": lambda: (lambda x, c: 1.0, dict(config=Configuration(var=(Discrete([(1, 3), (1, 4)], adapt=True),), dof=[[1]], seed=104), niter=10)),
        "singular1": lambda: (lambda X, c: np.log(X[0]) / np.sqrt(X[0]), dict(seed=105)),
        "singular2_one_pool": lambda: (lambda x, c: s2(x), dict(var=(Continuous(0.0, PI),), dof=[[3]], seed=106)),
        "composite_var": lambda: (lambda cvars, c: leaves(cvars),
                                  dict(var=CompositeVar(Continuous(0.0, PI), Continuous(0.0, PI), Continuous(0.0, PI)), dof=1, seed=107)),
        "continuous_highdim": lambda: (lambda cvars, c: leaves(cvars), dict(var=Continuous([(0.0, PI), (0.0, PI), (0.0, PI)]), dof=1, seed=108)),
        "complex1": lambda: (lambda x, c: x[0] + x[0] ** 2 * 1j, dict(type=complex, debug=True, seed=110)),
        "complex2": lambda: (lambda x, c: (x[0], x[0] ** 2 * 1j), dict(dof=[[1], [1]], type=complex, debug=True, seed=111)),
        "two_pools_8_point_grids": two_pools,
        "grid_1024_points": lambda: (lambda X, c: X[0], dict(var=(Continuous(0.0, 1.0, alpha=3.0, grid=np.linspace(0.0, 1.0, 1024), adapt=True),), dof=[[1]],
                                                             niter=10, seed=131)),
        "singular1_second_seed": lambda: (lambda X, c: np.log(X[0]) / np.sqrt(X[0]), dict(niter=10, seed=133)),
    }


@pytest.mark.parametrize("name", list(CASES))
def test_no_false_alarm_on_the_parity_layouts(oracle, overrides, capfd, name):
    """the check forced (marker or not) on every :vegas layout of tests/test_hip_parity.py's case table, both cadence variants: status 1,
    no warning.  None of them is a path the check leaves out."""
    overrides.set("vegas_self_check", 1)
    c, cfg, eng, ocfg = make(name, oracle)
    capfd.readouterr()
    eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    assert eng.vegas_check_status()[0] == 1 and eng.vegas_check_launches() == 3, name
    eng.iteration("vegas", 4000, 0, 8, iteration=1, seed=SEED, measurefreq=3)
    assert eng.vegas_check_status() == (1, 0) and eng.vegas_check_launches() == 6, name
    assert WARNING not in capfd.readouterr().err
    eng.close()


@pytest.mark.parametrize("name", list(closure_layouts()))
def test_no_false_alarm_on_closures(overrides, capfd, name):
    """... and on every :vegas call of the reference's battery as tests/test_hip_closure_battery.py types it (closures traced into device
    source): a pool with a variable offset, observables of different widths under a user measure, 7-increment and 1023-increment custom
    grids, two pools with dof = [[1, 3]], complex values.  Status 1 on each, verified in this process, no warning; none is skipped."""
    overrides.set("vegas_self_check", 1)
    f, kw = closure_layouts()[name]()
    kw = dict(dict(neval=40000, niter=2), **kw)
    capfd.readouterr()
    res = mci.integrate(f, print=-1, solver="vegas", **kw)
    assert isinstance(res.config._engine.integrand, mci.Integrand), "the closure was not written out as device source"
    assert res.vegas_check[0] == 1 and not res.vegas_check[1] & 6, (name, res.vegas_check)
    assert res.config._engine.vegas_check_launches() == 3
    assert WARNING not in capfd.readouterr().err


@pytest.mark.parametrize("seed", [4, 33])
def test_the_check_sees_a_shifted_histogram_whose_entries_are_tiny(oracle, tmp_path, monkeypatch, capfd, seed):
    """What 2 x 512 samples of the 16-D Gaussian add to their fullest bin of the untrained map depends on the seed: anything between 1e-27
    and 1e-5.  With these seeds it is below 3e-19 -- under the floor the propose / accept tables behind the histogram (3e-8 after a
    :vegas launch) would set if the histogram were compared in one section with them, and far under the clearStatistics! offsets.  The
    histogram is compared against its OWN largest entry, without the offsets: the perturbed pipelined unit trips all the same, and the
    user's iteration comes from the conservative unit with the oracle's histogram."""
    name = "c2_gauss16_shared_pool"
    c = CASES[name]
    ocfg = oracle.Config(c["oleaves"], c["dof"])
    x, jac, w = oracle_samples(oracle, ocfg, oracle.builtin(c["oname"]), c["ud"], 1, 512, 0, 2, 0, seed=seed)
    assert 0.0 < np.max((np.abs(w[:, 0]) * jac) ** 2) < 3e-19          # (the premise: the check's own samples)
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("MCI_JIT_FLAGS", "-DMCI_CHECK_PERTURB_HIST=1")
    c, cfg, eng, ocfg = make(name, oracle)
    capfd.readouterr()
    got = eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=seed)
    err = capfd.readouterr().err
    assert eng.vegas_check_status() == (-1, 0) and err.count(WARNING) == 1, err[-2000:]
    ref = ocfg.iteration(oracle.VEGAS, c["oname"], c["ud"], 4000, 0, 8, 0, seed)
    np.testing.assert_allclose(hist_split(got, 1, 1)[1], hist_split(ref, 1, 1)[1], rtol=1e-9)
    eng.close()


def test_an_empty_histogram_is_not_called_verified(tmp_path, monkeypatch, capfd):
    """every weight of the check's samples underflows in (|w| jac)^2: the two histograms are zero everywhere, which compares equal and
    shows nothing -- status stays 0 with flag bit 2, no marker, no warning, and the problem is not checked again in this process"""
    monkeypatch.setenv("MCI_KERNEL_CACHE", str(tmp_path))
    eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]], seed=SEED), mci.Integrand("w[0] = 1e-200 * x[0];"))
    capfd.readouterr()
    eng.iteration("vegas", 4000, 0, 8, iteration=0, seed=SEED)
    assert eng.vegas_check_status() == (0, 4) and eng.vegas_check_launches() == 3
    assert not os.path.exists(eng.code_object("vegas") + ".ok") and WARNING not in capfd.readouterr().err
    eng.iteration("vegas", 4000, 0, 8, iteration=1, seed=SEED)
    assert eng.vegas_check_launches() == 3
    eng.close()
