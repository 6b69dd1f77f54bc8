"""Batched :vegas parameter sweeps against a loop of ordinary calls (profiles/r10_sweep.txt).

    python tools/sweep_bench.py table  [--neval 10000] [--points 1,16,256,1024,4096] [--threads 256]
    python tools/sweep_bench.py threads [--neval 10000] [--points 256,1024] [--repeat 5]
    python tools/sweep_bench.py once --points 1024       (one warm sweep and nothing else: the run a kernel trace is taken of)
    python tools/sweep_bench.py table --layout bubble [--neval 10000] [--points 1,16,256,1024]      (profiles/r11_sweep_leaves.txt)
    python tools/sweep_bench.py strat [--neval 10000] [--points 1,16,256,1024]                      (profiles/r12_sweep_strat.txt)
    python tools/sweep_bench.py strat --layout leaves [--nevals 10000,100000] [--points 1,16,256]   (profiles/r17_sweep_strat_leaves.txt)
    python tools/sweep_bench.py chains [--nevals 10000,100000,1000000] [--points 1,16,256] [--chains 1,16,64,256]   (profiles/r14_sweep_chains.txt)
    python tools/sweep_bench.py mcmc   [--nevals 10000,100000] [--points 1,16,256] [--chains 1,16,64,256]          (profiles/r15_sweep_mcmc.txt)
    python tools/sweep_bench.py chains --resume | mcmc --resume [--nevals 10000,100000] [--points 16,256] [--chains 16,64,256] [--repeat 5]   (profiles/r20_sweep_resume.txt)
    python tools/sweep_bench.py until  [--nevals 10000,100000] [--points 256,2048] [--rtol 2e-3] [--repeat 7]       (profiles/r18_sweep_until.txt)

The 4-D Genz product peak, niter = 10, block = 16.  `table`: wall time and us per point-iteration of Engine.integrate_sweep at every P,
and of the same points as a loop of Engine.integrate calls with the persistent launch, in the same process.
`threads`: the sweep at 256 / 512 / 1024 threads per workgroup (a size whose kernel would spill is refused by the library: reported),
the sizes interleaved `--repeat` times so that a drift of the box shows as scatter, not as a difference between sizes.
`--layout bubble`: the polarisation bubble (catalog.bubble: four Continuous leaves, a Discrete one, a histogram over it) scanned over
rs, swept with set_sweep_leaves("all") against a loop of ordinary Engine.integrate calls -- what such a scan runs without the opt-in;
the header line gives the sweep kernel's LDS bytes, workgroups per CU, VGPRs and scratch.
`strat`: the stratified sweep (Engine.integrate_sweep_strat, the default plan) against a loop of ordinary stratified calls
(Engine.integrate on a stratified engine: the launch chain of csrc/mci_host_strat.h) and against the classic sweep, the points under
seeds of their own at ONE parameter value, so that the scatter of their means is the error: sigma^2 x time can be read off each column.
`strat --layout leaves`: the Watson integrand 1 / (1 - c cos x cos y cos z) / pi^3 on Continuous([(0, pi)] * 3) -- three grids, one per
axis -- scanned over c: the stratified sweep with set_sweep_strat_leaves("all") (csrc/mci_sweep_strat_leaves.h) against a loop of ordinary
stratified calls, which is what such a scan runs without the opt-in; the header gives the kernel's LDS bytes, chunk, VGPRs and scratch.
`chains`: the bubble under the default solver -- the chain sweep (Engine.integrate_sweep_chains, `nchain` chains per block, one workgroup
per point) against a loop of ordinary Engine.integrate("vegasmc") calls with the SAME nchain and carried chains off, and against a loop of
default calls (automatic chain count, lanes per chain, carried chains), every call of a loop starting from the untrained map and
the initial reweight factors; a sweep point-iteration is neval / min(nchain, 256) dependent Markov steps deep, which the last column gives.
`mcmc`: the same table under :mcmc (Engine.integrate_sweep_mcmc against loops of Engine.integrate("mcmc") calls, thermal_ratio = 0.1; the
default loop's calls size their chains themselves and may run warm-up launches again); a point-iteration is neval / nchain + nburn steps
deep per chain.  Both tables give the best and the worst of the timed runs of every column.
`chains --carry` | `mcmc --carry` (profiles/r16_sweep_carry.txt): the sweep with chains carried from iteration to iteration
(set_sweep_chain_carry) against the uncarried sweep at the same nchain and against a loop of ordinary calls with the same nchain and
carried chains (set_chain_carry(1)); the last columns give the dependent steps of a point-iteration without and with carrying.
`chains --resume` | `mcmc --resume`: the continuation call -- a carried sweep of niter = 10 that follows a training call of niter = 10
through maps=, reweight= and first_iteration = 10 -- with the points' chain states (state=: its first iteration continues the stored chains)
and without them (its first iteration starts afresh and, under :mcmc, burns in), the two calls alternating `--repeat` times after a warm-up
of each; `launch` is the library's clock, `call` the wall time of the Engine method, best / median / worst of each, and the last columns
give the dependent steps of the call without and with the states.  On a library whose sweeps take no state= only the side without is timed.
`until`: the Genz scan at niter = 20 with a target error (Engine.integrate_sweep_until) against the fixed sweep of the same points:
(a) the cost of asking -- the `until` unit with rtol = atol = 0, which runs every iteration, over the fixed sweep; (b) the gain -- the
`until` unit at --rtol over the fixed sweep, next to sum n_p / (20 P), the share of the iterations actually run, which is what a perfect
schedule would reach.  The three calls alternate `--repeat` times after a warm-up of each.  Two clocks per call: `launch`, the library's
own (result `seconds`: uploads, the one launch, read-back, up to the stream's synchronise -- what the kernel decides), and `call`, the
wall time of the Engine method (with the host's statistics and P result dicts); best / median / worst of each.
One GPU process; run each mode under its own time limit."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcintegration_jl_amd as mci  # noqa: E402

D, NITER, BLOCK, SEED = 4, 10, 16, 20240229


def point(k):
    rng = np.random.default_rng(1000 + k)
    return [float(D), 2.0 + 6.0 * ((k * 0.37) % 1.0)] + list(0.3 + 0.4 * rng.random(D))


def body():
    return mci.catalog.genz_product_peak(D).body


def sweep_engine(threads=0):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[D]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(body(), point(0), "genz_product_peak%d" % D))
    eng.sweep_threads(threads)
    return eng


def time_sweep(eng, P, neval, reps=3):
    uds = np.array([point(k) for k in range(P)])
    eng.integrate_sweep("vegas", userdata=uds[:min(P, 4)], neval=neval, niter=NITER, block=BLOCK, seed=SEED)      # (compile, first launch)
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        rs = eng.integrate_sweep("vegas", userdata=uds, neval=neval, niter=NITER, block=BLOCK, seed=SEED)
        best = min(best, time.perf_counter() - t0)
    assert all(r["status"] == 0 for r in rs)
    return best, rs


def time_loop(P, neval):
    """as many ordinary calls, one after another, on ONE engine: a fresh map per call (mci_set_grid), the persistent launch.  The
    userdata stays that of point 0 -- the library has no way to change it without reloading the code objects, and mci.integrate binds
    a new engine per userdata: both cost more than what is timed here, so the loop is timed at its cheapest."""
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[D]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(body(), point(0), "genz_product_peak%d" % D))
    eng.set_persistent("on")
    g0 = eng.grid(0).copy()
    eng.integrate("vegas", neval=neval, niter=NITER, block=BLOCK, seed=SEED)
    assert eng.last_integrate_persistent()
    n = min(P, 256)      # (a loop is linear in P: 256 calls are timed, larger P scaled)
    out = []
    t0 = time.perf_counter()
    for k in range(n):
        eng.set_grid(0, g0)
        out.append(eng.integrate("vegas", neval=neval, niter=NITER, block=BLOCK, seed=SEED)["mean"][0])
    dt = time.perf_counter() - t0
    return dt * P / n, out


# ---- --layout bubble: several variable leaves (csrc/mci_sweep_leaves.h)
def bubble_point(k):
    """ud row of scan point k: rs from 1 to 2 (kF and the external momenta follow), the T domain -- the dimensionless beta of point 0 -- fixed"""
    rs = 1.0 + (k * 0.37) % 1.0
    p = mci.catalog.bubble_parameters(rs=rs)
    return [p["kF"], mci.catalog.bubble_parameters()["beta"], p["me"], float(p["spin"]), float(p["dim"]), float(p["Qsize"])] + list(p["extQ"])


def bubble_engine(ud, leaves="one"):
    import math
    beta = mci.catalog.bubble_parameters()["beta"]
    var = (mci.Continuous(0.0, 1.0, alpha=3.0), mci.Continuous(0.0, math.pi, alpha=3.0), mci.Continuous(0.0, 2 * math.pi, alpha=3.0),
           mci.Continuous(0.0, beta, alpha=3.0), mci.Discrete(1, 4, adapt=False))
    cfg = mci.Configuration(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(mci.catalog.bubble().body, ud, "bubble"), measure=mci.bin_by(4))
    eng.set_sweep_leaves(leaves)
    return eng


def bubble_table(Ps, neval):
    from mcintegration_jl_amd import isa_mix
    eng = bubble_engine(bubble_point(0), "all")
    assert eng.sweep_supported() is None
    eng.compile("vegas_sweep_leaves")
    res = isa_mix.resources(eng.code_object("vegas_sweep_leaves"))["mci_vegas_sweep_leaves"]
    lds = eng.sweep_lds_bytes()
    print("# bubble (4 Continuous leaves of 999 increments + Discrete(1, 4), q histogram), neval = %d, niter = %d, block = %d" % (neval, NITER, BLOCK))
    print("# mci_vegas_sweep_leaves: %d bytes of LDS per workgroup -> %d workgroup(s) per CU, %d VGPRs, %d bytes of scratch"
          % (lds, 2 if lds <= 80 * 1024 else 1, res["vgpr"], res["scratch"]))
    print("# sweep | loop of ordinary calls, ms (us per point-iteration) | loop / sweep")
    loop_eng = bubble_engine(bubble_point(0))
    g0 = [loop_eng.grid(l).copy() for l in range(4)]
    kw = dict(neval=neval, niter=NITER, block=BLOCK, seed=SEED)
    loop_eng.integrate("vegas", **kw)
    for P in Ps:
        uds = np.array([bubble_point(k) for k in range(P)])
        eng.integrate_sweep("vegas", userdata=uds[:min(P, 4)], **kw)
        ts = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            rs = eng.integrate_sweep("vegas", userdata=uds, **kw)
            ts = min(ts, time.perf_counter() - t0)
        assert all(r["status"] == 0 for r in rs)
        n = min(P, 64)       # (a loop is linear in P: up to 64 calls are timed, larger P scaled; ud stays point 0's, as in time_loop)
        tl = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            for k in range(n):
                for l in range(4):
                    loop_eng.set_grid(l, g0[l])
                q = loop_eng.integrate("vegas", **kw)
            tl = min(tl, (time.perf_counter() - t0) * P / n)
        same = np.max(np.abs(rs[0]["mean"] - q["mean"]) / np.abs(q["mean"]))
        print("P %5d  sweep %10.3f ms (%8.3f us)  loop %10.3f ms (%8.3f us)  loop / sweep %7.2f   grid x threads = %s   point 0: means differ by %.1e%s"
              % (P, 1e3 * ts, 1e6 * ts / (P * NITER), 1e3 * tl, 1e6 * tl / (P * NITER), tl / ts, eng.last_sweep_launch(), same,
                 "  (loop: %d calls timed, scaled)" % n if P > n else ""))


# ---- strat: stratified points (csrc/mci_sweep_strat.h)
def strat_table(Ps, neval):
    from mcintegration_jl_amd import isa_mix
    kw = dict(neval=neval, niter=NITER, block=BLOCK)
    strat = sweep_engine()
    strat.set_stratification()
    assert strat.sweep_strat_supported(**kw) is None
    strat.compile("vegas_sweep_strat")
    res = isa_mix.resources(strat.code_object("vegas_sweep_strat"))["mci_vegas_sweep_strat"]
    plan = strat.sweep_strat_plan(neval, BLOCK)
    print("# 4-D Genz product peak (point 0), neval = %d, niter = %d, block = %d; plan nstrat = %s (%d hypercubes), beta = %g"
          % (neval, NITER, BLOCK, plan["nstrat"], plan["ncube"], plan["beta"]))
    print("# mci_vegas_sweep_strat: %d VGPRs, %d bytes of scratch" % (res["vgpr"], res["scratch"]))
    print("# stratified sweep | loop of ordinary stratified calls | classic sweep: ms (us per point-iteration), scatter of the points' means over their seeds")
    classic = sweep_engine()
    loop = sweep_engine()
    loop.set_stratification()
    g0 = loop.grid(0).copy()
    loop.integrate("vegas", seed=SEED, **kw)
    for P in Ps:
        uds = np.array([point(0)] * P)
        seeds = [SEED + 1 + k for k in range(P)]
        out = {}
        for name, fn in (("strat", strat.integrate_sweep_strat), ("classic", classic.integrate_sweep)):
            fn("vegas", userdata=uds[:min(P, 4)], seeds=seeds[:min(P, 4)], **kw)      # (compile, first launch)
            best = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                rs = fn("vegas", userdata=uds, seeds=seeds, **kw)
                best = min(best, time.perf_counter() - t0)
            assert all(r["status"] == 0 for r in rs)
            out[name] = (best, np.array([r["mean"][0] for r in rs]))
        n = min(P, 64)       # (a loop is linear in P: up to 64 calls are timed, larger P scaled)
        tl, means = float("inf"), []
        for rep in range(3):
            means = []
            t0 = time.perf_counter()
            for k in range(n):
                loop.set_grid(0, g0)
                means.append(loop.integrate("vegas", seed=seeds[k], **kw)["mean"][0])
            tl = min(tl, (time.perf_counter() - t0) * P / n)
        out["loop"] = (tl, np.array(means))

        def col(name):
            t, m = out[name]
            return "%10.3f ms (%8.3f us) scatter %s" % (1e3 * t, 1e6 * t / (P * NITER), "%.3e" % np.std(m, ddof=1) if m.size > 1 else "   -     ")
        print("P %5d  strat sweep %s | strat loop %s | classic sweep %s | loop / strat sweep %6.2f, classic / strat sweep %5.2f   grid x threads = %s%s"
              % (P, col("strat"), col("loop"), col("classic"), out["loop"][0] / out["strat"][0], out["classic"][0] / out["strat"][0],
                 strat.last_sweep_launch(), "  (loop: %d calls timed, scaled)" % n if P > n else ""))


# ---- strat --layout leaves: stratified points with several Continuous leaves (csrc/mci_sweep_strat_leaves.h)
WATSON3 = "w[0] = 1.0 / (1.0 - ud[0] * cos(x[0]) * cos(x[1]) * cos(x[2])) / (M_PI * M_PI * M_PI);"


def watson_point(k):
    return [0.5 + 0.49 * ((k * 0.37) % 1.0)]


def watson_engine(leaves="one"):
    import math
    cfg = mci.Configuration(var=mci.Continuous([(0.0, math.pi)] * 3), dof=[[1]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(WATSON3, watson_point(0), "watson3"))
    eng.set_sweep_strat_leaves(leaves)
    eng.set_stratification()
    return eng


def strat_leaves_table(Ps, nevals):
    from mcintegration_jl_amd import isa_mix
    eng = watson_engine("all")
    eng.compile("vegas_sweep_strat_leaves")
    res = isa_mix.resources(eng.code_object("vegas_sweep_strat_leaves"))["mci_vegas_sweep_strat_leaves"]
    print("# Watson integrand on Continuous([(0, pi)] * 3) (three grids of 999 increments), scanned over c; niter = %d, block = %d" % (NITER, BLOCK))
    print("# mci_vegas_sweep_strat_leaves: %d VGPRs, %d bytes of scratch" % (res["vgpr"], res["scratch"]))
    print("# stratified sweep | loop of ordinary stratified calls (what the scan runs without the opt-in): ms (us per point-iteration)")
    loop = watson_engine()
    g0 = [loop.grid(l).copy() for l in range(3)]
    for neval in nevals:
        kw = dict(neval=neval, niter=NITER, block=BLOCK, seed=SEED)
        assert eng.sweep_strat_supported(**kw) is None and "3 variable leaves" in loop.sweep_strat_supported(**kw)
        plan, geo = eng.sweep_strat_plan(neval, BLOCK), eng.sweep_strat_geometry(neval, BLOCK)
        print("# neval = %d: plan nstrat = %s (%d hypercubes), chunk %d samples, %d bytes of LDS per workgroup -> %d workgroup(s) per CU"
              % (neval, plan["nstrat"], plan["ncube"], geo["chunk"], geo["lds_bytes"], 2 if geo["lds_bytes"] <= 80 * 1024 else 1))
        loop.integrate("vegas", **kw)                                                            # (compile, first launches)
        for P in Ps:
            uds = np.array([watson_point(k) for k in range(P)])
            eng.integrate_sweep_strat("vegas", userdata=uds[:min(P, 4)], **kw)                   # (first launch)
            ts, tsw = float("inf"), 0.0
            for _ in range(3):
                t0 = time.perf_counter()
                rs = eng.integrate_sweep_strat("vegas", userdata=uds, **kw)
                dt = time.perf_counter() - t0
                ts, tsw = min(ts, dt), max(tsw, dt)
            assert all(r["status"] == 0 for r in rs)
            n = min(P, 16)       # (a loop is linear in P: up to 16 calls are timed, larger P scaled; ud stays point 0's, as in time_loop)
            tl, tlw = float("inf"), 0.0
            for _ in range(3):
                t0 = time.perf_counter()
                for k in range(n):
                    for l in range(3):
                        loop.set_grid(l, g0[l])
                    q = loop.integrate("vegas", **kw)
                dt = (time.perf_counter() - t0) * P / n
                tl, tlw = min(tl, dt), max(tlw, dt)
            same = abs(rs[0]["mean"][0] - q["mean"][0]) / abs(q["mean"][0])
            print("neval %7d  P %4d  strat sweep %10.3f ms (%9.3f us; worst %10.3f)  strat loop %10.3f ms (%9.3f us; worst %10.3f)  loop / sweep %6.2f"
                  "   grid x threads = %s   point 0: means differ by %.1e%s"
                  % (neval, P, 1e3 * ts, 1e6 * ts / (P * NITER), 1e3 * tsw, 1e3 * tl, 1e6 * tl / (P * NITER), 1e3 * tlw, tl / ts, eng.last_sweep_launch(), same,
                     "  (loop: %d calls timed, scaled)" % n if P > n else ""), flush=True)


# ---- chains | mcmc: :vegasmc | :mcmc points (csrc/mci_sweep_chains.h)
def mcmc_chain_steps(npb, nchain):
    """steps of one of the bubble's :mcmc chains in a block of npb evaluations: the measured ones and the burn-in (mci_mcmc_burnin: a tenth
    of them, and for several chains at least 64 nslots + 16 (npool + 1) nd = 512 for the bubble's 5 pools of one slot and 2 integrands)"""
    from mcintegration_jl_amd._lib import lib
    steps = npb // nchain
    return steps + int(lib().mci_mcmc_burnin(steps, nchain, 5, 2, 5, 0.1))


def chains_table(Ps, nevals, chains, budget=3.0, solver="vegasmc"):
    from mcintegration_jl_amd import isa_mix
    eng = bubble_engine(bubble_point(0))
    unit = solver + "_sweep"
    eng.compile(unit)
    res = isa_mix.resources(eng.code_object(unit))["mci_" + unit]
    sweep = eng.integrate_sweep_chains if solver == "vegasmc" else eng.integrate_sweep_mcmc
    print("# bubble (4 Continuous leaves of 999 increments + Discrete(1, 4), q histogram), solver :%s, niter = %d, block = %d" % (solver, NITER, BLOCK))
    print("# mci_%s: %d VGPRs, %d bytes of scratch, %d bytes of static LDS" % (unit, res["vgpr"], res["scratch"], res["lds"]))
    print("# chain sweep | loop of ordinary calls with the same nchain, carry off | loop of default calls: ms (us per point-iteration)")
    loops = {"same": bubble_engine(bubble_point(0)), "default": bubble_engine(bubble_point(0))}
    loops["same"].set_chain_carry(0)
    g0 = [eng.grid(l).copy() for l in range(4)]
    rw0 = eng.reweight().copy()

    def timed(fn, reps=3):
        """(best, worst) of up to `reps` runs; a run longer than the budget is not repeated"""
        best, worst = float("inf"), 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            best, worst = min(best, dt), max(worst, dt)
            if dt > budget:
                break
        return (best, worst), out

    def loop(which, n, nchain, kw):
        e = loops[which]
        for k in range(n):
            for l in range(4):
                e.set_grid(l, g0[l])
            e.set_reweight(rw0)
            q = e.integrate(solver, nchain=nchain, **kw)
        return q
    for neval in nevals:
        kw = dict(neval=neval, niter=NITER, block=BLOCK, seed=SEED)
        loop("default", 1, 0, kw)                                                          # (compile, first launches)
        for nchain in chains:
            if nchain > neval // BLOCK:
                continue
            loop("same", 1, nchain, kw)
            for P in Ps:
                uds = np.array([bubble_point(k) for k in range(P)])
                sweep(solver, userdata=uds[:1], nchain=nchain, **dict(kw, niter=1))     # (first launch)
                (ts, tsw), rs = timed(lambda: sweep(solver, userdata=uds, nchain=nchain, **kw))
                assert all(r["status"] == 0 for r in rs)
                n = min(P, 16)   # (a loop is linear in P: up to 16 calls are timed, larger P scaled; ud stays point 0's, as in time_loop)
                (tl, tlw), q = timed(lambda: loop("same", n, nchain, kw))
                (td, tdw), _ = timed(lambda: loop("default", n, 0, kw))
                tl, td, tlw, tdw = tl * P / n, td * P / n, tlw * P / n, tdw * P / n
                sig = np.max(np.abs(rs[0]["mean"] - q["mean"]) / np.hypot(rs[0]["stdev"], q["stdev"]))
                deep = neval // min(nchain, 256) if solver == "vegasmc" else BLOCK * mcmc_chain_steps(neval // BLOCK, nchain)
                print("neval %8d  nchain %4d  P %4d  sweep %11.3f ms (%9.3f us; worst %11.3f)  same-nchain loop %11.3f ms (%9.3f us; worst %11.3f)"
                      "  default loop %11.3f ms (%9.3f us; worst %11.3f)"
                      "  loop / sweep %7.2f  default / sweep %7.2f   grid x threads = %s  steps deep %8d  point 0: %.1f sigma apart%s"
                      % (neval, nchain, P, 1e3 * ts, 1e6 * ts / (P * NITER), 1e3 * tsw, 1e3 * tl, 1e6 * tl / (P * NITER), 1e3 * tlw, 1e3 * td,
                         1e6 * td / (P * NITER), 1e3 * tdw, tl / ts, td / ts, eng.last_sweep_launch(), deep, sig,
                         "  (loops: %d calls timed, scaled)" % n if P > n else ""),
                      flush=True)


def carry_table(Ps, nevals, chains, budget=3.0, solver="vegasmc"):
    """carried sweep | uncarried sweep | loop of ordinary calls with the same nchain and carried chains"""
    from mcintegration_jl_amd import isa_mix
    from mcintegration_jl_amd._lib import lib
    eng = bubble_engine(bubble_point(0))
    unit = solver + "_sweep_carry"
    eng.compile(unit)
    res = isa_mix.resources(eng.code_object(unit))["mci_" + unit]
    sweep = eng.integrate_sweep_chains if solver == "vegasmc" else eng.integrate_sweep_mcmc
    print("# bubble (4 Continuous leaves of 999 increments + Discrete(1, 4), q histogram), solver :%s, niter = %d, block = %d" % (solver, NITER, BLOCK))
    print("# mci_%s: %d VGPRs, %d bytes of scratch, %d bytes of static LDS" % (unit, res["vgpr"], res["scratch"], res["lds"]))
    print("# carried sweep | uncarried sweep, same nchain | loop of ordinary calls, same nchain, carried chains: ms (us per point-iteration)")
    ordinary = bubble_engine(bubble_point(0))
    ordinary.set_chain_carry(1)
    g0 = [eng.grid(l).copy() for l in range(4)]
    rw0 = eng.reweight().copy()

    def timed(fn, reps=3):
        best, worst = float("inf"), 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            best, worst = min(best, dt), max(worst, dt)
            if dt > budget:
                break
        return (best, worst), out

    def loop(n, nchain, kw):
        for k in range(n):
            for l in range(4):
                ordinary.set_grid(l, g0[l])
            ordinary.set_reweight(rw0)
            ordinary.set_chain_carry(1)      # (drops nothing; a call's first iteration follows another problem state: starts afresh)
            q = ordinary.integrate(solver, nchain=nchain, **kw)
        return q
    for neval in nevals:
        kw = dict(neval=neval, niter=NITER, block=BLOCK, seed=SEED)
        for nchain in chains:
            if nchain > neval // BLOCK:
                continue
            loop(1, nchain, kw)                                                                # (compile, first launches)
            steps = neval // BLOCK // nchain
            if solver == "mcmc":
                fresh = BLOCK * -(-nchain // 256) * (steps + int(lib().mci_mcmc_burnin(steps, nchain, 5, 2, 5, 0.1)))
                deep = (fresh, BLOCK * -(-nchain // 256) * steps)
            else:
                deep = (BLOCK * -(-nchain // 256) * steps,) * 2
            for P in Ps:
                uds = np.array([bubble_point(k) for k in range(P)])
                for carry in (True, False):
                    sweep(solver, userdata=uds[:1], nchain=nchain, carry=carry, **dict(kw, niter=1))     # (first launch)
                (tc, tcw), rc = timed(lambda: sweep(solver, userdata=uds, nchain=nchain, carry=True, **kw))
                (tu, tuw), ru = timed(lambda: sweep(solver, userdata=uds, nchain=nchain, **kw))
                assert all(r["status"] == 0 for r in rc) and all(r["status"] == 0 for r in ru)
                n = min(P, 16)   # (a loop is linear in P: up to 16 calls are timed, larger P scaled)
                (tl, tlw), q = timed(lambda: loop(n, nchain, kw))
                tl, tlw = tl * P / n, tlw * P / n
                # (the timed loop reuses one problem, whose map has been trained by the calls before: its :vegasmc chains are carried out of a
                # call's first iteration too, plan_may_carry.  The comparison of point 0 is with a FRESH problem's call, one lane per chain.)
                fresh = bubble_engine(bubble_point(0))
                fresh.set_chain_carry(1)
                fresh.set_chain_speculation(1)
                q = fresh.integrate(solver, nchain=nchain, **kw)
                fresh.close()
                sig = np.max(np.abs(rc[0]["mean"] - q["mean"]) / np.hypot(rc[0]["stdev"], q["stdev"]))
                print("neval %8d  nchain %4d  P %4d  carried sweep %11.3f ms (%9.3f us; worst %11.3f)  uncarried sweep %11.3f ms (%9.3f us; worst %11.3f)"
                      "  carried loop %11.3f ms (%9.3f us; worst %11.3f)  uncarried / carried %6.2f  loop / carried %6.2f"
                      "   grid x threads = %s  steps deep %7d -> %7d (first iteration: %d)  correlated %s  point 0: %.1f sigma from a fresh problem's carried call%s"
                      % (neval, nchain, P, 1e3 * tc, 1e6 * tc / (P * NITER), 1e3 * tcw, 1e3 * tu, 1e6 * tu / (P * NITER), 1e3 * tuw, 1e3 * tl,
                         1e6 * tl / (P * NITER), 1e3 * tlw, tu / tc, tl / tc, eng.last_sweep_launch(), deep[0], deep[1], deep[0], rc[0]["correlated"], sig,
                         "  (loop: %d calls timed, scaled)" % n if P > n else ""),
                      flush=True)


def resume_table(Ps, nevals, chains, reps, solver="vegasmc"):
    """the continuation call with | without the chain states of the call before"""
    import inspect
    from mcintegration_jl_amd._lib import lib
    eng = bubble_engine(bubble_point(0))
    sweep = eng.integrate_sweep_chains if solver == "vegasmc" else eng.integrate_sweep_mcmc
    has_state = "state" in inspect.signature(sweep).parameters
    print("# bubble (4 Continuous leaves of 999 increments + Discrete(1, 4), q histogram), solver :%s, block = %d: a carried sweep of niter = %d, then the"
          " timed continuation call of niter = %d (maps, reweight, first_iteration = %d)" % (solver, BLOCK, NITER, NITER, NITER))
    print("# without the chain states | with them%s: ms best / median / worst over %d alternating repetitions after one warm-up call of each"
          % ("" if has_state else " (this library's sweeps take no state=: not timed)", reps))
    for neval in nevals:
        for nchain in chains:
            if nchain < 2 or nchain > neval // BLOCK:
                continue
            steps, trips = neval // BLOCK // nchain, -(-nchain // 256)
            burn = int(lib().mci_mcmc_burnin(steps, nchain, 5, 2, 5, 0.1)) if solver == "mcmc" else 0
            deep = (BLOCK * trips * (NITER * steps + burn), BLOCK * trips * NITER * steps)
            for P in Ps:
                uds = np.array([bubble_point(k) for k in range(P)])
                kw = dict(userdata=uds, neval=neval, niter=NITER, block=BLOCK, seed=SEED, nchain=nchain, carry=True)
                head = sweep(solver, **kw)
                on = dict(kw, maps=[r["maps"] for r in head], reweight=[r["reweight"] for r in head], first_iteration=NITER)
                calls = [("without", lambda: sweep(solver, **on))]
                if has_state:
                    calls.append(("with", lambda: sweep(solver, state=[r["chain_state"] for r in head], **on)))
                out, times, secs = {}, {name: [] for name, _ in calls}, {name: [] for name, _ in calls}
                for name, fn in calls:
                    fn()                                               # (warm-up: code object loaded, buffer parked with the context)
                for _ in range(reps):
                    for name, fn in calls:
                        t0 = time.perf_counter()
                        out[name] = fn()
                        times[name].append(time.perf_counter() - t0)
                        secs[name].append(out[name][0]["seconds"])
                assert all(r["status"] == 0 for rs in out.values() for r in rs)
                col = lambda ts, name: "%9.3f / %9.3f / %9.3f" % tuple(1e3 * v for v in (min(ts[name]), float(np.median(ts[name])), max(ts[name])))
                line = "neval %7d  nchain %4d  P %4d  launch: without %s" % (neval, nchain, P, col(secs, "without"))
                if has_state:
                    assert all(r["continued"] for r in out["with"]) and not any(r["continued"] for r in out["without"])
                    line += "  with %s  without / with %.3f   call: without %s  with %s  without / with %.3f   neval of point 0: %d -> %d" % (
                        col(secs, "with"), np.median(secs["without"]) / np.median(secs["with"]), col(times, "without"), col(times, "with"),
                        np.median(times["without"]) / np.median(times["with"]), out["without"][0]["neval"], out["with"][0]["neval"])
                else:
                    line += "   call: without %s" % col(times, "without")
                print(line + "   steps deep %d -> %d (derived ratio %.2f)   grid x threads = %s" % (deep[0], deep[1], deep[0] / deep[1], eng.last_sweep_launch()), flush=True)


# ---- until: a target error per point (csrc/mci_sweep.h vegas_sweep<Cfg, true>)
def until_table(Ps, nevals, rtol, reps, niter=20):
    from mcintegration_jl_amd import isa_mix
    eng = sweep_engine()
    for unit in ("vegas_sweep", "vegas_sweep_until"):
        eng.compile(unit)
        res = isa_mix.resources(eng.code_object(unit))["mci_" + unit]
        print("# mci_%s: %d VGPRs, %d bytes of scratch" % (unit, res["vgpr"], res["scratch"]))
    print("# 4-D Genz product peak, a from 2 to 8, niter = %d, block = %d, ignore = 1; %d alternating repetitions after one warm-up call of each"
          % (niter, BLOCK, reps))
    print("# fixed sweep | until, rtol = atol = 0 | until, rtol = %g: ms best / median / worst; launch = the library's clock up to the stream's synchronise, "
          "call = the Engine method's wall time" % rtol)
    for neval in nevals:
        kw = dict(neval=neval, niter=niter, block=BLOCK, seed=SEED)
        for P in Ps:
            uds = np.array([point(k) for k in range(P)])
            calls = (("fixed", lambda: eng.integrate_sweep("vegas", userdata=uds, **kw)),
                     ("zero", lambda: eng.integrate_sweep_until("vegas", userdata=uds, rtol=0.0, atol=0.0, **kw)),
                     ("until", lambda: eng.integrate_sweep_until("vegas", userdata=uds, rtol=rtol, **kw)))
            out, times, secs = {}, {name: [] for name, _ in calls}, {name: [] for name, _ in calls}
            for name, fn in calls:
                fn()                                                   # (warm-up: code object loaded, buffer parked with the context)
            for _ in range(reps):
                for name, fn in calls:
                    t0 = time.perf_counter()
                    out[name] = fn()                                   # (ends in the stream's synchronise and the host's statistics)
                    times[name].append(time.perf_counter() - t0)
                    secs[name].append(out[name][0]["seconds"])
            assert all(r["status"] == 0 for rs in out.values() for r in rs)
            assert all(r["niter_run"] == niter for r in out["zero"])
            same = all(a["iter_mean"].tobytes() == b["iter_mean"].tobytes() and a["maps"].tobytes() == b["maps"].tobytes() for a, b in zip(out["fixed"], out["zero"]))
            nrun = np.array([r["niter_run"] for r in out["until"]])
            share = nrun.sum() / float(niter * P)
            col = lambda ts, name: "%8.3f / %8.3f / %8.3f" % tuple(1e3 * v for v in (min(ts[name]), float(np.median(ts[name])), max(ts[name])))
            med, smed = {name: float(np.median(times[name])) for name in times}, {name: float(np.median(secs[name])) for name in secs}
            print("neval %7d  P %5d  launch: fixed %s  zero target %s  rtol %s   zero / fixed %.3f   until / fixed %.3f   until / perfect schedule %.2f"
                  % (neval, P, col(secs, "fixed"), col(secs, "zero"), col(secs, "until"), smed["zero"] / smed["fixed"], smed["until"] / smed["fixed"],
                     smed["until"] / (share * smed["fixed"])))
            print("                        call:   fixed %s  zero target %s  rtol %s   zero / fixed %.3f   until / fixed %.3f"
                  % (col(times, "fixed"), col(times, "zero"), col(times, "until"), med["zero"] / med["fixed"], med["until"] / med["fixed"]))
            one_each = P <= eng.last_sweep_launch()[0]         # (one point per workgroup: the launch lasts as long as its slowest point)
            print("                        iterations run %.3f of %d P (converged %d of %d points, n_p min %d median %d max %d%s)   "
                  "zero target == fixed bit for bit: %s   grid x threads = %s"
                  % (share, niter, sum(1 for r in out["until"] if r["converged"]), P, nrun.min(), int(np.median(nrun)), nrun.max(),
                     "; the slowest workgroup's share %.3f" % (nrun.max() / float(niter)) if one_each else "", same, eng.last_sweep_launch()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["table", "threads", "once", "strat", "chains", "mcmc", "until"])
    ap.add_argument("--nevals", default="10000,100000,1000000")
    ap.add_argument("--chains", default="1,16,64,256")
    ap.add_argument("--neval", type=int, default=10000)
    ap.add_argument("--points", default="1,16,256,1024,4096")
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--layout", choices=["genz", "bubble", "leaves"], default="genz")
    ap.add_argument("--rtol", type=float, default=2e-3, help="until: the target error of the timed scan")
    ap.add_argument("--carry", action="store_true", help="chains | mcmc: the sweep with carried chains against the uncarried one and a loop of carried calls")
    ap.add_argument("--resume", action="store_true", help="chains | mcmc: the continuation call of a carried sweep with and without the chain states of the call before")
    a = ap.parse_args()
    Ps = [int(v) for v in a.points.split(",")]
    mci.use_rocm_compiler()
    if a.carry and a.mode not in ("chains", "mcmc"):
        ap.error("--carry goes with the chains and mcmc modes")
    if a.mode == "until":
        until_table([256, 2048] if a.points == "1,16,256,1024,4096" else Ps, [10000, 100000] if a.nevals == "10000,100000,1000000" else [int(v) for v in a.nevals.split(",")],
                    a.rtol, a.repeat if a.repeat > 1 else 7)
        return
    if a.resume and a.mode not in ("chains", "mcmc"):
        ap.error("--resume goes with the chains and mcmc modes")
    if a.resume:
        resume_table([16, 256] if a.points == "1,16,256,1024,4096" else Ps, [10000, 100000] if a.nevals == "10000,100000,1000000" else [int(v) for v in a.nevals.split(",")],
                     [16, 64, 256] if a.chains == "1,16,64,256" else [int(v) for v in a.chains.split(",")], a.repeat if a.repeat > 1 else 5,
                     solver="vegasmc" if a.mode == "chains" else "mcmc")
        return
    if a.mode in ("chains", "mcmc"):
        (carry_table if a.carry else chains_table)([P for P in Ps if P <= 256] if a.points == "1,16,256,1024,4096" else Ps, [int(v) for v in a.nevals.split(",")],
                     [int(v) for v in a.chains.split(",")], solver="vegasmc" if a.mode == "chains" else "mcmc")
        return
    if a.layout == "leaves":
        if a.mode != "strat":
            ap.error("--layout leaves goes with the strat mode")
        strat_leaves_table([P for P in Ps if P <= 256] if a.points == "1,16,256,1024,4096" else Ps,
                           [10000, 100000] if a.nevals == "10000,100000,1000000" else [int(v) for v in a.nevals.split(",")])
        return
    if a.mode == "strat":
        strat_table([P for P in Ps if P <= 1024] if a.points == "1,16,256,1024,4096" else Ps, a.neval)
        return
    if a.layout == "bubble":
        if a.mode != "table":
            ap.error("--layout bubble goes with the table mode")
        bubble_table(Ps, a.neval)
        return
    if a.mode == "once":
        eng = sweep_engine(a.threads)
        t, _ = time_sweep(eng, Ps[0], a.neval, reps=1)
        print("sweep P = %d neval = %d: %.3f ms, grid x threads = %s" % (Ps[0], a.neval, 1e3 * t, eng.last_sweep_launch()))
        return
    if a.mode == "threads":
        print("# sweep, neval = %d, niter = %d, block = %d: ms per call (us per point-iteration) by threads per workgroup" % (a.neval, NITER, BLOCK))
        engines, refused = {T: sweep_engine(T) for T in (256, 512, 1024)}, set()
        for rep in range(a.repeat):
            for T, eng in engines.items():
                for P in Ps:
                    if T in refused:
                        break
                    try:
                        t, _ = time_sweep(eng, P, a.neval)
                        print("pass %d  threads %4d  P %5d  %9.3f ms  (%7.3f us)  grid x threads = %s"
                              % (rep, T, P, 1e3 * t, 1e6 * t / (P * NITER), eng.last_sweep_launch()))
                    except mci.MCIError as e:
                        print("pass %d  threads %4d  P %5d  refused: %s" % (rep, T, P, str(e).splitlines()[0]))
                        refused.add(T)
        return
    print("# neval = %d, niter = %d, block = %d: sweep | loop of persistent calls, ms (us per point-iteration) | loop / sweep" % (a.neval, NITER, BLOCK))
    eng = sweep_engine(a.threads)
    for P in Ps:
        ts, rs = time_sweep(eng, P, a.neval)
        tl, means = time_loop(P, a.neval)
        same = abs(rs[0]["mean"][0] - means[0]) / abs(means[0])      # (point 0 is the same integral on both sides)
        print("P %5d  sweep %10.3f ms (%8.3f us)  loop %10.3f ms (%8.3f us)  loop / sweep %7.2f   point 0: means differ by %.1e%s"
              % (P, 1e3 * ts, 1e6 * ts / (P * NITER), 1e3 * tl, 1e6 * tl / (P * NITER), tl / ts, same, "  (loop: 256 calls timed, scaled)" if P > 256 else ""))


if __name__ == "__main__":
    main()
