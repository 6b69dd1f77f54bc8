#!/usr/bin/env python3
"""The carried VEGAS+ allocation (Stratify(carry=True), mci_set_stratification_carry) against the default, on the train-then-freeze
recipe: benchmark1.jl's Watson integral trained at neval = 2e5 x 10 iterations, then measured at 2e5 x 10 with adapt=False on the
same Configuration -- carried (the production call runs on the allocation the training learned) and not carried (it stratifies
evenly), seed by seed; and the time of remap + allocation at 2^24 hypercubes (two draws, N = 2^25), which runs once per call: HIP
events around the run that starts the allocation, less the same run without it.

    python tools/strat_carry_bench.py [--out profiles/r09_strat_carry.txt] [--seeds 32]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mcintegration_jl_amd as mci  # noqa: E402

WATSON = "w[0] = 1.0 / (1.0 - cos(x[0]) * cos(x[1]) * cos(x[2])) / (M_PI * M_PI * M_PI);"
EXACT = 1.3932039297


def watson_cfg(seed):
    return mci.Configuration(var=mci.Continuous(0.0, math.pi, alpha=3.0), dof=[[3]], seed=seed)


def train_then_freeze(seed, carry):
    st = mci.Stratify(carry=carry)
    res = mci.integrate(WATSON, config=watson_cfg(seed), solver="vegas", neval=2e5, niter=10, stratify=st)
    r = mci.integrate(WATSON, config=res.config, solver="vegas", neval=2e5, niter=10, adapt=False, stratify=st)
    return r.mean[0], r.stdev[0], r.stratification["carried"]


def watson(P, nseed):
    rows = {c: [train_then_freeze(s, c) for s in range(1, nseed + 1)] for c in (True, False)}
    P("# Watson integral (benchmark1, exact %.10f), default plan (29^3 = 24389 hypercubes at neval = 2e5), beta = 0.75" % EXACT)
    P("# train: neval 2e5 x 10 iterations; production: neval 2e5 x 10 iterations, adapt=False, config=res.config")
    P("# seed | carried: mean, reported error (start) | not carried: mean, reported error (start) | ratio of the reported errors")
    for s in range(nseed):
        a, b = rows[True][s], rows[False][s]
        P("%2d  %.8f %.4g (%s)   %.8f %.4g (%s)   %.3f" % (s + 1, a[0], a[1], a[2], b[0], b[1], b[2], a[1] / b[1]))
    for n in sorted({min(8, nseed), nseed}):
        m, e = (np.array([r[k] for r in rows[True][:n]]) for k in (0, 1))
        m0, e0 = (np.array([r[k] for r in rows[False][:n]]) for k in (0, 1))
        pooled, pooled0 = math.sqrt(np.mean(e * e)), math.sqrt(np.mean(e0 * e0))
        rms, rms0 = math.sqrt(np.mean((m - EXACT) ** 2)), math.sqrt(np.mean((m0 - EXACT) ** 2))
        P("seeds 1 .. %d: pooled reported error  carried %.4g  not carried %.4g  ratio %.3f" % (n, pooled, pooled0, pooled / pooled0))
        P("    scatter of the means  carried %.4g (%.2f x its mean reported error)  not carried %.4g (%.2f x)  ratio %.3f" % (
            np.std(m, ddof=1), np.std(m, ddof=1) / e.mean(), np.std(m0, ddof=1), np.std(m0, ddof=1) / e0.mean(), np.std(m, ddof=1) / np.std(m0, ddof=1)))
        P("    rms deviation from the exact value  carried %.4g  not carried %.4g  ratio %.3f" % (rms, rms0, rms / rms0))


def remap_cost(P):
    import torch
    from mcintegration_jl_amd._lib import lib
    from mcintegration_jl_amd.engine import context
    N = 2 ** 25
    P("# remap + allocation at 2^24 hypercubes, once per call (x2y2, two draws, N = 2^25; one run each)")
    for plan_a, plan_b, beta_b in (((2048, 2048), (4096, 4096), 0.75), ((4096, 4096), (4096, 4096), 0.5)):
        eng = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=1), mci.catalog.x2y2())
        stream = torch.cuda.ExternalStream(lib().mci_ctx_stream(context(eng.device)))
        eng.set_stratification(nstrat=list(plan_a), carry=True)
        eng.integrate("vegas", N, niter=2, block=16, seed=1)
        eng.set_stratification(nstrat=list(plan_b), beta=beta_b, carry=True)
        ms, wall, how = [], [], None
        for k in range(3):   # k = 0: remap + allocation + sample launch; k = 1, 2: the sample launch alone (adapt=False keeps the allocation)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            eng.run("vegas", N // 16, 0, 16, 2 + k, 1)
            e1.record(stream)
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
            eng.finish("vegas", 16, adapt=False)
            how = eng.strat_carry() if k == 0 else how
        P("%s -> %s, beta 0.75 -> %g (%s): run that starts the allocation %.3f ms (HIP events; wall %.3f), sample launch alone %.3f | %.3f ms "
          "(wall %.3f | %.3f): remap + allocation + new buffers = %.3f ms" % (plan_a, plan_b, beta_b, eng.CARRIED[how[1]], ms[0], wall[0], ms[1], ms[2],
                                                                             wall[1], wall[2], ms[0] - min(ms[1:])))
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--skip-remap", action="store_true")
    a = ap.parse_args()
    mci.use_rocm_compiler()
    fh = open(a.out, "w") if a.out else None

    def P(s):
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()
    watson(P, a.seeds)
    if not a.skip_remap:
        remap_cost(P)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
