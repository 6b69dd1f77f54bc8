#!/usr/bin/env python3
"""Stratified :vegas (VEGAS+, integrate(..., stratify=...)) against classic :vegas at equal neval and niter: sigma, wall time and
sigma^2 * time on benchmark1.jl's Watson integral, benchmark4.jl's 4-D Gaussian and C2 (16-D Gaussian, neval = 1e8); the sample
kernels' rates from their HIP-event times; the time the allocation and reduce launches add per iteration (the stratified iteration's
wall time less its sample kernel); and whether the reported errors are honest: over --cov-seeds seeds, the scatter of the final means
against the mean reported error, classic and stratified (default plan, beta = 0.75 and beta = 0, and the old two-samples-per-hypercube
plan), on benchmark1, benchmark4 and C1 (log(x)/sqrt(x)); C2 at neval = 1e6 iteration by iteration.

    python tools/strat_bench.py [--out profiles/r07_stratified.txt] [--c2-neval 1e8]
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mcintegration_jl_amd as mci  # noqa: E402

L = math.sqrt(50.0)
WATSON = "w[0] = 1.0 / (1.0 - cos(x[0]) * cos(x[1]) * cos(x[2])) / (M_PI * M_PI * M_PI);"
GAUSS4 = ("double s = 0.0; for (int d = 0; d < 4; ++d) { const double t = x[d] - 0.5; s += t * t; } "
          "w[0] = exp(-100.0 * s) * 1013.2118364296088;")


def cases(c2_neval):
    return [
        ("benchmark1 Watson 3-D", WATSON, lambda s: mci.Configuration(var=mci.Continuous(0.0, math.pi, alpha=3.0), dof=[[3]], seed=s), 2e5, 10,
         1.3932039297),
        ("benchmark4 Gaussian 4-D", GAUSS4, lambda s: mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]], seed=s), 1e5, 10, 1.0),
        ("C2 Gaussian 16-D", mci.catalog.gaussian(16), lambda s: mci.Configuration(var=mci.Continuous(-L, L), dof=[[16]], seed=s), c2_neval, 10,
         math.erf(5.0) ** 16),
    ]


def run(f, cfg, neval, niter, stratify):
    mci.integrate(f, config=cfg, solver="vegas", neval=neval, niter=2, stratify=stratify)   # compile + warm
    cfg.iterations_done = 0
    t0 = time.perf_counter()
    res = mci.integrate(f, config=cfg, solver="vegas", neval=neval, niter=niter, stratify=stratify)
    return res, time.perf_counter() - t0


LOGSQRT = "w[0] = log(x[0]) / sqrt(x[0]);"


def coverage(nseed):
    out = ["# reported errors against the scatter of the final means over %d seeds (neval per iteration, niter = 10, ignore = 1): scatter / mean "
           "reported sigma ~ 1 is an honest error; 'gain' = scatter / classic scatter" % nseed]
    cov = [("benchmark1 Watson", WATSON, lambda s: mci.Configuration(var=mci.Continuous(0.0, math.pi, alpha=3.0), dof=[[3]], seed=s), 2e5, 1.3932039297),
           ("benchmark4 Gauss4", GAUSS4, lambda s: mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[4]], seed=s), 1e5, 1.0),
           ("C1 log(x)/sqrt(x)", LOGSQRT, lambda s: mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[1]], seed=s), 1e5, -4.0)]
    for name, f, mk, neval, exact in cov:
        base = None
        # the plan of neval/2 hypercubes, two samples each (mci_strat_plan's rule with neval/2 in place of neval/8)
        ndim = int(sum(mk(1).maxdof))
        ns = (C.c_int32 * ndim)()
        mci.lib().mci_strat_plan(int(neval) * 4, ndim, int(neval) // 2, ns)
        for label, st in (("classic", None), ("default plan", True), ("default plan, beta 0", mci.Stratify(beta=0.0)),
                          ("2 per hypercube", mci.Stratify(nstrat=list(ns)))):
            m, e = [], []
            for seed in range(1, nseed + 1):
                r = mci.integrate(f, config=mk(seed), solver="vegas", neval=neval, niter=10, stratify=st)
                m.append(r.mean[0])
                e.append(r.stdev[0])
            m, e = np.array(m), np.array(e)
            sc = m.std(ddof=1)
            base = sc if base is None else base
            out.append("  %-18s %-22s neval %7.0e | scatter %-10.4g mean sigma %-10.4g scatter/sigma %5.2f | mean z^2 %6.2f  max |z| %5.1f | gain %.3f" % (
                name, label, neval, sc, e.mean(), sc / e.mean(), (((m - exact) / e) ** 2).mean(), np.abs((m - exact) / e).max(), sc / base))
    L2 = math.sqrt(50.0)
    for label, st in (("classic", None), ("default plan", True)):
        r = mci.integrate(mci.catalog.gaussian(16), config=mci.Configuration(var=mci.Continuous(-L2, L2), dof=[[16]], seed=1), solver="vegas",
                          neval=1e6, niter=12, stratify=st)
        out.append("  C2 at neval 1e6, seed 1, %-13s iteration means %s" % (label, " ".join("%.4f" % v for v in r.iter_mean[:, 0])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_stratified.txt"))
    ap.add_argument("--c2-neval", type=float, default=1e8)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--cov-seeds", type=int, default=32)
    args = ap.parse_args()
    mci.use_rocm_compiler()
    lines = ["# stratified :vegas (VEGAS+, stratify=True: default plan, beta = 0.75) vs classic :vegas at equal neval / niter",
             "# tools/strat_bench.py on one MI355X; sigma = Result.stdev (ignore = 1), time = wall seconds of the integrate() call (warm)",
             "# %-26s %9s %4s %5s | %-12s %-12s %9s | %-12s %-12s %9s | %8s %10s" % (
                 "case", "neval", "nit", "seed", "classic sig", "z", "s", "strat sig", "z", "s", "sig ratio", "s2t ratio")]
    summary = {}
    for name, f, mk, neval, niter, exact in cases(args.c2_neval):
        for seed in range(1, args.seeds + 1):
            rc, tc = run(f, mk(seed), neval, niter, None)
            rs, ts = run(f, mk(seed), neval, niter, True)
            sr = rs.stdev[0] / rc.stdev[0]
            s2t = (rs.stdev[0] ** 2 * ts) / (rc.stdev[0] ** 2 * tc)
            summary.setdefault(name, []).append((sr, s2t))
            plan = rs.stratification
            lines.append("  %-26s %9.0e %4d %5d | %-12.4g %-12.3f %9.4f | %-12.4g %-12.3f %9.4f | %8.3f %10.3f" % (
                name, neval, niter, seed, rc.stdev[0], (rc.mean[0] - exact) / rc.stdev[0], tc, rs.stdev[0], (rs.mean[0] - exact) / rs.stdev[0],
                ts, sr, s2t))
        lines.append("  %-26s geometric mean over seeds: sigma ratio %.3f, sigma^2*time ratio %.3f   (%d hypercubes: %.1f samples each, "
                     "%.1f %% of the samples follow the variance)" % (
                         name, math.exp(np.mean([math.log(a) for a, _ in summary[name]])), math.exp(np.mean([math.log(b) for _, b in summary[name]])),
                         plan["ncube"], neval / plan["ncube"], 100.0 * (neval - 2 * plan["ncube"]) / neval))
    # kernel rates: HIP-event times of the sample launches of one iteration each (C2 layout)
    lines.append("# sample kernels, C2 layout, neval = %.0e: kernel ms per iteration (HIP events), Gsamples/s" % args.c2_neval)
    for label, strat in (("mci_vegas_batch", None), ("mci_vegas_strat", True)):
        cfg = mci.Configuration(var=mci.Continuous(-L, L), dof=[[16]], seed=1)
        mci.integrate(mci.catalog.gaussian(16), config=cfg, solver="vegas", neval=args.c2_neval, niter=2, stratify=strat)
        eng = cfg._engine
        eng.set_kernel_timing(1)
        t0 = time.perf_counter()
        mci.integrate(mci.catalog.gaussian(16), config=cfg, solver="vegas", neval=args.c2_neval, niter=5, stratify=strat)
        wall = (time.perf_counter() - t0) / 5
        ms = np.asarray(eng.kernel_times_ms(5)[0])
        k = float(np.median(ms)) if ms.size else float("nan")
        lines.append("  %-16s kernel %.3f ms  %.1f Gsamples/s   wall per iteration %.3f ms   (wall - kernel: %.3f ms: merge, train!%s)" % (
            label, k, args.c2_neval / (k * 1e-3) / 1e9, wall * 1e3, wall * 1e3 - k, ", k_strat_reduce, k_strat_alloc" if strat else ""))
    lines += coverage(args.cov_seeds)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
