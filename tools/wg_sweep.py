#!/usr/bin/env python3
"""Development tool (GPU box): the headline workload of bench.py (16-D Gaussian, :vegas, 1e8 samples in 16 blocks) at forced workgroup
counts -- ms per step of the library loop (run + finish, as bench.py times it) and the sample kernel's own HIP-event duration.
Every setting is measured `rounds` times, the settings interleaved, so that clock drift lands on all of them alike.
usage: python tools/wg_sweep.py [--rounds R] [--steps K] [--passes P] [workgroups ...]      (0 = the launch rule's own choice)"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import mcintegration_jl_amd as mci

mci.use_rocm_compiler()
import torch  # noqa: E402  (as bench.py: the HIP runtime of the process is PyTorch's)

args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


rounds, steps, passes = opt("--rounds", 3), opt("--steps", 20), opt("--passes", 25)
grids = [int(x) for x in args] or [512, 1024, 2048, 4096, 0]
D, L, block, neval, seed = 16, math.sqrt(50.0), 16, 10 ** 8, 20240229
cfg = mci.Configuration(var=mci.Continuous(-L, L), dof=[[D]], seed=seed)
mci.integrate(mci.catalog.gaussian(D), config=cfg, solver="vegas", neval=neval, niter=5, block=block, adapt=True)
eng = cfg._engine
eng.reserve_iterations(steps * (passes + 1) * rounds * len(grids) + 64)
npb = neval // block
res = {g: {"step": [], "kern": [], "wg": None} for g in grids}
for r in range(rounds):
    for g in grids:
        eng.set_launch(0, g // block)
        dts = []
        for ip in range(passes + 1):   # (the first pass of a setting is its warm-up)
            it0 = cfg.iterations_done
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(steps):
                eng.run("vegas", npb, 0, block, it0 + it, cfg.seed)
                eng.finish("vegas", block, adapt=True, want_stats=False)
            torch.cuda.synchronize()
            if ip:
                dts.append((time.perf_counter() - t0) / steps * 1e3)
            cfg.iterations_done += steps
        kms, wgs, threads = eng.kernel_times_ms(steps * passes)
        res[g]["step"].append(float(np.median(dts)))
        res[g]["kern"].append(float(np.mean(kms)))
        res[g]["wg"] = (wgs, threads)
eng.check_status()
print("workgroups x threads   ms_per_step (median pass) per round        kernel_ms_avg per round")
for g in grids:
    v = res[g]
    print("%5d x %-4d %s   %s   | median %.4f  kernel %.4f" % (v["wg"][0], v["wg"][1], " ".join("%.4f" % x for x in v["step"]),
                                                              " ".join("%.4f" % x for x in v["kern"]), float(np.median(v["step"])),
                                                              float(np.median(v["kern"]))), flush=True)
eng.close()
cfg._engine = None
mci.shutdown()
