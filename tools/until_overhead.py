#!/usr/bin/env python3
"""Development tool (GPU box): what a target error costs an ordinary integrate() call (mci_integrate_until), by the library's own clock
(mci_result.seconds: first launch to the last synchronisation), per iteration that was run.

    fixed   the fixed call: default-size :vegas as one persistent launch, and the launch chain at neval = 1e4 and 1e6
    zero    the same three calls with rtol = atol = 0 next to the fixed ones: the price of the rule alone (it never stops)
    genz    the five 4-D Genz points of tests/until_cases.py at niter = 20: rtol = 2e-3 against the fixed call, persistent and launch chain

--root DIR imports the package from another checkout (the parent commit's tree, for `fixed` in alternating repetitions)."""
import argparse
import os
import sys

import numpy as np

D = 4
SEED = 20240229


def point(k):   # tests/test_hip_sweep.py point(k)
    rng = np.random.default_rng(1000 + k)
    return [float(D), 2.0 + 6.0 * ((k * 0.37) % 1.0)] + list(0.3 + 0.4 * rng.random(D))


def engine(mci, ud, mode):
    cfg = mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[D]], seed=SEED)
    eng = mci.Engine(cfg, mci.Integrand(mci.catalog.genz_product_peak(D).body, list(ud), "genz_product_peak%d" % D))
    eng.set_persistent(mode)
    return eng


def per_iteration(eng, reps, first=0, **kw):
    """median, min (us per iteration run) over reps calls, the iterations a call ran, whether the last one was persistent"""
    ts, n = [], kw["niter"]
    for i in range(reps + 3):
        r = eng.integrate("vegas", seed=SEED, first_iteration=first, **kw)
        n = r.get("niter_run", kw["niter"])
        if i >= 3:
            ts.append(r["seconds"] / n * 1e6)
    return np.median(ts), np.min(ts), n, eng.last_integrate_persistent()


SHAPES = [("persistent, neval 1e4", "on", 10000, 200), ("launch chain, neval 1e4", "off", 10000, 200), ("launch chain, neval 1e6", "off", 1000000, 40)]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["fixed", "zero", "genz"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import mcintegration_jl_amd as mci
    if a.mode in ("fixed", "zero"):
        for name, mode, neval, reps in SHAPES:
            eng = engine(mci, point(0), mode)
            kw = dict(neval=neval, niter=10, block=16)
            med, lo, n, pers = per_iteration(eng, reps, **kw)
            line = "%-8s %-24s fixed %7.2f us / iteration (min %7.2f, %d calls, persistent %s)" % (a.tag, name, med, lo, reps, pers)
            if a.mode == "zero":
                med0, lo0, n0, pers0 = per_iteration(eng, reps, target=(0.0, 0.0, 0), **kw)
                assert n0 == 10
                line += " | rtol = atol = 0: %7.2f us / iteration (min %7.2f, persistent %s)" % (med0, lo0, pers0)
            print(line, flush=True)
    else:
        for mode in ("on", "off"):
            for k in (0, 1, 3, 4, 6):
                kw = dict(neval=16000, niter=20, block=16)
                # every repetition from the same untrained map: a fresh engine's first call, 20 of them
                tf, tu, nu = [], [], 0
                for rep in range(20):
                    e = engine(mci, point(k), mode)
                    e.integrate("vegas", seed=SEED, **dict(kw, niter=1, adapt=False, ignore=0))                    # (loads the code object)
                    tf.append(e.integrate("vegas", seed=SEED, **kw)["seconds"] * 1e6)
                    e = engine(mci, point(k), mode)
                    e.integrate("vegas", seed=SEED, target=(0.0, 0.0, 0), **dict(kw, niter=1, adapt=False, ignore=0))
                    r = e.integrate("vegas", seed=SEED, target=(2e-3, 0.0, 0), **kw)
                    tu.append(r["seconds"] * 1e6)
                    nu, pers = r["niter_run"], e.last_integrate_persistent()
                print("%-8s genz k = %d, %-12s fixed niter = 20: %8.1f us | rtol = 2e-3: %8.1f us, %2d iterations run (converged %s, %d samples discarded)"
                      % (a.tag, k, "persistent" if pers else "launch chain", np.median(tf), np.median(tu), nu, r["converged"], r["neval_discarded"]), flush=True)
