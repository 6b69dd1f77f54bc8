"""A parameter scan as ONE launch: the 4-D Genz product peak  prod_d 1 / (a^-2 + (x_d - u_d)^2)  over its sharpness `a`.

The closure reads its parameters off `config.userdata` (a struct of floats); mci.integrate_sweep traces it once, evaluates every
point's parameters from its object, and runs all points in one launch -- one workgroup per point runs that point's whole :vegas loop.
Every result is what mci.integrate(peak, userdata=that object, ...) returns on a fresh configuration; all points share the seed, so the
curve over `a` is smooth (common random numbers).

Reference pattern:  for a in as;  integrate((x, c) -> ...; userdata = Para(a, u), var = Continuous(0, 1), dof = [[4]], solver = :vegas)  end"""
import math
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcintegration_jl_amd as mci  # noqa: E402

D = 4


def peak(x, c):
    p = c.userdata
    q = 1.0
    for d in range(D):
        t = x[d] - p.u[d]
        q = q * (1.0 / (p.a * p.a) + t * t)
    return 1.0 / q


def exact(p):
    return math.prod(p.a * (math.atan(p.a * (1.0 - u)) + math.atan(p.a * u)) for u in p.u)


def main(points=64):
    u = np.array([0.3 + 0.4 * d / (D - 1) for d in range(D)])
    scan = [types.SimpleNamespace(a=float(a), u=u) for a in np.linspace(2.0, 8.0, points)]
    results = mci.integrate_sweep(peak, params=scan, var=mci.Continuous(0.0, 1.0), dof=[[D]], solver="vegas", neval=1e4, niter=10, seed=7)
    print("batched:", all(r.sweep_batched for r in results), "| %.2f ms for %d points" % (1e3 * results[0].seconds, len(scan)))
    for p, r in list(zip(scan, results))[::max(1, points // 8)]:
        print("a = %5.2f   %12.5f +- %-10.5f  exact %12.5f  (%+.1f sigma)" % (p.a, r.mean[0], r.stdev[0], exact(p), (r.mean[0] - exact(p)) / r.stdev[0]))
    return scan, results


if __name__ == "__main__":
    main()
