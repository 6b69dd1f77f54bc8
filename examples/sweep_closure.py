"""A parameter scan as ONE launch: the 4-D Genz product peak  prod_d 1 / (a^-2 + (x_d - u_d)^2)  over its sharpness `a`.

The closure reads its parameters off `config.userdata` (a struct of floats); mci.integrate_sweep traces it once, evaluates every
point's parameters from its object, and runs all points in one launch -- one workgroup per point runs that point's whole :vegas loop.
Every result is what mci.integrate(peak, userdata=that object, ...) returns on a fresh configuration; all points share the seed, so the
curve over `a` is smooth (common random numbers).  `stratified()` runs the same scan with stratify=True (VEGAS+ at every point, still one
launch) and then freezes what it learned for a second scan.  `stratified_two_types()` is one short stratified scan over two variable
types with ranges of their own: `leaves="all"` lets it run as one launch too.

Reference pattern:  for a in as;  integrate((x, c) -> ...; userdata = Para(a, u), var = Continuous(0, 1), dof = [[4]], solver = :vegas)  end

Then the reference's flagship example, the polarisation bubble (test/bubble.jl:12-133; the closures of examples/bubble_closure.py), scanned
over the density parameter rs at a fixed dimensionless temperature: kF, the external momenta and the imaginary-time domain (0, beta)
follow rs.  Four Continuous variable types, a Discrete external-momentum index and a histogram over it: `leaves="all"` lets such a
problem run as a sweep.  The momenta are a table the integrand looks up by the Discrete draw (every point's row carries its own), and
every point starts from a map of its own -- its T grid spans its own (0, beta).  `bubble_scan(solver="vegasmc", chains=64)` runs the
same scan under the reference's default solver: 64 fresh chains per block and point, still one launch.  `bubble_scan(solver="mcmc",
mcmc_chains=64)` runs it under :mcmc, the solver the reference runs this example with: the closures are then called in that solver's
form, integrand(idx, var, config) and measure(idx, var, obs, relative_weight, config), and every point reports its longest holding
time.  `bubble_train_then_produce()` is a training scan followed by a production scan that goes on from it: maps, reweight factors AND
chains (carry=True, chain_state=), so the production scan's first iteration neither starts its chains afresh nor burns them in."""
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


def stratified(points=64):
    """the same scan with VEGAS+ adaptive stratified sampling at every point (stratify=True: what mci.integrate(..., stratify=True) runs),
    still one launch; then train-then-freeze over the whole scan: the maps and hypercube allocations the first scan learned, kept
    (adapt=False) for a second one under other seeds"""
    u = np.array([0.3 + 0.4 * d / (D - 1) for d in range(D)])
    scan = [types.SimpleNamespace(a=float(a), u=u) for a in np.linspace(2.0, 8.0, points)]
    kw = lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[D]], solver="vegas", neval=1e4, niter=10)   # (a variable object per call: a bound one belongs to its engine)
    trained = mci.integrate_sweep(peak, params=scan, stratify=True, seed=7, **kw())
    s = trained[0].stratification
    print("stratified, batched:", all(r.sweep_batched for r in trained), "| nstrat %s (%d hypercubes) | %.2f ms for %d points"
          % (s["nstrat"], s["ncube"], 1e3 * trained[0].seconds, len(scan)))
    frozen = mci.integrate_sweep(peak, params=scan, stratify=True, adapt=False, alloc=[r.strat_d for r in trained], maps=[r.map for r in trained],
                                 seeds=[100 + k for k in range(points)], **kw())
    for p, r, f in list(zip(scan, trained, frozen))[::max(1, points // 8)]:
        print("a = %5.2f   adapting %12.5f +- %-10.5f  frozen (%s) %12.5f +- %-10.5f  exact %12.5f" % (p.a, r.mean[0], r.stdev[0], f.stratification["carried"],
                                                                                                     f.mean[0], f.stdev[0], exact(p)))
    return scan, trained, frozen


def ellipse(X, c):
    x, y = X
    return x[0] ** 2 + c.userdata.a * y[0] ** 2


def stratified_two_types(points=8):
    """a stratified scan over two Continuous variable types, x in (0, 1) and y in (0, 2), each with a grid of its own: with leaves="all"
    the points run as ONE launch (without it they would run as integrate(..., stratify=True) calls, one after another)"""
    scan = [types.SimpleNamespace(a=float(a)) for a in np.linspace(0.5, 2.0, points)]
    results = mci.integrate_sweep(ellipse, params=scan, stratify=True, leaves="all", var=(mci.Continuous(0.0, 1.0), mci.Continuous(0.0, 2.0)),
                                  solver="vegas", neval=2e4, niter=5, seed=7)
    print("stratified over two variable types, batched:", all(r.sweep_batched for r in results), "| grids of",
          [len(g) for g in results[0].maps_by_leaf], "points")
    for p, r in zip(scan, results):
        print("a = %5.2f   %10.6f +- %-9.6f  exact %10.6f" % (p.a, r.mean[0], r.stdev[0], 2.0 / 3.0 + 8.0 * p.a / 3.0))
    return scan, results


PI = math.pi


def green(tau, omega, beta):                                                 # test/bubble.jl:40-51
    if tau >= 0.0:
        return np.exp(-omega * tau) / (1 + np.exp(-omega * beta)) if omega > 0.0 else np.exp(omega * (beta - tau)) / (1 + np.exp(omega * beta))
    return -np.exp(-omega * (tau + beta)) / (1 + np.exp(-omega * beta)) if omega > 0.0 else -np.exp(-omega * tau) / (1 + np.exp(omega * beta))


def bubble(vars, config):                                                    # test/bubble.jl:53-78
    R, Theta, Phi, T, Ext = vars
    para = config.userdata
    kF, beta, me = para.kF, para.beta, para.me
    r = R[0] / (1 - R[0])
    theta, phi = Theta[0], Phi[0]
    k = np.array([r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)])
    factor = 1.0 / (2 * PI) ** para.dim
    factor *= r ** 2 / (1 - R[0]) ** 2 * np.sin(theta)
    q = para.extQ[Ext[0] - 1]                                                # external momentum: a table looked up by the Discrete draw
    kq = k + q
    g1 = green(T[0], (np.dot(k, k) - kF ** 2) / (2 * me), beta)
    g2 = green(-T[0], (np.dot(kq, kq) - kF ** 2) / (2 * me), beta)
    return g1 * g2 * para.spin * factor


def q_histogram(vars, obs, weight, config):                                  # test/bubble.jl:84-88
    Ext = vars[-1]
    obs[0][Ext[0] - 1] += weight[0]


def bubble_mcmc(idx, vars, config):                                           # integrand(idx, var, config): mcmc/montecarlo.jl:34
    return bubble(vars, config)


def q_histogram_mcmc(idx, vars, obs, relative_weight, config):               # measure(idx, var, obs, relative_weight, config): :166-169
    Ext = vars[-1]
    obs[0][Ext[0] - 1] += relative_weight


def bubble_para(rs, beta=25.0, spin=2, Qsize=4, dim=3, me=0.5):             # test/bubble.jl:12-22
    kF = (9 * PI / (2 * spin)) ** (1 / 3) / rs
    return types.SimpleNamespace(rs=rs, kF=kF, beta=beta / (kF ** 2 / 2 / me), me=me, spin=spin, dim=dim, Qsize=Qsize,
                                 extQ=[np.array([q, 0.0, 0.0]) for q in np.linspace(0.0, 1.5 * kF, Qsize)])


def bubble_scan(points=16, ninc=1000, solver="vegas", chains=None, mcmc_chains=None):
    scan = [bubble_para(float(rs)) for rs in np.linspace(1.0, 2.0, points)]
    Qsize = scan[0].Qsize
    var = (mci.Continuous(0.0, 1.0, alpha=3.0), mci.Continuous(0.0, PI, alpha=3.0), mci.Continuous(0.0, 2 * PI, alpha=3.0),
           mci.Continuous(0.0, scan[0].beta, alpha=3.0), mci.Discrete(1, Qsize, adapt=False))
    # a point's starting map, leaf by leaf (Engine.sweep_map_doubles): four grids, then the Discrete leaf's accumulation and distribution
    uniform = np.full(Qsize, 1.0 / Qsize)
    maps = [np.concatenate([np.linspace(0.0, hi, ninc) for hi in (1.0, PI, 2 * PI, p.beta)] + [np.concatenate([[0.0], np.cumsum(uniform)]), uniform])
            for p in scan]
    f, measure = (bubble_mcmc, q_histogram_mcmc) if solver == "mcmc" else (bubble, q_histogram)
    results = mci.integrate_sweep(f, params=scan, leaves="all", maps=maps, measure=measure, var=var, dof=[[1, 1, 1, 1, 1]],
                                  obs=[np.zeros(Qsize)], solver=solver, chains=chains, mcmc_chains=mcmc_chains, neval=1e5, niter=10, seed=7)
    print("bubble (%s) batched:" % solver, all(r.sweep_batched for r in results), "| %.2f ms for %d points" % (1e3 * results[0].seconds, len(scan)))
    if chains is not None or mcmc_chains is not None:   # the chain solver's own state, point by point
        print("reweight factors of the first and the last point:", results[0].reweight, results[-1].reweight)
    if mcmc_chains is not None:   # (report(result) says so where 16 x the longest hold exceeds a chain's measured steps)
        print("longest holding time (upper bound) over the points: %d of %d measured steps per chain"
              % (max(r.hold_max for r in results), results[0].chain_steps))
    print("%6s  %s" % ("rs", "  ".join("q = %.1f kF: avg +- err      " % (q[0] / scan[0].kF) for q in scan[0].extQ)))
    for p, r in list(zip(scan, results))[::max(1, points // 8)]:
        print("%6.3f  %s" % (p.rs, "  ".join("%12.6f +- %-10.6f" % (r.mean[0][i], r.stdev[0][i]) for i in range(Qsize))))
    return scan, results


def bubble_train_then_produce(points=16, ninc=1000, mcmc_chains=64):
    """train, then production, under :mcmc with carried chains: the second scan takes every point's map, factors and chain state from the
    first, keeps the maps (adapt=False) and measures more; its iterations are numbered on from the first scan's by themselves"""
    scan = [bubble_para(float(rs)) for rs in np.linspace(1.0, 2.0, points)]
    Qsize = scan[0].Qsize
    var = lambda: (mci.Continuous(0.0, 1.0, alpha=3.0), mci.Continuous(0.0, PI, alpha=3.0), mci.Continuous(0.0, 2 * PI, alpha=3.0),
                   mci.Continuous(0.0, scan[0].beta, alpha=3.0), mci.Discrete(1, Qsize, adapt=False))
    uniform = np.full(Qsize, 1.0 / Qsize)
    maps = [np.concatenate([np.linspace(0.0, hi, ninc) for hi in (1.0, PI, 2 * PI, p.beta)] + [np.concatenate([[0.0], np.cumsum(uniform)]), uniform])
            for p in scan]
    kw = lambda: dict(params=scan, leaves="all", measure=q_histogram_mcmc, var=var(), dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(Qsize)], solver="mcmc",
                      mcmc_chains=mcmc_chains, carry=True, seed=7)
    head = mci.integrate_sweep(bubble_mcmc, maps=maps, neval=1e4, niter=5, **kw())
    tail = mci.integrate_sweep(bubble_mcmc, maps=[r.map for r in head], reweight=[r.reweight for r in head], chain_state=[r.chain_state for r in head],
                               adapt=False, neval=1e5, niter=10, **kw())
    print("train, then production (:mcmc, %d carried chains per block): the production scan starts at iteration %d, its chains stored by iteration %d;"
          " %d + %d evaluations at the first point" % (mcmc_chains, head[0].chain_state.iteration + 1, tail[0].chain_state.iteration, head[0].neval, tail[0].neval))
    for p, r in list(zip(scan, tail))[::max(1, points // 8)]:
        print("%6.3f  %s" % (p.rs, "  ".join("%12.6f +- %-10.6f" % (r.mean[0][i], r.stdev[0][i]) for i in range(Qsize))))
    return scan, head, tail


if __name__ == "__main__":
    main()
    stratified()
    stratified_two_types()
    bubble_scan()
    bubble_scan(solver="vegasmc", chains=64)
    bubble_scan(solver="mcmc", mcmc_chains=64)
    bubble_train_then_produce()
