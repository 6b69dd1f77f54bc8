"""`integrate_sweep(integrand, params; solver, ...)`: the integral at every entry of `params`, as one launch where the layout allows.

KINDS is the table of sweep kinds -- fixed, until, strat, chains, mcmc --, one entry each: the keyword that selects it, its solver, the
Engine query that refuses it, the Engine method that runs it with the keywords it adds to the common ones, what it adds to a point's
Result, which call-only inputs (INPUTS) it owns and what the looped form passes to integrate() in its place.  integrate_sweep is a short
driver over four pieces that read the table: _request (every keyword check before a Configuration exists), _bind_sweep (closure trace,
userdata rows, measure trace), _point_result (one point's Result) and _looped (the fallback of ordinary integrate() calls).  A new kind
is a new entry."""
import copy
import importlib
import types
import warnings

import numpy as np

from . import trace as tr
from ._lib import SOLVERS
from .comm import LocalComm
from .configuration import Configuration
from .engine import Engine
from .integrand import HostIntegrand, HostMeasure, Integrand, Measure
from .integrate import StratD, _bind, _stratify_request, callback_form, standardize_block
from .statistics import ChainState, Result, report

_I = importlib.import_module(".integrate", __package__)   # the module, not the function of the same name: integrate and TRACE_DEFAULT are looked up on it at call time


# ---- the table of sweep kinds ----------------------------------------------------------------------------------------------------------

# The inputs only a call carries, in the order they are checked: what a call of a kind that does not own one is told, and what the
# looped form, which takes none of them, says.  config= and maps= go with every kind.
INPUTS = {
    "config": (None, "the looped form builds one Configuration per point from keywords (var=..., dof=...), not from config="),
    "maps": (None, "maps= needs the batched form"),
    "reweight": ('reweight= belongs to a chain sweep (solver="vegasmc", chains=K)', "reweight= needs the batched form"),
    "chain_state": ("chain_state= belongs to a chain sweep with carried chains: give carry=True (and chains=K or mcmc_chains=K)",
                    "chain_state= needs the batched form"),
    "alloc": ("alloc= belongs to a stratified sweep (stratify=True or mci.Stratify(...))", "alloc= needs the batched form"),
    "tolerance": ("min_niter= belongs to a target error: give rtol= or atol=", "rtol= / atol= need the batched form"),
}


class Kind:
    """One kind of sweep.  flag: the keyword whose presence selects it (None: the default); solver: the one it belongs to -- _request
    refuses `flag` under another with `elsewhere`'s words (the chain kinds) or its own (until); a :vegas kind without a flag is refused
    by its query, stratify= by _stratify_request --; query: the Engine query whose reason sends the call to the looped form, asked with
    the fields of the request named in `asks` as keywords; demands: a second query, asked with the kind's own keywords, whose reason is a
    ValueError; run: the Engine method; owns: its call-only inputs; prepare(rq, eng): engine settings the query reads; plan(rq, eng): what
    the driver keeps as rq.plan once the query has passed; keywords(rq): what `run` takes beyond the common keywords; result(rq, r, res):
    what a point's Result carries beyond the common attributes; looped(rq): what integrate() takes in its place.  The functions read the
    request alone: its fields are listed at _request."""

    def __init__(self, solver, query, run, flag=None, asks=(), demands=None, owns=(), elsewhere=None, prepare=None, plan=lambda rq, eng: None,
                 keywords=lambda rq: {}, result=lambda rq, r, res: None, looped=lambda rq: {}):
        self.solver, self.query, self.run, self.flag, self.asks, self.demands, self.owns = solver, query, run, flag, asks, demands, owns
        self.elsewhere, self.prepare, self.plan, self.keywords, self.result, self.looped = elsewhere, prepare, plan, keywords, result, looped


def _strat_prepare(rq, eng):
    eng.set_sweep_strat_leaves(rq.leaves)      # (leaves="all" opts in to both leaf modes)
    eng.set_stratification(rq.strat.nstrat, rq.strat.beta, rq.strat.max_nhcube)


def _strat_keywords(rq):
    return dict(d=_sweep_alloc_rows(rq.alloc, rq.P, rq.plan) if rq.alloc is not None else None)


def _strat_result(rq, r, res):
    plan = rq.plan
    res.stratification = dict(nstrat=list(plan["nstrat"]), ncube=plan["ncube"], beta=plan["beta"], carry=False,
                              carried="same plan" if rq.alloc is not None else "uniform")
    res.strat_d, res.strat_counts = StratD(r["strat_d"], plan["nstrat"], plan["beta"]), r["strat_counts"]


def _chain_keywords(rq):
    kw = dict(nchain=rq.nchain, carry=rq.carry, reweight=rq.reweight)
    if rq.chain_state is not None:
        kw["state"] = rq.chain_state
    return kw


def _chain_result(rq, r, res):
    res.config._sweep_tables = (r["propose"], r["accept"])   # config.propose / config.accept: this point's, not the engine's
    res.correlated = r["correlated"]
    if r["correlated"]:              # (carried chains: the block-lineage error, made by the library from the point's block means)
        res._flat_std = np.asarray(r["stdev"], dtype=np.float64)
        res.stdev = res._shape(res._flat_std)
    res.reweight, res.chain_state = r["reweight"], r.get("chain_state")


def _mcmc_result(rq, r, res):
    _chain_result(rq, r, res)
    res.holds, res.hold_max, res.chain_steps = r["holds"], r["hold_max"], rq.neval // rq.block // rq.nchain
    res.chains_carried = bool(r.get("carried"))


VEGAS_ONLY = "stratification is :vegas's"

KINDS = {
    "fixed": Kind("vegas", "sweep_supported", "integrate_sweep"),
    "until": Kind("vegas", "sweep_supported", "integrate_sweep_until", flag="until", demands="sweep_until_supported", owns=("tolerance",),
                  keywords=lambda rq: dict(rtol=rq.rtol or 0.0, atol=rq.atol or 0.0, min_niter=rq.min_niter or 0),
                  result=lambda rq, r, res: vars(res).update(niter_run=r["niter_run"], converged=r["converged"])),
    "strat": Kind("vegas", "sweep_strat_supported", "integrate_sweep_strat", flag="stratify", owns=("alloc",), prepare=_strat_prepare,
                  plan=lambda rq, eng: eng.sweep_strat_plan(rq.neval, rq.block), keywords=_strat_keywords, result=_strat_result, looped=lambda rq: dict(stratify=rq.strat)),
    "chains": Kind("vegasmc", "sweep_chains_supported", "integrate_sweep_chains", flag="chains", asks=("nchain", "first_iteration"),
                   owns=("reweight", "chain_state"),
                   elsewhere={"vegas": '"vegas" is swept without it', "mcmc": 'a sweep of "mcmc" points is a follow-up'},
                   keywords=_chain_keywords, result=_chain_result, looped=lambda rq: dict(nchain=rq.nchain)),
    "mcmc": Kind("mcmc", "sweep_mcmc_supported", "integrate_sweep_mcmc", flag="mcmc_chains", asks=("nchain", "first_iteration", "thermal_ratio"),
                 owns=("reweight", "chain_state"),
                 elsewhere={"vegas": '"vegas" is swept without it', "vegasmc": '"vegasmc" takes chains='},
                 keywords=lambda rq: dict(_chain_keywords(rq), thermal_ratio=rq.thermal_ratio), result=_mcmc_result,
                 looped=lambda rq: dict(nchain=rq.nchain, thermal_ratio=rq.thermal_ratio)),
}

# ---- the request check -----------------------------------------------------------------------------------------------------------------

def _stratified(stratify):
    return stratify is not None and stratify is not False


def _chains_per_block(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError("integrate_sweep: %s must be an int >= 1 (chains per block), got %r" % (name, value))
    return int(value)


def _together(given, x, others, why):
    """X (as the message names it) next to one of the keywords `others`: the two do not go together"""
    for y in others:
        if given[y]:
            raise ValueError("integrate_sweep: %s and %s= do not go together (%s)" % (x, y, why))


def _one_per_point(name, what, n, P):
    if n != P:
        raise ValueError("integrate_sweep: %s must hold one %s per point (%d), got %d" % (name, what, P, n))


def _listed(name, what, make, value):
    try:
        return make(value)
    except TypeError:
        raise ValueError("integrate_sweep: %s must be a list with one %s per point" % (name, what))


def _chain_states(chain_state, P):
    """chain_state= as a list, and the iteration that continues the states"""
    chain_state = _listed("chain_state", "ChainState", list, chain_state)
    _one_per_point("chain_state", "ChainState", len(chain_state), P)
    if not all(isinstance(s, ChainState) for s in chain_state):
        raise ValueError("integrate_sweep: chain_state must hold ChainState objects (the chain_state of an earlier sweep's results; None: that "
                         "call kept no chains -- carry=True and more than one chain per block)")
    nexts = sorted({s.iteration + 1 for s in chain_state})
    if len(nexts) != 1:
        raise ValueError("integrate_sweep: the chain states disagree with each other: they were stored by iterations %s"
                         % ", ".join(str(n - 1) for n in nexts))
    return chain_state, nexts[0]


def _request(params, config=None, solver="vegas", leaves="one", seeds=None, maps=None, stratify=None, alloc=None, chains=None, reweight=None, mcmc_chains=None,
             carry=False, rtol=None, atol=None, min_niter=None, chain_state=None):
    """The keywords of an integrate_sweep call, checked as far as they can be before a Configuration exists -> the request, the one
    object the kinds' functions, _point_result and _looped read.  Raises ValueError, the first in the order of the checks below.
    Set here: kind (the entry of KINDS the call selects), P, solver (normalised), leaves, nchain (chains / mcmc_chains as an int, else
    None), carry, rtol, atol, min_niter, reweight, alloc, chain_state (a list) with first_iteration (the iteration that continues the
    states; None without states), inputs (every call-only input of INPUTS, None where not given).
    Set by the driver, None until then: once the Configuration exists first_iteration (its iterations_done), ignore, strat (the
    Stratify or None), neval (per iteration, standardised) and block, print, thermal_ratio; once the kind's query has passed, plan
    (kind.plan: {nstrat, ncube, beta} of a stratified sweep, else None)."""
    if solver in (":vegas", ":vegasmc", ":mcmc"):
        solver = solver[1:]
    if solver not in SOLVERS:
        raise ValueError("Solver %s is not supported!" % solver)
    if leaves not in ("one", "all"):
        raise ValueError('integrate_sweep: leaves must be "one" or "all", got %r' % (leaves,))
    try:
        P = len(params)
    except TypeError:
        raise ValueError("integrate_sweep: params must be a sequence with one entry per point")
    if not 1 <= P <= Engine.SWEEP_MAX_POINTS:
        raise ValueError("integrate_sweep: %d points; a sweep takes 1 to %d" % (P, Engine.SWEEP_MAX_POINTS))
    for name, what, value in (("seeds", "seed", seeds), ("maps", "map", maps)):
        if value is not None:
            _one_per_point(name, what, len(value), P)
    if carry not in (False, True):
        raise ValueError("integrate_sweep: carry must be True or False, got %r" % (carry,))
    given = dict(stratify=_stratified(stratify), chains=chains is not None, mcmc_chains=mcmc_chains is not None, carry=carry,
                 until=rtol is not None or atol is not None)
    if carry:
        _together(given, "carry=", ("stratify",), VEGAS_ONLY)
        if solver == "vegas":
            raise ValueError('integrate_sweep: carry= belongs to a chain sweep (solver="vegasmc", chains=K or solver="mcmc", mcmc_chains=K); "vegas" has no chains')
        if not given["chains"] and not given["mcmc_chains"]:
            raise ValueError("integrate_sweep: carry= belongs to a chain sweep: give chains=K (solver=\"vegasmc\") or mcmc_chains=K (solver=\"mcmc\")")
    if min_niter is not None and not given["until"]:
        raise ValueError("integrate_sweep: " + INPUTS["tolerance"][0])
    if given["until"]:
        if solver != KINDS["until"].solver:
            raise ValueError("integrate_sweep: rtol= / atol= / min_niter=: solver is not :vegas (chain solvers are not swept)")
        _together(given, "rtol= / atol= / min_niter=", ("stratify", "chains", "mcmc_chains"), "the stratified, :vegasmc and :mcmc sweeps have no target error")
        if min_niter is not None and (isinstance(min_niter, bool) or not isinstance(min_niter, (int, np.integer))):
            raise ValueError("integrate_sweep: min_niter must be an int >= 0, got %r" % (min_niter,))
    if given["chains"] and given["mcmc_chains"]:
        raise ValueError('integrate_sweep: chains= (solver="vegasmc") and mcmc_chains= (solver="mcmc") do not go together')
    nchain = None
    for k, value in ((KINDS["chains"], chains), (KINDS["mcmc"], mcmc_chains)):
        if value is not None:
            nchain = _chains_per_block(k.flag, value)
            if solver != k.solver:
                raise ValueError('integrate_sweep: %s= belongs to solver="%s" (%s)' % (k.flag, k.solver, k.elsewhere[solver]))
            _together(given, k.flag + "=", ("stratify",), VEGAS_ONLY)
    kind = next((k for k in KINDS.values() if k.flag and given[k.flag]), KINDS["fixed"])
    inputs = dict(config=config, maps=maps, reweight=reweight, chain_state=chain_state, alloc=alloc, tolerance=True if given["until"] else None)
    first_iteration = None
    for name in ("reweight", "chain_state", "alloc"):
        if inputs[name] is None:
            continue
        if name not in kind.owns or (name == "chain_state" and not carry):
            raise ValueError("integrate_sweep: " + INPUTS[name][0])
        if name == "reweight":
            _one_per_point("reweight", "vector", len(reweight), P)
        elif name == "chain_state":
            inputs[name], first_iteration = _chain_states(chain_state, P)
        else:
            _one_per_point("alloc", "strat_d array", _listed("alloc", "strat_d array", len, alloc), P)
    return types.SimpleNamespace(kind=kind, P=P, solver=solver, leaves=leaves, nchain=nchain, carry=carry, rtol=rtol, atol=atol, min_niter=min_niter,
                                 inputs=inputs, reweight=reweight, alloc=alloc, chain_state=inputs["chain_state"], first_iteration=first_iteration,
                                 ignore=None, strat=None, neval=None, block=None, print=None, thermal_ratio=None, plan=None)


# ---- the binder ------------------------------------------------------------------------------------------------------------------------

class _MeasureConfig:
    """the configuration a sweep's measure closure is traced on: point 0's, with every read off config.userdata on record"""

    def __init__(self, config, userdata, rec):
        self._config, self._rec, self._touched = config, rec, False
        self._plain = userdata
        self._view = tr._userdata_view(userdata, rec, False, ())
        self._lazy = isinstance(self._view, tr._UserdataView)   # (anything else -- a number, an array -- is read the moment it is touched)
        if not self._lazy:
            del rec.literals[:]

    def __getattr__(self, name):
        return getattr(self._config, name)

    @property
    def userdata(self):
        self._touched = True
        return self._view if self._lazy else self._plain

    def reads(self):
        if self._lazy:
            return list(self._rec.literals)
        return [((), self._plain)] if self._touched and self._plain is not None else []


def _trace_sweep_measure(measure, traced_on, params, solver):
    """The measure closure of a sweep, traced on the configuration the integrand was traced on (point 0).  A sweep has ONE ud row per
    point and that row is the integrand's: a measure whose body would hold a value read off config.userdata -- a float, an array -- is
    refused with a ValueError naming it, and so is one that reads anything else (an int, a string) in which the points differ.
    Returns the traced Measure, or None when the closure does not trace (it is then bound like any other closure)."""
    rec = tr._Trace()
    mcfg = _MeasureConfig(traced_on, params[0], rec)
    mindexed = callback_form(measure, solver, what="measure") == "indexed"
    try:
        traced = tr.trace_measure(measure, mcfg, indexed=mindexed)
    except tr.TraceError:
        traced = None
    for path, was in mcfg.reads():
        name = tr._path_name(path)
        if isinstance(was, (float, np.floating, np.ndarray, list, tuple)) and not isinstance(was, bool):
            raise ValueError("integrate_sweep: the measure reads %s off config.userdata, and its value would be written into the measure's "
                             "body: a sweep has one ud row per point, and that row is the integrand's" % name)
        for q in params[1:]:
            try:
                now = tr._reach(q, path)
            except Exception as e:
                raise ValueError("integrate_sweep: the measure reads %s, which cannot be read at every point (%s: %s)" % (name, type(e).__name__, e))
            if not tr._same_leaf(was, now):
                raise ValueError("integrate_sweep: the measure reads %s, which is %r at the traced point and %r at another: the points "
                                 "would trace to different measure bodies" % (name, was, now))
    return traced


def _is_closure(integrand):
    return callable(integrand) and not isinstance(integrand, (Integrand, HostIntegrand))


def _bind_sweep(integrand, params, measure, solver, config, trace):
    """(bound integrand, bound measure, userdata rows [P][nuserdata], why): a closure is traced ONCE, on params[0], and every point's row is
    evaluated from its object; device source takes params as the rows.  why: the reason the integrand is a host integrand -- which no
    sweep takes: the bound integrand and the rows are then None --, else None"""
    if _is_closure(integrand):
        traced_on = copy.copy(config)      # (the caller's Configuration keeps its userdata)
        traced_on.userdata = params[0]
        form = callback_form(integrand, solver, False)
        try:
            if trace is False:
                raise tr.TraceError("trace = False")
            bound = tr.trace_integrand(integrand, traced_on, indexed=form == "indexed", inplace=form == "inplace")
            if getattr(bound, "userdata_for", None) is None:
                raise ValueError("integrate_sweep: the closure's body depends on the values of its parameters (a Python branch on a captured "
                                 "float, a table indexed with a draw): the points would trace to different bodies")
            rows = np.array([bound.userdata_for(p) for p in params], dtype=np.float64).reshape(len(params), len(bound.userdata))
        except tr.TraceError as e:   # (also a later point whose parameters do not evaluate: userdata_for raises it)
            return None, measure, None, "the closure was not traced (%s): a host integrand" % e
        if callable(measure) and not isinstance(measure, (Measure, HostMeasure)) and not hasattr(measure, "pool"):
            measure = _trace_sweep_measure(measure, traced_on, params, solver) or measure
        return bound, measure, rows, None
    if isinstance(integrand, str):
        integrand = Integrand(integrand, None)
    if isinstance(integrand, HostIntegrand):
        return None, measure, None, "a host integrand (device source or a traced closure only)"
    rows = np.asarray(params, dtype=np.float64)
    if rows.ndim != 2 or (len(integrand.userdata) and rows.shape[1] != len(integrand.userdata)):
        raise ValueError("integrate_sweep: params must be userdata rows [points][%d] for this integrand, got shape %s"
                         % (len(integrand.userdata), rows.shape))
    return Integrand(integrand.body, rows[0], integrand.name), measure, rows, None


def _sweep_alloc_rows(alloc, P, plan):
    """alloc= of a stratified sweep -> [P][ncube] d_h, checked against the call's plan {nstrat, ncube, beta}"""
    rows = np.zeros((P, plan["ncube"]))
    for k, v in enumerate(alloc):
        ns, beta = getattr(v, "nstrat", None), getattr(v, "beta", None)
        if ns is not None and (list(ns) != list(plan["nstrat"]) or beta != plan["beta"]):
            raise ValueError("integrate_sweep: alloc[%d] was measured on nstrat = %s under beta = %r, this call runs nstrat = %s under beta = %r "
                             "(there is no remap in a sweep)" % (k, list(ns), beta, list(plan["nstrat"]), plan["beta"]))
        v = np.asarray(v, dtype=np.float64)
        if v.shape != (plan["ncube"],):
            raise ValueError("integrate_sweep: alloc[%d] has shape %s, the plan nstrat = %s has %d hypercubes" % (k, v.shape, list(plan["nstrat"]), plan["ncube"]))
        rows[k] = v
    return rows


# ---- the results -----------------------------------------------------------------------------------------------------------------------

def _point_result(kind, r, config, p, rq):
    """The Result of one point of a sweep of `kind`, from the dict r the engine returned for it: a copy of the configuration with the
    point's userdata (p; None for device source) and visited, the attributes every sweep point carries, and the kind's own.  rq: the
    request -- ignore, block, print, and what the kind's result function reads"""
    c = copy.copy(config)            # (the points share the engine; a sweep leaves its map, factors, logs and allocation alone)
    c.userdata = p
    c.visited = r["visited"]
    res = Result(r["iter_mean"], r["iter_std"], c, rq.ignore, neval=r["neval"], seconds=r["seconds"], block=rq.block)
    res.sweep_batched, res.map, res.status, res.maps_by_leaf = True, r["maps"], r["status"], r.get("maps_by_leaf")
    res.warmup, res.neval_discarded = 0, 0
    kind.result(rq, r, res)
    if rq.print >= 0:
        report(res)
    return res


def _looped(rq, why, call, integrand, bound, rows, params, seeds, pristine, eng):
    """Not a sweep layout (why): the points one after another, each an ordinary integrate() call -- keywords `call` and the kind's own --
    on a Configuration of its own, built from the keywords `pristine`; a call-only input that was given needs the batched form.  eng: the
    engine the refused sweep was bound to, if any: closed"""
    for name, value in rq.inputs.items():
        if value is not None:
            raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and %s" % (why, INPUTS[name][1]))
    warnings.warn("integrate_sweep: this problem does not run as a sweep (%s): %d ordinary integrate() calls, one after another" % (why, rq.P),
                  RuntimeWarning, stacklevel=3)
    if eng is not None:
        eng.close()
    out = []
    for k, p in enumerate(params):
        kw = copy.deepcopy(pristine)
        if _is_closure(integrand):
            kw["userdata"], f = p, integrand
        else:
            f = integrand if bound is None else Integrand(bound.body, rows[k], bound.name)   # (a HostIntegrand as it is)
        c = Configuration(**kw)
        if seeds is not None:
            c.seed = int(seeds[k])
        res = _I.integrate(f, config=c, **call, **rq.kind.looped(rq))
        res.sweep_batched, res.map, res.maps_by_leaf, res.status = False, None, None, 0
        out.append(res)
    return out


def integrate_sweep(integrand, params, *, solver="vegas", config=None, neval=1e4, niter=10, block=16, gamma=1.0, adapt=True, ignore=None,
                    measure=None, measurefreq=1, seeds=None, maps=None, device=None, trace=None, print=-1, leaves="one", stratify=None, alloc=None,
                    chains=None, reweight=None, mcmc_chains=None, thermal_ratio=0.1, carry=False, rtol=None, atol=None, min_niter=None, chain_state=None, **kwargs):
    """A parameter sweep: the integral at every entry of `params`, as ONE launch where the layout allows (Engine.integrate_sweep,
    mci_integrate_sweep: one workgroup runs a point's whole loop).  Returns a list of Result, one per point; result p is what
    integrate() returns for point p on a fresh copy of the configuration -- every point starts from the configuration's current
    map, and by default all points share the seed (common random numbers: a smooth curve over the scan); seeds = one per point.

    params: what the integrand reads its parameters from.  For a Python closure these are the `config.userdata` objects (a struct of
    floats, a dict, a number: examples/bubble_closure.py) -- the closure is traced ONCE, on params[0], and every point's ud row is
    evaluated from its object by the trace's parameter evaluation (trace.py "Captured parameters").  Only FLOATS are parameters:
    ints, bools, strings, non-finite floats and array shapes the closure reads off userdata are written into the body, so points that
    differ in one of them (`Para(a=2)` next to `Para(a=3)`: write 2.0, 3.0), and a closure whose body depends on the values, are
    refused with a ValueError naming the field -- never run on the body of point 0.  For a device-source string or an Integrand (mci.catalog) they are the
    userdata rows.  A float array the closure indexes with a Discrete draw (`para.extQ[Ext[0] - 1]`) is a table of the body: every
    point's row carries its own values, and its shape must be the same at every point.  maps: None or [P][Engine.sweep_map_doubles()]
    starting maps; every Result carries `map` (the point's map after its last iteration, the flat row), `maps_by_leaf` (leaf by leaf: a
    Continuous leaf's grid, a Discrete leaf's distribution), `status` (device flags of that point, 0 = none) and `sweep_batched`.

    leaves: "one" (default) sweeps problems with ONE Continuous variable leaf; "all" opts in to sweeps of any mix of Continuous and
    Discrete leaves that fits a workgroup's LDS (Engine.set_sweep_leaves) -- composites, histograms over a Discrete draw.  A `measure`
    closure is traced on the same point as the integrand; one that reads a value off config.userdata is refused (ValueError).

    stratify: True or Stratify(beta, nstrat, max_nhcube) -- every point runs VEGAS+ adaptive stratified sampling, what
    integrate(..., stratify=...) runs, still in ONE launch (Engine.integrate_sweep_strat; one Continuous variable leaf, or with
    leaves="all" several of them: variable types with ranges of their own, a composite with one grid per axis --
    Engine.set_sweep_strat_leaves; `map` is then the flat row of every leaf's grid, `maps_by_leaf` the grids one by one).  Every Result
    then carries `stratification` (nstrat, ncube, beta, carried = "uniform" | "same plan"), `strat_d` (the d_h its last iteration
    measured) and `strat_counts` (the allocation that iteration used).  alloc: a list of P strat_d arrays, e.g. [r.strat_d for r in
    trained] -- every point's first allocation is made from its entry, which must have been measured on this call's plan and beta
    (there is no remap in a sweep: a strat_d remembers the plan and beta it was measured under, and another one raises ValueError);
    with adapt=False the whole scan keeps it: train, then freeze.  A sweep carries through alloc, never through Stratify(carry=True).
    Where the stratified sweep is refused (Engine.sweep_strat_supported: several Continuous leaves without leaves="all", a map that does
    not fit a workgroup's LDS, ...) the points run as integrate(..., stratify=...) calls, as below; alloc= then raises.

    chains: None (default) or an int >= 1 -- with solver="vegasmc", the reference's default solver, every point runs its :vegasmc loop
    with that many chains per block, fresh in every iteration, still in ONE launch (Engine.integrate_sweep_chains: one workgroup per
    point, a lane per chain; any mix of Continuous and Discrete leaves, whatever `leaves` says).  Every Result then also carries
    `reweight` (the point's factors after its last doReweight!), and its config.visited / config.propose / config.accept are the
    point's own; correlated = False.  reweight = [r.reweight for r in head] together with maps = [r.map for r in head] goes on with a
    scan.  Without chains= a chain solver is not swept (the loop below, as ever); chains= with solver="vegas", with stratify= or under
    "mcmc" raises ValueError.  Where the chain sweep is refused (Engine.sweep_chains_supported) the points run as
    integrate(..., nchain=chains) calls, as below; reweight= then raises.

    mcmc_chains: None (default) or an int >= 1 -- with solver="mcmc" every point runs its :mcmc loop with that many chains per block
    and burn-in floor(steps * thermal_ratio) (mci_mcmc_burnin), fresh in every iteration, still in ONE launch
    (Engine.integrate_sweep_mcmc; no warm-up repetition, no automatic chain count).  Closures are called in the solver's form,
    integrand(idx, var, config) and measure(idx, var, obs, relative_weight, config).  Every Result carries what a chains= sweep's
    does (`reweight`, own visited / propose / accept, correlated = False) and `holds` (the point's holding-time histogram, 64 counts
    over the call) and `hold_max` (the upper bound 2^b - 1 of its highest occupied bin b, 0 if none); report() adds a note where
    16 * hold_max exceeds the measured steps of a chain.  reweight= goes with it as with chains=.  mcmc_chains= with another solver,
    together with chains= or with stratify= raises ValueError; without it an :mcmc scan loops as below.  Where the sweep is refused
    (Engine.sweep_mcmc_supported) the points run as integrate(..., solver="mcmc", nchain=mcmc_chains, thermal_ratio=...) calls;
    reweight= then raises.

    carry: False (default) or True -- with chains= or mcmc_chains= every iteration of a point after its first continues the chains of
    the one before, resampled to the target train! and doReweight! have moved (Engine.set_sweep_chain_carry: what integrate() does by
    default; :vegasmc with adapt=True from the third iteration on; one chain per block carries nothing).  :mcmc chains then burn in
    only in a point's first iteration.  The first iteration of every call starts afresh -- chain state does not travel between calls.
    Results of carried points have correlated = True and the block-lineage error as `stdev` (with_ignore() falls back to the
    reference's); report()'s hold note asks for 4 x hold_max instead of 16 x.  carry=True without chains= / mcmc_chains=, with
    stratify= or under "vegas" raises ValueError.  Where the sweep is refused, the looped integrate() calls carry by their own default.

    chain_state: None (default) or [r.chain_state for r in head] -- with carry=True and more than one chain per block every Result
    carries `chain_state` (a ChainState: the record of its chains and one array), and a later call that takes the list next to maps= and
    reweight= goes on from those chains instead of starting afresh: a point is then what integrate(..., nchain=K) is on the engine that
    has just run the earlier call (Engine.integrate_sweep_chains / integrate_sweep_mcmc, state=).  Its first iteration continues the
    stored chains -- :mcmc without any burn-in; :vegasmc unless they ran on a never-refined map that was refined since -- and the call's
    chain count may differ from the stored one.  On a fresh configuration (no config=) the call takes first_iteration from the states;
    states that disagree with each other or with config.iterations_done raise ValueError, and so does chain_state= without carry=True,
    with the wrong length, or where the sweep is refused and the points would loop over ordinary calls.  A state of another solver,
    block count or layout is refused by name (MCIError).  Results of a call whose first iteration continued have correlated = True and
    the block-lineage error, as in integrate().

    rtol, atol: None (default) or a target error -- under solver="vegas" every point stops once each of its statistics columns has
    stdev <= max(atol, rtol * |mean|) (the weighted average over its counted iterations and that average's error, as Result computes
    them), from iteration max(ignore + 2, min_niter) on; `niter` becomes the maximum.  Still ONE launch (Engine.integrate_sweep_until):
    a workgroup that has finished a point takes the next one.  Every Result then carries `niter_run` (the iterations it ran; its tables
    hold that many rows) and `converged` (False when it ran all `niter` without meeting the target; report() says so); a point's
    numbers are those of the fixed sweep with niter = niter_run.  leaves="all" works as before.  A column that is NaN or infinite never
    converges.  The three keywords with another solver, with stratify=, chains= or mcmc_chains=, or min_niter without a tolerance,
    raise ValueError; so does a tolerance on a problem that does not run as a sweep: the loop of integrate() calls below has no
    such stop, and never runs in its place.

    A problem that cannot run as a sweep (Engine.sweep_supported: several variable leaves or a Discrete variable without leaves = "all",
    measurefreq != 1, a host integrand, ...) runs the points as ordinary integrate() calls, one after another, each on a fresh Configuration(**kwargs);
    a RuntimeWarning says so once, with the reason, and the results have sweep_batched = False.  Keywords as integrate()."""
    if trace is None:
        trace = _I.TRACE_DEFAULT
    rq = _request(params, config, solver, leaves, seeds, maps, stratify, alloc, chains, reweight, mcmc_chains, carry, rtol, atol, min_niter, chain_state)
    kind, solver = rq.kind, rq.solver
    fresh = config is None
    pristine = copy.deepcopy(kwargs) if fresh else None
    if fresh:
        config = Configuration(**kwargs)
    if chain_state is not None:
        if fresh:
            config.iterations_done = rq.first_iteration    # (a fresh configuration goes on where the states' call stopped)
        elif config.iterations_done != rq.first_iteration:
            raise ValueError("integrate_sweep: the chain states were stored by iteration %d, and config.iterations_done = %d: the call would "
                             "not start at the iteration that continues them (%d)" % (rq.first_iteration - 1, config.iterations_done, rq.first_iteration))
    if ignore is None:
        ignore = 1 if adapt else 0
    rq.first_iteration, rq.ignore, rq.print, rq.thermal_ratio = config.iterations_done, ignore, print, thermal_ratio
    rq.strat = _stratify_request(stratify, solver, config, integrand, measure, measurefreq, trace, LocalComm())
    if rq.strat is not None and rq.strat.carry:
        raise ValueError("integrate_sweep: Stratify(carry=True) is the ordinary call's way to carry an allocation; a sweep takes alloc=")
    bound, bound_measure, rows, why = _bind_sweep(integrand, params, measure, solver, config, trace)
    if device is None:
        device = 0
    nevalperblock, block = standardize_block(int(neval), block, 1)
    rq.neval, rq.block = nevalperblock * block, block
    eng = None
    if why is None:
        eng = _bind(config, bound, bound_measure, solver, trace=trace, print=print, device=device)
        eng.set_sweep_leaves(leaves)
        if kind.prepare:
            kind.prepare(rq, eng)
        why = getattr(eng, kind.query)(solver, rq.neval, niter, block, measurefreq, **{name: getattr(rq, name) for name in kind.asks})
    if why is None:
        rq.plan = kind.plan(rq, eng)
        own = kind.keywords(rq)
        bad = kind.demands and getattr(eng, kind.demands)(solver, rq.neval, niter, block, measurefreq, **own)
        if bad:     # (the target itself: in the words of mci_sweep_until_supported)
            raise ValueError("integrate_sweep: %s" % bad)
        rs = getattr(eng, kind.run)(solver, userdata=rows, neval=rq.neval, niter=niter, block=block, ignore=ignore, adapt=adapt, gamma=gamma,
                                    measurefreq=measurefreq, seed=config.seed, seeds=seeds, maps=maps, first_iteration=rq.first_iteration, **own)
        return [_point_result(kind, r, config, p if _is_closure(integrand) else None, rq) for p, r in zip(params, rs)]
    call = dict(solver=solver, neval=neval, niter=niter, block=block, gamma=gamma, adapt=adapt, ignore=ignore, measure=measure, measurefreq=measurefreq,
                device=device, trace=trace, print=print)
    return _looped(rq, why, call, integrand, bound, rows, params, seeds, pristine, eng)
