"""`integrate(integrand; solver, config, neval, niter, block, ...)`  reference src/main.jl:71-218."""
import ctypes as C
import time

import numpy as np

from . import catalog
from ._lib import MCMC, SOLVERS, VEGAS, VEGASMC, lib
from .comm import LocalComm
from .configuration import Configuration
from .engine import Engine
from .integrand import HostIntegrand, HostMeasure, Integrand, Measure
from .statistics import Result, chain_estimator_bias, report
from .variables import Continuous, Discrete


class Stratify:
    """integrate(..., solver="vegas", stratify=Stratify(...)): VEGAS+ adaptive stratified sampling (Lepage, J. Comput. Phys. 439
    (2021) 110386; the default mode of the Python `vegas` package).  y-space is cut into prod(nstrat) hypercubes, every hypercube gets at
    least two of an iteration's samples, and after every iteration the samples move between hypercubes in proportion to
    (sum of the hypercube's variances)^(beta/2); beta = 0 keeps the stratification even.  nstrat None: the default plan for neval
    (mci_strat_plan: about eight samples per hypercube, at most max_nhcube hypercubes).  An iteration's error is the stratified one:
    `block` plays no part in it.  It is built from every hypercube's sample variance, so it is only as good as those: with an explicit
    nstrat that leaves about two samples per hypercube, or with beta = 0, a heavy-tailed integrand's error comes out too small
    (log(x)/sqrt(x): the means scatter 5.1 | 2.4 times the reported error, profiles/r07_stratified.txt); report() says so.
    carry=True (mci_set_stratification_carry): the call starts from the allocation the engine of `config=res.config` learned in its last
    call -- or loaded from a state file -- instead of a uniform one, moved onto this call's plan and beta where they differ; with
    adapt=False the whole call keeps it (train at a small neval, then measure at a large one).  The default, False, starts uniform."""

    def __init__(self, beta=0.75, nstrat=None, max_nhcube=2 ** 24, carry=False):
        if not isinstance(carry, (bool, np.bool_)):
            raise ValueError("Stratify: carry = %r, must be True or False" % (carry,))
        self.beta, self.max_nhcube, self.carry = float(beta), int(max_nhcube), bool(carry)
        self.nstrat = None if nstrat is None else [int(v) for v in nstrat]

    def __repr__(self):
        return "Stratify(beta=%r, nstrat=%r, max_nhcube=%r, carry=%r)" % (self.beta, self.nstrat, self.max_nhcube, self.carry)


class StratD(np.ndarray):
    """Result.strat_d of a stratified sweep: the d_h of a point's last iteration, with the plan (`nstrat`) and `beta` it was measured
    under, so that integrate_sweep(alloc=...) can refuse it on another plan"""

    def __new__(cls, values, nstrat, beta):
        obj = np.asarray(values, dtype=np.float64).view(cls)
        obj.nstrat, obj.beta = [int(v) for v in nstrat], float(beta)
        return obj

    def __array_finalize__(self, obj):
        self.nstrat, self.beta = getattr(obj, "nstrat", None), getattr(obj, "beta", None)


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


def _stratify_request(stratify, solver, config, integrand, measure, measurefreq, trace, comm):
    """the Stratify an integrate() call asks for (None: plain), refused -- before any engine exists -- where this mode does not reach"""
    if stratify is None or stratify is False:
        return None
    st = Stratify() if stratify is True else stratify
    if not isinstance(st, Stratify):
        raise ValueError("stratify = %r: True or mci.Stratify(beta=..., nstrat=..., max_nhcube=..., carry=...)" % (stratify,))
    why = None
    if SOLVERS.get(solver) != VEGAS:   # (the solver by name or by its constant, as integrate() takes it)
        why = "solver = %r (stratified sampling is a :vegas mode)" % solver
    elif any(not hasattr(lf, "ninc") for lf in config.leaves):
        why = "a Discrete or FermiK variable (only Continuous variables are stratified)"
    elif measure is not None:
        why = "a user measure (the default measure only)"
    elif measurefreq != 1:
        why = "measurefreq = %s (every sample is measured)" % measurefreq
    elif isinstance(integrand, HostIntegrand) or (trace is False and callable(integrand) and not isinstance(integrand, Integrand)):
        why = "a host integrand (trace=False): device source or a traced closure only"
    elif comm.size > 1:
        why = "%d ranks (one rank only)" % comm.size
    if why:
        raise ValueError("stratify: refused for %s" % why)
    return st


def standardize_block(neval, nblock, nworker=1):
    """_standardize_block (main.jl:220-234)"""
    assert neval > nblock, "neval=%s should be larger than nblock = %s" % (neval, nblock)   # :222
    a, b = C.c_int64(), C.c_int64()
    lib().mci_standardize_block(int(neval), int(nblock), int(nworker), C.byref(a), C.byref(b))
    return a.value, b.value


def required_positionals(fn, fallback):
    """positional parameters of a closure that have NO default -- what decides between the reference's two callback forms
    (`integrand(var, config)` vegas/montecarlo.jl:140-144 | `integrand(idx, var, config)` mcmc/montecarlo.jl:34-36; likewise
    `measure`).  A defaulted or keyword-only parameter is the closure's own business; `fallback` for callables without a signature."""
    import inspect
    try:
        return len([q for q in inspect.signature(fn).parameters.values()
                    if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) and q.default is q.empty])
    except (TypeError, ValueError):
        return fallback


def _positional_range(fn):
    """(required, most) positional arguments the closure takes; most = None with *args; None when it has no signature"""
    import inspect
    try:
        ps = list(inspect.signature(fn).parameters.values())
    except (TypeError, ValueError):
        return None
    pos = [q for q in ps if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD)]
    return len([q for q in pos if q.default is q.empty]), (None if any(q.kind == q.VAR_POSITIONAL for q in ps) else len(pos))


_INTEGRAND_CALL = {"plain": "integrand(var, config)", "inplace": "integrand(var, weights, config)", "indexed": "integrand(idx, var, config)"}
_MEASURE_CALL = {"plain": "measure(var, obs, relative_weights, config)", "indexed": "measure(idx, var, obs, relative_weight, config)"}


def callback_form(fn, solver, inplace=False, form=None, what="integrand"):
    """Which of the reference's callback forms a bare closure is called in -- decided like the reference decides it, by the SOLVER and
    the `inplace` keyword, never by counting parameters (main.jl:26-28, :38-40):

        solver = "mcmc"                -> integrand(idx, var, config)             mcmc/montecarlo.jl:34-36
        otherwise, inplace = True      -> integrand(var, weights, config)         vegas/montecarlo.jl:140-141, vegas_mc/updates.jl:67-70
        otherwise                      -> integrand(var, config)                  vegas/montecarlo.jl:142-143, vegas_mc/updates.jl:71-75
        measure: solver = "mcmc"       -> measure(idx, var, obs, relative_weight, config)   mcmc/montecarlo.jl:166-169
                 otherwise             -> measure(var, obs, relative_weights, config)       vegas/montecarlo.jl:156-161

    The closure's own parameter count is only a cross-check: one that cannot be called that way raises TypeError here (the
    reference's MethodError at the first call) instead of being read as another form.  `form` ("plain" | "inplace" | "indexed";
    integrate's integrand_form / measure_form keywords) overrides the rule: an engine extension -- every form runs under every solver."""
    calls = _INTEGRAND_CALL if what == "integrand" else _MEASURE_CALL
    if form is None:
        form = "indexed" if solver == "mcmc" else "inplace" if (inplace and what == "integrand") else "plain"
    elif form not in calls:
        raise ValueError("%s_form = %r: one of %s" % (what, form, sorted(calls)))
    want = calls[form].count(",") + 1
    rng = _positional_range(fn)
    if rng is not None and (rng[0] > want or (rng[1] is not None and rng[1] < want)):
        has = "%d" % rng[0] if rng[1] == rng[0] else "%d to %s" % (rng[0], "any number of" if rng[1] is None else rng[1])
        hint = ""
        if what == "integrand":
            hint = ("  The form follows the solver and the `inplace` keyword (reference src/main.jl:26-28): solver = \"vegas\" / \"vegasmc\" call "
                    "integrand(var, config), with inplace = True integrand(var, weights, config); solver = \"mcmc\" calls integrand(idx, var, config).  "
                    "integrand_form = \"plain\" | \"inplace\" | \"indexed\" forces a form under any solver.")
        else:
            hint = ("  The form follows the solver (reference src/main.jl:38-40): solver = \"mcmc\" calls measure(idx, var, obs, relative_weight, config), "
                    "the others measure(var, obs, relative_weights, config).  measure_form = \"plain\" | \"indexed\" forces a form under any solver.")
        raise TypeError("solver = %r%s calls %s -- %d arguments -- but the %s closure %s takes %s positional argument%s.%s"
                        % (solver, ", inplace = True" if (inplace and what == "integrand" and solver != "mcmc") else "", calls[form], want, what,
                           getattr(fn, "__name__", "?"), has, "" if has == "1" else "s", hint))
    return form


TRACE_DEFAULT = None   # what integrate(trace=None) means: None = trace Python closures where possible, silently; False = host callbacks


def _not_traced(what, err, trace, verbosity):
    """a closure that could not be written out as device source keeps the host callback path; say why when it was asked for"""
    msg = "%s not traced (%s): host callback path" % (what, err)
    if trace:
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
    elif verbosity > 0:
        import builtins
        builtins.print(msg)


def _bind(config, integrand, measure, solver, *, inplace=False, trace=None, print=-1, device=0, engine_factory=None, rng_bits=52,
          rng_rounds=10, deterministic=False, integrand_form=None, measure_form=None):
    """The engine of `config` for this integrand and measure (created, or kept when nothing it was built for has changed): closures are
    put into the form the solver calls them in and traced where they can be; grids and reweight factors trained so far survive a change
    of integrand.  Shared by integrate() and the solver seam (Vegas / VegasMC / MCMC .montecarlo)."""
    config._sweep_tables = None   # (a point of a chain sweep handed on as config=: propose / accept are the engine's again)
    if isinstance(integrand, str):
        integrand = Integrand(integrand, config.userdata)
    elif callable(integrand) and not isinstance(integrand, (Integrand, HostIntegrand)):
        # a Python closure, called in the form the reference's solver calls it in (callback_form; main.jl:26-28): traced into device
        # source where possible, else the host "batch callback" path (vegas: per launch, vegasmc / mcmc: per Markov step).
        # HostIntegrand(fn, indexed=..., inplace=...) / trace_integrand(...) say the form explicitly.
        form = callback_form(integrand, solver, inplace, integrand_form)
        traced = None
        if trace is None or trace:
            from .trace import TraceError, trace_integrand
            try:
                traced = trace_integrand(integrand, config, indexed=form == "indexed", inplace=form == "inplace")
            except TraceError as e:
                _not_traced("integrand", e, trace, print)
        integrand = traced if traced is not None else HostIntegrand(integrand, indexed=form == "indexed", inplace=form == "inplace")
    if callable(measure) and not isinstance(measure, (Measure, HostMeasure)) and not hasattr(measure, "pool"):
        # a Python closure as measure: the reference's :mcmc form measure(idx, var, obs, relative_weight, config) under solver = "mcmc"
        # (mcmc/montecarlo.jl:166-169), measure(var, obs, weights, config) under the others (vegas/montecarlo.jl:156-161)
        mindexed = callback_form(measure, solver, form=measure_form, what="measure") == "indexed"
        tmeasure = None
        if trace is None or trace:
            from .trace import TraceError, trace_measure
            try:
                tmeasure = trace_measure(measure, config, indexed=mindexed)
            except TraceError as e:
                _not_traced("measure", e, trace, print)
        measure = tmeasure if tmeasure is not None else HostMeasure(measure, indexed=mindexed)
    mkey = None if measure is None else measure.body if isinstance(measure, (Measure, HostMeasure)) else (measure.pool, measure.slot, measure.leaf)
    key = (integrand.body, tuple(integrand.userdata), mkey, device,
           repr(config.neighbor), int(rng_bits), int(rng_rounds), bool(deterministic))
    if config._engine is None or config._engine_key != key:
        # grids trained so far survive a change of integrand (`var = (res.config.var[1], ...)`, docs/src/index.md:129)
        # and so does the learned reweight (config.reweight lives across integrate calls, configuration.jl:50)
        old = config._engine
        saved, saved_rw = None, None
        if old is not None:
            saved = [(old.grid(i) if hasattr(lf, "ninc") else None if hasattr(lf, "kF") else old.distribution(i)[0])
                     for i, lf in enumerate(config.leaves)]
            saved_rw = old.reweight()
        eng = (engine_factory or Engine)(config, integrand, measure=measure, device=device, **({"rng_bits": rng_bits} if rng_bits != 52 else {}),
                                         **({"rng_rounds": rng_rounds} if rng_rounds != 10 else {}), **({"deterministic": True} if deterministic else {}))
        if saved is not None:
            for i, lf in enumerate(config.leaves):
                if saved[i] is not None:   # (a FermiK has nothing trained)
                    (eng.set_grid if hasattr(lf, "ninc") else eng.set_distribution)(i, saved[i])
            if hasattr(eng, "set_reweight"):
                eng.set_reweight(saved_rw)
            if hasattr(old, "close"):
                old.close()                # its device buffers go now, not at some later garbage collection
        config._engine, config._engine_key = eng, key
        if getattr(config, "_pending_state", None):
            eng.load_state(config._pending_state)
            config._pending_state = None
    return config._engine


def integrate(integrand, *, solver="vegasmc", config=None, neval=1e4, niter=10, block=16, verbose=-1, gamma=1.0,
              adapt=True, debug=False, reweight_goal=None, ignore=None, measure=None, measurefreq=1,
              thermal_ratio=0.1, inplace=False, parallel="nothread", print=-1, printio=None, timer=None,
              comm=None, device=None, nchain=0, engine_factory=None, rng_bits=52, rng_rounds=10, deterministic=False, trace=None,
              integrand_form=None, measure_form=None, stratify=None, **kwargs):
    """Same keywords as the reference (main.jl:71-90; unknown ones go to Configuration, :95-97).
    Extra, engine-specific keywords: `comm` (LocalComm | RcclComm | TorchDistComm), `device`, `nchain`
    (vegasmc chains per block; 0 = auto), `rng_bits` (52 | 32: opt-in cheaper uniform stream of solver="vegas", see
    mci_set_rng_bits), `rng_rounds` (10 | 7: opt-in Philox4x32-7 for every stream, mci_set_rng_rounds), `deterministic` (bit-identical
    results for a fixed seed like the reference's sequential loop, mci_set_deterministic), `trace` (None, the default, and True: a
    Python closure as integrand or measure is run once on symbolic draws and written out as device source -- trace.trace_integrand /
    trace_measure -- so that it runs inside the kernels like Julia's inlined closure does in the reference's loop; a closure that
    cannot be written out takes the host batch-callback path, silently with None, with a RuntimeWarning naming the reason with True;
    False: always the host path), `integrand_form` / `measure_form` (callback_form: by default a closure is called in the form the
    reference's solver calls it in -- `inplace` included -- and one whose parameters do not fit raises TypeError), `stratify` (True or
    Stratify(beta, nstrat, max_nhcube, carry): VEGAS+ adaptive stratified sampling under solver="vegas", see Stratify), `engine_factory`
    (test seam)."""
    if trace is None:
        trace = TRACE_DEFAULT
    if solver in (":vegas", ":vegasmc", ":mcmc"):
        solver = solver[1:]
    if solver not in SOLVERS:
        raise ValueError("Solver %s is not supported!" % solver)                      # main.jl:263
    print = max(print, verbose)                                                       # main.jl:93
    if config is None:
        config = Configuration(**kwargs)                                              # main.jl:95-97
    for mx, v in zip(config.maxdof, config.var):
        assert mx + 2 <= v.size, "maxdof should be less than the length of var"      # main.jl:99-101
    if ignore is None:
        ignore = 1 if adapt else 0                                                    # main.jl:82
    comm = comm or LocalComm()
    strat = _stratify_request(stratify, solver, config, integrand, measure, measurefreq, trace, comm)
    if device is None:   # an RcclComm is bound to one device: the engine has to live there (its all_reduce checks it)
        device = getattr(comm, "device", 0)
    neval = int(neval)
    nevalperblock, block = standardize_block(neval, block, comm.size)                 # main.jl:121
    assert block % comm.size == 0                                                     # main.jl:122
    per = block // comm.size
    lo, hi = per * comm.rank, per * (comm.rank + 1)

    eng = _bind(config, integrand, measure, solver, inplace=inplace, trace=trace, print=print, device=device, engine_factory=engine_factory,
                rng_bits=rng_bits, rng_rounds=rng_rounds, deterministic=deterministic, integrand_form=integrand_form, measure_form=measure_form)
    s = SOLVERS[solver]
    if strat is not None:
        if isinstance(eng.integrand, HostIntegrand):
            raise ValueError("stratify: refused for a host integrand (the closure did not trace): device source or a traced closure only")
        if strat.carry:   # (the allocation starts from what this engine learned or loaded; a test double may not know the keyword)
            eng.set_stratification(strat.nstrat, strat.beta, strat.max_nhcube, carry=True)
        else:             # (the allocation starts uniform)
            eng.set_stratification(strat.nstrat, strat.beta, strat.max_nhcube)
        eng._strat_on = True
    elif getattr(eng, "_strat_on", False):   # a plain call on an engine an earlier call stratified: the plain kernels again
        eng.set_stratification(on=False)
        eng._strat_on = False
    if hasattr(eng, "set_reweight_goal"):
        eng.set_reweight_goal(reweight_goal)                                          # main.jl:81, :334-337

    t0 = time.time()
    means, stds = [], []
    neval_done = 0
    warmup = 0                             # launches run again instead of being counted (automatic :mcmc chain lengths)
    neval_discarded = 0
    block_mean, correlated = None, False   # chain solvers: every block's mean of every iteration | the iterations continued each other's chains
    if type(comm) is LocalComm and engine_factory is None and hasattr(eng, "integrate") and getattr(eng, "comm_ranks", lambda: 0)() == 1:
        # one process: the whole loop runs inside the library (mci_integrate: the iterations are queued back to back on the
        # engine's stream and the statistics of all of them are read back once -- 22 us per launch-bound iteration instead of
        # 82 us with a host round trip per iteration, tools/call_overhead.py).  Same iterations, same numbers as the loop below.
        r = eng.integrate(s, nevalperblock * block, niter=niter, block=block, ignore=ignore, adapt=adapt, gamma=gamma,
                          measurefreq=measurefreq, seed=config.seed, nchain=nchain, first_iteration=config.iterations_done,
                          thermal_ratio=thermal_ratio, reweight_goal=reweight_goal)
        means, stds = list(r["iter_mean"]), list(r["iter_std"])
        block_mean, correlated, warmup = r.get("block_mean"), r.get("correlated", False), r.get("warmup", 0)
        neval_discarded = r.get("neval_discarded", 0)
        neval_done = nevalperblock * block * niter
        niter_loop = 0
        config.visited = r["visited"]    # config.visited of the last iteration (configuration.jl:46), for report(config)
    else:
        niter_loop = niter
        if s != VEGAS and hasattr(eng, "reset_block_log"):
            eng.reset_block_log()
    for it in range(niter_loop):                                                      # main.jl:142
        attempt = 0
        if hasattr(eng, "set_iteration_counted"):
            eng.set_iteration_counted(it >= ignore)                                   # (main.jl:82, :211; what mci_integrate tells its launches)
        while True:
            eng.run(s, nevalperblock, lo, hi, config.iterations_done + it + 16384 * attempt, config.seed, measurefreq, nchain, thermal_ratio)   # main.jl:152-166
            comm.all_reduce(eng)                                                      # main.jl:177-188
            fin_solver = s                                                            # doReweight! runs on the device (main.jl:183)
            m, e = eng.finish(fin_solver, block, adapt, gamma)                        # main.jl:190-203
            # warm-up of the automatic :mcmc chain length, like mci_integrate: an iteration whose chains were too short for the holds
            # they measured is run again (longer chains, new streams) instead of being counted, until the first one that is long enough
            if (s != MCMC or nchain > 0 or not hasattr(eng, "mcmc_launch_valid") or (it == 0 and ignore >= 1) or attempt >= 7
                    or config.iterations_done + it >= 16384 or eng.last_chain_launch()[0] <= 1):
                break
            valid, warm, _, _ = eng.mcmc_launch_valid()
            if valid or warm:
                break
            eng.discard_iteration()
            attempt += 1
            warmup += 1
            neval_discarded += nevalperblock * block
        means.append(m)
        stds.append(e)
        neval_done += nevalperblock * block
    if niter_loop and hasattr(eng, "set_iteration_counted"):
        eng.set_iteration_counted(False)
    config.iterations_done += niter
    config.neval = nevalperblock * block
    config._last_solver = solver
    if niter_loop and hasattr(eng, "get_packed"):   # config.visited of the last iteration (configuration.jl:46), for report(config)
        try:
            pk = eng.get_packed()
            config.visited = pk[2 * eng.nobs + 2: 2 * eng.nobs + 2 + config.N + 1].copy()
        except Exception:
            pass
    if niter_loop and s != VEGAS and hasattr(eng, "block_means"):
        block_mean, ncarried = eng.block_means(niter)
        correlated = ncarried > 0
    if comm.size > 1 and block_mean is not None:
        # every rank holds its own blocks' means: gathered ONCE, here, where all ranks take part (a sum of arrays that are zero outside the
        # rank's own blocks), so that the Result is plain data and Result.with_ignore never enters a collective
        full = np.zeros((np.asarray(block_mean).shape[0], block, np.asarray(block_mean).shape[2]))
        full[:, lo:hi, :] = block_mean
        block_mean = np.asarray(comm.sum_host(eng, full.ravel())).reshape(full.shape)
    res = Result(np.array(means), np.array(stds), config, ignore, neval=neval_done, seconds=time.time() - t0, block_mean=block_mean,
                 correlated=correlated, block=block)   # main.jl:211
    if s != VEGAS and hasattr(eng, "last_chain_launch") and hasattr(eng, "acceptance"):
        try:   # one chain per block: what its ratio estimator costs at this block length (statistics.chain_estimator_bias; a note of report())
            pr, ac = eng.acceptance()
            res.chain_bias = chain_estimator_bias(solver, nevalperblock, eng.last_chain_launch()[0], block, niter - ignore, pr, ac, eng.ndraw)
        except Exception:
            res.chain_bias = None
    res.stratification = eng.stratification() if strat is not None else None   # {nstrat, ncube, beta, carry, carried} of a stratified run
    if res.stratification is not None:
        res.stratification.setdefault("carry", False)
        res.stratification.setdefault("carried", "uniform")
    if s == VEGAS and hasattr(eng, "vegas_check_status"):
        try:   # was the kernel that produced these grids checked?  (status, flags) of mci_vegas_check_status; a note of report() when negative
            res.vegas_check = eng.vegas_check_status()
        except Exception:
            res.vegas_check = None
    res.warmup = warmup   # launches that were run again instead of being counted (automatic :mcmc chain lengths)
    res.neval_discarded = neval_discarded   # ... and their evaluations: spent (they trained the map), in neither res.neval nor the estimate
    if print >= 0:
        report(res, io=printio)                                                       # main.jl:212-213
    return res


class _MeasureConfig:
    """the configuration a sweep's measure closure is traced on: point 0's, with every read off config.userdata on record"""

    def __init__(self, config, userdata, rec):
        from . import trace as tr
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
    from . import trace as tr
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
    import copy
    import warnings
    if trace is None:
        trace = TRACE_DEFAULT
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
    if seeds is not None and len(seeds) != P:
        raise ValueError("integrate_sweep: seeds must hold one seed per point (%d), got %d" % (P, len(seeds)))
    if maps is not None and len(maps) != P:
        raise ValueError("integrate_sweep: maps must hold one map per point (%d), got %d" % (P, len(maps)))
    if carry not in (False, True):
        raise ValueError("integrate_sweep: carry must be True or False, got %r" % (carry,))
    if carry:
        if stratify is not None and stratify is not False:
            raise ValueError("integrate_sweep: carry= and stratify= do not go together (stratification is :vegas's)")
        if solver == "vegas":
            raise ValueError('integrate_sweep: carry= belongs to a chain sweep (solver="vegasmc", chains=K or solver="mcmc", mcmc_chains=K); "vegas" has no chains')
        if chains is None and mcmc_chains is None:
            raise ValueError("integrate_sweep: carry= belongs to a chain sweep: give chains=K (solver=\"vegasmc\") or mcmc_chains=K (solver=\"mcmc\")")
    until = rtol is not None or atol is not None
    if min_niter is not None and not until:
        raise ValueError("integrate_sweep: min_niter= belongs to a target error: give rtol= or atol=")
    if until:
        if solver != "vegas":
            raise ValueError("integrate_sweep: rtol= / atol= / min_niter=: solver is not :vegas (chain solvers are not swept)")
        for name, given in (("stratify", stratify is not None and stratify is not False), ("chains", chains is not None), ("mcmc_chains", mcmc_chains is not None)):
            if given:
                raise ValueError("integrate_sweep: rtol= / atol= / min_niter= and %s= do not go together (the stratified, :vegasmc and :mcmc "
                                 "sweeps have no target error)" % name)
        if min_niter is not None and (isinstance(min_niter, bool) or not isinstance(min_niter, (int, np.integer))):
            raise ValueError("integrate_sweep: min_niter must be an int >= 0, got %r" % (min_niter,))
    if chains is not None and mcmc_chains is not None:
        raise ValueError('integrate_sweep: chains= (solver="vegasmc") and mcmc_chains= (solver="mcmc") do not go together')
    if chains is not None:
        if isinstance(chains, bool) or not isinstance(chains, (int, np.integer)) or chains < 1:
            raise ValueError("integrate_sweep: chains must be an int >= 1 (chains per block), got %r" % (chains,))
        if solver != "vegasmc":
            raise ValueError('integrate_sweep: chains= belongs to solver="vegasmc" (%s)'
                             % ('"vegas" is swept without it' if solver == "vegas" else 'a sweep of "mcmc" points is a follow-up'))
        if stratify is not None and stratify is not False:
            raise ValueError("integrate_sweep: chains= and stratify= do not go together (stratification is :vegas's)")
        chains = int(chains)
    if mcmc_chains is not None:
        if isinstance(mcmc_chains, bool) or not isinstance(mcmc_chains, (int, np.integer)) or mcmc_chains < 1:
            raise ValueError("integrate_sweep: mcmc_chains must be an int >= 1 (chains per block), got %r" % (mcmc_chains,))
        if solver != "mcmc":
            raise ValueError('integrate_sweep: mcmc_chains= belongs to solver="mcmc" (%s)'
                             % ('"vegas" is swept without it' if solver == "vegas" else '"vegasmc" takes chains='))
        if stratify is not None and stratify is not False:
            raise ValueError("integrate_sweep: mcmc_chains= and stratify= do not go together (stratification is :vegas's)")
        mcmc_chains = int(mcmc_chains)
    if reweight is not None and chains is None and mcmc_chains is None:
        raise ValueError('integrate_sweep: reweight= belongs to a chain sweep (solver="vegasmc", chains=K)')
    if reweight is not None and len(reweight) != P:
        raise ValueError("integrate_sweep: reweight must hold one vector per point (%d), got %d" % (P, len(reweight)))
    if chain_state is not None:
        from .statistics import ChainState
        if not carry:
            raise ValueError("integrate_sweep: chain_state= belongs to a chain sweep with carried chains: give carry=True (and chains=K or mcmc_chains=K)")
        try:
            chain_state = list(chain_state)
        except TypeError:
            raise ValueError("integrate_sweep: chain_state must be a list with one ChainState per point")
        if len(chain_state) != P:
            raise ValueError("integrate_sweep: chain_state must hold one ChainState per point (%d), got %d" % (P, len(chain_state)))
        if not all(isinstance(s, ChainState) for s in chain_state):
            raise ValueError("integrate_sweep: chain_state must hold ChainState objects (the chain_state of an earlier sweep's results; None: that "
                             "call kept no chains -- carry=True and more than one chain per block)")
        nexts = sorted({s.iteration + 1 for s in chain_state})
        if len(nexts) != 1:
            raise ValueError("integrate_sweep: the chain states disagree with each other: they were stored by iterations %s"
                             % ", ".join(str(n - 1) for n in nexts))
    if alloc is not None and (stratify is None or stratify is False):
        raise ValueError("integrate_sweep: alloc= belongs to a stratified sweep (stratify=True or mci.Stratify(...))")
    if alloc is not None:
        try:
            nalloc = len(alloc)
        except TypeError:
            raise ValueError("integrate_sweep: alloc must be a list with one strat_d array per point")
        if nalloc != P:
            raise ValueError("integrate_sweep: alloc must hold one strat_d array per point (%d), got %d" % (P, nalloc))
    fresh = config is None
    pristine = copy.deepcopy(kwargs) if fresh else None
    if fresh:
        config = Configuration(**kwargs)
    if chain_state is not None:
        if fresh:
            config.iterations_done = nexts[0]    # (a fresh configuration goes on where the states' call stopped)
        elif config.iterations_done != nexts[0]:
            raise ValueError("integrate_sweep: the chain states were stored by iteration %d, and config.iterations_done = %d: the call would "
                             "not start at the iteration that continues them (%d)" % (nexts[0] - 1, config.iterations_done, nexts[0]))
    if ignore is None:
        ignore = 1 if adapt else 0
    strat = _stratify_request(stratify, solver, config, integrand, measure, measurefreq, trace, LocalComm())
    if strat is not None and strat.carry:
        raise ValueError("integrate_sweep: Stratify(carry=True) is the ordinary call's way to carry an allocation; a sweep takes alloc=")
    closure = callable(integrand) and not isinstance(integrand, (Integrand, HostIntegrand))
    why = rows = bound = None
    if closure:
        from . import trace as tr
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
            rows = np.array([bound.userdata_for(p) for p in params], dtype=np.float64).reshape(P, len(bound.userdata))
        except tr.TraceError as e:
            why = "the closure was not traced (%s): a host integrand" % e
        bound_measure = measure
        if why is None and trace is not False and callable(measure) and not isinstance(measure, (Measure, HostMeasure)) and not hasattr(measure, "pool"):
            bound_measure = _trace_sweep_measure(measure, traced_on, params, solver) or measure
    else:
        if isinstance(integrand, str):
            integrand = Integrand(integrand, None)
        if isinstance(integrand, HostIntegrand):
            why = "a host integrand (device source or a traced closure only)"
        else:
            rows = np.asarray(params, dtype=np.float64)
            if rows.ndim != 2 or (len(integrand.userdata) and rows.shape[1] != len(integrand.userdata)):
                raise ValueError("integrate_sweep: params must be userdata rows [points][%d] for this integrand, got shape %s"
                                 % (len(integrand.userdata), rows.shape))
            bound = Integrand(integrand.body, rows[0], integrand.name)
    if device is None:
        device = 0
    nevalperblock, block = standardize_block(int(neval), block, 1)
    eng = None
    if why is None:
        eng = _bind(config, bound, bound_measure if closure else measure, solver, trace=trace, print=print, device=device)
        if hasattr(eng, "set_sweep_leaves"):
            eng.set_sweep_leaves(leaves)
        if strat is not None and hasattr(eng, "set_sweep_strat_leaves"):
            eng.set_sweep_strat_leaves(leaves)      # (leaves="all" opts in to both leaf modes)
        if strat is not None:
            if not hasattr(eng, "integrate_sweep_strat"):
                why = "this engine has no stratified sweep"
            else:
                eng.set_stratification(strat.nstrat, strat.beta, strat.max_nhcube)
                why = eng.sweep_strat_supported(solver, nevalperblock * block, niter, block, measurefreq)
        elif chains is not None:
            why = (eng.sweep_chains_supported(solver, nevalperblock * block, niter, block, measurefreq, nchain=chains,
                                              first_iteration=config.iterations_done)
                   if hasattr(eng, "sweep_chains_supported") else "this engine has no chain sweep")
        elif mcmc_chains is not None:
            why = (eng.sweep_mcmc_supported(solver, nevalperblock * block, niter, block, measurefreq, nchain=mcmc_chains,
                                            first_iteration=config.iterations_done, thermal_ratio=thermal_ratio)
                   if hasattr(eng, "sweep_mcmc_supported") else "this engine has no :mcmc sweep")
        elif until:
            why = (eng.sweep_supported(solver, nevalperblock * block, niter, block, measurefreq) if hasattr(eng, "sweep_until_supported")
                   else "this engine has no sweep to a target error")
            bad = why is None and eng.sweep_until_supported(solver, nevalperblock * block, niter, block, measurefreq, rtol=rtol or 0.0, atol=atol or 0.0,
                                                            min_niter=min_niter or 0)
            if bad:     # (the target itself: in the words of mci_sweep_until_supported)
                raise ValueError("integrate_sweep: %s" % bad)
        else:
            why = eng.sweep_supported(solver, nevalperblock * block, niter, block, measurefreq) if hasattr(eng, "sweep_supported") else "this engine has no sweep"
    if why is None and strat is not None:
        plan = eng.sweep_strat_plan(nevalperblock * block, block)
        d_rows = _sweep_alloc_rows(alloc, P, plan) if alloc is not None else None
        rs = eng.integrate_sweep_strat(solver, userdata=rows, neval=nevalperblock * block, niter=niter, block=block, ignore=ignore, adapt=adapt,
                                       gamma=gamma, measurefreq=measurefreq, seed=config.seed, seeds=seeds, maps=maps,
                                       first_iteration=config.iterations_done, d=d_rows)
        out = []
        for p, r in zip(params, rs):
            c = copy.copy(config)            # (the points share the engine; a sweep leaves its map, logs and allocation alone)
            c.userdata = p if closure else None
            c.visited = r["visited"]
            res = Result(r["iter_mean"], r["iter_std"], c, ignore, neval=r["neval"], seconds=r["seconds"], block=block)
            res.sweep_batched, res.map, res.status = True, r["maps"], r["status"]
            res.maps_by_leaf = r.get("maps_by_leaf")
            res.stratification = dict(nstrat=list(plan["nstrat"]), ncube=plan["ncube"], beta=plan["beta"], carry=False,
                                      carried="same plan" if alloc is not None else "uniform")
            res.strat_d, res.strat_counts = StratD(r["strat_d"], plan["nstrat"], plan["beta"]), r["strat_counts"]
            res.vegas_check, res.warmup, res.neval_discarded = None, 0, 0
            if print >= 0:
                report(res)
            out.append(res)
        return out
    if why is None and (chains is not None or mcmc_chains is not None):
        kw = dict(userdata=rows, neval=nevalperblock * block, niter=niter, block=block, ignore=ignore, adapt=adapt, gamma=gamma,
                  measurefreq=measurefreq, seed=config.seed, seeds=seeds, maps=maps, first_iteration=config.iterations_done, reweight=reweight)
        if chain_state is not None:
            kw["state"] = chain_state
        rs = (eng.integrate_sweep_chains(solver, nchain=chains, carry=carry, **kw) if chains is not None
              else eng.integrate_sweep_mcmc(solver, nchain=mcmc_chains, thermal_ratio=thermal_ratio, carry=carry, **kw))
        out = []
        for p, r in zip(params, rs):
            c = copy.copy(config)            # (the points share the engine; a sweep leaves its map, factors and logs alone)
            c.userdata = p if closure else None
            c.visited = r["visited"]
            c._sweep_tables = (r["propose"], r["accept"])   # config.propose / config.accept: this point's, not the engine's
            res = Result(r["iter_mean"], r["iter_std"], c, ignore, neval=r["neval"], seconds=r["seconds"], block=block, correlated=r["correlated"])
            if r["correlated"]:              # (carried chains: the block-lineage error, made by the library from the point's block means)
                res._flat_std = np.asarray(r["stdev"], dtype=np.float64)
                res.stdev = res._shape(res._flat_std)
            res.sweep_batched, res.map, res.status, res.reweight = True, r["maps"], r["status"], r["reweight"]
            res.maps_by_leaf = r.get("maps_by_leaf")
            res.chain_state = r.get("chain_state")
            res.stratification, res.vegas_check, res.warmup, res.neval_discarded, res.chain_bias = None, None, 0, 0, None
            if mcmc_chains is not None:
                res.holds, res.hold_max, res.chain_steps = r["holds"], r["hold_max"], nevalperblock // mcmc_chains
                res.chains_carried = bool(r.get("carried"))
            if print >= 0:
                report(res)
            out.append(res)
        return out
    if why is None:
        kw = dict(userdata=rows, neval=nevalperblock * block, niter=niter, block=block, ignore=ignore, adapt=adapt, gamma=gamma, measurefreq=measurefreq,
                  seed=config.seed, seeds=seeds, maps=maps, first_iteration=config.iterations_done)
        rs = (eng.integrate_sweep_until(solver, rtol=rtol or 0.0, atol=atol or 0.0, min_niter=min_niter or 0, **kw) if until
              else eng.integrate_sweep(solver, **kw))
        out = []
        for p, r in zip(params, rs):
            c = copy.copy(config)            # (the points share the engine; a sweep leaves its map and logs alone)
            c.userdata = p if closure else None
            c.visited = r["visited"]
            res = Result(r["iter_mean"], r["iter_std"], c, ignore, neval=r["neval"], seconds=r["seconds"], block=block)
            res.sweep_batched, res.map, res.status = True, r["maps"], r["status"]
            res.maps_by_leaf = r.get("maps_by_leaf")
            res.stratification, res.vegas_check, res.warmup, res.neval_discarded = None, None, 0, 0
            if until:
                res.niter_run, res.converged = r["niter_run"], r["converged"]
            if print >= 0:
                report(res)
            out.append(res)
        return out
    # not a sweep layout: the points one after another, each an ordinary call on a configuration of its own
    if not fresh:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and the looped form builds one Configuration per "
                         "point from keywords (var=..., dof=...), not from config=" % why)
    if maps is not None:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and maps= needs the batched form" % why)
    if alloc is not None:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and alloc= needs the batched form" % why)
    if reweight is not None:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and reweight= needs the batched form" % why)
    if chain_state is not None:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and chain_state= needs the batched form" % why)
    if until:
        raise ValueError("integrate_sweep: this problem does not run as a sweep (%s), and rtol= / atol= need the batched form" % why)
    warnings.warn("integrate_sweep: this problem does not run as a sweep (%s): %d ordinary integrate() calls, one after another" % (why, P),
                  RuntimeWarning, stacklevel=2)
    if eng is not None and hasattr(eng, "close"):
        eng.close()
    out = []
    for k, p in enumerate(params):
        kw = copy.deepcopy(pristine)
        if closure:
            kw["userdata"], f = p, integrand
        else:
            f = integrand if isinstance(integrand, HostIntegrand) else Integrand(integrand.body, rows[k], integrand.name)
        c = Configuration(**kw)
        if seeds is not None:
            c.seed = int(seeds[k])
        res = integrate(f, solver=solver, config=c, neval=neval, niter=niter, block=block, gamma=gamma, adapt=adapt, ignore=ignore, measure=measure,
                        measurefreq=measurefreq, device=device, trace=trace, print=print, **({"stratify": strat} if strat is not None else {}), **({"nchain": chains} if chains is not None else {}),
                        **({"nchain": mcmc_chains, "thermal_ratio": thermal_ratio} if mcmc_chains is not None else {}))
        res.sweep_batched, res.map, res.maps_by_leaf, res.status = False, None, None, 0
        out.append(res)
    return out


def prefill_kernel_cache():
    """Compile (hiprtc, gfx950, no GPU needed) the sample-batch kernels of the BASELINE configs and of the
    test battery into the in-tree kernel cache, so that the GPU box starts from code objects."""
    import math
    L = math.sqrt(50.0)
    jobs = [
        (Configuration(var=Continuous(0.0, 1.0), dof=[[1]]), catalog.log_over_sqrt(), None),                      # C1
        (Configuration(var=Continuous(-L, L), dof=[[16]]), catalog.gaussian(16), None),                           # C2 shared pool
        (Configuration(var=Continuous([(-L, L)] * 16), dof=[[1]]), catalog.gaussian(16), None),                   # C2 16 grids
        (Configuration(var=Continuous([(0.0, 1.0)] * 32), dof=[[1]]), catalog.genz_product_peak(32), None),       # C4
    ]
    p = catalog.bubble_parameters()
    from .integrand import bin_by
    var = (Continuous(0.0, 1.0, alpha=3.0), Continuous(0.0, math.pi, alpha=3.0), Continuous(0.0, 2 * math.pi, alpha=3.0),
           Continuous(0.0, p["beta"], alpha=3.0), Discrete(1, 4, adapt=False))
    jobs.append((Configuration(var=var, dof=[[1, 1, 1, 1, 1]], obs=[np.zeros(4)]), catalog.bubble(), bin_by(4)))  # C3
    n = 0
    for cfg, f, meas in jobs:
        eng = Engine(cfg, f, measure=meas, device=-1)
        eng.compile("vegas")
        if n == 1:
            eng.compile("vegas_big")       # ... whose launches of 2^26 samples and more (bench.py's 1e8) run sixteen histogram copies
        if meas is not None:
            eng.compile("vegasmc")  # C3 is a :vegasmc config
            eng.compile("vegasmc_lanes")   # ... whose launches of few chains (the example's neval = 1e6) give every chain a group of lanes
            eng.set_sweep_leaves("all")    # ... and which is scanned over rs as one launch (integrate_sweep(..., leaves="all"))
            eng.compile("vegas_sweep_leaves")
            eng.compile("vegasmc_sweep")   # ... or, under its own solver, with integrate_sweep(..., solver="vegasmc", chains=K)
            eng.compile("mcmc_sweep")      # ... or under the reference example's, with integrate_sweep(..., solver="mcmc", mcmc_chains=K)
        eng.close()
        n += 1
    # C5: 4 integrands on a 12-D pool, :mcmc
    eng = Engine(Configuration(var=Continuous(0.0, 1.0), dof=[[3], [6], [9], [12]]), catalog.nested_gauss(), device=-1)
    eng.compile("mcmc")
    eng.compile("mcmc_lanes")   # (the pilot-length first launch of a cold call runs few, long chains)
    eng.close()
    return n + 1
