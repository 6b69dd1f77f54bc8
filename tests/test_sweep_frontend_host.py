"""CPU tests of the front end of mci.integrate_sweep, with the five Engine.integrate_sweep* entry points replaced by fakes on offline
engines (tests/sweep_frontend_cases.py): the outcome of every combination of its keywords -- exception type and full message, the
fallback's warning, or the kind of sweep that ran --, the malformed values the matrix leaves out, and for every kind of completed call
the Engine method it went to with exactly which keywords, the full attribute set of every point's Result and the point's configuration.
Closures: a trace that succeeds, trace=False, a later point whose parameters do not evaluate (a TraceError after the trace: the looped
form, as for any closure that does not trace), points that differ in an int, and a measure closure that is refused, or does not trace,
at the binder (tests/test_sweep_leaves_host.py holds the measure refusals on a layout with a Discrete leaf and a table)."""
import types
import warnings

import numpy as np
import pytest

import mcintegration_jl_amd as mci
import sweep_frontend_cases as K
from mcintegration_jl_amd.integrate import StratD
from mcintegration_jl_amd.statistics import Result


@pytest.fixture
def fakes(monkeypatch):
    return K.Fakes(monkeypatch)


@pytest.fixture
def looped(monkeypatch):
    seen = []
    I, fake = K.fake_integrate(seen)
    monkeypatch.setattr(I, "integrate", fake)
    return seen


# ---- (a) every keyword combination ---------------------------------------------------------------------------------------------------

def test_the_table_is_whole():
    assert len(set(K.OUTCOMES)) == len(K.OUTCOMES) <= len(K.ALPHABET)
    assert set(K.TABLE) == {(layout, solver) for layout in K.LAYOUTS for solver in K.SOLVERS}
    assert all(len(line) == 1 << len(K.FLAGS) for line in K.TABLE.values())
    ran = {layout: sum(K.OUTCOMES[K.ALPHABET.index(ch)].startswith("ran: ") for s in K.SOLVERS for ch in K.TABLE[layout, s]) for layout in K.LAYOUTS}
    warned = sum(K.OUTCOMES[K.ALPHABET.index(ch)].startswith("RuntimeWarning: ") for s in K.SOLVERS for ch in K.TABLE["refused", s])
    assert ran == {"one": 17, "refused": 12} and warned == 4


@pytest.mark.parametrize("solver", K.SOLVERS)
@pytest.mark.parametrize("layout", list(K.LAYOUTS))
def test_every_keyword_combination_ends_as_recorded(fakes, looped, layout, solver):
    line = K.TABLE[layout, solver]
    wrong = []
    for i, ch in enumerate(line):
        given = K.combination(i)
        got = K.outcome(fakes, looped, layout, solver, given)
        if got != K.OUTCOMES[K.ALPHABET.index(ch)]:
            wrong.append((sorted(given), got, K.OUTCOMES[K.ALPHABET.index(ch)]))
    assert not wrong, "%d of %d, the first: %s gave %r, recorded %r" % ((len(wrong), len(line)) + wrong[0])


def sweep(f=None, params=K.ROWS, layout="one", **kw):
    return mci.integrate_sweep(f if f is not None else mci.Integrand(K.BODY, [1.0]), params, **kw, **K.LAYOUTS[layout]())


def closure(x, c):
    return x[0] * x[0] + c.userdata.a * x[1] * x[1]


def objects(values=(1.0, 0.5, 0.25)):
    return [types.SimpleNamespace(a=a) for a in values]


VMC, MC = dict(solver="vegasmc", chains=4), dict(solver="mcmc", mcmc_chains=4)
ST = dict(stratify=mci.Stratify(nstrat=K.NSTRAT))
NOT_A_SWEEP = "integrate_sweep: this problem does not run as a sweep (measurefreq = 2 (a sweep measures every sample)), and "

MALFORMED = [
    (dict(solver="foo"), "Solver foo is not supported!"),
    (dict(leaves="some"), "integrate_sweep: leaves must be \"one\" or \"all\", got 'some'"),
    (dict(params=5), "integrate_sweep: params must be a sequence with one entry per point"),
    (dict(params=[]), "integrate_sweep: 0 points; a sweep takes 1 to 65536"),
    (dict(seeds=[1, 2]), "integrate_sweep: seeds must hold one seed per point (3), got 2"),
    (dict(maps=[np.zeros(5)] * 2), "integrate_sweep: maps must hold one map per point (3), got 2"),
    (dict(carry=2), "integrate_sweep: carry must be True or False, got 2"),
    (dict(params=[[1.0, 2.0]] * 3), "integrate_sweep: params must be userdata rows [points][1] for this integrand, got shape (3, 2)"),
    (dict(rtol=1e-3, min_niter=2.5), "integrate_sweep: min_niter must be an int >= 0, got 2.5"),
    (dict(atol=1e-3, min_niter=True), "integrate_sweep: min_niter must be an int >= 0, got True"),
    (dict(rtol=-1e-3), "integrate_sweep: rtol is negative or not finite"),
    (dict(atol=float("nan")), "integrate_sweep: atol is negative or not finite"),
    (dict(rtol=1e-3, min_niter=-2), "integrate_sweep: min_niter < 0"),
    (dict(stratify=3), "stratify = 3: True or mci.Stratify(beta=..., nstrat=..., max_nhcube=..., carry=...)"),
    (dict(stratify=True, measurefreq=2), "stratify: refused for measurefreq = 2 (every sample is measured)"),
    (dict(stratify=mci.Stratify(carry=True)), "integrate_sweep: Stratify(carry=True) is the ordinary call's way to carry an allocation; a sweep takes alloc="),
    (dict(ST, alloc=5), "integrate_sweep: alloc must be a list with one strat_d array per point"),
    (dict(ST, alloc=[np.ones(12)] * 2), "integrate_sweep: alloc must hold one strat_d array per point (3), got 2"),
    (dict(ST, alloc=[np.ones(12), np.ones(11), np.ones(12)]), "integrate_sweep: alloc[1] has shape (11,), the plan nstrat = [4, 3] has 12 hypercubes"),
    (dict(ST, alloc=[StratD(np.ones(12), [3, 4], 0.75)] * 3), "integrate_sweep: alloc[0] was measured on nstrat = [3, 4] under beta = 0.75, this call runs "
                                                              "nstrat = [4, 3] under beta = 0.75 (there is no remap in a sweep)"),
    (dict(VMC, reweight=[np.ones(2)] * 2), "integrate_sweep: reweight must hold one vector per point (3), got 2"),
    (dict(VMC, carry=True, chain_state=5), "integrate_sweep: chain_state must be a list with one ChainState per point"),
    (dict(VMC, carry=True, chain_state=[K.chain_state()] * 2), "integrate_sweep: chain_state must hold one ChainState per point (3), got 2"),
    (dict(MC, carry=True, chain_state=[K.chain_state(), None, K.chain_state()]),
     "integrate_sweep: chain_state must hold ChainState objects (the chain_state of an earlier sweep's results; None: that call kept no chains -- carry=True "
     "and more than one chain per block)"),
    (dict(VMC, carry=True, chain_state=[K.chain_state(4), K.chain_state(6), K.chain_state(4)]),
     "integrate_sweep: the chain states disagree with each other: they were stored by iterations 4, 6"),
    (dict(measurefreq=2, maps=[np.zeros(5)] * 3), NOT_A_SWEEP + "maps= needs the batched form"),
    (dict(VMC, measurefreq=2, reweight=[np.ones(2)] * 3), NOT_A_SWEEP + "reweight= needs the batched form"),
    (dict(MC, measurefreq=2, carry=True, chain_state=[K.chain_state()] * 3), NOT_A_SWEEP + "chain_state= needs the batched form"),
    (dict(MC, measurefreq=2, carry=True, maps=[np.zeros(5)] * 3, reweight=[np.ones(2)] * 3, chain_state=[K.chain_state()] * 3),
     NOT_A_SWEEP + "maps= needs the batched form"),
    (dict(atol=1e-3, measurefreq=2), NOT_A_SWEEP + "rtol= / atol= need the batched form"),
    (dict(f=closure, params=objects(), trace=False, maps=[np.zeros(5)] * 3),
     "integrate_sweep: this problem does not run as a sweep (the closure was not traced (trace = False): a host integrand), and maps= needs the batched form"),
    (dict(f=closure, params=[types.SimpleNamespace(a=1.0), types.SimpleNamespace(a=2)]),
     "the points would trace to different bodies: parameter userdata.a (TypeError: 2 is no float)"),
]


def huge(x, c):
    return x[0] * x[1] * (c.userdata.a * 1e300)


def reads_a_float(var, obs, weights, c):
    obs[0] += weights[0] * c.userdata.a


def reads_an_int(var, obs, weights, c):
    obs[0] += weights[0] * (1.0 if c.userdata.n > 1 else 2.0)


def plain_measure(var, obs, weights, c):
    obs[0] += weights[0]


NOT_TRACED = ("integrate_sweep: this problem does not run as a sweep (the closure was not traced (a captured parameter evaluates to a non-finite "
              "value): a host integrand)")
OVERFLOWS = [types.SimpleNamespace(a=1.0), types.SimpleNamespace(a=1e300), types.SimpleNamespace(a=2.0)]      # (a * 1e300 at the second point)
WITH_N = [types.SimpleNamespace(a=1.0, n=1), types.SimpleNamespace(a=0.5, n=2), types.SimpleNamespace(a=0.25, n=1)]
MALFORMED += [
    (dict(f=huge, params=OVERFLOWS, maps=[np.zeros(5)] * 3), NOT_TRACED + ", and maps= needs the batched form"),
    (dict(f=huge, params=OVERFLOWS, rtol=1e-3), NOT_TRACED + ", and rtol= / atol= need the batched form"),
    (dict(ST, f=huge, params=OVERFLOWS, alloc=[np.ones(12)] * 3), NOT_TRACED + ", and alloc= needs the batched form"),
    (dict(f=closure, params=WITH_N, measure=reads_a_float),
     "integrate_sweep: the measure reads userdata.a off config.userdata, and its value would be written into the measure's body: a sweep has one ud "
     "row per point, and that row is the integrand's"),
    (dict(f=closure, params=WITH_N, measure=reads_an_int),
     "integrate_sweep: the measure reads userdata.n, which is 1 at the traced point and 2 at another: the points would trace to different measure bodies"),
    (dict(f=closure, params=[WITH_N[0]] + objects((0.5, 0.25)), measure=reads_an_int),
     "integrate_sweep: the measure reads userdata.n, which cannot be read at every point (AttributeError: 'types.SimpleNamespace' object has no "
     "attribute 'n')"),
]
for name, solver in (("chains", "vegasmc"), ("mcmc_chains", "mcmc")):
    for bad in (0, True, 2.5):
        MALFORMED.append(({"solver": solver, name: bad}, "integrate_sweep: %s must be an int >= 1 (chains per block), got %r" % (name, bad)))


@pytest.mark.parametrize("k", range(len(MALFORMED)))
def test_a_malformed_value_raises_by_name(fakes, looped, k):
    kw, message = MALFORMED[k]
    with pytest.raises(ValueError) as e:
        sweep(**kw)
    assert str(e.value) == message and type(e.value) is ValueError
    assert not fakes.calls and not looped


def test_config_next_to_a_refusal_or_to_other_chain_states_raises(fakes, looped):
    def cfg():
        return mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]])
    f = mci.Integrand(K.BODY, [1.0])
    with pytest.raises(ValueError) as e:
        mci.integrate_sweep(f, K.ROWS, config=cfg(), measurefreq=2, maps=[np.zeros(5)] * 3, device=-1)
    assert str(e.value) == ("integrate_sweep: this problem does not run as a sweep (measurefreq = 2 (a sweep measures every sample)), and the looped form "
                            "builds one Configuration per point from keywords (var=..., dof=...), not from config=")
    with pytest.raises(ValueError) as e:
        mci.integrate_sweep(f, K.ROWS, config=cfg(), carry=True, chain_state=[K.chain_state()] * 3, device=-1, **VMC)
    assert str(e.value) == ("integrate_sweep: the chain states were stored by iteration 4, and config.iterations_done = 0: the call would not start at "
                            "the iteration that continues them (5)")
    assert not fakes.calls and not looped


# ---- (b) every completed call ----------------------------------------------------------------------------------------------------------

def same(a, b):
    """equal in type and value, arrays in dtype, shape and every element"""
    if a is b:
        return True
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    return type(a) is type(b) and a == b


KW = dict(neval=16000, niter=4, block=16)      # (standardize_block: 1000 evaluations in each of 16 blocks)
COMMON = dict(neval=16000, niter=4, block=16, ignore=1, adapt=True, gamma=1.0, measurefreq=1, seed=7, seeds=None, maps=None, first_iteration=0)


def config():
    return mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2]], seed=7)


def check_call(fakes, name, solver, **own):
    """the one Engine call of the sweep: its method, its solver and exactly these keywords; -> the dicts it answered with"""
    assert len(fakes.calls) == 1
    got_name, got_solver, kw = fakes.calls[0]
    want = dict(COMMON, userdata=np.array(K.ROWS), **own)
    assert (got_name, got_solver) == (name, solver)
    assert sorted(kw) == sorted(want)
    for k in want:
        assert same(kw[k], want[k]), (k, kw[k], want[k])
    return fakes.answers[0]


def check_points(results, answers, cfg, userdata, added, ignore=1, tables=False, done=0):
    """every Result: vars(res) in names and values -- what Result makes of the point's rows, the attributes every sweep point has, and
    added(q, r) of the kind --, and the point's own configuration"""
    assert len(results) == len(answers) == K.P
    for q, (res, r) in enumerate(zip(results, answers)):
        c = res.config
        ref = Result(r["iter_mean"], r["iter_std"], c, ignore, neval=r["neval"], seconds=r["seconds"], block=16, correlated=r["correlated"])
        want = dict(vars(ref), sweep_batched=True, map=r["maps"], status=r["status"], maps_by_leaf=r["maps_by_leaf"], warmup=0, neval_discarded=0)
        want.update(added(q, r))
        got = vars(res)
        assert sorted(got) == sorted(want)
        for k in want:
            if k == "iterations":
                assert len(got[k]) == len(want[k]) and all(same(g[:2], w[:2]) and g[2] is c for g, w in zip(got[k], want[k]))
            else:
                assert same(got[k], want[k]), (q, k, got[k], want[k])
        assert c is not cfg and c._engine is cfg._engine and c.visited is r["visited"]
        assert c.userdata is userdata[q] if userdata is not None else c.userdata is None
        if tables:
            assert c._sweep_tables[0] is r["propose"] and c._sweep_tables[1] is r["accept"] and c.propose is r["propose"] and c.accept is r["accept"]
        else:
            assert c._sweep_tables is None
    assert cfg.iterations_done == done and cfg.userdata is None and cfg._sweep_tables is None
    assert len({id(res.config) for res in results}) == K.P


def nothing(q, r):
    return {}


def test_a_fixed_sweep_of_device_source(fakes):
    cfg, seeds, maps = config(), [11, 12, 13], [np.linspace(0.0, 1.0, 5)] * 3
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, seeds=seeds, maps=maps, gamma=0.5, device=-1, **KW)
    answers = check_call(fakes, "integrate_sweep", "vegas", seeds=seeds, maps=maps, gamma=0.5)
    check_points(rs, answers, cfg, None, nothing)
    assert not hasattr(rs[0], "reweight") and not hasattr(rs[0], "strat_d")


def test_a_fixed_sweep_of_a_closure(fakes):
    cfg, ps = config(), objects()
    rs = mci.integrate_sweep(closure, ps, config=cfg, adapt=False, device=-1, **KW)
    answers = check_call(fakes, "integrate_sweep", "vegas", adapt=False, ignore=0)
    check_points(rs, answers, cfg, ps, nothing, ignore=0)
    assert list(cfg._engine.integrand.userdata) == [1.0]       # (traced once, on params[0])


def test_a_sweep_to_a_target_error_that_stops_early(monkeypatch):
    fakes = K.Fakes(monkeypatch, niter_run=3)
    cfg = config()
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, rtol=1e-3, min_niter=3, solver=":vegas", device=-1, **KW)
    answers = check_call(fakes, "integrate_sweep_until", "vegas", rtol=1e-3, atol=0.0, min_niter=3)
    check_points(rs, answers, cfg, None, lambda q, r: dict(niter_run=3, converged=True))
    assert rs[0].iter_mean.shape == (3, 1) and len(rs[0].iterations) == 3 and rs[0].neval == 48000


def test_a_sweep_to_a_target_error_that_runs_out(fakes):
    cfg = config()
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, atol=1e-9, device=-1, **KW)
    answers = check_call(fakes, "integrate_sweep_until", "vegas", rtol=0.0, atol=1e-9, min_niter=0)
    check_points(rs, answers, cfg, None, lambda q, r: dict(niter_run=4, converged=False))


@pytest.mark.parametrize("with_alloc", [False, True])
def test_a_stratified_sweep(fakes, with_alloc):
    cfg = config()
    alloc = [StratD(np.arange(12.0) + q, K.NSTRAT, 0.75) for q in range(K.P)] if with_alloc else None
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, alloc=alloc, device=-1, **ST, **KW)
    answers = check_call(fakes, "integrate_sweep_strat", "vegas", d=np.array([np.arange(12.0) + q for q in range(K.P)]) if with_alloc else None)

    def added(q, r):
        return dict(stratification=dict(nstrat=[4, 3], ncube=12, beta=0.75, carry=False, carried="same plan" if with_alloc else "uniform"),
                    strat_d=np.asarray(r["strat_d"]).view(StratD), strat_counts=r["strat_counts"])
    check_points(rs, answers, cfg, None, added)
    for res in rs:
        assert type(res.strat_d) is StratD and res.strat_d.nstrat == [4, 3] and res.strat_d.beta == 0.75
    assert not hasattr(rs[0], "reweight") and rs[0].niter_run is None


def chain_added(q, r):
    return dict(reweight=r["reweight"], chain_state=r["chain_state"])


def test_a_fresh_chain_sweep(fakes):
    cfg, rw = config(), [np.array([1.0, 2.0])] * 3
    rs = mci.integrate_sweep(closure, objects(), config=cfg, reweight=rw, device=-1, **VMC, **KW)
    answers = check_call(fakes, "integrate_sweep_chains", "vegasmc", nchain=4, carry=False, reweight=rw)
    check_points(rs, answers, cfg, [r.config.userdata for r in rs], chain_added, tables=True)
    assert all(r.chain_state is None and not r.correlated for r in rs)


def test_a_carried_chain_sweep_that_goes_on_from_states(monkeypatch):
    """correlated = True: the lineage stdev of the engine's dict replaces the one Result averaged"""
    fakes = K.Fakes(monkeypatch, correlated=True, chain_states=True)
    states = [K.chain_state()] * 3
    cfg = config()
    cfg.iterations_done = 5
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, carry=True, chain_state=states, chains=np.int64(4), solver="vegasmc",
                             device=-1, **KW)
    answers = check_call(fakes, "integrate_sweep_chains", "vegasmc", nchain=4, carry=True, reweight=None, state=states, first_iteration=5)
    assert type(fakes.calls[0][2]["nchain"]) is int

    def added(q, r):
        return dict(chain_added(q, r), _flat_std=np.array([0.75 + q]), stdev=[0.75 + q])
    check_points(rs, answers, cfg, None, added, tables=True, done=5)
    assert all(r.correlated and r.chain_state.iteration == 8 and r.config.iterations_done == 5 for r in rs)
    # a fresh configuration goes on where the states' call stopped
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, carry=True, chain_state=states, chains=4, solver="vegasmc", **K.LAYOUTS["one"](), **KW)
    assert fakes.calls[1][2]["first_iteration"] == 5 and all(r.config.iterations_done == 5 for r in rs)


@pytest.mark.parametrize("carry", [False, True])
def test_an_mcmc_sweep(monkeypatch, carry):
    fakes = K.Fakes(monkeypatch, correlated=carry, chain_states=carry)
    cfg = config()
    rs = mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=cfg, carry=carry, thermal_ratio=0.25, device=-1, **MC, **KW)
    answers = check_call(fakes, "integrate_sweep_mcmc", "mcmc", nchain=4, carry=carry, reweight=None, thermal_ratio=0.25)

    def added(q, r):
        own = dict(chain_added(q, r), holds=r["holds"], hold_max=r["hold_max"], chain_steps=250, chains_carried=carry)
        return dict(own, _flat_std=np.array([0.75 + q]), stdev=[0.75 + q]) if carry else own
    check_points(rs, answers, cfg, None, added, tables=True)


def test_print_reports_every_point(fakes, capsys):
    mci.integrate_sweep(mci.Integrand(K.BODY, [1.0]), K.ROWS, config=config(), print=0, device=-1, **KW)
    assert capsys.readouterr().out.count("Integral 1") >= K.P


# ---- the fallback's ordinary calls -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fixed", "strat", "chains", "mcmc"])
def test_the_fallback_hands_the_kinds_keywords_to_integrate(fakes, looped, kind):
    own = dict(fixed={}, strat=ST, chains=VMC, mcmc=dict(MC, thermal_ratio=0.2))[kind]
    layout = "refused" if kind == "strat" else "one"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rs = sweep(layout=layout, seeds=[5, 6, 7], gamma=0.5, **dict(own, **({} if kind == "strat" else {"measurefreq": 2})), **KW)
    mine = [x for x in w if "does not run as a sweep" in str(x.message)]
    assert len(mine) == 1 and mine[0].category is RuntimeWarning and mine[0].filename == __file__
    assert len(looped) == K.P and not fakes.calls
    extra = dict(fixed={}, strat=dict(stratify=ST["stratify"]), chains=dict(nchain=4), mcmc=dict(nchain=4, thermal_ratio=0.2))[kind]
    for q, (f, kw) in enumerate(looped):
        c = kw.pop("config")
        assert same(kw, dict(solver=own.get("solver", "vegas"), neval=16000, niter=4, block=16, gamma=0.5, adapt=True, ignore=1, measure=None,
                             measurefreq=1 if kind == "strat" else 2, device=-1, trace=None, print=-1, **extra))
        assert c.seed == 5 + q and c is rs[q].config and c is not looped[0][1].get("config")
        assert isinstance(f, mci.Integrand) and f.body == K.BODY and list(f.userdata) == K.ROWS[q]
        assert (rs[q].sweep_batched, rs[q].map, rs[q].maps_by_leaf, rs[q].status) == (False, None, None, 0)


@pytest.mark.parametrize("case", ["later point", "later point, stratified", "host measure"])
def test_a_closure_that_the_binder_cannot_bind_runs_as_ordinary_calls(fakes, looped, case):
    """a TraceError after the trace -- a later point's parameter evaluates to a non-finite value -- and a measure closure that does not
    trace: the looped form with its one warning, the closure and the point's object handed to integrate() as they are"""
    f, params, own = dict([("later point", (huge, OVERFLOWS, {})), ("later point, stratified", (huge, OVERFLOWS, ST)),
                           ("host measure", (closure, WITH_N, dict(measure=plain_measure)))])[case]
    why = ("a host measure (device source only)" if case == "host measure"
           else "the closure was not traced (a captured parameter evaluates to a non-finite value): a host integrand")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rs = sweep(f=f, params=params, **own, **KW)
    mine = [str(x.message) for x in w if "integrate_sweep" in str(x.message)]
    assert mine == ["integrate_sweep: this problem does not run as a sweep (%s): 3 ordinary integrate() calls, one after another" % why]
    assert not fakes.calls and len(looped) == K.P and not any(r.sweep_batched for r in rs)
    for q, (g, kw) in enumerate(looped):
        assert g is f and kw["config"].userdata is params[q] and kw["measure"] is own.get("measure") and kw.get("stratify") is own.get("stratify")


# ---- the pieces on their own: the table, the request check, the point-result builder --------------------------------------------------

def test_the_table_of_kinds_names_engine_methods_that_exist():
    from mcintegration_jl_amd import sweep as S
    assert list(S.KINDS) == ["fixed", "until", "strat", "chains", "mcmc"]
    assert [k.flag for k in S.KINDS.values()] == [None, "until", "stratify", "chains", "mcmc_chains"]
    for kind in S.KINDS.values():
        for name in (kind.query, kind.run, kind.demands):
            assert name is None or callable(getattr(mci.Engine, name))
        assert kind.solver in K.SOLVERS and set(kind.owns) <= set(S.INPUTS)
        assert set(kind.asks) <= set(vars(S._request(K.ROWS)))         # (the query's keywords are fields of the request)
    assert {K.KIND_OF[k.run] for k in S.KINDS.values()} == set(S.KINDS)
    owned = {name for k in S.KINDS.values() for name in k.owns}
    assert owned == {name for name, (belongs, needs) in S.INPUTS.items() if belongs}      # (config= and maps= go with every kind)


def test_the_request_check_alone():
    from mcintegration_jl_amd import sweep as S
    rq = S._request(K.ROWS, None, ":vegas")
    assert rq.kind is S.KINDS["fixed"] and (rq.P, rq.solver, rq.nchain, rq.chain_state, rq.first_iteration) == (3, "vegas", None, None, None)
    assert rq.inputs == dict(config=None, maps=None, reweight=None, chain_state=None, alloc=None, tolerance=None)
    assert S._request(K.ROWS, None, "vegas", atol=1e-3, min_niter=np.int64(3)).kind is S.KINDS["until"]
    assert S._request(K.ROWS, None, "vegas", stratify=True, alloc=np.ones((3, 12))).kind is S.KINDS["strat"]
    assert S._request(K.ROWS, None, "vegas", stratify=False).kind is S.KINDS["fixed"]
    states = (K.chain_state(6) for _ in range(3))                         # (any iterable: the request holds a list)
    rq = S._request(K.ROWS, None, "mcmc", mcmc_chains=np.int32(8), carry=True, chain_state=states, reweight=np.ones((3, 2)))
    assert rq.kind is S.KINDS["mcmc"] and type(rq.nchain) is int and rq.nchain == 8 and rq.first_iteration == 7
    assert type(rq.chain_state) is list and len(rq.chain_state) == 3 and rq.inputs["chain_state"] is rq.chain_state
    assert [name for name, v in rq.inputs.items() if v is not None] == ["reweight", "chain_state"]
    # precedence: the first check in the order of the function decides
    for kw, needle in ((dict(solver="foo", leaves="some"), "Solver foo"), (dict(leaves="some", seeds=[1]), "leaves must be"),
                       (dict(seeds=[1], maps=[1]), "seeds must hold"), (dict(maps=[1], carry=2), "maps must hold"),
                       (dict(carry=True, stratify=True, min_niter=2), "carry= and stratify="), (dict(min_niter=2, chains=0), "min_niter= belongs"),
                       (dict(rtol=1.0, min_niter=2.5, stratify=True), "and stratify= do not"), (dict(chains=0, mcmc_chains=0), "chains= (solver="),
                       (dict(chains=0, stratify=True, solver="mcmc"), "chains must be an int"), (dict(chains=2, stratify=True, solver="mcmc"), "follow-up"),
                       (dict(solver="vegasmc", chains=2, reweight=[1], alloc=[1]), "reweight must hold"),
                       (dict(solver="vegasmc", chains=2, reweight=[1] * 3, alloc=[1]), "alloc= belongs"),
                       (dict(solver="vegasmc", chains=2, chain_state=[1] * 3, alloc=[1]), "chain_state= belongs")):
        with pytest.raises(ValueError) as e:
            S._request(K.ROWS, **kw)
        assert needle in str(e.value), (kw, str(e.value))


@pytest.mark.parametrize("kind", ["fixed", "until", "strat", "chains", "mcmc"])
def test_the_point_result_builder_alone(kind, capsys):
    from mcintegration_jl_amd import sweep as S
    cfg, p = config(), types.SimpleNamespace(a=2.0)
    kw = dict(neval=16000, niter=4, first_iteration=0, nchain=4)
    r = K.point_dict(kind, 1, 4, kw, correlated=kind == "chains", niter_run=3 if kind == "until" else None)
    before = copy_of(r)
    rq = S._request(K.ROWS, None, S.KINDS[kind].solver, **{"chains": dict(chains=4), "mcmc": dict(mcmc_chains=4)}.get(kind, {}))
    vars(rq).update(ignore=1, block=16, print=-1, neval=16000, plan=dict(nstrat=[4, 3], ncube=12, beta=0.5) if kind == "strat" else None)
    res = S._point_result(S.KINDS[kind], r, cfg, p, rq)
    assert same(r, before)                                                # (the engine's dict is read, not changed)
    assert res.config is not cfg and res.config.userdata is p and res.config.visited is r["visited"] and cfg.userdata is None
    assert (res.sweep_batched, res.status, res.warmup, res.neval_discarded, res.ignore, res.block) == (True, 1, 0, 0, 1, 16) and res.map is r["maps"]
    own = dict(fixed=set(), until=set(), strat={"strat_d", "strat_counts"}, chains={"reweight"}, mcmc={"reweight"})[kind]
    ref = Result(r["iter_mean"], r["iter_std"], res.config, 1, block=16)
    assert set(vars(res)) - set(vars(ref)) == {"sweep_batched", "map", "status", "maps_by_leaf", "warmup", "neval_discarded"} | own
    assert (res.niter_run, res.converged) == ((3, True) if kind == "until" else (None, None))
    assert res.stratification == (dict(nstrat=[4, 3], ncube=12, beta=0.5, carry=False, carried="uniform") if kind == "strat" else None)
    assert (res.hold_max, res.chain_steps) == ((3, 250) if kind == "mcmc" else (None, None))
    assert res.correlated == (kind == "chains") and res.stdev == ([1.75] if kind == "chains" else ref.stdev)
    assert (getattr(res.config, "_sweep_tables", None) is not None) == (kind in ("chains", "mcmc"))
    assert capsys.readouterr().out == ""
    rq.print = 0
    S._point_result(S.KINDS[kind], r, cfg, None, rq)
    assert "Integral 1" in capsys.readouterr().out


def copy_of(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else list(v) if isinstance(v, list) else v) for k, v in r.items()}
