"""The cases tests/test_sweep_frontend_host.py (CPU) holds the front end of mci.integrate_sweep to: the keyword matrix with the outcome of
every combination, the engine fakes that stand in for the five Engine.integrate_sweep* entry points on offline engines (device=-1), and
the made-up per-point dicts they hand back (the shape of Engine._sweep_call's).

The matrix: three solvers x presence / absence of the nine keywords of FLAGS, on a layout the sweeps take (LAYOUTS["one"]) and on one
they refuse (LAYOUTS["refused"]: two Continuous leaves without leaves="all").  OUTCOMES holds every distinct outcome once -- an exception
as "Type: message", the fallback as "RuntimeWarning: text", a completed sweep as "ran: kind" --, TABLE one letter of ALPHABET per
combination: combination i gives FLAGS[b] where bit b of i is set.  `python tests/sweep_frontend_cases.py` prints OUTCOMES and TABLE as
the code under test gives them; they were recorded before integrate_sweep was split into mcintegration.jl_amd/sweep.py and hold it to
what it did then."""
import string
import sys
import warnings

import numpy as np

import mcintegration_jl_amd as mci

BODY = "w[0] = x[0] * x[0] + ud[0] * x[1] * x[1];"
ROWS = [[1.0], [0.5], [0.25]]
P = len(ROWS)
SOLVERS = ("vegas", "vegasmc", "mcmc")
FLAGS = ("stratify", "chains", "mcmc_chains", "carry", "rtol", "min_niter", "reweight", "alloc", "chain_state")
NSTRAT = [4, 3]
ALPHABET = string.ascii_letters + string.digits

LAYOUTS = {
    "one": lambda: dict(var=mci.Continuous(0.0, 1.0), dof=[[2]], device=-1),
    "refused": lambda: dict(var=mci.Continuous([(0.0, 1.0)] * 2), dof=[[1]], device=-1),
}


def chain_state(iteration=4, solver="vegasmc", nchain=4):
    """a ChainState as an earlier carried sweep of 16 blocks would have left it (its array: zeros of the right length)"""
    st = mci.ChainState(solver, 16, nchain, 2, 2, iteration, iteration, True, np.zeros(1))
    st.data = np.zeros(st.row_doubles())
    return st


def flag_values():
    return dict(stratify=mci.Stratify(nstrat=NSTRAT), chains=4, mcmc_chains=4, carry=True, rtol=1e-3, min_niter=3, reweight=[np.ones(2)] * P,
                alloc=[np.ones(12)] * P, chain_state=[chain_state()] * P)


def combination(i):
    vals = flag_values()
    return {name: vals[name] for b, name in enumerate(FLAGS) if i >> b & 1}


# ---- the engine fakes ----------------------------------------------------------------------------------------------------------------

KIND_OF = {"integrate_sweep": "fixed", "integrate_sweep_until": "until", "integrate_sweep_strat": "strat", "integrate_sweep_chains": "chains",
           "integrate_sweep_mcmc": "mcmc"}


def point_dict(kind, q, niter, kw, correlated=False, niter_run=None, chain_states=False):
    """point q's dict of a made-up call: the keys Engine._sweep_call sets and those the kind's entry point adds"""
    rows = niter if niter_run is None else niter_run
    im = 1.0 + 0.125 * q + 0.01 * np.arange(rows, dtype=np.float64).reshape(rows, 1)
    ie = 0.05 / (1.0 + np.arange(rows, dtype=np.float64)).reshape(rows, 1)
    maps = np.linspace(0.0, 1.0, 5) ** (q + 1)
    r = dict(mean=im[-1], stdev=ie[-1], chi2=np.zeros(1), iter_mean=im, iter_std=ie, neval=kw["neval"] * rows, seconds=0.5 + q,
             visited=np.array([10.0 + q, 20.0 + q]), correlated=correlated, block_mean=None, warmup=0, neval_discarded=0, maps=maps,
             maps_by_leaf=[maps], status=q)
    if kind == "until":
        r.update(niter_run=rows, converged=rows < niter)
    if kind == "strat":
        r.update(strat_d=np.arange(12.0) + q, strat_counts=np.arange(12, dtype=np.int64) + 2 + q)
    if kind in ("chains", "mcmc"):
        tables = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2) + 100.0 * q
        r.update(reweight=np.array([1.0, 0.5 + q]), propose=tables[0], accept=tables[1], continued=kw.get("state") is not None,
                 chain_state=chain_state(kw["first_iteration"] + niter - 1, kw_solver(kind), kw["nchain"]) if chain_states else None)
        if correlated:
            r["stdev"] = np.array([0.75 + q])
    if kind == "mcmc":
        holds = np.zeros(64, dtype=np.uint64)
        holds[:q + 2] = 3
        r.update(holds=holds, hold_max=(1 << (q + 1)) - 1, carried=bool(kw.get("carry")))
    return r


def kw_solver(kind):
    return "mcmc" if kind == "mcmc" else "vegasmc"


class Fakes:
    """The five Engine.integrate_sweep* entry points replaced on the class: every call is recorded as (method name, solver, keywords) in
    `calls` and answered with point_dict()s; `shape` (correlated, niter_run, chain_states) shapes the answer."""

    def __init__(self, monkeypatch, **shape):
        self.calls, self.answers, self.shape = [], [], shape
        for name in KIND_OF:
            monkeypatch.setattr(mci.Engine, name, self._method(name))

    def _method(self, name):
        def method(eng, solver, **kw):
            self.calls.append((name, solver, kw))
            rs = [point_dict(KIND_OF[name], q, kw["niter"], kw, **self.shape) for q in range(len(kw["userdata"]))]
            self.answers.append(rs)
            return rs
        return method


def fake_integrate(seen):
    """what the tests of the fallback put in the place of integrate() on its module: records the keywords, answers with a Result"""
    I = sys.modules[mci.integrate.__module__]

    def fake(f, **kw):
        seen.append((f, kw))
        return I.Result(np.zeros((1, 1)), np.ones((1, 1)), kw["config"], 0, neval=1, seconds=0.0, block=16)
    return I, fake


def outcome(fakes, seen, layout, solver, given):
    """one call of the matrix -> its outcome, in the words of OUTCOMES"""
    ncall, nseen = len(fakes.calls), len(seen)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            rs = mci.integrate_sweep(mci.Integrand(BODY, [1.0]), ROWS, solver=solver, **given, **LAYOUTS[layout]())
        except Exception as e:
            assert len(fakes.calls) == ncall and len(seen) == nseen, "raised after it ran"
            return "%s: %s" % (type(e).__name__, e)
    assert len(rs) == P
    mine = [x for x in w if "integrate_sweep" in str(x.message)]
    if mine:
        assert len(mine) == 1 and len(fakes.calls) == ncall and len(seen) == nseen + P and not any(r.sweep_batched for r in rs)
        return "%s: %s" % (mine[0].category.__name__, mine[0].message)
    assert len(fakes.calls) == ncall + 1 and len(seen) == nseen and all(r.sweep_batched for r in rs)
    return "ran: %s" % KIND_OF[fakes.calls[-1][0]]


# ---- recorded before the split -------------------------------------------------------------------------------------------------------

OUTCOMES = [
    'ran: fixed',
    'ran: strat',
    'ValueError: integrate_sweep: chains= belongs to solver="vegasmc" ("vegas" is swept without it)',
    'ValueError: integrate_sweep: mcmc_chains= belongs to solver="mcmc" ("vegas" is swept without it)',
    'ValueError: integrate_sweep: chains= (solver="vegasmc") and mcmc_chains= (solver="mcmc") do not go together',
    'ValueError: integrate_sweep: carry= belongs to a chain sweep (solver="vegasmc", chains=K or solver="mcmc", mcmc_chains=K); "vegas" has no chains',
    "ValueError: integrate_sweep: carry= and stratify= do not go together (stratification is :vegas's)",
    'ran: until',
    'ValueError: integrate_sweep: rtol= / atol= / min_niter= and stratify= do not go together (the stratified, :vegasmc and :mcmc sweeps have no target error)',
    'ValueError: integrate_sweep: rtol= / atol= / min_niter= and chains= do not go together (the stratified, :vegasmc and :mcmc sweeps have no target error)',
    'ValueError: integrate_sweep: rtol= / atol= / min_niter= and mcmc_chains= do not go together (the stratified, :vegasmc and :mcmc sweeps have no target error)',
    'ValueError: integrate_sweep: min_niter= belongs to a target error: give rtol= or atol=',
    'ValueError: integrate_sweep: reweight= belongs to a chain sweep (solver="vegasmc", chains=K)',
    'ValueError: integrate_sweep: alloc= belongs to a stratified sweep (stratify=True or mci.Stratify(...))',
    'ValueError: integrate_sweep: chain_state= belongs to a chain sweep with carried chains: give carry=True (and chains=K or mcmc_chains=K)',
    'RuntimeWarning: integrate_sweep: this problem does not run as a sweep (solver is not :vegas (chain solvers are not swept)): 3 ordinary integrate() calls, one after another',
    "ValueError: stratify: refused for solver = 'vegasmc' (stratified sampling is a :vegas mode)",
    'ran: chains',
    "ValueError: integrate_sweep: chains= and stratify= do not go together (stratification is :vegas's)",
    'ValueError: integrate_sweep: mcmc_chains= belongs to solver="mcmc" ("vegasmc" takes chains=)',
    'ValueError: integrate_sweep: carry= belongs to a chain sweep: give chains=K (solver="vegasmc") or mcmc_chains=K (solver="mcmc")',
    'ValueError: integrate_sweep: rtol= / atol= / min_niter=: solver is not :vegas (chain solvers are not swept)',
    "ValueError: stratify: refused for solver = 'mcmc' (stratified sampling is a :vegas mode)",
    'ValueError: integrate_sweep: chains= belongs to solver="vegasmc" (a sweep of "mcmc" points is a follow-up)',
    'ran: mcmc',
    "ValueError: integrate_sweep: mcmc_chains= and stratify= do not go together (stratification is :vegas's)",
    'RuntimeWarning: integrate_sweep: this problem does not run as a sweep (2 variable leaves (a sweep point refines ONE Continuous grid)): 3 ordinary integrate() calls, one after another',
    'RuntimeWarning: integrate_sweep: this problem does not run as a sweep (2 variable leaves (a stratified sweep point refines ONE Continuous grid; several Continuous leaves are a follow-up)): 3 ordinary integrate() calls, one after another',
    'ValueError: integrate_sweep: this problem does not run as a sweep (2 variable leaves (a sweep point refines ONE Continuous grid)), and rtol= / atol= need the batched form',
    'ValueError: integrate_sweep: this problem does not run as a sweep (2 variable leaves (a stratified sweep point refines ONE Continuous grid; several Continuous leaves are a follow-up)), and alloc= needs the batched form',
]
TABLE = {
    ('one', 'vegas'): (
        'abccddeefgfgfgfghijikijifgfgfgfgllllllllfgfgfgfghijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'nbccddeefgfgfgfgnijikijifgfgfgfgllllllllfgfgfgfgnijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'ooccddeefgfgfgfgoijikijifgfgfgfgllllllllfgfgfgfgoijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'ooccddeefgfgfgfgoijikijifgfgfgfgllllllllfgfgfgfgoijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
    ),
    ('one', 'vegasmc'): (
        'pqrstteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmrstteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'nqnstteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmnstteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooostteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmostteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooostteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmostteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
    ),
    ('one', 'mcmc'): (
        'pwxxyzeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxyzeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'nwxxnzeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxnzeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooxxozeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxozeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooxxozeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxozeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
    ),
    ('refused', 'vegas'): (
        'ABccddeefgfgfgfgCijikijifgfgfgfgllllllllfgfgfgfgCijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'nDccddeefgfgfgfgnijikijifgfgfgfgllllllllfgfgfgfgnijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'ooccddeefgfgfgfgoijikijifgfgfgfgllllllllfgfgfgfgoijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
        'ooccddeefgfgfgfgoijikijifgfgfgfgllllllllfgfgfgfgoijikijifgfgfgfgmmccddeefgfgfgfgmijikijifgfgfgfgllllllllfgfgfgfgmijikijifgfgfgfg'
    ),
    ('refused', 'vegasmc'): (
        'pqrstteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmrstteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'nqnstteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmnstteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooostteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmostteeugrgtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooostteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmostteeugngtgegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
    ),
    ('refused', 'mcmc'): (
        'pwxxyzeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxyzeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'nwxxnzeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxnzeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooxxozeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxozeeugxgygegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
        'ooxxozeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvgmmxxozeeugxgngegvvvvvvvvugvgvgvglllllllluglglglgvvvvvvvvugvgvgvg'
    ),
}


if __name__ == "__main__":
    import pytest
    mp = pytest.MonkeyPatch()
    fakes, seen = Fakes(mp), []
    I, fake = fake_integrate(seen)
    mp.setattr(I, "integrate", fake)
    found, table = [], {}
    for layout in LAYOUTS:
        for solver in SOLVERS:
            line = ""
            for i in range(1 << len(FLAGS)):
                o = outcome(fakes, seen, layout, solver, combination(i))
                if o not in found:
                    found.append(o)
                line += ALPHABET[found.index(o)]
            table[(layout, solver)] = line
    mp.undo()
    print("OUTCOMES = [")
    for o in found:
        print("    %r," % o)
    print("]")
    print("TABLE = {")
    for k, line in table.items():
        print("    %r: (" % (k,))
        for at in range(0, len(line), 128):
            print("        %r" % line[at:at + 128])
        print("    ),")
    print("}")
