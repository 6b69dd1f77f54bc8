#!/usr/bin/env python3
"""Which code objects does the library build?  Compiles, offline (device = -1) and into an EMPTY kernel cache, every JIT unit of the
BASELINE configurations (tests/test_code_objects.py) and a few configurations that steer the :vegas kernel plan, and prints one line
per case -- file name, histogram_copies(), launch bound and VGPRs of the unit's main kernel -- and then the listing of the cache
directory with a digest per file.  File names are hashes of source, headers, options and compiler: two trees whose listings agree
generate the same sources, compile the same candidates and choose the same ones.  Run on two checkouts and diff the outputs
(profiles/r14_kernel_units.txt).  With --online (a GPU) it lists instead what only a launch compiles: the any-cadence :vegas unit
(measurefreq = 3), as the first :vegas unit of a problem and as the second.
usage: python tools/kernel_units_listing.py [--online] [--cache DIR]"""
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
CACHE = sys.argv[sys.argv.index("--cache") + 1] if "--cache" in sys.argv else tempfile.mkdtemp(prefix="mci_units_")
os.makedirs(CACHE, exist_ok=True)
assert not os.listdir(CACHE), "the kernel cache directory must be empty: %s" % CACHE
os.environ["MCI_KERNEL_CACHE"] = CACHE
import mcintegration_jl_amd as mci            # noqa: E402
from mcintegration_jl_amd import isa_mix      # noqa: E402
from mcintegration_jl_amd._lib import lib, check   # noqa: E402
from test_code_objects import BASELINE        # noqa: E402

mci.use_rocm_compiler()
ONLINE = "--online" in sys.argv
MAIN = {"vegas": "mci_vegas_batch", "vegasmc": "mci_vegasmc_chains", "mcmc": "mci_mcmc_chains", "vegasmc_lanes": "mci_vegasmc_spec",
        "mcmc_lanes": "mci_mcmc_spec", "vegas_persistent": "mci_vegas_persist", "vegas_strat": "mci_vegas_strat", "vegas_sweep": "mci_vegas_sweep",
        "vegas_sweep_leaves": "mci_vegas_sweep_leaves", "vegas_sweep_strat": "mci_vegas_sweep_strat"}


def line(case, unit, eng, prepare=None):
    try:
        if prepare:
            prepare(eng)
        eng.compile(unit)
        path = eng.code_object(unit)
        r = isa_mix.resources(path)[MAIN[unit]]
        print("%-28s %-18s %s copies=%d max_threads=%d vgpr=%d scratch=%d" % (case, unit, os.path.basename(path), eng.histogram_copies(),
                                                                               r["max_threads"], r["vgpr"], r["scratch"]), flush=True)
    except Exception as e:   # (a layout that has no such unit: the refusal is part of the listing)
        print("%-28s %-18s -- %s" % (case, unit, str(e).splitlines()[0][:110]), flush=True)


def engine(b, **kw):
    return mci.Engine(b[1](), b[2](), measure=b[3]() if b[3] else None, device=-1, **kw)


for b in BASELINE if not ONLINE else ():
    eng = engine(b)
    for unit in ("vegas", "vegasmc", "mcmc", "vegasmc_lanes", "mcmc_lanes", "vegas_persistent", "vegas_sweep"):
        line(b[0], unit, eng)
    line(b[0], "vegas_sweep_leaves", eng, lambda e: e.set_sweep_leaves("all"))
    eng.close()
    eng = engine(b)   # (stratified: a problem of its own)
    line(b[0], "vegas_strat", eng, lambda e: e.set_stratification())
    line(b[0], "vegas_sweep_strat", eng)
    eng.close()

if not ONLINE:
    c2 = [b for b in BASELINE if b[0] == "c2"][0]
    eng = engine(c2)
    line("c2 deterministic", "vegas", eng, lambda e: e.set_deterministic(True))
    eng.close()
    eng = engine(c2)
    line("c2 set_launch(128)", "vegas", eng, lambda e: e.set_launch(128))
    eng.close()
    eng = engine(c2, rng_bits=32, rng_rounds=7)
    line("c2 rng 32 bits, 7 rounds", "vegas", eng)
    eng.close()
    check(lib().mci_debug_override(b"hist_copies", 4, 1))
    try:
        eng = engine(c2)
        line("c2 hist_copies=4", "vegas", eng)
        eng.close()
    finally:
        check(lib().mci_debug_override(b"hist_copies", 0, 0))
    # the arms of the copies rule no BASELINE configuration takes (tests/test_code_objects.py): at most 80 VGPRs | more than 128
    light = mci.Engine(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[6]]),
                       mci.Integrand("double q = 0.0; for (int i = 0; i < 6; ++i) q += x[i] * x[i]; w[0] = q;"), device=-1)
    line("6-D light", "vegas", light)
    light.close()
    fat = mci.Engine(c2[1](), mci.Integrand("""double m = 0.0; for (int i = 0; i < 16; ++i) m += x[i]; m *= 0.0625;
    double y[16], q = 0.0; for (int i = 0; i < 16; ++i) { y[i] = sin(x[i] - m) * cos(x[(i + 7) % 16] + m); q += y[i]; }
    double p = 1.0; for (int i = 0; i < 16; ++i) p *= 1.0 + (y[i] - q) * exp(x[15 - i] - y[(i + 5) % 16]); w[0] = p;"""), device=-1)
    line("16-D fat", "vegas", fat)
    fat.close()

if ONLINE:   # the any-cadence :vegas unit: first alone (it makes the plan), then behind the measurefreq == 1 unit (the plan stands)
    for b in [x for x in BASELINE if x[4] == "vegas"]:
        for first in (3, 1):
            eng = mci.Engine(b[1](), b[2](), device=0)
            for mf in (first, 4 - first):
                eng.iteration("vegas", 512, 0, 2, iteration=0, seed=1, measurefreq=mf)
                print("%-28s vegas mf=%d (first %d) %s copies=%d" % (b[0], mf, first, os.path.basename(eng.code_object("vegas")), eng.histogram_copies()), flush=True)
            eng.close()

print("\n# kernel cache")
for name in sorted(os.listdir(CACHE)):
    if name.endswith(".hsaco"):
        print(name, hashlib.sha256(open(os.path.join(CACHE, name), "rb").read()).hexdigest()[:16])
mci.shutdown()
