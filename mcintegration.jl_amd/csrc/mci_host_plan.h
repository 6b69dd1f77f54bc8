// mci_host_plan.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// the plan of one sample launch -- everything mci_iteration_run decides before it touches memory -- and the rules that fill it.  A rule takes the problem (const), the request, the test overrides and the plan so far; it makes no HIP call and writes nothing to the problem.  The steps that must touch the device (hold_consume, compile_spec, spec_self_check, spec_upload, cursor_resident) sit between the rules, in mci_iteration_run.
namespace {

// what mci_iteration_run was asked for
struct LaunchRequest {
    int32_t solver;
    int64_t nevalperblock, block_lo, block_hi, nblocks;
    int32_t iteration;
    uint64_t seed;
    int64_t measurefreq;
    double thermal_ratio;
    bool auto_chains; // (the holding times of an :mcmc launch are handed to the host only when the next one may size its chains from them)
    int kern;         // the kernel slot of the :vegas / lane-per-chain code object
};

// ... and what it decided.  Values only; the rules below fill it in the order of its fields.
struct LaunchPlan {
    int T = 0;                  // workgroup size of the :vegas / lane-per-chain kernel
    bool may_carry = false;     // the launch may continue the chains of the one before it
    int64_t nchain = 1;         // chains per block (in: what the caller asked for, <= 0 = automatic)
    double burnin = 0.0;        // :vegasmc burn-in steps of a chain
    int64_t nburn = 0;          // :mcmc burn-in steps of a chain
    int64_t units = 0;          // lanes of useful work per block
    int G = 1, spec_maxacc = 0; // lanes per chain, accept levels of their tree
    int T_launch = 0;           // workgroup size of the sample launch itself (the several-lanes-per-chain kernel has its own)
    int wpb = 0;                // workgroups per block
    bool cursor = false;        // ranges handed out by cursor
    bool hist_lds = false, split = false, atomic_flush = false;
    int ghist_buffers = 0;      // buffers an atomic flush spreads over (BatchArgs::hist_atomic)
    int64_t nrows = 0, nwg = 0; // partial rows | workgroups of the sample launch
    int64_t chunk_len = 0, nchunks = 1;     // a many-grid launch in chunks of a block's samples
    int64_t hist_rows = 0;                  // histogram rows the merge reads: nrows, or the replay's own
    int tiles_wpb = 0;                      // split-all: replay workgroups per block and tile (0: one per sample-pass row)
    int64_t hm_n = 0, hm_first = 0, hm_count = 0; // host measure: records per block | the measured-step window of a chain
    int hm_rows = 0;                              // ... rows of relative weights per record
    bool time_this_launch = false;
    bool carried() const { return may_carry && nchain > 1; }
};

void plan_threads(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    pl.T = solver_threads(p, rq.solver);
    // mid-size :vegas launches of a plain-layout kernel compiled for it: 512-thread workgroups (VegasKernelPlan::wide)
    if (rq.solver == MCI_VEGAS && p->vegas.wide && !p->vegas.threads_vegas && p->wg_per_block <= 0 && rq.nblocks * rq.nevalperblock < ((int64_t)1 << 22) &&
        rq.nblocks * rq.nevalperblock * p->shape.ndraw >= ((int64_t)1 << 19))
        pl.T = 512;
    if (rq.kern == mci_problem::kVegasBig) pl.T = kBigThreads; // (the big unit's launches, its self-check's included)
}

// dynamic LDS of the sample launch: the solver's, or the big unit's sixteen copies
int64_t plan_launch_lds(const mci_problem *p, const LaunchRequest &rq) {
    return rq.kern == mci_problem::kVegasBig ? sixteen_copies_lds(p) : solver_lds(p, rq.solver);
}

// Which launches take the big :vegas unit (mci_host_vegas_plan.h vegas_big_rule): everything the rule looks at, from the problem, the
// request and the overrides.  `assume_unit`: ask as if the unit were loaded and resident (before it is compiled).
// kVegasBigSamples: the smallest launch that takes it.  2^25 keeps the standing geometry; at 2^26 (16 x 2^22, bench.py --neval-per-gpu
// 67108864, three alternating pairs against the parent) 0.9029 / 0.9036 / 0.9043 -> 0.8986 / 0.8986 / 0.9002 ms per step: -0.0050 ms
// = 3.6 x the parent's spread, every new run below every parent run; at the headline's 1e8 (five pairs) 1.3313 -> 1.3118 ms, 6.5 x
// the spread (profiles/vegas_sixteen_copies.txt).  (Never below the cursor's own 2^25: the unit runs by cursor only.)
// kVegasBigAdds: the fewest histogram adds per sample.  The lightest layout measured is the 8-D Gaussian at 1e8 (8 adds per sample;
// override off | natural, three alternating pairs): 0.7224 / 0.7225 / 0.7230 -> 0.7150 / 0.7157 / 0.7160 ms per step -- it wins there
// too, so the floor is no measured loss but the edge of what was measured; with fewer adds the conflicts the unit removes weigh less.
const int64_t kVegasBigSamples = (int64_t)1 << 26;
const int kVegasBigAdds = 8;
VegasBigIn plan_big_in(const mci_problem *p, const LaunchRequest &rq, const Overrides &ov, bool assume_unit) {
    VegasBigIn in{};
    in.vegas = rq.solver == MCI_VEGAS;
    in.mf1 = rq.measurefreq == 1;
    in.pipe_unit = !p->in_self_check && vegas_pipe_unit(p) && !(ov.vegas_cursor.on && ov.vegas_cursor.v == 0);
    in.forced_grid = p->wg_per_block > 0;
    in.deterministic = p->deterministic;
    in.override_big = ov.vegas_big_unit.on ? (ov.vegas_big_unit.v != 0 ? 1 : 0) : -1;
    in.cursor_forced = ov.vegas_cursor.on && ov.vegas_cursor.v == 1;
    in.copy_plan = p->vegas.hcopy_plan;
    in.conservative = p->vegas.conservative;
    in.copies_forced = ov.hist_copies.on;
    in.threads_explicit = p->threads_explicit;
    in.copies = p->shape.hcopy;
    in.threads = solver_threads(p, MCI_VEGAS);
    in.sixteen_fit_lds = sixteen_copies_fit_lds(p);
    in.samples = rq.nblocks * rq.nevalperblock;
    in.threshold = kVegasBigSamples;
    in.adds = vegas_adds_per_sample(p);
    in.adds_floor = kVegasBigAdds;
    in.nblocks = rq.nblocks;
    in.resident = assume_unit ? rq.nblocks : p->vegas_big.resident;
    in.state = assume_unit && p->vegas_big.state == 0 ? 1 : p->vegas_big.state;
    return in;
}

// Does this launch continue the chains of the previous one?  (the next iteration of the same solver over the same blocks;
// decided before the chains are sized -- carried chains start from configurations that are already distributed like
// the chain's target, so they neither need the many-chain burn-in floors nor their length as a safety margin against start-up bias)
// (:mcmc: a chain's state includes the integrand index, whose weight doReweight! moves between iterations -- the stored chains are
// resampled to the moved target first, k_resample_chains below.  Chains carried as they were started over-represented exactly where
// the new factors say "fewer": 2 sigma per run low on the 12-D member of BASELINE configs[4], profiles/r03_chain_carry.txt.)
// (:vegasmc: not out of a launch on the untrained map onto a refined one -- chains of the automatic length have not reached their
// target there, and no resampling turns them into a sample of the new one, profiles/r05_bias.txt A4; while the map stays as it is
// -- adapt = false -- they go on towards the same target)
bool plan_may_carry(const mci_problem *p, const LaunchRequest &rq) {
    return rq.solver != MCI_VEGAS && p->chain_carry != 0 && p->launch.chain_valid && p->launch.chain_solver == rq.solver &&
           p->launch.chain_lo == rq.block_lo && p->launch.chain_hi == rq.block_hi && p->launch.chain_nchain > 1 &&
           (rq.solver != MCI_VEGASMC || p->launch.chain_ntrain >= 1 || p->launch.chain_ntrain == p->ntrain) &&
           ((p->launch.chain_iteration & (kRepeatStride - 1)) + 1 == (rq.iteration & (kRepeatStride - 1)) ||                        // the next iteration
            ((p->launch.chain_iteration & (kRepeatStride - 1)) == (rq.iteration & (kRepeatStride - 1)) && rq.iteration > p->launch.chain_iteration)); // ... or the same one again (mci_integrate, warm-up)
}

// :vegasmc: chains per block, their burn-in
int plan_vegasmc_chains(const mci_problem *p, const LaunchRequest &rq, const Overrides &ov, LaunchPlan &pl) {
    int nslots = 0; // (pool, slot) pairs changeVariable can pick (updates.jl:50,:58)
    for (int v = 0; v < p->npool; ++v) nslots += p->maxdof[v];
    if (pl.nchain <= 0) { // auto: as many chains as keep 2 waves per SIMD busy (kChainFill lanes per GPU, tools/chain_sweep.py),
        // but never shorter than 8 burn-in floors.  Short chains under-sample the sticky high-|f|/q states of
        // singular integrands: measured on 1/(1 - cos x cos y cos z) at 2e9 steps, 381-step chains are 6 sigma low,
        // 763-step chains are within 1.4 sigma (tools/chain_bias_c1.py).
        // Carried chains are stationary from their first step: two floors per iteration let them settle on the refined map.
        const int64_t fl = 64 * (int64_t)nslots > 128 ? 64 * (int64_t)nslots : 128;
        // A launch on a map train! has never refined whose estimate COUNTS (mci_integrate with ignore = 0: adapt = false, main.jl:82)
        // runs chains 8 x as long: on the untrained map chains of 8 floors have not reached their target -- 3.4 sigma per run low on
        // the 12-D member of BASELINE configs[4], 5 on 1/(1 - cos x cos y cos z), with every iteration counted; with 64 floors
        // within errors (profiles/r05_bias.txt A5, A6).  The default call ignores that iteration and keeps the short ones.
        const int64_t fresh = ov.fresh_floors.on ? ov.fresh_floors.v : (p->launch_counted && p->ntrain == 0) ? 64 : 8;
        pl.nchain = rq.nevalperblock / ((pl.may_carry ? 2 : fresh) * fl);
        const int64_t cap = mci_problem::kChainFill / rq.nblocks > 64 ? mci_problem::kChainFill / rq.nblocks : 64;
        if (pl.nchain > cap) pl.nchain = cap;
        if (pl.nchain < 1) pl.nchain = 1;
    }
    if (pl.nchain > rq.nevalperblock) return fail(MCI_ERR_INVALID, "nchain=%lld exceeds the %lld steps of a block", (long long)pl.nchain, (long long)rq.nevalperblock);
    // (carried chains keep the reference's own `ne >= neval/100` only, vegas_mc/montecarlo.jl:213)
    pl.burnin = mci_chain_burnin(rq.nevalperblock / pl.nchain, (pl.may_carry && pl.nchain > 1) ? 1 : pl.nchain, nslots);
    if (ov.fresh_burnin_pct.on && !pl.may_carry && pl.nchain > 1 && rq.auto_chains) { // (experiment: tools/run_batch.sh r05_floors)
        const double b = (double)(rq.nevalperblock / pl.nchain) * (double)ov.fresh_burnin_pct.v / 100.0;
        if (b > pl.burnin) pl.burnin = b;
    }
    pl.units = pl.nchain;
    return MCI_OK;
}

// :mcmc: chains per block (automatic: from the holding times hold_consume has just taken in), their burn-in
int plan_mcmc_chains(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    int nslots = 0;
    for (int v = 0; v < p->npool; ++v) nslots += p->maxdof[v];
    if (pl.nchain <= 0) { // auto: LONG chains.  The walk over (integrand, variables) mixes slowly when |f|/q is heavy-tailed:
        // on the bubble diagram 1e3-step chains are 2.7 % (55 sigma) off at 2e9 steps and need ~1e5 burn-in steps each
        // to lose that bias (tools/bubble_mcmc_bias.py); only chains much longer than the mixing time are safe, which
        // is what the reference's one-chain-per-block gives.  More chains: raise `block` (the reference's own knob) or
        // pass nchain explicitly for integrands known to mix fast (C5: 10 Gsteps/s at nchain = 4096).
        // From the second :mcmc launch of a problem on, the length follows what the previous launch measured: 16 x the
        // longest time any chain's slot (or integrand index) went without changing (mci_mcmc_auto_chains).
        // Carried chains (resampled to the moved target, k_resample_chains) start from stationary configurations AND a stationary
        // integrand index: nothing to burn in.  What their length still has to cover is the longest holding time: a population
        // grows by duplication (a launch of more chains than the one before continues every stored chain several times), and the
        // copies of a chain must have gone their own ways before they are copied again -- 4 x the longest hold instead of the
        // 16 x (+ burn-in) of fresh chains.  profiles/r03_chain_carry.txt: carried chains of two burn-in floors on 1/(1 - cos^3)
        // keep their few ancestors' view of its sticky states for many iterations (-4.8 sigma pooled over 64 seeds); at 2, 4
        // and 16 x the hold the pooled deviations are those of fresh chains.  profiles/r04_mcmc_policy.txt D: 4 x against the 8 x of
        // round 3 on 384-512 seeds (same pulls, same scatter / error; 2 x: the error bars start to fall short).
        // The holds are those of the launch BEFORE this one (hold_consume waits for its sample kernel); a first launch, with nothing
        // measured, runs pilot-length chains, and a launch's chains are at most kMcmcGrow times as long as those that measured the
        // holds (mci_mcmc_auto_chains).
        // (once warm: the larger of the last two launches' holds, and no growth cap -- both were measured by chains that held them)
        const int64_t hold_eff = p->launch.mcmc_warm && p->launch.hold_prev > p->launch.hold_max ? p->launch.hold_prev : p->launch.hold_max;
        pl.nchain = mci_mcmc_auto_chains(rq.nevalperblock, rq.nblocks, nslots, p->ni + 1, p->npool, hold_eff, p->launch.mcmc_warm && p->launch.hold_valid ? 0 : p->launch.hold_len,
                                      pl.may_carry ? 1 : 0);
    }
    if (pl.nchain > rq.nevalperblock) return fail(MCI_ERR_INVALID, "nchain=%lld exceeds the %lld steps of a block", (long long)pl.nchain, (long long)rq.nevalperblock);
    // (carried chains have no start to burn in: floor(steps * thermal_ratio), mcmc/montecarlo.jl:133, is the burn-in of a chain that
    // begins at a random configuration; a chain that continues a stationary one measures from its first step)
    pl.nburn = (pl.may_carry && pl.nchain > 1) ? 0 : mci_mcmc_burnin(rq.nevalperblock / pl.nchain, pl.nchain, nslots, p->ni + 1, p->npool, rq.thermal_ratio);
    pl.units = pl.nchain;
    return MCI_OK;
}

// Several lanes per chain (mci_spec.h): a launch whose chains leave most of the chip idle gives every chain a group of G lanes that
// step it speculatively -- the same chain, G <= 64 proposals evaluated per trip.  Automatic: the largest G that keeps the launch
// within one wave per SIMD (kSpecFill lanes).  Host integrands keep the lock-step launches; the deterministic mode one lane per chain.
void plan_spec_lanes(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    const auto &s = p->shape;
    if (rq.solver != MCI_VEGAS && !s.host_integrand && !p->deterministic && p->spec_lanes != 1) {
        if (p->spec_lanes > 1) pl.G = p->spec_lanes;
        else {
            pl.G = 64;
            while (pl.G > 1 && rq.nblocks * pl.nchain * pl.G > mci_problem::kSpecFill) pl.G >>= 1;
            // (groups of 2 and 4 lanes lose: a trip costs more than a lane-per-chain step and advances barely more -- BASELINE configs[4],
            // 24400 pilot chains: 32.3 ms with 2 lanes per chain against 21.8; the bubble diagram 3.5 | 2.15 | 1.1 us per step at 4 | 16 | 64
            // lanes against 5.6 with one, profiles/r05_spec.txt)
            if (pl.G < 8) pl.G = 1;
        }
    }
}

// the grid of the fixed partition: workgroups per block
void plan_grid(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    const auto &s = p->shape;
    pl.wpb = p->wg_per_block;
    if (pl.G > 1) {
        if (pl.wpb <= 0) pl.wpb = (int)((2048 + rq.nblocks - 1) / rq.nblocks);
        const int64_t maxw = (pl.units + pl.T_launch - 1) / pl.T_launch;
        if (pl.wpb > maxw) pl.wpb = (int)maxw;
        if (pl.wpb < 1) pl.wpb = 1;
    } else
    if (pl.wpb <= 0) { // 256 CUs x 8..16 workgroups in the grid, never a workgroup without work
        // The fixed partition's grid, measured on C2 (tools/wg_sweep.py, profiles/vegas_cursor.txt; 512-thread workgroups of the
        // histogram-copy plan, sample kernel per launch): 512 / 1024 / 2048 / 4096 workgroups 1.395 / 1.366 / 1.357 / 1.360 ms.  One
        // round of resident workgroups leaves the CUs that finish early idle (equal shares, unequal clocks); every further round halves
        // that and costs 3-4 us of prologues and epilogues that the two workgroups of a CU run in phase, plus its partial rows for
        // k_hist_stage1.  Four rounds (2048 of 512 threads, 4096 of 256) are the best a fixed partition does -- while a workgroup's
        // tables are cheap to stage: C3 with 66 KB per workgroup lost 15 % at 4096.  Big launches of the pipelined loop leave this
        // rule for the cursor below, which has neither cost.
        const int64_t big = pl.T >= 1024 ? 1024 : pl.T >= 512 ? 2048 : 4096;
        int64_t target = (pl.units * rq.nblocks >= (int64_t)1 << 25 && p->lds_bytes <= 32 * 1024) ? big : 2048;
        // :vegas launches of up to a few million samples: a workgroup's prologue and epilogue (tables staged, histogram zeroed and
        // flushed) cost what ~50 samples per thread cost, so the grid shrinks to one workgroup per CU (tools/latency.py, us per
        // iteration at neval = 1e6: 2048 workgroups 39.9, 512: 27.7, 256: 26.9; C2 at 1e6: 64.8 -> 43.9).  Longer launches keep the
        // full grid: a grid between 256 and 512 workgroups leaves half of the CUs' second slot empty (C2 at 1e7: 320 workgroups
        // 271.7 us, 2048: 210.1)
        if (rq.solver == MCI_VEGAS && pl.units * rq.nblocks < ((int64_t)1 << 22) && target > 256) target = 256;
        // ... and light launches (samples x draws below 2^19: a 2-D integrand at neval = 1e5) to a quarter of the CUs: their prologues and
        // epilogues weigh more than a few more samples per lane (tools/latency.py, x^2 + y^2 at 1e5: 22.0 -> 18.6 us per iteration; the
        // 16-D Gaussian at 1e5 keeps the full 256: 23.4 against 25.9 us)
        if (rq.solver == MCI_VEGAS && pl.units * rq.nblocks * s.ndraw < ((int64_t)1 << 19) && target > 64) target = 64;
        pl.wpb = (int)((target + rq.nblocks - 1) / rq.nblocks);
        const int64_t maxw = (pl.units + pl.T - 1) / pl.T;
        if (pl.wpb > maxw) pl.wpb = (int)maxw;
        if (pl.wpb < 1) pl.wpb = 1;
    }
}

// Big :vegas launches of the pipelined one-tile loop: ranges handed out by cursor (mci_device.h, the cursor section) to a grid that
// is resident at once.  Every workgroup stages its tables and zeroes its histogram copies once and writes one partial row, so the
// rounds of prologues and epilogues of the fixed partition, its idle CUs behind the last round and three quarters of its partial
// rows are gone (profiles/vegas_cursor.txt: C2 1.332 -> 1.309 ms per iteration, k_hist_stage1 7.4 -> 4.2 us).  The grid comes from the runtime's occupancy query -- the headline layout: two
// 512-thread workgroups on each of 256 CUs, 32 per block -- and nobody waits for another workgroup, so a grid that is NOT resident
// at once (a forced wg_per_block) is as correct.  Not for: a forced grid, the deterministic mode (the partition would follow the
// hardware), a self-check's launches, anything below 2^25 samples (its few rounds cost less than the pulls' tail).
// 0: the fixed partition | 1: the cursor, forced (override vegas_cursor = 1) | 2: the cursor if the grid the runtime reports as
// resident is large enough (cursor_resident, then plan_cursor_grid)
int plan_cursor_candidate(const mci_problem *p, const LaunchRequest &rq, const Overrides &ov, const LaunchPlan &pl) {
    if (!(rq.solver == MCI_VEGAS && pl.G == 1 && !p->in_self_check && vegas_pipe_unit(p) && !(ov.vegas_cursor.on && ov.vegas_cursor.v == 0))) return 0;
    if (ov.vegas_cursor.on && ov.vegas_cursor.v == 1) return 1;
    return p->wg_per_block <= 0 && pl.units * rq.nblocks >= ((int64_t)1 << 25) ? 2 : 0;
}
void plan_cursor_grid(const LaunchRequest &rq, int resident, LaunchPlan &pl) {
    // (a resident grid of at most kAtomicRows rows would flush its histograms by atomics, the plan of launch-bound
    // iterations: such layouts -- one workgroup per CU -- keep the fixed partition and its partial rows; the big unit's launches are
    // one 1024-thread workgroup per CU by design and keep their partial rows, plan_tiles)
    if (resident >= rq.nblocks && ((resident / rq.nblocks) * rq.nblocks > kAtomicRows || rq.kern == mci_problem::kVegasBig)) {
        pl.cursor = true;
        pl.wpb = (int)(resident / rq.nblocks);
        const int64_t maxw = (pl.units + pl.T - 1) / pl.T;
        if (pl.wpb > maxw) pl.wpb = (int)maxw;
    }
}

// bytes a many-grid :vegas launch parks per sample: the weights, the packed bins of the replayed draws
int64_t parked_bytes_per_sample(const mci_problem *p) { return (int64_t)p->shape.ni * 8 + (int64_t)(p->tdraw_words > 0 ? p->tdraw_words : 1) * 4; }

// histogram tiles, partial rows, the flush of the histograms, the chunks of a many-grid launch
void plan_tiles(const mci_problem *p, const LaunchRequest &rq, const Overrides &ov, LaunchPlan &pl) {
    const auto &s = p->shape;
    pl.hist_lds = (s.table_mode == 0 || s.table_mode == 3);
    // Few partial rows (launch-bound :vegas iterations): no partial histograms, no first merge launch -- the workgroups add their
    // non-zero bins to the merged histogram directly (global f64 atomics; the order of those adds follows the hardware, so the
    // deterministic mode keeps the fixed-order merge).  tools/latency.py, us per iteration: x^2 + y^2 at neval = 1e4 22.7 -> 17-19,
    // 1e5 23.8 -> 18.6, 1e6 26.5 -> 24.4; 16-D Gaussian at 1e5 27.3 -> 23.4, 1e6 41.8 -> 37.2.
    // NTILE > 1 histogram tiles.  vegas: ONE sample pass (tile 0) parks weights + bins per sample, mci_vegas_tiles
    // replays them for the other tiles.  Chain solvers: NTILE workgroups per row, each recomputing the chain and
    // keeping one tile.
    pl.split = rq.solver == MCI_VEGAS && s.ntile > 1;
    if (!pl.split && pl.wpb * s.ntile > 4096 / rq.nblocks && s.ntile > 1) pl.wpb = (int)(4096 / rq.nblocks / s.ntile) > 0 ? (int)(4096 / rq.nblocks / s.ntile) : 1;
    pl.nrows = rq.nblocks * pl.wpb;   // partial rows: one per (block, slice)
    // (a cursor launch of the big unit -- 256 rows on the headline -- is no launch-bound iteration: partial rows and k_hist_stage1)
    pl.atomic_flush = rq.solver == MCI_VEGAS && pl.hist_lds && s.ntile == 1 && atomic_rows_ok(p) && pl.nrows <= kAtomicRows && !s.host_integrand &&
                      !(pl.cursor && rq.kern == mci_problem::kVegasBig);
    pl.nwg = pl.split ? pl.nrows : pl.nrows * s.ntile;
    // (three buffers from 64 rows on: x^2 + y^2 at neval = 1e6, 256 rows: see tools/latency.py)
    pl.ghist_buffers = pl.atomic_flush ? (pl.nrows > 64 ? 3 : 1) : 0;
    // Many-grid launches park (weights, bins) of every sample for the replay.  The stream is bounded whatever neval is -- the reference's
    // loop allocates nothing per sample (vegas/montecarlo.jl:117-187) -- by running the launch in chunks of a block's samples: sample pass
    // -> replay per chunk, same Philox indices, the partial rows of a later chunk added to those before it (BatchArgs::chunk_lo).  A chunk
    // is at most 2^27 samples over all blocks and at most 7.5 GB of parked stream (C4, 48 B per sample: all of neval = 1e8 in one
    // chunk as before, neval = 1e10 in 75); host closures read the whole launch's stream and keep the one chunk (they are refused above 8 GiB).
    pl.chunk_len = rq.nevalperblock;
    pl.nchunks = 1;
    if (pl.split && !s.host_integrand && !s.host_measure) {
        const int64_t bytes = parked_bytes_per_sample(p);
        int64_t cap = (int64_t)1 << 27;
        if (cap * bytes > (int64_t)7500000000) cap = (int64_t)7500000000 / bytes;
        if (ov.split_chunk.on && ov.split_chunk.v > 0) cap = ov.split_chunk.v;
        int64_t per = (cap / rq.nblocks) & ~(int64_t)3; // (a multiple of four: the replay reads four consecutive samples per lane as 16-byte loads)
        if (per < 4) per = 4;
        if (per < pl.chunk_len) {
            pl.chunk_len = per;
            pl.nchunks = (rq.nevalperblock + pl.chunk_len - 1) / pl.chunk_len;
        }
    }
}

// Split-all :vegas: the replay partitions a block's parked samples on its own.  Every replay workgroup zeroes and flushes a whole LDS
// tile (C4: 128 KB) and every row it writes is read again by the merge, so it runs ~2 workgroups per CU and tile pair instead of one
// per sample-pass row (C4: 512 instead of 2048 workgroups, 67 instead of 262 MB of partial histograms written and read back:
// k_hist_stage1 100 -> 12.6 us, profiles/r04_c4_kernel_stats.txt).  The partition only decides which workgroup adds a sample to the
// histogram: sums differ by reassociation.
void plan_replay(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    const auto &s = p->shape;
    pl.hist_rows = pl.nrows;
    if (pl.split && s.split_all) {
        int64_t rwpb = 512 / (rq.nblocks * s.ntile);
        if (rwpb > pl.wpb) rwpb = pl.wpb;
        if (rwpb < 1) rwpb = 1;
        pl.tiles_wpb = (int)rwpb;
        pl.hist_rows = rq.nblocks * rwpb;
    }
}

// host measure: records per block, rows of relative weights per record, measured-step window of a chain (BatchArgs::hm_*)
void plan_host_measure(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    const auto &s = p->shape;
    if (!s.host_measure) return;
    const int nw = s.ni * s.ncomp;
    if (rq.solver == MCI_VEGAS) {
        pl.hm_n = rq.nevalperblock;
        pl.hm_rows = nw;
    } else {
        // a chain measures at steps j * measurefreq: :vegasmc from `burnin` on (vegas_mc/montecarlo.jl:213), :mcmc from nburn on
        // (mcmc/montecarlo.jl:143) -- the same comparisons the kernels make
        const int64_t mfq = rq.measurefreq > 0 ? rq.measurefreq : 1;
        const int64_t last = rq.solver == MCI_VEGASMC ? rq.nevalperblock / pl.nchain : rq.nevalperblock / pl.nchain + pl.nburn;
        pl.hm_first = 1;
        if (rq.solver == MCI_VEGASMC) {
            pl.hm_first = (int64_t)(pl.burnin / (double)mfq);
            if (pl.hm_first < 1) pl.hm_first = 1;
            while (pl.hm_first > 1 && (double)((pl.hm_first - 1) * mfq) >= pl.burnin) --pl.hm_first;
            while ((double)(pl.hm_first * mfq) < pl.burnin) ++pl.hm_first;
        } else if (pl.nburn > 0) {
            pl.hm_first = (pl.nburn + mfq - 1) / mfq;
            if (pl.hm_first < 1) pl.hm_first = 1;
        }
        pl.hm_count = last / mfq - pl.hm_first + 1;
        if (pl.hm_count < 0) pl.hm_count = 0;
        pl.hm_n = pl.nchain * pl.hm_count;
        pl.hm_rows = rq.solver == MCI_MCMC ? s.ncomp : nw;
    }
}

// HIP events around the sample launch (mci_kernel_times_ms): each record is a barrier packet with a signal, ~5.5 us of idle
// queue -- a third of a launch-bound iteration (neval = 1e4: 36 -> 25 us), nothing next to a launch of millions of samples.
// mci_set_kernel_timing: -1 (default) = launches of >= 2^20 samples, 0 = never, 1 = always
void plan_timing(const mci_problem *p, const LaunchRequest &rq, LaunchPlan &pl) {
    pl.time_this_launch = p->kernel_timing > 0 || (p->kernel_timing < 0 && rq.nblocks * rq.nevalperblock >= ((int64_t)1 << 20));
}

} // namespace
