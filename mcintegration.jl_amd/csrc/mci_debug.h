/* mci_debug.h -- development and test hooks of libmci_hip.so.  NOT part of the drop-in boundary (include/mci.h): nothing here stands
 * in for reference code, tests and tools/ may use it, a binding must not. */
#ifndef MCI_DEBUG_H
#define MCI_DEBUG_H
#include "../../include/mci.h"
#ifdef __cplusplus
extern "C" {
#endif
/* tools/persist_trace.py: the persistent kernel's counter words and, in builds with -DMCI_PERSIST_TRACE, the wall-clock stamps of
 * three of its workgroups over the first eight turns of the last launch */
int mci_debug_persist_words(mci_problem *prob, unsigned long long *out, int32_t n);
/* out[0] = serial walks of train! (mci_set_train_walk mode 1) this problem has run as slots with given decisions, out[1] = walks in
 * the general form (mode 2, a decision that did not hold, grids too long for the slots' LDS).  Synchronises the stream. */
int mci_debug_walk_counts(mci_problem *prob, int64_t *out);
/* test hook: the serial walk of train! with one decision deliberately wrong, so that its check and the fall-back to the general form
 * run (same results as mci_set_train_walk(prob, 1)); on = 0 takes it back */
int mci_debug_plant_wrong_decision(mci_problem *prob, int32_t on);
/* test hook: ticks of the 100 MHz clock a grid-wide wait of the persistent :vegas launch may take before it gives up (default 2 s =
 * 200000000); a tiny value forces the stall so that the fall-back to the launch chain can be tested */
int mci_debug_persist_spin_ticks(mci_problem *prob, unsigned long long ticks);
/* Layout decisions of mci_problem_create that tests and A/B tools force; process-wide, consulted by the NEXT mci_problem_create; on = 0
 * takes an override back.  Keys:
 *   table_mode      0 .. 3   placement of grids / histograms
 *   hist_tile_bins  n        bins of an LDS histogram tile (forces several tiles)
 *   no_split_all    1        tiled :vegas: tile 0 stays in the sample pass, only the other tiles are replayed
 *   l1_phase        0 | 1    dimension-major gather phase of the many-grid sample pass
 *   hist_copies     n        interleaved histogram copies of the :vegas sample kernel (1 = none)
 *   train_walk      0 | 1 | 2  = mci_set_train_walk on every new problem
 *   fresh_floors    n        (consulted per launch) length of automatic :vegasmc chains that start afresh, in burn-in floors (8)
 *   fresh_burnin_pct n       (per launch) ... and the least part of such a chain that is not measured, in per cent (profiles/r05_bias.txt A5)
 *   split_chunk      n       (per launch) samples per chunk, over all blocks, of a many-grid :vegas launch (mci_debug_split_chunks)
 *   spec_self_check  0 | 1   (per launch) the self-check of a several-lanes-per-chain code object (mci_chain_speculation_status): never |
 *                            also when the kernel cache holds the marker of an earlier pass (the guard test of tests/test_hip_spec.py)
 *   vegas_self_check 0 | 1   (per launch) the self-check of a :vegas code object (mci_vegas_check_status): never | also when the kernel
 *                            cache holds the marker of an earlier pass
 *   vegas_cursor     0 | 1   (per launch) cursor hand-out of :vegas launches through the pipelined one-tile loop (mci_device.h, the cursor
 *                            section): never | every such launch, whatever its size and with a forced wg_per_block too
 *   cursor_log2_big  n       (per launch) log2 of the units in a big range, 1 .. 16 (4)
 *   cursor_ones      n       (per launch) single-unit ranges per wave at the end of a block, 1 .. 4096 (4)
 *   vegas_big_unit   0 | 1   (per launch) the big :vegas unit (sixteen histogram copies, 1024 threads; mci_host_vegas_plan.h): never | at
 *                            any size and with a forced wg_per_block too, together with vegas_cursor = 1
 * (The library reads two environment variables and no others: MCI_KERNEL_CACHE -- the directory code objects are cached in -- and
 * MCI_JIT_FLAGS -- extra hiprtc options; INTEGRATION.md.) */
int mci_debug_override(const char *key, int64_t value, int32_t on);
/* the last many-grid (several histogram tiles) :vegas launch of the problem: how many chunks of the blocks' samples it ran as (sample pass
 * -> replay per chunk; override key split_chunk = samples per chunk over all blocks, default min(2^27, 7.5 GB of stream)) and the bytes of
 * parked (weights, bins) stream it held at a time */
int mci_debug_split_chunks(const mci_problem *prob, int64_t *chunks, int64_t *bytes);
/* test hook: the NEXT stratified :vegas iteration of the problem (mci_set_stratification) also leaves, for each of its n samples (n must be
 * that iteration's N), the draws x[n][ndraw], the uniforms y[n][ndraw] after the move into the sample's hypercube, the hypercube h[n],
 * the Jacobian jac[n] (without r_h) and the weights w[n][ni * ncomp] in these host buffers; the run synchronises.  n = 0 takes it back. */
int mci_debug_strat_dump(mci_problem *prob, int64_t n, double *x, double *y, int64_t *h, double *jac, double *w);
/* test hook: d[n] = the damped weights d_h = (sum_k s^2_{h,k})^(beta/2) the last finished stratified iteration wrote (what the next
 * allocation is made from); n must be the plan's hypercube count, call it after mci_iteration_finish.  Synchronises the stream. */
int mci_debug_strat_d(mci_problem *prob, double *d, int64_t n);
/* test hook: the NEXT first allocation of a stratified run (a call's first iteration, a new plan or N) also leaves the d_h it is made
 * from -- the carried values as they are, remapped or raised to the new beta (mci_set_stratification_carry); ones for a uniform start --
 * in d[n]; n must be that plan's hypercube count.  The run synchronises.  n = 0 takes it back. */
int mci_debug_strat_start_d(mci_problem *prob, double *d, int64_t n);
/* used: did the problem's last sample launch hand its ranges out by cursor (else: the fixed partition)?  base: what its blocks' cursor
 * words hold once every launch queued so far is through (tickets + waves per launch; tests/test_hip_vegas_cursor.py) */
int mci_debug_vegas_cursor(const mci_problem *prob, int32_t *used, uint64_t *base);
/* what mci_jit.h puts into the kernel-cache key for "which compiler made this code object" (hiprtc version, the files of libhiprtc and
 * libamd_comgr, the target): set != NULL overrides it for this process ("" takes the override back); out: the identity in force */
int mci_debug_compiler_id(const char *set, char *out, int32_t n);
/* the constants of the automatic :mcmc chain length (DESIGN.md "Chains"), process-wide, for A/B campaigns (tools/mcmc_policy.py): measured
 * steps of a first launch (4096) | how much longer than the chains that measured the holds a launch's chains may be (2) | length of a
 * carried chain in longest holds (4) | its minimum in half burn-in floors (2); <= 0 keeps a value */
int mci_debug_mcmc_policy(int64_t pilot_steps, int64_t grow, int64_t carry_holds, int64_t carry_half_floors);
/* test hook: the library's static :vegas kernel (k_check_vegas, what a new :vegas code object is held against) on its own -- one
 * iteration of blocks [block_lo, block_lo + nblocks) x nevalperblock samples (at most 1024 in all) into packed[packed size], in the
 * layout of mci_get_packed.  x[n][ndraw], jac[n], w[n][ni * ncomp]: the samples as mci_sample_dump lays them out, block after block
 * (all NULL: this problem's own mci_sample_dump); bad[0] / bad[1]: samples whose x (bit for bit) / jac (1e-13) the kernel does not
 * reproduce.  Problems the check covers only (one histogram tile, device integrand and measure). */
int mci_debug_vegas_check(mci_problem *prob, int32_t iteration, uint64_t seed, int64_t nevalperblock, int64_t block_lo, int64_t nblocks,
                          int64_t measurefreq, const double *x, const double *jac, const double *w, double *packed, int64_t *bad);
/* launches made on behalf of the :vegas self-check of this problem so far (sample kernel under test, sample dump, static kernel) */
int mci_debug_vegas_check_launches(const mci_problem *prob, int64_t *launches);
/* the run-time layout table the static :vegas kernel is given (no device needed).  head[8]: ndraw, ni, ncomp, nobs, ncols, nbin, covered
 * (0 | 1), default or binning measure (0: a user measure); draws[ndraw][6]: kind, table offset, distribution offset, bins, histogram
 * offset, takes histogram adds; scales[ndraw]: the Jacobian scale; own[ni]: own-draw masks; obs[ni][3]: observable offset, bins,
 * binning draw.  NULL: not wanted. */
int mci_debug_vegas_check_layout(const mci_problem *prob, int32_t *head, int32_t *draws, double *scales, uint64_t *own, int32_t *obs);
/* test hook: workgroups of this problem's next sweeps (mci_integrate_sweep; at most one per point is launched), so that a test can
 * make one workgroup run several points; 0 = the default, two per CU */
int mci_debug_sweep_workgroups(mci_problem *prob, int32_t g);
/* A/B hook (tools/sweep_bench.py): threads per workgroup of this problem's next sweeps, 256 | 512 | 1024; 0 = the default */
int mci_debug_sweep_threads(mci_problem *prob, int32_t threads);
/* workgroups and threads per workgroup of the problem's last sweep launch */
int mci_debug_sweep_last_launch(const mci_problem *prob, int32_t *workgroups, int32_t *threads);
/* (tools/sweep_bench.py) dynamic LDS bytes per workgroup of this problem's sweeps under its present mci_set_sweep_leaves mode */
int mci_debug_sweep_lds_bytes(const mci_problem *prob, int64_t *bytes);
/* (tests, tools/sweep_bench.py) what mci_integrate_sweep_strat lays a launch of these arguments out as, under the problem's present
 * mci_set_sweep_strat_leaves mode: samples per chunk, dynamic LDS bytes per workgroup, where the point's map lies in it (doubles), and the
 * blocks the ordinary stratified call merges its rows as.  No device needed; refused as mci_sweep_strat_supported refuses.  NULL: not wanted. */
int mci_debug_sweep_strat_geometry(const mci_problem *prob, const mci_integrate_args *args, int64_t *chunk, int64_t *lds_bytes, int32_t *map_off,
                                   int32_t *mblocks);
/* test hook: the carried chains' resampler (k_resample_chains, mci_static_kernels.h) on its own -- nblocks workgroups of 256 threads over
 * the given stored chains, launched as an ordinary carried launch launches it: curr_old[nblocks][n_old] the integrand every stored chain
 * ended on, rw_now[nd] / rw_used[nd] the reweight factors now and those the chains ran under, w_chain[nblocks][n_old] a weight per stored
 * chain instead (NULL: the :mcmc rule), src[nblocks][n_new] the picks, W[nblocks][n_old] the running weights (NULL: not wanted).  The
 * problem gives its device and stream only: its own stored chains and the record of its last launch stay as they are.  Synchronises.
 * Both outputs are filled with 0xFF bytes before the launch: what the kernel leaves unwritten comes back as -1 | NaN.
 * Refused: nblocks, n_old or n_new < 1, nd outside 1 .. 64, blocks of 2^31 chains or more. */
int mci_debug_resample(mci_problem *prob, int64_t nblocks, int64_t n_old, int64_t n_new, int32_t nd, const int32_t *curr_old,
                       const double *rw_now, const double *rw_used, const double *w_chain, int32_t *src, double *W);
/* test hook: the merge kernels (mci_static_kernels.h k_add_host_obs, k_hist_stage1, k_finalize | k_finish; the device functions
 * merge_stats, merge_hist_bin, merge_pa of mci_train.h) on their own over partial rows the caller made up, launched with the grids, thread
 * counts and dynamic LDS the product launches them with (the same helpers give both).  The problem gives its device, its stream and its
 * shape -- nobs, ni, ncols, nbin, npa, nstat and the leaf table, mci_debug_merge_shape -- and nothing else: every buffer the kernels read
 * or write is the hook's own, the status word included; the problem's partial rows, `packed`, pending merge and status stay as they are.
 * Every output is filled with 0xFF bytes before the launches: what the kernels leave unwritten comes back as NaN (status: its own word
 * starts at 0).  Synchronises.
 * Refused (MCI_ERR_INVALID): nblocks, wg_per_block or nrows < 1, nrows < nblocks * wg_per_block, neither or both of hist_rows and
 * use_ghist, use_ghist > 64, a missing part_cols | part_hist | ghist | packed, products that do not fit an int, path other than 0 | 1;
 * an offline context (MCI_ERR_NO_DEVICE). */
typedef struct mci_debug_merge_io {
    int32_t nblocks, wg_per_block; /* statistical blocks and partial rows per block: merge_stats reads rows [0, nblocks * wg_per_block) */
    int32_t nrows;                 /* rows of part_cols and part_pa (merge_pa sums all of them) */
    int32_t hist_rows;             /* rows of part_hist (k_hist_stage1 runs), or 0 */
    int32_t use_ghist;             /* or: the number of global histogram buffers in `ghist` (no first stage) */
    int32_t hist_no_offset;        /* MergeArgs::hist_no_offset */
    int32_t path;                  /* 0: k_hist_stage1 -> k_finalize | 1: k_hist_stage1 -> k_finish (no reweighting, no log row; merge only unless do_train, below) */
    const double *part_cols;       /* [nrows][ncols] */
    const double *part_hist;       /* [hist_rows][nbin] */
    const double *ghist;           /* [use_ghist][nbin] */
    const double *part_pa;         /* [nrows][2 npa] or NULL (a :vegas pass) */
    const unsigned long long *hold; /* [64] or NULL */
    const double *obs;             /* [nblocks][nobs] or NULL: k_add_host_obs runs first, as behind a host measure */
    /* out; NULL: not wanted (block_means = NULL: the kernels are not asked for them either) */
    double *packed;                /* [mci_reduce_size] */
    double *stage1;                /* [32][nbin] */
    double *scratch;               /* [nblocks][ncols] */
    double *block_means;           /* [nblocks][nobs] */
    int32_t *status;               /* the hook's own ST_* word */
    double *part_cols_out;         /* [nrows][ncols] as the kernels left them */
    double *ghist_out;             /* [use_ghist + 1][nbin]: the buffers as left behind, then a guard row the hook filled with NaN */
    /* "and train" (path 1 only): k_finish goes on to refine every adapting leaf from the merged histogram in its LDS, as launch_train
     * has it do behind a pending merge -- on tables of the HOOK's own, uploaded from here and read back to here, leaf after leaf in the
     * problem's leaf order; the problem's grids and distributions stay as they are.  Refused: do_train on path 0, a walk outside
     * 0 .. 3, a missing table. */
    int32_t do_train;              /* 0: merge only (everything below is ignored) */
    int32_t train_walk;            /* TrainArgs::serial_walk: 0 prefix scan | 1 serial | 2 serial, general form | 3 serial, one decision planted wrong */
    const double *grids;           /* the Continuous leaves' old grids, npts doubles each (NULL only if there is none) */
    const double *dists;           /* the Discrete leaves' distributions, K doubles each */
    const double *accs;            /* ... and accumulations, K + 1 doubles each */
    double *grids_out, *dists_out, *accs_out; /* the same tables as k_finish left them */
    int64_t *walk_counts;          /* [2] or NULL: serial walks run as slots | in the general form (mci_debug_walk_counts, of the hook's own word) */
} mci_debug_merge_io;
int mci_debug_merge(mci_problem *prob, const mci_debug_merge_io *io);
/* test hooks: the three static kernels of stratified :vegas (mci_static_kernels.h k_strat_alloc, k_strat_reduce, k_strat_remap) on their
 * own over inputs the caller made up, launched by the helpers the product launches them with (mci_host_strat.h strat_alloc_launches,
 * strat_reduce_launch, strat_remap_launch: phases, grids and thread counts are written down once).  The problem gives its device and its
 * stream only and need not be stratified: every buffer is the hook's own, the problem's plan, offsets, d_h and carried allocation stay as
 * they are.  Every output is filled with 0xFF bytes before the launch: what a kernel leaves unwritten comes back as -1 | NaN.  Each hook
 * synchronises.  An offline context: MCI_ERR_NO_DEVICE.
 * mci_debug_strat_alloc: d[ncube] -> off_out[ncube + 1] and the scratch tsum_out[2 ntile + 2] = tile sums | tile bases | total | uniform
 * flag, ntile = min(ceil(ncube / 256), 1024); uniform = 1: d_h = 1 whatever d holds.  Refused (MCI_ERR_INVALID): ncube outside
 * 1 .. 2^31 - 1, nsamp < 2 ncube or > 2^52, uniform other than 0 | 1. */
int mci_debug_strat_alloc(mci_problem *prob, const double *d, int64_t ncube, int64_t nsamp, int32_t uniform, int64_t *off_out, double *tsum_out);
/* mci_debug_strat_reduce: the chunks' partial rows and boundary records as the sample kernel leaves them (mci_strat.h StratArgs) -> out,
 * log_row and the d_h of the cut hypercubes.  Refused: ncube outside 1 .. 2^31 - 1, nchunk outside 1 .. 2^24, nw outside 1 .. 8, a beta
 * that is negative or not finite, a rec_h entry outside -1 .. ncube - 1 (the kernel indexes off and dnext with it). */
typedef struct mci_debug_strat_reduce_io {
    int64_t ncube, nchunk;
    int32_t nw;            /* weight columns, 1 .. 8 */
    double beta;
    const int64_t *off;    /* [ncube + 1] */
    const double *part;    /* [nchunk][2 nw] */
    const int64_t *rec_h;  /* [nchunk][2], -1 = none */
    const double *rec_s;   /* [nchunk][2][2 nw] */
    double *dnext;         /* [ncube] in and out: the caller's fill goes up, what the kernel left comes back */
    double *out;           /* [2 nw] out: mean | var */
    double *log_row;       /* [2 nw] out, or NULL: the kernel is given no log row */
} mci_debug_strat_reduce_io;
int mci_debug_strat_reduce(mci_problem *prob, const mci_debug_strat_reduce_io *io);
/* mci_debug_strat_remap: d_old[prod n_old] on the plan n_old[ndim] -> d_new_out[prod n_new] on the plan n_new[ndim], raised to e.
 * Refused: ndim outside 1 .. 32, a cell count < 1, more than 2^31 - 1 hypercubes on either side, an e that is not finite. */
int mci_debug_strat_remap(mci_problem *prob, int32_t ndim, const int32_t *n_old, const int32_t *n_new, double e, const double *d_old, double *d_new_out);
/* shape[8] = nobs, ni, ncols, nbin, npa, nstat, leaves, bins of the largest leaf; leaves[nleaf][2] (or NULL) = offset into the histogram
 * section, bins.  No device needed. */
int mci_debug_merge_shape(const mci_problem *prob, int32_t *shape, int32_t *leaves);
/* stored chains per block up to which a carried sweep point's resampler (mci_sweep_chains.h) keeps the running weights in LDS: the
 * map_off - kResampleThreads the carried sweep units are handed (beyond: its bisections read them in global memory); no device needed */
int mci_debug_sweep_resample_lds(const mci_problem *prob, int64_t *lds_w);
#ifdef __cplusplus
}
#endif
#endif
