// mci_sweep_chains.h -- batched parameter sweeps under the chain solvers (mci_integrate_sweep_chains: :vegasmc points; mci_integrate_sweep_mcmc:
// :mcmc points): vegas_sweep_leaves of mci_sweep_leaves.h with a chain solver's sample loop (mci_device.h vegasmc_chains,
// vegas_mc/montecarlo.jl:112-241; mcmc_chains, mcmc/montecarlo.jl:72-187 and mcmc/updates.jl) in place of vegas_batch, and the chain
// solvers' per-iteration state: a point's reweight factors (doReweight!, main.jl:183, :322-346) and its propose | accept tables.
// ONE body, chain_sweep<Cfg, MCMC>, two instantiations: vegasmc_sweep and mcmc_sweep differ in the one line that calls the chain loop.
// Compiled by hiprtc next to mci_device.h, mci_train.h and mci_sweep_common.h into a translation unit of its own per solver (mci_jit.h
// kUnitSweepChains, generated for MCI_VEGASMC; kUnitSweepMcmc, generated for MCI_MCMC): every other code object stays what it was.
// Free of host / std headers.
//
//     workgroup g   for p = g, g + G, ...:   map of point p -> LDS (the SweepBlock of mci_sweep_common.h);
//                   for every iteration:  for every statistical block, one after another: its `nchain` chains, one lane per chain,
//                   lanes striding over the chains (vegasmc_chains | mcmc_chains with wg_per_block = 1: row = block) -> merge the block rows
//                   (merge_stats) and the blocks' propose | accept rows (merge_pa) -> statistics head -> this point's log row ->
//                   doReweight! on this point's factors (iteration_bookkeeping, thread 0) -> leaf by leaf the merged histogram slice
//                   and train! on the leaf's part of the LDS map;   at the end the map -> maps_out[p]
//
// Streams are keyed by (seed, iteration, block, chain, step) as in the ordinary launch, and every chain starts afresh in every iteration
// (carry_x = store_x = NULL: the semantics of mci_set_chain_carry(prob, 0)), so a point's chains are the chains mci_iteration_run runs for
// the same nchain with one lane per chain.  :mcmc: `nburn` is the host's (mci_mcmc_burnin, BatchArgs::nburn, the same for every point),
// the start of a chain is tried at most 10000 times (mcmc/montecarlo.jl:118-124; a point whose integrand stays zero reports ST_MCMC_INIT
// in its own status word and goes on), and every loop bound of the chain loop is a kernel argument or a compile-time constant.
//
// The synchronisation is mci_sweep_common.h's.  What this unit adds to a point's traffic through global memory is written and read by
// the point's own workgroup, with a sweep_round_trip() between the two sides:
//   * the blocks' propose | accept rows (flush_workgroup, plain stores by all threads) -> merge_pa, behind the round trip that follows
//     the last block;
//   * the reweight factors: thread 0 writes them in iteration_bookkeeping, every lane reads them at the start of the next vegasmc_chains |
//     mcmc_chains call -- the round trip of the first leaf's histogram slice stands in between (NLEAF >= 1), and thread 0's own wait covers
//     its stores.  The same under either solver.
// What :mcmc adds, its holding-time histogram (SweepChainArgs::holds, 64 words per point), is write-only here: the chain loop's vector
// atomics add to the point's words, nothing in the kernel reads them (MergeArgs::hold stays NULL: merge_pa leaves zeros in the packed row's
// last 64 doubles) -- reading them would take loads that bypass the CU's L1 in every iteration after the first, the argument of
// mci_sweep_common.h for the histogram row.  The host zeroes the words before the launch and copies them out behind it: sums over all
// iterations and blocks of the call.
// merge_pa sums four entries per call, one wave each: the workgroup has at least four waves (the host launches kSweepThreads = 256).
//
// Carried chains (chain_sweep<Cfg, MCMC, true>: the units kUnitSweepChainsCarry | kUnitSweepMcmcCarry, mci_set_sweep_chain_carry; the two units
// above keep their instructions -- everything below stands under `if constexpr (CARRY)` and reads an argument of its own, SweepCarryArgs).  A carried point is integrate(..., nchain = K) on a
// fresh problem with mci_set_chain_carry(prob, 1) and one lane per chain: iteration `it` of the call (0-based) continues the chains of
// iteration it - 1 iff K > 1 and it >= carry_first (1 under :mcmc or with adapt = false; 2 under :vegasmc with adapt = true, whose chains are
// not carried out of the iteration that ran on the map before its first refinement in this call: plan_may_carry).  The first iteration
// of every call starts afresh: chain state does not travel between calls.  Every iteration of such a point stores its chains' ends
// (BatchArgs::store_x | store_curr | store_P) in one of the point's two buffers -- two, because with K > 256 a lane's second chain starts
// after other chains of the block have stored their ends --, and before block b's chains of a carried iteration the workgroup
//   * (:vegasmc) strides over the block's K stored chains with vegasmc_carry_weight (mci_device.h: pi_new / pi_old on the refined map and
//     the moved factors) -> carry_w;
//   * resamples the block with resample_block (mci_train.h; scratch: the front of the LDS segment, where the chain loop's carve is dead;
//     running weights that do not fit there are bisected in the global W) -> carry_src: :mcmc with probability ~ reweight_now[curr] /
//     reweight_used[curr], reweight_used being the factors as they stood when the storing iteration's chains ran (copied before that
//     iteration's doReweight!);
//   * runs the chain loop with carry_* / store_* on the point's rows and the burn-in of a carried launch (nburn = 0; mci_chain_burnin(steps, 1,
//     nslots)).
// All of it is written and read by the point's own workgroup with plain stores and loads, and a sweep_round_trip() stands between each
// writer and its readers: chain ends -> next iteration's weights / resampling (the round trip behind the last block), carry_w ->
// resampling, carry_src -> chain starts, reweight_used -> resampling (the round trips of the leaves' histogram slices).  merge_stats writes
// the blocks' means of every iteration (MergeArgs::block_means) for the host's block-lineage error (mci_lineage_sums).
//
// Chains that go on from the call before (chain_sweep<Cfg, MCMC, true, true>: the units kUnitSweepChainsResume | kUnitSweepMcmcResume, the
// entry points mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume; the four units above keep their instructions --
// everything below stands under `if constexpr (RESUME)` and reads an argument of its own, SweepResumeArgs).  What is said above remains
// true of mci_integrate_sweep_chains | mci_integrate_sweep_mcmc; through the new entry points a point's chain ends go out behind the launch
// (the host copies the buffer the last iteration wrote, (niter - 1) & 1) and come in again as a read-only input segment.  Iteration 0 of a
// point then continues the K_old stored chains per block of its state row where the host found the state to fit (plan_may_carry with the
// state's record in place of the problem's): carry_x | carry_curr | carry_P | carry_nchain | carry_cap | carry_total and ResampleArgs::n_old
// are the state's (K_old, stride blocks * K_old), store_* and n_new the call's K, reweight_used (:mcmc) the state's factors, and the
// resampler's LDS limit (lds_w) is held against K_old.  From iteration 1 on the body is the carried unit's.  The input segment is only
// read, so the ordering argument of mci_sweep_common.h holds as written; carry_W and carry_w have room for max(K_old, K) chains a block.
//
// LDS: the chain loop's carve Lds<Cfg> (tables | histogram | observables | reduction scratch | propose / accept counters) and the
// refinement's scratch share the front of the segment -- each is dead while the other runs --, the point's map block lies behind both
// (SweepHead::map_off; the host's sweep_leaves_lds counts the carve including the counters).
#pragma once
#include "mci_sweep_common.h"

namespace mci {

struct SweepChainArgs {
    SweepHead h;          // h.m.npa = the problem's, h.m.nrows = the blocks; h.t.do_reweight = 1, h.t.nd, h.t.gamma (h.t.goal: none)
    double *reweight;     // [npoint][nd]  in: where every point starts; out: its factors after the last doReweight!
    double *part_pa;      // [npoint][nblocks][2 * npa]  the blocks' propose | accept rows
    int packed_stride;    // doubles of a point's packed row: statistics [nstat] | (histogram [nbin], unused) | propose | accept [2 npa] | holds [64]
    unsigned long long *holds; // [npoint][64] or NULL  :mcmc: the points' holding-time histograms (BatchArgs::hold_hist; zeroed by the host, never read here)
};
// the second argument of the two units with carried chains: the one above, then what a point keeps between its iterations
// (cap = nblocks * nchain).  An argument type of their own, so that the uncarried units' argument -- and with it the offsets their
// instructions address the launch's hidden arguments by -- stays what it was.
struct SweepCarryArgs {
    double *chain_x;      // [npoint][2][ndraw][cap]  the chains' end configurations, two buffers: iteration `it` writes it & 1, reads the other
    int *chain_curr;      // [npoint][2][cap]         :mcmc: the integrand each chain ended on
    double *chain_P;      // [npoint][2][cap]         :vegasmc: the target at each end configuration
    int *carry_src;       // [npoint][cap]            which stored chain of its block each chain continues
    double *carry_W;      // [npoint][cap]            resample_block's running weights
    double *carry_w;      // [npoint][cap]            :vegasmc: pi_new / pi_old of the stored chains
    double *rw_used;      // [npoint][nd]             :mcmc: the factors the stored chains ran under
    double *block_means;  // [npoint][niter][nblocks][nobs]
    double burnin_carried; // BatchArgs::burnin | nburn of a carried iteration (a0 holds those of fresh chains)
    i64 nburn_carried;
    int carry_first;      // the first iteration of the call that continues the one before: 1 | 2
    int lds_w;            // doubles of LDS behind resample_block's partial sums: map_off - kResampleThreads
};
struct SweepChainCarryArgs {
    SweepChainArgs c; // (first: the host fills one object for all four units)
    SweepCarryArgs k;
};
// the third part of the argument of the two units whose first iteration continues the chains of the call before: the two above, then
// the states the points come in with.  A point's row: x [ndraw][blocks * nchain_old] | P [blocks * nchain_old] (:vegasmc) or curr
// [blocks * nchain_old] ints, padded to a double, and reweight_used [nd] (:mcmc)
struct SweepResumeArgs {
    const double *state_in; // [npoint][state_stride]  read only
    i64 state_stride;       // doubles of a row
    i64 nchain_old;         // stored chains per block, > 1
    i64 wcap;               // doubles of a point's carry_W | carry_w row: blocks * max(nchain_old, nchain)
};
struct SweepChainResumeArgs {
    SweepChainArgs c; // (the layout of SweepChainCarryArgs, then the states)
    SweepCarryArgs k;
    SweepResumeArgs r;
};

// pi_new / pi_old of block lb's stored chains: the workgroup's lanes stride over them (vegasmc_carry_weights for one block)
template <class Cfg> __device__ __forceinline__ void carry_weights_block(const BatchArgs &a, const i64 lb) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, T = blockDim.x;
    const Tables<Cfg> t = chain_setup<Cfg, false>(a, smem);
    double rw[Cfg::NI + 1];
    load_reweight<Cfg>(a, rw);
    for (i64 from = tid; from < a.carry_nchain; from += T) vegasmc_carry_weight<Cfg>(a, t, rw, lb * a.carry_nchain + from);
}

template <class Cfg, bool MCMC, bool CARRY = false, bool RESUME = false>
__device__ __forceinline__ void chain_sweep(const BatchArgs &a0, const SweepChainArgs &fc, const SweepCarryArgs *kp = nullptr, const SweepResumeArgs *rp = nullptr) {
    static_assert(CARRY || !RESUME, "only carried chains go on from a state");
    static_assert(Cfg::NLEAF >= 1 && sweep_kinds_ok<Cfg>() && Cfg::NTILE == 1 && Cfg::TABLE_MODE == 0 && Cfg::HCOPY == 1 && Cfg::DET == 0 && Cfg::EC_DOUBLES == 0 &&
                      Cfg::HOST_MEASURE == 0 && Cfg::HOST_INTEGRAND == 0,
                  "a sweep point keeps Continuous and Discrete leaves, their tables and one histogram tile in LDS, and measures on the device (the host checks)");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const SweepHead &f = fc.h;
    const int tid = threadIdx.x, T = blockDim.x;
    constexpr int MAXN = sweep_max_nbin<Cfg>(), NROW = sweep_row_off<Cfg>(Cfg::NLEAF), NPA2 = 2 * PaTable<Cfg>::N;
    using B = SweepBlock<Cfg>;
    double *sm = smem, *hl = sm + train_lds_doubles(MAXN), *ps = hl + MAXN, *blk = smem + f.map_off;
    double *bedges = blk + B::E, *bdacc = blk + B::DA, *bddist = blk + B::DD, *flags = blk + B::FLAGS;
    int *bad = reinterpret_cast<int *>(flags); // bad[0], bad[1]: the verdicts of the even and the odd leaves; flags[2]: train_leaf's spare word
    const int nblocks = f.m.nblocks;
    for (int p = (int)blockIdx.x; p < f.npoint; p += (int)gridDim.x) {
        __syncthreads(); // (the point before: its last LDS reads are through)
        if (f.maps_in) sweep_copy_row<Cfg, false>(blk, nullptr, f.maps_in + (size_t)p * NROW);
        else {
            for (int i = tid; i < Cfg::NEDGE; i += T) bedges[i] = f.t.edges[i];
            for (int i = tid; i < Cfg::NDACC; i += T) bdacc[i] = f.t.dacc[i];
            for (int i = tid; i < Cfg::NDDIST; i += T) bddist[i] = f.t.ddist[i];
        }
        MergeArgs m;
        BatchArgs a;
        sweep_point<Cfg>(f, a0, p, nblocks, m, a);
        double *rw = fc.reweight + (size_t)p * f.t.nd;
        m.packed = f.m.packed + (size_t)p * fc.packed_stride; // (this unit's rows are longer than the statistics head: the tables follow)
        m.part_pa = fc.part_pa + (size_t)p * nblocks * NPA2;
        a.part_pa = fc.part_pa + (size_t)p * nblocks * NPA2;
        a.reweight = rw;
        a.hold_hist = fc.holds ? fc.holds + (size_t)p * 64 : nullptr; // (:vegasmc never looks at it)
        a.edges = bedges; // (LDS through the generic address space: stage_tables reads the three tables once per call)
        a.dacc = bdacc;
        a.ddist = bddist;
        // carried chains: this point's rows (cap stored chains a buffer); nothing is kept or continued with one chain per block
        const i64 cap = (i64)nblocks * a0.nchain;
        const bool keep = CARRY && a0.nchain > 1;
        double *rwu = nullptr;
        if constexpr (CARRY) rwu = kp->rw_used + (size_t)p * f.t.nd;
        for (int it = 0; it < f.niter; ++it) {
            a.iteration = a0.iteration + (u32)it;
            if (tid == 0) bad[0] = 0;
            bool cont = false; // this iteration's chains continue those of the one before
            bool first = false; // ... those of the call before: the point's state row
            if constexpr (CARRY) {
                const SweepCarryArgs &fk = *kp;
                cont = keep && it >= fk.carry_first;
                if constexpr (RESUME) {
                    first = keep && it == 0;
                    cont = cont || first;
                }
                if (keep) {
                    const int wb = it & 1;
                    double *x2 = fk.chain_x + (size_t)p * 2 * Cfg::NDRAW * cap;
                    a.store_x = x2 + (size_t)wb * Cfg::NDRAW * cap;
                    a.store_cap = cap;
                    if constexpr (MCMC) a.store_curr = fk.chain_curr + ((size_t)p * 2 + wb) * cap;
                    else a.store_P = fk.chain_P + ((size_t)p * 2 + wb) * cap;
                    a.carry_x = cont ? x2 + (size_t)(1 - wb) * Cfg::NDRAW * cap : nullptr;
                    a.carry_nchain = a0.nchain;
                    a.carry_cap = cap;
                    a.carry_src = cont ? fk.carry_src + (size_t)p * cap : nullptr;
                    if constexpr (MCMC) {
                        a.carry_curr = fk.chain_curr + ((size_t)p * 2 + (1 - wb)) * cap;
                        a.nburn = cont ? fk.nburn_carried : a0.nburn;
                    } else {
                        a.carry_P = fk.chain_P + ((size_t)p * 2 + (1 - wb)) * cap;
                        a.carry_w = fk.carry_w + (size_t)p * cap;
                        a.carry_total = cap;
                        a.burnin = cont ? fk.burnin_carried : a0.burnin;
                    }
                    if constexpr (RESUME) {
                        const SweepResumeArgs &fr = *rp;
                        if constexpr (!MCMC) a.carry_w = fk.carry_w + (size_t)p * fr.wcap;
                        if (first) { // the stored side is the state's: nchain_old chains a block, a row of its own
                            const i64 cap_old = (i64)nblocks * fr.nchain_old;
                            const double *row = fr.state_in + (size_t)p * fr.state_stride;
                            a.carry_x = row;
                            a.carry_nchain = fr.nchain_old;
                            a.carry_cap = cap_old;
                            if constexpr (MCMC) a.carry_curr = reinterpret_cast<const int *>(row + (size_t)Cfg::NDRAW * cap_old);
                            else {
                                a.carry_P = row + (size_t)Cfg::NDRAW * cap_old;
                                a.carry_total = cap_old;
                            }
                        }
                    }
                }
                m.block_means = fk.block_means + ((size_t)p * f.niter + it) * nblocks * f.m.nobs;
            }
            for (int b = 0; b < nblocks; ++b) {
                a.chunk_lo = b;  // work_item: row = block (wg_per_block = 1)
                if constexpr (CARRY) {
                    if (cont) { // which stored chain of block b each of its chains continues: the stored ones resampled to the moved target
                        const SweepCarryArgs &fk = *kp;
                        ResampleArgs ra;
                        ra.curr_old = a.carry_curr;
                        ra.n_old = ra.n_new = a0.nchain;
                        ra.nd = f.t.nd;
                        ra.rw_now = rw;
                        ra.rw_used = rwu;
                        ra.src = fk.carry_src + (size_t)p * cap;
                        ra.W = fk.carry_W + (size_t)p * cap;
                        ra.w_chain = nullptr;
                        if constexpr (RESUME) {
                            const SweepResumeArgs &fr = *rp;
                            ra.W = fk.carry_W + (size_t)p * fr.wcap;
                            if (first) {
                                ra.n_old = fr.nchain_old;
                                if constexpr (MCMC) // (behind the integrand indices, which end on a double)
                                    ra.rw_used = fr.state_in + (size_t)p * fr.state_stride + (size_t)Cfg::NDRAW * nblocks * fr.nchain_old + ((size_t)nblocks * fr.nchain_old + 1) / 2;
                            }
                        }
                        __syncthreads(); // (whatever read the front of the LDS segment before is through)
                        if constexpr (!MCMC) {
                            carry_weights_block<Cfg>(a, b);
                            sweep_round_trip(); // carry_w -> resampling (and the staged tables are read: the scratch takes their place)
                            ra.w_chain = a.carry_w;
                        }
                        resample_block(ra, b, smem, fk.lds_w);
                        sweep_round_trip(); // carry_src -> chain starts
                    }
                }
                __syncthreads(); // (map, flag and -- from the second iteration on -- whatever read this LDS before are through)
                // tables <- the map block, the block's chains, its partial row and its propose | accept row, histogram atomics into this point's row
                if constexpr (MCMC) mcmc_chains<Cfg>(a); else vegasmc_chains<Cfg>(a);
            }
            sweep_round_trip();
            if constexpr (CARRY && MCMC) { // the factors this iteration's chains ran under: doReweight! moves them below
                if (keep)
                    for (int i = tid; i < f.t.nd; i += T) rwu[i] = rw[i];
            }
            merge_stats(m); // main.jl:273-287
            for (int e = 0; e < merge_pa_blocks(m); ++e) merge_pa(m, e); // configuration.jl:297-298
            __syncthreads(); // the head of `packed` was written by this workgroup
            TrainArgs t = sweep_log_row(f, p, it);
            t.packed = m.packed;
            t.reweight = rw;
            iteration_bookkeeping(t); // log row; doReweight! by thread 0 (main.jl:183: whatever `adapt` says)
#pragma unroll 1
            for (int l = 0; l < Cfg::NLEAF; ++l) {
                const LeafDev L = f.t.leaves[l];
                const int N = L.nbin;
                const bool train = f.t.do_train && L.adapt; // variable.jl:208
                int *verdict = bad + (l & 1);
                if (tid == 0) bad[(l + 1) & 1] = 0; // (the next leaf's; its last reader passed the barrier that closed the leaf before this one)
                sweep_take_hist(m.ghist + L.boff, hl, N, (tid + T - L.boff % T) % T, (double)(nblocks + 1) * 1.0e-10, verdict);
                sweep_round_trip(); // (hl, the verdict, the reweight factors; the zeroed slice is out before the next iteration adds to it)
                if (train) train_leaf(L, hl, nullptr, sm, ps, *verdict, flags[2], bedges, bdacc, bddist, 0, m.status, false, nullptr, true);
                __syncthreads();
            }
        }
        sweep_copy_row<Cfg, true>(blk, f.maps_out + (size_t)p * NROW, nullptr);
    }
}

template <class Cfg> __device__ __forceinline__ void vegasmc_sweep(const BatchArgs &a0, const SweepChainArgs &fc) { chain_sweep<Cfg, false>(a0, fc); }
template <class Cfg> __device__ __forceinline__ void mcmc_sweep(const BatchArgs &a0, const SweepChainArgs &fc) { chain_sweep<Cfg, true>(a0, fc); }
// ... and with chains carried from iteration to iteration (mci_set_sweep_chain_carry): two more units, the same body
template <class Cfg> __device__ __forceinline__ void vegasmc_sweep_carry(const BatchArgs &a0, const SweepChainCarryArgs &f) { chain_sweep<Cfg, false, true>(a0, f.c, &f.k); }
template <class Cfg> __device__ __forceinline__ void mcmc_sweep_carry(const BatchArgs &a0, const SweepChainCarryArgs &f) { chain_sweep<Cfg, true, true>(a0, f.c, &f.k); }
// ... and with a first iteration that continues the chains of the call before (mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume)
template <class Cfg> __device__ __forceinline__ void vegasmc_sweep_resume(const BatchArgs &a0, const SweepChainResumeArgs &f) { chain_sweep<Cfg, false, true, true>(a0, f.c, &f.k, &f.r); }
template <class Cfg> __device__ __forceinline__ void mcmc_sweep_resume(const BatchArgs &a0, const SweepChainResumeArgs &f) { chain_sweep<Cfg, true, true, true>(a0, f.c, &f.k, &f.r); }

} // namespace mci
