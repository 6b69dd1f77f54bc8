// mci_sweep.h -- batched :vegas parameter sweeps: P independent integrals in ONE launch (mci_integrate_sweep).
// Compiled by hiprtc next to mci_device.h, mci_train.h and mci_sweep_common.h into a translation unit of its own (mci_jit.h kUnitSweep): the classic,
// persistent and stratified code objects stay what they were.  Free of host / std headers.
//
// A scan over a parameter (an external momentum, a temperature, a coupling) is P launch-bound integrate() calls that differ in
// nothing but the closure's captured floats -- the `ud` row.  Each of them is small enough for ONE workgroup to run its whole loop
// (main.jl:142-207), so the parallelism is taken across the points:
//
//     workgroup g   for p = g, g + G, ...:   map of point p -> LDS;  for every iteration:  for every statistical block: sample it
//                   (vegas_batch: the same code, the same Philox indices and sums as a sampling workgroup of the ordinary call with
//                   wg_per_block = 1) -> merge the block rows (merge_stats) -> statistics head -> this point's log row -> merged
//                   histogram with the clearStatistics! offsets -> train! on the LDS map (train_leaf, prefix-scan walk);
//                   at the end the map -> maps_out[p]
//
// The synchronisation -- nothing waits grid-wide; a round trip between the two sides of whatever a point passes through global memory;
// who touches which histogram bin -- is mci_sweep_common.h's, with the grid's slice at boff = 0: bin i belongs to thread i % T.
//
// Everything a point leaves in LDS is written again before the next point reads it: vegas_batch stages the tables from the map and
// zeroes its histogram and observable copies at every call, train_leaf fills its scratch before it reads it, and the map, the `bad`
// flag and the merged histogram are set here per point / iteration.
//
// vegas_sweep<Cfg, true> (kernel mci_vegas_sweep_until, mci_integrate_sweep_until) is the same body with a target error per point:
// everything it adds stands under `if constexpr (UNTIL)`.  Behind merge_stats the stop rule of mci_sweep_common.h runs on the statistics
// head (sweep_until_columns); the workgroup's verdict -- words[0] of the last flag slot, which nothing else uses: the host's layout counts
// four -- is complete behind the round trip that follows and is read THERE, between two barriers, because thread 0 resets the word
// behind the iteration's closing barrier.  A converged point runs this iteration's train! and leaves its loop; the workgroup takes
// its next point from the cursor (sweep_next_point).
#pragma once
#include "mci_sweep_common.h"

namespace mci {

template <class Cfg, bool UNTIL = false> __device__ __forceinline__ void vegas_sweep(const BatchArgs &a0, const SweepHead &f, const SweepUntil *u = nullptr) {
    static_assert(Cfg::NLEAF == 1 && Cfg::leaf_kind(0) == 0 && Cfg::NTILE == 1, "a sweep point refines ONE Continuous grid in one tile (the host checks)");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, T = blockDim.x;
    constexpr int N = Cfg::leaf_nbin(0);
    double *sm = smem, *hl = sm + train_lds_doubles(N), *ps = hl + N, *gcur = smem + f.map_off, *flags = gcur + N + 2;
    int *bad = reinterpret_cast<int *>(flags), *words = reinterpret_cast<int *>(flags + 3); // words: UNTIL's verdict | next point
    const LeafDev L = f.t.leaves[0];
    const bool train = f.t.do_train && L.adapt; // variable.jl:208
    const int nblocks = f.m.nblocks;
    int n_run = f.niter;
    for (int p = (int)blockIdx.x; p < f.npoint; p = sweep_next_point<UNTIL>(p, u, words, n_run)) {
        __syncthreads(); // (the point before: its last LDS reads are through)
        const double *g0 = f.maps_in ? f.maps_in + (size_t)p * (N + 1) : f.t.edges + L.eoff;
        for (int i = tid; i <= N; i += T) gcur[i] = g0[i];
        MergeArgs m;
        BatchArgs a;
        sweep_point<Cfg>(f, a0, p, nblocks, m, a);
        a.edges = gcur - L.eoff; // (LDS through the generic address space: stage_tables reads it once per call)
        if constexpr (UNTIL) n_run = f.niter;
        for (int it = 0; it < f.niter; ++it) {
            a.iteration = a0.iteration + (u32)it;
            if (tid == 0) *bad = 0;
            if constexpr (UNTIL)
                if (tid == 0) words[0] = 0;
            for (int b = 0; b < nblocks; ++b) {
                a.chunk_lo = b;  // work_item: row = block (wg_per_block = 1)
                __syncthreads(); // (map and flag complete; whatever read this LDS before is through)
                vegas_batch<Cfg, false>(a); // pair table <- gcur, the block's samples, its partial row, histogram atomics into this point's row
            }
            sweep_round_trip();
            merge_stats(m); // main.jl:273-287
            __syncthreads(); // the head of `packed` was written by this workgroup
            const TrainArgs t = sweep_log_row(f, p, it);
            iteration_bookkeeping(t);
            if constexpr (UNTIL) sweep_until_columns(*u, m.packed, f.m.nobs, nblocks, p, it + 1, words);
            // merge_hist_bin: clearStatistics! offsets + what the blocks added; the row is zero again for the next iteration
            sweep_take_hist(m.ghist + L.boff, hl, N, tid, (double)(nblocks + 1) * 1.0e-10, bad);
            sweep_round_trip(); // (hl, the verdict; the zeroed row is out before the next iteration adds to it)
            [[maybe_unused]] bool done = false;
            if constexpr (UNTIL) done = words[0] == 0;
            // a bad histogram: train! refuses (the map stays), the bits go to this point's status word, the other points never see it
            if (train) train_leaf(L, hl, nullptr, sm, ps, *bad, flags[1], gcur - L.eoff, f.t.dacc, f.t.ddist, 0, m.status, false, nullptr, true);
            __syncthreads();
            if constexpr (UNTIL)
                if (done) { // (the whole workgroup read one verdict)
                    n_run = it + 1;
                    break;
                }
        }
        for (int i = tid; i <= N; i += T) f.maps_out[(size_t)p * (N + 1) + i] = gcur[i];
    }
}

template <class Cfg> __device__ __forceinline__ void vegas_sweep_until(const BatchArgs &a0, const SweepUntilArgs &f) { vegas_sweep<Cfg, true>(a0, f.h, &f.u); }

} // namespace mci
