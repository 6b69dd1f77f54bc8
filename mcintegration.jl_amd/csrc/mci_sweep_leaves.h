// mci_sweep_leaves.h -- batched :vegas parameter sweeps of problems with SEVERAL variable leaves, Continuous and Discrete (the opt-in
// mci_set_sweep_leaves(prob, MCI_SWEEP_ALL_LEAVES)): vegas_sweep of mci_sweep.h generalised from one Continuous grid to the whole map.
// Compiled by hiprtc next to mci_device.h, mci_train.h and mci_sweep_common.h into a translation unit of its own (mci_jit.h kUnitSweepLeaves): the
// one-grid sweep unit, the classic, persistent and stratified code objects stay what they were.  Free of host / std headers.
//
//     workgroup g   for p = g, g + G, ...:   map of point p (every grid, every Discrete accumulation and distribution) -> LDS;
//                   for every iteration:  for every statistical block: sample it (vegas_batch) -> merge the block rows (merge_stats) ->
//                   statistics head -> this point's log row -> leaf by leaf: the merged histogram slice with the clearStatistics!
//                   offsets -> train! on the leaf's part of the LDS map (train_leaf: prefix-scan walk, or the Discrete form);
//                   at the end the map -> maps_out[p]
//
// The synchronisation is mci_sweep_common.h's, in its general form: a leaf's slice [boff, boff + nbin) of the histogram row is read and
// zeroed by the thread whose index is (boff + i) % T for bin boff + i.
//
// The map block  edges[NEDGE] | dacc[NDACC] | ddist[NDDIST] | flags[4]  (each part starting on 16 bytes) lies behind BOTH the sample
// loop's carve and the refinement's scratch.  vegas_batch reads all three tables from it once per call (stage_tables) behind a barrier;
// train_leaf writes a leaf's part of it -- a grid through `edges + eoff` by all threads, a Discrete leaf's `dacc + eoff` and
// `ddist + doff` by thread 0 -- and a barrier follows every leaf.  Everything a point leaves in LDS is written again before the next
// point reads it: the block is filled from maps_in[p] (or the problem's own tables) behind the barrier that opens a point, vegas_batch
// stages the tables and zeroes its histogram and observable copies at every call, train_leaf fills its scratch before it reads it, the
// merged slice is written before it is read, and the two verdict words are reset before the leaf that uses them (they alternate, so
// that a reset never meets the atomicOr of the leaf before without a barrier in between).
//
// vegas_sweep_leaves<Cfg, true> (kernel mci_vegas_sweep_leaves_until, mci_integrate_sweep_until on a problem that opted in) is the same
// body with a target error per point, everything new under `if constexpr (UNTIL)`: what mci_sweep.h says of vegas_sweep<Cfg, true>.  The
// verdict and the next point are the two words of flags[3], which nothing else uses; the verdict is read behind a leaf's round trip
// and held until the last leaf's train! and its closing barrier have passed.
#pragma once
#include "mci_sweep_common.h"

namespace mci {

template <class Cfg, bool UNTIL = false> __device__ __forceinline__ void vegas_sweep_leaves(const BatchArgs &a0, const SweepHead &f, const SweepUntil *u = nullptr) {
    static_assert(Cfg::NLEAF >= 1 && sweep_kinds_ok<Cfg>() && Cfg::NTILE == 1 && Cfg::TABLE_MODE == 0 && (UNTIL ? Cfg::DET != 0 : Cfg::HCOPY == 1 && Cfg::DET == 0) && Cfg::EC_DOUBLES == 0,
                  "a sweep point keeps Continuous and Discrete leaves, their tables and one histogram tile in LDS (the host checks)");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, T = blockDim.x;
    constexpr int MAXN = sweep_max_nbin<Cfg>(), NROW = sweep_row_off<Cfg>(Cfg::NLEAF);
    using B = SweepBlock<Cfg>;
    double *sm = smem, *hl = sm + train_lds_doubles(MAXN), *ps = hl + MAXN, *blk = smem + f.map_off;
    double *bedges = blk + B::E, *bdacc = blk + B::DA, *bddist = blk + B::DD, *flags = blk + B::FLAGS;
    int *bad = reinterpret_cast<int *>(flags); // bad[0], bad[1]: the verdicts of the even and the odd leaves; flags[2]: train_leaf's spare word
    int *words = reinterpret_cast<int *>(flags + 3); // UNTIL's verdict | next point
    const int nblocks = f.m.nblocks;
    int n_run = f.niter;
    for (int p = (int)blockIdx.x; p < f.npoint; p = sweep_next_point<UNTIL>(p, u, words, n_run)) {
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
        a.edges = bedges; // (LDS through the generic address space: stage_tables reads the three tables once per call)
        a.dacc = bdacc;
        a.ddist = bddist;
        if constexpr (UNTIL) n_run = f.niter;
        for (int it = 0; it < f.niter; ++it) {
            a.iteration = a0.iteration + (u32)it;
            if (tid == 0) bad[0] = 0;
            if constexpr (UNTIL)
                if (tid == 0) words[0] = 0;
            for (int b = 0; b < nblocks; ++b) {
                a.chunk_lo = b;  // work_item: row = block (wg_per_block = 1)
                __syncthreads(); // (map and flag complete; whatever read this LDS before is through)
                vegas_batch<Cfg, false>(a); // tables <- the map block, the block's samples, its partial row, histogram atomics into this point's row
            }
            sweep_round_trip();
            merge_stats(m); // main.jl:273-287
            __syncthreads(); // the head of `packed` was written by this workgroup
            const TrainArgs t = sweep_log_row(f, p, it);
            iteration_bookkeeping(t);
            [[maybe_unused]] bool done = false;
            if constexpr (UNTIL) sweep_until_columns(*u, m.packed, f.m.nobs, nblocks, p, it + 1, words);
#pragma unroll 1
            for (int l = 0; l < Cfg::NLEAF; ++l) {
                const LeafDev L = f.t.leaves[l];
                const int N = L.nbin;
                const bool train = f.t.do_train && L.adapt; // variable.jl:208
                int *verdict = bad + (l & 1);
                if (tid == 0) bad[(l + 1) & 1] = 0; // (the next leaf's; its last reader passed the barrier that closed the leaf before this one)
                // merge_hist_bin: clearStatistics! offsets + what the blocks added; the slice is zero again for the next iteration
                // (this thread's first bin of the slice: (boff + first) % T == tid)
                sweep_take_hist(m.ghist + L.boff, hl, N, (tid + T - L.boff % T) % T, (double)(nblocks + 1) * 1.0e-10, verdict);
                sweep_round_trip(); // (hl, the verdict; the zeroed slice is out before the next iteration adds to it)
                if constexpr (UNTIL) done = words[0] == 0;
                // a bad histogram: this leaf's train! refuses (its map stays), the bits go to this point's status word; the other leaves
                // and the other points never see it
                if (train) train_leaf(L, hl, nullptr, sm, ps, *verdict, flags[2], bedges, bdacc, bddist, 0, m.status, false, nullptr, true);
                __syncthreads();
            }
            if constexpr (UNTIL)
                if (done) { // (the whole workgroup read one verdict)
                    n_run = it + 1;
                    break;
                }
        }
        sweep_copy_row<Cfg, true>(blk, f.maps_out + (size_t)p * NROW, nullptr);
    }
}

template <class Cfg> __device__ __forceinline__ void vegas_sweep_leaves_until(const BatchArgs &a0, const SweepUntilArgs &f) { vegas_sweep_leaves<Cfg, true>(a0, f.h, &f.u); }

} // namespace mci
