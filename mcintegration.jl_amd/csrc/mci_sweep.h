// mci_sweep.h -- batched :vegas parameter sweeps: P independent integrals in ONE launch (mci_integrate_sweep).
// Compiled by hiprtc next to mci_device.h and mci_train.h into a translation unit of its own (mci_jit.h kUnitSweep): the classic,
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
// No workgroup ever waits for another one: no grid-wide counters, no spinning, no residency condition, and every loop's trip count is a
// kernel argument.  What travels through global memory inside a point -- the blocks' partial rows, merge_stats' scratch and head, the
// histogram row the blocks add to with f64 atomics -- is written and read by the SAME workgroup: between the two sides every wave
// waits for its own stores and atomics (s_waitcnt vmcnt(0): a barrier alone orders nothing in global memory, see persist_signal in
// mci_train.h) and the workgroup meets at a barrier; the CU's write-through L1 is coherent for its own workgroup's plain stores,
// and the histogram row, which the atomics change in L2 behind that L1, is read with agent-scope atomic loads that bypass it.
// Bin i of that row is only ever touched by thread i % T (flush_workgroup's adds, the read and the zeroing below), in program order.
//
// Everything a point leaves in LDS is written again before the next point reads it: vegas_batch stages the tables from the map and
// zeroes its histogram and observable copies at every call, train_leaf fills its scratch before it reads it, and the map, the `bad`
// flag and the merged histogram are set here per point / iteration.
#pragma once
#include "mci_train.h"

namespace mci {

struct SweepArgs {
    MergeArgs m;           // of point 0: part_cols [npoint][nblocks][ncols], scratch [npoint][nblocks * ncols], packed [npoint][nstat],
                           // ghist [npoint][nbin], status [npoint]; use_ghist = 1, wg_per_block = 1
    TrainArgs t;           // t.edges: the problem's own map (read only: where a point starts when maps_in == NULL); t.iter_log_row:
                           // [npoint][niter][nstat]
    int npoint, niter, nuserdata;
    int map_off;           // doubles: LDS behind both the sample loop's carve and the refinement's (PersistArgs::map_off)
    const double *ud;      // [npoint][nuserdata]
    const u64 *seeds;      // [npoint] or NULL: BatchArgs::seed for every point
    const double *maps_in; // [npoint][N + 1] or NULL
    double *maps_out;      // [npoint][N + 1]
};

// every wave has performed its global stores and atomics, then the workgroup meets
__device__ __forceinline__ void sweep_global_round_trip() {
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
    __syncthreads();
}

template <class Cfg> __device__ __forceinline__ void vegas_sweep(const BatchArgs &a0, const SweepArgs &f) {
    static_assert(Cfg::NLEAF == 1 && Cfg::leaf_kind(0) == 0 && Cfg::NTILE == 1, "a sweep point refines ONE Continuous grid in one tile (the host checks)");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, T = blockDim.x;
    constexpr int N = Cfg::leaf_nbin(0);
    double *sm = smem, *hl = sm + train_lds_doubles(N), *ps = hl + N, *gcur = smem + f.map_off, *flags = gcur + N + 2;
    int *bad = reinterpret_cast<int *>(flags);
    const LeafDev L = f.t.leaves[0];
    const bool train = f.t.do_train && L.adapt; // variable.jl:208
    const int nblocks = f.m.nblocks, ncols = f.m.ncols, nstat = f.t.nstat;
    for (int p = (int)blockIdx.x; p < f.npoint; p += (int)gridDim.x) {
        __syncthreads(); // (the point before: its last LDS reads are through)
        const double *g0 = f.maps_in ? f.maps_in + (size_t)p * (N + 1) : f.t.edges + L.eoff;
        for (int i = tid; i <= N; i += T) gcur[i] = g0[i];
        MergeArgs m = f.m;
        m.part_cols = f.m.part_cols + (size_t)p * nblocks * ncols;
        m.scratch = f.m.scratch + (size_t)p * nblocks * ncols;
        m.packed = f.m.packed + (size_t)p * nstat;
        m.ghist = f.m.ghist + (size_t)p * Cfg::NBIN;
        m.status = f.m.status + p;
        BatchArgs a = a0;
        a.edges = gcur - L.eoff; // (LDS through the generic address space: stage_tables reads it once per call)
        a.ud = f.ud + (size_t)p * f.nuserdata;
        a.part_cols = const_cast<double *>(m.part_cols);
        a.ghist = m.ghist;
        a.status = m.status;
        if (f.seeds) a.seed = f.seeds[p];
        for (int it = 0; it < f.niter; ++it) {
            a.iteration = a0.iteration + (u32)it;
            if (tid == 0) *bad = 0;
            for (int b = 0; b < nblocks; ++b) {
                a.chunk_lo = b;  // work_item: row = block (wg_per_block = 1)
                __syncthreads(); // (map and flag complete; whatever read this LDS before is through)
                vegas_batch<Cfg, false>(a); // pair table <- gcur, the block's samples, its partial row, histogram atomics into this point's row
            }
            sweep_global_round_trip();
            merge_stats(m); // main.jl:273-287
            __syncthreads(); // the head of `packed` was written by this workgroup
            TrainArgs t = f.t;
            t.packed = m.packed;
            t.iter_log_row = f.t.iter_log_row + ((size_t)p * f.niter + it) * nstat;
            iteration_bookkeeping(t);
            // merge_hist_bin: clearStatistics! offsets + what the blocks added; the row is zero again for the next iteration
            double *gh = m.ghist + L.boff;
            int hbad = 0;
            for (int base = 0; base < N; base += kTrainQ * T) {
                double v[kTrainQ];
#pragma unroll
                for (int q = 0; q < kTrainQ; ++q) {
                    const int i = base + q * T + tid;
                    v[q] = i < N ? __hip_atomic_load(&gh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
                }
#pragma unroll
                for (int q = 0; q < kTrainQ; ++q) {
                    const int i = base + q * T + tid;
                    if (i < N) {
                        __hip_atomic_store(&gh[i], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const double h = (double)(nblocks + 1) * 1.0e-10 + v[q];
                        hl[i] = h;
                        if (!isfinite(h)) hbad |= ST_HIST_NONFINITE;      // variable.jl:212
                        else if (!(h > 0.0)) hbad |= ST_HIST_NONPOSITIVE; // variable.jl:213 / common.jl:71
                    }
                }
            }
            if (hbad) atomicOr(bad, hbad);
            sweep_global_round_trip(); // (hl, the verdict; the zeroed row is out before the next iteration adds to it)
            // a bad histogram: train! refuses (the map stays), the bits go to this point's status word, the other points never see it
            if (train) train_leaf(L, hl, nullptr, sm, ps, *bad, flags[1], gcur - L.eoff, f.t.dacc, f.t.ddist, 0, m.status, false, nullptr, true);
            __syncthreads();
        }
        for (int i = tid; i <= N; i += T) f.maps_out[(size_t)p * (N + 1) + i] = gcur[i];
    }
}

} // namespace mci
