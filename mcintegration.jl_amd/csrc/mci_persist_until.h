// mci_persist_until.h -- the persistent :vegas launch of mci_train.h (vegas_persist: all iterations of a launch-bound integrate() call as
// ONE launch) with a target error: mci_integrate_until on a default-size :vegas call.  A translation unit of its own (mci_jit.h
// kUnitVegasPersistUntil, kernel mci_vegas_persist_until), so that mci_train.h, the fixed persistent unit and the sweep units keep their
// text, their kernel-cache keys and their code objects: what follows is vegas_persist's protocol -- same waits, same counters, same three
// histogram buffers, same two partial-row buffers; read its header comment first -- plus the four things a stop needs.  Free of host /
// std headers.
//
// The rule runs in the statistics workgroup behind the block merge of turn `it`: sweep_until_columns (mci_sweep_common.h) as it stands,
// column o is thread o % T's, its running sums W | S in a row of global memory only that thread touches (zeroed by the same thread when
// the launch starts: nothing for the host to reset).  On convergence at turn `it` < niter - 1 the workgroup leaves in `packed` what the
// last turn of a launch leaves there (the merged histogram, or train!'s clearStatistics! state), writes the turn's log row as ever,
// stores done0 + it + 1 into the stop word ctr[3] BEFORE its persist_signal -- thread 0's store, then thread 0's agent-scope release
// fence and counter add: whoever sees the turn counted sees the word -- and leaves its loop.  The word holds an ABSOLUTE turn count, so
// like the counters it only grows and is never reset between launches: stop_n = word - done0 where word > done0, else 0 (what an
// earlier launch left is <= this launch's done0).  A verdict in the last turn changes nothing and is not written.
//
// The invariant that keeps the grid from disagreeing.  The statistics workgroup runs one turn behind the samplers: a sampler that
// passes its persist_wait of turn `it` has seen `done0 + it` turns counted, so the verdicts of turns < it are visible to it (published
// before those counts), and the verdict of turn `it` itself may or may not be.  It therefore acts on stop_n only when 1 <= stop_n <= it
// and ignores anything larger until the next turn -- for every thread of every sampling workgroup the answer in turn `it` is the same,
// whenever it loads the word (only one store ever happens in a launch).  All G sampling workgroups thus leave in turn it = stop_n, behind
// that turn's wait, with its samples discarded: no train_leaf (their maps have seen stop_n refinements, what workgroup 0 writes back),
// and the statistics workgroup has left its loop, so no log row.  The price of a stop is that one turn of samples, at most one
// iteration of a launch-bound call.
//
// Clean-up.  The statistics workgroup then waits for all G arrivals of turn stop_n and the samplers' final "through" signal -- (stop_n +
// 2) G arrivals since the launch began -- and zeroes BOTH dirty histogram buffers: turn stop_n - 1's (the one a later turn would have
// zeroed) and turn stop_n's with the discarded adds.
//
// Counters (the host's record, mci_host_integrate.h persist_launch / integrate_call).  A launch that stopped at stop_n < niter adds
// (stop_n + 2) G to the arrive count -- turns 0 .. stop_n arrive once each, plus the final signal -- and stop_n to the done count
// (turns 0 .. stop_n - 1).  One that ran all niter turns adds (niter + 1) G and niter, like vegas_persist.  The host reads the stop word
// behind the launch, in the synchronisation it makes anyway, and advances its record by what the launch really added; a wrong record
// shows as ST_PERSIST_STALL on the NEXT persistent launch (the waits stay bounded in wall-clock time), not as a hang.
#pragma once
#include "mci_sweep_common.h"

namespace mci {

struct PersistUntilArgs {
    PersistArgs p; // (first: the fixed unit's fields where the fixed unit has them)
    SweepUntil u;  // rtol, atol, min_niter, ignore; sums: [2 nobs], this launch's W | S; iters, cursor: unused (NULL)
};
enum { kPersistStopWord = 3 }; // PersistArgs::ctr[3]: done0 + stop_n of the last launch that stopped early

template <class Cfg> __device__ __forceinline__ void vegas_persist_until(const BatchArgs &a0, const PersistUntilArgs &fu) {
    static_assert(Cfg::NLEAF == 1 && Cfg::leaf_kind(0) == 0, "the persistent kernel refines ONE Continuous grid (the host checks)");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const PersistArgs &f = fu.p;
    const int tid = threadIdx.x, T = blockDim.x;
    constexpr int N = Cfg::leaf_nbin(0);
    double *sm = smem, *hl = sm + train_lds_doubles(N), *ps = hl + N, *gcur = smem + f.map_off, *flags = gcur + N + 2;
    int *verdict = reinterpret_cast<int *>(flags + 2), *pending = reinterpret_cast<int *>(flags + 3); // (the last of the four flag slots)
    const u64 G = gridDim.x - 1; // sampling workgroups; workgroup G merges the statistics
    const int wg = (int)blockIdx.x;
    const size_t rows = (size_t)G * f.m.ncols;
    const LeafDev L = f.t.leaves[0];
    const bool train = f.t.do_train && L.adapt; // variable.jl:208
    if (wg == (int)G) { // ---- the statistics workgroup
        for (int o = tid; o < f.m.nobs; o += T) fu.u.sums[o] = fu.u.sums[f.m.nobs + o] = 0.0; // (column o's sums: this thread's alone)
        int stop_n = 0;
        for (int it = 0; it < f.niter; ++it) {
            if (!persist_wait(f, f.arrive0 + (u64)(it + 1) * G, f.done0 + (u64)it, verdict)) return;
            MergeArgs m = f.m;
            m.part_cols = f.m.part_cols + (size_t)(it & 1) * rows;
            merge_stats(m); // main.jl:273-287
            // config.propose / config.accept of a :vegas iteration: the clearStatistics! offsets alone (configuration.jl:247-248)
            for (int e = tid; e < 2 * m.npa; e += T)
                m.packed[2 * m.nobs + 2 + m.ni + 1 + m.nbin + e] = (double)(m.nblocks + 1) * (e < m.npa ? 1.0e-8 : 1.0e-10);
            if (it > 0) { // the histogram buffer of the turn before: everybody who read it has arrived again
                double *gz = a0.ghist + (size_t)((it + 2) % 3) * Cfg::NBIN + L.boff;
                for (int i = tid; i < N; i += T) gz[i] = 0.0;
            }
            if (tid == 0) *pending = 0;
            __syncthreads(); // the head of `packed` was written by this workgroup; the rule's word is reset
            sweep_until_columns(fu.u, m.packed, m.nobs, m.nblocks, 0, it + 1, pending);
            __syncthreads();
            const bool stop = *pending == 0 && it < f.niter - 1;
            if (it == f.niter - 1 || stop) { // what the launch leaves in `packed`: the merged histogram, or train!'s clearStatistics! (variable.jl:238 -> :565)
                const double *gh = a0.ghist + (size_t)(it % 3) * Cfg::NBIN + L.boff;
                double *hp = f.t.packed + f.t.nstat + L.boff;
                for (int i = tid; i < N; i += T)
                    hp[i] = train ? 1.0e-10 : (double)(m.nblocks + 1) * 1.0e-10 + __hip_atomic_load(&gh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            TrainArgs t = f.t;
            if (t.iter_log_row) t.iter_log_row += (size_t)it * t.nstat;
            iteration_bookkeeping(t);
            __syncthreads();
            // (thread 0's store, then -- inside persist_signal -- thread 0's release fence and its add to the counter)
            if (stop && tid == 0) __hip_atomic_store(&f.ctr[kPersistStopWord], f.done0 + (u64)(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            persist_signal(&f.ctr[0], 1ull << kPersistDoneShift);
            if (stop) {
                stop_n = it + 1;
                break;
            }
        }
        if (stop_n) { // turn stop_n's arrivals and the samplers' final signal: both dirty buffers, turn stop_n - 1's and turn stop_n's
            if (!persist_wait(f, f.arrive0 + (u64)(stop_n + 2) * G, f.done0, verdict)) return;
            double *gz0 = a0.ghist + (size_t)((stop_n - 1) % 3) * Cfg::NBIN + L.boff, *gz1 = a0.ghist + (size_t)(stop_n % 3) * Cfg::NBIN + L.boff;
            for (int i = tid; i < N; i += T) gz0[i] = gz1[i] = 0.0;
            return;
        }
        // the last turn's histogram buffer: zeroed once everybody has read it
        if (!persist_wait(f, f.arrive0 + (u64)(f.niter + 1) * G, f.done0, verdict)) return;
        double *gz = a0.ghist + (size_t)((f.niter - 1) % 3) * Cfg::NBIN + L.boff;
        for (int i = tid; i < N; i += T) gz[i] = 0.0;
        return;
    }
    // ---- a sampling workgroup
    for (int i = tid; i <= N; i += T) gcur[i] = f.t.edges[L.eoff + i]; // this workgroup's copy of the map
    for (int it = 0; it < f.niter; ++it) {
        BatchArgs a = a0;
        a.iteration = a0.iteration + (u32)it;
        a.edges = gcur - L.eoff;                              // (LDS through the generic address space: stage_tables reads it once)
        a.part_cols = a0.part_cols + (size_t)(it & 1) * rows;
        a.ghist = a0.ghist + (size_t)(it % 3) * Cfg::NBIN;
        if (tid == 0) *reinterpret_cast<int *>(flags) = 0; // train_leaf's `bad`
        __syncthreads(); // (gcur complete; the previous turn's scratch is free)
        vegas_batch<Cfg, false>(a); // pair table <- gcur, samples, partial row, histogram atomics
        __syncthreads();
        persist_signal(&f.ctr[0], 1ull);
        // all G rows and histograms of this turn are out; the statistics workgroup is through with the turn before (its rows, the
        // histogram buffer it zeroed -- and its verdict)
        if (!persist_wait(f, f.arrive0 + (u64)(it + 1) * G, f.done0 + (u64)it, verdict)) return;
        // the verdicts of turns < it are in; one for this turn may or may not be and is left for the next turn (the header's invariant)
        const u64 word = __hip_atomic_load(&f.ctr[kPersistStopWord], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (word > f.done0 && word - f.done0 <= (u64)it) break; // this turn's samples are discarded: no refinement
        const double *gh = a.ghist + L.boff;
        int hbad = 0; // train!'s checks of the histogram ride along (train_leaf(..., checked = true)); `bad` was cleared before the arrive
        for (int base = 0; base < N; base += kTrainQ * T) { // merge_hist_bin: clearStatistics! offsets + what the workgroups added
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
                    const double h = (double)(f.m.nblocks + 1) * 1.0e-10 + v[q];
                    hl[i] = h;
                    if (!isfinite(h)) hbad |= ST_HIST_NONFINITE;      // variable.jl:212
                    else if (!(h > 0.0)) hbad |= ST_HIST_NONPOSITIVE; // variable.jl:213 / common.jl:71
                }
            }
        }
        if (hbad) atomicOr(reinterpret_cast<int *>(flags), hbad);
        __syncthreads();
        if (train) train_leaf(L, hl, nullptr, sm, ps, *reinterpret_cast<int *>(flags), flags[1], gcur - L.eoff, f.t.dacc, f.t.ddist, 0, f.t.status, false, nullptr, true);
        __syncthreads();
    }
    __syncthreads();
    persist_signal(&f.ctr[0], 1ull); // "through with the last turn's histogram": the statistics workgroup zeroes it
    if (wg == 0 && train)
        for (int i = tid; i <= N; i += T) f.t.edges[L.eoff + i] = gcur[i]; // the refined map, for the host and the next launch
}

} // namespace mci
