// mci_sweep_strat_leaves.h -- stratified (VEGAS+) points in batched :vegas parameter sweeps of problems with SEVERAL Continuous variable
// leaves (the opt-in mci_set_sweep_strat_leaves(prob, MCI_SWEEP_ALL_LEAVES)): vegas_sweep_strat of mci_sweep_strat.h with the map
// handling of vegas_sweep_leaves (mci_sweep_leaves.h).  Compiled by hiprtc next to mci_device.h, mci_strat.h, mci_train.h,
// mci_sweep_common.h and mci_sweep_strat.h (SweepStratArgs, sweep_strat_alloc: included, not changed) into a translation unit of its own
// (mci_jit.h kUnitSweepStratLeaves): the one-grid stratified sweep unit and every other code object stay what they were.  Free of host /
// std headers.
//
//     workgroup g   for p = g, g + G, ...:   map of point p (every grid) -> LDS;  for every iteration:
//                   allocation (sweep_strat_alloc) -> off[p]
//                   the chunks of S samples in order (strat_trip), the cut hypercube carried in LDS from chunk to chunk, d_h written
//                   flush_workgroup -> merge_stats -> log row, its head overwritten with the stratified mean | var
//                   leaf by leaf: the histogram slice with the clearStatistics! offsets -> train! on the leaf's part of the LDS map
//                   at the end the map -> maps_out[p]; d[p] and off[p] stay in the sweep's buffer for the host
//
// The synchronisation is mci_sweep_common.h's in its general form (a leaf's slice [boff, boff + nbin) is read and zeroed by the thread
// whose index is (boff + i) % T for bin boff + i); every global store the workgroup reads again stands behind a sweep_round_trip().
//
// LDS.  The front of the segment is shared by the sample carve (Lds<Cfg> + strat_lds_doubles) and the refinement's scratch for the
// largest leaf; each is dead while the other runs.  Behind both, at map_off: the map block (SweepBlock: edges | dacc | ddist |
// flags[4]) | the iteration's running sums and the cut hypercube's sums [4 kStratMaxCols] | the two doubles sweep_strat_alloc
// broadcasts through.  flags[0] holds the two verdict words (even and odd leaves, alternating as in vegas_sweep_leaves), flags[2] is
// train_leaf's spare word; the broadcast pair lies behind the sums, so it meets neither.  The host's sweep_strat_leaves_lds lays out the same.
#pragma once
#include "mci_sweep_strat.h"

namespace mci {

template <class Cfg> constexpr bool sweep_all_continuous() {
    for (int k = 0; k < Cfg::NLEAF; ++k)
        if (Cfg::leaf_kind(k) != 0) return false;
    return true;
}

template <class Cfg> __device__ __forceinline__ void vegas_sweep_strat_leaves(const BatchArgs &a0, const SweepStratArgs &fs) {
    static_assert(Cfg::NLEAF >= 1 && sweep_all_continuous<Cfg>(), "a stratified sweep point refines Continuous grids only (the host checks)");
    static_assert(Cfg::NTILE == 1 && Cfg::TABLE_MODE == 0 && Cfg::HCOPY == 1 && Cfg::DET == 0 && Cfg::EC_DOUBLES == 0,
                  "a sweep point keeps its tables and one histogram tile in LDS (the host checks)");
    static_assert(Cfg::CUSTOM_MEASURE == 0 && Cfg::HOST_INTEGRAND == 0 && Cfg::HOST_MEASURE == 0, "stratified :vegas: device integrand, default measure");
    static_assert(Cfg::NDRAW <= kStratMaxDraw && Cfg::NW <= kStratMaxCols, "stratified :vegas: draws / columns");
    static_assert(Mode<Cfg>::HIST_LDS, "the point's histogram sits in LDS, one copy");
    static_assert(Cfg::NOBS == Cfg::NW, "default measure: one observable per weight column (row[k] = mean, row[nobs + k] = var)");
    const SweepHead &f = fs.h;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    using LD = Lds<Cfg>;
    using B = SweepBlock<Cfg>;
    constexpr int NW = Cfg::NW, MAXN = sweep_max_nbin<Cfg>(), NROW = sweep_row_off<Cfg>(Cfg::NLEAF);
    constexpr int DPC = Cfg::RNG_BITS == 32 ? 4 : 2;
    const int tid = threadIdx.x, T = blockDim.x;
    // the refinement's view of the LDS (vegas_sweep_leaves) ...
    double *sm = smem, *hl = sm + train_lds_doubles(MAXN), *ps = hl + MAXN, *blk = smem + f.map_off;
    double *bedges = blk + B::E, *bdacc = blk + B::DA, *bddist = blk + B::DD, *flags = blk + B::FLAGS;
    double *tot = blk + B::END, *cut = tot + 2 * kStratMaxCols, *bc = cut + 2 * kStratMaxCols;
    int *bad = reinterpret_cast<int *>(flags); // bad[0], bad[1]: the verdicts of the even and the odd leaves; flags[2]: train_leaf's spare word
    // ... and the sample loop's (vegas_strat)
    double *sE = smem + LD::E, *sDA = smem + LD::DA, *sDD = smem + LD::DD, *sH = smem + LD::H, *sO = smem + LD::O;
    long long *sOff = reinterpret_cast<long long *>(smem + LD::END);
    double *sS = smem + LD::END + fs.st.nloc + 1;
    int *sLane = reinterpret_cast<int *>(sS + fs.st.nloc * 2 * NW);
    double *sV = sS + fs.st.nloc * 2 * NW + T;
    const long long ncube = fs.st.ncube, nsamp = fs.st.nsamp;
    const double V = 1.0 / (double)ncube;
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
        sweep_point<Cfg>(f, a0, p, 1, m, a); // (one partial row per point)
        a.edges = bedges; // (LDS through the generic address space: stage_tables reads the three tables once per iteration)
        a.dacc = bdacc;
        a.ddist = bddist;
        StratArgs st = fs.st;
        long long *off = const_cast<long long *>(fs.st.off) + (size_t)p * (size_t)(ncube + 1);
        double *d = fs.st.dnext + (size_t)p * (size_t)ncube;
        st.off = off;
        st.dnext = d;
        const RoundKeys<false> keys = make_round_keys<false>((u32)a.seed, (u32)(a.seed >> 32));
        for (int it = 0; it < f.niter; ++it) {
            a.iteration = a0.iteration + (u32)it;
            __syncthreads(); // (map complete; the refinement of the iteration before has read its scratch)
            // ---- allocation: uniform at a fresh start, from d where one was given or measured; adapt off: the first one stays
            if (it == 0 || f.t.do_train) sweep_strat_alloc(d, off, fs.tbase + (size_t)p * fs.ntile, ncube, nsamp, fs.ntile, it == 0 && !fs.have_d && fs.start_uniform ? 1 : 0, ps, bc);
            // ---- the sample loop's tables from the map block, empty histogram and sums
            if (tid == 0) bad[0] = 0;
            stage_tables<Cfg>(a.edges, a.dacc, a.ddist, sE, sDA, sDD);
            for (int i = tid; i < Cfg::HTILE * Cfg::HCOPY; i += T) sH[i] = 0.0;
            for (int i = tid; i < Cfg::NOBS * ocopy<Cfg>(); i += T) sO[i] = 0.0;
            for (int i = tid; i < 4 * kStratMaxCols; i += T) tot[i] = 0.0; // (tot | cut)
            __syncthreads();
            Tables<Cfg> t;
            t.EC = nullptr;
            if constexpr (Mode<Cfg>::EDGE_LDS) t.E = sE;
            else t.E = a.edges;
            t.DA = sDA;
            t.DD = sDD;
            const u32 stream = a.iteration * 8u + STREAM_VEGAS;
            double acc[NW];
            static_for<0, NW>([&](auto I) { acc[decltype(I)::value] = 0.0; });
            double extra[Cfg::NCOLS - Cfg::NOBS];
            static_for<0, Cfg::NCOLS - Cfg::NOBS>([&](auto I) { extra[decltype(I)::value] = 0.0; });
            long long hcut = -1; // the hypercube the chunk before left cut (its S1 | S2 in `cut`)
            for (long long chunk = 0; chunk < st.nchunk; ++chunk) {
                const long long c0 = chunk * st.chunk, c1 = c0 + st.chunk < nsamp ? c0 + st.chunk : nsamp;
                long long lo = 0, hi = ncube - 1; // largest h with off[h] <= c0
                while (lo < hi) {
                    const long long mm = (lo + hi + 1) >> 1;
                    if (off[mm] <= c0) lo = mm;
                    else hi = mm - 1;
                }
                const long long hfirst = lo;
                hi = ncube - 1; // largest h with off[h] <= c1 - 1
                while (lo < hi) {
                    const long long mm = (lo + hi + 1) >> 1;
                    if (off[mm] <= c1 - 1) lo = mm;
                    else hi = mm - 1;
                }
                int nl = (int)(lo - hfirst + 1); // <= chunk / 2 + 1 = st.nloc while every n_h >= 2
                if (nl > st.nloc) nl = st.nloc;  // (never taken with a valid allocation: keeps the LDS carve whatever the offsets say)
                for (int j = tid; j <= nl; j += T) sOff[j] = off[hfirst + j];
                const bool seeded = hcut == hfirst;
                for (int j = tid; j < nl * 2 * NW; j += T) sS[j] = (seeded && j < 2 * NW) ? cut[j] : 0.0;
                __syncthreads();
                for (long long base = c0; base < c1; base += T) strat_trip<Cfg, DPC>(a, st, t, keys, stream, base, c1, hfirst, nl, sOff, sS, sLane, sV, sH, acc, extra);
                // the hypercubes that end in this chunk -> running sums + d_h; the one the chunk end cuts -> `cut`
                double pm[2 * NW];
                static_for<0, 2 * NW>([&](auto Q) { pm[decltype(Q)::value] = 0.0; });
                for (int j = tid; j < nl; j += T) {
                    const long long o0 = sOff[j], o1 = sOff[j + 1];
                    const double n = (double)(o1 - o0);
                    const double *sj = sS + j * 2 * NW;
                    if (o1 <= c1) {
                        double ssum = 0.0;
                        static_for<0, NW>([&](auto Q) {
                            constexpr int qq = decltype(Q)::value;
                            const double v2 = strat_s2(sj[qq], sj[NW + qq], n);
                            pm[qq] += V / n * sj[qq];
                            pm[NW + qq] += V * V * v2 / n;
                            ssum += v2;
                        });
                        d[hfirst + j] = strat_damp(ssum, st.beta);
                    } else if (j == nl - 1) {
                        static_for<0, 2 * NW>([&](auto Q) { cut[decltype(Q)::value] = sj[decltype(Q)::value]; });
                    }
                }
                hcut = sOff[nl] > c1 ? hfirst + nl - 1 : -1;
                // per-lane sums -> LDS -> one lane per column adds them in lane order onto the iteration's running sum
                static_for<0, 2 * NW>([&](auto Q) { sV[decltype(Q)::value * T + tid] = pm[decltype(Q)::value]; });
                __syncthreads();
                if (tid < 2 * NW) {
                    double v = 0.0;
                    for (int u = 0; u < T; ++u) v += sV[tid * T + u];
                    tot[tid] += v;
                }
                __syncthreads();
            }
            // ---- statistics: the one partial row + histogram atomics, the head as merge_stats leaves it, the stratified mean | var over it
            flush_workgroup<Cfg, LD>(a, smem, acc, extra, (i64)0, 0);
            sweep_round_trip();
            merge_stats(m); // (one block of one row)
            __syncthreads(); // the head of `packed` was written by this workgroup
            const TrainArgs tr = sweep_log_row(f, p, it);
            iteration_bookkeeping(tr);
            if (tid < 2 * NW) tr.iter_log_row[tid < NW ? tid : Cfg::NOBS + (tid - NW)] = tot[tid]; // (the thread that copied this entry: program order)
            // ---- leaf by leaf: the histogram slice, train! on the leaf's part of the LDS map
#pragma unroll 1
            for (int l = 0; l < Cfg::NLEAF; ++l) {
                const LeafDev L = f.t.leaves[l];
                const int N = L.nbin;
                const bool train = f.t.do_train && L.adapt; // variable.jl:208
                int *verdict = bad + (l & 1);
                if (tid == 0) bad[(l + 1) & 1] = 0; // (the next leaf's; its last reader passed the barrier that closed the leaf before this one)
                // clearStatistics! offsets + what the chunks added; the slice is zero again for the next iteration
                // (this thread's first bin of the slice: (boff + first) % T == tid)
                sweep_take_hist(m.ghist + L.boff, hl, N, (tid + T - L.boff % T) % T, (double)(fs.mblocks + 1) * 1.0e-10, verdict);
                sweep_round_trip(); // (hl, the verdict, d; the zeroed slice is out before the next iteration adds to it)
                if (train) train_leaf(L, hl, nullptr, sm, ps, *verdict, flags[2], bedges, bdacc, bddist, 0, m.status, false, nullptr, true);
                __syncthreads();
            }
        }
        sweep_copy_row<Cfg, true>(blk, f.maps_out + (size_t)p * NROW, nullptr);
    }
}

} // namespace mci
