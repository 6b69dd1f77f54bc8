// mci_sweep_strat.h -- stratified (VEGAS+) points in batched :vegas parameter sweeps: P independent stratified integrate() loops in ONE
// launch (mci_integrate_sweep_strat).  Compiled by hiprtc next to mci_device.h, mci_strat.h, mci_train.h and mci_sweep_common.h into a translation unit of its
// own (mci_jit.h kUnitSweepStrat): the classic, persistent, stratified, sweep and sweep-leaves code objects stay what they were.  Free of
// host / std headers.
//
// As in mci_sweep.h one workgroup owns a point and runs its whole loop; what the ordinary stratified call spreads over a grid -- the
// three-phase allocation, the chunks' partial rows and boundary records, the one-workgroup reduce -- collapses into that workgroup:
//
//     workgroup g   for p = g, g + G, ...:   map of point p -> LDS;  for every iteration:
//                   allocation (mci_strat.h strat_alloc_*: the tiles of k_strat_alloc walked in order) -> off[p]
//                   the chunks of S samples in order (strat_trip: the trip of vegas_strat): a hypercube that ends in a chunk adds its
//                   V / n_h S1 | V^2 s^2 / n_h to the iteration's running sums and writes d_h; the one a chunk end cuts keeps its S1 | S2
//                   in LDS and seeds slot 0 of the next chunk
//                   flush_workgroup (one row, histogram atomics into this point's row) -> merge_stats -> log row, its head overwritten
//                   with the stratified mean | var -> histogram with the clearStatistics! offsets -> train! on the LDS map (train_leaf)
//                   at the end the map -> maps_out[p]; d[p] and off[p] stay in the sweep's buffer for the host
//
// The synchronisation is mci_sweep_common.h's, with the grid's slice at boff = 0 (bin i belongs to thread i % T); every loop's trip count
// is a kernel argument or bounded by one.  What this unit adds to the traffic through global memory inside a point -- off, d, the tile
// bases -- is likewise written and read by the SAME workgroup with a sweep_round_trip() between the two sides.
#pragma once
#include "mci_strat.h"
#include "mci_sweep_common.h"

namespace mci {

struct SweepStratArgs {
    SweepHead h;           // m: nblocks = 1, one partial row per point; map_off: LDS behind both the sample carve (+ strat_lds_doubles)
                           // and the refinement's scratch: the map [N + 2] | flags [4] | the iteration's running sums [2 kStratMaxCols] |
                           // the cut hypercube's S1 | S2 [2 kStratMaxCols]
    StratArgs st;          // of point 0: off [npoint][ncube + 1], dnext [npoint][ncube]; chunk = S, nchunk, nloc, beta, the cell decode;
                           // part / rec_* / dump_* unused (NULL)
    int have_d;            // d rows were filled by the host (d_in): every allocation is made from them
    int start_uniform;     // the first iteration of a point without d_in samples every hypercube alike
    int mblocks;           // the blocks the ordinary stratified call merges this N and block as: (mblocks + 1) 1e-10 per histogram bin
    int ntile;             // strat_alloc_ntile(ncube)
    double *tbase;         // [npoint][ntile] allocation scratch: the tile bases
};

// the allocation of point-local d -> off, by one workgroup of 256 threads; part: 256 doubles of LDS, bc: 2 doubles of LDS
__device__ __forceinline__ void sweep_strat_alloc(const double *d, long long *off, double *tbase, long long ncube, long long nsamp, int ntile, int ask_uniform,
                                                  double *part, double *bc) {
    const int tid = threadIdx.x;
    long long lo, hi;
    if (tid == 0) off[0] = 0;
    double base = 0.0; // (thread 0: the tiles before this one, added in order)
    if (!ask_uniform)
        for (int g = 0; g < ntile; ++g) {
            strat_alloc_stretch(ncube, ntile, g, tid, lo, hi);
            part[tid] = strat_alloc_stretch_sum(d, lo, hi);
            __syncthreads();
            if (tid == 0) {
                tbase[g] = base;
                base += strat_alloc_base(part, 256);
            }
            __syncthreads();
        }
    if (tid == 0) {
        bc[0] = base;
        bc[1] = strat_alloc_uniform(ask_uniform, base) ? 1.0 : 0.0;
    }
    sweep_round_trip(); // (tbase, bc)
    const double total = bc[0];
    const bool uniform = bc[1] != 0.0;
    for (int g = 0; g < ntile; ++g) {
        strat_alloc_stretch(ncube, ntile, g, tid, lo, hi);
        double sbase = 0.0, tb = 0.0;
        if (!uniform) {
            part[tid] = strat_alloc_stretch_sum(d, lo, hi);
            __syncthreads();
            sbase = strat_alloc_base(part, tid);
            tb = tbase[g];
        }
        strat_alloc_offsets(d, off, ncube, nsamp, lo, hi, uniform ? 1 : 0, sbase, tb, total);
        if (!uniform) __syncthreads(); // (part is written again for the next tile)
    }
    sweep_round_trip(); // (off)
}

template <class Cfg> __device__ __forceinline__ void vegas_sweep_strat(const BatchArgs &a0, const SweepStratArgs &fs) {
    static_assert(Cfg::NLEAF == 1 && Cfg::leaf_kind(0) == 0 && Cfg::NTILE == 1, "a sweep point refines ONE Continuous grid in one tile (the host checks)");
    static_assert(Cfg::CUSTOM_MEASURE == 0 && Cfg::HOST_INTEGRAND == 0 && Cfg::HOST_MEASURE == 0, "stratified :vegas: device integrand, default measure");
    static_assert(Cfg::NDRAW <= kStratMaxDraw && Cfg::NW <= kStratMaxCols, "stratified :vegas: draws / columns");
    static_assert(Mode<Cfg>::HIST_LDS && Cfg::HCOPY == 1 && Cfg::DET == 0, "the point's histogram sits in LDS, one copy");
    static_assert(Cfg::NOBS == Cfg::NW, "default measure: one observable per weight column (row[k] = mean, row[nobs + k] = var)");
    const SweepHead &f = fs.h;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    using LD = Lds<Cfg>;
    constexpr int NW = Cfg::NW, N = Cfg::leaf_nbin(0);
    constexpr int DPC = Cfg::RNG_BITS == 32 ? 4 : 2;
    const int tid = threadIdx.x, T = blockDim.x;
    // the refinement's view of the LDS (vegas_sweep) ...
    double *sm = smem, *hl = sm + train_lds_doubles(N), *ps = hl + N, *gcur = smem + f.map_off, *flags = gcur + N + 2;
    double *tot = flags + 4, *cut = tot + 2 * kStratMaxCols;
    int *bad = reinterpret_cast<int *>(flags);
    // ... and the sample loop's (vegas_strat)
    double *sE = smem + LD::E, *sDA = smem + LD::DA, *sDD = smem + LD::DD, *sH = smem + LD::H, *sO = smem + LD::O;
    long long *sOff = reinterpret_cast<long long *>(smem + LD::END);
    double *sS = smem + LD::END + fs.st.nloc + 1;
    int *sLane = reinterpret_cast<int *>(sS + fs.st.nloc * 2 * NW);
    double *sV = sS + fs.st.nloc * 2 * NW + T;
    const LeafDev L = f.t.leaves[0];
    const bool train = f.t.do_train && L.adapt; // variable.jl:208
    const long long ncube = fs.st.ncube, nsamp = fs.st.nsamp;
    const double V = 1.0 / (double)ncube;
    for (int p = (int)blockIdx.x; p < f.npoint; p += (int)gridDim.x) {
        __syncthreads(); // (the point before: its last LDS reads are through)
        const double *g0 = f.maps_in ? f.maps_in + (size_t)p * (N + 1) : f.t.edges + L.eoff;
        for (int i = tid; i <= N; i += T) gcur[i] = g0[i];
        MergeArgs m;
        BatchArgs a;
        sweep_point<Cfg>(f, a0, p, 1, m, a); // (one partial row per point)
        a.edges = gcur - L.eoff; // (LDS through the generic address space: stage_tables reads it once per iteration)
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
            if (it == 0 || f.t.do_train) sweep_strat_alloc(d, off, fs.tbase + (size_t)p * fs.ntile, ncube, nsamp, fs.ntile, it == 0 && !fs.have_d && fs.start_uniform ? 1 : 0, ps, flags + 2);
            // ---- the sample loop's tables from the map, empty histogram and sums
            if (tid == 0) *bad = 0;
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
            // ---- the histogram row: clearStatistics! offsets + what the chunks added; zero again for the next iteration
            sweep_take_hist(m.ghist + L.boff, hl, N, tid, (double)(fs.mblocks + 1) * 1.0e-10, bad);
            sweep_round_trip(); // (hl, the verdict, d; the zeroed row is out before the next iteration adds to it)
            if (train) train_leaf(L, hl, nullptr, sm, ps, *bad, flags[1], gcur - L.eoff, f.t.dacc, f.t.ddist, 0, m.status, false, nullptr, true);
            __syncthreads();
        }
        for (int i = tid; i <= N; i += T) f.maps_out[(size_t)p * (N + 1) + i] = gcur[i];
    }
}

} // namespace mci
