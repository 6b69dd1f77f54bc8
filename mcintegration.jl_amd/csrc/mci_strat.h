// mci_strat.h -- the stratified :vegas sample kernel (VEGAS+ adaptive stratified sampling; Lepage, J. Comput. Phys. 439 (2021) 110386).
// Compiled by hiprtc next to mci_device.h into a translation unit of its own (mci_jit.h kUnitStrat): the unit of a problem without
// stratification is not touched.  Free of host / std headers.
//
// y-space is cut into ncube = prod nstrat[d] hypercubes, hypercube h = sum_d i_d * prod_{d' < d} nstrat[d'] (draw 0 fastest), and the
// N samples of an iteration are allocated to them: hypercube h owns the global samples off[h] <= s < off[h + 1], n_h >= 2 of them
// (k_strat_alloc, mci_static_kernels.h).  Sample s draws the uniforms classic :vegas draws for sample s (same Philox stream and counter)
// and moves them into its cell, y_d = (i_d + u_d) * (1 / nstrat[d]); everything behind the draw -- map, integrand, LDS histogram -- is
// mci_device.h's.  Per sample: Jacobian jac * r_h with r_h = N / (ncube n_h); histogram weight (|w| jac)^2 r_h.
//
// A workgroup runs chunks of S consecutive samples (chunk c = blockIdx.x + k * gridDim.x).  Since n_h >= 2 a chunk touches at most
// S/2 + 1 hypercubes; their offsets are staged in LDS, a lane finds its hypercube by bisection there.  Sums of f J and (f J)^2 per
// hypercube and column are kept in LDS: after every trip of T samples the first lane of each run of equal hypercubes (samples of one
// hypercube sit in consecutive lanes) adds the run up in lane order -- fixed order, no atomics.  At the end of a chunk the hypercubes
// wholly inside it give their share of (mean, var) to the chunk's partial row and write their d_h; the (at most two) hypercubes the chunk
// boundary cuts leave their partial sums in the chunk's two boundary records, which k_strat_reduce folds in chunk order.
#pragma once

namespace mci {

enum { kStratMaxDraw = 32, kStratMaxCols = 8 };

struct StratArgs {
    const long long *off;   // [ncube + 1] first sample of every hypercube (off[ncube] = nsamp)
    double *dnext;          // [ncube] out: d_h of the next allocation (the interior hypercubes of a chunk; the cut ones: k_strat_reduce)
    double *part;           // [nchunk][2 * NW] out: sum over the chunk's interior hypercubes of  V / n_h * S1  |  V^2 s^2 / n_h
    long long *rec_h;       // [nchunk][2] out: hypercube of the chunk's leading | trailing boundary record, -1 = none
    double *rec_s;          // [nchunk][2][2 * NW] out: its partial S1 | S2
    long long ncube, nsamp, chunk, nchunk, first_index; // first_index: Philox counter of sample 0
    int nloc;               // LDS room for the hypercubes of one chunk (chunk / 2 + 1)
    double beta;
    unsigned magic[kStratMaxDraw]; // h / nstrat[d] = (h * magic[d]) >> shift[d], exact for h < 2^31 (Granlund-Montgomery)
    int shift[kStratMaxDraw];
    int nstrat[kStratMaxDraw];
    double inv[kStratMaxDraw];     // 1 / nstrat[d]
    // test hook (mci_debug_strat_dump): per sample x [nsamp][NDRAW], y [nsamp][NDRAW], h, jac, w [nsamp][NW]; NULL = off
    double *dump_x, *dump_y, *dump_jac, *dump_w;
    long long *dump_h;
};

// The allocation rule of k_strat_alloc (mci_static_kernels.h) and of the stratified sweep (mci_sweep_strat.h), per tile and thread: the
// hypercubes are cut into ntile tiles, a tile into 256 stretches; P_h = tile base + (stretch base + running sum), every base the
// sequential sum of what lies before it; C_h = M P_h / P (M = N - 2 ncube), off[h + 1] = 2 (h + 1) + floor(C_h), the last C_h := M.
// C_h is rounded as (M P_h) / P; only where that product leaves the double range it is M (P_h / P), so that a finite total always gives
// an allocation in proportion and every input whose product is finite keeps its bits.
// k_strat_alloc takes the tile from blockIdx.x, the sweep's one workgroup walks the tiles in order.
// >>> strat alloc rule (compiled for the host by tests/test_sweep_strat_host.py)
__host__ __device__ inline int strat_alloc_ntile(long long ncube) { return (int)((ncube + 255) / 256 < 1024 ? (ncube + 255) / 256 : 1024); }
// the hypercubes [lo, hi) of thread tid of 256 in tile `tile` of ntile
__host__ __device__ inline void strat_alloc_stretch(long long ncube, int ntile, int tile, int tid, long long &lo, long long &hi) {
    const long long tl = (ncube + ntile - 1) / ntile, t0 = (long long)tile * tl, t1 = t0 + tl < ncube ? t0 + tl : ncube;
    const long long per = (t1 - t0 + 255) / 256;
    lo = t0 + (long long)tid * per;
    if (lo > t1) lo = t1;
    hi = lo + per < t1 ? lo + per : t1;
}
__host__ __device__ inline double strat_alloc_stretch_sum(const double *d, long long lo, long long hi) {
    double mine = 0.0;
    for (long long h = lo; h < hi; ++h) mine += d[h];
    return mine;
}
// 256 stretch sums of a tile -> the tile's sum | the base of stretch tid: added in stretch order
__host__ __device__ inline double strat_alloc_base(const double *part, int tid) {
    double s = 0.0;
    for (int t = 0; t < tid; ++t) s += part[t];
    return s;
}
// d_h = 1 whatever d holds: asked for, or a total that is 0 or not finite
__host__ __device__ inline int strat_alloc_uniform(int asked, double total) { return (asked || !(total > 0.0) || !(total - total == 0.0)) ? 1 : 0; }
// off[h + 1] for the hypercubes [lo, hi) of one stretch; sbase / tbase / total are not read when uniform
__host__ __device__ inline void strat_alloc_offsets(const double *d, long long *off, long long ncube, long long nsamp, long long lo, long long hi, int uniform,
                                                    double sbase, double tbase, double total) {
    const long long M = nsamp - 2 * ncube;
    if (uniform) { // C_h = M (h + 1) / ncube
        for (long long h = lo; h < hi; ++h) {
            double C = (double)M * (double)(h + 1) / (double)ncube;
            if (h == ncube - 1 || C > (double)M) C = (double)M;
            off[h + 1] = 2 * (h + 1) + (long long)floor(C);
        }
        return;
    }
    double run = 0.0;
    for (long long h = lo; h < hi; ++h) {
        run += d[h];
        const double P = tbase + (sbase + run);
        double C = (double)M * P / total;
        if (!(C - C == 0.0)) C = (double)M * (P / total); // M P_h beyond the double range (d_h near 1e305): the quotient first, P_h / P <= 1
        if (h == ncube - 1 || C > (double)M) C = (double)M;
        off[h + 1] = 2 * (h + 1) + (long long)floor(C);
    }
}
// <<< strat alloc rule

// largest y below 1: (i + u) / n rounds to 1.0 for some u < 1 (i = 2, n = 3, u = 1 - 2^-52), and draw_leaf would read bin N
__device__ __forceinline__ double strat_clamp(double y) { return fmin(y, 0x1.fffffffffffffp-1); }

template <class Cfg, bool KV, int DPC> __device__ __forceinline__ void draw_sample_strat(const Tables<Cfg> &t, const RoundKeys<KV> &keys, u32 stream, u64 index,
                                                                                         const StratArgs &st, const int *cell, Sample<Cfg> &s, double *ydump) {
    constexpr unsigned long long ALL = Cfg::NDRAW >= 64 ? ~0ull : ((1ull << Cfg::NDRAW) - 1ull);
    constexpr int NCH = (Cfg::NDRAW + DPC - 1) / DPC;
    const u32 ilo = (u32)index, ihi = (u32)(index >> 32);
    s.jac = 1.0;
    static_for<0, Cfg::NI>([&](auto I) { s.jaci[decltype(I)::value] = 1.0; });
    static_for<0, tdraw_words<Cfg>()>([&](auto J) { s.word[decltype(J)::value] = 0u; });
    static_for<0, NCH>([&](auto C) {
        constexpr int c = decltype(C)::value;
        const u32x4 r = philox4x32_10<KV>(ilo, ihi, (u32)c, stream, keys);
        if constexpr ((DPC * c) % kJacGroup == 0) { // open a group of draws: its N factors, as draw_sample applies them
            constexpr int lo = DPC * c, hi = lo + kJacGroup;
            constexpr double sc = jac_scale_product<Cfg>(ALL, lo, hi);
            if constexpr (sc != 1.0) s.jac *= sc;
            static_for<0, Cfg::NI>([&](auto I) {
                constexpr int i = decltype(I)::value;
                constexpr double si = jac_scale_product<Cfg>(Cfg::own_mask(i), lo, hi);
                if constexpr (Cfg::own_mask(i) != ALL && si != 1.0) s.jaci[i] *= si;
            });
        }
        static_for<0, DPC>([&](auto H) {
            constexpr int k = DPC * c + decltype(H)::value;
            if constexpr (k < Cfg::NDRAW) {
                const double u = block_u12<DPC, decltype(H)::value>(r) - 1.0; // exact: the uniform classic :vegas draws
                const double y = strat_clamp(((double)cell[k] + u) * st.inv[k]);
                if (ydump) ydump[k] = y;
                double raw;
                draw_leaf<Cfg, k, false>(t, y, s.x[k], raw, s.bin[k]);
                s.pj[k] = raw * jac_scale<Cfg>(k);
                s.jac *= raw; // jac /= prob   vegas/montecarlo.jl:126 (scale applied above, in the groups draw_sample applies it in)
                static_for<0, Cfg::NI>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    if constexpr (((Cfg::own_mask(i) >> k) & 1ull) && Cfg::own_mask(i) != ALL) s.jaci[i] *= raw;
                });
            }
        });
    });
    static_for<0, Cfg::NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        if constexpr (Cfg::own_mask(i) == ALL) s.jaci[i] = s.jac;
    });
}

// variance estimate of one hypercube's column from its sums (clamped at 0 against rounding)
__device__ __forceinline__ double strat_s2(double s1, double s2, double n) {
    const double v = (s2 - s1 * s1 / n) / (n - 1.0);
    return v > 0.0 ? v : 0.0;
}

// d_h = (sum_k s^2_{h,k})^(beta / 2) of the next allocation, for every kernel that writes one (the sample kernel's interior hypercubes,
// k_strat_reduce's cut ones, the stratified sweep).  beta = 2 hands the sum through: the device's pow(x, 1.0) is within an ulp of x, not x.
__device__ __forceinline__ double strat_damp(double ssum, double beta) {
    const double a = 0.5 * beta;
    return a == 1.0 ? ssum : pow(ssum, a);
}

// LDS behind the sample kernel's own carve (doubles): offsets [nloc + 1] (int64) | sums [nloc][2 NW] | lane hypercubes [T] (int) |
// lane values / reduction scratch [T][2 NW]
template <class Cfg> constexpr int strat_lds_doubles(int nloc, int T) { return (nloc + 1) + nloc * 2 * Cfg::NW + T + T * 2 * Cfg::NW; }

// One trip of the chunk [c0, c1): the T samples base + tid.  The chunk's hypercubes are hfirst .. hfirst + nl - 1, their offsets staged in
// sOff[nl + 1]; a lane finds its hypercube by bisection there, draws, evaluates, adds to the LDS histogram and to its own acc / extra; then
// the first lane of every run of one hypercube adds the run up, in lane order, into that hypercube's sums sS.  Ends behind a barrier.
// Shared by vegas_strat and the stratified sweep (mci_sweep_strat.h).
template <class Cfg, int DPC> __device__ __forceinline__ void strat_trip(const BatchArgs &a, const StratArgs &st, const Tables<Cfg> &t, const RoundKeys<false> &keys, u32 stream,
                                                                          long long base, long long c1, long long hfirst, int nl, const long long *sOff, double *sS,
                                                                          int *sLane, double *sV, double *sH, double *acc /*[NW]*/, double *extra /*[NCOLS - NOBS]*/) {
    constexpr int NW = Cfg::NW;
    const int tid = threadIdx.x, T = blockDim.x;
    const long long sidx = base + tid;
    const bool valid = sidx < c1;
    int jl = -1;
    if (valid) {
        int l = 0, h = nl - 1; // largest j with sOff[j] <= sidx
        while (l < h) {
            const int m = (l + h + 1) >> 1;
            if (sOff[m] <= sidx) l = m;
            else h = m - 1;
        }
        jl = l;
        const long long hc = hfirst + l;
        const long long nh = sOff[l + 1] - sOff[l];
        const double r = (double)st.nsamp / ((double)st.ncube * (double)nh); // r_h
        int cell[Cfg::NDRAW];
        u32 q = (u32)hc;
        static_for<0, Cfg::NDRAW>([&](auto K) { // mixed radix, draw 0 fastest
            constexpr int k = decltype(K)::value;
            const u32 qn = (u32)(((u64)q * st.magic[k]) >> st.shift[k]);
            cell[k] = (int)(q - qn * (u32)st.nstrat[k]);
            q = qn;
        });
        Sample<Cfg> s;
        double *yd = st.dump_y ? st.dump_y + sidx * Cfg::NDRAW : nullptr;
        draw_sample_strat<Cfg, false, DPC>(t, keys, stream, (u64)(st.first_index + sidx), st, cell, s, yd);
        double w[NW];
        Cfg::integrand(s.x, w, a.ud, -1); // vegas/montecarlo.jl:140-144
        extra[Cols<Cfg>::NEVAL - Cfg::NOBS] += 1.0;
        extra[Cols<Cfg>::NORM - Cfg::NOBS] += 1.0;
        static_for<0, NW>([&](auto Q) {
            constexpr int qq = decltype(Q)::value;
            const double fj = w[qq] * s.jaci[qq / Cfg::NCOMP]; // f J  (vegas/montecarlo.jl:152, J without r_h)
            acc[qq] += fj * r;                                 // the observable: jac * r_h
            sV[tid * NW + qq] = fj;
        });
        double wh[Cfg::NI];
        static_for<0, Cfg::NI>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const double wj = absw<Cfg, i>(w) * s.jac; // vegas/montecarlo.jl:173-174
            wh[i] = wj * wj * r;                       // (|w| jac)^2 r_h: each bin estimates what classic :vegas estimates
        });
        hist_update<Cfg, 0>(s, wh, sH, a.ghist, 0);
        if (st.dump_x) {
            static_for<0, Cfg::NDRAW>([&](auto K) { st.dump_x[sidx * Cfg::NDRAW + decltype(K)::value] = s.x[decltype(K)::value]; });
            static_for<0, NW>([&](auto Q) { st.dump_w[sidx * NW + decltype(Q)::value] = w[decltype(Q)::value]; });
            st.dump_jac[sidx] = s.jac;
            st.dump_h[sidx] = hc;
        }
    }
    sLane[tid] = jl;
    __syncthreads();
    // the first lane of every run of one hypercube adds the run up, in lane order, into that hypercube's LDS sums
    if (valid && (tid == 0 || sLane[tid - 1] != jl)) {
        double s1[NW], s2[NW];
        static_for<0, NW>([&](auto Q) { s1[decltype(Q)::value] = 0.0; s2[decltype(Q)::value] = 0.0; });
        for (int u = tid; u < T && sLane[u] == jl; ++u)
            static_for<0, NW>([&](auto Q) {
                constexpr int qq = decltype(Q)::value;
                const double v = sV[u * NW + qq];
                s1[qq] += v;
                s2[qq] += v * v;
            });
        static_for<0, NW>([&](auto Q) {
            constexpr int qq = decltype(Q)::value;
            sS[jl * 2 * NW + qq] += s1[qq];
            sS[jl * 2 * NW + NW + qq] += s2[qq];
        });
    }
    __syncthreads();
}

template <class Cfg> __device__ __forceinline__ void vegas_strat(const BatchArgs &a, const StratArgs &st) {
    static_assert(Cfg::NTILE == 1 && Cfg::CUSTOM_MEASURE == 0 && Cfg::HOST_INTEGRAND == 0 && Cfg::HOST_MEASURE == 0, "stratified :vegas: one tile, device integrand, default measure");
    static_assert(Cfg::NDRAW <= kStratMaxDraw && Cfg::NW <= kStratMaxCols, "stratified :vegas: draws / columns");
    constexpr int NW = Cfg::NW;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    using L = Lds<Cfg>;
    const int tid = threadIdx.x, T = blockDim.x;
    double *sE = smem + L::E, *sDA = smem + L::DA, *sDD = smem + L::DD, *sH = smem + L::H, *sO = smem + L::O;
    long long *sOff = reinterpret_cast<long long *>(smem + L::END);
    double *sS = smem + L::END + st.nloc + 1;
    int *sLane = reinterpret_cast<int *>(sS + st.nloc * 2 * NW);
    double *sV = sS + st.nloc * 2 * NW + T;
    stage_tables<Cfg>(a.edges, a.dacc, a.ddist, sE, sDA, sDD);
    if constexpr (Mode<Cfg>::HIST_LDS)
        for (int i = tid; i < Cfg::HTILE * Cfg::HCOPY; i += T) sH[i] = 0.0;
    for (int i = tid; i < Cfg::NOBS * ocopy<Cfg>(); i += T) sO[i] = 0.0;
    __syncthreads();
    Tables<Cfg> t;
    t.EC = nullptr;
    if constexpr (Mode<Cfg>::EDGE_LDS) t.E = sE;
    else t.E = a.edges;
    t.DA = sDA;
    t.DD = sDD;

    const u32 stream = a.iteration * 8u + STREAM_VEGAS;
    constexpr int DPC = Cfg::RNG_BITS == 32 ? 4 : 2;
    const RoundKeys<false> keys = make_round_keys<false>((u32)a.seed, (u32)(a.seed >> 32));
    double acc[NW];
    static_for<0, NW>([&](auto I) { acc[decltype(I)::value] = 0.0; });
    double extra[Cfg::NCOLS - Cfg::NOBS];
    static_for<0, Cfg::NCOLS - Cfg::NOBS>([&](auto I) { extra[decltype(I)::value] = 0.0; });
    const double V = 1.0 / (double)st.ncube;

    for (long long chunk = blockIdx.x; chunk < st.nchunk; chunk += gridDim.x) {
        const long long c0 = chunk * st.chunk, c1 = c0 + st.chunk < st.nsamp ? c0 + st.chunk : st.nsamp;
        // first and last hypercube of the chunk: bisection in the global offsets (wave-uniform)
        long long lo = 0, hi = st.ncube - 1; // largest h with off[h] <= c0
        while (lo < hi) {
            const long long m = (lo + hi + 1) >> 1;
            if (st.off[m] <= c0) lo = m;
            else hi = m - 1;
        }
        const long long hfirst = lo;
        hi = st.ncube - 1; // largest h with off[h] <= c1 - 1
        while (lo < hi) {
            const long long m = (lo + hi + 1) >> 1;
            if (st.off[m] <= c1 - 1) lo = m;
            else hi = m - 1;
        }
        int nl = (int)(lo - hfirst + 1); // <= chunk / 2 + 1 = st.nloc while every n_h >= 2 (k_strat_alloc)
        if (nl > st.nloc) nl = st.nloc;  // (never taken with a valid allocation: keeps the LDS carve whatever the offsets say)
        for (int j = tid; j <= nl; j += T) sOff[j] = st.off[hfirst + j];
        for (int j = tid; j < nl * 2 * NW; j += T) sS[j] = 0.0;
        __syncthreads();
        for (long long base = c0; base < c1; base += T) strat_trip<Cfg, DPC>(a, st, t, keys, stream, base, c1, hfirst, nl, sOff, sS, sLane, sV, sH, acc, extra);
        // the chunk's hypercubes: interior ones -> partial row + d_h, cut ones -> boundary records
        double pm[2 * NW];
        static_for<0, 2 * NW>([&](auto Q) { pm[decltype(Q)::value] = 0.0; });
        if (tid == 0) { // leading record: the first hypercube when the chunk cuts it; trailing: the last one when it starts inside and is cut
            st.rec_h[2 * chunk] = (sOff[0] < c0 || sOff[1] > c1) ? hfirst : -1;
            st.rec_h[2 * chunk + 1] = (nl > 1 && sOff[nl] > c1) ? hfirst + nl - 1 : -1;
        }
        for (int j = tid; j < nl; j += T) {
            const long long o0 = sOff[j], o1 = sOff[j + 1];
            const double n = (double)(o1 - o0);
            const double *sj = sS + j * 2 * NW;
            if (o0 >= c0 && o1 <= c1) {
                double ssum = 0.0;
                static_for<0, NW>([&](auto Q) {
                    constexpr int qq = decltype(Q)::value;
                    const double v2 = strat_s2(sj[qq], sj[NW + qq], n);
                    pm[qq] += V / n * sj[qq];
                    pm[NW + qq] += V * V * v2 / n;
                    ssum += v2;
                });
                st.dnext[hfirst + j] = strat_damp(ssum, st.beta);
            } else {
                const int rr = (j == 0) ? 0 : 1; // cut at the chunk's start (or both ends) | at its end
                double *rs = st.rec_s + (2 * chunk + rr) * 2 * NW;
                static_for<0, 2 * NW>([&](auto Q) { rs[decltype(Q)::value] = sj[decltype(Q)::value]; });
            }
        }
        // partial row: per-lane sums -> LDS -> one lane per column adds them in lane order
        static_for<0, 2 * NW>([&](auto Q) { sV[decltype(Q)::value * T + tid] = pm[decltype(Q)::value]; });
        __syncthreads();
        if (tid < 2 * NW) {
            double v = 0.0;
            for (int u = 0; u < T; ++u) v += sV[tid * T + u];
            st.part[chunk * 2 * NW + tid] = v;
        }
        __syncthreads();
    }
    flush_workgroup<Cfg, L>(a, smem, acc, extra, (i64)blockIdx.x, 0);
}

} // namespace mci
