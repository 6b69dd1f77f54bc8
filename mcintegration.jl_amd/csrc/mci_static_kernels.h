// mci_static_kernels.h -- configuration-independent gfx950 kernels, compiled ahead of time by hipcc:
// partial reduction (block merge, reference src/main.jl:273-287, src/configuration.jl:252-262),
// reweighting (src/main.jl:322-346) and grid refinement (src/distribution/variable.jl:206-239,
// :369-382 with src/distribution/common.jl:43-82).  These are O(bins) per iteration; they stay on the
// device so that an iteration is one asynchronous chain  sample -> merge -> all-reduce -> train  with
// no host round trip.
#pragma once
#include <hip/hip_runtime.h>

#include "mci_train.h" // merge / train device functions, ST_* status bits
#include "mci_strat.h" // the allocation rule k_strat_alloc shares with the stratified sweep (strat_alloc_*)

namespace mci {

// stage 1 of the histogram merge: out[g][bin] = sum over this group's workgroups (fixed order)
__global__ void __launch_bounds__(256) k_hist_stage1(const double *__restrict__ part_hist, int nwg, int nbin, int ngroup,
                                                     double *__restrict__ out) {
    const int bin = blockIdx.x * 256 + threadIdx.x;
    const int g = blockIdx.y;
    if (bin >= nbin) return;
    const int per = (nwg + ngroup - 1) / ngroup;
    const int w0 = g * per, w1 = min(nwg, w0 + per);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int w = w0;
    for (; w + 3 < w1; w += 4) {
        s0 += part_hist[(size_t)(w + 0) * nbin + bin];
        s1 += part_hist[(size_t)(w + 1) * nbin + bin];
        s2 += part_hist[(size_t)(w + 2) * nbin + bin];
        s3 += part_hist[(size_t)(w + 3) * nbin + bin];
    }
    for (; w < w1; ++w) s0 += part_hist[(size_t)w * nbin + bin];
    out[(size_t)g * nbin + bin] = (s0 + s1) + (s2 + s3);
}

// host measure: obs[b][o] (accumulated by the host closure over block b's samples) goes into the observable columns of the
// block's first partial row, which the kernel left at zero
__global__ void __launch_bounds__(256) k_add_host_obs(const double *__restrict__ obs, int nblocks, int nobs, int ncols, int wg_per_block,
                                                      double *__restrict__ part_cols) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nblocks * nobs) return;
    const int b = i / nobs, o = i % nobs;
    part_cols[(size_t)b * wg_per_block * ncols + o] += obs[i];
}

__global__ void __launch_bounds__(256) k_finalize(MergeArgs m) {
    const int nhb = (m.nbin + 255) / 256;
    const int hoff = 2 * m.nobs + 2 + m.ni + 1;
    if ((int)blockIdx.x < nhb) {
        const int bin = blockIdx.x * 256 + threadIdx.x;
        if (bin < m.nbin) m.packed[hoff + bin] = merge_hist_bin(m, bin);
        return;
    }
    if ((int)blockIdx.x > nhb) { // grid = nhb + 1 + merge_pa_blocks
        merge_pa(m, (int)blockIdx.x - nhb - 1);
        return;
    }
    merge_stats(m);
}

// Carried chains: which stored chain every chain of the next launch continues -- one workgroup per block runs resample_block
// (mci_train.h: the rule, ResampleArgs and the body, which a sweep point's workgroup runs too, mci_sweep_chains.h).
__global__ void __launch_bounds__(256) k_resample_chains(ResampleArgs a) {
    constexpr int kLdsW = 8192; // stored chains per block whose running weights also sit in LDS: the bisections then read LDS
    __shared__ double scratch[kResampleThreads + kLdsW];
    resample_block(a, (long long)blockIdx.x, scratch, kLdsW);
}

// One workgroup per leaf: Dist.train! then clearStatistics!; workgroup `nleaf`: bookkeeping.
__global__ void __launch_bounds__(512) k_train(TrainArgs a) { // (launched with 256 or 512 threads; the serial walk's lane wants ~200 registers)
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double ps[256]; // block_prefix scratch
    __shared__ int bad;
    __shared__ double ssum;
    if ((int)blockIdx.x == a.nleaf) {
        iteration_bookkeeping(a);
        return;
    }
    if (!a.do_train) return;
    const LeafDev L = a.leaves[blockIdx.x];
    if (!L.adapt) return; // variable.jl:208, :370
    double *h = a.packed + a.nstat + L.boff;
    train_leaf(L, h, h, sm, ps, bad, ssum, a.edges, a.dacc, a.ddist, a.serial_walk, a.status, false, nullptr, false, a.spare ? sm + train_lds_doubles(a.maxn) : nullptr);
}

// Single-rank iterations need no all-reduce between the merge and the refinement: k_finalize and k_train as ONE
// launch.  Workgroup l < nleaf merges its leaf's histogram (second stage) into LDS and `packed`, then trains from
// the LDS copy; workgroup nleaf merges the statistics head, then does the bookkeeping.
__global__ void __launch_bounds__(512) k_finish(MergeArgs m, TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[]; // [train_lds_doubles(maxn)] train scratch | [maxn] merged histogram, then ([train_spare_doubles(maxn)], a.spare) the serial walk's slots
    __shared__ double ps[256];
    __shared__ int bad;
    __shared__ double ssum;
    const int tid = threadIdx.x, T = blockDim.x;
    if ((int)blockIdx.x == a.nleaf) {
        merge_stats(m);
        __syncthreads(); // the head of `packed` was written by this workgroup
        iteration_bookkeeping(a);
        return;
    }
    if ((int)blockIdx.x > a.nleaf) { // grid = nleaf + 1 + merge_pa_blocks
        merge_pa(m, (int)blockIdx.x - a.nleaf - 1);
        return;
    }
    const LeafDev L = a.leaves[blockIdx.x];
    double *hl = sm + train_lds_doubles(a.maxn);
    double *hp = a.packed + a.nstat + L.boff;
    const bool train = a.do_train && L.adapt;
    if (train) train_stage_grid(L, sm, a.edges); // (the old grid's loads fly together with the histogram's)
    for (int i = tid; i < L.nbin; i += T) {
        const double v = merge_hist_bin(m, L.boff + i);
        hl[i] = v;
        hp[i] = v;
    }
    __syncthreads();
    if (!train) return;
    train_leaf(L, hl, hp, sm, ps, bad, ssum, a.edges, a.dacc, a.ddist, a.serial_walk, a.status, true, nullptr, false, a.spare ? hl : nullptr); // (hl: free once smoothed)
}

// =============================================================================================
// Stratified :vegas (VEGAS+ hypercube redistribution, mci_strat.h): allocation and the iteration's statistics
// =============================================================================================
// k_strat_alloc: damped weights d_h -> sample offsets o_h.  C_h = M * P_h / P (M = N - 2 ncube, P_h = sum_{j <= h} d_j, P = P_{ncube-1}),
// n_h = 2 + floor(C_h) - floor(C_{h-1}), o_h = 2 h + floor(C_{h-1}), C_{ncube-1} := M.  The prefix is formed in a fixed order -- every
// thread adds its stretch of a tile sequentially, the stretches of a tile and the tiles are chained sequentially -- as
// P_h = tile base + (stretch base + run), which is monotone in h (the addends are non-negative and every base is the exact sum the
// stretch or tile before it ends on), so n_h >= 2 holds in floating point.  Three launches: phase 0 (ntile workgroups) tile sums, phase 1
// (one workgroup) tile bases, total and the decision "uniform" (first iteration of a call, or a total that is 0 or not finite: d_h = 1),
// phase 2 (ntile workgroups) the offsets.  d_h is not range-checked: a total that is finite allocates in proportion however large the
// d_h are (M P_h overflowing is recomputed as M (P_h / P), strat_alloc_offsets), one that is 0, inf or NaN allocates uniformly.
struct StratAllocArgs {
    const double *d;        // [ncube]
    long long *off;         // [ncube + 1] out
    double *tsum;           // [2 * ntile + 2] scratch: tile sums | tile bases | total | uniform flag
    long long ncube, nsamp;
    int ntile;
    int uniform;            // 1: d_h = 1 whatever d holds
};
// The arithmetic per tile and thread is mci_strat.h's allocation rule (strat_alloc_*), which the stratified sweep's one workgroup walks
// tile by tile (mci_sweep_strat.h); here blockIdx.x selects the tile.
__global__ void __launch_bounds__(256) k_strat_alloc(StratAllocArgs a, int phase) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    if (phase == 1) {
        if (tid != 0) return;
        double base = 0.0;
        for (int g = 0; g < a.ntile; ++g) {
            a.tsum[a.ntile + g] = base;
            base += a.tsum[g];
        }
        a.tsum[2 * a.ntile] = base;
        a.tsum[2 * a.ntile + 1] = strat_alloc_uniform(a.uniform, base) ? 1.0 : 0.0;
        return;
    }
    long long lo, hi;
    strat_alloc_stretch(a.ncube, a.ntile, (int)blockIdx.x, tid, lo, hi);
    const bool uniform = phase == 2 && a.tsum[2 * a.ntile + 1] != 0.0;
    part[tid] = uniform ? 0.0 : strat_alloc_stretch_sum(a.d, lo, hi);
    __syncthreads();
    if (phase == 0) {
        if (tid == 0) a.tsum[blockIdx.x] = strat_alloc_base(part, 256);
        return;
    }
    if (blockIdx.x == 0 && tid == 0) a.off[0] = 0;
    // (this thread's stretch base within the tile: the stretches before it, added in order)
    const double sbase = uniform ? 0.0 : strat_alloc_base(part, tid);
    strat_alloc_offsets(a.d, a.off, a.ncube, a.nsamp, lo, hi, uniform ? 1 : 0, sbase, a.tsum[a.ntile + blockIdx.x], a.tsum[2 * a.ntile]);
}

// k_strat_remap: a carried d_h (mci_set_stratification_carry) moved from the plan it was measured on to another plan of the same
// draws, and from the beta it was measured under to another: d'[h'] = d[h]^e, e = beta_new / beta_old, h = the old hypercube that holds
// the CENTRE of new hypercube h'.  Per draw, new cell j of n' sits in old cell i = floor((2 j + 1) n / (2 n')) of n -- integers only, so
// a centre that falls on an old cell's edge (n = 2, n' = 3, j = 1: 6 / 6 -> 1, the upper cell) is decided the same way on every machine.  The values
// are NOT rescaled by the refinement factor: the allocation is proportional to d_h / sum d, and copying a parent's value to each of its
// m children keeps every family's share of the samples (m d / (m sum) = d / sum); where the plans do not nest the shares move by the
// cells' overlap, which is what a warm start may do -- any allocation with n_h >= 2 gives an unbiased estimate.  e == 1 copies the bits.
// One thread per NEW hypercube on a grid-stride loop, the mixed-radix decode (draw 0 fastest) by the magic reciprocals the sample kernel
// divides with (strat_magic, mci_host_strat.h); plain loads and stores, no LDS.
// >>> strat remap cell rule (compiled for the host by tests/test_strat_carry_host.py)
__host__ __device__ inline int strat_remap_cell(int j, int n_old, int n_new) {
    return (int)(((2ull * (unsigned long long)j + 1ull) * (unsigned long long)n_old) / (2ull * (unsigned long long)n_new));
}
// old hypercube of the new hypercube whose cells are j[ndim]
__host__ __device__ inline long long strat_remap_index(const int *j, const int *n_old, const int *n_new, int ndim) {
    long long h = 0, stride = 1;
    for (int d = 0; d < ndim; ++d) {
        h += (long long)strat_remap_cell(j[d], n_old[d], n_new[d]) * stride;
        stride *= n_old[d];
    }
    return h;
}
// <<< strat remap cell rule
enum { kStratRemapMaxDraw = 32 };
struct StratRemapArgs {
    const double *d_old; // [prod n_old]
    double *d_new;       // [ncube] out
    long long ncube;     // prod n_new
    int ndim;
    double e;            // beta_new / beta_old
    unsigned magic[kStratRemapMaxDraw]; // h' / n_new[d] = (h' * magic[d]) >> shift[d], exact for h' < 2^31
    int shift[kStratRemapMaxDraw];
    int n_new[kStratRemapMaxDraw], n_old[kStratRemapMaxDraw];
};
__global__ void __launch_bounds__(256) k_strat_remap(StratRemapArgs a) {
    const long long step = (long long)gridDim.x * 256;
    for (long long hn = (long long)blockIdx.x * 256 + threadIdx.x; hn < a.ncube; hn += step) {
        unsigned q = (unsigned)hn;
        long long h = 0, stride = 1;
        for (int d = 0; d < a.ndim; ++d) {
            const unsigned qn = (unsigned)(((unsigned long long)q * a.magic[d]) >> a.shift[d]);
            const int j = (int)(q - qn * (unsigned)a.n_new[d]);
            q = qn;
            h += (long long)strat_remap_cell(j, a.n_old[d], a.n_new[d]) * stride;
            stride *= a.n_old[d];
        }
        const double v = a.d_old[h];
        a.d_new[hn] = a.e == 1.0 ? v : pow(v, a.e);
    }
}

// k_strat_reduce: the iteration's (mean, var) per column from the chunks' partial rows (their interior hypercubes) and the boundary
// records (the hypercubes the chunk boundaries cut: the pieces of one hypercube are the records of consecutive chunks, folded in chunk
// order), and d_h = (sum_k s^2_{h,k})^(beta/2) of the cut hypercubes.  One workgroup; every thread takes a stretch of chunks, the threads'
// sums are combined by a fixed tree: bit-identical run to run.  Writes out[2 nw] = mean | var and, when given, the same into the
// iteration log row (row[k] = mean, row[nobs + k] = var).
enum { kStratReduceCols = 8, kStratReduceThreads = 1024 };
struct StratReduceArgs {
    const long long *off;
    const double *part;
    const long long *rec_h;
    const double *rec_s;
    long long ncube, nchunk;
    int nw;
    double beta;
    double *dnext;
    double *out;
    double *log_row;
};
__global__ void __launch_bounds__(kStratReduceThreads) k_strat_reduce(StratReduceArgs a) {
    __shared__ double red[kStratReduceThreads];
    const int tid = threadIdx.x, T = blockDim.x, nw = a.nw;
    double acc[2 * kStratReduceCols];
    for (int q = 0; q < 2 * kStratReduceCols; ++q) acc[q] = 0.0;
    const double V = 1.0 / (double)a.ncube;
    const long long per = (a.nchunk + T - 1) / T;
    long long c0 = (long long)tid * per;
    if (c0 > a.nchunk) c0 = a.nchunk;
    const long long c1 = c0 + per < a.nchunk ? c0 + per : a.nchunk;
    for (long long c = c0; c < c1; ++c) {
        for (int q = 0; q < 2 * nw; ++q) acc[q] += a.part[c * 2 * nw + q];
        for (int rr = 0; rr < 2; ++rr) {
            const long long h = a.rec_h[2 * c + rr];
            if (h < 0) continue;
            if (rr == 0 && c > 0) { // a continuation of the previous chunk's last piece: folded there
                const long long ph = a.rec_h[2 * c - 1] >= 0 ? a.rec_h[2 * c - 1] : a.rec_h[2 * c - 2];
                if (ph == h) continue;
            }
            double S[2 * kStratReduceCols];
            for (int q = 0; q < 2 * nw; ++q) S[q] = a.rec_s[(2 * c + rr) * 2 * nw + q];
            for (long long d = c + 1; d < a.nchunk && a.rec_h[2 * d] == h; ++d)
                for (int q = 0; q < 2 * nw; ++q) S[q] += a.rec_s[(2 * d) * 2 * nw + q];
            const double n = (double)(a.off[h + 1] - a.off[h]);
            double ssum = 0.0;
            for (int q = 0; q < nw; ++q) {
                double v2 = (S[nw + q] - S[q] * S[q] / n) / (n - 1.0);
                v2 = v2 > 0.0 ? v2 : 0.0;
                acc[q] += V / n * S[q];
                acc[nw + q] += V * V * v2 / n;
                ssum += v2;
            }
            a.dnext[h] = strat_damp(ssum, a.beta);
        }
    }
    for (int q = 0; q < 2 * nw; ++q) {
        red[tid] = acc[q];
        __syncthreads();
        for (int s = T / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) {
            a.out[q] = red[0];
            if (a.log_row) a.log_row[q] = red[0]; // (nobs == nw: row[k] = mean, row[nobs + k] = var)
        }
        __syncthreads();
    }
}

} // namespace mci
