// mci_sweep_common.h -- what the four batched-sweep kernels share: mci_sweep.h (one Continuous grid), mci_sweep_leaves.h (any mix of
// Continuous and Discrete leaves), mci_sweep_strat.h (stratified points) and mci_sweep_chains.h (:vegasmc points; :mcmc points: the same body's other instantiation).  Each of them is a translation unit of its own (mci_jit.h
// kUnits) and includes this header; the host (mci_host_sweep.h) compiles the same text, so the argument layout cannot drift.  Free of
// host / std headers.
//
// In all four ONE workgroup owns a point and runs its whole loop, and no workgroup ever waits for another one: no counter anybody waits for, no
// spinning, no residency condition, and every loop's trip count is a kernel argument or a constant of the translation unit.  (The two
// `until` units -- vegas_sweep<Cfg, true>, vegas_sweep_leaves<Cfg, true> -- hand out the points behind the first gridDim.x through one
// word, SweepUntil::cursor: a workgroup that has finished a point adds 1 to it and takes what it gets.  Nothing ever waits on that word
// or reads it back; a point's iteration loop stays bounded by the kernel argument niter, and it leaves the loop early only on numbers
// its own workgroup holds.)
//
// The ordering argument.  What travels through global memory inside a point -- the partial rows, merge_stats' scratch and head, the
// histogram row the sample loop adds to with f64 atomics, and whatever a unit adds of its own -- is written and read by the SAME
// workgroup.  Between the two sides stands sweep_round_trip(): every wave waits for its own stores and atomics (s_waitcnt vmcnt(0): a
// barrier alone orders nothing in global memory, see persist_signal in mci_train.h), then the workgroup meets at a barrier.  The CU's
// write-through L1 is coherent for its own workgroup's plain stores, so plain loads see them behind that round trip.  The histogram row is
// different: the atomics change it in L2 behind that L1, so sweep_take_hist() reads it with agent-scope atomic loads that bypass the L1,
// and zeroes it the same way.  And no two threads ever touch one bin: flush_workgroup's adds run over the whole row [0, NBIN) with stride
// T, so bin j of the row belongs to thread j % T; a leaf's slice [boff, boff + N) is read and zeroed by the thread whose index is
// (boff + i) % T for bin boff + i -- which is `first = (tid + T - boff % T) % T`, and plainly `tid` where boff == 0.  Adds, read and
// zeroing of a bin are therefore one thread's, in program order, with a round trip between one iteration's zeroing and the next one's adds.
#pragma once
#include "mci_train.h"

namespace mci {

// the head of every sweep kernel's second argument (the stratified unit appends its own fields: SweepStratArgs)
struct SweepHead {
    MergeArgs m;           // of point 0: part_cols [npoint][rows][ncols], scratch [npoint][rows * ncols], packed [npoint][nstat],
                           // ghist [npoint][nbin], status [npoint]; use_ghist = 1, wg_per_block = 1; rows: sweep_point's rows_per_point
    TrainArgs t;           // t.edges / t.dacc / t.ddist: the problem's own map (read only: where a point starts when maps_in == NULL);
                           // t.iter_log_row: [npoint][niter][nstat]; t.maxn: bins of the largest leaf
    int npoint, niter, nuserdata;
    int map_off;           // doubles: where the point's map lies in LDS, behind both the sample loop's carve and the refinement's scratch
    const double *ud;      // [npoint][nuserdata]
    const u64 *seeds;      // [npoint] or NULL: BatchArgs::seed for every point
    const double *maps_in; // [npoint][doubles of a map row] or NULL
    double *maps_out;      // [npoint][doubles of a map row]
};

// ---- a target error per point (mci_integrate_sweep_until): the `until` units' own argument behind the head, and the stop rule
struct SweepUntil {
    double rtol, atol;     // a column has converged when E <= max(atol, rtol |M|)
    int min_niter, ignore; // ... and n >= max(ignore + 2, min_niter); ignore as mci_integrate resolved it
    double *sums;          // [npoint][2 nobs], zeroed by the host: W_o | sum w m of column o, written and read by thread o % T alone
    int *iters;            // [npoint]: n_p, the iterations point p ran
    int *cursor;           // one word, zeroed by the host: points handed out behind the first gridDim.x
};
struct SweepUntilArgs {
    SweepHead h;
    SweepUntil u;
};

// The stop rule, in the reference's own arithmetic; tests/test_sweep_until_host.py compiles the lines between the markers for the host.
// >>> sweep until rule
// mci_mean_std of one column of a statistics head (main.jl:297-317): sum and sum of squares of the blocks' means
__host__ __device__ inline void sweep_until_mean_std(double sum, double sq, int nblocks, double &m, double &s) {
    m = sum / (double)nblocks; // main.jl:317
    s = 0.0;                   // main.jl:311
    if (nblocks > 1) {
        const double v = (sq / (double)nblocks - m * m) / (double)(nblocks - 1); // main.jl:308
        s = v < 0.0 ? 0.0 : sqrt(v);                                             // main.jl:297-299
    }
}
// iteration n (1-based) of a column enters its running sums from n = ignore + 1 on: W += w, S += w m, w = 1 / (s + 1e-10)^2 (statistics.jl:186-204)
__host__ __device__ inline void sweep_until_add(double m, double s, int n, int ignore, double &W, double &S) {
    if (n <= ignore) return;
    const double sd = s + 1.0e-10, w = 1.0 / (sd * sd);
    W += w;
    S += w * m;
}
// the column after its iteration n: M = S / W, E = 1 / sqrt(W) (mci_average) is an error estimate from two averaged iterations on
// (below that mci_average returns iteration 1, statistics.jl:189-191); a column whose E or M is NaN or infinite never converges
__host__ __device__ inline bool sweep_until_done(double W, double S, int n, int ignore, int min_niter, double rtol, double atol) {
    const int first = ignore + 2 > min_niter ? ignore + 2 : min_niter;
    if (n < first) return false;
    const double M = S / W, E = 1.0 / sqrt(W);
    if (!(isfinite(M) && isfinite(E))) return false;
    const double rel = rtol * fabs(M), bound = atol > rel ? atol : rel;
    return E <= bound;
}
// <<< sweep until rule

// every wave has performed its global stores and atomics, then the workgroup meets
__device__ __forceinline__ void sweep_round_trip() {
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
    __syncthreads();
}

// point p's own rows of the sweep's buffers: m <- f.m, a <- a0, both rebased (the caller sets a's tables: they lie in its LDS)
template <class Cfg> __device__ __forceinline__ void sweep_point(const SweepHead &f, const BatchArgs &a0, int p, int rows_per_point, MergeArgs &m, BatchArgs &a) {
    const int ncols = f.m.ncols, nstat = f.t.nstat;
    m = f.m;
    m.part_cols = f.m.part_cols + (size_t)p * rows_per_point * ncols;
    m.scratch = f.m.scratch + (size_t)p * rows_per_point * ncols;
    m.packed = f.m.packed + (size_t)p * nstat;
    m.ghist = f.m.ghist + (size_t)p * Cfg::NBIN;
    m.status = f.m.status + p;
    a = a0;
    a.ud = f.ud + (size_t)p * f.nuserdata;
    a.part_cols = const_cast<double *>(m.part_cols);
    a.ghist = m.ghist;
    a.status = m.status;
    if (f.seeds) a.seed = f.seeds[p];
}

// iteration_bookkeeping's arguments for point p, iteration `it`
__device__ __forceinline__ TrainArgs sweep_log_row(const SweepHead &f, int p, int it) {
    TrainArgs t = f.t;
    t.packed = f.m.packed + (size_t)p * f.t.nstat;
    t.iter_log_row = f.t.iter_log_row + ((size_t)p * f.niter + it) * f.t.nstat;
    return t;
}

// The rule on point p's statistics head after its iteration n (1-based), behind merge_stats and its barrier: column o is thread o % T's
// -- it reads the head's sum and sum of squares, moves the column's running sums in the point's row of u.sums (written and read by this
// thread alone, in program order: the header's ordering argument as it stands) and objects through *pending (LDS, reset by thread 0
// before the iteration's sample loop) when the column has not converged.  The word is complete behind the workgroup's next barrier.
__device__ __forceinline__ void sweep_until_columns(const SweepUntil &u, const double *packed, int nobs, int nblocks, int p, int n, int *pending) {
    double *row = u.sums + (size_t)p * 2 * nobs;
    int wait = 0;
    for (int o = threadIdx.x; o < nobs; o += blockDim.x) {
        double m, s, W = row[o], S = row[nobs + o];
        sweep_until_mean_std(packed[o], packed[nobs + o], nblocks, m, s);
        sweep_until_add(m, s, n, u.ignore, W, S);
        row[o] = W;
        row[nobs + o] = S;
        if (!sweep_until_done(W, S, n, u.ignore, u.min_niter, u.rtol, u.atol)) wait = 1;
    }
    if (wait) atomicOr(pending, 1);
}
// The point a workgroup runs behind point p.  UNTIL: thread 0 leaves n_p in u.iters[p] and fetches the next point from the cursor --
// gridDim.x + what the word held --, the others read it from words[1] (LDS) behind a barrier; the barrier that opens a point stands
// between these reads and the next write.
template <bool UNTIL> __device__ __forceinline__ int sweep_next_point(int p, const SweepUntil *u, int *words, int n_run) {
    if constexpr (UNTIL) {
        if (threadIdx.x == 0) {
            u->iters[p] = n_run;
            words[1] = (int)gridDim.x + atomicAdd(u->cursor, 1);
        }
        __syncthreads();
        return words[1];
    } else {
        (void)u, (void)words, (void)n_run;
        return p + (int)gridDim.x;
    }
}

// merge_hist_bin for a slice of N bins at gh: hl <- the clearStatistics! offset + what the sample loop added; the slice is zero again for
// the next iteration; a bad histogram's bits go to *verdict (LDS).  first: this thread's first bin of the slice (the header comment)
__device__ __forceinline__ void sweep_take_hist(double *gh, double *hl, int N, int first, double offset, int *verdict) {
    const int T = blockDim.x;
    int hbad = 0;
    for (int base = 0; base < N; base += kTrainQ * T) {
        double v[kTrainQ];
#pragma unroll
        for (int q = 0; q < kTrainQ; ++q) {
            const int i = base + q * T + first;
            v[q] = i < N ? __hip_atomic_load(&gh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kTrainQ; ++q) {
            const int i = base + q * T + first;
            if (i < N) {
                __hip_atomic_store(&gh[i], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double h = offset + v[q];
                hl[i] = h;
                if (!isfinite(h)) hbad |= ST_HIST_NONFINITE;      // variable.jl:212
                else if (!(h > 0.0)) hbad |= ST_HIST_NONPOSITIVE; // variable.jl:213 / common.jl:71
            }
        }
    }
    if (hbad) atomicOr(verdict, hbad);
}

// ---- the map of a point with several leaves (mci_sweep_leaves.h, mci_sweep_chains.h): its maps_in / maps_out row and its block in LDS
// One maps_in / maps_out row: the leaves in order; a Continuous leaf its nbin + 1 grid points, a Discrete leaf its accumulation
// [nbin + 1] and then its distribution [nbin]  (the host's sweep_map_doubles, mci_host_sweep.h)
template <class Cfg> constexpr int sweep_row_off(int l) {
    int n = 0;
    for (int k = 0; k < l; ++k) n += Cfg::leaf_kind(k) == 0 ? Cfg::leaf_nbin(k) + 1 : 2 * Cfg::leaf_nbin(k) + 1;
    return n;
}
template <class Cfg> constexpr int sweep_max_nbin() {
    int n = 1;
    for (int k = 0; k < Cfg::NLEAF; ++k) n = Cfg::leaf_nbin(k) > n ? Cfg::leaf_nbin(k) : n;
    return n;
}
template <class Cfg> constexpr bool sweep_kinds_ok() {
    for (int k = 0; k < Cfg::NLEAF; ++k)
        if (Cfg::leaf_kind(k) != 0 && Cfg::leaf_kind(k) != 1) return false;
    return true;
}
// the map block's parts, doubles from map_off (the host's sweep_leaves_lds lays out the same)
template <class Cfg> struct SweepBlock {
    static constexpr int E = 0;
    static constexpr int DA = E + ((Cfg::NEDGE + 1) & ~1);
    static constexpr int DD = DA + ((Cfg::NDACC + 1) & ~1);
    static constexpr int FLAGS = DD + ((Cfg::NDDIST + 1) & ~1);
    static constexpr int END = FLAGS + 4;
};

// row <-> block, leaf by leaf (TO_ROW: block -> maps_out row; else row -> block)
template <class Cfg, bool TO_ROW> __device__ __forceinline__ void sweep_copy_row(double *blk, double *row_out, const double *row_in) {
    const int tid = threadIdx.x, T = blockDim.x;
    static_for<0, Cfg::NLEAF>([&](auto Lf) {
        constexpr int l = decltype(Lf)::value, N = Cfg::leaf_nbin(l), ro = sweep_row_off<Cfg>(l);
        if constexpr (Cfg::leaf_kind(l) == 0) {
            double *g = blk + SweepBlock<Cfg>::E + Cfg::leaf_eoff(l);
            for (int i = tid; i <= N; i += T) {
                if constexpr (TO_ROW) row_out[ro + i] = g[i];
                else g[i] = row_in[ro + i];
            }
        } else {
            double *acc = blk + SweepBlock<Cfg>::DA + Cfg::leaf_eoff(l), *dist = blk + SweepBlock<Cfg>::DD + Cfg::leaf_doff(l);
            for (int i = tid; i <= N; i += T) {
                if constexpr (TO_ROW) row_out[ro + i] = acc[i];
                else acc[i] = row_in[ro + i];
            }
            for (int i = tid; i < N; i += T) {
                if constexpr (TO_ROW) row_out[ro + N + 1 + i] = dist[i];
                else dist[i] = row_in[ro + N + 1 + i];
            }
        }
    });
}

} // namespace mci
