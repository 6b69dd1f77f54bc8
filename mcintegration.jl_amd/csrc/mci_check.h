// mci_check.h -- an independent :vegas iteration for a layout described AT RUN TIME, compiled ahead of time by hipcc (never by hiprtc).
// It is the yardstick a NEW :vegas code object is held against before its first launch (mci_host_check.h vegas_self_check): every user
// integrand is a new hiprtc translation unit, and one of ours once came out with the right estimates and its histogram adds in the wrong
// bins.  k_check_vegas is the plain definition of Vegas.montecarlo (vegas/montecarlo.jl:117-187) with the integrand values handed in:
// one thread per sample, the uniforms regenerated from the library's Philox streams (DESIGN.md "RNG streams"), iy = floor(y N),
// x = g[iy] + dy (g[iy+1] - g[iy]) (sampler.jl:293-305), Discrete draws by bisection (sampler.jl:17-20, common.jl:16-25), the padding
// probabilities of mixed-dof integrands as products over an integrand's own draws (variable.jl:628-641), global f64 atomics into a zeroed
// buffer.  Deliberately plain: no Cfg traits, no LDS, no packing, no pipelining, no inline assembly -- nothing it shares with the sample
// kernels of mci_device.h but the documented stream addressing and the constants of Philox4x32.  Bins come from y, never from a search of
// x in the edge table (ambiguous when x rounds onto an edge; a false alarm is worse than no check).
#pragma once
#include <hip/hip_runtime.h>

namespace mci {

// one draw of a sample, in draw order (pool, slot, leaf)
struct CheckDraw {
    int kind;     // 0 Continuous, 1 Discrete
    int off;      // Continuous: offset of the leaf's edges in `edges`; Discrete: of its accumulation table in `dacc`
    int doff;     // Discrete: offset of its distribution in `ddist`
    int nbin;     // increments of the grid | entries of the distribution
    int boff;     // offset of the leaf's histogram in the histogram section
    int hist;     // the draw's leaf adapts and some integrand covers the draw: its bin takes histogram adds
    double scale; // 1/prob = raw * scale: N for a Continuous leaf (raw = the increment's width), 1 for a Discrete one (raw = 1/distribution)
    double lower; // Discrete: value of the first entry
};
struct CheckIntegrand {
    unsigned long long own;                // draws the integrand covers (bit = draw)
    int obs_off, obs_nbin, obs_bin_draw;   // its observable columns | their number | the Discrete draw that bins them (-1: none)
    int pad_;
};
struct CheckArgs {
    const CheckDraw *draw;      // [ndraw]
    const CheckIntegrand *intg; // [ni]
    int ndraw, ni, ncomp, nobs, ncols;
    int rng_bits, rng_rounds;   // 52 | 32 bits per draw; 10 | 7 Philox rounds
    int with_obs;               // 0: a user measure -- the observable columns stay zero
    const double *edges, *dacc, *ddist;
    unsigned long long seed;
    unsigned int iteration;
    long long block_lo, neval_per_block, measurefreq, n; // first global statistical block | samples per block | cadence | samples of this launch: whole blocks from block_lo on
    const double *x, *jac, *w;  // [n][ndraw], [n], [n][ni * ncomp]: what mci_sample_dump produced for these samples
    double *cols;               // [blocks][ncols] every block's column sums: observables | normalization | neval | visited
    double *hist;               // [nbin] histogram section, all blocks
    unsigned long long *bad;    // [0] samples whose x differs in some bit, [1] whose jac differs by more than 1e-13 relative
};

__device__ inline void check_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, int rounds, unsigned *out) {
    for (int r = 0; r < rounds; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// uniform of draw k of sample `index`: key = seed, counter = (index lo, index hi, Philox block of the draw, stream)
__device__ inline double check_uniform(const CheckArgs &a, unsigned long long index, int k) {
    const unsigned stream = a.iteration * 8u; // (+ STREAM_VEGAS = 0)
    unsigned r[4];
    unsigned long long bits;
    if (a.rng_bits == 32) { // one word per draw: its 32 bits are the top mantissa bits
        check_philox((unsigned)index, (unsigned)(index >> 32), (unsigned)(k >> 2), stream, (unsigned)a.seed, (unsigned)(a.seed >> 32), a.rng_rounds, r);
        bits = 0x3FF0000000000000ull | ((unsigned long long)r[k & 3] << 20);
    } else { // a word pair per draw: 52 mantissa bits
        check_philox((unsigned)index, (unsigned)(index >> 32), (unsigned)(k >> 1), stream, (unsigned)a.seed, (unsigned)(a.seed >> 32), a.rng_rounds, r);
        const unsigned lo = r[2 * (k & 1)], hi = r[2 * (k & 1) + 1];
        bits = 0x3FF0000000000000ull | ((((unsigned long long)hi << 32) | lo) >> 12);
    }
    return __longlong_as_double((long long)bits) - 1.0; // [1, 2) - 1: exact
}

// product of 1/prob over the draws of `mask`, draw by draw as the reference forms it (vegas/montecarlo.jl:126): no bare product of
// increments, which leaves the doubles where the Jacobian itself does not (DESIGN.md "Jacobian")
__device__ inline double check_jacobian(const CheckArgs &a, const double *raw, unsigned long long mask) {
    double j = 1.0;
    for (int k = 0; k < a.ndraw; ++k)
        if ((mask >> k) & 1ull) j *= raw[k] * a.draw[k].scale;
    return j;
}

__global__ void __launch_bounds__(256) k_check_vegas(CheckArgs a) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; // sample of the launch
    if (n >= a.n) return;
    const long long lb = n / a.neval_per_block, ne = n % a.neval_per_block; // its block | its number in the block
    const unsigned long long index = (unsigned long long)(a.block_lo * a.neval_per_block + n);
    double *cols = a.cols + lb * a.ncols;
    double raw[64];
    int bin[64];
    bool xbad = false;
    for (int k = 0; k < a.ndraw; ++k) {
        const CheckDraw d = a.draw[k];
        const double y = check_uniform(a, index, k);
        double x;
        if (d.kind == 0) {
            const double yn = y * (double)d.nbin;
            int iy = (int)yn;
            if (iy > d.nbin - 1) iy = d.nbin - 1; // (y < 1, so this never binds; it keeps the reads inside the table whatever comes in)
            const double dy = yn - (double)iy;
            const double g0 = a.edges[d.off + iy], dx = a.edges[d.off + iy + 1] - g0;
            x = g0 + dy * dx;
            raw[k] = dx;
            bin[k] = iy;
        } else {
            int jl = 1, ju = d.nbin + 2;
            while (ju - jl > 1) {
                const int jm = (jl + ju) >> 1;
                if (y < a.dacc[d.off + jm - 1]) ju = jm;
                else jl = jm;
            }
            if (jl > d.nbin) jl = d.nbin;
            x = d.lower + (double)(jl - 1);
            raw[k] = 1.0 / a.ddist[d.doff + jl - 1];
            bin[k] = jl - 1;
        }
        if (__double_as_longlong(x) != __double_as_longlong(a.x[n * a.ndraw + k])) xbad = true;
    }
    const unsigned long long all = a.ndraw >= 64 ? ~0ull : ((1ull << a.ndraw) - 1ull);
    const double jac = check_jacobian(a, raw, all);
    if (xbad) atomicAdd(&a.bad[0], 1ull);
    {
        const double jd = a.jac[n], big = fmax(fabs(jac), fabs(jd));
        if (!(fabs(jac - jd) <= 1.0e-13 * big)) atomicAdd(&a.bad[1], 1ull);
    }
    const int nw = a.ni * a.ncomp;
    const double *w = a.w + n * nw;
    atomicAdd(&cols[a.nobs + 1], 1.0);           // config.neval += 1           vegas/montecarlo.jl:118
    if ((ne + 1) % a.measurefreq == 0) {            //                             :148
        atomicAdd(&cols[a.nobs], 1.0);           // config.normalization += 1   :164
        for (int i = 0; i < a.ni && a.with_obs; ++i) {
            const CheckIntegrand g = a.intg[i];
            const double ji = g.own == all ? jac : check_jacobian(a, raw, g.own); // weights * padding_probability * jac   :152
            if (g.obs_bin_draw < 0) {
                for (int q = 0; q < a.ncomp; ++q) atomicAdd(&cols[g.obs_off + q], w[i * a.ncomp + q] * ji);
            } else {
                const int b = bin[g.obs_bin_draw];
                if (b >= 0 && b < g.obs_nbin) atomicAdd(&cols[g.obs_off + b], w[i] * ji);
            }
        }
    }
    for (int k = 0; k < a.ndraw; ++k) {            // accumulate!(var, pos, (abs(weights[i]) * jac)^2)   :170-185
        const CheckDraw d = a.draw[k];
        if (!d.hist) continue;
        double wk = 0.0;
        for (int i = 0; i < a.ni; ++i)
            if ((a.intg[i].own >> k) & 1ull) {
                const double aw = a.ncomp == 1 ? fabs(w[i]) : hypot(w[2 * i], w[2 * i + 1]);
                const double wj = aw * jac;
                wk += wj * wj;
            }
        if (bin[k] >= 0 && bin[k] < d.nbin) atomicAdd(&a.hist[d.boff + bin[k]], wk);
    }
}

} // namespace mci
