// mci_host_strat.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// stratified :vegas (VEGAS+ adaptive stratified sampling): the plan, the setters, the sample launch (mci_strat.h) and the iteration's
// reduce + next allocation (k_strat_reduce, k_strat_alloc).  mci_iteration_run / _finish and mci_integrate call in here when the
// problem is stratified; nothing here runs otherwise.
static_assert(mci::kStratMaxCols == mci::kStratReduceCols, "k_strat_reduce keeps the columns the sample kernel writes");
static int flush_merge(mci_problem *p);

// The default plan leaves kStratSamplesPerCube samples per hypercube on average, not the two every hypercube must have: with two, the
// per-hypercube variances are two-sample estimates whose sum is far too small on heavy tails (32 seeds of log(x)/sqrt(x) at neval = 1e5:
// scatter of the means 5.1 x the reported error; the Watson integral 1.3 x), and N - 2 ncube = 0 samples are left to move.  With eight
// the reported errors match the scatter (1.01, 1.00) and three quarters of the samples follow the variance (profiles/r07_stratified.txt).
static const int64_t kStratSamplesPerCube = 8;

int mci_strat_plan(int64_t neval, int32_t ndim, int64_t max_nhcube, int32_t *nstrat) {
    if (!nstrat || ndim < 1) return fail(MCI_ERR_INVALID, "stratification: ndim must be positive");
    if (max_nhcube < 1) return fail(MCI_ERR_INVALID, "stratification: max_nhcube must be positive");
    const int64_t per = neval / kStratSamplesPerCube, cap = per < max_nhcube ? per : max_nhcube;
    if (cap < 1) return fail(MCI_ERR_INVALID, "stratification: neval = %lld is too small for %lld samples per hypercube", (long long)neval,
                             (long long)kStratSamplesPerCube);
    // prod of ndim factors v, or cap + 1 once it exceeds cap
    auto power_le = [cap](int64_t v, int n) {
        int64_t r = 1;
        for (int i = 0; i < n; ++i) {
            if (r > cap / v) return cap + 1;
            r *= v;
        }
        return r;
    };
    int64_t s = (int64_t)floor(pow((double)cap, 1.0 / ndim));
    if (s < 1) s = 1;
    while (s > 1 && power_le(s, ndim) > cap) --s;
    while (power_le(s + 1, ndim) <= cap) ++s;
    int64_t ncube = power_le(s, ndim);
    for (int d = 0; d < ndim; ++d) nstrat[d] = (int32_t)s;
    for (int d = 0; d < ndim; ++d) {
        if (ncube / s * (s + 1) > cap) break;
        ncube = ncube / s * (s + 1);
        nstrat[d] = (int32_t)(s + 1);
    }
    return MCI_OK;
}

namespace {
// what a stratified problem must not have (the follow-ups of this mode): checked when it is switched on
int strat_layout_check(const mci_problem *p, int32_t ndim) {
    const auto &s = p->shape;
    for (const auto &L : p->leaves)
        if (L.kind != 0) return fail(MCI_ERR_INVALID, "stratification: only Continuous variables are stratified (a Discrete or FermiK variable is refused)");
    if (!s.measure_body.empty() || s.host_measure) return fail(MCI_ERR_INVALID, "stratification: a user measure is refused (the default measure only)");
    if (s.host_integrand) return fail(MCI_ERR_INVALID, "stratification: a host integrand is refused (device source or a traced closure only)");
    if (p->ctx->nranks != 1) return fail(MCI_ERR_INVALID, "stratification: more than one rank is refused");
    if (s.ntile > 1 || s.ec_doubles > 0) return fail(MCI_ERR_INVALID, "stratification: a layout with several histogram tiles is refused");
    if (!(s.table_mode == 0 || s.table_mode == 3)) return fail(MCI_ERR_INVALID, "stratification: histograms outside LDS (table mode %d) are refused", s.table_mode);
    if (ndim != s.ndraw) return fail(MCI_ERR_INVALID, "stratification: ndim = %d, but a sample has %d draws", (int)ndim, s.ndraw);
    if (s.ndraw > mci::kStratMaxDraw) return fail(MCI_ERR_INVALID, "stratification: %d draws per sample (at most %d)", s.ndraw, (int)mci::kStratMaxDraw);
    if (s.ni * s.ncomp > mci::kStratMaxCols) return fail(MCI_ERR_INVALID, "stratification: %d weight columns (at most %d)", s.ni * s.ncomp, (int)mci::kStratMaxCols);
    return MCI_OK;
}

// The geometry of a stratified iteration of N samples in `nblocks` statistical blocks (strat_run; the stratified sweep asks for mblocks, and
// for the chunk of its own LDS need).  Chunk size: the largest of 8 | 4 | 2 | 1 trips of 256 samples whose LDS -- need[0 .. 3] bytes, with
// strat_nloc(trips) hypercubes per chunk -- stays within 64 KiB (two workgroups per CU), else within a CU's 159 KiB; trips = 0: neither.
// Workgroups: one per chunk up to 2048, a multiple of the call's block count where there are enough chunks: the merge then groups the
// rows into the call's blocks, whose clearStatistics! offsets the histogram carries as classic :vegas's does -- one hypercube gives
// classic's histogram and map.
struct StratGeometry {
    int trips = 0;
    int64_t lds = 0, S = 0, nchunk = 0, nwg = 0, mblocks = 0;
};
// LDS behind the sample kernel's own carve, bytes (mci_strat.h strat_lds_doubles at 256 threads)
int strat_nloc(int trips) { return trips * 256 / 2 + 1; }
int64_t strat_chunk_lds_bytes(int nloc, int NW) { return (int64_t)((nloc + 1) + nloc * 2 * NW + 256 + 256 * 2 * NW) * 8; }
void strat_geometry(int64_t N, int64_t nblocks, const int64_t (&need)[4], StratGeometry &g) {
    g = StratGeometry();
    const int T = 256;
    for (int64_t lim : {(int64_t)64 * 1024, (int64_t)159 * 1024}) {
        for (int k = 8; k >= 1 && !g.trips; k >>= 1) {
            const int64_t bytes = need[k == 8 ? 0 : k == 4 ? 1 : k == 2 ? 2 : 3];
            if (bytes <= lim) {
                g.trips = k;
                g.lds = bytes;
            }
        }
        if (g.trips) break;
    }
    if (!g.trips) return;
    g.S = (int64_t)g.trips * T;
    g.nchunk = (N + g.S - 1) / g.S;
    g.nwg = g.nchunk < 2048 ? g.nchunk : 2048;
    g.mblocks = g.nwg >= nblocks ? nblocks : 1;
    g.nwg -= g.nwg % g.mblocks;
}

int strat_alloc_tiles(int64_t ncube) { return mci::strat_alloc_ntile(ncube); }

// The launches of the three stratified static kernels, for the product (below) and for the test hooks of csrc/mci_debug.h alike, so that
// grids, thread counts and phases are written down once.
// k_strat_alloc: tile sums (ntile workgroups), tile bases + total + the uniform verdict (one), offsets (ntile)
hipError_t strat_alloc_launches(const mci::StratAllocArgs &a, hipStream_t stream) {
    for (int phase = 0; phase < 3; ++phase) {
        hipLaunchKernelGGL(mci::k_strat_alloc, dim3(phase == 1 ? 1 : (unsigned)a.ntile), dim3(256), 0, stream, a, phase);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// k_strat_reduce: one workgroup
hipError_t strat_reduce_launch(const mci::StratReduceArgs &r, hipStream_t stream) {
    hipLaunchKernelGGL(mci::k_strat_reduce, dim3(1), dim3(mci::kStratReduceThreads), 0, stream, r);
    return hipGetLastError();
}

// the allocation of the run about to start, over the offsets the last run used: from d_h, or uniform
int strat_launch_alloc(mci_problem *p, bool uniform) {
    auto &st = p->strat;
    mci::StratAllocArgs a{};
    a.d = st.d_d;
    a.off = st.d_off;
    a.tsum = st.d_tsum;
    a.ncube = st.ncube;
    a.nsamp = st.nsamp;
    a.ntile = strat_alloc_tiles(st.ncube);
    a.uniform = uniform ? 1 : 0;
    HIPCHK(strat_alloc_launches(a, p->ctx->stream));
    st.alloc_valid = true;
    st.alloc_pending = false;
    return MCI_OK;
}

// h / n = (h * magic) >> shift, exact for h < 2^31 (Granlund-Montgomery, N = 31): the reciprocals the sample kernel decodes a hypercube
// into its cells with (StratArgs) and k_strat_remap a new hypercube into its
// >>> strat magic (compiled for the host by tests/test_strat_kernels_host.py)
void strat_magic(uint32_t n, uint32_t *magic, int *shift) {
    int l = 0;
    while (((uint64_t)1 << l) < n) ++l;
    // h < 2^31: q = floor(h * m / 2^(32 + l)), m = ceil(2^(32 + l) / n) < 2^33 ... kept in 32 bits by folding one bit into the shift
    // for l <= 31: m' = ceil(2^(31 + l) / n) <= 2^32 and q = (h * m') >> (31 + l), exact for h < 2^31
    const uint64_t m = (((uint64_t)1 << (31 + l)) + n - 1) / n;
    *magic = (uint32_t)(m > 0xFFFFFFFFull ? 0xFFFFFFFFull : m);
    *shift = 31 + l;
    if (n == 1) { // (h / 1: m' = 2^31, shift 31)
        *magic = 0x80000000u;
        *shift = 31;
    }
}
// <<< strat magic

// k_strat_remap over a.ncube = prod n_new new hypercubes: the plans and their reciprocals into the arguments, one thread per new hypercube
// up to 4096 workgroups of 256 (the kernel strides beyond)
hipError_t strat_remap_launch(mci::StratRemapArgs &a, const int *n_old, const int *n_new, int D, hipStream_t stream) {
    a.ndim = D;
    for (int d = 0; d < D; ++d) {
        strat_magic((uint32_t)n_new[d], &a.magic[d], &a.shift[d]);
        a.n_new[d] = n_new[d];
        a.n_old[d] = n_old[d];
    }
    const unsigned grid = (unsigned)((a.ncube + 255) / 256 < 4096 ? (a.ncube + 255) / 256 : 4096);
    hipLaunchKernelGGL(mci::k_strat_remap, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// d_off / d_d with room for ncube hypercubes (what they held is gone when they grow)
int strat_reserve(mci_problem *p, int64_t ncube) {
    auto &st = p->strat;
    int rc = st.d_tsum.reserve(2 * 1024 + 2);
    if (rc || ncube <= st.d_d.capacity()) return rc;
    if ((rc = st.d_off.reserve(ncube + 1)) || (rc = st.d_d.reserve(ncube))) return rc;
    HIPCHK(hipMemsetAsync(st.d_d, 0, (size_t)ncube * sizeof(double), p->ctx->stream));
    return MCI_OK;
}

// The first allocation of plan ns for N samples (a call starts, the plan or N changed, a setter was called): uniform -- or, on a problem
// that carries its allocation (mci_set_stratification_carry) and holds a d_h, from that d_h: as it is on the plan and under the beta it
// was measured with, else moved onto this plan and this beta by k_strat_remap.  beta = 0 on either side (nothing learned | an even
// allocation is asked for) starts uniform.
int strat_start_alloc(mci_problem *p, const std::vector<int> &ns, int64_t ncube, int64_t N) {
    auto &st = p->strat;
    const int D = (int)ns.size();
    const bool have = st.carry && st.c_valid && (int)st.c_nstrat.size() == D && st.c_beta > 0.0 && st.beta > 0.0;
    const bool same = have && st.c_nstrat == ns && st.c_beta == st.beta;
    const bool waiting = !st.c_host.empty(); // (the values of a state file, not on the device yet)
    int rc;
    if (!have) {
        if (st.c_host.empty() && st.c_nstrat != ns) st.c_valid = false; // (d_d is about to hold another plan's values)
        if ((rc = strat_reserve(p, ncube))) return rc;
        st.carry_how = 0;
    } else if (same) {
        if (waiting) {
            if ((rc = strat_reserve(p, ncube))) return rc;
            HIPCHK(hipMemcpyAsync(st.d_d, st.c_host.data(), (size_t)ncube * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream));
            HIPCHK(hipStreamSynchronize(p->ctx->stream));
        }
        st.carry_how = 1;
    } else {
        // new buffers first, old -> new, then the old ones go (hipFree waits for the kernel)
        double *src = st.d_d, *upload = nullptr, *d_new = nullptr;
        long long *off_new = nullptr;
        if ((rc = st.d_tsum.reserve(2 * 1024 + 2))) return rc;
        if (waiting) {
            HIPCHK(hipMalloc((void **)&upload, (size_t)st.c_ncube * sizeof(double)));
            if (hipMemcpyAsync(upload, st.c_host.data(), (size_t)st.c_ncube * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream) != hipSuccess ||
                hipStreamSynchronize(p->ctx->stream) != hipSuccess) {
                (void)hipFree(upload);
                return fail(MCI_ERR_HIP, "stratification: the carried d_h could not be copied to the device");
            }
            src = upload;
        }
        if (hipMalloc((void **)&off_new, (size_t)(ncube + 1) * sizeof(long long)) != hipSuccess ||
            hipMalloc((void **)&d_new, (size_t)ncube * sizeof(double)) != hipSuccess) {
            for (void *q : {(void *)upload, (void *)off_new, (void *)d_new})
                if (q) (void)hipFree(q);
            return fail(MCI_ERR_HIP, "stratification: no device memory for %lld hypercubes", (long long)ncube);
        }
        mci::StratRemapArgs a{};
        a.d_old = src;
        a.d_new = d_new;
        a.ncube = ncube;
        a.e = st.beta / st.c_beta;
        const hipError_t launched = strat_remap_launch(a, st.c_nstrat.data(), ns.data(), D, p->ctx->stream);
        if (upload) (void)hipFree(upload);
        st.d_off.adopt(off_new, ncube + 1);
        st.d_d.adopt(d_new, ncube);
        if (launched != hipSuccess) {
            st.c_valid = false;
            st.c_host.clear();
            st.nstrat.clear(); // (re-planned, uniform, at the next run)
            return fail(MCI_ERR_HIP, "stratification: k_strat_remap: %s", hipGetErrorString(launched));
        }
        st.carry_how = 2;
    }
    st.nstrat = ns;
    st.ncube = ncube;
    st.nsamp = N;
    if (have) { // d_d now holds the carried values on THIS plan, under this beta
        st.c_host.clear();
        st.c_host.shrink_to_fit();
        st.c_nstrat = ns;
        st.c_ncube = ncube;
        st.c_beta = st.beta;
    }
    if (st.hstart) { // test hook (mci_debug_strat_start_d)
        double *out = st.hstart;
        const int64_t n = st.hstart_n;
        st.hstart = nullptr;
        st.hstart_n = 0;
        if (n != ncube) return fail(MCI_ERR_INVALID, "mci_debug_strat_start_d: %lld values asked for, the plan has %lld hypercubes", (long long)n, (long long)ncube);
        if (have) {
            HIPCHK(hipMemcpyAsync(out, st.d_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
            HIPCHK(hipStreamSynchronize(p->ctx->stream));
        } else
            for (int64_t h = 0; h < n; ++h) out[h] = 1.0;
    }
    return strat_launch_alloc(p, !have);
}

// the plan for N samples per iteration; buffers sized for it; a new plan starts uniform, or from the carried d_h (strat_start_alloc)
int strat_prepare(mci_problem *p, int64_t N) {
    auto &st = p->strat;
    const int D = p->shape.ndraw;
    std::vector<int> ns(D);
    if (st.want.empty()) {
        int rc = mci_strat_plan(N, D, st.max_nhcube, ns.data());
        if (rc) return rc;
    } else ns = st.want;
    int64_t ncube = 1;
    for (int v : ns) {
        if (ncube > (((int64_t)1 << 31) - 1) / v) return fail(MCI_ERR_INVALID, "stratification: more than 2^31 - 1 hypercubes");
        ncube *= v;
    }
    if (ncube > N / 2) return fail(MCI_ERR_INVALID, "stratification: %lld hypercubes need at least %lld samples per iteration (two each), neval = %lld",
                                   (long long)ncube, (long long)(2 * ncube), (long long)N);
    const bool replan = ns != st.nstrat || N != st.nsamp;
    if (replan) st.ran = false;
    if (replan || !st.alloc_valid) return strat_start_alloc(p, ns, ncube, N);
    if (st.alloc_pending) return strat_launch_alloc(p, false);
    return MCI_OK;
}

} // namespace

static int compile_strat(mci_problem *p) {
    auto &st = p->strat;
    const int det = p->deterministic ? 1 : 0;
    KernelUnit &u = p->kernel[mci_problem::kStrat];
    if (u.compiled && st.compiled_det == det) return MCI_OK;
    u.drop();
    Candidate c;
    mcijit::ProblemShape sh = p->shape;
    sh.det = det;               // deterministic mode: one histogram copy per wave (mci_device.h hslot)
    sh.hcopy = det ? 256 / 64 : 1;
    c.unit = mcijit::kUnitStrat;
    c.src = mcijit::generate_source(sh, MCI_VEGAS, mcijit::kUnitStrat);
    c.threads = 256;
    if (c.build()) return c.failed(" (stratified :vegas kernel)");
    static const KernelUnit::Rules rules = {KernelUnit::kFail, false, "the stratified code object declares static LDS", ""};
    if (int rc = u.load(p->ctx, c, mcijit::kUnits[c.unit].kernel, 160 * 1024, rules)) return rc;
    st.compiled_det = det;
    return MCI_OK;
}

int mci_set_stratification(mci_problem *p, int32_t ndim, const int32_t *nstrat, double beta, int64_t max_nhcube) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(MCI_ERR_INVALID, "stratification: beta must be finite and >= 0");
    if (max_nhcube < 1 || max_nhcube > (((int64_t)1 << 31) - 1)) return fail(MCI_ERR_INVALID, "stratification: max_nhcube must lie in [1, 2^31 - 1]");
    int rc = strat_layout_check(p, ndim);
    if (rc) return rc;
    std::vector<int> want;
    if (nstrat) {
        int64_t prod = 1;
        for (int d = 0; d < ndim; ++d) {
            if (nstrat[d] < 1) return fail(MCI_ERR_INVALID, "stratification: nstrat[%d] = %d, must be >= 1", d, (int)nstrat[d]);
            prod *= nstrat[d];
            if (prod > (((int64_t)1 << 31) - 1)) return fail(MCI_ERR_INVALID, "stratification: more than 2^31 - 1 hypercubes");
            want.push_back(nstrat[d]);
        }
    }
    auto &st = p->strat;
    const bool keep = st.carry && st.c_valid && !st.last_run; // a carrying problem keeps its d_h, with the plan and beta it belongs to
    st.on = true;
    st.want = want;
    st.beta = beta;
    st.max_nhcube = max_nhcube;
    if (keep) { // (the next run starts its allocation from it: strat_start_alloc)
        st.alloc_valid = st.alloc_pending = false;
        return MCI_OK;
    }
    st.c_valid = false;
    st.c_host.clear();
    st.nstrat.clear(); // (re-planned, and the allocation started uniform, at the next run)
    st.nsamp = 0;
    st.ncube = 0;
    st.alloc_valid = st.alloc_pending = false;
    st.last_run = false;
    st.ran = false;
    return MCI_OK;
}

int mci_set_stratification_off(mci_problem *p) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    auto &st = p->strat;
    st.on = false;
    st.want.clear();
    st.nstrat.clear();
    st.c_valid = false; // (the carried d_h goes too)
    st.c_host.clear();
    st.carry_how = 0;
    st.ncube = st.nsamp = 0;
    st.alloc_valid = st.alloc_pending = false;
    st.last_run = false;
    st.ran = false;
    return MCI_OK;
}

int mci_set_stratification_carry(mci_problem *p, int32_t on) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (on != 0 && on != 1) return fail(MCI_ERR_INVALID, "stratification: carry must be 0 or 1");
    p->strat.carry = on != 0;
    return MCI_OK;
}

int mci_get_strat_carry(const mci_problem *p, int32_t *on, int32_t *how) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (on) *on = p->strat.carry ? 1 : 0;
    if (how) *how = p->strat.on ? p->strat.carry_how : 0;
    return MCI_OK;
}

int mci_get_stratification(const mci_problem *p, int32_t *nstrat, int64_t *ncube, double *beta) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    const auto &st = p->strat;
    if (nstrat)
        for (int d = 0; d < p->shape.ndraw; ++d) nstrat[d] = !st.on ? 0 : !st.nstrat.empty() ? st.nstrat[d] : !st.want.empty() ? st.want[d] : 0;
    if (ncube) *ncube = st.on ? st.ncube : 0;
    if (beta) *beta = st.beta;
    return MCI_OK;
}

int mci_get_strat_counts(mci_problem *p, int64_t *n_h, int64_t n) {
    if (!p || (n > 0 && !n_h)) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    const auto &st = p->strat;
    if (!st.on || !st.ran) return fail(MCI_ERR_INVALID, "stratification: no stratified iteration has run");
    if (n != st.ncube) return fail(MCI_ERR_INVALID, "stratification: %lld hypercubes, %lld asked for", (long long)st.ncube, (long long)n);
    HIPCHK(hipSetDevice(p->ctx->device));
    std::vector<long long> off((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(off.data(), st.d_off, off.size() * sizeof(long long), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    for (int64_t h = 0; h < n; ++h) n_h[h] = off[h + 1] - off[h];
    return MCI_OK;
}

int mci_debug_strat_dump(mci_problem *p, int64_t n, double *x, double *y, int64_t *h, double *jac, double *w) {
    if (!p || (n > 0 && (!x || !y || !h || !jac || !w))) return fail(MCI_ERR_INVALID, "NULL argument");
    auto &st = p->strat;
    st.hn = n > 0 ? n : 0;
    st.hx = x;
    st.hy = y;
    st.hh = (long long *)h;
    st.hjac = jac;
    st.hw = w;
    return MCI_OK;
}

int mci_debug_strat_d(mci_problem *p, double *d, int64_t n) {
    if (!p || (n > 0 && !d)) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    const auto &st = p->strat;
    if (!st.on || !st.ran || st.last_run) return fail(MCI_ERR_INVALID, "stratification: no stratified iteration has been finished");
    if (n != st.ncube) return fail(MCI_ERR_INVALID, "stratification: %lld hypercubes, %lld asked for", (long long)st.ncube, (long long)n);
    HIPCHK(hipSetDevice(p->ctx->device));
    HIPCHK(hipMemcpyAsync(d, st.d_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    return MCI_OK;
}

int mci_debug_strat_start_d(mci_problem *p, double *d, int64_t n) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    p->strat.hstart = n > 0 ? d : nullptr;
    p->strat.hstart_n = n > 0 && d ? n : 0;
    return MCI_OK;
}

// csrc/mci_debug.h: k_strat_alloc, k_strat_reduce and k_strat_remap alone over inputs the caller made up, launched by the helpers the
// product launches them with (strat_alloc_launches, strat_reduce_launch, strat_remap_launch); buffers of the hooks' own, nothing of the
// problem's but the device and the stream -- p->strat is neither read nor written
int mci_debug_strat_alloc(mci_problem *p, const double *d, int64_t ncube, int64_t nsamp, int32_t uniform, int64_t *off_out, double *tsum_out) {
    if (!p || !d || !off_out || !tsum_out) return fail(MCI_ERR_INVALID, "NULL argument");
    if (ncube < 1 || ncube > (((int64_t)1 << 31) - 1)) return fail(MCI_ERR_INVALID, "strat alloc: %lld hypercubes (1 .. 2^31 - 1)", (long long)ncube);
    if (nsamp < 2 * ncube || nsamp > ((int64_t)1 << 52))
        return fail(MCI_ERR_INVALID, "strat alloc: %lld samples for %lld hypercubes (two each at least, 2^52 at most)", (long long)nsamp, (long long)ncube);
    if (uniform != 0 && uniform != 1) return fail(MCI_ERR_INVALID, "strat alloc: uniform must be 0 or 1");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t hs = p->ctx->stream;
    const int ntile = strat_alloc_tiles(ncube);
    DevBuf<double> d_d, d_tsum;
    DevBuf<long long> d_off;
    int rc;
    if ((rc = d_d.reserve(ncube)) || (rc = d_off.reserve(ncube + 1)) || (rc = d_tsum.reserve(2 * ntile + 2))) return rc;
    HIPCHK(hipMemcpyAsync(d_d, d, (size_t)ncube * sizeof(double), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemsetAsync(d_off, 0xFF, (size_t)(ncube + 1) * sizeof(long long), hs)); // (an offset the kernel leaves unwritten comes back as
    HIPCHK(hipMemsetAsync(d_tsum, 0xFF, (size_t)(2 * ntile + 2) * sizeof(double), hs)); // -1, a scratch entry as NaN)
    HIPCHK(hipStreamSynchronize(hs)); // (the upload has read the caller's pageable memory)
    mci::StratAllocArgs a{};
    a.d = d_d;
    a.off = d_off;
    a.tsum = d_tsum;
    a.ncube = ncube;
    a.nsamp = nsamp;
    a.ntile = ntile;
    a.uniform = uniform;
    HIPCHK(strat_alloc_launches(a, hs));
    HIPCHK(hipMemcpyAsync(off_out, d_off, (size_t)(ncube + 1) * sizeof(long long), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipMemcpyAsync(tsum_out, d_tsum, (size_t)(2 * ntile + 2) * sizeof(double), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs)); // (the buffers are freed behind it)
    return MCI_OK;
}

int mci_debug_strat_reduce(mci_problem *p, const mci_debug_strat_reduce_io *io) {
    if (!p || !io || !io->off || !io->part || !io->rec_h || !io->rec_s || !io->dnext || !io->out) return fail(MCI_ERR_INVALID, "NULL argument");
    const int64_t ncube = io->ncube, nchunk = io->nchunk;
    const int nw = io->nw;
    if (ncube < 1 || ncube > (((int64_t)1 << 31) - 1)) return fail(MCI_ERR_INVALID, "strat reduce: %lld hypercubes (1 .. 2^31 - 1)", (long long)ncube);
    if (nchunk < 1 || nchunk > ((int64_t)1 << 24)) return fail(MCI_ERR_INVALID, "strat reduce: %lld chunks (1 .. 2^24)", (long long)nchunk);
    if (nw < 1 || nw > mci::kStratReduceCols) return fail(MCI_ERR_INVALID, "strat reduce: %d weight columns (1 .. %d)", nw, (int)mci::kStratReduceCols);
    if (!std::isfinite(io->beta) || io->beta < 0.0) return fail(MCI_ERR_INVALID, "strat reduce: beta must be finite and >= 0");
    for (int64_t i = 0; i < 2 * nchunk; ++i) // (the kernel reads off[h], off[h + 1] and writes dnext[h] of every record's h)
        if (io->rec_h[i] < -1 || io->rec_h[i] >= ncube)
            return fail(MCI_ERR_INVALID, "strat reduce: rec_h[%lld] = %lld, outside -1 .. %lld", (long long)i, (long long)io->rec_h[i], (long long)(ncube - 1));
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t hs = p->ctx->stream;
    DevBuf<long long> d_off, d_rec_h;
    DevBuf<double> d_part, d_rec_s, d_dnext, d_out, d_row;
    int rc;
    if ((rc = d_off.reserve(ncube + 1)) || (rc = d_rec_h.reserve(2 * nchunk)) || (rc = d_part.reserve(nchunk * 2 * nw)) || (rc = d_rec_s.reserve(nchunk * 4 * nw)) ||
        (rc = d_dnext.reserve(ncube)) || (rc = d_out.reserve(2 * nw)) || (rc = d_row.reserve(2 * nw)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_off, io->off, (size_t)(ncube + 1) * sizeof(long long), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemcpyAsync(d_rec_h, io->rec_h, (size_t)(2 * nchunk) * sizeof(long long), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemcpyAsync(d_part, io->part, (size_t)(nchunk * 2 * nw) * sizeof(double), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemcpyAsync(d_rec_s, io->rec_s, (size_t)(nchunk * 4 * nw) * sizeof(double), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemcpyAsync(d_dnext, io->dnext, (size_t)ncube * sizeof(double), hipMemcpyHostToDevice, hs)); // (the caller's fill: the sample kernel's part)
    HIPCHK(hipMemsetAsync(d_out, 0xFF, (size_t)(2 * nw) * sizeof(double), hs));
    HIPCHK(hipMemsetAsync(d_row, 0xFF, (size_t)(2 * nw) * sizeof(double), hs));
    HIPCHK(hipStreamSynchronize(hs));
    mci::StratReduceArgs r{};
    r.off = d_off;
    r.part = d_part;
    r.rec_h = d_rec_h;
    r.rec_s = d_rec_s;
    r.ncube = ncube;
    r.nchunk = nchunk;
    r.nw = nw;
    r.beta = io->beta;
    r.dnext = d_dnext;
    r.out = d_out;
    r.log_row = io->log_row ? d_row.get() : nullptr;
    HIPCHK(strat_reduce_launch(r, hs));
    HIPCHK(hipMemcpyAsync(io->dnext, d_dnext, (size_t)ncube * sizeof(double), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipMemcpyAsync(io->out, d_out, (size_t)(2 * nw) * sizeof(double), hipMemcpyDeviceToHost, hs));
    if (io->log_row) HIPCHK(hipMemcpyAsync(io->log_row, d_row, (size_t)(2 * nw) * sizeof(double), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    return MCI_OK;
}

int mci_debug_strat_remap(mci_problem *p, int32_t ndim, const int32_t *n_old, const int32_t *n_new, double e, const double *d_old, double *d_new_out) {
    if (!p || !n_old || !n_new || !d_old || !d_new_out) return fail(MCI_ERR_INVALID, "NULL argument");
    if (ndim < 1 || ndim > mci::kStratRemapMaxDraw) return fail(MCI_ERR_INVALID, "strat remap: %d draws (1 .. %d)", (int)ndim, (int)mci::kStratRemapMaxDraw);
    if (!std::isfinite(e)) return fail(MCI_ERR_INVALID, "strat remap: the exponent must be finite");
    int64_t c_old = 1, c_new = 1;
    for (int d = 0; d < ndim; ++d) {
        if (n_old[d] < 1 || n_new[d] < 1) return fail(MCI_ERR_INVALID, "strat remap: draw %d is cut into %d -> %d cells (each >= 1)", d, (int)n_old[d], (int)n_new[d]);
        c_old *= n_old[d];
        c_new *= n_new[d];
        if (c_old > (((int64_t)1 << 31) - 1) || c_new > (((int64_t)1 << 31) - 1)) return fail(MCI_ERR_INVALID, "strat remap: more than 2^31 - 1 hypercubes");
    }
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t hs = p->ctx->stream;
    DevBuf<double> d_src, d_dst;
    int rc;
    if ((rc = d_src.reserve(c_old)) || (rc = d_dst.reserve(c_new))) return rc;
    HIPCHK(hipMemcpyAsync(d_src, d_old, (size_t)c_old * sizeof(double), hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemsetAsync(d_dst, 0xFF, (size_t)c_new * sizeof(double), hs));
    HIPCHK(hipStreamSynchronize(hs));
    mci::StratRemapArgs a{};
    a.d_old = d_src;
    a.d_new = d_dst;
    a.ncube = c_new;
    a.e = e;
    std::vector<int> o(n_old, n_old + ndim), n(n_new, n_new + ndim);
    HIPCHK(strat_remap_launch(a, o.data(), n.data(), ndim, hs));
    HIPCHK(hipMemcpyAsync(d_new_out, d_dst, (size_t)c_new * sizeof(double), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    return MCI_OK;
}

// every stratified allocation of a call starts afresh (mci_integrate): uniform, or from the carried d_h (strat_start_alloc)
static void strat_call_start(mci_problem *p) { p->strat.alloc_valid = p->strat.alloc_pending = false; }

// One stratified :vegas iteration's sample launch + the histogram merge (mci_iteration_run's :vegas path for a stratified problem).
// The nwg partial rows are merged as the call's blocks (or one): the merged statistics head is overwritten with the stratified (mean,
// var) by mci_iteration_finish (strat_finish).
static int strat_run(mci_problem *p, int64_t nevalperblock, int64_t block_lo, int64_t block_hi, int32_t iteration, uint64_t seed, int64_t measurefreq) {
    auto &st = p->strat;
    const auto &s = p->shape;
    if (measurefreq != 1) return fail(MCI_ERR_INVALID, "stratification: measurefreq = %lld is refused (every sample is measured)", (long long)measurefreq);
    if (p->ctx->nranks != 1) return fail(MCI_ERR_INVALID, "stratification: more than one rank is refused");
    int rc = flush_merge(p);
    if (rc) return rc;
    if ((rc = compile_strat(p))) return rc;
    HIPCHK(hipSetDevice(p->ctx->device));
    const int64_t N = (block_hi - block_lo) * nevalperblock;
    if ((rc = strat_prepare(p, N))) return rc;
    const int T = 256, NW = s.ni * s.ncomp;
    const int64_t base = p->deterministic ? det_lds(p, T) : p->lds_bytes;
    const int64_t need[4] = {base + strat_chunk_lds_bytes(strat_nloc(8), NW), base + strat_chunk_lds_bytes(strat_nloc(4), NW), base + strat_chunk_lds_bytes(strat_nloc(2), NW),
                             base + strat_chunk_lds_bytes(strat_nloc(1), NW)};
    StratGeometry g;
    strat_geometry(N, block_hi - block_lo, need, g);
    if (!g.trips) return fail(MCI_ERR_INVALID, "stratification: the tables and the chunk's hypercubes do not fit one CU's LDS");
    const int64_t lds = g.lds, S = g.S, nchunk = g.nchunk, nwg = g.nwg, mblocks = g.mblocks;
    if ((rc = ensure_capacity(p, nwg, 1))) return rc;
    if ((rc = st.d_part.reserve(nchunk * 2 * NW)) || (rc = st.d_rec_s.reserve(nchunk * 2 * 2 * NW)) || (rc = st.d_rec_h.reserve(nchunk * 2)) ||
        (rc = st.d_stat.reserve(2 * mci::kStratMaxCols)))
        return rc;
    st.ran = true;
    st.last_nchunk = nchunk;

    mci::BatchArgs a{};
    fill_batch(p, a);
    a.seed = seed;
    a.iteration = (mci::u32)iteration;
    a.neval_per_block = nevalperblock;
    a.block_lo = block_lo;
    a.wg_per_block = (int)nwg;
    a.measurefreq = 1;
    a.nchain = 1;
    a.status = p->d_status;
    a.hist_atomic = 0;
    a.nrows = nwg;
    mci::StratArgs sa{};
    sa.off = st.d_off;
    sa.dnext = st.d_d;
    sa.part = st.d_part;
    sa.rec_h = st.d_rec_h;
    sa.rec_s = st.d_rec_s;
    sa.ncube = st.ncube;
    sa.nsamp = N;
    sa.chunk = S;
    sa.nchunk = nchunk;
    sa.first_index = block_lo * nevalperblock;
    sa.nloc = (int)(S / 2 + 1);
    sa.beta = st.beta;
    for (int d = 0; d < s.ndraw; ++d) {
        const uint32_t n = (uint32_t)st.nstrat[d];
        strat_magic(n, &sa.magic[d], &sa.shift[d]);
        sa.nstrat[d] = (int)n;
        sa.inv[d] = 1.0 / (double)n;
    }
    DevBuf<double> dump_x, dump_y, dump_jac, dump_w; // (test hook; freed on every way out)
    DevBuf<long long> dump_h;
    const bool dumping = st.hn > 0;
    if (dumping) {
        if (st.hn != N) return fail(MCI_ERR_INVALID, "mci_debug_strat_dump: %lld samples asked for, the iteration has %lld", (long long)st.hn, (long long)N);
        if ((rc = dump_x.reserve(N * s.ndraw)) || (rc = dump_y.reserve(N * s.ndraw)) || (rc = dump_h.reserve(N)) || (rc = dump_jac.reserve(N)) ||
            (rc = dump_w.reserve(N * NW)))
            return rc;
        sa.dump_x = dump_x;
        sa.dump_y = dump_y;
        sa.dump_h = dump_h;
        sa.dump_jac = dump_jac;
        sa.dump_w = dump_w;
    }
    void *args[] = {&a, &sa};
    // HIP events around the sample launch under the rule of the classic one (mci_set_kernel_timing, mci_kernel_times_ms)
    const int slot = (int)(p->launch.launches % mci_problem::kEvRing);
    p->launch.time_this_launch = p->kernel_timing > 0 || (p->kernel_timing < 0 && N >= ((int64_t)1 << 20));
    if (p->launch.time_this_launch) HIPCHK(hipEventRecord(p->evs[2 * slot], p->ctx->stream));
    HIPCHK(hipModuleLaunchKernel(p->kernel[mci_problem::kStrat].f, (unsigned)nwg, 1, 1, (unsigned)T, 1, 1, (unsigned)lds, p->ctx->stream, args, nullptr));
    if (p->launch.time_this_launch) HIPCHK(hipEventRecord(p->evs[2 * slot + 1], p->ctx->stream));
    p->launch.ev_valid[slot] = p->launch.time_this_launch;
    p->launch.clock_valid[slot] = false;
    p->launch.launches += 1;
    if (dumping) {
        hipStream_t hs = p->ctx->stream;
        HIPCHK(hipMemcpyAsync(st.hx, dump_x, (size_t)N * s.ndraw * sizeof(double), hipMemcpyDeviceToHost, hs));
        HIPCHK(hipMemcpyAsync(st.hy, dump_y, (size_t)N * s.ndraw * sizeof(double), hipMemcpyDeviceToHost, hs));
        HIPCHK(hipMemcpyAsync(st.hh, dump_h, (size_t)N * sizeof(long long), hipMemcpyDeviceToHost, hs));
        HIPCHK(hipMemcpyAsync(st.hjac, dump_jac, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, hs));
        HIPCHK(hipMemcpyAsync(st.hw, dump_w, (size_t)N * NW * sizeof(double), hipMemcpyDeviceToHost, hs));
        HIPCHK(hipStreamSynchronize(hs));
        st.hn = 0;
    }
    // merge: the nwg rows as mblocks blocks (the statistics head is replaced by the stratified estimate in strat_finish)
    if (s.nbin > 0)
        hipLaunchKernelGGL(mci::k_hist_stage1, hist_stage1_grid(s.nbin), dim3(256), 0, p->ctx->stream, p->d_part_hist, (int)nwg, s.nbin,
                           (int)mci_problem::kGroups, p->d_stage1);
    HIPCHK(hipGetLastError());
    p->merge = merge_args(p, mblocks, (int)(nwg / mblocks), nwg);
    p->merge_pending = true;
    record_launch(p, N, nwg, T, mblocks);
    st.last_run = true;
    return MCI_OK;
}

// behind launch_train of a stratified iteration: the stratified (mean, var) into the iteration log row (row[k], row[nobs + k]) and the
// d_h of the next allocation; when the map adapts, the next run turns them into its offsets first (strat_prepare), so that d_off keeps
// the allocation this iteration used until then (mci_get_strat_counts) and ONE offset array serves both
static int strat_finish(mci_problem *p, double *row, int32_t adapt) {
    auto &st = p->strat;
    st.last_run = false;
    mci::StratReduceArgs r{};
    r.off = st.d_off;
    r.part = st.d_part;
    r.rec_h = st.d_rec_h;
    r.rec_s = st.d_rec_s;
    r.ncube = st.ncube;
    r.nchunk = st.last_nchunk;
    r.nw = p->shape.ni * p->shape.ncomp;
    r.beta = st.beta;
    r.dnext = st.d_d;
    r.out = st.d_stat;
    r.log_row = row;
    HIPCHK(strat_reduce_launch(r, p->ctx->stream));
    st.alloc_pending = adapt != 0; // (adapt = false: the allocation the call started with stays)
    // d_d is now the d_h of a finished iteration of this plan: what a carrying problem starts its next call from
    st.c_valid = true;
    st.c_host.clear();
    if (st.c_nstrat != st.nstrat) st.c_nstrat = st.nstrat;
    st.c_ncube = st.ncube;
    st.c_beta = st.beta;
    return MCI_OK;
}

// (mean, std) of a stratified iteration log row
static void strat_mean_std(const double *row, int nobs, double *mean, double *std) {
    for (int o = 0; o < nobs; ++o) {
        mean[o] = row[o];
        std[o] = row[nobs + o] > 0.0 ? sqrt(row[nobs + o]) : 0.0;
    }
}
