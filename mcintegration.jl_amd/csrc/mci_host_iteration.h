// mci_host_iteration.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// one iteration: mci_iteration_run (validate, compile and gate, plan -- mci_host_plan.h --, the stages of the sample launch, record), reduce (the ONE all-reduce), finish (train!, doReweight!, statistics).
// ---------------------------------------------------------------------------------------------------
// one iteration
// ---------------------------------------------------------------------------------------------------
// ---- the stages of a sample launch, in the order mci_iteration_run goes through them.  Each takes the problem, the request, the plan and
// (where it fills any) the launch's BatchArgs; one that fails leaves the problem as it stands at that point ----------------------------

// partial rows, the chain solvers' propose | accept rows, the parked stream of a many-grid launch
static int reserve_launch_buffers(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl) {
    const auto &s = p->shape;
    int rc = ensure_capacity(p, pl.nrows, rq.nblocks);
    if (!rc && rq.solver != MCI_VEGAS) rc = p->d_part_pa.reserve(pl.nrows * 2 * p->npa);
    if (rc || !pl.split) return rc;
    const int64_t words = p->tdraw_words > 0 ? p->tdraw_words : 1, bytes = parked_bytes_per_sample(p);
    const int64_t nsamp = rq.nblocks * pl.chunk_len;
    if (nsamp > p->cap_tile) {
        tile_release(p);
        const size_t wbytes = (((size_t)nsamp * s.ni * sizeof(double)) + 255) & ~(size_t)255; // (the bins start 256-byte aligned: 16-byte loads)
        if ((rc = tile_alloc(p, wbytes + (size_t)nsamp * words * sizeof(uint32_t)))) return rc;
        p->d_tile_bins = (uint32_t *)((char *)p->d_tile_w + wbytes);
        p->cap_tile = nsamp;
    }
    p->launch.last_split_chunks = pl.nchunks;
    p->launch.last_split_bytes = nsamp * bytes;
    return MCI_OK;
}

// what every launch of the plan is given: the tables and the request ...
static mci::BatchArgs request_args(const mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl) {
    mci::BatchArgs a{};
    fill_batch(p, a);
    a.part_pa = p->d_part_pa;
    a.seed = rq.seed;
    a.iteration = (mci::u32)rq.iteration;
    a.neval_per_block = rq.nevalperblock;
    a.block_lo = rq.block_lo;
    a.wg_per_block = pl.wpb;
    a.measurefreq = rq.measurefreq;
    a.nchain = pl.nchain;
    a.burnin = pl.burnin;
    a.nburn = pl.nburn;
    a.hist_atomic = pl.ghist_buffers;
    return a;
}

// ... and, for the sample launches, where they report and the geometry (not for the carry-weights launch, which is given a copy of `a`
// as it stands before this)
static void geometry_args(const mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    a.status = p->d_status;
    a.tile_w = p->d_tile_w;
    a.tile_bins = p->d_tile_bins;
    a.tile_stride = rq.nblocks * pl.chunk_len;
    a.chunk_lo = 0;
    a.chunk_hi = rq.nevalperblock;
    a.chunk_len = pl.chunk_len;
    a.accum = 0;
    a.nrows = pl.nrows;
    if (pl.tiles_wpb) {
        a.tiles_wpb = pl.tiles_wpb;
        a.tiles_rows = pl.hist_rows;
    }
}

// chain solvers: the stored chains this launch continues (resampled to the moved target), the buffers it stores its own in, and the
// record of what they are (launch.chain_*)
static int prepare_carried_chains(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    const auto &s = p->shape;
    const bool carry_on = p->chain_carry != 0;
    int rc;
    const bool carried = pl.carried();
    const bool keep = carry_on && pl.nchain > 1;
    if (keep && p->in_self_check) return fail(MCI_ERR_INVALID, "the self-check's launch would overwrite the stored chains");
    if (carried) {
        a.carry_x = p->d_chain_x[p->launch.chain_cur];
        a.carry_curr = p->d_chain_curr[p->launch.chain_cur];
        a.carry_nchain = p->launch.chain_nchain;
        a.carry_cap = p->chain_stride(p->launch.chain_cur);
    }
    if (carried) { // which stored chain each chain continues: the stored ones resampled to the moved target
        if ((rc = p->d_carry_src.reserve(rq.nblocks * pl.nchain)) || (rc = p->d_carry_W.reserve(rq.nblocks * p->launch.chain_nchain))) return rc;
        mci::ResampleArgs ra{};
        ra.curr_old = p->d_chain_curr[p->launch.chain_cur];
        ra.n_old = p->launch.chain_nchain;
        ra.n_new = pl.nchain;
        ra.nd = p->ni + 1;
        ra.rw_now = p->d_reweight;
        ra.rw_used = p->d_reweight_used;
        ra.src = p->d_carry_src;
        ra.W = p->d_carry_W;
        if (rq.solver == MCI_VEGASMC) {
            // :vegasmc: the target itself moved with the map and the reweight factors -- pi_new / pi_old at every stored configuration
            // (the chain kernel's own code object evaluates it: relocate, integrand, paddings), then the same systematic resampling
            const int64_t total = rq.nblocks * p->launch.chain_nchain;
            if ((rc = p->d_carry_w.reserve(total))) return rc;
            a.carry_P = p->d_chain_P[p->launch.chain_cur];
            a.carry_w = p->d_carry_w;
            a.carry_total = total;
            mci::BatchArgs wa = a; // (edges, tables, reweight, userdata and the carry fields; everything else unused)
            // a host closure: evaluated at the stored configurations here, one more callback per iteration
            DevBuf<double> d_cw; // (freed on every way out of this block, the failing ones included)
            if (s.host_integrand) {
                const int nw = s.ni * s.ncomp;
                std::vector<double> hx((size_t)total * s.ndraw), hw((size_t)total * nw);
                for (int k = 0; k < s.ndraw; ++k)
                    HIPCHK(hipMemcpyAsync(hx.data() + (size_t)k * total, a.carry_x + (size_t)k * a.carry_cap, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
                HIPCHK(hipStreamSynchronize(p->ctx->stream));
                if ((rc = eval_host_integrand(p, nullptr, hx.data(), hw.data(), total))) return rc;
                if ((rc = d_cw.reserve((int64_t)hw.size()))) return rc;
                HIPCHK(hipMemcpyAsync(d_cw, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream));
                HIPCHK(hipStreamSynchronize(p->ctx->stream)); // (`hw` leaves scope)
                wa.host_w = d_cw;
            }
            void *wargs[] = {&wa};
            const int64_t wgrid = (total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048;
            const int tw = pl.G > 1 ? 256 : (pl.T < 256 ? pl.T : 256); // (within the launch bound its code object was compiled for)
            HIPCHK(hipModuleLaunchKernel(p->f_carryw[pl.G > 1 ? 1 : 0], (unsigned)wgrid, 1, 1, (unsigned)tw, 1, 1, (unsigned)p->lds_bytes, p->ctx->stream, wargs, nullptr));
            if (d_cw) HIPCHK(hipStreamSynchronize(p->ctx->stream)); // (the kernel has read it before `d_cw` lets go of it)
            ra.w_chain = p->d_carry_w;
        }
        hipLaunchKernelGGL(mci::k_resample_chains, dim3((unsigned)rq.nblocks), dim3(256), 0, p->ctx->stream, ra);
        HIPCHK(hipGetLastError());
        a.carry_src = p->d_carry_src;
    }
    if (keep && rq.solver == MCI_MCMC) { // the reweight factors this launch's chains run under (doReweight! moves them behind it)
        if ((rc = p->d_reweight_used.reserve(p->ni + 1))) return rc;
        HIPCHK(hipMemcpyAsync(p->d_reweight_used, p->d_reweight, (size_t)(p->ni + 1) * sizeof(double), hipMemcpyDeviceToDevice, p->ctx->stream));
    }
    if (keep) {
        const int wb = p->launch.chain_valid ? 1 - p->launch.chain_cur : p->launch.chain_cur;
        const int64_t need = rq.nblocks * pl.nchain;
        if ((rc = p->d_chain_x[wb].reserve(need * s.ndraw)) || (rc = p->d_chain_curr[wb].reserve(need)) || (rc = p->d_chain_P[wb].reserve(need))) return rc;
        a.store_x = p->d_chain_x[wb];
        a.store_curr = p->d_chain_curr[wb];
        a.store_P = rq.solver == MCI_VEGASMC ? p->d_chain_P[wb].get() : nullptr;
        a.store_cap = p->chain_stride(wb);
        p->launch.chain_cur = wb;
        p->launch.chain_valid = true;
        p->launch.chain_ntrain = p->ntrain;
        p->launch.chain_solver = rq.solver;
        p->launch.chain_iteration = rq.iteration;
        p->launch.chain_lo = rq.block_lo;
        p->launch.chain_hi = rq.block_hi;
        p->launch.chain_nchain = pl.nchain;
    } else {
        p->launch.chain_valid = false;
    }
    p->launch.last_carried = carried;
    return MCI_OK;
}

// csrc/mci_debug.h: k_resample_chains alone, over chains the caller made up, launched as above; buffers of its own, nothing of the
// problem's but the device and the stream
int mci_debug_resample(mci_problem *p, int64_t nblocks, int64_t n_old, int64_t n_new, int32_t nd, const int32_t *curr_old, const double *rw_now,
                       const double *rw_used, const double *w_chain, int32_t *src, double *W) {
    if (!p || !src || (!w_chain && (!curr_old || !rw_now || !rw_used))) return fail(MCI_ERR_INVALID, "NULL argument");
    if (nblocks < 1 || n_old < 1 || n_new < 1) return fail(MCI_ERR_INVALID, "resample: %lld blocks of %lld stored and %lld new chains (each >= 1)", (long long)nblocks, (long long)n_old, (long long)n_new);
    if (nd < 1 || nd > 64) return fail(MCI_ERR_INVALID, "resample: %d integrands (1 .. 64)", (int)nd);
    if (n_old > INT32_MAX || n_new > INT32_MAX || nblocks > INT32_MAX / n_old || nblocks > INT32_MAX / n_new)
        return fail(MCI_ERR_INVALID, "resample: %lld blocks of %lld stored and %lld new chains are more than a test hook takes", (long long)nblocks, (long long)n_old, (long long)n_new);
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    const size_t told = (size_t)nblocks * (size_t)n_old, tnew = (size_t)nblocks * (size_t)n_new;
    DevBuf<int> d_curr, d_src;
    DevBuf<double> d_rw, d_w, d_W;
    int rc;
    if ((rc = d_src.reserve((int64_t)tnew)) || (rc = d_W.reserve((int64_t)told))) return rc;
    HIPCHK(hipMemsetAsync(d_src, 0xFF, tnew * sizeof(int), st)); // (a pick the kernel does not write comes back as -1, a running weight it
    HIPCHK(hipMemsetAsync(d_W, 0xFF, told * sizeof(double), st)); // does not write, or adds to what was there, as NaN)
    mci::ResampleArgs ra{};
    if (curr_old) {
        if ((rc = d_curr.reserve((int64_t)told))) return rc;
        HIPCHK(hipMemcpyAsync(d_curr, curr_old, told * sizeof(int), hipMemcpyHostToDevice, st));
        ra.curr_old = d_curr;
    }
    if (rw_now && rw_used) {
        if ((rc = d_rw.reserve(2 * (int64_t)nd))) return rc;
        HIPCHK(hipMemcpyAsync(d_rw, rw_now, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_rw + nd, rw_used, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));
        ra.rw_now = d_rw;
        ra.rw_used = d_rw + nd;
    }
    if (w_chain) {
        if ((rc = d_w.reserve((int64_t)told))) return rc;
        HIPCHK(hipMemcpyAsync(d_w, w_chain, told * sizeof(double), hipMemcpyHostToDevice, st));
        ra.w_chain = d_w;
    }
    ra.n_old = n_old;
    ra.n_new = n_new;
    ra.nd = nd;
    ra.src = d_src;
    ra.W = d_W;
    HIPCHK(hipStreamSynchronize(st)); // (the uploads have read the caller's pageable memory)
    hipLaunchKernelGGL(mci::k_resample_chains, dim3((unsigned)nblocks), dim3(256), 0, st, ra);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(src, d_src, tnew * sizeof(int), hipMemcpyDeviceToHost, st));
    if (W) HIPCHK(hipMemcpyAsync(W, d_W, told * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // (the buffers are freed behind it)
    return MCI_OK;
}

// the :mcmc holding-time histogram, the speculation trees of a several-lanes-per-chain launch
static int prepare_chain_tables(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    const auto &s = p->shape;
    if (rq.solver == MCI_MCMC && !s.host_integrand && rq.nevalperblock / pl.nchain + pl.nburn < ((int64_t)1 << 31) - 1) {
        if (int rc = p->d_hold.reserve(64)) return rc;
        HIPCHK(hipMemsetAsync(p->d_hold, 0, 64 * sizeof(unsigned long long), p->ctx->stream));
        a.hold_hist = p->d_hold;
    }
    if (pl.G > 1) {
        a.spec_tab = p->d_spec_tab;
        a.spec_lanes = pl.G;
        a.spec_maxacc = pl.spec_maxacc;
        a.spec_ntree = p->spec_ntree;
        a.spec_first = p->spec_first;
        for (int k = 0; k < 8; ++k) a.spec_accept[k] = p->spec_accepts[k];
    }
    return MCI_OK;
}

static int prepare_host_integrand(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    const auto &s = p->shape;
    int rc;
    // "batch callback": the closure cannot run on the device, so the draws of this launch go to the host (SoA,
    // x[k*n + i]), the callback fills w[q*n + i], and the sample kernel regenerates the same draws (same Philox
    // indices) around the uploaded weights.  PCIe + host bound by construction; solver = :vegas only.
    if (rq.solver != MCI_VEGAS && s.ntile > 1) return fail(MCI_ERR_INVALID, "a host integrand under a chain solver needs the histograms in one LDS tile");
    // :vegas -- the draws of the whole launch; chain solvers -- one configuration per chain and Markov step (below)
    const int64_t n = rq.solver == MCI_VEGAS ? rq.nblocks * rq.nevalperblock : rq.nblocks * pl.nchain;
    if ((double)n * (double)(s.ndraw + s.ni * s.ncomp) * 8.0 > 8.0 * 1024 * 1024 * 1024)
        return fail(MCI_ERR_INVALID, "a host integrand over %lld configurations of %d doubles per launch (more than 8 GiB): lower neval or "
                                     "give the integrand as device source (mci_set_integrand_source)", (long long)n, s.ndraw + s.ni * s.ncomp);
    if ((rc = p->d_hx.reserve(n * s.ndraw)) || (rc = p->d_hw.reserve(n * s.ni * s.ncomp)) || (rc = p->h_hx.reserve(n * s.ndraw)) ||
        (rc = p->h_hw.reserve(n * s.ni * s.ncomp)))
        return rc;
    if (rq.solver == MCI_VEGAS) {
    mci::DumpArgs d{};
    fill_tables(p, d);
    d.ud = p->d_ud;
    d.x = p->d_hx;
    d.soa = 1;
    d.seed = rq.seed;
    d.iteration = (mci::u32)rq.iteration;
    d.first_index = rq.block_lo * rq.nevalperblock;
    d.n = n;
    void *dargs[] = {&d};
    const unsigned dgrid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipStream_t hs = p->ctx->stream;
    HIPCHK(hipModuleLaunchKernel(p->kernel[kSlotDump].f, dgrid, 1, 1, 256, 1, 1, (unsigned)p->lds_bytes, hs, dargs, nullptr));
    HIPCHK(hipMemcpyAsync(p->h_hx, p->d_hx, (size_t)n * s.ndraw * sizeof(double), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    if ((rc = eval_host_integrand(p, nullptr, p->h_hx, p->h_hw, n))) return rc;
    HIPCHK(hipMemcpyAsync(p->d_hw, p->h_hw, (size_t)n * s.ni * s.ncomp * sizeof(double), hipMemcpyHostToDevice, hs));
    }
    a.host_w = p->d_hw;
    return MCI_OK;
}

// host measure: the records' buffers, preset
static int prepare_host_measure(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    const auto &s = p->shape;
    const int nw = s.ni * s.ncomp;
    const int64_t n = rq.nblocks * pl.hm_n > 0 ? rq.nblocks * pl.hm_n : 1;
    // every record crosses PCIe and sits in pinned host memory: refuse launches whose records would not reasonably fit
    if ((double)n * (double)(s.ndraw + nw + 1) * 8.0 > 8.0 * 1024 * 1024 * 1024)
        return fail(MCI_ERR_INVALID, "a host measure over %lld records of %d doubles per launch (more than 8 GiB): lower neval, raise measurefreq "
                                     "or give the measure as device source (mci_set_measure_source)", (long long)n, s.ndraw + nw);
    int rc;
    if ((rc = p->d_mx.reserve(n * s.ndraw)) || (rc = p->d_mrelw.reserve(n * nw)) || (rc = p->d_midx.reserve(n)) || (rc = p->h_mx.reserve(n * s.ndraw)) ||
        (rc = p->h_mrelw.reserve(n * nw)) || (rc = p->h_midx.reserve(n)) || (rc = p->d_mobs.reserve(rq.nblocks * s.nobs)))
        return rc;
    a.host_mx = p->d_mx;
    a.host_relw = p->d_mrelw;
    a.host_midx = p->d_midx;
    a.hm_first = pl.hm_first;
    a.hm_count = pl.hm_count;
    a.hm_stride = rq.nblocks * pl.hm_n;
    if (rq.solver != MCI_VEGAS) { // a chain on the normalization integrand leaves no record (:mcmc): preset "none"
        HIPCHK(hipMemsetAsync(p->d_mx, 0, (size_t)n * s.ndraw * sizeof(double), p->ctx->stream));
        HIPCHK(hipMemsetAsync(p->d_mrelw, 0, (size_t)n * pl.hm_rows * sizeof(double), p->ctx->stream));
        HIPCHK(hipMemsetAsync(p->d_midx, 0xFF, (size_t)n * sizeof(int32_t), p->ctx->stream));
    }
    return MCI_OK;
}

// the cursor words of this launch's blocks, and where they stand
static int prepare_cursor(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    mci::CursorRule r;
    r.units = (mci::u64)((rq.nevalperblock + 127) >> 7);
    r.waves = (mci::u32)(pl.wpb * (pl.T / 64));
    r.log2_big = (mci::u32)(g_over.cursor_log2_big.on && g_over.cursor_log2_big.v >= 1 && g_over.cursor_log2_big.v <= 16 ? g_over.cursor_log2_big.v : mci_problem::kCursorLog2Big);
    r.ones = (mci::u32)(g_over.cursor_ones.on && g_over.cursor_ones.v >= 1 && g_over.cursor_ones.v <= 4096 ? g_over.cursor_ones.v : mci_problem::kCursorOnes);
    // the words of this launch's blocks all stand at cursor_base: a launch over another number of blocks starts a new set (the only
    // time anything is cleared; the words only grow and 64 bits do not wrap)
    if (rq.nblocks != p->cursor_nblocks) {
        if (int rc = p->d_cursor.reserve(rq.nblocks * mci::kCursorStride)) return rc;
        HIPCHK(hipMemsetAsync(p->d_cursor, 0, (size_t)rq.nblocks * mci::kCursorStride * sizeof(unsigned long long), p->ctx->stream));
        p->cursor_nblocks = rq.nblocks;
        p->cursor_base = 0;
    }
    a.cursor = p->d_cursor;
    a.cursor_base = p->cursor_base;
    a.cursor_log2_big = r.log2_big;
    a.cursor_ones = r.ones;
    p->cursor_base += mci::cursor_tickets(r) + r.waves; // every wave stops at its first ticket beyond the last range
    return MCI_OK;
}

// The closure sits inside the Markov step (vegas_mc/updates.jl:67-75, mcmc/updates.jl:35-38): the chains of this launch advance
// in lock step, one kernel launch per step; each hands the host the nc configurations to evaluate and takes their weights back
// (vegasmc_host_step, mcmc_host_step).  PCIe- and host-bound by construction: two copies, one callback and one launch per step.
static int launch_host_closure_steps(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a, hipFunction_t f) {
    const auto &s = p->shape;
    hipStream_t st = p->ctx->stream;
    void *args[] = {&a};
    int rc;
    const int64_t nc = rq.nblocks * pl.nchain, steps = rq.nevalperblock / pl.nchain;
    const int nw = s.ni * s.ncomp, nd = s.ndraw;
    if (nc >= ((int64_t)1 << 31) || steps + pl.nburn >= ((int64_t)1 << 31) - 1) return fail(MCI_ERR_INVALID, "too many chains or steps for the host-closure path");
    // doubles: cx, cprob, pprob [nd] each; cw [nw]; cprobability, pprop, puacc, cwabs; ints: cbin, pbin [nd] each; pvi, ccurr, cit, ctr, pnew, put, hidx; done
    if ((rc = p->d_hstep.reserve(nc * (int64_t)((3 * nd + nw + 4) * sizeof(double) + (2 * nd + 7) * sizeof(int)) + 16)) || (rc = p->h_hidx.reserve(nc + 1))) return rc;
    {
        double *dp = (double *)p->d_hstep.get();
        a.hs.cx = dp; dp += (size_t)nd * nc;
        a.hs.cprob = dp; dp += (size_t)nd * nc;
        a.hs.pprob = dp; dp += (size_t)nd * nc;
        a.hs.cw = dp; dp += (size_t)nw * nc;
        a.hs.cprobability = dp; dp += nc;
        a.hs.pprop = dp; dp += nc;
        a.hs.puacc = dp; dp += nc;
        a.hs.cwabs = dp; dp += nc;
        int *ip = (int *)dp;
        a.hs.cbin = ip; ip += (size_t)nd * nc;
        a.hs.pbin = ip; ip += (size_t)nd * nc;
        a.hs.pvi = ip; ip += nc;
        a.hs.ccurr = ip; ip += nc;
        a.hs.cit = ip; ip += nc;
        a.hs.ctr = ip; ip += nc;
        a.hs.pnew = ip; ip += nc;
        a.hs.put = ip; ip += nc;
        a.hs.hidx = ip; ip += nc; // (hidx[nc] = done: one copy brings both back)
        a.hs.done = ip;
    }
    a.hs.hx = p->d_hx;
    a.hs.nc = nc;
    a.hs.steps = steps;
    // the step launches ADD to the partial rows
    HIPCHK(hipMemsetAsync(p->d_part_cols, 0, (size_t)pl.nrows * s.ncols * sizeof(double), st));
    if (pl.hist_lds && s.nbin > 0) HIPCHK(hipMemsetAsync(p->d_part_hist, 0, (size_t)pl.nrows * s.nbin * sizeof(double), st));
    HIPCHK(hipMemsetAsync(p->d_part_pa, 0, (size_t)pl.nrows * 2 * p->npa * sizeof(double), st));
    HIPCHK(hipMemsetAsync(a.hs.done, 0, sizeof(int), st));
    if (rq.solver == MCI_VEGASMC) {
        for (int64_t ne = 0; ne <= steps + 1; ++ne) {
            a.hs.ne = ne;
            HIPCHK(hipModuleLaunchKernel(f, (unsigned)pl.nwg, 1, 1, (unsigned)pl.T, 1, 1, (unsigned)solver_lds(p, rq.solver), st, args, nullptr));
            if (ne > steps) break;
            HIPCHK(hipMemcpyAsync(p->h_hx, p->d_hx, (size_t)nc * nd * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if ((rc = eval_host_integrand(p, nullptr, p->h_hx, p->h_hw, nc))) return rc;
            HIPCHK(hipMemcpyAsync(p->d_hw, p->h_hw, (size_t)nc * nw * sizeof(double), hipMemcpyHostToDevice, st));
        }
    } else {
        // every chain counts its own steps (a start that has to be redrawn costs a launch): launch until all of them are through
        const int64_t limit = steps + pl.nburn + 2 + 10000; // (mcmc/montecarlo.jl:118: at most 10000 tries of the start)
        for (int64_t ne = 0;; ++ne) {
            a.hs.ne = ne;
            HIPCHK(hipModuleLaunchKernel(f, (unsigned)pl.nwg, 1, 1, (unsigned)pl.T, 1, 1, (unsigned)solver_lds(p, rq.solver), st, args, nullptr));
            HIPCHK(hipMemcpyAsync(p->h_hidx, a.hs.hidx, (size_t)(nc + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(p->h_hx, p->d_hx, (size_t)nc * nd * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (p->h_hidx[nc] >= nc) break;
            if (ne > limit) return fail(MCI_ERR_INVALID, "host-closure :mcmc chains did not finish (%d of %lld)", (int)p->h_hidx[nc], (long long)nc);
            if ((rc = eval_host_integrand(p, p->h_hidx, p->h_hx, p->h_hw, nc))) return rc;
            HIPCHK(hipMemcpyAsync(p->d_hw, p->h_hw, (size_t)nc * s.ncomp * sizeof(double), hipMemcpyHostToDevice, st));
        }
    }
    return MCI_OK;
}

// the replay of a chunk's parked samples into the other histogram tiles
static int launch_replay(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a) {
    const auto &s = p->shape;
    void *args[] = {&a};
    HIPCHK(hipModuleLaunchKernel(p->f_tiles[rq.kern == kSlotVegasAny ? 1 : 0], (unsigned)(((pl.hist_rows + 7) / 8) * 8 * (s.ntile - (s.split_all ? 0 : 1))), 1, 1, (unsigned)pl.T, 1, 1, (unsigned)p->lds_bytes, p->ctx->stream, args, nullptr));
    return MCI_OK;
}

// the sample launch, chunk by chunk; the replay of every chunk but the last (that one follows the holding-time hand-over)
static int launch_sample_chunks(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, mci::BatchArgs &a, hipFunction_t f) {
    hipStream_t st = p->ctx->stream;
    void *args[] = {&a};
    int rc;
    for (int64_t c = 0; c < pl.nchunks; ++c) { // (one trip, except for a many-grid launch whose parked stream is bounded: sample pass -> replay per chunk)
        if (pl.nchunks > 1) {
            a.chunk_lo = c * pl.chunk_len;
            a.chunk_hi = a.chunk_lo + pl.chunk_len < rq.nevalperblock ? a.chunk_lo + pl.chunk_len : rq.nevalperblock;
            a.accum = c > 0 ? 1 : 0;
        }
        HIPCHK(hipModuleLaunchKernel(f, (unsigned)pl.nwg, 1, 1, (unsigned)pl.T_launch, 1, 1, (unsigned)plan_launch_lds(p, rq), st, args, nullptr));
        if (pl.split && c + 1 < pl.nchunks && (rc = launch_replay(p, rq, pl, a))) return rc;
    }
    return MCI_OK;
}

static int finish_host_measure(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl) {
    const auto &s = p->shape;
    hipStream_t st = p->ctx->stream;
    // the closure cannot run on the device: this launch's (measured) configurations and relative weights go to the host
    // (draw-major, like the host integrand path), the callback accumulates block b's observables from block b's records, and
    // they join the block's partial row before the merge.  PCIe- and host-bound by construction.
    const int64_t n = rq.nblocks * pl.hm_n;
    const int nw = s.ni * s.ncomp, nc = s.ncomp;
    std::vector<double> obs((size_t)rq.nblocks * s.nobs, 0.0);
    // (the self-check of a new several-lanes-per-chain code object, spec_self_check, never calls the USER's closure: its two small
    // launches compare histograms, normalisation, visits and acceptance tables; the observables stay zero in both)
    if (n > 0 && !p->in_self_check) {
        HIPCHK(hipMemcpyAsync(p->h_mx, p->d_mx, (size_t)n * s.ndraw * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(p->h_mrelw, p->d_mrelw, (size_t)n * pl.hm_rows * sizeof(double), hipMemcpyDeviceToHost, st));
        if (rq.solver == MCI_MCMC) HIPCHK(hipMemcpyAsync(p->h_midx, p->d_midx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const double *relw = p->h_mrelw;
        if (rq.solver == MCI_MCMC && p->hmeas_fn) { // plain form: every integrand's row, zero except the one the chain sat on
            p->h_mtmp.assign((size_t)n * nw, 0.0);
            for (int64_t i = 0; i < n; ++i)
                if (p->h_midx[i] >= 0)
                    for (int q = 0; q < nc; ++q) p->h_mtmp[(size_t)(p->h_midx[i] * nc + q) * n + i] = p->h_mrelw[(size_t)q * n + i];
            relw = p->h_mtmp.data();
        }
        if (rq.solver != MCI_MCMC && p->hmeas_idx_fn) p->h_mitmp.resize((size_t)pl.hm_n);
        // :vegas calls `measure` for the samples with (ne % measurefreq == 0) only (vegas/montecarlo.jl:148-165): the records the
        // cadence skips are squeezed out on the host, so that a measure which is not linear in the weights (a visit count, a
        // per-call bin count) sees exactly the calls the reference makes
        const bool squeeze = rq.solver == MCI_VEGAS && rq.measurefreq > 1;
        const int64_t keep = squeeze ? rq.nevalperblock / rq.measurefreq : pl.hm_n;
        std::vector<double> sx, sw;
        if (squeeze) {
            sx.resize((size_t)(keep > 0 ? keep : 1) * s.ndraw);
            sw.resize((size_t)(keep > 0 ? keep : 1) * nw);
        }
        for (int64_t b = 0; b < rq.nblocks; ++b) {
            const int64_t off = b * pl.hm_n;
            double *ob = obs.data() + (size_t)b * s.nobs;
            int hrc = 0;
            if (squeeze) {
                for (int k = 0; k < s.ndraw; ++k)
                    for (int64_t j = 0; j < keep; ++j) sx[(size_t)k * keep + j] = p->h_mx[(size_t)k * n + off + (j + 1) * rq.measurefreq - 1];
                for (int q = 0; q < nw; ++q)
                    for (int64_t j = 0; j < keep; ++j) sw[(size_t)q * keep + j] = relw[(size_t)q * n + off + (j + 1) * rq.measurefreq - 1];
                if (p->hmeas_fn) hrc = p->hmeas_fn(sx.data(), sw.data(), keep, keep, s.ndraw, nw, rq.block_lo + b, ob, s.nobs, p->hmeas_user);
                else {
                    p->h_mitmp.resize((size_t)(keep > 0 ? keep : 1));
                    for (int j = 0; j < s.ni && !hrc; ++j) {
                        std::fill(p->h_mitmp.begin(), p->h_mitmp.end(), (int32_t)j);
                        hrc = p->hmeas_idx_fn(p->h_mitmp.data(), sx.data(), sw.data() + (size_t)j * nc * keep, keep, keep, s.ndraw, nc, rq.block_lo + b, ob,
                                              s.nobs, p->hmeas_user);
                    }
                }
            } else if (p->hmeas_fn) {
                hrc = p->hmeas_fn(p->h_mx + off, relw + off, pl.hm_n, n, s.ndraw, nw, rq.block_lo + b, ob, s.nobs, p->hmeas_user);
            } else if (rq.solver == MCI_MCMC) {
                hrc = p->hmeas_idx_fn(p->h_midx + off, p->h_mx + off, relw + off, pl.hm_n, n, s.ndraw, nc, rq.block_lo + b, ob, s.nobs, p->hmeas_user);
            } else { // indexed form under :vegas / :vegasmc: every integrand in turn
                for (int j = 0; j < s.ni && !hrc; ++j) {
                    std::fill(p->h_mitmp.begin(), p->h_mitmp.end(), (int32_t)j);
                    hrc = p->hmeas_idx_fn(p->h_mitmp.data(), p->h_mx + off, relw + (size_t)j * nc * n + off, pl.hm_n, n, s.ndraw, nc, rq.block_lo + b, ob,
                                          s.nobs, p->hmeas_user);
                }
            }
            if (hrc) return fail(MCI_ERR_INVALID, "the host measure failed (%d)", hrc);
        }
    }
    HIPCHK(hipMemcpyAsync(p->d_mobs, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mci::k_add_host_obs, dim3((unsigned)((rq.nblocks * s.nobs + 255) / 256)), dim3(256), 0, st, p->d_mobs, (int)rq.nblocks, s.nobs, s.ncols, pl.wpb,
                       p->d_part_cols);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st)); // `obs` leaves scope
    return MCI_OK;
}

// merge: block sums -> packed (queued lazily: merge_pending)
static int queue_merge(mci_problem *p, const LaunchRequest &rq, const LaunchPlan &pl, const unsigned long long *hold_hist) {
    const auto &s = p->shape;
    hipStream_t st = p->ctx->stream;
    int rc;
    // (reading a few partial rows directly in the second stage instead -- no first-stage launch when an iteration is launch-bound --
    // was measured at neval = 1e4: k_finish grows by what the launch took, 26 us per iteration either way)
    if (pl.hist_lds && s.nbin > 0 && !pl.atomic_flush)
        hipLaunchKernelGGL(mci::k_hist_stage1, hist_stage1_grid(s.nbin), dim3(256), 0, st, p->d_part_hist, (int)pl.hist_rows, s.nbin,
                           (int)mci_problem::kGroups, p->d_stage1);
    HIPCHK(hipGetLastError());
    mci::MergeArgs &m = p->merge;
    m = merge_args(p, rq.nblocks, pl.wpb, pl.nrows);
    m.use_ghist = (pl.hist_lds && !pl.atomic_flush) ? 0 : pl.atomic_flush ? pl.ghist_buffers : 1;
    m.part_pa = rq.solver != MCI_VEGAS ? p->d_part_pa.get() : nullptr;
    m.hist_no_offset = (p->in_self_check && p->check_slot >= 0) ? 1 : 0; // (vegas_self_check compares the bare sums)
    m.hold = hold_hist; // (:mcmc: the 64 counts follow the tables in `packed`, so that ONE all-reduce carries them; NULL: zeros)
    // the chain solvers keep every block's mean of every iteration (one row of the block log; not the self-check's launches: their rows,
    // of another stride, would land on the logged ones)
    if (rq.solver != MCI_VEGAS && !p->in_self_check) {
        const int64_t stride = rq.nblocks * s.nobs;
        if (stride != p->launch.blk_stride || rq.block_lo != p->launch.blk_lo) {
            p->launch.blk_rows = 0;
            p->launch.blk_carried = 0;
            p->launch.blk_stride = stride;
            p->launch.blk_lo = rq.block_lo;
        }
        if ((rc = grow_block_log(p, p->launch.blk_rows + 1))) return rc;
        m.block_means = p->d_blocklog + (size_t)p->launch.blk_rows * stride;
        p->launch.blk_rows += 1;
        p->launch.blk_carried += p->launch.last_carried ? 1 : 0;
    }
    p->merge_pending = true;
    return MCI_OK;
}

// Does this :vegas launch run the big unit (mci_host_vegas_plan.h vegas_big_rule)?  Asked first as if the unit were usable; a launch
// that would take it compiles it (once per problem) and lets it prove itself (mci_host_check.h), then the rule is asked again with what
// the unit turned out to be.  Yes: rq.kern names it.  Anything else -- a unit over its register budget, one that did not compile (one
// note) or failed its check (one warning) -- leaves the request as it came: the standing unit runs.
static int select_vegas_big(mci_problem *p, LaunchRequest &rq) {
    if (vegas_big_rule(plan_big_in(p, rq, g_over, /*assume_unit=*/true)) != kBigTake) return MCI_OK;
    if (p->vegas_big.state == 0) {
        const int rc = compile_vegas_big(p);
        if (rc == MCI_ERR_COMPILE || p->vegas_big.state == VegasBigUnit::kNoCompile) {
            p->vegas_big.state = VegasBigUnit::kNoCompile;
            fprintf(stderr, "mci: the big :vegas unit of this problem did not compile; big launches keep the standing unit\n%s\n", mci_last_error());
            return MCI_OK;
        }
        if (rc) return rc;
    }
    if (p->vegas_big.state == 1 && !p->vegas_big.check_done)
        if (int rc = vegas_check_gate(p, mci_problem::kVegasBig, rq.nevalperblock, rq.block_lo, rq.block_hi, rq.iteration, rq.seed, rq.measurefreq)) return rc;
    if (vegas_big_rule(plan_big_in(p, rq, g_over, /*assume_unit=*/false)) == kBigTake) rq.kern = mci_problem::kVegasBig;
    return MCI_OK;
}

int mci_iteration_run(mci_problem *p, int32_t solver, int64_t nevalperblock, int64_t block_lo, int64_t block_hi,
                      int32_t iteration, uint64_t seed, int64_t measurefreq, int64_t nchain, double thermal_ratio) {
    // ---- validate ----
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context: no device to run on");
    if (solver != MCI_VEGAS && solver != MCI_VEGASMC && solver != MCI_MCMC) return fail(MCI_ERR_INVALID, "Solver %d is not supported!", solver); // main.jl:263
    if (measurefreq <= 0) return fail(MCI_ERR_INVALID, "measurefreq must be positive"); // vegas/montecarlo.jl:77
    const int64_t nblocks = block_hi - block_lo;
    if (nblocks < 1 || nevalperblock < 1) return fail(MCI_ERR_INVALID, "empty iteration");
    if (p->has_fermik && solver != MCI_MCMC) return fail(MCI_ERR_INVALID, "FermiK variables work with solver=:mcmc only"); // test/bubble_FermiK.jl:2,:133
    if (p->strat.on) { // stratified :vegas (mci_host_strat.h): its own sample kernel and launch
        if (solver != MCI_VEGAS) return fail(MCI_ERR_INVALID, "stratification works with solver = :vegas only (mci_set_stratification_off first)");
        p->launch.last_vegas_big = false;
        return strat_run(p, nevalperblock, block_lo, block_hi, iteration, seed, measurefreq);
    }
    // ---- compile and gate ----
    // (inside vegas_self_check: the code object under test, whatever the cadence of its small launch)
    const int kern = (p->in_self_check && p->check_slot >= 0 && solver == MCI_VEGAS) ? p->check_slot : kslot(solver, measurefreq);
    LaunchRequest rq{solver, nevalperblock, block_lo, block_hi, nblocks, iteration, seed, measurefreq, thermal_ratio, /*auto_chains=*/nchain <= 0, kern};
    // (the big :vegas unit is no solver slot: compile_vegas_big loads it, select_vegas_big below or -- for its own check's launches -- before that)
    auto compile_unit = [&]() { return rq.kern == mci_problem::kVegasBig ? MCI_OK : compile_solver(p, rq.kern); };
    // (a chain solver's lane-per-chain kernel is compiled once the launch is known to run one lane per chain: a launch of few chains
    // runs the several-lanes-per-chain kernel instead, mci_spec.h, and pays for that code object only)
    int rc = (rq.solver == MCI_VEGAS || p->deterministic || p->shape.host_integrand || p->spec_lanes == 1) ? compile_unit() : MCI_OK;
    if (rc) return rc;
    // a :vegas code object that has neither a marker nor a passed check yet proves itself first (mci_host_check.h); afterwards this
    // launch runs as if nothing had happened
    if (rq.solver == MCI_VEGAS && !p->in_self_check && !p->vegas_check_done[rq.kern == kSlotVegasAny ? 1 : 0] &&
        (rc = vegas_check_gate(p, rq.kern, rq.nevalperblock, rq.block_lo, rq.block_hi, rq.iteration, rq.seed, rq.measurefreq)))
        return rc;
    // (a check that fell back to the conservative layout has unloaded the slot's module; if that unit did not compile the slot is empty:
    // compiled here again -- a no-op otherwise -- so that the launch below never goes through a handle of an unloaded module)
    if (rq.solver == MCI_VEGAS && (rc = compile_unit())) return rc;
    // a big launch of a layout on the eight-copy plan: the big unit instead, if it is (or turns out) usable -- else exactly as before
    if (rq.solver == MCI_VEGAS && !p->in_self_check && (rc = select_vegas_big(p, rq))) return rc;
    if (rq.solver == MCI_VEGAS && p->shape.host_integrand && (rc = ensure_dump(p))) return rc;
    if ((rc = flush_merge(p))) return rc; // a previous batch nobody looked at: merge it (resets the global histogram)
    HIPCHK(hipSetDevice(p->ctx->device));
    // ---- plan (mci_host_plan.h), with the steps that must touch the device where the plan needs their answer ----
    const auto &s = p->shape;
    LaunchPlan pl;
    pl.nchain = nchain;
    plan_threads(p, rq, pl);
    pl.units = nevalperblock;
    if (rq.solver != MCI_VEGAS && (rq.block_hi > 4096 || rq.iteration >= 131072 || rq.iteration < 0))
        return fail(MCI_ERR_INVALID, "chain solvers address a chain by (block < 4096, iteration < 131072): got block_hi=%lld, iteration=%d",
                    (long long)rq.block_hi, (int)rq.iteration);
    pl.may_carry = plan_may_carry(p, rq);
    if (solver == MCI_VEGASMC) rc = plan_vegasmc_chains(p, rq, g_over, pl);
    else if (solver == MCI_MCMC) {
        if (!(rq.thermal_ratio >= 0.0)) return fail(MCI_ERR_INVALID, "thermal_ratio must be non-negative");
        // the holding times the launch before this one measured: what plan_mcmc_chains sizes automatic chains from
        if (rq.auto_chains && (rc = hold_consume(p))) return rc;
        rc = plan_mcmc_chains(p, rq, pl);
    } else pl.nchain = 1;
    if (rc) return rc;
    plan_spec_lanes(p, rq, pl);
    pl.T_launch = pl.T;
    if (pl.G > 1 && p->spec_state[rq.solver - 1] < 0) pl.G = 1; // (its code object failed its self-check, or did not compile: one lane per chain)
    if (pl.G > 1) {
        rc = compile_spec(p, rq.solver);
        if (rc == MCI_ERR_COMPILE && p->spec_lanes == -1) {
            // automatic lanes: a unit that does not compile (up to 512 VGPRs, many bpermutes; a backend switch a later compiler may
            // refuse) must not take the solver down with it -- the lane-per-chain kernel steps the same chains
            fprintf(stderr, "mci: the several-lanes-per-chain kernel of this problem did not compile; one lane per chain instead\n%s\n", mci_last_error());
            p->spec_state[rq.solver - 1] = -2;
            pl.G = 1;
        } else if (rc) return rc;
    }
    if (pl.G > 1 && !p->in_self_check && ((p->spec_need_check[rq.solver - 1] && !(g_over.spec_self_check.on && g_over.spec_self_check.v == 0)) ||
                                       (g_over.spec_self_check.on && g_over.spec_self_check.v == 1 && p->spec_state[rq.solver - 1] == 0))) {
        if ((rc = spec_self_check(p, rq.solver, pl.G, rq.nevalperblock, rq.block_lo, rq.block_hi, rq.iteration, rq.seed, rq.measurefreq, rq.thermal_ratio))) return rc;
        if (p->spec_state[rq.solver - 1] < 0) pl.G = 1;
    }
    if (pl.G > 1) {
        // the trees: the one built for the acceptance that was given, else the solver's family (spec_upload)
        if ((rc = spec_upload(p, rq.solver, pl.G, p->spec_accept, p->spec_maxacc))) return rc;
        pl.spec_maxacc = p->spec_tab_maxacc;
        pl.units = pl.nchain * pl.G;
        pl.T_launch = pl.units >= 256 ? 256 : (int)((pl.units + 63) / 64) * 64;
    }
    if (pl.G == 1 && (rc = compile_unit())) return rc;
    p->launch.last_spec_lanes = pl.G;
    p->launch.last_spec_maxacc = pl.spec_maxacc;
    plan_grid(p, rq, pl);
    if (const int candidate = plan_cursor_candidate(p, rq, g_over, pl)) {
        int resident = 0;
        if (candidate == 1) pl.cursor = true;
        else if ((rc = cursor_resident(p, rq.kern, pl.T, &resident))) return rc;
        else plan_cursor_grid(rq, resident, pl);
    }
    plan_tiles(p, rq, g_over, pl);
    plan_replay(p, rq, pl);
    plan_host_measure(p, rq, pl);
    plan_timing(p, rq, pl);
    // ---- the stages.  (`a` is built behind both self-check gates above -- they re-enter this function and may grow any buffer -- and
    // behind reserve_launch_buffers: nothing it holds can be invalidated before the launch) ----
    if ((rc = reserve_launch_buffers(p, rq, pl))) return rc;
    mci::BatchArgs a = request_args(p, rq, pl);
    if (solver != MCI_VEGAS && (rc = prepare_carried_chains(p, rq, pl, a))) return rc;
    if ((rc = prepare_chain_tables(p, rq, pl, a))) return rc;
    geometry_args(p, rq, pl, a);
    if (s.host_integrand && (rc = prepare_host_integrand(p, rq, pl, a))) return rc;
    if (s.host_measure && (rc = prepare_host_measure(p, rq, pl, a))) return rc;
    if (pl.cursor && (rc = prepare_cursor(p, rq, pl, a))) return rc;
    p->launch.last_cursor = pl.cursor;
    hipFunction_t f = p->kernel[pl.G > 1 ? (rq.solver == MCI_VEGASMC ? kSlotVegasmcSpec : kSlotMcmcSpec) : rq.kern].f;
    hipStream_t st = p->ctx->stream;
    const int slot = (int)(p->launch.launches % mci_problem::kEvRing);
    p->launch.time_this_launch = pl.time_this_launch;
    if (p->launch.time_this_launch && rq.solver == MCI_VEGAS) { // ... and the clock the sample loop ran at (mci_kernel_clocks)
        if (!p->d_clocks) {
            if ((rc = p->d_clocks.reserve(2 * mci_problem::kEvRing))) return rc;
            HIPCHK(hipMemsetAsync(p->d_clocks, 0, (size_t)2 * mci_problem::kEvRing * sizeof(unsigned long long), st));
        }
        a.clock_out = p->d_clocks + 2 * slot;
    }
    if (p->launch.time_this_launch) HIPCHK(hipEventRecord(p->evs[2 * slot], st));
    if (solver != MCI_VEGAS && s.host_integrand) rc = launch_host_closure_steps(p, rq, pl, a, f);
    else rc = launch_sample_chunks(p, rq, pl, a, f);
    if (rc) return rc;
    if (rq.solver == MCI_MCMC) p->launch.hold_measured = a.hold_hist != nullptr;
    // (an explicit chain count: nobody sizes a launch from this one's holds, and the host keeps queueing launches back to back)
    if (a.hold_hist && rq.auto_chains && (rc = hold_publish(p, rq.nevalperblock / pl.nchain, rq.solver != MCI_VEGAS && p->launch.last_carried))) return rc;
    if (pl.split && (rc = launch_replay(p, rq, pl, a))) return rc; // (the replay of the one chunk, or of the last one)
    if (p->launch.time_this_launch) HIPCHK(hipEventRecord(p->evs[2 * slot + 1], st));
    p->launch.ev_valid[slot] = p->launch.time_this_launch;
    p->launch.clock_valid[slot] = a.clock_out != nullptr && !pl.split && s.ntile == 1; // (what the kernel stamps: mci_device.h vegas_batch `stamp`)
    p->launch.launches += 1;
    if (s.host_measure && (rc = finish_host_measure(p, rq, pl))) return rc;
    // ---- record ----
    record_launch(p, nblocks * nevalperblock, pl.nwg, pl.T_launch, nblocks);
    if (solver != MCI_VEGAS) p->launch.last_nchain = pl.nchain;
    else p->launch.last_vegas_big = rq.kern == mci_problem::kVegasBig; // (mci_get_histogram_copies, mci_kernel_code_object describe this unit)
    return queue_merge(p, rq, pl, a.hold_hist);
}

// partials -> packed, if the last mci_iteration_run has not been merged yet
static int flush_merge(mci_problem *p) {
    if (!p->merge_pending) return MCI_OK;
    p->merge_pending = false;
    HIPCHK(hipSetDevice(p->ctx->device));
    hipLaunchKernelGGL(mci::k_finalize, finalize_grid(p->shape.nbin, p->npa), dim3(256), 0, p->ctx->stream, p->merge);
    HIPCHK(hipGetLastError());
    return MCI_OK;
}

int mci_iteration_reduce(mci_problem *p) {
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    if (!p->ctx->comm) return MCI_OK; // no communicator: single process (mpi_nprocs() == 1)
    int rc = flush_merge(p);
    if (rc) return rc;
    // HIP events around the collective under the sample launch's rule (mci_set_kernel_timing): what a rank waits for here is the
    // slowest rank's sample pass plus the latency of one small all-reduce (mci_comm_times_ms)
    const bool timed = p->launch.time_this_launch;
    const int slot = (int)(p->reduces % mci_problem::kCevRing);
    if (timed) {
        if (p->cevs.empty()) {
            p->cevs.resize(2 * mci_problem::kCevRing);
            for (auto &e : p->cevs) HIPCHK(hipEventCreate(&e));
        }
        HIPCHK(hipEventRecord(p->cevs[2 * slot], p->ctx->stream));
    }
    // ONE collective per iteration whatever the solver: [statistics | histograms | propose | accept] and, behind an :mcmc launch that
    // measured its holding times, the 64 counts of their histogram (exact in doubles)
    const size_t count = (size_t)p->packed_n + (p->launch.hold_deferred ? 64 : 0);
    int r = g_rccl.AllReduce(p->d_packed, p->d_packed, count, kNcclFloat64, kNcclSum, p->ctx->comm, p->ctx->stream);
    if (r) return fail(MCI_ERR_COMM, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    p->ctx->collectives += 1;
    p->ctx->last_count = (long long)count;
    if (p->launch.hold_deferred && (rc = hold_publish_reduced(p))) return rc; // the summed holding-time counts -> pinned host memory
    if (timed) HIPCHK(hipEventRecord(p->cevs[2 * slot + 1], p->ctx->stream));
    p->cev_valid[slot] = timed;
    p->reduces += 1;
    return MCI_OK;
}

int mci_comm_collectives(const mci_ctx *c, int64_t *calls, int64_t *last_count) {
    if (!c) return fail(MCI_ERR_INVALID, "NULL argument");
    if (calls) *calls = c->collectives;
    if (last_count) *last_count = c->last_count;
    return MCI_OK;
}

// An external reducer (comm.py TorchDistComm) has summed mci_reduce_size() doubles of `packed` over the ranks: what the library does
// behind its own all-reduce -- the summed :mcmc holding-time counts go to the host, every rank sizes its next chains from them
int mci_external_reduce_done(mci_problem *p) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    if (!p->launch.hold_ext_pending) return MCI_OK;
    p->launch.hold_ext_pending = false;
    HIPCHK(hipSetDevice(p->ctx->device));
    return hold_publish_reduced(p);
}

int mci_reduce_size(const mci_problem *p, int64_t *n) {
    if (!p || !n) return fail(MCI_ERR_INVALID, "NULL argument");
    *n = p->packed_n + 64;
    return MCI_OK;
}

int mci_comm_times_ms(mci_problem *p, float *ms, int32_t n, int32_t *got) {
    if (!p || !ms || !got) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    int64_t have = p->reduces < mci_problem::kCevRing ? p->reduces : mci_problem::kCevRing;
    if (have > n) have = n;
    int32_t k = 0;
    for (int64_t i = 0; i < have; ++i) { // oldest first
        const int slot = (int)((p->reduces - have + i) % mci_problem::kCevRing);
        if (!p->cev_valid[slot]) continue;
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, p->cevs[2 * slot], p->cevs[2 * slot + 1]));
        ms[k++] = t;
    }
    *got = k;
    return MCI_OK;
}

static int launch_train(mci_problem *p, int do_train, int do_reweight, double gamma, double *log_row) {
    const auto &s = p->shape;
    const int maxn = max_leaf_bins(p);
    mci::TrainArgs a{};
    fill_train(p, a);
    a.iter_log_row = log_row;
    a.goal = p->h_goal.empty() ? nullptr : p->d_goal.get();
    a.do_reweight = do_reweight;
    a.gamma = gamma;
    a.do_train = do_train;
    if (do_train) p->ntrain += 1;
    a.serial_walk = p->train_serial >= 0 ? p->train_serial : (p->launch.last_samples == 0 || p->launch.last_samples >= mci_problem::kSerialWalkSamples) ? 1 : 0;
    if (p->debug_wrong_decision && a.serial_walk == 1) a.serial_walk = 3;
    a.maxn = maxn;
    const size_t sm = train_lds_bytes(maxn, &a.spare);
    const unsigned tt = train_threads(maxn);
    if (sm > 64 * 1024 && !p->train_lds_raised) { // grids of more than ~1600 increments
        HIPCHK(hipFuncSetAttribute((const void *)mci::k_train, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrainLdsMax));
        HIPCHK(hipFuncSetAttribute((const void *)mci::k_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrainLdsMax));
        p->train_lds_raised = true;
    }
    if (p->merge_pending) { // nothing looked at `packed` since the sample batch: merge + refine in one launch
        p->merge_pending = false;
        hipLaunchKernelGGL(mci::k_finish, finish_grid(s.nleaf, p->npa), dim3(tt), sm, p->ctx->stream, p->merge, a);
    } else {
        hipLaunchKernelGGL(mci::k_train, dim3(s.nleaf + 1), dim3(tt), sm, p->ctx->stream, a);
    }
    HIPCHK(hipGetLastError());
    return MCI_OK;
}

// csrc/mci_debug.h: the problem's shape as the merge sees it
int mci_debug_merge_shape(const mci_problem *p, int32_t *shape, int32_t *leaves) {
    if (!p || !shape) return fail(MCI_ERR_INVALID, "NULL argument");
    const auto &s = p->shape;
    const int32_t v[8] = {s.nobs, s.ni, s.ncols, s.nbin, p->npa, p->nstat, s.nleaf, max_leaf_bins(p)};
    memcpy(shape, v, sizeof v);
    if (leaves)
        for (size_t l = 0; l < p->leaves.size(); ++l) {
            leaves[2 * l] = p->leaves[l].boff;
            leaves[2 * l + 1] = p->leaves[l].nbin;
        }
    return MCI_OK;
}

// csrc/mci_debug.h: the merge kernels alone, over rows the caller made up, launched as queue_merge / finish_host_measure, flush_merge and
// launch_train launch them; buffers of its own, nothing of the problem's but the device, the stream, the shape and the leaf table
int mci_debug_merge(mci_problem *p, const mci_debug_merge_io *io) {
    if (!p || !io || !io->part_cols || !io->packed) return fail(MCI_ERR_INVALID, "NULL argument");
    const auto &s = p->shape;
    const int64_t nblocks = io->nblocks, wpb = io->wg_per_block, nrows = io->nrows, hrows = io->hist_rows, k = io->use_ghist;
    if (nblocks < 1 || wpb < 1 || nrows < 1) return fail(MCI_ERR_INVALID, "merge: %lld blocks of %lld rows in %lld rows (each >= 1)", (long long)nblocks, (long long)wpb, (long long)nrows);
    if (hrows < 0 || k < 0 || k > 64) return fail(MCI_ERR_INVALID, "merge: %lld histogram rows, %lld global histogram buffers (0 .. 64)", (long long)hrows, (long long)k);
    if (hrows > 0 && k > 0) return fail(MCI_ERR_INVALID, "merge: hist_rows and use_ghist exclude each other");
    if (hrows == 0 && k == 0) return fail(MCI_ERR_INVALID, "merge: one of hist_rows and use_ghist must be given");
    if ((hrows > 0 && !io->part_hist) || (k > 0 && !io->ghist)) return fail(MCI_ERR_INVALID, "merge: the histogram rows are missing");
    if (io->path != 0 && io->path != 1) return fail(MCI_ERR_INVALID, "merge: path %d (0: k_finalize, 1: k_finish)", (int)io->path);
    const int64_t nbin1 = s.nbin ? s.nbin : 1, wide = std::max<int64_t>(std::max<int64_t>(s.ncols, 2 * (int64_t)p->npa), 1);
    if (nblocks > INT32_MAX / wpb || nrows > INT32_MAX / wide || nblocks > INT32_MAX / wide || hrows > INT32_MAX / nbin1 || (k + 1) > INT32_MAX / nbin1)
        return fail(MCI_ERR_INVALID, "merge: %lld blocks, %lld rows and %lld histogram rows are more than a test hook takes", (long long)nblocks, (long long)nrows, (long long)hrows);
    if (nrows < nblocks * wpb) return fail(MCI_ERR_INVALID, "merge: %lld rows for %lld blocks of %lld", (long long)nrows, (long long)nblocks, (long long)wpb);
    // "and train": the caller's tables, leaf after leaf, in doubles
    const bool train = io->do_train != 0;
    size_t ngrid = 0, ndist = 0, nacc = 0;
    for (auto &L : p->leaves) {
        if (L.kind == MCI_CONTINUOUS) ngrid += (size_t)L.npts;
        else if (L.kind == MCI_DISCRETE) ndist += (size_t)L.nbin, nacc += (size_t)L.nbin + 1;
    }
    if (train) {
        if (io->path != 1) return fail(MCI_ERR_INVALID, "merge: do_train needs path 1 (k_finish)");
        if (io->train_walk < 0 || io->train_walk > 3) return fail(MCI_ERR_INVALID, "merge: train walk %d (0 .. 3)", (int)io->train_walk);
        if ((ngrid && (!io->grids || !io->grids_out)) || (ndist && (!io->dists || !io->accs || !io->dists_out || !io->accs_out)))
            return fail(MCI_ERR_INVALID, "merge: do_train without its tables");
    }
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    const size_t ncell = (size_t)nrows * s.ncols, nhist = (size_t)hrows * s.nbin, ngh = (size_t)(k + 1) * nbin1, npart = (size_t)nrows * 2 * p->npa;
    const size_t npacked = (size_t)p->packed_n + 64, nst1 = (size_t)mci_problem::kGroups * nbin1, nscr = (size_t)nblocks * s.ncols, nbm = (size_t)nblocks * s.nobs;
    DevBuf<double> d_cols, d_hist, d_gh, d_pa, d_obs, d_packed, d_st1, d_scr, d_bm;
    DevBuf<unsigned long long> d_hold;
    DevBuf<int> d_stat;
    int rc;
    if ((rc = d_cols.reserve((int64_t)ncell)) || (rc = d_packed.reserve((int64_t)npacked)) || (rc = d_st1.reserve((int64_t)nst1)) || (rc = d_scr.reserve((int64_t)nscr)) ||
        (rc = d_bm.reserve((int64_t)(nbm ? nbm : 1))) || (rc = d_gh.reserve((int64_t)ngh)) || (rc = d_stat.reserve(4)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_cols, io->part_cols, ncell * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_packed, 0xFF, npacked * sizeof(double), st)); // (what the kernels do not write comes back as NaN)
    HIPCHK(hipMemsetAsync(d_st1, 0xFF, nst1 * sizeof(double), st));
    HIPCHK(hipMemsetAsync(d_scr, 0xFF, nscr * sizeof(double), st));
    HIPCHK(hipMemsetAsync(d_bm, 0xFF, (nbm ? nbm : 1) * sizeof(double), st));
    HIPCHK(hipMemsetAsync(d_gh, 0xFF, ngh * sizeof(double), st)); // (the guard row behind the k buffers stays like this)
    HIPCHK(hipMemsetAsync(d_stat, 0, 4 * sizeof(int), st));
    if (k > 0) HIPCHK(hipMemcpyAsync(d_gh, io->ghist, (size_t)k * s.nbin * sizeof(double), hipMemcpyHostToDevice, st));
    if (hrows > 0) {
        if ((rc = d_hist.reserve((int64_t)(nhist ? nhist : 1)))) return rc;
        HIPCHK(hipMemcpyAsync(d_hist, io->part_hist, nhist * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (io->part_pa) {
        if ((rc = d_pa.reserve((int64_t)npart))) return rc;
        HIPCHK(hipMemcpyAsync(d_pa, io->part_pa, npart * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (io->hold) {
        if ((rc = d_hold.reserve(64))) return rc;
        HIPCHK(hipMemcpyAsync(d_hold, io->hold, 64 * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    }
    if (io->obs && nbm) {
        if ((rc = d_obs.reserve((int64_t)nbm))) return rc;
        HIPCHK(hipMemcpyAsync(d_obs, io->obs, nbm * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // the hook's own tables for "and train", laid out as the problem lays its own out (Leaf::eoff, doff)
    DevBuf<double> d_tedges, d_tdacc, d_tddist;
    std::vector<double> t_edges, t_dacc, t_ddist;
    if (train) {
        t_edges = p->h_edges;
        t_dacc = p->h_dacc;
        t_ddist = p->h_ddist;
        size_t ig = 0, id = 0, ia = 0;
        for (auto &L : p->leaves) {
            if (L.kind == MCI_CONTINUOUS) {
                memcpy(t_edges.data() + L.eoff, io->grids + ig, (size_t)L.npts * sizeof(double));
                ig += (size_t)L.npts;
            } else if (L.kind == MCI_DISCRETE) {
                memcpy(t_ddist.data() + L.doff, io->dists + id, (size_t)L.nbin * sizeof(double));
                memcpy(t_dacc.data() + L.eoff, io->accs + ia, ((size_t)L.nbin + 1) * sizeof(double));
                id += (size_t)L.nbin;
                ia += (size_t)L.nbin + 1;
            }
        }
        if ((rc = d_tedges.reserve((int64_t)t_edges.size() + 1)) || (rc = d_tdacc.reserve((int64_t)t_dacc.size() + 1)) || (rc = d_tddist.reserve((int64_t)t_ddist.size() + 1)))
            return rc;
        if (!t_edges.empty()) HIPCHK(hipMemcpyAsync(d_tedges, t_edges.data(), t_edges.size() * sizeof(double), hipMemcpyHostToDevice, st));
        if (!t_dacc.empty()) HIPCHK(hipMemcpyAsync(d_tdacc, t_dacc.data(), t_dacc.size() * sizeof(double), hipMemcpyHostToDevice, st));
        if (!t_ddist.empty()) HIPCHK(hipMemcpyAsync(d_tddist, t_ddist.data(), t_ddist.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st)); // (the uploads have read the caller's pageable memory)
    if (io->obs && nbm) { // finish_host_measure
        hipLaunchKernelGGL(mci::k_add_host_obs, dim3((unsigned)((nblocks * s.nobs + 255) / 256)), dim3(256), 0, st, d_obs, (int)nblocks, s.nobs, s.ncols, (int)wpb, d_cols);
        HIPCHK(hipGetLastError());
    }
    if (hrows > 0 && s.nbin > 0) { // queue_merge
        hipLaunchKernelGGL(mci::k_hist_stage1, hist_stage1_grid(s.nbin), dim3(256), 0, st, d_hist, (int)hrows, s.nbin, (int)mci_problem::kGroups, d_st1);
        HIPCHK(hipGetLastError());
    }
    mci::MergeArgs m{};
    m.part_cols = d_cols;
    m.ncols = s.ncols;
    m.nobs = s.nobs;
    m.ni = s.ni;
    m.nblocks = (int)nblocks;
    m.wg_per_block = (int)wpb;
    m.stage1 = d_st1;
    m.ngroup = (int)mci_problem::kGroups;
    m.ghist = d_gh;
    m.use_ghist = (int)k;
    m.nbin = s.nbin;
    m.packed = d_packed;
    m.status = d_stat;
    m.scratch = d_scr;
    m.part_pa = io->part_pa ? d_pa.get() : nullptr;
    m.npa = p->npa;
    m.nrows = (int)nrows;
    m.block_means = io->block_means ? d_bm.get() : nullptr;
    m.hold = io->hold ? d_hold.get() : nullptr;
    m.hist_no_offset = io->hist_no_offset ? 1 : 0;
    if (io->path == 0) { // flush_merge
        hipLaunchKernelGGL(mci::k_finalize, finalize_grid(s.nbin, p->npa), dim3(256), 0, st, m);
    } else { // launch_train with a pending merge, told to do nothing but merge
        const int maxn = max_leaf_bins(p);
        mci::TrainArgs a{};
        a.leaves = p->d_leaves;
        a.nleaf = s.nleaf;
        a.packed = d_packed;
        a.nstat = p->nstat;
        a.nd = s.ni + 1;
        a.status = d_stat;
        a.maxn = maxn;
        if (train) { // ... or to refine as well, on the hook's tables
            a.edges = d_tedges;
            a.dacc = d_tdacc;
            a.ddist = d_tddist;
            a.do_train = 1;
            a.serial_walk = io->train_walk;
        }
        const size_t sm = train_lds_bytes(maxn, &a.spare);
        if (sm > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)mci::k_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrainLdsMax));
        hipLaunchKernelGGL(mci::k_finish, finish_grid(s.nleaf, p->npa), dim3(train_threads(maxn)), sm, st, m, a);
    }
    HIPCHK(hipGetLastError());
    int h_stat[4] = {0, 0, 0, 0};
    if (train) {
        if (!t_edges.empty()) HIPCHK(hipMemcpyAsync(t_edges.data(), d_tedges, t_edges.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (!t_dacc.empty()) HIPCHK(hipMemcpyAsync(t_dacc.data(), d_tdacc, t_dacc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (!t_ddist.empty()) HIPCHK(hipMemcpyAsync(t_ddist.data(), d_tddist, t_ddist.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_stat, d_stat, sizeof(h_stat), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(io->packed, d_packed, npacked * sizeof(double), hipMemcpyDeviceToHost, st));
    if (io->stage1) HIPCHK(hipMemcpyAsync(io->stage1, d_st1, (size_t)mci_problem::kGroups * s.nbin * sizeof(double), hipMemcpyDeviceToHost, st));
    if (io->scratch) HIPCHK(hipMemcpyAsync(io->scratch, d_scr, nscr * sizeof(double), hipMemcpyDeviceToHost, st));
    if (io->block_means && nbm) HIPCHK(hipMemcpyAsync(io->block_means, d_bm, nbm * sizeof(double), hipMemcpyDeviceToHost, st));
    if (io->status) HIPCHK(hipMemcpyAsync(io->status, d_stat, sizeof(int), hipMemcpyDeviceToHost, st));
    if (io->part_cols_out) HIPCHK(hipMemcpyAsync(io->part_cols_out, d_cols, ncell * sizeof(double), hipMemcpyDeviceToHost, st));
    if (io->ghist_out) HIPCHK(hipMemcpyAsync(io->ghist_out, d_gh, (size_t)(k + 1) * s.nbin * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // (the buffers are freed behind it)
    if (train) {
        size_t ig = 0, id = 0, ia = 0;
        for (auto &L : p->leaves) {
            if (L.kind == MCI_CONTINUOUS) {
                memcpy(io->grids_out + ig, t_edges.data() + L.eoff, (size_t)L.npts * sizeof(double));
                ig += (size_t)L.npts;
            } else if (L.kind == MCI_DISCRETE) {
                memcpy(io->dists_out + id, t_ddist.data() + L.doff, (size_t)L.nbin * sizeof(double));
                memcpy(io->accs_out + ia, t_dacc.data() + L.eoff, ((size_t)L.nbin + 1) * sizeof(double));
                id += (size_t)L.nbin;
                ia += (size_t)L.nbin + 1;
            }
        }
        if (io->walk_counts) io->walk_counts[0] = h_stat[1], io->walk_counts[1] = h_stat[2];
    }
    return MCI_OK;
}

// room for `rows` more iterations in the device-side iteration log (it grows by itself, with a stream synchronisation each time:
// a caller that must not synchronise inside a timed loop reserves first)
static int grow_iteration_log(mci_problem *p, int64_t need) {
    return grow_keeping(p, p->d_iterlog, need, 64, p->nstat);
}

int mci_reserve_iteration_log(mci_problem *p, int32_t rows) {
    if (!p || rows < 0) return fail(MCI_ERR_INVALID, "bad argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    return grow_iteration_log(p, (int64_t)p->log_row + rows);
}

int mci_iteration_finish(mci_problem *p, int32_t solver, int64_t block_total, int32_t adapt, double gamma, double *mean, double *std) {
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    HIPCHK(hipSetDevice(p->ctx->device));
    const auto &s = p->shape;
    if (int grc = grow_iteration_log(p, (int64_t)p->log_row + 1)) return grc;
    double *row = p->d_iterlog + (size_t)p->log_row * p->nstat;
    // doReweight! runs for the chain solvers whether or not the grid adapts (main.jl:183 is outside the `if adapt`)
    const bool strat = p->strat.last_run;
    int rc = launch_train(p, adapt ? 1 : 0, (solver == MCI_VEGASMC || solver == MCI_MCMC) ? 1 : 0, gamma, row);
    if (rc) return rc;
    if (strat && (rc = strat_finish(p, row, adapt))) return rc; // (the row's head: the stratified mean | var)
    p->log_row += 1;
    if (mean || std) {
        std::vector<double> h(p->nstat);
        HIPCHK(hipMemcpyAsync(h.data(), row, (size_t)p->nstat * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
        if ((rc = check_status(p))) return rc; // synchronises
        std::vector<double> m(s.nobs), e(s.nobs);
        if (strat) strat_mean_std(h.data(), s.nobs, m.data(), e.data());
        else
        mci_mean_std(h.data(), h.data() + s.nobs, s.nobs, block_total, m.data(), e.data());
        if (mean) memcpy(mean, m.data(), s.nobs * sizeof(double));
        if (std) memcpy(std, e.data(), s.nobs * sizeof(double));
    }
    return MCI_OK;
}

int mci_train(mci_problem *p) {
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    int rc = flush_merge(p);
    if (rc) return rc;
    rc = launch_train(p, 1, 0, 1.0, nullptr);
    if (rc) return rc;
    return check_status(p);
}

