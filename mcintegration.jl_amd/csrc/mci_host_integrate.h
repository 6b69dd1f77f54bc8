// mci_host_integrate.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// the persistent :vegas launch and the iteration loop mci_integrate (src/main.jl:142-218).
// ---------------------------------------------------------------------------------------------------
// persistent :vegas iterations: all `niter` iterations of a launch-bound mci_integrate call as ONE launch (mci_train.h vegas_persist)
// ---------------------------------------------------------------------------------------------------
namespace {
// LDS of the persistent kernel (bytes): the sample loop's carve (plain layout) or the refinement's (scratch, merged histogram, scan
// scratch), whichever is larger -- each is dead while the other runs --, and behind them (map_off, doubles) the workgroup's own copy of
// the map and the flag words (mci_train.h PersistArgs)
int64_t persist_lds(const mci_problem *p, int *map_off, int64_t more_carve = 0) { // more_carve: doubles a unit's sample carve takes beyond the plain one (sweep_until_carve)
    const int N = p->leaves.empty() ? 1 : p->leaves[0].nbin;
    const int64_t a = (p->lds_bytes + 7) / 8 + more_carve, b = (int64_t)mci::train_lds_doubles(N) + N + 256;
    const int64_t off = ((a > b ? a : b) + 1) & ~(int64_t)1;
    if (map_off) *map_off = (int)off;
    return (off + (N + 2) + 4) * 8;
}
// Structural conditions of the persistent kernel: ONE Continuous leaf (every sampling workgroup refines its own copy of the map), tables
// and histograms in LDS in one tile, device-source integrand and measure, everything within the 64 KiB every workgroup may ask for.
bool persist_layout(const mci_problem *p) {
    const auto &s = p->shape;
    if (p->deterministic || s.table_mode != 0 || s.ntile != 1 || s.host_integrand || s.host_measure || s.nbin <= 0 || s.ec_doubles > 0) return false;
    if (s.nleaf != 1 || p->leaves.size() != 1 || p->leaves[0].kind != 0) return false;
    return persist_lds(p, nullptr) <= 64 * 1024;
}
// Which calls run persistently, and on how many workgroups per block: one rank, :vegas at measurefreq == 1, the prefix-scan walk, no
// forced geometry or timing, a grid that is co-resident next to another one like it (<= 128 sampling workgroups + the statistics one).
// Automatic mode adds: launches of samples x draws < 2^19 per iteration over at most 7 draws per sample (tools/latency.py and sweeps of
// sizes and dimensions on the final code, us per iteration by the library's clock, persistent | launch chain: 2-D 11.5 | 12.8 at neval =
// 1e4, 13.7 | 13.9 at 1e5, 15.5 | 16.4 at 2e5, 19.6 | 19.2 at 5e5; 4-D 13.1 | 15.2 at 1e4, 16.6 | 19.7 at 1.2e5; 6-D 13.5 | 16.3 at 1e4,
// 17.1 | 17.6 at 8e4; 16-D 18.3 | 15.8 at 1e4 -- from 8 draws on the launch chain runs the hand-pipelined loop on its tuned layout,
// histogram copies and 512-thread workgroups, which this kernel's plain 256-thread layout does not match).
bool persist_plan(const mci_problem *p, const mci_integrate_args *a, int64_t nevalperblock, int64_t nblocks, int *wpb_out) {
    const auto &s = p->shape;
    if (p->persistent == 0 || p->persist_failed || p->vegas.conservative) return false; // (conservative: the persistent unit is a pipelined one)
    if (a->solver != MCI_VEGAS || a->measurefreq != 1 || a->niter < 1) return false;
    if (p->ctx->nranks != 1) return false; // (a one-rank communicator's all-reduce is the identity)
    if (!persist_layout(p)) return false;
    if (p->wg_per_block > 0 || p->kernel_timing > 0 || p->train_serial >= 1) return false;
    const int64_t work = nevalperblock * nblocks * s.ndraw;
    if (p->persistent < 0 && (work >= ((int64_t)1 << 19) || s.ndraw > 7)) return false;
    const int T = p->threads;
    int64_t target = work < ((int64_t)1 << 19) ? 64 : 128;
    int64_t wpb = (target + nblocks - 1) / nblocks;
    const int64_t maxw = (nevalperblock + T - 1) / T;
    if (wpb > maxw) wpb = maxw;
    if (wpb < 1) wpb = 1;
    while (wpb > 1 && wpb * nblocks > 128) --wpb;
    if (wpb * nblocks > 255) return false;
    if (wpb_out) *wpb_out = (int)wpb;
    return true;
}
} // namespace

static bool persist_layout_ok(const mci_problem *p) { return persist_layout(p); }

// one hiprtc job on a thread of its own (the thread touches nothing but this record)
struct mci_problem::PersistJob {
    Candidate c;
    std::thread th;
    std::atomic<bool> done{false};
};
// A problem that goes away (or changes its kernels) while its job is still compiling does not wait for it: the job moves to a
// process-wide list -- its code object still lands in the kernel cache, where the next problem with that kernel finds it -- and the
// list is joined when a context is destroyed and at exit (a thread inside hiprtc must not outlive the process's static objects).
namespace {
std::mutex g_orphan_mu;
std::vector<mci_problem::PersistJob *> g_orphans;
void persist_orphans_join() {
    std::vector<mci_problem::PersistJob *> mine;
    {
        std::lock_guard<std::mutex> g(g_orphan_mu);
        mine.swap(g_orphans);
    }
    for (auto *j : mine) {
        if (j->th.joinable()) j->th.join();
        delete j;
    }
}
} // namespace
static void persist_job_drop(mci_problem *p) {
    for (mci_problem::PersistJob *&slot : p->persist_job) {
        if (!slot) continue;
        mci_problem::PersistJob *j = slot;
        slot = nullptr;
        if (j->done.load(std::memory_order_acquire)) {
            if (j->th.joinable()) j->th.join();
            delete j;
            continue;
        }
        static std::once_flag once;
        std::call_once(once, [] { atexit(persist_orphans_join); });
        std::lock_guard<std::mutex> g(g_orphan_mu);
        g_orphans.push_back(j);
    }
}
// MCI_OK with the unit's `compiled` set: the kernel is loaded.  MCI_OK without: not yet (background == true and the code object is
// still being compiled) -- the caller takes the launch chain this time.  until: the unit with a target error (mci_persist_until.h,
// kernel[kPersistUntil]; chosen for mci_integrate_until alone) instead of the fixed one.
static int compile_persist(mci_problem *p, bool background, bool until) {
    KernelUnit &u = p->kernel[until ? mci_problem::kPersistUntil : mci_problem::kPersist];
    if (u.compiled) return MCI_OK;
    Candidate local, *c = &local;
    mci_problem::PersistJob *&job = p->persist_job[until ? 1 : 0];
    if (job) {
        if (!job->done.load(std::memory_order_acquire)) {
            if (background) return MCI_OK;
            job->th.join(); // (a caller that insists)
        }
        if (job->th.joinable()) job->th.join();
        local = std::move(job->c);
        delete job;
        job = nullptr;
    } else {
        mcijit::ProblemShape sh = p->shape;
        sh.hcopy = 1;
        sh.det = 0;
        c->unit = until ? mcijit::kUnitVegasPersistUntil : mcijit::kUnitVegasPersist;
        c->src = mcijit::generate_source(sh, MCI_VEGAS, c->unit, p->leaves[0].alpha);
        // (512 threads for the hand-pipelined loops of 8..16 draws -- what the launch chain runs them at -- was tried: 22.5 instead of 18.3 us
        // per iteration of the 16-D Gaussian at neval = 1e4, against 15.8 as a launch chain; the automatic rule stops at 7 draws)
        c->threads = p->threads;
        if (c->build(/*cache_only=*/background) == -1) { // not in the kernel cache: compile it behind the caller's back ...
            // ... once this process has made kPersistAfterCalls launch-bound calls of this kernel (by this problem or others with the same
            // shape and integrand): the persistent launch saves ~40 us per default-size call and its translation unit costs 0.8 s of hiprtc
            // -- on a thread of its own, but comgr serialises compiles, so another new kernel compiled meanwhile queues behind it (measured:
            // 0.69 instead of 0.24 s, tools/cold_start.py).  A loop of hundreds of small calls gets it (and every later process finds it in
            // the kernel cache); a script that makes a few calls never pays.
            {
                static const int kPersistAfterCalls = 256;
                static std::mutex mu;
                static std::map<uint64_t, int> asked;
                std::lock_guard<std::mutex> g(mu);
                if (++asked[mcijit::fnv1a(c->src)] < kPersistAfterCalls) return MCI_OK;
            }
            job = new mci_problem::PersistJob;
            job->c = std::move(local);
            mci_problem::PersistJob *j = job;
            j->th = std::thread([j] {
                j->c.build();
                j->done.store(true, std::memory_order_release);
            });
            return MCI_OK;
        }
    }
    if (c->rc) {
        p->persist_failed = true; // (the launch chain's own compile reports what is wrong with the integrand)
        return c->failed();
    }
    if (!p->ctx->offline && !p->d_persist) {
        HIPCHK(hipSetDevice(p->ctx->device));
        if (int rc = p->d_persist.reserve((int64_t)kPersistWords)) return rc;
        HIPCHK(hipMemsetAsync(p->d_persist, 0, kPersistWords * sizeof(unsigned long long), p->ctx->stream));
        p->persist_arrive = p->persist_done = 0;
    }
    // (a refusal is not an error of the call: it takes the launch chain; its LDS stays below the limit that needs raising)
    static const KernelUnit::Rules rules = {KernelUnit::kUnlinkAndFail, true, "the persistent :vegas kernel came out with static LDS or scratch",
                                            "the persistent :vegas code object"};
    if (until && !p->ctx->offline)
        if (int rc = p->d_persist_sums.reserve(2 * (int64_t)p->shape.nobs)) return rc;
    const int rc = u.load(p->ctx, *c, mcijit::kUnits[c->unit].kernel, 0, rules);
    if (rc) p->persist_failed = true;
    return rc;
}

// queue the one launch that runs iterations first_iteration .. first_iteration + niter - 1 over blocks [lo, hi); until: NULL, or the target
// of mci_integrate_until (the unit of mci_persist_until.h: the same launch, which may stop early -- persist_stopped() tells)
static int persist_launch(mci_problem *p, const mci_integrate_args *ia, int64_t nevalperblock, int64_t lo, int64_t hi, int wpb, const mci_sweep_target *until,
                          int ignore) {
    const auto &s = p->shape;
    const int64_t nblocks = hi - lo, nrows = nblocks * wpb;
    int rc;
    if ((rc = flush_merge(p))) return rc; // (a batch nobody looked at resets the global histogram when it is merged)
    HIPCHK(hipSetDevice(p->ctx->device));
    if ((rc = ensure_capacity(p, 2 * nrows, nblocks))) return rc; // (the partial rows are double-buffered by the turn's parity)
    if ((rc = grow_iteration_log(p, (int64_t)p->log_row + ia->niter))) return rc;
    const KernelUnit &unit = p->kernel[until ? mci_problem::kPersistUntil : mci_problem::kPersist];
    const int T = unit.threads;
    mci::BatchArgs a{};
    fill_batch(p, a);
    a.seed = ia->seed;
    a.iteration = (mci::u32)ia->first_iteration;
    a.neval_per_block = nevalperblock;
    a.block_lo = lo;
    a.wg_per_block = wpb;
    a.measurefreq = 1;
    a.nchain = 1;
    a.hist_atomic = 1;
    a.status = p->d_status;
    a.tile_stride = nblocks * nevalperblock;
    a.nrows = nrows;
    mci::PersistUntilArgs fu{}; // (the fixed unit is given its head alone)
    mci::PersistArgs &f = fu.p;
    mci::MergeArgs &m = f.m;
    m = merge_args(p, nblocks, wpb, nrows);
    m.use_ghist = 1;
    mci::TrainArgs &t = f.t;
    fill_train(p, t);
    t.iter_log_row = p->d_iterlog + (size_t)p->log_row * p->nstat;
    t.do_reweight = 0; // (:vegas: main.jl:183 runs doReweight! for the chain solvers only)
    t.gamma = ia->gamma;
    t.do_train = ia->adapt ? 1 : 0;
    t.serial_walk = 0;
    t.maxn = p->leaves[0].nbin;
    f.niter = ia->niter;
    const int64_t lds = persist_lds(p, &f.map_off);
    f.ctr = p->d_persist;
    if (p->persist_arrive > (1ull << 39)) { // (the arrive count owns 40 bits of the counter word: start over long before it spills)
        HIPCHK(hipMemsetAsync(p->d_persist, 0, kPersistCtrWords * sizeof(unsigned long long), p->ctx->stream));
        p->persist_arrive = p->persist_done = 0;
    }
    f.arrive0 = p->persist_arrive;
    f.done0 = p->persist_done;
    f.spin_ticks = p->persist_spin_ticks; // 2 s of the 100 MHz wall clock per wait
    if (until) fu.u = mci::SweepUntil{until->rtol, until->atol, until->min_niter, ignore, p->d_persist_sums, nullptr, nullptr};
    void *args[] = {&a, until ? (void *)&fu : (void *)&f};
    // The map the call starts from, kept aside: workgroup 0 writes the refined map back as soon as ITS last turn is through, and another
    // workgroup can still run out of time after that -- the fall-back to the launch chain (mci_integrate) restores this copy instead
    // of trusting that `edges` was not touched (8 KB, device to device, behind nothing: ~2 us of a 0.17 ms call)
    if ((rc = p->d_edges_backup.reserve(p->h_edges.size() ? (int64_t)p->h_edges.size() : 1))) return rc;
    if (p->h_edges.size()) HIPCHK(hipMemcpyAsync(p->d_edges_backup, p->d_edges, p->h_edges.size() * sizeof(double), hipMemcpyDeviceToDevice, p->ctx->stream));
    // nrows sampling workgroups + the statistics workgroup
    HIPCHK(hipModuleLaunchKernel(unit.f, (unsigned)nrows + 1, 1, 1, (unsigned)T, 1, 1, (unsigned)lds, p->ctx->stream, args, nullptr));
    p->persist_arrive += (unsigned long long)(ia->niter + 1) * (unsigned long long)nrows; // (+ one "finished reading" per workgroup at the end)
    p->persist_done += (unsigned long long)ia->niter;
    p->launch.time_this_launch = false;
    p->merge_pending = false;
    p->merge = m; // (what `packed` was merged from, for the record)
    p->merge.part_cols = p->d_part_cols + (size_t)((ia->niter - 1) & 1) * (size_t)nrows * s.ncols;
    record_launch(p, nblocks * nevalperblock, nrows, T, nblocks);
    p->log_row += ia->niter;
    return MCI_OK;
}
// Behind a launch with a target that stopped at turn n < niter (the stop word of mci_persist_until.h, read in the call's own
// synchronisation): the record persist_launch made for niter turns, put right.  Such a launch has added (n + 2) G arrivals -- turns
// 0 .. n once each and the final signal -- and n turns done, not (niter + 1) G and niter; its log holds n rows; the partial rows that
// `packed` was merged from are turn n - 1's.
static void persist_stopped(mci_problem *p, const mci_integrate_args *ia, int n) {
    const unsigned long long G = (unsigned long long)p->merge.nrows;
    p->persist_arrive -= (unsigned long long)(ia->niter + 1) * G;
    p->persist_arrive += (unsigned long long)(n + 2) * G;
    p->persist_done -= (unsigned long long)(ia->niter - n);
    p->log_row -= ia->niter - n;
    const size_t rows = (size_t)G * p->shape.ncols;
    p->merge.part_cols = p->d_part_cols + (size_t)((n - 1) & 1) * rows;
}

// sum over the ranks of a few host doubles (the lineage sums of a run): through a device scratch word of the communicator's stream
static int comm_sum_host(mci_problem *p, double *v, int n) {
    if (!p->ctx->comm) return MCI_OK;
    double *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)n * sizeof(double)));
    hipStream_t st = p->ctx->stream;
    hipError_t e = hipMemcpyAsync(d, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st);
    int r = e == hipSuccess ? g_rccl.AllReduce(d, d, (size_t)n, kNcclFloat64, kNcclSum, p->ctx->comm, st) : 0;
    p->ctx->collectives += 1;
    p->ctx->last_count = n;
    if (e == hipSuccess && !r) e = hipMemcpyAsync(v, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !r) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    if (r) return fail(MCI_ERR_COMM, "ncclAllReduce (lineage sums): %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    if (e != hipSuccess) return fail(MCI_ERR_HIP, "lineage sums: %s", hipGetErrorString(e));
    return MCI_OK;
}

// ---------------------------------------------------------------------------------------------------
// the tail of a call: log rows -> mci_result, for mci_integrate (everything at once, n = niter) and for mci_integrate_until (after
// every iteration the rule looks at, n = that iteration): ONE text, so "the numbers mci_integrate would report with niter = n" is what
// the rule reads
// ---------------------------------------------------------------------------------------------------
namespace {
struct IntegrateRows {
    int rows = 0;           // log rows already turned into res->iter_mean / iter_std
    int64_t blk = 0;        // rows of the block log already in `bm`
    std::vector<double> bm; // [blk][local blocks][nobs]
};
} // namespace
// h: the call's log rows [n][nstat] (host).  Fills res->iter_mean / iter_std rows [st.rows, n), neval, visited, mean / stdev / chi2 and
// correlated as mci_integrate with niter = n does; fetches the block-log rows it has not seen yet when the call is correlated.
static int integrate_result(mci_problem *p, const mci_integrate_args *a, int n, int64_t block, int64_t nb, int ignore, bool strat, int64_t blk_row0,
                            const double *h, IntegrateRows &st, mci_result *res) {
    const auto &s = p->shape;
    int rc;
    for (int it = st.rows; it < n; ++it) { // main.jl:203
        const double *row = h + (size_t)it * p->nstat;
        if (strat) strat_mean_std(row, s.nobs, res->iter_mean + (size_t)it * s.nobs, res->iter_std + (size_t)it * s.nobs);
        else
        mci_mean_std(row, row + s.nobs, s.nobs, block, res->iter_mean + (size_t)it * s.nobs, res->iter_std + (size_t)it * s.nobs);
    }
    if (n > st.rows) st.rows = n;
    res->neval = 0;
    for (int it = 0; it < n; ++it) res->neval += (int64_t)h[(size_t)it * p->nstat + 2 * s.nobs + 1];
    if (res->visited && n > 0) memcpy(res->visited, h + (size_t)(n - 1) * p->nstat + 2 * s.nobs + 2, (size_t)(s.ni + 1) * sizeof(double));
    for (int o = 0; o < s.nobs; ++o) // main.jl:211 -> statistics.jl:24-55
        mci_average(res->iter_mean + o, res->iter_std + o, s.nobs, ignore + 1, n, &res->mean[o], &res->stdev[o], &res->chi2[o]);
    // Carried chains: consecutive iterations are not independent, which statistics.jl:186-220 assumes -- but the blocks are (a block's
    // chains descend from that block's chains only), so the error comes from the scatter of the blocks' weighted averages over the run
    // (mci_lineage_sums + the reference's own _mean_std over them); same weights, same mean.
    res->correlated = 0;
    if (a->solver != MCI_VEGAS && blk_row0 >= 0 && p->launch.blk_rows - blk_row0 == n && p->launch.blk_carried > 0 && n > ignore + 1) {
        const size_t stride = (size_t)nb * s.nobs;
        st.bm.resize((size_t)n * stride);
        if (st.blk < n) {
            HIPCHK(hipMemcpyAsync(st.bm.data() + (size_t)st.blk * stride, p->d_blocklog + (size_t)(blk_row0 + st.blk) * p->launch.blk_stride,
                                  (size_t)(n - st.blk) * stride * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
            HIPCHK(hipStreamSynchronize(p->ctx->stream));
            st.blk = n;
        }
        std::vector<double> sums(2 * (size_t)s.nobs);
        mci_lineage_sums(st.bm.data(), n, nb, s.nobs, res->iter_std, ignore + 1, n, sums.data(), sums.data() + s.nobs);
        if ((rc = comm_sum_host(p, sums.data(), (int)sums.size()))) return rc;
        std::vector<double> lm(s.nobs), le(s.nobs);
        mci_mean_std(sums.data(), sums.data() + s.nobs, s.nobs, block, lm.data(), le.data());
        // (a column that is identically zero -- the imaginary part of a real integrand -- keeps the reference's 1e-10-regularised error,
        // statistics.jl:192-198, instead of an exact 0)
        for (int o = 0; o < s.nobs; ++o) res->stdev[o] = le[o] > 0.0 ? le[o] : res->stdev[o];
        res->correlated = 1;
    }
    return MCI_OK;
}

// (tests/test_integrate_until_host.py compiles the lines between the markers for the host, next to the rule text of mci_sweep_common.h)
// >>> integrate until rule
// The stop rule of mci_integrate_until after counted iteration n (mci_sweep_common.h, the host side of the same text).  Uncorrelated
// call: the columns' running sums W | S in `ws` [2 nobs] (sweep_until_add over rows [*added, n)), M = S / W, E = 1 / sqrt(W) as
// sweep_until_done forms them.  Correlated call: res->mean / res->stdev as integrate_result has just left them (the block-lineage error).
static bool integrate_until_met(const mci_sweep_target *t, const mci_result *res, int nobs, int n, int ignore, double *ws, int *added) {
    for (; *added < n; ++*added)
        for (int o = 0; o < nobs; ++o)
            mci::sweep_until_add(res->iter_mean[(size_t)*added * nobs + o], res->iter_std[(size_t)*added * nobs + o], *added + 1, ignore, ws[o], ws[nobs + o]);
    const int first = ignore + 2 > t->min_niter ? ignore + 2 : t->min_niter;
    if (n < first) return false;
    for (int o = 0; o < nobs; ++o) {
        // (sweep_until_done's own lines from M, E on: its unqualified isfinite() is the device's overload in this translation unit's host pass)
        const double M = res->correlated ? res->mean[o] : ws[nobs + o] / ws[o], E = res->correlated ? res->stdev[o] : 1.0 / sqrt(ws[o]);
        if (!(std::isfinite(M) && std::isfinite(E))) return false;
        const double rel = t->rtol * fabs(M);
        if (!(E <= (t->atol > rel ? t->atol : rel))) return false;
    }
    return true;
}
// <<< integrate until rule

// integrate  (reference src/main.jl:71-218)
// t: NULL (mci_integrate: all a->niter iterations) or the target of mci_integrate_until, which then leaves the iterations it ran in *niter_run
static int integrate_call(mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, mci_result *res, int32_t *niter_run) {
    if (!p || !a || !res) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context: no device to run on");
    const auto &s = p->shape;
    if (res->niter < a->niter || res->nobs != s.nobs) return fail(MCI_ERR_INVALID, "result buffers too small");
    if (!(a->neval > a->block)) return fail(MCI_ERR_INVALID, "neval=%lld should be larger than nblock = %lld", (long long)a->neval, (long long)a->block); // main.jl:222
    int64_t nevalperblock, block;
    mci_standardize_block(a->neval, a->block, p->ctx->nranks, &nevalperblock, &block); // main.jl:121
    const int64_t per = block / p->ctx->nranks;                                         // main.jl:122
    const int64_t lo = per * p->ctx->rank, hi = lo + per;
    if (a->solver != MCI_VEGAS && a->solver != MCI_VEGASMC && a->solver != MCI_MCMC) return fail(MCI_ERR_INVALID, "Solver %d is not supported!", a->solver); // main.jl:263
    // launch-bound :vegas calls: the whole loop below as one persistent launch (same iterations, same Philox streams)
    int wpb_persist = 0, rc = 0;
    const bool strat = p->strat.on; // (stratified :vegas: the launch chain, never the persistent launch)
    if (strat) {
        if (a->solver != MCI_VEGAS) return fail(MCI_ERR_INVALID, "stratification works with solver = :vegas only (mci_set_stratification_off first)");
        if (a->measurefreq != 1) return fail(MCI_ERR_INVALID, "stratification: measurefreq = %lld is refused (every sample is measured)", (long long)a->measurefreq);
        strat_call_start(p); // (the first iteration of a call samples every hypercube alike)
    }
    bool persist = !strat && persist_plan(p, a, nevalperblock, hi - lo, &wpb_persist);
    // (automatic mode: a code object that is not in the kernel cache yet is compiled on a thread of its own, and until it is there the
    // calls go through the launch chain -- a new integrand's first call costs what it did, 0.2 s, not the 0.8 s of the larger unit)
    // (a call with a target: the unit of mci_persist_until.h, by the same rules)
    if (persist) (void)compile_persist(p, p->persistent < 0, t != nullptr);
    persist = persist && p->kernel[t ? mci_problem::kPersistUntil : mci_problem::kPersist].compiled;
    if (!persist && !strat && (rc = compile_solver(p, kslot(a->solver, a->measurefreq)))) return rc;
    if ((rc = mci_set_reweight_goal(p, a->reweight_goal, a->reweight_goal ? p->ni + 1 : 0))) return rc;
    const int ignore = a->ignore >= 0 ? a->ignore : (a->adapt ? 1 : 0);
    const size_t nlog = (size_t)a->niter * p->nstat; // the pinned landing place of the statistics (+ the status word), sized outside the timed loop
    if ((int64_t)nlog + 2 > p->h_log.capacity()) { // (+ the stop word of a persistent launch with a target)
        int64_t ncap = p->h_log.capacity() ? p->h_log.capacity() : (int64_t)64 * p->nstat + 2;
        while (ncap < (int64_t)nlog + 2) ncap *= 2;
        if ((rc = p->h_log.reserve(ncap))) return rc;
    }
    int64_t blk_row0 = -1; // this call's first row of the block log (chain solvers): the log starts over with every call
    if (a->solver != MCI_VEGAS) {
        if ((rc = flush_merge(p))) return rc; // (a pending merge writes its row of the old log)
        p->launch.blk_rows = 0;
        p->launch.blk_carried = 0;
        p->launch.blk_stride = (hi - lo) * s.nobs;
        p->launch.blk_lo = lo;
        blk_row0 = 0;
        if ((rc = grow_block_log(p, a->niter))) return rc;
    }
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    const int row0 = p->log_row;
    auto t0 = std::chrono::steady_clock::now();
    double *h = p->h_log;
    int *hstatus = reinterpret_cast<int *>(p->h_log + nlog);
    int res_warmup = 0;
    p->last_discarded_neval = 0;
    p->last_discarded_launches = 0;
    // mci_integrate_until: n, the iterations the call runs (the rule below shortens it); what has come back so far
    int n = a->niter, copied = 0, added = 0;
    IntegrateRows rows;
    std::vector<double> ws(t ? 2 * (size_t)s.nobs : 0, 0.0);
    const int first = t ? (ignore + 2 > t->min_niter ? ignore + 2 : t->min_niter) : 0;
    for (int attempt = 0;; ++attempt) {
        p->last_persistent = persist;
        if (persist && (rc = persist_launch(p, a, nevalperblock, lo, hi, wpb_persist, t, ignore))) return rc;
        const unsigned long long persist_done0 = p->persist_done - (unsigned long long)a->niter; // (the launch's done0: what its stop word is counted from)
        // (a hipGraph replay of this chain was measured and dropped: 37.6 against 34.8 us per launch-bound iteration for the eager
        // asynchronous launches on ROCm 7.0 / MI355X, profiles/r02_ablation.txt)
        for (int it = 0; it < a->niter && !persist; ++it) { // main.jl:142
            for (int attempt = 0;; ++attempt) {
                const int32_t iter = a->first_iteration + it + kRepeatStride * attempt;
                p->launch_counted = it >= ignore;
                if ((rc = mci_iteration_run(p, a->solver, nevalperblock, lo, hi, iter, a->seed, a->measurefreq, a->nchain, a->thermal_ratio))) return rc;
                if ((rc = mci_iteration_reduce(p))) return rc;                                   // main.jl:177-188
                if ((rc = mci_iteration_finish(p, a->solver, block, a->adapt, a->gamma, nullptr, nullptr))) return rc; // main.jl:183-199
                // Warm-up of the automatic :mcmc chain length (mci_mcmc_auto_chains): an iteration whose chains turned out too short for
                // the holding times they measured is not counted -- it has trained the map and moved the reweight factors, its chains
                // go on -- and runs again with longer chains (the Philox streams of iteration + kRepeatStride * attempt), until the
                // first launch that is long enough; from then on nothing is repeated.  The first iteration of a call that ignores it
                // anyway (main.jl:82) is let through as it is.
                if (a->solver != MCI_MCMC || a->nchain > 0 || p->launch.mcmc_warm || (it == 0 && ignore >= 1) || attempt >= kMaxRepeats ||
                    a->first_iteration + it >= kRepeatStride || p->launch.last_nchain <= 1 || !p->launch.hold_inflight)
                    break;
                int32_t valid = 0;
                if ((rc = mci_mcmc_launch_valid(p, &valid, nullptr, nullptr, nullptr))) return rc;
                if (valid) break;
                if ((rc = mci_iteration_discard(p))) return rc; // (the repeat overwrites this attempt's rows of the iteration log and of the block log)
                res_warmup += 1;
                p->last_discarded_neval += nevalperblock * (hi - lo);
                p->last_discarded_launches += 1;
            }
            // mci_integrate_until: up to iteration first - 1 the launches are queued back to back as ever; from there on the rows that
            // have not come back yet do, behind one synchronisation per iteration, and the rule reads what mci_integrate would report
            // with niter = it + 1 (an iteration is looked at only once it has been accepted: behind the warm-up repeats above)
            if (t && it + 1 >= first) {
                HIPCHK(hipMemcpyAsync(h + (size_t)copied * p->nstat, p->d_iterlog + (size_t)(row0 + copied) * p->nstat, (size_t)(it + 1 - copied) * p->nstat * sizeof(double),
                                      hipMemcpyDeviceToHost, p->ctx->stream));
                HIPCHK(hipStreamSynchronize(p->ctx->stream));
                copied = it + 1;
                if ((rc = integrate_result(p, a, it + 1, block, hi - lo, ignore, strat, blk_row0, h, rows, res))) return rc;
                if (integrate_until_met(t, res, s.nobs, it + 1, ignore, ws.data(), &added)) {
                    n = it + 1;
                    break;
                }
            }
        }
        p->launch_counted = false;
        // the statistics of all iterations and the status word come back behind the last kernel in ONE synchronisation, into pinned memory (a
        // pageable destination goes through a staging copy: ~15 us of a 0.2 ms default-size call)
        // (mci_integrate_until's launch chain: the rows the rule has not fetched already)
        if (n > copied)
            HIPCHK(hipMemcpyAsync(h + (size_t)copied * p->nstat, p->d_iterlog + (size_t)(row0 + copied) * p->nstat, (size_t)(n - copied) * p->nstat * sizeof(double),
                                  hipMemcpyDeviceToHost, p->ctx->stream));
        HIPCHK(hipMemcpyAsync(hstatus, p->d_status, sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
        // (a persistent launch with a target: where it stopped comes back in the same synchronisation, behind the status word)
        unsigned long long *hstop = reinterpret_cast<unsigned long long *>(p->h_log + nlog + 1);
        if (persist && t) HIPCHK(hipMemcpyAsync(hstop, p->d_persist + mci::kPersistStopWord, sizeof(unsigned long long), hipMemcpyDeviceToHost, p->ctx->stream));
        HIPCHK(hipStreamSynchronize(p->ctx->stream));
        if (persist && attempt == 0 && (*hstatus & mci::ST_PERSIST_STALL)) {
            // A grid-wide wait of the persistent launch ran out of time (its workgroups were not all resident: a device shared with another
            // long-running kernel).  Nothing of the call is lost: the map the call started from is restored from the copy persist_launch
            // took (workgroup 0 may have written its refined map back before another workgroup gave up), counters, histogram buffers and
            // the status word are reset, the iteration log is rewound, and the same iterations run through the launch chain (as every
            // later call of this problem does).
            if (p->d_edges_backup && p->h_edges.size())
                HIPCHK(hipMemcpyAsync(p->d_edges, p->d_edges_backup, p->h_edges.size() * sizeof(double), hipMemcpyDeviceToDevice, p->ctx->stream));
            if ((rc = persist_recover(p))) return rc;
            p->log_row = row0;
            persist = false;
            if ((rc = compile_solver(p, kslot(a->solver, a->measurefreq)))) return rc;
            continue;
        }
        if (persist && t && *hstop > persist_done0 && *hstop - persist_done0 < (unsigned long long)a->niter) {
            // the launch stopped at turn n: its turn n + 1 of samples was drawn and thrown away (neither in res->neval nor in the estimate)
            n = (int)(*hstop - persist_done0);
            persist_stopped(p, a, n);
            p->last_discarded_neval += nevalperblock * (hi - lo);
        }
        break;
    }
    if (*hstatus && (rc = check_status(p))) return rc; // (reads it again, clears it, names the failure)
    auto t1 = std::chrono::steady_clock::now();
    res->seconds = std::chrono::duration<double>(t1 - t0).count();
    res->warmup = res_warmup;
    if ((rc = integrate_result(p, a, n, block, hi - lo, ignore, strat, blk_row0, h, rows, res))) return rc;
    if (niter_run) *niter_run = n;
    return MCI_OK;
}

int mci_integrate(mci_problem *p, const mci_integrate_args *a, mci_result *res) { return integrate_call(p, a, nullptr, res, nullptr); }

// ---------------------------------------------------------------------------------------------------
// mci_integrate with a target error: the same call, stopped by the rule of mci_sweep_common.h
// ---------------------------------------------------------------------------------------------------
int mci_integrate_until_supported(const mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, char *why, int32_t n) {
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    char buf[160];
    const char *r = nullptr;
    if (!t) r = "the target is NULL";
    else if (!(std::isfinite(t->rtol) && t->rtol >= 0.0)) r = "rtol is negative or not finite";
    else if (!(std::isfinite(t->atol) && t->atol >= 0.0)) r = "atol is negative or not finite";
    else if (t->min_niter < 0) r = "min_niter < 0";
    else if (p->ctx->nranks != 1) r = "more than one rank (the block-lineage sums would need a collective per iteration)";
    // ... and what mci_integrate refuses
    else if (!(a->neval > a->block)) snprintf(buf, sizeof buf, "neval=%lld should be larger than nblock = %lld", (long long)a->neval, (long long)a->block), r = buf;
    else if (a->solver != MCI_VEGAS && a->solver != MCI_VEGASMC && a->solver != MCI_MCMC) snprintf(buf, sizeof buf, "Solver %d is not supported!", a->solver), r = buf;
    else if (p->strat.on && a->solver != MCI_VEGAS) r = "stratification works with solver = :vegas only (mci_set_stratification_off first)";
    else if (p->strat.on && a->measurefreq != 1) r = "stratification: measurefreq != 1 is refused (every sample is measured)";
    if (!r) return MCI_OK;
    if (why && n > 0) snprintf(why, (size_t)n, "%s", r);
    return fail(MCI_ERR_INVALID, "this call cannot run to a target error: %s", r);
}

int mci_integrate_until(mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, mci_result *res, int32_t *niter_run) {
    if (!p || !a || !res || !niter_run) return fail(MCI_ERR_INVALID, "NULL argument");
    if (int rc = mci_integrate_until_supported(p, a, t, nullptr, 0)) return rc; // (first: a refusal is the same with and without a device)
    return integrate_call(p, a, t, res, niter_run);
}

