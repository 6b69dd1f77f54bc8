// mci_host_jit.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// the kernel slots and their JIT, the speculation trees of the several-lanes-per-chain kernels, the per-problem setters.
// ---- JIT of the sample-batch kernels ------------------------------------------------------------------------------------
// Kernel slots: 0 :vegas for measurefreq == 1 (the reference's default, main.jl:84: the loop without the carried remainder),
// 1 :vegasmc, 2 :mcmc, 3 :vegas for any measurefreq -- each its own code object, compiled the first time it is needed (a new
// integrand pays for the loop it runs, not for both).  The sample-dump kernel is a fifth, equally lazy one.
enum { kSlotVegasAny = 3, kSlotDump = 4, kSlotVegasmcSpec = 5, kSlotMcmcSpec = 6 };
static int kslot(int solver, int64_t measurefreq) { return solver == MCI_VEGAS && measurefreq != 1 ? kSlotVegasAny : solver; }
static int slot_solver(int slot) { return slot == kSlotVegasAny ? MCI_VEGAS : slot == kSlotVegasmcSpec ? MCI_VEGASMC : slot == kSlotMcmcSpec ? MCI_MCMC : slot; }

namespace {
struct Candidate { // one hiprtc job
    std::string src;
    int threads = 256;
    int unit = mcijit::kUnitSolver;
    std::vector<char> code;
    std::string log, path;
    bool cached = false;
    int rc = 0;
    long vgprs() const { return mcijit::kernel_vgprs(code, "mci_vegas_batch"); }
    long scratch() const { return mcijit::kernel_scratch_bytes(code, "mci_vegas_batch"); }
    int build(bool cache_only = false) { return rc = mcijit::compile(src, threads, code, log, cached, &path, unit, cache_only); }
    // the message of a candidate that did not compile; `of`: which kernel, for the units that say so (" (stratified :vegas kernel)")
    int failed(const std::string &of = "") const { return fail(MCI_ERR_COMPILE, "integrand failed to compile for gfx950%s:\n%s", of.c_str(), log.c_str()); }
};
// the candidates of a plan are independent translation units: compiled side by side (hiprtc is re-entrant), so a plan that has to
// look at two or three of them before it knows which one runs costs the latency of the slowest, not their sum
void compile_all(const std::vector<Candidate *> &cs) {
    std::vector<std::thread> th;
    for (size_t i = 1; i < cs.size(); ++i) th.emplace_back([c = cs[i]] { c->build(); });
    if (!cs.empty()) cs[0]->build();
    for (auto &t : th) t.join();
}

int KernelUnit::load(const mci_ctx *ctx, Candidate &c, const char *kernel, int64_t lds, const Rules &rules) {
    const long static_lds = mcijit::max_static_lds_bytes(c.code);
    if (static_lds != 0 || (rules.no_scratch && mcijit::kernel_scratch_bytes(c.code, kernel) != 0)) {
        if (!rules.refusal.empty()) return fail(MCI_ERR_COMPILE, "%s", rules.refusal.c_str());
        // (mci_device.h draw_leaf: the pair table is addressed from LDS address 0)
        return fail(MCI_ERR_COMPILE, "the code object declares static LDS (%ld bytes): the sample kernels expect their dynamic segment at LDS address 0", static_lds);
    }
    code_object = c.path;
    threads = c.threads;
    if (!ctx->offline) {
        HIPCHK(hipSetDevice(ctx->device));
        if (rules.stale == kFail) HIPCHK(hipModuleLoadData(&module, c.code.data()));
        else if (hipModuleLoadData(&module, c.code.data()) != hipSuccess) {
            if (c.cached) unlink(c.path.c_str());
            if (!c.cached || rules.stale == kUnlinkAndFail) return fail(MCI_ERR_HIP, "hipModuleLoadData failed for %s", rules.what.c_str());
            if (c.build()) return c.failed(); // (compiled afresh, once)
            HIPCHK(hipModuleLoadData(&module, c.code.data()));
        }
        if (int rc = entry(&f, kernel, lds)) return rc;
    }
    compiled = true;
    return MCI_OK;
}
} // namespace

static const KernelUnit::Rules kSlotRules = {KernelUnit::kRecompileOnce, false, "", "a freshly compiled code object"};
// The main kernel of a JIT unit: its row of mcijit::kUnits -- or, for the rows that leave it open, what generate_source calls the
// solver's kernel in such a unit.
static const char *unit_kernel(int unit, int solver) {
    if (const char *k = mcijit::kUnits[unit].kernel) return k;
    if (unit == mcijit::kUnitDump) return "mci_sample_dump";
    if (unit == mcijit::kUnitSpec) return solver == MCI_VEGASMC ? "mci_vegasmc_spec" : "mci_mcmc_spec";
    return solver == MCI_VEGAS ? "mci_vegas_batch" : solver == MCI_VEGASMC ? "mci_vegasmc_chains" : "mci_mcmc_chains";
}
// a slot's code object, and the second entry points of the same module
static int load_slot(mci_problem *p, int slot, Candidate &c, int64_t lds) {
    KernelUnit &u = p->kernel[slot];
    if (int rc = u.load(p->ctx, c, unit_kernel(c.unit, slot_solver(slot)), lds, kSlotRules)) return rc;
    if (p->ctx->offline) return MCI_OK;
    if (slot == MCI_VEGASMC || slot == kSlotVegasmcSpec)
        if (int rc = u.entry(&p->f_carryw[slot == MCI_VEGASMC ? 0 : 1], "mci_vegasmc_carry_weights", lds)) return rc;
    if (slot_solver(slot) == MCI_VEGAS && slot != kSlotDump && p->shape.ntile > 1)
        if (int rc = u.entry(&p->f_tiles[slot == kSlotVegasAny ? 1 : 0], "mci_vegas_tiles", p->lds_bytes)) return rc;
    return MCI_OK;
}

// the map + integrand alone (mci_sample_dump, host integrands): its own small code object
static int ensure_dump(mci_problem *p) {
    if (p->kernel[kSlotDump].compiled) return MCI_OK;
    Candidate c;
    mcijit::ProblemShape sh = p->shape;
    sh.hcopy = 1;
    sh.det = 0;
    c.unit = mcijit::kUnitDump;
    c.src = mcijit::generate_source(sh, MCI_VEGAS, mcijit::kUnitDump);
    c.threads = 256;
    if (c.build()) return c.failed();
    return load_slot(p, kSlotDump, c, p->lds_bytes);
}

// vegas/montecarlo.jl:104, mcmc/montecarlo.jl:84
static int default_measure_fits(const mci_problem *p) {
    for (int i = 0; i < p->ni && p->shape.measure_body.empty() && !p->shape.host_measure; ++i)
        if (p->shape.obs_bin_draw[i] < 0 && p->shape.obs_nbin[i] != p->shape.ncomp)
            return fail(MCI_ERR_INVALID, "the default measure can only handle observable as Vector with %d scalar elements!", p->ni);
    return MCI_OK;
}

// prefix of a :vegas unit in the conservative layout: no hand-pipelined sample loop (mci_device.h pipe_eligible)
static const char *const kVegasPlainLoop = "#define MCI_VEGAS_PLAIN_LOOP 1\n";
static const char *const kVgprKeys = "#define MCI_PIPE_VGPR_KEYS 1\n";
// The driver of every solver slot: one candidate for the chain solvers and the deterministic mode; for :vegas the candidates
// vegas_kernel_rule (mci_host_vegas_plan.h) asks for, batch by batch, and of those the one it chose.
static int compile_solver(mci_problem *p, int slot) {
    if (slot < 0 || slot > kSlotVegasAny) return fail(MCI_ERR_INVALID, "Solver %d is not supported!", slot); // main.jl:263
    if (p->kernel[slot].compiled) return MCI_OK;
    const int solver = slot_solver(slot);
    const int unit = slot == MCI_VEGAS ? mcijit::kUnitVegasMf1 : mcijit::kUnitSolver;
    // (a problem whose :vegas unit failed its self-check, mci_host_check.h: EVERY :vegas unit it compiles from then on -- either cadence,
    // planned or planned again after drop_modules -- is the plain loop)
    auto gen = [&](const mcijit::ProblemShape &sh, bool keys = false) {
        return std::string(keys ? kVgprKeys : "") + (p->vegas.conservative && solver == MCI_VEGAS ? kVegasPlainLoop : "") + mcijit::generate_source(sh, solver, unit);
    };
    if (int rc = default_measure_fits(p)) return rc;
    struct Built { VegasVariant v; Candidate c; };
    std::deque<Built> built; // (every candidate of the call, in the order it was asked for)
    auto add = [&](const VegasVariant &v) {
        built.push_back({v, {}});
        Candidate &c = built.back().c;
        mcijit::ProblemShape sh = p->shape;
        sh.hcopy = v.copies;
        c.unit = unit;
        c.src = gen(sh, v.keys);
        c.threads = v.threads;
        return &c;
    };
    Candidate *chosen = nullptr;
    int64_t lds = p->lds_bytes;
    if (p->deterministic) {
        // one copy of the LDS histograms (and observables) per wave, as many waves as fit: 512 / 256 / 128 / 64 threads
        if (p->shape.ntile > 1 || p->shape.table_mode == 1 || p->shape.table_mode == 2 || p->shape.ec_doubles > 0)
            return fail(MCI_ERR_INVALID, "deterministic mode keeps one copy of the workgroup's histograms per wave in LDS: %d bins (%d tile(s)) do not fit",
                        p->shape.nbin, p->shape.ntile);
        int T = solver == MCI_VEGAS ? 512 : (p->threads < 512 ? p->threads : 512); // (the chain kernels need ~200 registers: 256 threads)
        while (T > 64 && det_lds(p, T) > 159 * 1024) T >>= 1;
        if (det_lds(p, T) > 159 * 1024) return fail(MCI_ERR_INVALID, "deterministic mode: the tables do not fit one CU's LDS");
        p->threads_det[solver] = T;
        p->shape.det = 1;
        p->shape.hcopy = T / 64;
        lds = det_lds(p, T);
    } else p->shape.det = 0;
    if (p->deterministic || solver != MCI_VEGAS) {
        chosen = add({p->shape.hcopy, false, p->deterministic ? p->threads_det[solver] : p->threads});
        if (chosen->build()) return chosen->failed();
    } else {
        const auto &s = p->shape;
        const VegasRuleIn in = {p->threads, p->threads_explicit, s.ndraw, s.host_integrand != 0, p->deterministic, g_over.hist_copies.on, sixteen_copies_fit(p), s.hcopy};
        size_t batch = 0; // where the last batch starts
        auto build = [&](const std::vector<VegasVariant> &vs, std::vector<VegasBuilt> &out) {
            batch = built.size();
            std::vector<Candidate *> cs;
            for (const VegasVariant &v : vs) cs.push_back(add(v));
            compile_all(cs);
            out.clear();
            for (Candidate *c : cs) out.push_back({c->rc ? 0 : c->vgprs(), c->rc ? 0 : c->scratch(), c->rc == 0});
        };
        VegasVariant v{};
        const int rc = vegas_kernel_rule(p->vegas, in, build, &v);
        p->shape.hcopy = v.copies;
        for (size_t i = batch; rc && i < built.size(); ++i)
            if (built[i].c.rc) return built[i].c.failed();
        for (Built &b : built) // (the last one built of the chosen variant: of the last batch, or the plain layout of the first)
            if (b.v.copies == v.copies && b.v.keys == v.keys && b.v.threads == v.threads) chosen = &b.c;
        lds = vegas_lds(p);
        if (s.ec_doubles > 0 && p->lds_bytes_k1 > lds) lds = p->lds_bytes_k1;
        if (p->lds_bytes > lds) lds = p->lds_bytes;
    }
    return load_slot(p, slot, *chosen, lds);
}

// ---- the big :vegas unit (mci_host_vegas_plan.h) ------------------------------------------------------------------------------
// Does the layout have one at all?  What can be said without the standing unit's registers: the create-time half of vegas_big_rule.
static bool vegas_big_layout(const mci_problem *p) {
    return vegas_pipe_unit(p) && p->vegas.hcopy_plan && p->vegas.hcopy_auto >= 8 && !g_over.hist_copies.on && !p->threads_explicit && sixteen_copies_fit_lds(p);
}
// The measurefreq == 1 source of the problem with sixteen histogram copies, bound to 1024 threads, in kernel[kVegasBig]: its own
// candidate and cache entry (the source differs in HCOPY, the key in the launch bound too), compiled the first time a launch selects
// it.  Reads the problem's shape through a copy: the standing plan, shape.hcopy and the standing code objects stay as they are.
// VGPR round keys if the unit stays within 128 registers without scratch, else SGPR keys, else VegasBigUnit::kOverBudget.  What the
// call leaves is vegas_big.state; != MCI_OK only when the unit did not compile or load.
static int compile_vegas_big(mci_problem *p) {
    VegasBigUnit &b = p->vegas_big;
    if (b.state != 0) return MCI_OK;
    if (int rc = default_measure_fits(p)) return rc;
    mcijit::ProblemShape sh = p->shape;
    sh.hcopy = kBigCopies;
    sh.det = 0;
    const std::string src = mcijit::generate_source(sh, MCI_VEGAS, mcijit::kUnitVegasMf1);
    Candidate c[2]; // [0] VGPR keys | [1] SGPR keys
    for (int i = 0; i < 2; ++i) {
        c[i].unit = mcijit::kUnitVegasMf1;
        c[i].src = std::string(i == 0 ? kVgprKeys : "") + src;
        c[i].threads = kBigThreads;
    }
    auto built = [](const Candidate &k) { return VegasBuilt{k.vgprs(), k.scratch(), true}; };
    if (c[0].build()) {
        b.state = VegasBigUnit::kNoCompile;
        return c[0].failed(" (big :vegas unit)");
    }
    VegasBuilt with = built(c[0]), without{0, 0, false};
    if (too_fat(with)) {
        if (c[1].build()) {
            b.state = VegasBigUnit::kNoCompile;
            return c[1].failed(" (big :vegas unit)");
        }
        without = built(c[1]);
    }
    bool keys = false;
    if (vegas_big_budget(with, without.ok ? &without : nullptr, &keys) != 1) {
        b.state = VegasBigUnit::kOverBudget;
        return MCI_OK;
    }
    const int64_t lds = sixteen_copies_lds(p);
    if (int rc = p->kernel[mci_problem::kVegasBig].load(p->ctx, c[keys ? 0 : 1], "mci_vegas_batch", lds, kSlotRules)) {
        b.state = VegasBigUnit::kNoCompile;
        return rc;
    }
    if (!p->ctx->offline) { // the grid of its cursor launches: what the runtime says is resident at once (one workgroup per CU)
        int per_cu = 0, cus = 0;
        HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p->kernel[mci_problem::kVegasBig].f, kBigThreads, (size_t)lds));
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->ctx->device));
        b.resident = per_cu * cus;
    }
    b.keys = keys;
    b.state = 1;
    return MCI_OK;
}

// ---- several lanes per chain (mci_spec.h) ---------------------------------------------------------------------------------
// the chain solver's kernel with a group of lanes per chain: its own code object (slots 5, 6), compiled when a launch first asks for it
static int compile_spec(mci_problem *p, int solver) {
    const int slot = solver == MCI_VEGASMC ? kSlotVegasmcSpec : kSlotMcmcSpec;
    if (p->kernel[slot].compiled) return MCI_OK;
    if (int rc = default_measure_fits(p)) return rc;
    p->shape.det = 0;
    Candidate c, lane;
    c.unit = mcijit::kUnitSpec;
    c.src = mcijit::generate_source(p->shape, solver, mcijit::kUnitSpec);
    c.threads = 256; // (a launch of few chains runs one wave per SIMD: up to 512 registers per lane)
    // In the cache, with the marker of a passed self-check next to it: nothing else to do.  Otherwise the lane-per-chain unit the check
    // compares it with is compiled NEXT to it (hiprtc is re-entrant): the check costs the slower of the two compilations, not their sum.
    const bool cached = c.build(/*cache_only=*/true) == 0;
    const bool verified = cached && access((c.path + ".ok").c_str(), F_OK) == 0;
    std::thread side;
    if (!verified && !p->kernel[solver].compiled && !p->ctx->offline && !(g_over.spec_self_check.on && g_over.spec_self_check.v == 0)) {
        lane.src = mcijit::generate_source(p->shape, solver, mcijit::kUnitSolver);
        lane.threads = p->threads;
        side = std::thread([&lane] { lane.build(); });
    }
    if (!cached) {
        if (c.build() == 2) {
            // (the unit is built with a backend switch, mci_jit.h: a compiler that does not know it any more gets the unit without it --
            // the self-check below is what stands between such an object and the user's histogram)
            std::string log2;
            Candidate d;
            d.unit = c.unit;
            d.src = c.src;
            d.threads = c.threads;
            d.rc = mcijit::compile(d.src, d.threads, d.code, log2, d.cached, &d.path, mcijit::kUnitSpec, false, /*no_exec_mask_flag=*/true);
            if (d.rc == 0) {
                d.log = c.log;
                c = std::move(d);
            }
        }
    }
    if (side.joinable()) side.join();
    if (c.rc) return c.failed();
    if (int rc = load_slot(p, slot, c, p->lds_bytes)) return rc;
    p->spec_need_check[solver - 1] = !verified;
    if (verified && p->spec_state[solver - 1] == 0) p->spec_state[solver - 1] = 1;
    return MCI_OK;
}

// The comparison of two packed buffers both self-checks use (spec_self_check below, vegas_self_check in mci_host_check.h): the statistics
// head [0, nstat) to 1e-9, everything behind it (histogram, propose / accept tables) to 1e-8, relative to the larger entry with 1e-3 of
// the section's largest entry as the floor.  Entries [0, skip) are left out (the observable sums under a user measure, which the static
// kernel cannot run).  Non-finite entries agree when they are the same kind of non-finite.  nhist >= 0 (vegas_self_check): the histogram
// [nstat, nstat + nhist) is a section of its own, measured against ITS OWN largest entry -- next to the propose / accept tables, which a
// :vegas launch leaves at their clearStatistics! values of ~1e-8, every histogram entry below ~1e-19 would compare equal to anything;
// hist_top is that largest entry (0: the histogram holds nothing the comparison could have looked at).
namespace {
struct PackedDiff {
    long bad = 0, first_bad = -1;
    long bad_sec[3] = {0, 0, 0}; // ... in the statistics head | behind it (nhist >= 0: the histogram) | the tables behind the histogram
    double worst = 0.0;       // largest difference, in units of its section's largest entry
    double hist_top = 0.0;    // nhist >= 0: largest entry of the histogram section, either side
};
void compare_packed(const double *x, const double *y, size_t nstat, size_t n, size_t skip, PackedDiff *out, long nhist = -1) {
    PackedDiff r;
    const size_t hend = nhist >= 0 ? nstat + (size_t)nhist : n;
    for (int sec = 0; sec < (nhist >= 0 ? 3 : 2); ++sec) {
        const size_t lo = sec == 0 ? skip : sec == 1 ? nstat : hend, hi = sec == 0 ? nstat : sec == 1 ? hend : n;
        const double tol = sec ? 1e-8 : 1e-9;
        double top = 0.0;
        for (size_t i = lo; i < hi; ++i) top = std::fmax(top, std::fmax(std::fabs(x[i]), std::fabs(y[i])));
        if (sec == 1 && nhist >= 0) r.hist_top = top;
        for (size_t i = lo; i < hi; ++i) {
            const double a = x[i], b = y[i];
            const double d = std::fabs(a - b), lim = tol * (std::fmax(std::fabs(a), std::fabs(b)) + 1e-3 * top);
            const bool ok = (std::isfinite(a) && std::isfinite(b)) ? d <= lim : (std::isnan(a) == std::isnan(b) && (std::isnan(a) || a == b));
            if (!ok) {
                if (r.first_bad < 0) r.first_bad = (long)i;
                ++r.bad;
                ++r.bad_sec[sec];
                if (top > 0.0 && d / top > r.worst) r.worst = d / top;
            }
        }
    }
    *out = r;
}
} // namespace

// A NEW several-lanes-per-chain code object proves itself before it is trusted.  Every user integrand is a new translation unit, and
// one of ~1000 campaign layouts came out of ROCm 7.2's compiler with the right chains and its histogram adds in the wrong bins
// (profiles/r05_fuzz.txt: right estimates, a map adapting to noise, no error).  Both chain kernels of a problem are product kernels and
// step the SAME chain (same (chain, step)-addressed uniforms; nchain = 1 is the reference's chain, vegas_mc/montecarlo.jl:198-211), so
// the first launch through a code object without a marker is preceded by <= 2 blocks x <= 512 steps through it and through the
// lane-per-chain kernel, and the two packed buffers are compared: statistics to 1e-9, histogram and propose / accept tables to 1e-8
// (relative to the larger entry, with the section's largest entry as the floor).  Agreement: a marker file next to the code object,
// never checked again.  Disagreement: one warning, status -1, and the problem keeps one lane per chain.  The launch that triggered
// the check then runs as if nothing had happened: everything a launch leaves behind on the host side (p->launch) is put back.
static int spec_self_check(mci_problem *p, int solver, int G, int64_t nevalperblock, int64_t block_lo, int64_t block_hi, int32_t iteration,
                           uint64_t seed, int64_t measurefreq, double thermal_ratio) {
    const int slot = solver == MCI_VEGASMC ? kSlotVegasmcSpec : kSlotMcmcSpec;
    const int64_t nb = block_hi - block_lo < 2 ? block_hi - block_lo : 2, npb = nevalperblock < 512 ? nevalperblock : 512;
    const int64_t mf = measurefreq * 4 <= npb ? measurefreq : 1;
    // (the stored chains on the device are safe: the check launches run nchain = 1, so they keep none -- mci_iteration_run refuses to
    // otherwise -- and they log no block means)
    const mci_problem::LaunchState saved = p->launch; // (everything the two launches leave on the host: put back below)
    const int spec_lanes = p->spec_lanes, kernel_timing = p->kernel_timing; // (the two settings the check overrides)
    int rc = flush_merge(p);
    if (rc) return rc;
    int h_status[4] = {0, 0, 0, 0};
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    HIPCHK(hipMemcpy(h_status, p->d_status, sizeof(h_status), hipMemcpyDeviceToHost));
    std::vector<double> got[2];
    p->in_self_check = true;
    p->kernel_timing = 0;
    for (int pass = 0; pass < 2 && !rc; ++pass) {
        p->spec_lanes = pass == 0 ? G : 1;
        got[pass].assign((size_t)p->packed_n, 0.0);
        rc = mci_iteration_run(p, solver, npb, block_lo, block_lo + nb, iteration, seed, mf, 1, thermal_ratio);
        if (!rc) rc = mci_get_packed(p, got[pass].data(), p->packed_n); // (merges the launch and waits for it)
    }
    p->in_self_check = false;
    p->launch = saved;
    p->spec_lanes = spec_lanes;
    p->kernel_timing = kernel_timing;
    if (p->d_status) (void)hipMemcpy(p->d_status, h_status, sizeof(h_status), hipMemcpyHostToDevice); // (what the two small launches flagged is theirs)
    if (rc) return rc;
    PackedDiff df;
    compare_packed(got[0].data(), got[1].data(), (size_t)(2 * p->shape.nobs + 2 + p->ni + 1), (size_t)p->packed_n, 0, &df);
    const long bad = df.bad, first_bad = df.first_bad;
    const double worst = df.worst;
    p->spec_need_check[solver - 1] = false;
    if (bad == 0) {
        p->spec_state[solver - 1] = 1;
        const std::string id = mcijit::compiler_id() + "\n"; // (the marker: this code object has reproduced the lane-per-chain kernel on a device)
        mcijit::write_file_atomic(p->kernel[slot].code_object + ".ok", id.data(), id.size());
        return MCI_OK;
    }
    p->spec_state[solver - 1] = -1;
    fprintf(stderr, "mci: the several-lanes-per-chain kernel of this problem (%s, %s) does not reproduce its lane-per-chain kernel on a %lld-block, %lld-step "
                    "check: %ld of %lld packed entries differ (first at %ld, largest difference %.3g of its section's maximum).  A miscompiled code object -- "
                    "this problem keeps one lane per chain (same chains, slower for launches of few chains); mci_chain_speculation_status reports -1.\n",
            solver == MCI_VEGASMC ? ":vegasmc" : ":mcmc", p->kernel[slot].code_object.c_str(), (long long)nb, (long long)npb, bad, (long long)p->packed_n, first_bad, worst);
    return MCI_OK;
}

// The speculation tree of a group of `lanes` lanes: the `lanes` most probable nodes of the accept / reject tree of a chain whose
// steps change its configuration with probability `accept` (greedy: the most probable frontier node next; ties go to the older
// candidate), with at most `limit` accept edges on any way from the root (limit < 0: no bound).  accept -> 0 gives the reject chain,
// accept = 1/2 the complete binary tree.  Nodes are numbered in the order they are taken: ancestors first.
static const int kSpecMaxLevels = 12; // (:mcmc exchanges configurations once per accept level: mci_spec.h spec_wave_max counts below 64)
static void spec_build(int lanes, double accept, int limit, std::vector<mci::SpecNode> &tab, int *maxacc) {
    struct Cand { double prob; int parent; bool via_acc; long seq; };
    std::vector<Cand> front;
    front.push_back({1.0, -1, false, 0});
    long seq = 1;
    tab.clear();
    *maxacc = 0;
    while ((int)tab.size() < lanes && !front.empty()) {
        size_t best = 0;
        for (size_t i = 1; i < front.size(); ++i)
            if (front[i].prob > front[best].prob || (front[i].prob == front[best].prob && front[i].seq < front[best].seq)) best = i;
        const Cand cd = front[best];
        front.erase(front.begin() + (long)best);
        mci::SpecNode nd{};
        if (cd.parent < 0) {
            nd.depth = 0;
            nd.anc = -1;
            nd.nacc = 0;
            nd.needacc = nd.needrej = nd.accdepth = 0ull;
        } else {
            const mci::SpecNode &pn = tab[(size_t)cd.parent];
            nd.depth = pn.depth + 1;
            nd.anc = cd.via_acc ? cd.parent : pn.anc;
            nd.nacc = pn.nacc + (cd.via_acc ? 1 : 0);
            nd.needacc = pn.needacc | (cd.via_acc ? 1ull << cd.parent : 0ull);
            nd.needrej = pn.needrej | (cd.via_acc ? 0ull : 1ull << cd.parent);
            nd.accdepth = pn.accdepth | (cd.via_acc ? 1ull << pn.depth : 0ull);
        }
        const int me = (int)tab.size();
        tab.push_back(nd);
        if (nd.nacc > *maxacc) *maxacc = nd.nacc;
        front.push_back({cd.prob * (1.0 - accept), me, false, seq++});
        if ((limit < 0 || nd.nacc + 1 <= limit) && nd.nacc + 1 <= kSpecMaxLevels) front.push_back({cd.prob * accept, me, true, seq++});
    }
    int deepest = 0;
    for (auto &nd : tab) deepest = nd.depth > deepest ? nd.depth : deepest;
    unsigned long long any = 0ull;
    for (auto &nd : tab) any |= nd.accdepth;
    for (auto &nd : tab) {
        nd.levels = *maxacc | (deepest << 8);
        nd.anydepth = any;
    }
}

// The trees of the next launch on the device (rebuilt when lanes / acceptance / limit change).  accept > 0: that one tree.  accept <= 0
// (the default): the solver's family of trees, one per assumed acceptance -- a group starts on `first` and moves, every few trips, to the
// tree built for the acceptance its chain has shown (mci_spec.h spec_adapt).  :vegasmc proposals do not depend on the configuration they
// start from, an accept level costs one exchange: unbounded; :mcmc runs mcmc_propose once per level: at most `limit` (default 2, 3 on the
// trees for chains that accept most steps).
static int spec_upload(mci_problem *p, int solver, int lanes, double accept, int limit) {
    const double key = accept > 0.0 ? accept : -(double)(solver + 1);
    if (p->d_spec_tab && p->spec_tab_lanes == lanes && p->spec_tab_accept == key && p->spec_tab_limit == limit) return MCI_OK;
    static const double fam_vegasmc[7] = {0.03, 0.12, 0.3, 0.5, 0.7, 0.85, 0.93}, fam_mcmc[6] = {0.03, 0.1, 0.2, 0.35, 0.55, 0.8};
    std::vector<mci::SpecNode> all;
    p->spec_ntree = 0;
    p->spec_tab_maxacc = 0;
    auto add = [&](double acc, int lim) {
        std::vector<mci::SpecNode> tab;
        int maxacc = 0;
        spec_build(lanes, acc, lim, tab, &maxacc);
        all.insert(all.end(), tab.begin(), tab.end());
        p->spec_accepts[p->spec_ntree++] = (float)acc;
        if (maxacc > p->spec_tab_maxacc) p->spec_tab_maxacc = maxacc;
    };
    if (accept > 0.0) {
        add(accept, limit);
        p->spec_first = 0;
    } else if (solver == MCI_VEGASMC) {
        for (double acc : fam_vegasmc) add(acc, limit);
        p->spec_first = 3;
    } else {
        for (double acc : fam_mcmc) add(acc, limit >= 0 ? limit : (acc >= 0.5 ? 3 : 2));
        p->spec_first = 3;
    }
    if (int rc = p->d_spec_tab.reserve(8 * 64)) return rc;
    // (pageable source: the copy has left `all` when the call returns)
    HIPCHK(hipMemcpyAsync(p->d_spec_tab, all.data(), all.size() * sizeof(mci::SpecNode), hipMemcpyHostToDevice, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    p->spec_tab_lanes = lanes;
    p->spec_tab_accept = key;
    p->spec_tab_limit = limit;
    return MCI_OK;
}

int mci_set_chain_speculation(mci_problem *p, int32_t lanes, double accept, int32_t max_accepts) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (lanes != -1 && (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)))) return fail(MCI_ERR_INVALID, "lanes per chain: -1 (automatic), 1 (one lane per chain) or a power of two up to 64");
    if (accept >= 1.0) return fail(MCI_ERR_INVALID, "the acceptance a speculation tree is built for lies in (0, 1); <= 0: the solver's default");
    p->spec_lanes = lanes;
    p->spec_accept = accept > 0.0 ? accept : 0.0;
    p->spec_maxacc = max_accepts < 0 ? -1 : max_accepts;
    return MCI_OK;
}

int mci_last_integrate_discarded(const mci_problem *p, int64_t *neval, int32_t *launches) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (neval) *neval = p->last_discarded_neval;
    if (launches) *launches = p->last_discarded_launches;
    return MCI_OK;
}

int mci_chain_speculation_status(const mci_problem *p, int32_t solver, int32_t *status) {
    if (!p || !status || (solver != MCI_VEGASMC && solver != MCI_MCMC)) return fail(MCI_ERR_INVALID, "solver MCI_VEGASMC or MCI_MCMC");
    *status = p->spec_state[solver - 1];
    return MCI_OK;
}

int mci_last_chain_speculation(const mci_problem *p, int32_t *lanes, int32_t *max_accepts) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (lanes) *lanes = p->launch.last_spec_lanes;
    if (max_accepts) *max_accepts = p->launch.last_spec_maxacc;
    return MCI_OK;
}

int mci_speculation_tree(int32_t lanes, double accept, int32_t max_accepts, int32_t *depth, int32_t *anc, int32_t *nacc, uint64_t *needacc, uint64_t *needrej) {
    if (lanes < 1 || lanes > 64 || !(accept > 0.0 && accept < 1.0)) return fail(MCI_ERR_INVALID, "speculation tree: 1..64 lanes, acceptance in (0, 1)");
    std::vector<mci::SpecNode> tab;
    int maxacc = 0;
    spec_build(lanes, accept, max_accepts, tab, &maxacc);
    for (int i = 0; i < lanes; ++i) {
        if (depth) depth[i] = tab[(size_t)i].depth;
        if (anc) anc[i] = tab[(size_t)i].anc;
        if (nacc) nacc[i] = tab[(size_t)i].nacc;
        if (needacc) needacc[i] = tab[(size_t)i].needacc;
        if (needrej) needrej[i] = tab[(size_t)i].needrej;
    }
    return MCI_OK;
}

int mci_compile_chain_speculation(mci_problem *p, int32_t solver) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (solver != MCI_VEGASMC && solver != MCI_MCMC) return fail(MCI_ERR_INVALID, "several lanes per chain: solver MCI_VEGASMC or MCI_MCMC");
    if (p->shape.host_integrand) return fail(MCI_ERR_INVALID, "a host integrand keeps one lane per chain");
    return compile_spec(p, solver);
}

int mci_compile(mci_problem *p) { return compile_solver(p, MCI_VEGAS); }

int mci_kernel_code_object(mci_problem *p, int32_t solver, char *buf, int32_t n) {
    if (!p || !buf || n < 1) return fail(MCI_ERR_INVALID, "NULL argument");
    // which unit the name means, and what it is called when it is not there yet
    int k = -1;
    std::string what = "solver " + std::to_string(solver);
    if (solver == MCI_VEGAS_PERSISTENT) k = mci_problem::kPersist, what = "the persistent :vegas kernel";
    else if (solver == MCI_VEGAS_PERSISTENT_UNTIL) k = mci_problem::kPersistUntil, what = "the persistent :vegas kernel with a target error";
    else if (solver == MCI_VEGASMC_LANES || solver == MCI_MCMC_LANES) k = solver == MCI_VEGASMC_LANES ? kSlotVegasmcSpec : kSlotMcmcSpec, what = "the several-lanes-per-chain kernel";
    else if (solver == MCI_VEGAS_STRAT) k = mci_problem::kStrat, what = "the stratified :vegas kernel";
    else if (const int w = sweep_unit_of(solver); w >= 0) k = mci_problem::kSweep + w, what = std::string("the sweep kernel") + kSweepUnits[w].for_what;
    else if (solver == MCI_VEGAS_BIG) k = mci_problem::kVegasBig, what = "the big :vegas unit";
    else if (solver < 0 || solver > 2) return fail(MCI_ERR_INVALID, "Solver %d is not supported!", solver);
    // (:vegas: the unit the last :vegas launch ran -- the big one behind a big launch, the standing one before any launch and behind a small one)
    else if (solver == MCI_VEGAS && p->launch.last_vegas_big && p->kernel[mci_problem::kVegasBig].compiled) k = mci_problem::kVegasBig;
    else k =(solver == MCI_VEGAS && !p->kernel[solver].compiled && p->kernel[kSlotVegasAny].compiled) ? kSlotVegasAny : solver;
    if (!p->kernel[k].compiled) return fail(MCI_ERR_INVALID, "%s has not been compiled yet", what.c_str());
    snprintf(buf, (size_t)n, "%s", p->kernel[k].code_object.c_str());
    return MCI_OK;
}

int mci_set_rng_bits(mci_problem *p, int32_t bits) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (bits != 52 && bits != 32) return fail(MCI_ERR_INVALID, "rng bits must be 52 (default: the resolution of rand(Float64)) or 32");
    if (p->shape.rng_bits != bits) {
        p->shape.rng_bits = bits;
        drop_modules(p);
    }
    return MCI_OK;
}

int mci_set_rng_rounds(mci_problem *p, int32_t rounds) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (rounds != 10 && rounds != 7) return fail(MCI_ERR_INVALID, "Philox4x32 rounds must be 10 (default) or 7 (the fewest that pass BigCrush)");
    if (p->shape.rng_rounds != rounds) {
        p->shape.rng_rounds = rounds;
        drop_modules(p);
    }
    return MCI_OK;
}

int mci_set_train_walk(mci_problem *p, int32_t mode) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (mode < -1 || mode > 2) return fail(MCI_ERR_INVALID, "train walk mode must be -1 (automatic), 0 (prefix scan), 1 (serial recurrence) or 2 (serial recurrence, general form only)");
    p->train_serial = mode;
    return MCI_OK;
}

// csrc/mci_debug.h
int mci_debug_plant_wrong_decision(mci_problem *p, int32_t on) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    p->debug_wrong_decision = on != 0;
    return MCI_OK;
}

int mci_debug_override(const char *key, int64_t value, int32_t on) {
    Override *o = override_slot(key);
    if (!o) return fail(MCI_ERR_INVALID, "no such override: %s", key ? key : "(null)");
    o->on = on != 0;
    o->v = value;
    return MCI_OK;
}

int mci_debug_split_chunks(const mci_problem *p, int64_t *chunks, int64_t *bytes) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (chunks) *chunks = p->launch.last_split_chunks;
    if (bytes) *bytes = p->launch.last_split_bytes;
    return MCI_OK;
}

int mci_debug_vegas_cursor(const mci_problem *p, int32_t *used, uint64_t *base) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (used) *used = p->launch.last_cursor ? 1 : 0;
    if (base) *base = p->cursor_base;
    return MCI_OK;
}

int mci_debug_compiler_id(const char *set, char *out, int32_t n) {
    if (set) mcijit::compiler_id_override() = set; // ("" takes the override back)
    if (out && n > 0) snprintf(out, (size_t)n, "%s", mcijit::compiler_id().c_str());
    return MCI_OK;
}

int mci_debug_mcmc_policy(int64_t pilot_steps, int64_t grow, int64_t carry_holds, int64_t carry_half_floors) {
    if (pilot_steps > 0) mci_problem::kMcmcPilotSteps = pilot_steps;
    if (grow > 0) mci_problem::kMcmcGrow = grow;
    if (carry_holds > 0) mci_problem::kMcmcCarryHolds = carry_holds;
    if (carry_half_floors > 0) mci_problem::kMcmcCarryHalfFloors = carry_half_floors;
    return MCI_OK;
}

int mci_debug_persist_spin_ticks(mci_problem *p, unsigned long long ticks) {
    if (!p || ticks == 0) return fail(MCI_ERR_INVALID, "bad argument");
    p->persist_spin_ticks = ticks;
    return MCI_OK;
}

int mci_set_deterministic(mci_problem *p, int32_t on) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    const bool want = on != 0;
    if (want != p->deterministic) {
        p->deterministic = want;
        p->shape.det = want ? 1 : 0;
        drop_modules(p);
    }
    return MCI_OK;
}

int mci_set_chain_carry(mci_problem *p, int32_t mode) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (mode < -1 || mode > 1) return fail(MCI_ERR_INVALID, "chain carry mode must be -1 (automatic) or 1 (many-chain launches of :vegasmc and :mcmc continue the chains of the iteration before) or 0 (every launch starts its chains afresh)");
    p->chain_carry = mode;
    if (mode == 0) p->launch.chain_valid = false;
    return MCI_OK;
}

int mci_set_iteration_counted(mci_problem *p, int32_t counted) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    p->launch_counted = counted != 0;
    return MCI_OK;
}

int mci_set_persistent(mci_problem *p, int32_t mode) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (mode < -1 || mode > 1) return fail(MCI_ERR_INVALID, "persistent mode must be -1 (automatic: launch-bound :vegas calls), 0 (one launch chain per iteration) or 1 (whenever the layout allows)");
    p->persistent = mode;
    return MCI_OK;
}

// development aid (tools/persist_trace.py): the raw counter / stamp words of the persistent kernel
int mci_debug_persist_words(mci_problem *p, unsigned long long *out, int32_t n) {
    if (!p || !out || !p->d_persist) return fail(MCI_ERR_INVALID, "no persistent launch yet");
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    HIPCHK(hipMemcpy(out, p->d_persist, (size_t)(n < (int)kPersistWords ? n : (int)kPersistWords) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return MCI_OK;
}

// development aid (tools/fuzz_layouts.py --walk): how many serial walks of train! ran as slots with given decisions, how many in the general form
int mci_debug_walk_counts(mci_problem *p, int64_t *out) {
    if (!p || !out || !p->d_status) return fail(MCI_ERR_INVALID, "NULL argument");
    int h[2] = {0, 0};
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    HIPCHK(hipMemcpy(h, p->d_status + 1, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0];
    out[1] = h[1];
    return MCI_OK;
}

int mci_last_integrate_persistent(const mci_problem *p, int32_t *persistent) {
    if (!p || !persistent) return fail(MCI_ERR_INVALID, "NULL argument");
    *persistent = p->last_persistent ? 1 : 0;
    return MCI_OK;
}

int mci_last_chain_launch(const mci_problem *p, int64_t *nchain, int32_t *carried) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (nchain) *nchain = p->launch.last_nchain;
    if (carried) *carried = p->launch.last_carried ? 1 : 0;
    return MCI_OK;
}

int mci_check_status(mci_problem *p) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    return check_status(p);
}
static int compile_persist(mci_problem *p, bool background, bool until);
static bool persist_layout_ok(const mci_problem *p);
static int compile_strat(mci_problem *p); // (mci_host_strat.h)
static int compile_sweep_unit(mci_problem *p, int which); // (mci_host_sweep.h)
static bool sweep_leaves_unit(const mci_problem *p);
static bool sweep_strat_leaves_unit(const mci_problem *p);
int mci_compile_solver(mci_problem *p, int32_t solver) {
    if (solver == MCI_VEGAS_PERSISTENT) { // the persistent :vegas kernel (mci_set_persistent), for layouts that allow it
        if (!persist_layout_ok(p)) return fail(MCI_ERR_INVALID, "this layout has no persistent :vegas kernel (mci_set_persistent)");
        return compile_persist(p, false, false);
    }
    if (solver == MCI_VEGAS_PERSISTENT_UNTIL) { // ... and the one mci_integrate_until launches
        if (!persist_layout_ok(p)) return fail(MCI_ERR_INVALID, "this layout has no persistent :vegas kernel (mci_set_persistent)");
        return compile_persist(p, false, true);
    }
    if (solver == MCI_VEGASMC_LANES || solver == MCI_MCMC_LANES) return mci_compile_chain_speculation(p, solver == MCI_VEGASMC_LANES ? MCI_VEGASMC : MCI_MCMC);
    if (solver == MCI_VEGAS_STRAT) { // (mci_host_strat.h)
        if (!p->strat.on) return fail(MCI_ERR_INVALID, "the problem is not stratified (mci_set_stratification)");
        return compile_strat(p);
    }
    if (const int w = sweep_unit_of(solver); w >= 0) { // (mci_host_sweep.h: a problem the unit's own query accepts)
        mci_integrate_args a{};
        a.solver = MCI_VEGAS;
        a.measurefreq = 1;
        a.niter = 1;
        if (w == mci_problem::Sweep::kChains || w == mci_problem::Sweep::kChainsCarry || w == mci_problem::Sweep::kChainsResume) { // (the layout alone, as below: any chain count the call may bring)
            a.solver = MCI_VEGASMC;
            a.nchain = 1;
            a.neval = (int64_t)1 << 40;
            a.block = 1;
            if (int rc = mci_sweep_chains_supported(p, &a, nullptr, 0)) return rc;
        } else if (w == mci_problem::Sweep::kMcmc || w == mci_problem::Sweep::kMcmcCarry || w == mci_problem::Sweep::kMcmcResume) { // (likewise)
            a.solver = MCI_MCMC;
            a.nchain = 1;
            a.neval = (int64_t)1 << 30; // (steps + nburn of the one chain stay below 2^31 - 1)
            a.block = 1;
            a.thermal_ratio = 0.1;
            if (int rc = mci_sweep_mcmc_supported(p, &a, nullptr, 0)) return rc;
        } else if (w == mci_problem::Sweep::kStrat || w == mci_problem::Sweep::kStratLeaves) {
            a.neval = (int64_t)1 << 40; // (the plan is the call's: here only the layout is asked about)
            a.block = 1;
            if (int rc = mci_sweep_strat_supported(p, &a, nullptr, 0)) return rc;
            // (which of the two a stratified sweep of this problem runs: whether it has opted in, mci_set_sweep_strat_leaves, and is no one-grid layout)
            if (w == mci_problem::Sweep::kStrat && sweep_strat_leaves_unit(p))
                return fail(MCI_ERR_INVALID, "a stratified sweep of this problem runs the sweep kernel for several leaves (MCI_VEGAS_SWEEP_STRAT_LEAVES; mci_set_sweep_strat_leaves)");
            if (w == mci_problem::Sweep::kStratLeaves && !sweep_strat_leaves_unit(p))
                return fail(MCI_ERR_INVALID, "a stratified sweep of this problem runs the one-grid stratified sweep kernel (MCI_VEGAS_SWEEP_STRAT; mci_set_sweep_strat_leaves)");
        } else {
            const bool until = w == mci_problem::Sweep::kUntil || w == mci_problem::Sweep::kLeavesUntil;
            const mci_sweep_target any{0.0, 0.0, 0}; // (the `until` units: their own query, for the LDS their histogram copies take)
            if (int rc = until ? mci_sweep_until_supported(p, &a, &any, nullptr, 0) : mci_sweep_supported(p, &a, nullptr, 0)) return rc;
            // (which of the two a sweep of this problem runs: whether it has opted in, mci_set_sweep_leaves, and is no one-grid layout)
            if ((w == mci_problem::Sweep::kOne || w == mci_problem::Sweep::kUntil) && sweep_leaves_unit(p))
                return fail(MCI_ERR_INVALID, "a sweep of this problem runs the sweep kernel for several leaves (MCI_VEGAS_SWEEP_LEAVES; mci_set_sweep_leaves)");
            if ((w == mci_problem::Sweep::kLeaves || w == mci_problem::Sweep::kLeavesUntil) && !sweep_leaves_unit(p))
                return fail(MCI_ERR_INVALID, "a sweep of this problem runs the one-grid sweep kernel (MCI_VEGAS_SWEEP; mci_set_sweep_leaves)");
        }
        return compile_sweep_unit(p, w);
    }
    if (solver == MCI_VEGAS_BIG) { // the big :vegas unit, for layouts that have one (launches compile it by themselves when they first select it)
        if (!vegas_big_layout(p)) return fail(MCI_ERR_INVALID, "this layout has no big :vegas unit (the eight-copy plan of the pipelined one-tile loop, sixteen copies within the CU's LDS)");
        if (int rc = compile_vegas_big(p)) return rc;
        if (p->vegas_big.state == VegasBigUnit::kOverBudget) return fail(MCI_ERR_COMPILE, "the big :vegas unit needs more than %ld VGPRs or scratch at 1024 threads: big launches keep the standing unit", kVgprsTwoWide);
        if (p->vegas_big.state == VegasBigUnit::kNoCompile) return fail(MCI_ERR_COMPILE, "the big :vegas unit did not compile");
        return MCI_OK;
    }
    if (solver < 0 || solver > 2) return fail(MCI_ERR_INVALID, "Solver %d is not supported!", solver); // main.jl:263
    return compile_solver(p, solver);
}

int mci_get_histogram_copies(const mci_problem *p, int32_t *copies) {
    if (!p || !copies) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->launch.last_vegas_big) *copies = kBigCopies; // (the unit the last :vegas launch ran)
    else *copies = (p->kernel[MCI_VEGAS].compiled || p->kernel[kSlotVegasAny].compiled) ? p->shape.hcopy : planned_hcopy(p, nullptr);
    return MCI_OK;
}

int mci_problem_info(const mci_problem *p, int32_t *ndraw, int32_t *nobs, int64_t *packed_size, int32_t *table_mode, int64_t *lds_bytes) {
    if (ndraw) *ndraw = p->shape.ndraw;
    if (nobs) *nobs = p->shape.nobs;
    if (packed_size) *packed_size = p->packed_n;
    if (table_mode) *table_mode = p->shape.table_mode;
    if (lds_bytes) *lds_bytes = p->lds_bytes;
    return MCI_OK;
}

