// mci_host_check.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// the self-check of a new :vegas code object against the static kernel k_check_vegas (mci_check.h).
//
// Every user integrand is a new hiprtc translation unit, and the :vegas units -- hand-pipelined loop, interleaved histogram copies --
// are the most aggressive code handed to that compiler.  The first mci_iteration_run through a classic single-tile :vegas sample kernel
// that has no marker next to it in the kernel cache is therefore preceded by <= 2 blocks x <= 512 samples through it; the same samples
// go through mci_sample_dump (map + integrand only, its own small code object) and k_check_vegas, and the two packed buffers are
// compared with the rule of spec_self_check (compare_packed: relative to the larger entry, with 1e-3 of the SECTION's largest entry as
// the floor).  What a section is decides what the rule can see.  1024 samples of a peaked integrand on an untrained map put anything
// between 1e-27 and 1e-5 into their fullest bin (the 16-D Gaussian, seeds 1 .. 39), so the histogram is (a) merged and compared WITHOUT the
// clearStatistics! offsets -- next to 3e-10 the rule's limit is ~3e-18 absolute, and the headline layout with every add one bin off
// passed -- and (b) a section of its own, measured against its own largest entry, not against the propose / accept tables behind it
// (3e-8 after a :vegas launch: a floor of 3e-19).  A histogram whose largest entry is zero on both sides (every weight underflowed) has
// not been compared: no marker, status stays 0, flag bit 2.  Agreement: a marker file, never checked again.  Disagreement: one
// warning, the unit is compiled again in the generator's most conservative layout (plain loop, one histogram copy) and checked the same
// way; that object is used from then on (status -1; -2 and a second warning if it disagrees too).  Advisory: the call returns MCI_OK.
// What is covered: DESIGN.md section 9 item 0.

// the run-time layout table of k_check_vegas, from the problem's static shape
namespace {
struct CheckLayout {
    std::vector<mci::CheckDraw> draw;
    std::vector<mci::CheckIntegrand> intg;
};
// layouts the check covers: device integrand and measure, one histogram tile, no FermiK leaf (:vegas refuses those anyway)
bool vegas_check_covers(const mci_problem *p) {
    const auto &s = p->shape;
    if (s.host_integrand || s.host_measure || s.ntile != 1 || p->has_fermik || p->strat.on) return false;
    for (int i = 0; i < s.ni; ++i) // (binned observables are real, mci_device.h measure: the static kernel adds w[i], not a (re, im) pair)
        if (s.ncomp != 1 && s.obs_bin_draw[(size_t)i] >= 0) return false;
    return s.ndraw >= 1 && s.ndraw <= 64;
}
void vegas_check_layout(const mci_problem *p, CheckLayout *out) {
    const auto &s = p->shape;
    CheckLayout &L = *out;
    for (int k = 0; k < s.ndraw; ++k) {
        const int leaf = s.draw_leaf[(size_t)k];
        mci::CheckDraw d{};
        d.kind = s.leaf_kind[(size_t)leaf];
        d.off = s.leaf_eoff[(size_t)leaf];
        d.doff = s.leaf_doff[(size_t)leaf];
        d.nbin = s.leaf_nbin[(size_t)leaf];
        d.boff = s.leaf_boff[(size_t)leaf];
        d.hist = (s.leaf_adapt[(size_t)leaf] != 0 && s.cover_mask[(size_t)k] != 0ull) ? 1 : 0;
        d.scale = d.kind == 0 ? (double)d.nbin : 1.0;
        d.lower = s.leaf_lower[(size_t)leaf];
        L.draw.push_back(d);
    }
    for (int i = 0; i < s.ni; ++i) {
        mci::CheckIntegrand g{};
        g.own = s.own_mask[(size_t)i];
        g.obs_off = s.obs_off[(size_t)i];
        g.obs_nbin = s.obs_nbin[(size_t)i];
        g.obs_bin_draw = s.obs_bin_draw[(size_t)i];
        L.intg.push_back(g);
    }
}
struct DevFree { // (freed on every way out)
    void *p = nullptr;
    ~DevFree() { if (p) (void)hipFree(p); }
};
} // namespace

static int sample_dump_device(mci_problem *p, int32_t iteration, uint64_t seed, int64_t first_index, int64_t n); // (mci_host_access.h)

// The :vegas units of the problem in the generator's most conservative layout from here on: the plain sample loop (no hand pipelining),
// one histogram copy, the default workgroup size -- what the table_mode / hist_copies overrides and MCI_VEGAS_PLAIN_LOOP select.  The
// deterministic mode keeps its copy per wave (that is what makes it deterministic) and loses the pipelined loop only.  `slot` is compiled
// at once, the other cadence variant when a launch next needs it; the persistent launch (its own, pipelined unit) is no longer taken
// (mci_host_integrate.h persist_plan looks at vegas.conservative).
static int vegas_make_conservative(mci_problem *p, int slot) {
    p->vegas.make_conservative(p->deterministic);
    if (!p->deterministic) p->shape.hcopy = 1;
    p->kernel[MCI_VEGAS].drop();
    p->kernel[kSlotVegasAny].drop();
    p->vegas_check_done[0] = p->vegas_check_done[1] = false;
    return compile_solver(p, slot);
}

// One :vegas iteration of blocks [block_lo, block_lo + nblocks) x nevalperblock samples through k_check_vegas, into `packed` (the layout
// of mci_get_packed).  hx / hjac / hw != NULL: the dumped samples come from the caller ([nblocks * nevalperblock][...], block after
// block); NULL: from mci_sample_dump of this problem.  bad[0] / bad[1]: samples whose x / jac the kernel does not reproduce.
// hist_offsets = false: the histogram section without the clearStatistics! offsets (MergeArgs::hist_no_offset: what the self-check compares).
static int vegas_check_reference(mci_problem *p, int32_t iteration, uint64_t seed, int64_t nevalperblock, int64_t block_lo, int64_t nblocks,
                                 int64_t measurefreq, const double *hx, const double *hjac, const double *hw, double *packed, int64_t *bad,
                                 bool hist_offsets) {
    const auto &s = p->shape;
    if (!vegas_check_covers(p)) return fail(MCI_ERR_INVALID, "this layout has no static :vegas check (host closures, several histogram tiles, stratification)");
    if (nblocks < 1 || nevalperblock < 1 || nblocks * nevalperblock > 1024 || measurefreq < 1) return fail(MCI_ERR_INVALID, "the static :vegas check runs 1..1024 samples per launch");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    CheckLayout L;
    vegas_check_layout(p, &L);
    const int nw = s.ni * s.ncomp;
    const int64_t n = nevalperblock, per = s.ndraw + 1 + nw;
    const size_t nraw = (size_t)nblocks * s.ncols + (size_t)(s.nbin ? s.nbin : 1);
    DevFree d_draw, d_intg, d_raw, d_bad, d_in;
    HIPCHK(hipMalloc(&d_draw.p, L.draw.size() * sizeof(mci::CheckDraw)));
    HIPCHK(hipMalloc(&d_intg.p, L.intg.size() * sizeof(mci::CheckIntegrand)));
    HIPCHK(hipMalloc(&d_raw.p, nraw * sizeof(double)));
    HIPCHK(hipMalloc(&d_bad.p, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemcpyAsync(d_draw.p, L.draw.data(), L.draw.size() * sizeof(mci::CheckDraw), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_intg.p, L.intg.data(), L.intg.size() * sizeof(mci::CheckIntegrand), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_raw.p, 0, nraw * sizeof(double), st));
    HIPCHK(hipMemsetAsync(d_bad.p, 0, 2 * sizeof(unsigned long long), st));
    if (hx) HIPCHK(hipMalloc(&d_in.p, (size_t)(nblocks * n * per) * sizeof(double)));
    mci::CheckArgs a{};
    a.draw = (const mci::CheckDraw *)d_draw.p;
    a.intg = (const mci::CheckIntegrand *)d_intg.p;
    a.ndraw = s.ndraw;
    a.ni = s.ni;
    a.ncomp = s.ncomp;
    a.nobs = s.nobs;
    a.ncols = s.ncols;
    a.rng_bits = s.rng_bits;
    a.rng_rounds = s.rng_rounds;
    a.with_obs = s.measure_body.empty() ? 1 : 0;
    fill_tables(p, a);
    a.seed = seed;
    a.iteration = (unsigned)iteration;
    a.neval_per_block = nevalperblock;
    a.measurefreq = measurefreq;
    a.hist = (double *)d_raw.p + (size_t)nblocks * s.ncols;
    a.bad = (unsigned long long *)d_bad.p;
    const int64_t total = nblocks * n;
    if (hx) {
        double *in = (double *)d_in.p;
        HIPCHK(hipMemcpyAsync(in, hx, (size_t)total * s.ndraw * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(in + total * s.ndraw, hjac, (size_t)total * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(in + total * (s.ndraw + 1), hw, (size_t)total * nw * sizeof(double), hipMemcpyHostToDevice, st));
        a.x = in;
    } else {
        // (the blocks are consecutive stretches of the sample index; the dump stays on the device: x | jac | w in p->d_dump)
        if (int rc = sample_dump_device(p, iteration, seed, block_lo * nevalperblock, total)) return rc;
        p->check_launches += 1;
        a.x = p->d_dump;
    }
    a.jac = a.x + total * s.ndraw;
    a.w = a.jac + total;
    a.block_lo = block_lo;
    a.n = total;
    a.cols = (double *)d_raw.p;
    hipLaunchKernelGGL(mci::k_check_vegas, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    p->check_launches += 1;
    std::vector<double> raw(nraw);
    unsigned long long hbad[2] = {0ull, 0ull};
    HIPCHK(hipMemcpyAsync(raw.data(), d_raw.p, nraw * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hbad, d_bad.p, sizeof(hbad), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) {
        bad[0] = (int64_t)hbad[0];
        bad[1] = (int64_t)hbad[1];
    }
    // block sums -> packed, as the merge forms it (mci_train.h merge_stats, merge_hist_bin, merge_pa): every block and the merged config
    // start from clearStatistics! values (configuration.jl:238-250)
    const int nobs = s.nobs, cnorm = nobs, cneval = nobs + 1, cvis = nobs + 2;
    for (int64_t i = 0; i < p->packed_n; ++i) packed[i] = 0.0;
    double norm = 1.0e-10, neval = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const double *row = raw.data() + (size_t)b * s.ncols;
        const double nb = row[cnorm] + 1.0e-10;
        for (int o = 0; o < nobs; ++o) {
            const double m = row[o] / nb;
            packed[o] += m;
            packed[nobs + o] += m * m;
        }
        norm += nb;
        neval += row[cneval];
    }
    packed[2 * nobs] = norm;
    packed[2 * nobs + 1] = neval;
    for (int i = 0; i < s.ni + 1; ++i) {
        double v = 1.0e-8;
        for (int64_t b = 0; b < nblocks; ++b) v += raw[(size_t)b * s.ncols + cvis + i] + 1.0e-8;
        packed[2 * nobs + 2 + i] = v;
    }
    for (int i = 0; i < s.nbin; ++i) packed[p->nstat + i] = (hist_offsets ? (double)(nblocks + 1) * 1.0e-10 : 0.0) + raw[(size_t)nblocks * s.ncols + i];
    for (int e = 0; e < 2 * p->npa && p->nstat + s.nbin + e < p->packed_n; ++e)
        packed[p->nstat + s.nbin + e] = (double)(nblocks + 1) * (e < p->npa ? 1.0e-8 : 1.0e-10);
    return MCI_OK;
}

// one round of the check on the loaded code object of `slot`: 0 agreement, 1 disagreement (what differs in *df / bad)
static int vegas_check_round(mci_problem *p, int slot, int64_t npb, int64_t block_lo, int64_t nb, int32_t iteration, uint64_t seed, int64_t mf, PackedDiff *df,
                             int64_t *bad, bool *differs) {
    std::vector<double> got((size_t)p->packed_n, 0.0), ref((size_t)p->packed_n, 0.0);
    p->check_slot = slot;
    int rc = mci_iteration_run(p, MCI_VEGAS, npb, block_lo, block_lo + nb, iteration, seed, mf, 1, 0.0);
    p->check_slot = -1;
    if (!rc) p->check_launches += 1;
    if (!rc) rc = mci_get_packed(p, got.data(), p->packed_n); // (merges the launch and waits for it)
    if (!rc) rc = vegas_check_reference(p, iteration, seed, npb, block_lo, nb, mf, nullptr, nullptr, nullptr, ref.data(), bad, /*hist_offsets=*/false);
    if (rc) return rc;
    const size_t skip = p->shape.measure_body.empty() ? 0 : (size_t)(2 * p->shape.nobs); // (a user measure: the static kernel cannot run its body)
    compare_packed(got.data(), ref.data(), (size_t)p->nstat, (size_t)p->packed_n, skip, df, (long)p->shape.nbin); // (the histogram against its own maximum)
    *differs = df->bad != 0 || bad[0] != 0 || bad[1] != 0;
    return MCI_OK;
}

static int vegas_self_check(mci_problem *p, int slot, int64_t nevalperblock, int64_t block_lo, int64_t block_hi, int32_t iteration, uint64_t seed,
                            int64_t measurefreq) {
    // The big unit (mci_host_vegas_plan.h) goes through the same rounds with its own marker.  A big unit that disagrees is never
    // selected again -- one warning, flag bit 3, the standing units and their status untouched, no conservative layout compiled: the
    // launch that triggered the check runs the standing unit.
    const bool big = slot == mci_problem::kVegasBig;
    const int u = slot == kSlotVegasAny ? 1 : 0;
    const int64_t nb = block_hi - block_lo < 2 ? block_hi - block_lo : 2, npb = nevalperblock < 512 ? nevalperblock : 512;
    const int64_t mf = measurefreq * 4 <= npb ? measurefreq : 1;
    const mci_problem::LaunchState saved = p->launch; // (everything the small launches leave on the host: put back below)
    const int kernel_timing = p->kernel_timing;
    int rc = flush_merge(p);
    if (rc) return rc;
    int h_status[4] = {0, 0, 0, 0};
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    HIPCHK(hipMemcpy(h_status, p->d_status, sizeof(h_status), hipMemcpyDeviceToHost));
    p->in_self_check = true;
    p->kernel_timing = 0;
    if (!p->shape.measure_body.empty()) p->vegas_check_flags |= 1;
    int state = 0;
    for (int round = 0; round < 2 && !rc; ++round) {
        PackedDiff df;
        int64_t bad[2] = {0, 0};
        bool differs = false;
        const std::string object = p->kernel[slot].code_object;
        rc = vegas_check_round(p, slot, npb, block_lo, nb, iteration, seed, mf, &df, bad, &differs);
        if (rc) break;
        if (!differs) {
            state = round == 0 ? 1 : -1;
            bool takes = false; // (some draw's bin takes histogram adds at all)
            for (int k = 0; k < p->shape.ndraw; ++k)
                takes = takes || (p->shape.leaf_adapt[(size_t)p->shape.draw_leaf[(size_t)k]] != 0 && p->shape.cover_mask[(size_t)k] != 0ull);
            if (takes && !(df.hist_top > 0.0)) { // nothing in the histogram the comparison could have looked at: not verified, no marker
                p->vegas_check_flags |= 4;
                if (round == 0) state = 0;
                break;
            }
            const std::string id = mcijit::compiler_id() + "\n"; // (the marker: this code object has reproduced the static kernel on a device)
            mcijit::write_file_atomic(object + ".ok", id.data(), id.size());
            break;
        }
        if (big) {
            fprintf(stderr, "mci: the big :vegas unit of this problem (%s) does not reproduce the library's static :vegas kernel on a %lld-block, "
                            "%lld-sample check: %ld of %lld packed entries differ (first at %ld; statistics %ld, histogram %ld), draws of %lld samples and "
                            "Jacobians of %lld differ.  A miscompiled code object -- big launches of this problem keep the standing :vegas unit; "
                            "mci_vegas_check_status sets flag bit 3.\n",
                    object.c_str(), (long long)nb, (long long)npb, df.bad, (long long)p->packed_n, df.first_bad, df.bad_sec[0], df.bad_sec[1], (long long)bad[0],
                    (long long)bad[1]);
            state = -1;
            break;
        }
        fprintf(stderr, "mci: the :vegas sample kernel of this problem (%s%s) does not reproduce the library's static :vegas kernel on a %lld-block, "
                        "%lld-sample check: %ld of %lld packed entries differ (first at %ld; statistics %ld, histogram %ld), draws of %lld samples and "
                        "Jacobians of %lld differ.  A miscompiled code object -- %s; mci_vegas_check_status reports %d.\n",
                object.c_str(), round ? ", the conservative layout" : "", (long long)nb, (long long)npb, df.bad, (long long)p->packed_n, df.first_bad,
                df.bad_sec[0], df.bad_sec[1], (long long)bad[0], (long long)bad[1],
                round ? "no layout of this unit agrees, its results are not to be trusted" : "the problem compiles its :vegas units again in the plain layout (plain loop, one histogram copy)",
                round ? -2 : -1);
        state = -2;
        if (round == 0) { // the most conservative layout the generator has, for both cadence variants from here on
            rc = vegas_make_conservative(p, slot);
        }
    }
    p->in_self_check = false;
    p->launch = saved;
    p->kernel_timing = kernel_timing;
    if (p->d_status) (void)hipMemcpy(p->d_status, h_status, sizeof(h_status), hipMemcpyHostToDevice); // (what the small launches flagged is theirs)
    p->merge.hist_no_offset = 0;
    if (big) { // (state 0 -- an empty histogram, a check that could not run -- leaves the unit usable and unverified, as it leaves the standing ones)
        p->vegas_big.check_done = true;
        if (state < 0) {
            p->vegas_big.state = VegasBigUnit::kFailedCheck;
            p->vegas_check_flags |= 8;
        }
        if (rc) {
            fprintf(stderr, "mci: the self-check of this problem's big :vegas unit (%s) could not run: %s -- nothing was verified\n",
                    p->kernel[slot].code_object.c_str(), mci_last_error());
            p->merge_pending = false;
        }
        return MCI_OK;
    }
    p->vegas_check_done[u] = true;
    if (rc) {
        // advisory: a check that could not run (the dump unit does not compile, no memory for its buffers) must not fail a launch that
        // works without it -- one note, nothing verified.  (A conservative unit that did not compile has left its slot empty:
        // mci_iteration_run compiles the slot again behind the gate and reports that error itself.)
        fprintf(stderr, "mci: the self-check of this problem's :vegas code object (%s) could not run: %s -- nothing was verified "
                        "(mci_vegas_check_status stays %d)\n", p->kernel[slot].code_object.c_str(), mci_last_error(), state == -2 ? -2 : 0);
        p->merge_pending = false;
        if (state == -2) p->vegas_check_state[u] = -2;
        return MCI_OK;
    }
    p->vegas_check_state[u] = state;
    return MCI_OK;
}

// before a :vegas launch through `slot`: does its code object still have to prove itself?
static int vegas_check_gate(mci_problem *p, int slot, int64_t nevalperblock, int64_t block_lo, int64_t block_hi, int32_t iteration, uint64_t seed,
                            int64_t measurefreq) {
    const int u = slot == kSlotVegasAny ? 1 : 0;
    const bool big = slot == mci_problem::kVegasBig;
    bool &done = big ? p->vegas_big.check_done : p->vegas_check_done[u];
    const bool force = g_over.vegas_self_check.on && g_over.vegas_self_check.v == 1;
    if (g_over.vegas_self_check.on && g_over.vegas_self_check.v == 0) return MCI_OK;
    if (!vegas_check_covers(p) || p->ctx->offline) { // (status 0: nobody looked)
        done = true;
        return MCI_OK;
    }
    if (!force && access((p->kernel[slot].code_object + ".ok").c_str(), F_OK) == 0) {
        done = true;
        if (big) return MCI_OK; // (the status is the standing units')
        if (p->vegas_check_state[u] == 0) {
            p->vegas_check_state[u] = 1;
            p->vegas_check_flags |= 2;
        }
        return MCI_OK;
    }
    return vegas_self_check(p, slot, nevalperblock, block_lo, block_hi, iteration, seed, measurefreq);
}

int mci_vegas_check_status(const mci_problem *p, int32_t *status, int32_t *flags) {
    if (!p || !status) return fail(MCI_ERR_INVALID, "NULL argument");
    const int a = p->vegas_check_state[0], b = p->vegas_check_state[1];
    *status = (a < 0 || b < 0) ? (a < b ? a : b) : (a > b ? a : b);
    if (flags) *flags = p->vegas_check_flags;
    return MCI_OK;
}

// csrc/mci_debug.h
int mci_debug_vegas_check(mci_problem *p, int32_t iteration, uint64_t seed, int64_t nevalperblock, int64_t block_lo, int64_t nblocks, int64_t measurefreq,
                          const double *x, const double *jac, const double *w, double *packed, int64_t *bad) {
    if (!p || !packed) return fail(MCI_ERR_INVALID, "NULL argument");
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context");
    if ((x || jac || w) && !(x && jac && w)) return fail(MCI_ERR_INVALID, "x, jac and w come together");
    int rc = flush_merge(p);
    if (rc) return rc;
    return vegas_check_reference(p, iteration, seed, nevalperblock, block_lo, nblocks, measurefreq, x, jac, w, packed, bad, /*hist_offsets=*/true);
}

int mci_debug_vegas_check_launches(const mci_problem *p, int64_t *launches) {
    if (!p || !launches) return fail(MCI_ERR_INVALID, "NULL argument");
    *launches = p->check_launches;
    return MCI_OK;
}

int mci_debug_vegas_check_layout(const mci_problem *p, int32_t *head, int32_t *draws, double *scales, uint64_t *own, int32_t *obs) {
    if (!p || !head) return fail(MCI_ERR_INVALID, "NULL argument");
    const auto &s = p->shape;
    CheckLayout L;
    vegas_check_layout(p, &L);
    head[0] = s.ndraw;
    head[1] = s.ni;
    head[2] = s.ncomp;
    head[3] = s.nobs;
    head[4] = s.ncols;
    head[5] = s.nbin;
    head[6] = vegas_check_covers(p) ? 1 : 0;
    head[7] = s.measure_body.empty() ? 1 : 0;
    for (size_t k = 0; k < L.draw.size(); ++k) {
        if (draws) {
            const mci::CheckDraw &d = L.draw[k];
            const int v[6] = {d.kind, d.off, d.doff, d.nbin, d.boff, d.hist};
            for (int j = 0; j < 6; ++j) draws[6 * k + j] = v[j];
        }
        if (scales) scales[k] = L.draw[k].scale;
    }
    for (size_t i = 0; i < L.intg.size(); ++i) {
        if (own) own[i] = L.intg[i].own;
        if (obs) {
            obs[3 * i] = L.intg[i].obs_off;
            obs[3 * i + 1] = L.intg[i].obs_nbin;
            obs[3 * i + 2] = L.intg[i].obs_bin_draw;
        }
    }
    return MCI_OK;
}
