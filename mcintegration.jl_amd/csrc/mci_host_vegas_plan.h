// mci_host_vegas_plan.h -- part of the ONE translation unit mci_api.hip (included there, first; not a stand-alone header):
// which code object a problem's :vegas launches run -- the state of that choice (VegasKernelPlan, a member of mci_problem) and the rule that makes it.  Between the marker lines there is no HIP type and no mci_problem: tests/test_vegas_kernel_rule_host.py compiles the section with g++ and walks the rule arm by arm.
// >>> vegas kernel rule
namespace {

// The choice, as it stands: made when the first :vegas unit of a problem is compiled, kept for the other cadence variant.
struct VegasKernelPlan {
    bool planned = false, keys = false; // the plan (workgroup size, histogram copies, VGPR round keys) stands for both variants
    // Plain-layout :vegas kernels of light integrands are compiled for workgroups of up to 512 threads (they need <= 128 registers anyway),
    // and mid-size launches -- one workgroup per CU, 2^19 <= samples x draws, samples < 2^22: the sizes the reference's own tests and
    // examples run -- use them: twice the lanes behind the same 256 prologues, epilogues and partial rows (tools/midsize_sweep.py,
    // profiles/r05_latency.txt: -7 .. -11 % per iteration on 2-D and 6-D integrands at 3e5 .. 3e6 samples)
    bool wide = false;
    // :vegas kernels whose tables take more than half of a CU's LDS (one workgroup per CU: 16 or 32 independent grids) pick their
    // workgroup size from the compiled code: the largest of 1024 / 768 / 512 threads (4 / 3 / 2 waves per SIMD) at which the sample
    // pass shows no scratch (128 / 168 / 256 registers).  threads_vegas = 0: the vegas kernel follows `threads`
    int threads_vegas = 0;
    bool ladder = false; // the ladder is active (no explicit size was asked for)
    // histogram copies of the :vegas sample kernel (mci_device.h hslot): what the placement rule picked (shape.hcopy is what the
    // compiled kernel uses: the rule's choice, or 1 when that kernel needs more than 128 VGPRs and two 512-thread workgroups
    // would not share a CU)
    int hcopy_auto = 1, hcopy_rule = 1; // in force | what the placement rule picked at create
    bool hcopy_plan = false;            // the rule also picked the workgroup size (512 threads) for the :vegas kernel
    bool conservative = false;          // the :vegas units are compiled in the generator's most conservative layout (plain loop, one histogram copy)

    // mci_problem_create, on the fresh plan: `copies` from the placement rule; one_per_cu: the tables take more than half of a CU's LDS
    void created(int copies, bool one_per_cu) {
        hcopy_auto = hcopy_rule = copies;
        ladder = one_per_cu;
        hcopy_plan = copies > 1 && !ladder; // two 512-thread workgroups per CU
        threads_vegas = ladder ? 1024 : hcopy_plan ? 512 : 0;
    }
    // drop_modules: the next :vegas unit plans afresh.  (threads_vegas stays: what create or the last plan left is where the next starts)
    void modules_dropped() { planned = keys = wide = false; }
    // mci_set_launch with another workgroup size: the vegas kernel follows it.  Histogram copies are sized for two 512-thread workgroups
    // per CU: smaller workgroups would leave the CU half empty
    void explicit_threads(int threads, bool override_on) {
        ladder = false;
        hcopy_plan = false;
        threads_vegas = 0;
        hcopy_auto = threads >= 512 || override_on ? hcopy_rule : 1;
    }
    // vegas_make_conservative.  The deterministic mode keeps its copy per wave.  (`ladder` and `planned` stay as they are: a many-grid
    // plan walks its ladder again from `threads`, and the caller compiles at once)
    void make_conservative(bool deterministic) {
        conservative = true;
        if (deterministic) return;
        hcopy_auto = 1;
        hcopy_plan = false;
        threads_vegas = 0;
        keys = wide = false;
    }
    // What the histogram-copy rule asks of the :vegas kernel the next time it is compiled: copies and workgroup size.  With BOTH opt-in
    // streams on (32 bits per draw, seven rounds) the loop is bound by its LDS pipe again, and sixteen copies -- conflict-free, one
    // 1024-thread workgroup per CU -- beat eight: 84.4 against 77.5 Gsamples/s on the headline configuration; with one opt-in or none
    // eight copies in two 512-thread workgroups win (bench.py: rounds 7: 73.6 against 70.2, 32 bits: 75.5 against 76.2, default: 66.7
    // against 61.7).  sixteen_fit: both streams are on and sixteen copies fit the CU's LDS
    // (Those default-stream numbers are round 2's, under the fixed partition: the fat workgroups ran in four rounds, each draining its
    // CU and zeroing and flushing 128 KB, and the unit of the day spilled at the 128-register cap, profiles/r02_ablation.txt.  Neither
    // holds any more -- the cursor runs one resident round and today's 16 x 1024 unit needs 123 VGPRs without scratch -- and on the
    // default stream sixteen copies now win for big launches: 1.3313 -> 1.3118 ms per step at 1e8 samples,
    // profiles/vegas_sixteen_copies.txt.  They run as an ADDITIONAL unit, VegasBigUnit below; this plan stays at eight.)
    int planned_copies(bool sixteen_fit, int *threads) const {
        const bool sixteen = hcopy_plan && hcopy_auto >= 8 && sixteen_fit;
        if (threads) *threads = sixteen ? 1024 : 512;
        return sixteen ? 16 : hcopy_auto;
    }
    int threads(int fallback) const { return threads_vegas ? threads_vegas : fallback; }
};

struct VegasVariant { // one :vegas code object the rule may ask for
    int copies;       // histogram copies (1: the plain layout)
    bool keys;        // Philox round keys in VGPRs (MCI_PIPE_VGPR_KEYS)
    int threads;      // the launch bound it is compiled for
};
struct VegasBuilt { long vgprs, scratch; bool ok; }; // ok: it compiled
struct VegasRuleIn {
    int threads;           // the problem's workgroup size
    bool threads_explicit; // ... named by mci_set_launch
    int ndraw;
    bool host_integrand, deterministic;
    bool copies_forced;    // the hist_copies override is on
    bool sixteen_fit;      // VegasKernelPlan::planned_copies
    int copies;            // histogram copies of the standing plan (shape.hcopy)
};
// builds a batch of variants side by side and reports each one's registers and scratch
typedef std::function<void(const std::vector<VegasVariant> &, std::vector<VegasBuilt> &)> VegasBuild;

// The thresholds.  Histogram copies pay when the kernel runs four or five waves per SIMD either way (81..128 VGPRs: two 512-thread
// workgroups share a CU).  More registers: two such workgroups no longer fit.  Fewer: the plain layout runs six or more waves per SIMD
// in 256-thread workgroups and the 80 KB of copies would cap it at four (C5 :vegas, 78 VGPRs: 1.88 ms per 1e8 samples plain,
// 2.21 ms with 8 copies; profiles/r02_ablation.txt).  And up to 128 VGPRs registers are free on the copy plan: the pipelined
// sample loop (mci_device.h draw_sample_pipe) asks for its Philox round keys in VGPRs (20 registers; the all-VGPR v_bitop3_b32
// issues faster than the form with an SGPR key: C2 1.358 -> 1.331 ms per 1e8 samples) unless that crosses the line.
const long kVgprsTwoWide = 128, kVgprsSixWaves = 80;
const int kWideThreads = 512, kWideMaxDraws = 8;
const int kLadder[3] = {1024, 768, 512};
inline bool too_fat(const VegasBuilt &b) { return b.vgprs > kVgprsTwoWide || b.scratch != 0; }

// Fills *chosen as it goes (a failed build leaves what had been decided until then, as the plan does).  != 0: a variant the rule had to
// look at did not compile -- the first such of the last batch.
inline int vegas_kernel_rule(VegasKernelPlan &pl, const VegasRuleIn &in, const VegasBuild &build_batch, VegasVariant *chosen) {
    std::vector<VegasBuilt> r;
    VegasVariant &v = *chosen;
    auto build = [&](const std::vector<VegasVariant> &vs) {
        build_batch(vs, r);
        int bad = 0;
        for (const VegasBuilt &b : r) bad |= !b.ok;
        return bad;
    };
    if (pl.planned) {
        // the other measurefreq variant of a kernel whose plan (workgroup size, histogram copies, round keys) stands
        v = {in.copies, pl.keys, pl.threads_vegas ? pl.threads_vegas : pl.wide ? kWideThreads : in.threads};
        if (build({v})) return 1;
        if (pl.keys && too_fat(r[0])) { // (this variant carries a few registers more)
            v.keys = false; // (for this compile only: pl.keys stays set, as it always did -- nothing reads it once both variants exist)
            if (build({v})) return 1;
        }
        if (!pl.threads_vegas && pl.wide && too_fat(r[0])) {
            // (the 512-thread launch bound of a light integrand's plain layout was checked on the FIRST variant only: this one does not
            // fit it -- both variants run 256-thread workgroups from here on, which the first one's code object allows)
            pl.wide = false;
            v.threads = in.threads;
            if (build({v})) return 1;
        }
        return 0;
    }
    const bool copy_plan = pl.hcopy_plan && !in.copies_forced && !pl.conservative;
    int tcopy = 512;
    const int copies = pl.planned_copies(in.sixteen_fit, &tcopy);
    if (pl.hcopy_plan) pl.threads_vegas = tcopy;
    const int T0 = pl.threads(in.threads);
    v = {copies, false, T0};
    // (light integrands: a launch bound of 512 threads costs the plain layout nothing -- see VegasKernelPlan::wide; anything that would need
    // scratch or more than 128 registers under it is compiled for the default size instead)
    const bool try_wide = !pl.conservative && in.threads == 256 && !in.threads_explicit && !in.deterministic && in.ndraw <= kWideMaxDraws && !in.host_integrand;
    auto plain_or_default = [&](VegasBuilt first, int fallback) { // `v` was built for kWideThreads if try_wide: keep that, or build it again
        pl.wide = try_wide && first.scratch == 0 && first.vgprs <= kVgprsTwoWide;
        if (!try_wide || pl.wide) return 0;
        v.threads = fallback;
        return build({v});
    };
    if (copy_plan) {
        // built side by side: [copies + VGPR keys], [plain layout]; [copies, SGPR keys] only if the first is too fat
        const VegasVariant plain = {1, false, try_wide ? kWideThreads : in.threads};
        v.keys = true;
        if (build({v, plain})) return 1;
        pl.keys = true;
        VegasBuilt copy = r[0], plain_built = r[1];
        if (too_fat(copy)) {
            v.keys = false;
            if (build({v})) return 1;
            pl.keys = false;
            copy = r[0];
        }
        if (copy.vgprs > kVgprsTwoWide || copy.vgprs <= kVgprsSixWaves) { // the plain layout
            pl.threads_vegas = 0;
            pl.keys = false;
            v = plain;
            if (plain_or_default(plain_built, in.threads)) return 1;
        }
    } else if (pl.ladder) {
        // many-grid plans (one workgroup per CU owns the LDS): the largest of 1024 / 768 / 512 threads at which the sample pass shows
        // no scratch -- the rungs compiled side by side
        std::vector<VegasVariant> rungs;
        for (int t : kLadder)
            if (t <= T0) rungs.push_back({v.copies, false, t});
        build_batch(rungs, r);
        size_t pick = rungs.size() - 1;
        for (size_t i = 0; i < rungs.size(); ++i) { // (a rung below a clean one is not looked at, compiled or not)
            if (!r[i].ok) return 1;
            if (r[i].scratch == 0) { pick = i; break; }
        }
        v = rungs[pick];
        pl.threads_vegas = v.threads;
    } else {
        if (try_wide) v.threads = kWideThreads;
        if (build({v})) return 1;
        if (plain_or_default(r[0], T0)) return 1;
    }
    pl.planned = true;
    return 0;
}

// ---- the big unit ----------------------------------------------------------------------------------------------------------------------
// A third :vegas code object next to the two cadence variants: the measurefreq == 1 source compiled for SIXTEEN histogram copies in one
// 1024-thread workgroup per CU (every lane of a 16-lane group adds to a bank-pair column of its own: conflict-free adds,
// profiles/r02_issue_costs.txt 26.8 -> 13.5 ns per wave-instruction), taken by big cursor launches only.  The standing plan above, its
// code objects and shape.hcopy are never touched by it: a launch that does not take the big unit runs exactly as it would without it.
const int kBigCopies = 16, kBigThreads = 1024;
struct VegasBigUnit {
    // 0 nothing decided (not compiled yet) | 1 loaded, within budget | kOverBudget more than 128 VGPRs or scratch with either kind of
    // round keys | kFailedCheck its self-check disagreed with the static kernel (never selected again) | kNoCompile it did not compile
    enum { kOverBudget = -1, kFailedCheck = -2, kNoCompile = -3 };
    int state = 0;
    bool keys = false;       // compiled with VGPR round keys
    bool check_done = false; // nothing left to decide for the loaded code object (mci_host_check.h)
    int resident = 0;        // workgroups the runtime reports as resident at once (asked once, when the unit is loaded)
    void modules_dropped() { *this = VegasBigUnit(); }
};
// everything the choice looks at.  The last two describe the unit itself: a caller that has not compiled it yet asks with state = 1
// and resident = nblocks -- "would this launch take it if it turned out usable?" -- and compiles only then.
struct VegasBigIn {
    bool vegas, mf1;                  // a :vegas launch | of measurefreq == 1
    bool pipe_unit;                   // plan_cursor_candidate's first condition: the pipelined one-tile loop, no self-check launch, cursor not overridden off
    bool forced_grid, deterministic;  // a forced wg_per_block | mci_set_deterministic
    int override_big;                 // override vegas_big_unit: -1 not set | 0 never | 1 at any size, with ...
    bool cursor_forced;               // ... override vegas_cursor = 1
    bool copy_plan;                   // VegasKernelPlan::hcopy_plan
    bool conservative, copies_forced, threads_explicit;
    int copies, threads;              // what the standing unit runs: shape.hcopy, its workgroup size
    bool sixteen_fit_lds;             // sixteen copies fit the CU's LDS next to the tables
    long long samples, threshold;     // of the launch, all blocks | kVegasBigSamples
    int adds, adds_floor;             // ds_add_f64 per sample | kVegasBigAdds
    long long nblocks, resident;      // blocks of the launch | VegasBigUnit::resident
    int state;                        // VegasBigUnit::state
};
enum VegasBigRefusal {
    kBigTake = 0, kBigNotMf1, kBigNoCursor, kBigForcedGrid, kBigDeterministic, kBigOverrideOff, kBigStandingPlan, kBigLds, kBigSmall, kBigFewAdds,
    kBigNotResident, kBigOverBudget, kBigFailedCheck, kBigNoCompile
};
inline VegasBigRefusal vegas_big_rule(const VegasBigIn &in) {
    const bool forced_on = in.override_big == 1 && in.cursor_forced; // (tests: any size, any grid)
    if (!in.vegas || !in.mf1) return kBigNotMf1;
    if (!in.pipe_unit) return kBigNoCursor;
    if (in.deterministic) return kBigDeterministic;
    if (in.override_big == 0) return kBigOverrideOff;
    if (in.forced_grid && !forced_on) return kBigForcedGrid;
    // the standing plan is the copy plan as the rule above leaves it for the headline kind of kernel: eight copies, 512 threads
    if (!in.copy_plan || in.conservative || in.copies_forced || in.threads_explicit || in.copies < 8 || in.threads != 512) return kBigStandingPlan;
    if (!in.sixteen_fit_lds) return kBigLds;
    if (!forced_on && in.samples < in.threshold) return kBigSmall;
    if (!forced_on && in.adds < in.adds_floor) return kBigFewAdds;
    if (in.state == VegasBigUnit::kOverBudget) return kBigOverBudget;
    if (in.state == VegasBigUnit::kFailedCheck) return kBigFailedCheck;
    if (in.state == VegasBigUnit::kNoCompile) return kBigNoCompile;
    // one resident round: every block gets a whole number (>= 1) of the workgroups that run at once
    if (!forced_on && in.resident < in.nblocks) return kBigNotResident;
    return kBigTake;
}
// the unit's registers against the budget of four waves per SIMD: VGPR round keys if they fit, else SGPR keys, else no big unit
inline int vegas_big_budget(const VegasBuilt &with_keys, const VegasBuilt *without, bool *keys) {
    *keys = !too_fat(with_keys);
    if (*keys) return 1;
    return without && !too_fat(*without) ? 1 : VegasBigUnit::kOverBudget;
}

} // namespace
// <<< vegas kernel rule
