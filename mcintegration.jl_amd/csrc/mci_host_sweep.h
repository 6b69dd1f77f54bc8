// mci_host_sweep.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// batched parameter sweeps -- eligibility, the sweep units' JIT, the one launch and the P results (mci_sweep.h vegas_sweep for
// one Continuous leaf; mci_sweep_leaves.h vegas_sweep_leaves for any mix of Continuous and Discrete leaves, by opt-in; mci_sweep_strat.h
// vegas_sweep_strat for stratified points, mci_sweep_strat_leaves.h vegas_sweep_strat_leaves for those of several Continuous leaves, by an
// opt-in of its own; mci_sweep_chains.h vegasmc_sweep for :vegasmc points and mcmc_sweep for :mcmc points, each by its
// own entry point).  One descriptor
// table (kSweepUnits), one compile, one refusal head, one driver (sweep_run).
namespace {
// Points of one sweep, and the device memory one may take.  Per point the launch holds the userdata row, a seed, two maps, niter log
// rows, nblocks partial rows and as much merge scratch, a statistics head, a histogram row and a status word: ~25 KB at the
// reference's sizes (999 increments, 16 blocks, 10 iterations), 1.6 GB at 65536 points.
const int32_t kSweepMaxPoints = 65536;
const int64_t kSweepMaxBytes = (int64_t)4 << 30;

// LDS of the sweep kernels for several leaves (mci_sweep_leaves.h, mci_sweep_chains.h), bytes: the sample loop's carve (mci_device.h Lds:
// the chain solvers' propose / accept counters are part of it under either solver) in the plain layout (tables in LDS,
// one histogram copy -- what that layout WOULD take where the problem was given another one, so that the refusal can name the count) or
// the refinement's scratch for the largest leaf, whichever is larger, and behind them (map_off, doubles) the point's map block
// edges | dacc | ddist | flags[4], each part on 16 bytes (SweepBlock)
int sweep_max_nbin(const mci_problem *p) {
    int n = 1;
    for (const Leaf &L : p->leaves) n = L.nbin > n ? L.nbin : n;
    return n;
}
int64_t sweep_leaves_lds(const mci_problem *p, int *map_off, int64_t more_carve = 0) { // more_carve: sweep_until_carve
    const auto &s = p->shape;
    const int maxn = sweep_max_nbin(p);
    const int64_t plain = (int64_t)s.ndacc + s.nddist + s.nobs + 16 * (int64_t)s.ncols + 2 * (int64_t)p->npa + s.nedge + s.nbin;
    const int64_t a = (s.table_mode == 0 && s.ntile == 1 && s.ec_doubles == 0 ? (p->lds_bytes + 7) / 8 : plain) + more_carve;
    const int64_t b = (int64_t)mci::train_lds_doubles(maxn) + maxn + 256;
    const int64_t off = ((a > b ? a : b) + 1) & ~(int64_t)1;
    if (map_off) *map_off = (int)off;
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };
    return (off + even(s.nedge) + even(s.ndacc) + even(s.nddist) + 4) * 8;
}
// doubles of one maps_in / maps_out row: the leaves in order, a grid's nbin + 1 points, a Discrete leaf's accumulation [nbin + 1] and
// distribution [nbin] (mci_sweep_leaves.h sweep_row_off)
int64_t sweep_map_doubles(const mci_problem *p) {
    int64_t n = 0;
    for (const Leaf &L : p->leaves) n += L.kind == MCI_CONTINUOUS ? L.nbin + 1 : 2 * L.nbin + 1;
    return n;
}
const int64_t kSweepLeavesMaxLds = 159 * 1024;
// what is left to check of a problem that opted in to sweeps over all its leaves and is no one-grid layout
const char *sweep_leaves_refusal(const mci_problem *p, std::string &buf) {
    const auto &s = p->shape;
    if (p->has_fermik) return "a FermiK variable (vegas doesn't work with FermiK)";
    for (const Leaf &L : p->leaves)
        if (L.kind != MCI_CONTINUOUS && L.kind != MCI_DISCRETE) return "a FermiK variable (vegas doesn't work with FermiK)";
    if (p->leaves.empty() || s.nleaf != (int)p->leaves.size() || s.nbin <= 0) return "no variable leaves";
    const int64_t lds = sweep_leaves_lds(p, nullptr);
    if (lds > kSweepLeavesMaxLds) {
        buf = "the sample tables, the refinement scratch and the point's map take " + std::to_string((long long)lds) + " bytes of LDS (" +
              std::to_string((long long)kSweepLeavesMaxLds) + " at most)";
        return buf.c_str();
    }
    if (s.table_mode != 0 || s.ntile != 1 || s.ec_doubles > 0) return "the tables and their histograms do not sit in LDS in one tile";
    return nullptr;
}
// the unit a sweep of this problem runs: the one-grid kernel wherever it applies, opted in or not
bool sweep_uses_leaves(const mci_problem *p) { return p->sweep.leaves_mode == MCI_SWEEP_ALL_LEAVES && !persist_layout(p); }

// What every query asks first, `strat`: of a stratified sweep, `chains`: the solver of a chain sweep's entry point.  Eligibility of either: measurefreq == 1, one rank, device-source integrand
// and measure, not deterministic.
const char *sweep_common_refusal(const mci_problem *p, const mci_integrate_args *a, std::string &buf, bool strat, int32_t chains = MCI_VEGAS) {
    const auto &s = p->shape;
    if (strat && !p->strat.on) return "the problem is not stratified (mci_set_stratification first; mci_integrate_sweep runs the others)";
    if (chains == MCI_MCMC) { // (mci_integrate_sweep_mcmc)
        if (a->solver != MCI_MCMC) return "solver is not :mcmc (mci_integrate_sweep runs :vegas, mci_integrate_sweep_chains :vegasmc)";
    } else if (chains == MCI_VEGASMC) { // (mci_integrate_sweep_chains: the solver test the other way round)
        if (a->solver == MCI_MCMC) return "solver is :mcmc (a sweep of :mcmc points is a follow-up)";
        if (a->solver != MCI_VEGASMC) return "solver is not :vegasmc (mci_integrate_sweep runs :vegas)";
    } else if (a->solver != MCI_VEGAS) return "solver is not :vegas (chain solvers are not swept)";
    if (a->measurefreq != 1) {
        buf = "measurefreq = " + std::to_string((long long)a->measurefreq) + " (a sweep measures every sample)";
        return buf.c_str();
    }
    if (a->niter < 1) return "niter < 1";
    if (p->ctx->nranks != 1) return "several ranks (one rank only)";
    if (!strat && p->strat.on) return "the problem is stratified (mci_set_stratification_off first)";
    if (s.host_integrand) return "a host integrand (device source or a traced closure only)";
    if (s.host_measure) return strat ? "a host measure (the default measure only)" : "a host measure (device source only)";
    if (strat && !s.measure_body.empty()) return "a user measure (the default measure only)";
    if (p->deterministic) return "deterministic mode";
    return nullptr;
}
// ONE Continuous leaf whose grid and histogram sit in LDS in one tile: the layout of the one-grid and the stratified unit
const char *sweep_one_grid_refusal(const mci_problem *p, std::string &buf, bool strat) {
    const auto &s = p->shape;
    if (s.nleaf != 1 || p->leaves.size() != 1) {
        buf = std::to_string(s.nleaf) + (strat ? " variable leaves (a stratified sweep point refines ONE Continuous grid; several Continuous leaves are a follow-up)"
                                                : " variable leaves (a sweep point refines ONE Continuous grid)");
        return buf.c_str();
    }
    if (p->leaves[0].kind != 0)
        return strat ? "a Discrete or FermiK variable (a stratified sweep point refines ONE Continuous grid)" : "a Discrete or FermiK variable (a sweep point refines ONE Continuous grid)";
    if (s.table_mode != 0 || s.ntile != 1 || s.nbin <= 0 || s.ec_doubles > 0) return "the grid and its histogram do not sit in LDS in one tile";
    return nullptr;
}

// Eligibility: persist_layout exactly (one Continuous leaf, table mode 0, one tile, device-source integrand and measure, not
// deterministic, within 64 KiB including the map copy), measurefreq == 1, one rank.  NOT the draw count: `ndraw <= 7` is
// persist_plan's rule for when the persistent launch beats the launch chain, nothing a sweep depends on.
const char *sweep_refusal(const mci_problem *p, const mci_integrate_args *a, std::string &buf) {
    if (const char *r = sweep_common_refusal(p, a, buf, false)) return r;
    if (sweep_uses_leaves(p)) return sweep_leaves_refusal(p, buf); // (opted in: mci_set_sweep_leaves)
    if (const char *r = sweep_one_grid_refusal(p, buf, false)) return r;
    if (persist_lds(p, nullptr) > 64 * 1024) {
        buf = "the sample tables, the refinement scratch and the map copy take " + std::to_string((long long)persist_lds(p, nullptr)) + " bytes of LDS (64 KiB at most)";
        return buf.c_str();
    }
    return nullptr;
}

// one device allocation per sweep: the context's spare buffer if it fits (tile_alloc's rule), else hipMalloc; handed back on return
int sweep_alloc(mci_ctx *c, size_t bytes, void **base, size_t *got) {
    *base = nullptr;
    {
        std::lock_guard<std::mutex> g(c->spare_mu);
        if (c->spare && c->spare_bytes >= bytes && c->spare_bytes <= 2 * bytes + ((size_t)64 << 20)) {
            *base = c->spare;
            *got = c->spare_bytes;
            c->spare = nullptr;
            c->spare_bytes = 0;
        }
    }
    if (!*base) {
        HIPCHK(hipMalloc(base, bytes));
        *got = bytes;
    }
    return MCI_OK;
}
// (a sweep's buffer grows with P, up to kSweepMaxBytes: only one of up to kSweepKeepBytes is parked with the context -- what a scan of
// a few thousand points at the reference's sizes takes, so that repeated sweeps do not allocate --, a larger one is freed at once)
const size_t kSweepKeepBytes = (size_t)256 << 20;
void sweep_release(mci_ctx *c, void *base, size_t bytes) {
    if (!base) return;
    void *drop = base;
    {
        std::lock_guard<std::mutex> g(c->spare_mu);
        if (bytes <= kSweepKeepBytes && bytes > c->spare_bytes) {
            drop = c->spare;
            c->spare = base;
            c->spare_bytes = bytes;
        }
    }
    if (drop) (void)hipFree(drop);
}
// Workgroup size of the sweep kernel.  Measured on the 4-D Genz product peak at niter = 10, block = 16 (tools/sweep_bench.py,
// profiles/r10_sweep.txt); csrc/mci_debug.h mci_debug_sweep_threads forces another one.
const int kSweepThreads = 256;
// The `until` units (mci_integrate_sweep_until) are compiled in the deterministic histogram layout (mci_device.h hslot, Cfg::DET): every
// wave of the workgroup adds to a histogram and an observable copy of its own, and the copies are summed in a fixed order -- a point's
// histogram, hence its map and every later iteration, does not depend on how the waves were scheduled, so its results are the same bytes
// whichever workgroup runs it and whatever ran before.  What that takes of LDS beyond the plain carve, doubles (det_lds's count):
int64_t sweep_until_carve(const mci_problem *p) { return ((int64_t)p->shape.htile + p->shape.nobs) * (kSweepThreads / 64 - 1); }
int64_t sweep_until_lds(const mci_problem *p, int *map_off) {
    return sweep_uses_leaves(p) ? sweep_leaves_lds(p, map_off, sweep_until_carve(p)) : persist_lds(p, map_off, sweep_until_carve(p));
}
// ... and what it refuses beyond sweep_refusal: the one-grid unit keeps within the 64 KiB every workgroup may ask for, the unit for several
// leaves within kSweepLeavesMaxLds
const char *sweep_until_lds_refusal(const mci_problem *p, std::string &buf) {
    const int64_t lds = sweep_until_lds(p, nullptr), most = sweep_uses_leaves(p) ? kSweepLeavesMaxLds : 64 * 1024;
    if (lds <= most) return nullptr;
    buf = "the sample tables with one histogram copy per wave (a point's results must not depend on the waves' schedule), the refinement scratch and the point's map take " +
          std::to_string((long long)lds) + " bytes of LDS (" + std::to_string((long long)most) + " at most)";
    return buf.c_str();
}
} // namespace

static bool sweep_leaves_unit(const mci_problem *p) { return sweep_uses_leaves(p); }

// A sweep unit's code object (kSweepUnits, mci_host_types.h): one histogram copy, kSweepThreads threads -- the one-grid unit is loaded
// again when mci_debug_sweep_threads asks for another workgroup size --, no static LDS, no scratch
static int compile_sweep_unit(mci_problem *p, int which) {
    const SweepUnitDesc &k = kSweepUnits[which];
    KernelUnit &u = p->sweep_unit(which);
    const int T = k.want_threads && p->sweep.want_threads > 0 ? p->sweep.want_threads : kSweepThreads;
    if (u.compiled && u.threads == T) return MCI_OK;
    u.drop();
    Candidate c;
    mcijit::ProblemShape sh = p->shape;
    const bool until = which == mci_problem::Sweep::kUntil || which == mci_problem::Sweep::kLeavesUntil;
    sh.hcopy = until ? T / 64 : 1; // (the `until` units: one histogram and observable copy per wave, sweep_until_carve)
    sh.det = until ? 1 : 0;
    c.unit = k.jit_unit;
    c.src = mcijit::generate_source(sh, k.runs, k.jit_unit, k.alpha ? p->leaves[0].alpha : 0.0);
    c.threads = T;
    const std::string tag = k.tag;
    if (c.build()) return c.failed(" (sweep kernel" + (tag.empty() ? tag : ", " + tag) + ")");
    const KernelUnit::Rules rules = {KernelUnit::kUnlinkAndFail, true,
                                     std::string("the sweep kernel") + k.for_what + " came out with static LDS or scratch at " + std::to_string(T) + " threads per workgroup",
                                     "the sweep code object" + (tag.empty() ? tag : " (" + tag + ")")};
    // (the several-leaves and the chain solvers' units' LDS is the layout's; the two stratified units' is the call's: sweep_run)
    const bool whole_map = which == mci_problem::Sweep::kLeaves || which == mci_problem::Sweep::kLeavesUntil || (which >= mci_problem::Sweep::kChains && which < mci_problem::Sweep::kStratLeaves) ||
                           which == mci_problem::Sweep::kChainsResume || which == mci_problem::Sweep::kMcmcResume;
    return u.load(p->ctx, c, mcijit::kUnits[k.jit_unit].kernel, which == mci_problem::Sweep::kLeavesUntil ? sweep_until_lds(p, nullptr) : whole_map ? sweep_leaves_lds(p, nullptr) : 0, rules);
}

int mci_set_sweep_leaves(mci_problem *p, int32_t mode) {
    if (!p || (mode != MCI_SWEEP_ONE_GRID && mode != MCI_SWEEP_ALL_LEAVES)) return fail(MCI_ERR_INVALID, "sweep leaves: MCI_SWEEP_ONE_GRID (0) or MCI_SWEEP_ALL_LEAVES (1)");
    p->sweep.leaves_mode = mode;
    return MCI_OK;
}

int mci_set_sweep_strat_leaves(mci_problem *p, int32_t mode) {
    if (!p || (mode != MCI_SWEEP_ONE_GRID && mode != MCI_SWEEP_ALL_LEAVES)) return fail(MCI_ERR_INVALID, "sweep strat leaves: MCI_SWEEP_ONE_GRID (0) or MCI_SWEEP_ALL_LEAVES (1)");
    p->sweep.strat_leaves_mode = mode;
    return MCI_OK;
}

int mci_set_sweep_chain_carry(mci_problem *p, int32_t on) {
    if (!p || (on != 0 && on != 1)) return fail(MCI_ERR_INVALID, "sweep chain carry: 0 (every iteration of a point starts its chains afresh) or 1 (it continues the chains of the one before)");
    p->sweep.chain_carry = on;
    return MCI_OK;
}
int mci_get_sweep_chain_carry(const mci_problem *p, int32_t *on) {
    if (!p || !on) return fail(MCI_ERR_INVALID, "NULL argument");
    *on = p->sweep.chain_carry;
    return MCI_OK;
}

int mci_sweep_map_doubles(const mci_problem *p, int32_t *n) {
    if (!p || !n) return fail(MCI_ERR_INVALID, "NULL argument");
    *n = (int32_t)sweep_map_doubles(p);
    return MCI_OK;
}

int mci_sweep_supported(const mci_problem *p, const mci_integrate_args *a, char *why, int32_t n) {
    if (why && n > 0) why[0] = 0;
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    std::string buf;
    const char *r = sweep_refusal(p, a, buf);
    if (!r) return MCI_OK;
    if (why && n > 0) snprintf(why, (size_t)n, "%s", r);
    return fail(MCI_ERR_INVALID, "this problem cannot run as a sweep: %s", r);
}

// csrc/mci_debug.h
int mci_debug_sweep_workgroups(mci_problem *p, int32_t g) {
    if (!p || g < 0) return fail(MCI_ERR_INVALID, "sweep workgroups: >= 1, or 0 for the default");
    p->sweep.grid = g;
    return MCI_OK;
}
int mci_debug_sweep_threads(mci_problem *p, int32_t threads) {
    if (!p || (threads != 0 && threads != 256 && threads != 512 && threads != 1024)) return fail(MCI_ERR_INVALID, "sweep threads: 256, 512, 1024, or 0 for the default");
    p->sweep.want_threads = threads;
    return MCI_OK;
}
int mci_debug_sweep_last_launch(const mci_problem *p, int32_t *workgroups, int32_t *threads) {
    if (!p) return fail(MCI_ERR_INVALID, "NULL argument");
    if (workgroups) *workgroups = p->sweep.last_grid;
    if (threads) *threads = p->sweep.last_threads;
    return MCI_OK;
}

int mci_debug_sweep_lds_bytes(const mci_problem *p, int64_t *bytes) {
    if (!p || !bytes) return fail(MCI_ERR_INVALID, "NULL argument");
    *bytes = sweep_uses_leaves(p) ? sweep_leaves_lds(p, nullptr) : persist_lds(p, nullptr);
    return MCI_OK;
}

namespace {
// stored chains per block whose running weights a carried sweep point's resample_block keeps in LDS (SweepChainCarry::lds_w): the
// front of the segment up to the point's map block, less the threads' partial sums
int sweep_resample_lds(int map_off) { return map_off - (int)mci::kResampleThreads; }
} // namespace
int mci_debug_sweep_resample_lds(const mci_problem *p, int64_t *lds_w) {
    if (!p || !lds_w) return fail(MCI_ERR_INVALID, "NULL argument");
    int map_off = 0;
    sweep_leaves_lds(p, &map_off); // (what sweep_chains_call lays its launch out by)
    *lds_w = sweep_resample_lds(map_off);
    return MCI_OK;
}

// ---------------------------------------------------------------------------------------------------
// the one driver of a sweep launch
// ---------------------------------------------------------------------------------------------------
namespace {
// The sweep's one device buffer: doubles, segment by segment, every segment [npoint][doubles per point]; behind them the status words.
// kSegOff, kSegTbase and kSegD are the stratified unit's, kSegRw and kSegPa the chain solvers' units', kSegHolds the :mcmc unit's,
// kSegCarry (the stored chains, the picks, the weights) and kSegBlk (the block means) the carried chain units' (none otherwise), kSegState
// (the state rows a call came in with: read only) the units' that continue the chains of the call before, kSegSums
// (every column's running W | sum w m) the `until` units'.  Everything from kSegGhist on is zeroed before the launch: histogram rows, d rows, holding-time histograms (64 words of 8
// bytes per point), running sums, (the seeds: copied next), status words, and behind them in an `until` sweep the points' iteration
// counts [npoint] and the cursor word.
enum { kSegUd, kSegMapsIn, kSegMapsOut, kSegLog, kSegPart, kSegScratch, kSegPacked, kSegOff, kSegTbase, kSegRw, kSegPa, kSegCarry, kSegBlk, kSegState, kSegGhist, kSegD, kSegHolds, kSegSums, kSegSeeds, kSegStatus, kSegCount = kSegStatus };

// What an entry point hands to sweep_run: the call's arguments as they came, and what its unit makes of them
struct SweepCall {
    int unit = 0; // mci_problem::Sweep::kOne | kLeaves | kStrat | kChains | kMcmc
    // the caller's arguments
    int32_t npoint = 0;
    const double *userdata = nullptr;
    const uint64_t *seeds = nullptr;
    const double *maps_in = nullptr;
    double *maps_out = nullptr;
    mci_result *results = nullptr;
    double *iter_mean = nullptr, *iter_std = nullptr;
    int32_t *status = nullptr;
    // mci_integrate_sweep_until: the target (NULL: every point runs niter iterations) and where the points' iteration counts go (or NULL)
    const mci_sweep_target *until = nullptr;
    int32_t *niter_run = nullptr;
    // plan(): the unit's sizes for this call, made behind the results[] check; it may refuse
    std::function<int(SweepCall &)> plan;
    int64_t rows = 0;            // partial rows per point: the statistical blocks, or 1 (stratified)
    int64_t neval_per_block = 0, blocks = 0; // main.jl:121
    size_t map_doubles = 0;      // one maps_in / maps_out row
    size_t off_doubles = 0, tbase_doubles = 0, d_doubles = 0; // per point: kSegOff, kSegTbase, kSegD
    size_t rw_doubles = 0, pa_doubles = 0;                    // per point: kSegRw (reweight factors), kSegPa (the blocks' propose | accept rows)
    size_t packed_doubles = 0;   // a point's packed row; 0: the statistics head alone
    size_t holds_doubles = 0;    // per point: kSegHolds (64 or none)
    size_t carry_doubles = 0, blk_doubles = 0; // per point: kSegCarry, kSegBlk (carried chains)
    size_t state_doubles = 0;    // per point: kSegState (the state row iteration 0 continues)
    bool first_continued = false; // iteration 0 continued the chains of the call before: every result is correlated
    const double *block_means = nullptr; // carried chains, set by finish(): [npoint][niter][blocks][nobs] on the host -- the points' errors come from their blocks' lineages
    int maxn = 0;                // bins of the largest leaf
    int64_t lds = 0;             // bytes of LDS of a workgroup
    int map_off = 0;             // SweepHead::map_off
    bool strat_stats = false;    // an iteration's mean | error: strat_mean_std over its log row, else mci_mean_std over the blocks
    const char *too_big = nullptr; // printf format of "this sweep does not fit": npoint, niter, too_big_count, bytes, limit
    long long too_big_count = 0;
    // the kernel's second argument behind its head: `h` is filled, `o` are the segments' offsets in `d`; NULL: the head is the argument
    std::function<void *(const mci::SweepHead &h, double *d, const size_t *o)> args;
    std::function<void(mci::BatchArgs &b)> batch; // what the unit's sample loop reads of the launch's BatchArgs beyond the :vegas ones
    // the unit's own copies in front of the launch / behind it (stream st), and what it makes of them once the stream has drained
    std::function<int(double *d, const size_t *o, hipStream_t st)> copy_in, copy_out;
    std::function<void()> finish;
};

// results[] check, buffer, uploads, arguments, launch, read-back, and per point what mci_integrate makes of its log rows
int sweep_run(mci_problem *p, const mci_integrate_args *a, SweepCall &c) {
    const auto &s = p->shape;
    const int npoint = c.npoint, nud = (int)p->h_ud.size(), nstat = p->nstat, niter = a->niter;
    mci_result *results = c.results;
    for (int q = 0; q < npoint; ++q)
        if (results[q].niter < a->niter || results[q].nobs != s.nobs || !results[q].mean || !results[q].stdev || !results[q].chi2)
            return fail(MCI_ERR_INVALID, "result buffers of point %d too small", q);
    int rc;
    if ((rc = c.plan(c))) return rc;
    const size_t P = (size_t)npoint, rows = (size_t)c.rows * s.ncols;
    const size_t per_point[kSegCount] = {(size_t)nud, c.maps_in ? c.map_doubles : 0, c.map_doubles, (size_t)niter * nstat, rows, rows, c.packed_doubles ? c.packed_doubles : (size_t)nstat,
                                         c.off_doubles,  c.tbase_doubles, c.rw_doubles, c.pa_doubles, c.carry_doubles, c.blk_doubles, c.state_doubles, (size_t)s.nbin, c.d_doubles, c.holds_doubles, c.until ? 2 * (size_t)s.nobs : 0,
                                         c.seeds ? (size_t)1 : 0};
    size_t o[kSegCount + 1] = {0};
    for (int k = 0; k < kSegCount; ++k) o[k + 1] = o[k] + P * per_point[k];
    const size_t ndbl = o[kSegStatus] + (c.until ? P + 1 : (P + 1) / 2); // status [P] ints; until: | iters [P] | cursor
    if ((int64_t)(ndbl * sizeof(double)) > kSweepMaxBytes)
        return fail(MCI_ERR_INVALID, c.too_big, (int)npoint, niter, c.too_big_count, (long long)(ndbl * sizeof(double)), (long long)kSweepMaxBytes);
    if ((rc = compile_sweep_unit(p, c.unit))) return rc;
    const KernelUnit &u = p->sweep_unit(c.unit);
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    void *base = nullptr;
    size_t got = 0;
    if ((rc = sweep_alloc(p->ctx, ndbl * sizeof(double), &base, &got))) return rc;
    double *d = (double *)base;
    std::vector<double> hlog(P * (size_t)niter * nstat);
    std::vector<int> hst(P), hit(c.until ? P : 0);
    mci::SweepUntilArgs fu{};
    auto run = [&]() -> int {
        auto t0 = std::chrono::steady_clock::now();
        if (nud > 0) HIPCHK(hipMemcpyAsync(d + o[kSegUd], c.userdata, P * nud * sizeof(double), hipMemcpyHostToDevice, st));
        if (c.maps_in) HIPCHK(hipMemcpyAsync(d + o[kSegMapsIn], c.maps_in, P * c.map_doubles * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d + o[kSegGhist], 0, (ndbl - o[kSegGhist]) * sizeof(double), st));
        if (c.copy_in && (rc = c.copy_in(d, o, st))) return rc;
        if (c.seeds) HIPCHK(hipMemcpyAsync(d + o[kSegSeeds], c.seeds, P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        mci::BatchArgs b{};
        fill_batch(p, b); // (the map and the reweight factors are the problem's; everything else lives in the sweep's own allocation)
        b.ud = d + o[kSegUd];
        b.part_cols = d + o[kSegPart];
        b.part_hist = nullptr;
        b.ghist = d + o[kSegGhist];
        b.seed = a->seed;
        b.iteration = (mci::u32)a->first_iteration;
        b.neval_per_block = c.neval_per_block;
        b.block_lo = 0;
        b.wg_per_block = 1;
        b.measurefreq = 1;
        b.nchain = 1;
        b.hist_atomic = 1;
        b.status = reinterpret_cast<int *>(d + o[kSegStatus]);
        b.tile_stride = c.blocks * c.neval_per_block;
        b.nrows = c.rows;
        if (c.batch) c.batch(b);
        mci::SweepHead h{};
        mci::MergeArgs &m = h.m;
        m = merge_args(p, c.rows, 1, c.rows);
        m.part_cols = d + o[kSegPart];
        m.stage1 = nullptr;
        m.ngroup = 0;
        m.ghist = d + o[kSegGhist];
        m.use_ghist = 1;
        m.packed = d + o[kSegPacked];
        m.status = b.status;
        m.scratch = d + o[kSegScratch];
        m.npa = 0;
        m.block_means = nullptr;
        mci::TrainArgs &t = h.t;
        fill_train(p, t);
        t.packed = d + o[kSegPacked];
        t.nstat = nstat;
        t.iter_log_row = d + o[kSegLog];
        t.reweight = nullptr;
        t.do_reweight = 0; // (:vegas: main.jl:183 runs doReweight! for the chain solvers only)
        t.gamma = a->gamma;
        t.do_train = a->adapt ? 1 : 0;
        t.serial_walk = 0;
        t.status = b.status;
        t.maxn = c.maxn;
        h.npoint = npoint;
        h.niter = niter;
        h.nuserdata = nud;
        h.map_off = c.map_off;
        h.ud = d + o[kSegUd];
        h.seeds = c.seeds ? reinterpret_cast<const mci::u64 *>(d + o[kSegSeeds]) : nullptr;
        h.maps_in = c.maps_in ? d + o[kSegMapsIn] : nullptr;
        h.maps_out = d + o[kSegMapsOut];
        void *karg = c.args ? c.args(h, d, o) : (void *)&h;
        if (c.until) { // (the `until` units: the head and the target behind it; the words behind the status words)
            const int ignore = a->ignore >= 0 ? a->ignore : (a->adapt ? 1 : 0);
            fu.h = h;
            fu.u = mci::SweepUntil{c.until->rtol, c.until->atol, c.until->min_niter, ignore, d + o[kSegSums], b.status + P, b.status + 2 * P};
            karg = &fu;
        }
        // workgroups: two per CU keep a CU's SIMDs busy while one of them sits in its refinement; any grid runs any npoint
        int cus = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->ctx->device));
        // (several leaves, stratified points: LDS that leaves no room for two workgroups in a CU's 160 KiB gets one)
        const int per_cu = c.unit != mci_problem::Sweep::kOne && c.unit != mci_problem::Sweep::kUntil && c.lds > 80 * 1024 ? 1 : 2;
        int64_t grid = p->sweep.grid > 0 ? p->sweep.grid : per_cu * (int64_t)(cus > 0 ? cus : 256);
        if (grid > npoint) grid = npoint;
        if ((c.unit == mci_problem::Sweep::kStrat || c.unit == mci_problem::Sweep::kStratLeaves) && c.lds > 64 * 1024) // (the chunk is the call's: not known when the unit is compiled)
            HIPCHK(hipFuncSetAttribute((const void *)u.f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
        void *args[] = {&b, karg};
        HIPCHK(hipModuleLaunchKernel(u.f, (unsigned)grid, 1, 1, (unsigned)u.threads, 1, 1, (unsigned)c.lds, st, args, nullptr));
        p->sweep.last_grid = (int)grid;
        p->sweep.last_threads = u.threads;
        HIPCHK(hipMemcpyAsync(hlog.data(), d + o[kSegLog], hlog.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hst.data(), d + o[kSegStatus], P * sizeof(int), hipMemcpyDeviceToHost, st));
        if (c.until) HIPCHK(hipMemcpyAsync(hit.data(), b.status + P, P * sizeof(int), hipMemcpyDeviceToHost, st));
        if (c.maps_out) HIPCHK(hipMemcpyAsync(c.maps_out, d + o[kSegMapsOut], P * c.map_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
        if (c.copy_out && (rc = c.copy_out(d, o, st))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int q = 0; q < npoint; ++q) results[q].seconds = seconds;
        return MCI_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st); // (nothing of a failed call is still reading the buffer when it goes back)
    sweep_release(p->ctx, base, got);
    if (rc) return rc;
    if (c.finish) c.finish();
    for (int q = 0; q < npoint && c.until; ++q) // (every point was run by some workgroup, for 1 to niter iterations)
        if (hit[q] < 1 || hit[q] > niter) return fail(MCI_ERR_HIP, "sweep: point %d came back with %d iterations run (1 to %d)", q, hit[q], niter);
    // per point what mci_integrate makes of its log rows (main.jl:203, :211; stratified: strat_mean_std)
    const int ignore = a->ignore >= 0 ? a->ignore : (a->adapt ? 1 : 0);
    std::vector<double> tm((size_t)niter * s.nobs), te((size_t)niter * s.nobs);
    for (int q = 0; q < npoint; ++q) {
        mci_result *res = &results[q];
        double *im = c.iter_mean ? c.iter_mean + (size_t)q * niter * s.nobs : res->iter_mean ? res->iter_mean : tm.data();
        double *ie = c.iter_std ? c.iter_std + (size_t)q * niter * s.nobs : res->iter_std ? res->iter_std : te.data();
        res->neval = 0;
        // (until: the point's own n_p rows -- the rows behind them were never written, and the log segment is not zeroed)
        const int np = c.until ? hit[q] : niter;
        for (int it = 0; it < np; ++it) {
            const double *row = hlog.data() + ((size_t)q * niter + it) * nstat;
            if (c.strat_stats) strat_mean_std(row, s.nobs, im + (size_t)it * s.nobs, ie + (size_t)it * s.nobs);
            else mci_mean_std(row, row + s.nobs, s.nobs, c.blocks, im + (size_t)it * s.nobs, ie + (size_t)it * s.nobs);
            res->neval += (int64_t)row[2 * s.nobs + 1];
            if (res->visited && it == np - 1) memcpy(res->visited, row + 2 * s.nobs + 2, (size_t)(s.ni + 1) * sizeof(double));
        }
        for (size_t k = (size_t)np * s.nobs; k < (size_t)niter * s.nobs; ++k) im[k] = ie[k] = 0.0;
        if (c.niter_run) c.niter_run[q] = np;
        if (c.iter_mean && res->iter_mean && res->iter_mean != im) memcpy(res->iter_mean, im, (size_t)niter * s.nobs * sizeof(double));
        if (c.iter_std && res->iter_std && res->iter_std != ie) memcpy(res->iter_std, ie, (size_t)niter * s.nobs * sizeof(double));
        for (int o2 = 0; o2 < s.nobs; ++o2) // main.jl:211 -> statistics.jl:24-55
            mci_average(im + o2, ie + o2, s.nobs, ignore + 1, np, &res->mean[o2], &res->stdev[o2], &res->chi2[o2]);
        res->correlated = 0;
        res->warmup = 0;
        // carried chains: the error from the scatter of the blocks' weighted averages over the run, as in mci_integrate (mci_host_integrate.h)
        if (c.block_means && niter > ignore + 1) {
            std::vector<double> sums(2 * (size_t)s.nobs), lm(s.nobs), le(s.nobs);
            mci_lineage_sums(c.block_means + (size_t)q * niter * c.blocks * s.nobs, niter, c.blocks, s.nobs, ie, ignore + 1, niter, sums.data(), sums.data() + s.nobs);
            mci_mean_std(sums.data(), sums.data() + s.nobs, s.nobs, c.blocks, lm.data(), le.data());
            for (int o2 = 0; o2 < s.nobs; ++o2) res->stdev[o2] = le[o2] > 0.0 ? le[o2] : res->stdev[o2];
            res->correlated = 1;
        }
        if (c.first_continued) res->correlated = 1; // (even where the call is too short for a lineage error)
        if (c.status) c.status[q] = hst[q];
    }
    return MCI_OK;
}

// what every entry point checks of its arguments before anything else; `supported`: its own query
int sweep_check_args(const mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const mci_result *results,
                     int (*supported)(const mci_problem *, const mci_integrate_args *, char *, int32_t)) {
    if (!p || !a || !results) return fail(MCI_ERR_INVALID, "NULL argument");
    if (npoint < 1 || npoint > kSweepMaxPoints) return fail(MCI_ERR_INVALID, "npoint = %d: a sweep takes 1 to %d points", (int)npoint, (int)kSweepMaxPoints);
    if (int rc = supported(p, a, nullptr, 0)) return rc;
    if (p->ctx->offline) return fail(MCI_ERR_NO_DEVICE, "offline context: no device to run on");
    const int nud = (int)p->h_ud.size();
    if (nud > 0 && !userdata) return fail(MCI_ERR_INVALID, "userdata is NULL (the integrand reads %d values per point)", nud);
    return MCI_OK;
}
} // namespace

// P independent integrate() loops (main.jl:142-207), one workgroup each, in one launch; t: NULL (every point runs niter iterations) or the
// target of mci_integrate_sweep_until (the `until` units)
static int sweep_vegas_call(mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, int32_t npoint, const double *userdata, const uint64_t *seeds,
                            const double *maps_in, double *maps_out, mci_result *results, double *iter_mean, double *iter_std, int32_t *status, int32_t *niter_run) {
    if (!(a->neval > a->block)) return fail(MCI_ERR_INVALID, "neval=%lld should be larger than nblock = %lld", (long long)a->neval, (long long)a->block); // main.jl:222
    SweepCall c;
    const bool leaves = sweep_uses_leaves(p); // (else one Continuous leaf: a row is its grid)
    c.unit = leaves ? (t ? mci_problem::Sweep::kLeavesUntil : mci_problem::Sweep::kLeaves) : (t ? mci_problem::Sweep::kUntil : mci_problem::Sweep::kOne);
    c.until = t, c.niter_run = niter_run;
    c.npoint = npoint, c.userdata = userdata, c.seeds = seeds, c.maps_in = maps_in, c.maps_out = maps_out;
    c.results = results, c.iter_mean = iter_mean, c.iter_std = iter_std, c.status = status;
    c.plan = [a](SweepCall &c) {
        mci_standardize_block(a->neval, a->block, 1, &c.neval_per_block, &c.blocks); // main.jl:121
        if (c.blocks > (int64_t)1 << 20) return fail(MCI_ERR_INVALID, "block = %lld: too many blocks for a sweep", (long long)c.blocks);
        c.rows = c.blocks;
        c.too_big_count = (long long)c.blocks;
        return (int)MCI_OK;
    };
    c.map_doubles = (size_t)sweep_map_doubles(p);
    c.maxn = sweep_max_nbin(p);
    // (the `until` units' two LDS words are the last of the four flag slots both layouts count behind the map: nothing else uses it)
    c.lds = t ? sweep_until_lds(p, &c.map_off) : leaves ? sweep_leaves_lds(p, &c.map_off) : persist_lds(p, &c.map_off);
    c.too_big = "a sweep of %d points x %d iterations x %lld blocks needs %lld bytes of device memory (limit %lld): split it";
    return sweep_run(p, a, c);
}
int mci_integrate_sweep(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                        double *maps_out, mci_result *results, double *iter_mean, double *iter_std, int32_t *status) {
    if (int rc = sweep_check_args(p, a, npoint, userdata, results, mci_sweep_supported)) return rc;
    return sweep_vegas_call(p, a, nullptr, npoint, userdata, seeds, maps_in, maps_out, results, iter_mean, iter_std, status, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// a target error per point: the same two kernels' `until` instantiations (mci_sweep.h vegas_sweep<Cfg, true>, mci_sweep_leaves.h
// vegas_sweep_leaves<Cfg, true>), the stop rule of mci_sweep_common.h
// ---------------------------------------------------------------------------------------------------
int mci_sweep_until_supported(const mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, char *why, int32_t n) {
    if (int rc = mci_sweep_supported(p, a, why, n)) return rc; // (whatever the fixed sweep refuses, with that reason)
    std::string buf;
    const char *r = !t ? "the target is NULL"
                    : !(std::isfinite(t->rtol) && t->rtol >= 0.0) ? "rtol is negative or not finite"
                    : !(std::isfinite(t->atol) && t->atol >= 0.0) ? "atol is negative or not finite"
                    : t->min_niter < 0 ? "min_niter < 0" : sweep_until_lds_refusal(p, buf);
    if (!r) return MCI_OK;
    if (why && n > 0) snprintf(why, (size_t)n, "%s", r);
    return fail(MCI_ERR_INVALID, "this sweep cannot run to a target error: %s", r);
}

static_assert(offsetof(mci::SweepUntilArgs, h) == 0, "the `until` units read the head where the fixed units do");
int mci_integrate_sweep_until(mci_problem *p, const mci_integrate_args *a, const mci_sweep_target *t, int32_t npoint, const double *userdata, const uint64_t *seeds,
                              const double *maps_in, double *maps_out, mci_result *results, double *iter_mean, double *iter_std, int32_t *status, int32_t *niter_run) {
    if (int rc = mci_sweep_until_supported(p, a, t, nullptr, 0)) return rc; // (first: a refusal is the same with and without a device)
    if (int rc = sweep_check_args(p, a, npoint, userdata, results, mci_sweep_supported)) return rc;
    return sweep_vegas_call(p, a, t, npoint, userdata, seeds, maps_in, maps_out, results, iter_mean, iter_std, status, niter_run);
}

// ---------------------------------------------------------------------------------------------------
// stratified (VEGAS+) points in a sweep: mci_sweep_strat.h vegas_sweep_strat, one workgroup runs a point's whole stratified loop
// ---------------------------------------------------------------------------------------------------
namespace {
// the plan of a stratified sweep of N samples per iteration: the problem's own request, or the default plan for N (strat_prepare's rule)
int sweep_strat_plan(const mci_problem *p, int64_t N, std::vector<int> &ns, int64_t *ncube) {
    const auto &st = p->strat;
    const int D = p->shape.ndraw;
    ns.assign((size_t)D, 1);
    if (st.want.empty()) {
        int rc = mci_strat_plan(N, D, st.max_nhcube, ns.data());
        if (rc) return rc;
    } else ns = st.want;
    int64_t nc = 1;
    for (int v : ns) {
        if (nc > (((int64_t)1 << 31) - 1) / v) return fail(MCI_ERR_INVALID, "stratification: more than 2^31 - 1 hypercubes");
        nc *= v;
    }
    *ncube = nc;
    return MCI_OK;
}
// LDS of the stratified sweep kernel, bytes, for chunks of nloc hypercubes: the sample carve + the chunk's hypercubes or the refinement's
// scratch, whichever is larger, and behind them (map_off, doubles) the map [N + 2] | flags [4] | running sums and the cut hypercube's
// sums [4 kStratMaxCols] (mci_sweep_strat.h SweepStratArgs::map_off)
int64_t sweep_strat_lds(const mci_problem *p, int nloc, int *map_off) {
    const int N = p->leaves.empty() ? 1 : p->leaves[0].nbin, NW = p->shape.ni * p->shape.ncomp;
    const int64_t a = (p->lds_bytes + 7) / 8 + strat_chunk_lds_bytes(nloc, NW) / 8, b = (int64_t)mci::train_lds_doubles(N) + N + 256;
    const int64_t off = ((a > b ? a : b) + 1) & ~(int64_t)1;
    if (map_off) *map_off = (int)off;
    return (off + (N + 2) + 4 + 4 * (int64_t)mci::kStratMaxCols) * 8;
}
// The unit a stratified sweep of this problem runs: the one-grid kernel wherever it applies, opted in (mci_set_sweep_strat_leaves) or not
bool sweep_strat_uses_leaves(const mci_problem *p) {
    std::string buf;
    return p->sweep.strat_leaves_mode == MCI_SWEEP_ALL_LEAVES && sweep_one_grid_refusal(p, buf, true) != nullptr;
}
// LDS of the stratified sweep kernel for several leaves (mci_sweep_strat_leaves.h), bytes, for chunks of nloc hypercubes: the sample carve
// (in the plain layout -- what it WOULD take where the problem was given another one, so that the refusal can name the count, as in
// sweep_leaves_lds) + the chunk's hypercubes or the refinement's scratch for the largest leaf, whichever is larger, and behind them
// (map_off, doubles) the map block edges | dacc | ddist | flags [4] (SweepBlock) | running sums and the cut hypercube's sums
// [4 kStratMaxCols] | sweep_strat_alloc's broadcast pair [2].  The only place this byte count is made.
int64_t sweep_strat_leaves_lds(const mci_problem *p, int nloc, int *map_off) {
    const auto &s = p->shape;
    const int maxn = sweep_max_nbin(p), NW = s.ni * s.ncomp;
    const int64_t plain = (int64_t)s.ndacc + s.nddist + s.nobs + 16 * (int64_t)s.ncols + 2 * (int64_t)p->npa + s.nedge + s.nbin;
    const int64_t carve = s.table_mode == 0 && s.ntile == 1 && s.ec_doubles == 0 ? (p->lds_bytes + 7) / 8 : plain;
    const int64_t a = carve + strat_chunk_lds_bytes(nloc, NW) / 8, b = (int64_t)mci::train_lds_doubles(maxn) + maxn + 256;
    const int64_t off = ((a > b ? a : b) + 1) & ~(int64_t)1;
    if (map_off) *map_off = (int)off;
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };
    return (off + even(s.nedge) + even(s.ndacc) + even(s.nddist) + 4 + 4 * (int64_t)mci::kStratMaxCols + 2) * 8;
}
// what is left to check of the layout of a stratified problem that opted in to sweeps over all its leaves and is no one-grid layout
const char *sweep_strat_leaves_refusal(const mci_problem *p, std::string &buf) {
    const auto &s = p->shape;
    for (const Leaf &L : p->leaves)
        if (L.kind != MCI_CONTINUOUS) return "a Discrete or FermiK variable (a stratified sweep point refines Continuous grids only)";
    if (p->leaves.empty() || s.nleaf != (int)p->leaves.size() || s.nbin <= 0) return "no variable leaves";
    const int64_t lds = sweep_strat_leaves_lds(p, strat_nloc(1), nullptr); // (the smallest chunk: one trip)
    if (lds > kSweepLeavesMaxLds) {
        buf = "the sample tables, one chunk's hypercubes, the refinement scratch and the point's map take " + std::to_string((long long)lds) + " bytes of LDS (" +
              std::to_string((long long)kSweepLeavesMaxLds) + " at most)";
        return buf.c_str();
    }
    if (s.table_mode != 0 || s.ntile != 1 || s.ec_doubles > 0) return "the tables and their histograms do not sit in LDS in one tile";
    return nullptr;
}
// LDS of the unit a stratified sweep of this problem runs, and the two geometries of a call of nsamp samples in `blocks` blocks: g0 the
// ordinary stratified call's (its mblocks: what strat_run merges the rows as), g this kernel's own (its chunk)
int64_t sweep_strat_unit_lds(const mci_problem *p, bool leaves, int nloc, int *map_off) {
    return leaves ? sweep_strat_leaves_lds(p, nloc, map_off) : sweep_strat_lds(p, nloc, map_off);
}
int sweep_strat_geometry(const mci_problem *p, bool leaves, int64_t nsamp, int64_t blocks, StratGeometry &g0, StratGeometry &g) {
    const int NW = p->shape.ni * p->shape.ncomp;
    int64_t need0[4], need[4];
    for (int k = 0; k < 4; ++k) {
        need0[k] = p->lds_bytes + strat_chunk_lds_bytes(strat_nloc(8 >> k), NW);
        need[k] = sweep_strat_unit_lds(p, leaves, strat_nloc(8 >> k), nullptr);
    }
    strat_geometry(nsamp, blocks, need0, g0);
    strat_geometry(nsamp, blocks, need, g);
    if (!g0.trips || !g.trips) return fail(MCI_ERR_INVALID, "stratification: the tables and the chunk's hypercubes do not fit one CU's LDS");
    return MCI_OK;
}
// samples per iteration of a call (main.jl:121 on one rank)
int64_t sweep_strat_nsamp(const mci_integrate_args *a, int64_t *nblocks) {
    int64_t nevalperblock, block;
    mci_standardize_block(a->neval, a->block, 1, &nevalperblock, &block);
    if (nblocks) *nblocks = block;
    return nevalperblock * block;
}
const char *sweep_strat_refusal(const mci_problem *p, const mci_integrate_args *a, std::string &buf) {
    const auto &s = p->shape;
    if (const char *r = sweep_common_refusal(p, a, buf, true)) return r;
    const bool leaves = sweep_strat_uses_leaves(p); // (opted in: mci_set_sweep_strat_leaves)
    if (leaves) {
        if (const char *r = sweep_strat_leaves_refusal(p, buf)) return r;
    } else if (const char *r = sweep_one_grid_refusal(p, buf, true)) return r;
    if (s.ndraw > mci::kStratMaxDraw) {
        buf = std::to_string(s.ndraw) + " draws per sample (at most " + std::to_string((int)mci::kStratMaxDraw) + ")";
        return buf.c_str();
    }
    if (s.ni * s.ncomp > mci::kStratMaxCols) {
        buf = std::to_string(s.ni * s.ncomp) + " weight columns (at most " + std::to_string((int)mci::kStratMaxCols) + ")";
        return buf.c_str();
    }
    if (!(a->neval > a->block)) return "neval should be larger than nblock";
    const int64_t N = sweep_strat_nsamp(a, nullptr);
    std::vector<int> ns;
    int64_t ncube = 0;
    if (sweep_strat_plan(p, N, ns, &ncube)) {
        buf = g_err;
        return buf.c_str();
    }
    if (ncube > N / 2) {
        buf = std::to_string((long long)ncube) + " hypercubes need at least " + std::to_string((long long)(2 * ncube)) + " samples per iteration (two each), neval = " +
              std::to_string((long long)N);
        return buf.c_str();
    }
    if (leaves) return nullptr; // (its LDS: sweep_strat_leaves_refusal)
    const int64_t lds = sweep_strat_lds(p, strat_nloc(1), nullptr); // (the smallest chunk: one trip)
    if (lds > kSweepLeavesMaxLds) {
        buf = "the sample tables, one chunk's hypercubes, the refinement scratch and the map copy take " + std::to_string((long long)lds) + " bytes of LDS (" +
              std::to_string((long long)kSweepLeavesMaxLds) + " at most)";
        return buf.c_str();
    }
    return nullptr;
}
} // namespace

static bool sweep_strat_leaves_unit(const mci_problem *p) { return sweep_strat_uses_leaves(p); }

// csrc/mci_debug.h
int mci_debug_sweep_strat_geometry(const mci_problem *p, const mci_integrate_args *a, int64_t *chunk, int64_t *lds_bytes, int32_t *map_off, int32_t *mblocks) {
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    if (int rc = mci_sweep_strat_supported(p, a, nullptr, 0)) return rc;
    const bool leaves = sweep_strat_uses_leaves(p);
    int64_t blocks = 0;
    const int64_t nsamp = sweep_strat_nsamp(a, &blocks);
    StratGeometry g0, g;
    if (int rc = sweep_strat_geometry(p, leaves, nsamp, blocks, g0, g)) return rc;
    int off = 0;
    const int64_t lds = sweep_strat_unit_lds(p, leaves, (int)(g.S / 2 + 1), &off);
    if (chunk) *chunk = g.S;
    if (lds_bytes) *lds_bytes = lds;
    if (map_off) *map_off = off;
    if (mblocks) *mblocks = (int32_t)g0.mblocks;
    return MCI_OK;
}

int mci_sweep_strat_supported(const mci_problem *p, const mci_integrate_args *a, char *why, int32_t n) {
    if (why && n > 0) why[0] = 0;
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    std::string buf;
    const char *r = sweep_strat_refusal(p, a, buf);
    if (!r) return MCI_OK;
    const std::string reason = r; // (may live in g_err, which fail() rewrites)
    if (why && n > 0) snprintf(why, (size_t)n, "%s", reason.c_str());
    return fail(MCI_ERR_INVALID, "this problem cannot run as a stratified sweep: %s", reason.c_str());
}

int mci_sweep_strat_doubles(const mci_problem *p, const mci_integrate_args *a, int64_t *ncube) {
    if (!p || !a || !ncube) return fail(MCI_ERR_INVALID, "NULL argument");
    int rc;
    if ((rc = mci_sweep_strat_supported(p, a, nullptr, 0))) return rc;
    std::vector<int> ns;
    return sweep_strat_plan(p, sweep_strat_nsamp(a, nullptr), ns, ncube);
}

// P independent stratified integrate() loops, one workgroup each, in one launch
static_assert(offsetof(mci::SweepStratArgs, h) == 0, "sweep_run fills the stratified unit's argument through its head");
int mci_integrate_sweep_strat(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                              double *maps_out, const double *d_in, double *d_out, int64_t *counts_out, mci_result *results, double *iter_mean, double *iter_std,
                              int32_t *status) {
    if (int rc = sweep_check_args(p, a, npoint, userdata, results, mci_sweep_strat_supported)) return rc;
    const auto &s = p->shape;
    const size_t P = (size_t)npoint;
    int64_t ncube = 0;
    std::vector<int> ns;
    StratGeometry g0, g;
    mci::SweepStratArgs f{};
    std::vector<long long> hoff;
    SweepCall c;
    const bool leaves = sweep_strat_uses_leaves(p); // (several Continuous leaves, opted in: mci_sweep_strat_leaves.h)
    c.unit = leaves ? mci_problem::Sweep::kStratLeaves : mci_problem::Sweep::kStrat;
    c.npoint = npoint, c.userdata = userdata, c.seeds = seeds, c.maps_in = maps_in, c.maps_out = maps_out;
    c.results = results, c.iter_mean = iter_mean, c.iter_std = iter_std, c.status = status;
    c.plan = [&, p, a](SweepCall &c) {
        const int64_t nsamp = sweep_strat_nsamp(a, &c.blocks);
        if (int rc = sweep_strat_plan(p, nsamp, ns, &ncube)) return rc;
        if (int rc = sweep_strat_geometry(p, leaves, nsamp, c.blocks, g0, g)) return rc;
        c.neval_per_block = nsamp / c.blocks;
        c.rows = 1;
        c.off_doubles = (size_t)ncube + 1;
        c.tbase_doubles = (size_t)mci::strat_alloc_ntile(ncube);
        c.d_doubles = (size_t)ncube;
        c.lds = sweep_strat_unit_lds(p, leaves, (int)(g.S / 2 + 1), &c.map_off);
        c.too_big_count = (long long)ncube;
        hoff.resize(counts_out ? P * ((size_t)ncube + 1) : 0);
        return (int)MCI_OK;
    };
    c.map_doubles = leaves ? (size_t)sweep_map_doubles(p) : (size_t)p->leaves[0].nbin + 1;
    c.maxn = leaves ? sweep_max_nbin(p) : p->leaves[0].nbin;
    c.strat_stats = true;
    c.too_big = "a stratified sweep of %d points x %d iterations x %lld hypercubes needs %lld bytes of device memory (limit %lld): split it";
    c.copy_in = [&](double *d, const size_t *o, hipStream_t st) {
        if (d_in) HIPCHK(hipMemcpyAsync(d + o[kSegD], d_in, P * (size_t)ncube * sizeof(double), hipMemcpyHostToDevice, st));
        return (int)MCI_OK;
    };
    c.args = [&, p](const mci::SweepHead &h, double *d, const size_t *o) -> void * {
        f.h = h;
        mci::StratArgs &sa = f.st;
        sa.off = reinterpret_cast<const long long *>(d + o[kSegOff]);
        sa.dnext = d + o[kSegD];
        sa.ncube = ncube;
        sa.nsamp = c.neval_per_block * c.blocks;
        sa.chunk = g.S;
        sa.nchunk = g.nchunk;
        sa.first_index = 0;
        sa.nloc = (int)(g.S / 2 + 1);
        sa.beta = p->strat.beta;
        for (int k = 0; k < s.ndraw; ++k) {
            const uint32_t n = (uint32_t)ns[k];
            strat_magic(n, &sa.magic[k], &sa.shift[k]);
            sa.nstrat[k] = (int)n;
            sa.inv[k] = 1.0 / (double)n;
        }
        f.have_d = d_in ? 1 : 0;
        f.start_uniform = 1;
        f.mblocks = (int)g0.mblocks;
        f.ntile = (int)c.tbase_doubles;
        f.tbase = d + o[kSegTbase];
        return &f;
    };
    c.copy_out = [&](double *d, const size_t *o, hipStream_t st) {
        if (d_out) HIPCHK(hipMemcpyAsync(d_out, d + o[kSegD], P * (size_t)ncube * sizeof(double), hipMemcpyDeviceToHost, st));
        if (counts_out) HIPCHK(hipMemcpyAsync(hoff.data(), d + o[kSegOff], hoff.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
        return (int)MCI_OK;
    };
    c.finish = [&] {
        const size_t nc = (size_t)ncube;
        if (counts_out)
            for (size_t q = 0; q < P; ++q)
                for (size_t h = 0; h < nc; ++h) counts_out[q * nc + h] = hoff[q * (nc + 1) + h + 1] - hoff[q * (nc + 1) + h];
    };
    return sweep_run(p, a, c);
}

// ---------------------------------------------------------------------------------------------------
// :vegasmc and :mcmc points in a sweep: mci_sweep_chains.h vegasmc_sweep | mcmc_sweep, one workgroup runs a point's whole chain-solver loop
// ---------------------------------------------------------------------------------------------------
namespace {
int sweep_nslots(const mci_problem *p) { // (pool, slot) pairs changeVariable can pick (plan_vegasmc_chains, plan_mcmc_chains)
    int nslots = 0;
    for (int v = 0; v < p->npool; ++v) nslots += p->maxdof[v];
    return nslots;
}
// what sweep_common_refusal and sweep_leaves_refusal check, the solver test the other way round, and what the chain loop adds;
// solver: the entry point's (MCI_VEGASMC: mci_integrate_sweep_chains, MCI_MCMC: mci_integrate_sweep_mcmc)
const char *sweep_chains_refusal(const mci_problem *p, const mci_integrate_args *a, std::string &buf, int32_t solver) {
    const bool mcmc = solver == MCI_MCMC;
    if (const char *r = sweep_common_refusal(p, a, buf, false, solver)) return r;
    if (a->nchain == 0) return "nchain = 0 (the automatic policy sizes chains from carried state a sweep does not have: give nchain >= 1)";
    if (a->nchain < 0) return "nchain < 0";
    if (a->reweight_goal || !p->h_goal.empty()) return "a reweight goal (a sweep point reweights without one)";
    // (:mcmc itself runs FermiK pools; the point's map block in LDS, SweepBlock, has no place for them yet)
    if (mcmc && p->has_fermik) return "a FermiK variable (a sweep point's map block holds Continuous and Discrete leaves only: FermiK points are a follow-up)";
    if (const char *r = sweep_leaves_refusal(p, buf)) return r; // (FermiK, the tables in LDS in one tile, the LDS budget: Lds<Cfg> counts the counters)
    if (!(a->neval > a->block)) return "neval should be larger than nblock";
    int64_t npb, blocks;
    mci_standardize_block(a->neval, a->block, 1, &npb, &blocks);
    // (a chain's streams are addressed by (block < 4096, iteration < 131072), mci_device.h vegasmc_chains: the limits of the ordinary
    // chain launch, mci_host_iteration.h -- a block or an iteration beyond them would run another one's chains again)
    if (blocks > 4096) {
        buf = "block = " + std::to_string((long long)blocks) + " (chain solvers address a chain by block < 4096)";
        return buf.c_str();
    }
    if (a->first_iteration < 0 || (int64_t)a->first_iteration + a->niter > 131072) {
        buf = "first_iteration = " + std::to_string((long long)a->first_iteration) + ", niter = " + std::to_string((long long)a->niter) +
              " (chain solvers address a chain by 0 <= iteration < 131072)";
        return buf.c_str();
    }
    if (a->nchain > npb) {
        buf = "nchain = " + std::to_string((long long)a->nchain) + " exceeds the " + std::to_string((long long)npb) + " steps of a block";
        return buf.c_str();
    }
    if (mcmc) {
        if (!std::isfinite(a->thermal_ratio) || a->thermal_ratio < 0.0) {
            buf = "thermal_ratio = " + std::to_string(a->thermal_ratio) + " (the burn-in is floor(steps * thermal_ratio): finite and >= 0)";
            return buf.c_str();
        }
        // (a chain counts its steps and its holding times in 32 bits, mci_device.h mcmc_chains: the ordinary launch drops the diagnostic
        // beyond, a sweep point has nothing else to say that its chains were too short)
        const int64_t steps = npb / a->nchain;
        // (a ratio whose floor(steps * thermal_ratio) would not fit an int64_t is past the limit whatever else holds)
        const int64_t nburn = (double)steps * a->thermal_ratio < 9.0e18 ? mci_mcmc_burnin(steps, a->nchain, sweep_nslots(p), p->ni + 1, p->npool, a->thermal_ratio)
                                                                        : ((int64_t)1 << 62);
        if (steps + nburn >= ((int64_t)1 << 31) - 1) {
            buf = "steps + nburn = " + std::to_string((long long)steps) + " + " + std::to_string((long long)nburn) + " per chain (a sweep's :mcmc chain has fewer than 2^31 - 1 steps)";
            return buf.c_str();
        }
    }
    return nullptr;
}

int sweep_chains_query(const mci_problem *p, const mci_integrate_args *a, char *why, int32_t n, int32_t solver) {
    if (why && n > 0) why[0] = 0;
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    std::string buf;
    const char *r = sweep_chains_refusal(p, a, buf, solver);
    if (!r) return MCI_OK;
    if (why && n > 0) snprintf(why, (size_t)n, "%s", r);
    return fail(MCI_ERR_INVALID, "this problem cannot run as a sweep of %s points: %s", solver == MCI_MCMC ? ":mcmc" : ":vegasmc", r);
}

// doubles of one point's chain state row (include/mci.h mci_sweep_chain_state; mci_sweep_chains.h SweepResumeArgs): x [ndraw][cap] | P [cap]
// (:vegasmc) or curr [cap] ints on whole doubles | reweight_used [nd] (:mcmc)
size_t sweep_state_doubles(int ndraw, int nd, int64_t blocks, int64_t nchain, bool mcmc) {
    const size_t cap = (size_t)blocks * (size_t)nchain;
    return (size_t)ndraw * cap + (mcmc ? (cap + 1) / 2 + (size_t)nd : cap);
}
// what the *_resume entry points refuse beyond sweep_chains_refusal, and whether iteration 0 continues the state's chains: plan_may_carry
// (mci_host_plan.h) with the state's record in place of launch.chain_*
const char *sweep_state_refusal(const mci_problem *p, const mci_integrate_args *a, const mci_sweep_chain_info *st, std::string &buf, bool *continues) {
    const bool mcmc = a->solver == MCI_MCMC;
    *continues = false;
    if (const char *r = sweep_chains_refusal(p, a, buf, mcmc ? MCI_MCMC : MCI_VEGASMC)) return r;
    if (!p->sweep.chain_carry) return "the sweep chain carry is off (mci_set_sweep_chain_carry(prob, 1) first: only carried chains travel between calls)";
    if (a->nchain == 1) return "nchain = 1 together with a chain state (nothing is carried with one chain per block)";
    if (!st) return nullptr;
    int64_t npb, blocks;
    mci_standardize_block(a->neval, a->block, 1, &npb, &blocks);
    if (st->solver != a->solver) {
        buf = std::string("the state is another solver's (stored under ") + (st->solver == MCI_MCMC ? ":mcmc" : st->solver == MCI_VEGASMC ? ":vegasmc" : "an unknown solver") +
              ", the call runs " + (mcmc ? ":mcmc" : ":vegasmc") + ")";
        return buf.c_str();
    }
    if (st->blocks != blocks) {
        buf = "the state holds another block count (" + std::to_string((long long)st->blocks) + " blocks stored, the call runs " + std::to_string((long long)blocks) + ")";
        return buf.c_str();
    }
    if (st->nd != p->ni + 1 || st->ndraw != p->shape.ndraw) {
        buf = "the state is another layout's (nd = " + std::to_string(st->nd) + ", ndraw = " + std::to_string(st->ndraw) + " stored, the problem has nd = " +
              std::to_string(p->ni + 1) + ", ndraw = " + std::to_string(p->shape.ndraw) + ")";
        return buf.c_str();
    }
    if (st->nchain < 2) {
        buf = "the state holds " + std::to_string((long long)st->nchain) + " chains per block (nothing is carried with fewer than two)";
        return buf.c_str();
    }
    if (st->nchain > ((int64_t)1 << 31) / blocks) { // (blocks >= 1: sweep_chains_refusal took neval > block)
        buf = "the state holds " + std::to_string((long long)st->nchain) + " chains per block (blocks x chains is addressed in 32 bits)";
        return buf.c_str();
    }
    if (st->ntrain < 0 || st->iteration < 0) return "the state's record is damaged (a negative iteration or train! count)";
    if ((int64_t)st->iteration + 1 != (int64_t)a->first_iteration) {
        buf = "a gap in the iteration numbers (the state was stored by iteration " + std::to_string(st->iteration) + ", the call starts at first_iteration = " +
              std::to_string((long long)a->first_iteration) + ": " + std::to_string(st->iteration + 1) + " continues it)";
        return buf.c_str();
    }
    // (:vegasmc: not out of an iteration on the never-refined map onto a refined one -- chain_ntrain >= 1 || chain_ntrain == ntrain)
    *continues = mcmc || st->ntrain >= 1 || !st->adapted;
    return nullptr;
}

// P independent chain-solver integrate() loops (main.jl:142-207 around vegas_mc/montecarlo.jl:112-241 | mcmc/montecarlo.jl:72-187), one
// workgroup each, in one launch.  What the two entry points share; solver: MCI_VEGASMC | MCI_MCMC (holds_out: the latter's)
static_assert(offsetof(mci::SweepChainArgs, h) == 0, "sweep_run fills the chain units' argument through its head");
static_assert(offsetof(mci::SweepChainCarryArgs, c) == 0, "one object serves the four chain units: the uncarried ones read its first member");
int sweep_chains_call(mci_problem *p, const mci_integrate_args *a, int32_t solver, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                      double *maps_out, const double *reweight_in, double *reweight_out, double *pa_out, uint64_t *holds_out, mci_result *results,
                      double *iter_mean, double *iter_std, int32_t *status, const mci_sweep_chain_state *state_in = nullptr, mci_sweep_chain_state *state_out = nullptr) {
    const bool mcmc = solver == MCI_MCMC;
    // chains that travel between calls (the *_resume entry points): the state's record against the call's, first -- a refusal is the same
    // with and without a device
    bool first_cont = false; // iteration 0 continues the state's chains
    int ntrain0 = 0;         // train! calls of the points' lineage before iteration 0
    int64_t k_old = 0;
    size_t state_row_in = 0;
    if (state_in || state_out) {
        if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
        if ((state_in && !state_in->rows) || (state_out && !state_out->rows)) return fail(MCI_ERR_INVALID, "a chain state without rows");
        if (a->solver != solver) return fail(MCI_ERR_INVALID, "this problem cannot run as a sweep of %s points: %s", mcmc ? ":mcmc" : ":vegasmc", mcmc ? "solver is not :mcmc" : "solver is not :vegasmc");
        int32_t cont = 0;
        if (int rc = mci_sweep_chain_state_supported(p, a, state_in ? &state_in->info : nullptr, nullptr, 0, &cont)) return rc;
        first_cont = cont != 0;
        if (state_in) {
            ntrain0 = state_in->info.ntrain + (state_in->info.adapted ? 1 : 0);
            k_old = state_in->info.nchain;
            state_row_in = sweep_state_doubles(state_in->info.ndraw, state_in->info.nd, state_in->info.blocks, k_old, mcmc);
        }
    }
    if (int rc = sweep_check_args(p, a, npoint, userdata, results, mcmc ? mci_sweep_mcmc_supported : mci_sweep_chains_supported)) return rc;
    const size_t P = (size_t)npoint, nd = (size_t)p->ni + 1, npa2 = 2 * (size_t)p->npa;
    const size_t tables = (size_t)p->nstat + p->shape.nbin; // where merge_pa leaves them in a packed row (mci_train.h)
    mci::SweepChainResumeArgs fa{}; // (the uncarried units' argument is its first member, the carried units' its first two)
    mci::SweepChainArgs &f = fa.c;
    mci::SweepCarryArgs &fk = fa.k;
    mci::SweepResumeArgs &fr = fa.r;
    std::vector<double> hrw, hbm;
    SweepCall c;
    // mci_set_sweep_chain_carry: the units with carried chains.  What a point keeps between its iterations, per point, in doubles of
    // kSegCarry (cap = blocks * nchain stored chains a buffer): x [2][ndraw][cap] | P [2][cap] (:vegasmc) or curr [2][cap] ints (:mcmc) |
    // W [cap] | w [cap] (:vegasmc) or reweight_used [nd] (:mcmc) | src [cap] ints
    const bool carry = p->sweep.chain_carry != 0;
    // (... nor, with a state, where the lineage's map was refined before iteration 0 already: ntrain0 >= 1)
    const int carry_first = (mcmc || !a->adapt || ntrain0 >= 1) ? 1 : 2; // (plan_may_carry: :vegasmc not out of the iteration on the map before its first refinement)
    const bool carried = carry && a->nchain > 1 && (a->niter > carry_first || first_cont); // some iteration of every point continues the one before
    size_t cx = 0, cp = 0, cw = 0, cw2 = 0, csrc = 0, wcap = 0; // offsets of the parts behind x, doubles; a point's running weights
    c.unit = carry ? (mcmc ? mci_problem::Sweep::kMcmcCarry : mci_problem::Sweep::kChainsCarry) : (mcmc ? mci_problem::Sweep::kMcmc : mci_problem::Sweep::kChains);
    if (first_cont) c.unit = mcmc ? mci_problem::Sweep::kMcmcResume : mci_problem::Sweep::kChainsResume; // (the carry setting is on: the query)
    c.first_continued = first_cont;
    c.state_doubles = first_cont ? state_row_in : 0;
    size_t state_row_out = 0;
    c.npoint = npoint, c.userdata = userdata, c.seeds = seeds, c.maps_in = maps_in, c.maps_out = maps_out;
    c.results = results, c.iter_mean = iter_mean, c.iter_std = iter_std, c.status = status;
    c.plan = [&, a, npa2](SweepCall &c) {
        mci_standardize_block(a->neval, a->block, 1, &c.neval_per_block, &c.blocks); // main.jl:121 (at most 4096 blocks: sweep_chains_refusal)
        c.rows = c.blocks;
        c.pa_doubles = (size_t)c.blocks * npa2;
        c.too_big_count = (long long)c.blocks;
        if (carry) {
            const size_t cap = (size_t)c.blocks * (size_t)a->nchain, half = (cap + 1) / 2;
            wcap = first_cont && k_old > a->nchain ? (size_t)c.blocks * (size_t)k_old : cap; // (iteration 0 weighs the state's K_old chains a block)
            cx = 2 * (size_t)p->shape.ndraw * cap;
            cp = cx;                            // P [2][cap] | curr [2][cap] ints
            cw = cp + (mcmc ? 2 * half : 2 * cap);
            cw2 = cw + wcap;                    // w [wcap] | reweight_used [nd]
            csrc = cw2 + (mcmc ? nd : wcap);
            state_row_out = sweep_state_doubles(p->shape.ndraw, (int)nd, c.blocks, a->nchain, mcmc);
            c.carry_doubles = csrc + half;
            c.blk_doubles = (size_t)a->niter * (size_t)c.blocks * (size_t)p->shape.nobs;
            hbm.resize(carried ? P * c.blk_doubles : 0);
        }
        return (int)MCI_OK;
    };
    c.map_doubles = (size_t)sweep_map_doubles(p);
    c.maxn = sweep_max_nbin(p);
    c.lds = sweep_leaves_lds(p, &c.map_off);
    c.rw_doubles = nd;
    c.packed_doubles = tables + npa2 + 64; // (+ 64: merge_pa's holding-time histogram: zeros under either solver, MergeArgs::hold stays NULL)
    c.holds_doubles = mcmc ? 64 : 0;       // (64 words of 8 bytes: the kernel adds to them, the host reads them)
    c.too_big = mcmc ? "a sweep of %d :mcmc points x %d iterations x %lld blocks needs %lld bytes of device memory (limit %lld): split it"
                     : "a sweep of %d :vegasmc points x %d iterations x %lld blocks needs %lld bytes of device memory (limit %lld): split it";
    c.batch = [p, a, &c, mcmc](mci::BatchArgs &b) { // (fresh chains in every iteration)
        b.nchain = a->nchain;
        if (mcmc) b.nburn = mci_mcmc_burnin(c.neval_per_block / a->nchain, a->nchain, sweep_nslots(p), p->ni + 1, p->npool, a->thermal_ratio);
        else b.burnin = mci_chain_burnin(c.neval_per_block / a->nchain, a->nchain, sweep_nslots(p));
    };
    c.copy_in = [&](double *d, const size_t *o, hipStream_t st) {
        if (!reweight_in) { // every point starts from the problem's current factors (the device's: doReweight! moves them there)
            hrw.resize(P * nd);
            HIPCHK(hipMemcpyAsync(hrw.data(), p->d_reweight, nd * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t q = 1; q < P; ++q) memcpy(hrw.data() + q * nd, hrw.data(), nd * sizeof(double));
        }
        HIPCHK(hipMemcpyAsync(d + o[kSegRw], reweight_in ? reweight_in : hrw.data(), P * nd * sizeof(double), hipMemcpyHostToDevice, st));
        if (first_cont) HIPCHK(hipMemcpyAsync(d + o[kSegState], state_in->rows, P * state_row_in * sizeof(double), hipMemcpyHostToDevice, st));
        return (int)MCI_OK;
    };
    c.args = [&, p, a](const mci::SweepHead &h, double *d, const size_t *o) -> void * {
        f.h = h;
        f.h.m.npa = p->npa;
        f.h.t.do_reweight = 1; // main.jl:183
        f.h.t.goal = nullptr;
        f.h.t.gamma = a->gamma;
        f.reweight = d + o[kSegRw];
        f.part_pa = d + o[kSegPa];
        f.packed_stride = (int)c.packed_doubles;
        f.holds = mcmc ? reinterpret_cast<unsigned long long *>(d + o[kSegHolds]) : nullptr; // (zeroed with everything from kSegGhist on)
        if (carry) { // (a point's parts lie one behind the other in its kSegCarry row: the kernel strides by the part's own length, so
            // every part is laid out [npoint][part] -- the segment is cut part by part, not point by point)
            const size_t cap = (size_t)c.blocks * (size_t)a->nchain, half = (cap + 1) / 2;
            double *g = d + o[kSegCarry];
            fk.chain_x = g;
            g += P * cx;
            if (mcmc) fk.chain_curr = reinterpret_cast<int *>(g), g += P * 2 * half;
            else fk.chain_P = g, g += P * 2 * cap;
            fk.carry_W = g;
            g += P * wcap;
            if (mcmc) fk.rw_used = g, g += P * nd;
            else fk.carry_w = g, g += P * wcap;
            fk.carry_src = reinterpret_cast<int *>(g);
            fk.block_means = d + o[kSegBlk];
            const int64_t steps = c.neval_per_block / a->nchain;
            fk.nburn_carried = 0;                                          // plan_mcmc_chains: carried chains have no start to burn in
            fk.burnin_carried = mci_chain_burnin(steps, 1, sweep_nslots(p)); // plan_vegasmc_chains: the reference's own neval / 100
            fk.carry_first = carry_first;
            fk.lds_w = sweep_resample_lds(c.map_off);
            if (first_cont) {
                fr.state_in = d + o[kSegState];
                fr.state_stride = (mci::i64)state_row_in;
                fr.nchain_old = k_old;
                fr.wcap = (mci::i64)wcap;
            }
        }
        return &fa;
    };
    c.copy_out = [&](double *d, const size_t *o, hipStream_t st) {
        if (reweight_out) HIPCHK(hipMemcpyAsync(reweight_out, d + o[kSegRw], P * nd * sizeof(double), hipMemcpyDeviceToHost, st));
        if (pa_out)
            HIPCHK(hipMemcpy2DAsync(pa_out, npa2 * sizeof(double), d + o[kSegPacked] + tables, c.packed_doubles * sizeof(double), npa2 * sizeof(double), P,
                                    hipMemcpyDeviceToHost, st));
        if (mcmc && holds_out) HIPCHK(hipMemcpyAsync(holds_out, d + o[kSegHolds], P * 64 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (!hbm.empty()) HIPCHK(hipMemcpyAsync(hbm.data(), d + o[kSegBlk], hbm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (state_out) { // the buffer the last iteration wrote, part by part into every point's row (the padding behind an odd count of indices: zero)
            const size_t cap = (size_t)c.blocks * (size_t)a->nchain, half = (cap + 1) / 2, nx = (size_t)p->shape.ndraw * cap, wb = (size_t)(a->niter - 1) & 1;
            const size_t row = state_row_out * sizeof(double);
            memset(state_out->rows, 0, P * row);
            HIPCHK(hipMemcpy2DAsync(state_out->rows, row, fk.chain_x + wb * nx, 2 * nx * sizeof(double), nx * sizeof(double), P, hipMemcpyDeviceToHost, st));
            if (mcmc) {
                HIPCHK(hipMemcpy2DAsync(state_out->rows + nx, row, fk.chain_curr + wb * cap, 2 * cap * sizeof(int), cap * sizeof(int), P, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpy2DAsync(state_out->rows + nx + half, row, fk.rw_used, nd * sizeof(double), nd * sizeof(double), P, hipMemcpyDeviceToHost, st));
            } else
                HIPCHK(hipMemcpy2DAsync(state_out->rows + nx, row, fk.chain_P + wb * cap, 2 * cap * sizeof(double), cap * sizeof(double), P, hipMemcpyDeviceToHost, st));
        }
        return (int)MCI_OK;
    };
    c.finish = [&] { c.block_means = hbm.empty() ? nullptr : hbm.data(); };
    if (int rc = sweep_run(p, a, c)) return rc;
    if (state_out) { // the record of what the rows hold: plan_may_carry's fields for the next call
        mci_sweep_chain_info &si = state_out->info;
        si.solver = solver;
        si.nd = (int32_t)nd;
        si.ndraw = p->shape.ndraw;
        si.iteration = a->first_iteration + a->niter - 1;
        si.ntrain = ntrain0 + (a->adapt ? a->niter - 1 : 0);
        si.adapted = a->adapt ? 1 : 0;
        si.blocks = c.blocks;
        si.nchain = a->nchain;
    }
    return MCI_OK;
}
} // namespace

int mci_sweep_chains_supported(const mci_problem *p, const mci_integrate_args *a, char *why, int32_t n) { return sweep_chains_query(p, a, why, n, MCI_VEGASMC); }
int mci_sweep_mcmc_supported(const mci_problem *p, const mci_integrate_args *a, char *why, int32_t n) { return sweep_chains_query(p, a, why, n, MCI_MCMC); }

int mci_integrate_sweep_chains(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                               double *maps_out, const double *reweight_in, double *reweight_out, double *pa_out, mci_result *results, double *iter_mean,
                               double *iter_std, int32_t *status) {
    return sweep_chains_call(p, a, MCI_VEGASMC, npoint, userdata, seeds, maps_in, maps_out, reweight_in, reweight_out, pa_out, nullptr, results, iter_mean, iter_std, status);
}
int mci_sweep_chain_state_supported(const mci_problem *p, const mci_integrate_args *a, const mci_sweep_chain_info *state, char *why, int32_t n, int32_t *continues) {
    if (why && n > 0) why[0] = 0;
    if (continues) *continues = 0;
    if (!p || !a) return fail(MCI_ERR_INVALID, "NULL argument");
    std::string buf;
    bool cont = false;
    const char *r = sweep_state_refusal(p, a, state, buf, &cont);
    if (!r) {
        if (continues) *continues = cont ? 1 : 0;
        return MCI_OK;
    }
    if (why && n > 0) snprintf(why, (size_t)n, "%s", r);
    return fail(MCI_ERR_INVALID, "this chain sweep cannot go on from a chain state: %s", r);
}
int mci_sweep_chain_state_doubles(const mci_problem *p, const mci_integrate_args *a, int64_t *doubles, mci_sweep_chain_info *info) {
    if (!p || !a || !doubles) return fail(MCI_ERR_INVALID, "NULL argument");
    const bool mcmc = a->solver == MCI_MCMC;
    if (int rc = sweep_chains_query(p, a, nullptr, 0, mcmc ? MCI_MCMC : MCI_VEGASMC)) return rc;
    if (a->nchain < 2) return fail(MCI_ERR_INVALID, "this chain sweep cannot go on from a chain state: nchain = 1 together with a chain state (nothing is carried with one chain per block)");
    int64_t npb, blocks;
    mci_standardize_block(a->neval, a->block, 1, &npb, &blocks);
    *doubles = (int64_t)sweep_state_doubles(p->shape.ndraw, p->ni + 1, blocks, a->nchain, mcmc);
    if (info) *info = mci_sweep_chain_info{a->solver, p->ni + 1, p->shape.ndraw, a->first_iteration + a->niter - 1, a->adapt ? a->niter - 1 : 0, a->adapt ? 1 : 0, blocks, a->nchain};
    return MCI_OK;
}
int mci_integrate_sweep_chains_resume(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                                      double *maps_out, const double *reweight_in, double *reweight_out, double *pa_out, const mci_sweep_chain_state *state_in,
                                      mci_sweep_chain_state *state_out, mci_result *results, double *iter_mean, double *iter_std, int32_t *status) {
    return sweep_chains_call(p, a, MCI_VEGASMC, npoint, userdata, seeds, maps_in, maps_out, reweight_in, reweight_out, pa_out, nullptr, results, iter_mean, iter_std, status, state_in, state_out);
}
int mci_integrate_sweep_mcmc_resume(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                                    double *maps_out, const double *reweight_in, double *reweight_out, double *pa_out, uint64_t *holds_out,
                                    const mci_sweep_chain_state *state_in, mci_sweep_chain_state *state_out, mci_result *results, double *iter_mean, double *iter_std,
                                    int32_t *status) {
    return sweep_chains_call(p, a, MCI_MCMC, npoint, userdata, seeds, maps_in, maps_out, reweight_in, reweight_out, pa_out, holds_out, results, iter_mean, iter_std, status, state_in, state_out);
}
// mcmc/montecarlo.jl:72-187, mcmc/updates.jl, main.jl:183, :322-346
int mci_integrate_sweep_mcmc(mci_problem *p, const mci_integrate_args *a, int32_t npoint, const double *userdata, const uint64_t *seeds, const double *maps_in,
                             double *maps_out, const double *reweight_in, double *reweight_out, double *pa_out, uint64_t *holds_out, mci_result *results,
                             double *iter_mean, double *iter_std, int32_t *status) {
    return sweep_chains_call(p, a, MCI_MCMC, npoint, userdata, seeds, maps_in, maps_out, reweight_in, reweight_out, pa_out, holds_out, results, iter_mean, iter_std, status);
}
