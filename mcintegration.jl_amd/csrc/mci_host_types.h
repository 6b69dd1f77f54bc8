// mci_host_types.h -- part of the ONE translation unit mci_api.hip (included there, in order; not a stand-alone header):
// the RCCL loader, mci_ctx, the problem's host-side state (mci_problem), the process-wide test overrides and the helpers every section uses (upload, capacity, status, the :mcmc holding-time hand-over).
namespace {

// ---- RCCL, loaded lazily so that single-GPU use never touches it -----------------------------------
struct Id128 { char b[128]; }; // ncclUniqueId (rccl.h:43)
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, Id128 /* by value */, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
const int kNcclFloat64 = 8, kNcclSum = 0; // ncclDouble, ncclSum (rccl.h)

// If the host process already carries an RCCL (PyTorch-ROCm bundles its own and resolves it through its rpath),
// bind to THAT copy: two RCCL instances in one process would each open their own IPC/proxy state on the same GPUs.
int find_loaded_rccl(struct dl_phdr_info *info, size_t, void *out) {
    const char *n = info->dlpi_name;
    if (n && strstr(n, "librccl.so")) {
        *(std::string *)out = n;
        return 1;
    }
    return 0;
}

int rccl_load() {
    if (g_rccl.h) return MCI_OK;
    void *h = nullptr;
    std::string loaded;
    dl_iterate_phdr(find_loaded_rccl, &loaded);
    if (!loaded.empty()) h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(MCI_ERR_COMM, "cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void **, int, Id128, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(MCI_ERR_COMM, "librccl.so lacks the nccl* entry points");
    g_rccl.h = h;
    return MCI_OK;
}

} // namespace

struct mci_ctx {
    int device = -1;
    bool offline = false; // compile-only context (no GPU): lets build() pre-fill the kernel cache
    hipStream_t stream = nullptr;
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    long long collectives = 0, last_count = 0; // ncclAllReduce calls issued on this context so far | elements of the last one (mci_comm_collectives)
    // The parked stream of a many-grid :vegas problem (GBs) outlives the problem: destroying it hands the buffer to the context, the
    // next problem that needs one takes it.  The driver wipes VRAM on release, and a hipMalloc that lands on pages still being wiped
    // waits for them: a second engine right after a first one's 4.8 GB were freed took 380 ms for a 5 ms launch
    // (profiles/r06_other_configs.txt) -- the pattern of every sweep that builds a Configuration per call.  Freed by mci_ctx_destroy.
    std::mutex spare_mu;
    void *spare = nullptr;
    size_t spare_bytes = 0;
};

namespace {
// train! stages one leaf in LDS: train_lds_doubles(nbin) + nbin doubles in k_finish (~4.5 per bin; + the serial walk's slots where they fit) next to ~2 KiB of static LDS
// -> the largest grid one workgroup can refine
const int64_t kTrainLdsMax = 160 * 1024 - 4096;
const int kMaxLeafBins = 4400;
struct Leaf {
    int kind, pool, npts, nbin, adapt, eoff, doff, boff;
    double lower, upper, alpha;
    int width = 1; // x entries per slot: D for a FermiK leaf
};

// An owning, grow-only buffer of device memory (DevBuf) or pinned host memory (PinBuf): a pointer and its capacity in elements.
// reserve(n) does nothing while n fits; otherwise it frees FIRST and then allocates (the peak is the larger of the two sizes, never
// their sum), the old contents are gone, and a failed allocation leaves the buffer empty.  The destructor frees; a buffer that never
// reserved anything (every buffer of an offline problem) makes no HIP call.
template <class T, bool kPinned> struct Buf {
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }
    T *get() const { return ptr; }
    operator T *() const { return ptr; }
    int64_t capacity() const { return cap; }
    void reset() { adopt(nullptr, 0); }
    // takes over an allocation of `n` elements made elsewhere (the logs that keep their contents when they grow); frees its own
    void adopt(T *q, int64_t n) {
        if (ptr) (void)(kPinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = q;
        cap = n;
    }
    int reserve(int64_t n) {
        if (n <= cap) return MCI_OK;
        reset();
        void *q = nullptr;
        HIPCHK(kPinned ? hipHostMalloc(&q, (size_t)n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, (size_t)n * sizeof(T)));
        ptr = (T *)q;
        cap = n;
        return MCI_OK;
    }

  private:
    T *ptr = nullptr;
    int64_t cap = 0;
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// The owning handle of one loaded code object (DevBuf's counterpart for modules): the module, its main kernel, the kernel-cache file it
// came from and the workgroup size it was compiled for.  `compiled` is all an offline problem ever has.  What else decides whether a
// unit can be used as it is (the stratified unit's deterministic flag, a sweep unit's thread count, the persistent unit's background
// job) is its caller's to ask.
struct Candidate; // one hiprtc job (mci_host_jit.h)
struct KernelUnit {
    hipModule_t module = nullptr;
    hipFunction_t f = nullptr;
    bool compiled = false;
    std::string code_object;
    int threads = 0;
    // a code object from the kernel cache that does not load (truncated by a crash, foreign file)
    enum Stale { kRecompileOnce, kUnlinkAndFail, kFail };
    struct Rules {
        Stale stale;
        bool no_scratch;     // the main kernel must not use scratch either
        std::string refusal; // the message for static LDS (or scratch); empty: the sample kernels' own
        std::string what;    // "hipModuleLoadData failed for <what>"
    };
    // (mci_host_jit.h) the refusals, then -- unless the context is offline -- module, main kernel and its dynamic-LDS limit
    int load(const mci_ctx *ctx, Candidate &c, const char *kernel, int64_t lds, const Rules &rules);
    // another entry point of the same module, with the same limit
    int entry(hipFunction_t *out, const char *name, int64_t lds) const {
        HIPCHK(hipModuleGetFunction(out, module, name));
        if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)*out, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return MCI_OK;
    }
    void drop() {
        compiled = false;
        f = nullptr;
        if (module) (void)hipModuleUnload(module);
        module = nullptr;
    }
};
} // namespace

struct mci_problem {
    mci_ctx *ctx = nullptr;
    std::vector<Leaf> leaves;
    int npool = 0, ni = 0;
    std::vector<int> dof, maxdof, pool_leaf0, pool_nleaf;
    mcijit::ProblemShape shape;
    int nstat = 0;
    int64_t packed_n = 0;
    int64_t lds_bytes = 0;
    int64_t lds_bytes_k1 = 0; // split-all sample pass: fixed part + edge cache
    // host mirrors of the tables (uploaded at create / set_*)
    std::vector<double> h_edges, h_dacc, h_ddist, h_reweight, h_ud;
    // device
    DevBuf<double> d_edges, d_dacc, d_ddist, d_reweight, d_ud;
    DevBuf<double> d_part_cols, d_part_hist, d_ghist, d_stage1, d_packed;
    DevBuf<double> d_scratch, d_iterlog, d_dump;
    DevBuf<int> d_status;
    DevBuf<mci::LeafDev> d_leaves;
    // kernels
    // one code object per unit, JIT-compiled (or loaded from the kernel cache) the first time it is needed
    // kernel slots (kslot): :vegas for measurefreq == 1 | :vegasmc | :mcmc | :vegas for any measurefreq | sample dump
    //                      | :vegasmc with several lanes per chain | :mcmc with several lanes per chain (mci_spec.h)
    // behind them: the persistent :vegas unit (mci_set_persistent), the stratified one (mci_host_strat.h), the twelve sweep units (Sweep)
    // ... and the big :vegas unit (sixteen histogram copies, 1024 threads: mci_host_vegas_plan.h VegasBigUnit)
    // ... and the persistent :vegas unit with a target error (mci_persist_until.h; mci_integrate_until)
    enum { kSlots = 7, kPersist = kSlots, kStrat, kSweep, kVegasBig = kSweep + 12, kPersistUntil, kKernels };
    KernelUnit kernel[kKernels];
    VegasKernelPlan vegas; // which :vegas code object the launches run (mci_host_vegas_plan.h)
    VegasBigUnit vegas_big; // ... and whether big launches have a third one to run (kernel[kVegasBig])
    // Several lanes per chain (mci_spec.h, mci_set_chain_speculation): lanes -1 automatic (as many as the launch's chains leave idle),
    // 1 never, 2..64 forced; the acceptance the speculation tree is built for (<= 0: the solver's default) and the most accept edges
    // on a way through it (-1: the solver's default); the tree of the last such launch on the device
    int spec_lanes = -1, spec_maxacc = -1;
    double spec_accept = 0.0;
    DevBuf<mci::SpecNode> d_spec_tab;
    int spec_tab_lanes = 0, spec_tab_limit = -2, spec_tab_maxacc = 0;
    int spec_ntree = 0, spec_first = 0; // trees on the device, the one a group starts on
    float spec_accepts[8] = {};          // the acceptance each of them was built for
    double spec_tab_accept = -1.0;
    // A several-lanes-per-chain code object proves itself before it is trusted (mci_host_jit.h spec_self_check): until a code object has
    // reproduced the lane-per-chain kernel's packed sums on THIS device (a marker file next to it in the kernel cache remembers that it did),
    // its first launch is preceded by a two-block, 512-step run through both kernels.  [0] :vegasmc, [1] :mcmc --
    // spec_state: 0 not looked at yet, 1 verified, -1 the check failed (one lane per chain from now on), -2 the unit did not compile
    // (automatic lanes: one lane per chain from now on)
    int spec_state[2] = {0, 0};
    bool spec_need_check[2] = {false, false}; // the loaded code object has no marker yet
    bool in_self_check = false;
    // A :vegas code object proves itself too (mci_host_check.h vegas_self_check): the first launch through a classic single-tile sample
    // kernel without a marker is preceded by <= 2 blocks x <= 512 samples through it, and the packed buffer is compared with what the
    // static kernel k_check_vegas (mci_check.h) makes of the same samples.  [0] the measurefreq == 1 unit, [1] the any-cadence unit.
    // vegas_check_state: 0 not looked at, 1 verified, -1 fell back to the conservative layout, -2 no layout agreed
    // (the big unit goes through the same check; what it leaves is in vegas_big -- state, check_done -- and in flag bit 3)
    int vegas_check_state[2] = {0, 0};
    bool vegas_check_done[2] = {false, false}; // nothing left to decide for the loaded code object of that unit
    int vegas_check_flags = 0;                 // bit 0: observables not compared (user measure), bit 1: verified from a marker, bit 3: the big unit failed
    int check_slot = -1;                       // inside vegas_self_check: the kernel slot its launch goes through, whatever its cadence
    int64_t check_launches = 0;                // launches made for vegas_self_check so far (mci_debug_vegas_check_launches)
    int64_t last_discarded_neval = 0;              // evaluations of the warm-up launches the last mci_integrate ran again instead of counting
    int32_t last_discarded_launches = 0;
    static const int64_t kSpecFill = 65536;        // lanes a launch of few chains spreads over: one wave on each of the 1024 SIMDs
    std::vector<double> h_goal; // reweight_goal (main.jl:81); empty = none
    DevBuf<double> d_goal;
    int npa = 0;                    // 3 * (ni+1) * max(ni+1, npool): entries of config.propose (configuration.jl:185)
    DevBuf<double> d_part_pa;       // [rows][2*npa] per-workgroup propose | accept tables of the chain solvers
    DevBuf<unsigned long long> d_hold; // [64] :mcmc holding-time histogram of the last launch (this rank), see mci_get_hold_histogram
    // split vegas pass (NTILE > 1): per-sample histogram weights and 16-bit bins of the tiles >= 1
    double *d_tile_w = nullptr;      // (one allocation: the weights, then -- 256-byte aligned -- the packed bins)
    uint32_t *d_tile_bins = nullptr;
    size_t tile_bytes = 0;           // its size
    int64_t cap_tile = 0;
    int ntdraw = 0; // draws whose histogram lives in a tile >= 1
    int tdraw_words = 0; // 32-bit words of packed bins per parked sample (mci_device.h tdraw_words)
    hipFunction_t f_tiles[2] = {nullptr, nullptr}; // replay kernel of the two :vegas variants
    // second merge stage (partials -> packed), launched lazily: a single-rank mci_iteration_finish fuses it with
    // the refinement (k_finish); anything else that looks at `packed` first flushes it (k_finalize)
    mci::MergeArgs merge{};
    bool merge_pending = false;
    bool has_fermik = false; // FermiK variables: solver = :mcmc only
    // host integrand ("batch callback"): draws dumped SoA -> callback -> weights uploaded -> accumulate kernel
    mci_host_integrand_fn host_fn = nullptr;
    mci_host_integrand_idx_fn host_idx_fn = nullptr; // the `integrand(idx, var, config)` form (mcmc/montecarlo.jl:34-36)
    PinBuf<int32_t> h_hidx;                          // pinned: which integrand the host evaluates per chain (:mcmc)
    std::vector<double> h_tmp;                       // all-integrands <-> one-integrand adaptation of the two callback forms
    void *host_user = nullptr;
    DevBuf<double> d_hx, d_hw; // device
    PinBuf<double> h_hx, h_hw; // pinned host
    // chain state between the per-step launches of a chain solver with a host integrand (BatchArgs::HostStep)
    DevBuf<char> d_hstep; // (bytes)
    // host measure ("batch callback"): draws + relative weights of the launch -> host closure per block -> block observables
    mci_host_measure_fn hmeas_fn = nullptr;
    mci_host_measure_idx_fn hmeas_idx_fn = nullptr; // the `measure(idx, var, obs, relative_weight, config)` form (mcmc/montecarlo.jl:166-169)
    void *hmeas_user = nullptr;
    DevBuf<double> d_mx, d_mrelw, d_mobs;
    PinBuf<double> h_mx, h_mrelw;
    DevBuf<int32_t> d_midx;                         // chain solvers: the integrand index of every record (:mcmc), -1 = no record
    PinBuf<int32_t> h_midx;
    std::vector<double> h_mtmp;                     // callback form != record form: rows regrouped here
    std::vector<int32_t> h_mitmp;
    int threads = 256, wg_per_block = 0; // 0 = auto
    bool threads_explicit = false;       // mci_set_launch named a workgroup size
    int kernel_timing = -1;       // mci_set_kernel_timing
    // deterministic mode (mci_set_deterministic): every solver's kernel keeps one histogram / observable copy per wave; the workgroup
    // size each was compiled for (the largest of 512 / 256 / 128 / 64 threads whose copies fit the CU's LDS)
    bool deterministic = false;
    int threads_det[3] = {0, 0, 0};
    // refinement walk of train! (variable.jl:227-234): -1 automatic -- the reference's serial recurrence whenever the sample
    // launch before it is long enough to hide its ~14 us per iteration (>= kSerialWalkSamples samples or chain steps on this
    // rank: 1 % of the headline iteration), the prefix-scan form below that; mci_set_train_walk forces one
    int train_serial = -1;
    bool debug_wrong_decision = false; // csrc/mci_debug.h: the serial walk's slots with one planted wrong decision (TrainArgs::serial_walk == 3)
    static const int64_t kSerialWalkSamples = (int64_t)1 << 26;
    bool train_lds_raised = false; // k_train / k_finish allowed more than 64 KiB of dynamic LDS (large grids)
    // HIP events around the per-iteration ncclAllReduce (mci_comm_times_ms), recorded under the same rule as the sample launch's
    std::vector<hipEvent_t> cevs;
    bool cev_valid[64] = {};
    int64_t reduces = 0;
    static const int kCevRing = 64;
    // :mcmc automatic chain length: the holding-time histogram of launch k is copied to pinned host memory behind the launch (after
    // an all-reduce over the ranks, so that every rank sizes its chains from the SAME histogram) and is looked at when launch k + 1
    // is sized: the host waits for the sample kernel of launch k (not for its merge / train!, which run while launch k + 1 is
    // queued) -- ~10 us of idle queue per iteration, nothing next to a chain launch; the lag is fixed, so a run is reproducible
    PinBuf<unsigned long long> h_hold;      // pinned [64]
    PinBuf<double> h_hold_d;                // pinned [64]: the histogram summed over the ranks, as it comes out of the packed all-reduce
    hipEvent_t hold_ev = nullptr;           // (the values of the hand-over: launch.hold_*)
    // per-block means of the chain solvers' iterations (MergeArgs::block_means): rows [launch.blk_rows][launch.blk_stride = local blocks * nobs];
    // what the block-lineage error of a run of carried chains is computed from (mci_lineage_sums)
    DevBuf<double> d_blocklog;
    // Carried chains (BatchArgs::carry_x): end configurations of the last chain launch, two buffers (read one, write the other),
    // and what that launch was (launch.chain_*) -- an iteration continues it when it is the NEXT iteration of the same solver over the same blocks
    DevBuf<double> d_chain_x[2];
    DevBuf<double> d_chain_P[2];               // :vegasmc: the target density at every stored configuration (BatchArgs::store_P)
    DevBuf<double> d_carry_w;                  // :vegasmc: new target / old target of the stored chains (mci_vegasmc_carry_weights)
    hipFunction_t f_carryw[2] = {nullptr, nullptr}; // that kernel in the lane-per-chain | several-lanes-per-chain code object of :vegasmc
    DevBuf<int> d_chain_curr[2];
    // chains the buffers of that side are laid out for: the stride of d_chain_x (BatchArgs::carry_cap / store_cap)
    int64_t chain_stride(int b) const { return d_chain_curr[b].capacity(); }
    int chain_carry = -1;        // mci_set_chain_carry: -1 automatic / 1 (the rule above), 0 never
    // :vegasmc chains are carried only out of a launch that ran on a map train! had refined at least once: chains of the automatic
    // length have not reached their target on the UNTRAINED map of a heavy-tailed integrand (log(x)/sqrt(x): the first iteration of a cold
    // call is 14 sigma per run off), and a population that is no sample of the old target cannot be resampled into one of the new --
    // carried out of iteration 1 the second iteration was 4 sigma per run-iteration off, started afresh 1.2 (profiles/r05_bias.txt A4)
    int64_t ntrain = 0;                   // train! steps of this problem so far (launch.chain_ntrain: ... when the stored chains were launched)
    bool launch_counted = false;          // mci_integrate | mci_set_iteration_counted: the iteration being launched enters the final estimate (it >= ignore)
    // :mcmc: the reweight factors the stored chains ran under, and which stored chain every chain of the launch in flight continues
    // (k_resample_chains: the stored chains resampled to the target doReweight! has moved since)
    DevBuf<double> d_reweight_used, d_carry_W;
    DevBuf<int> d_carry_src;
    // the event ring of the sample launches (launch.launches, launch.ev_valid / clock_valid)
    DevBuf<unsigned long long> d_clocks;    // [kEvRing][2] shader-clock | reference-clock ticks of the timed :vegas launches' sample loops
    std::vector<hipEvent_t> evs; // ring of (start, stop) pairs around the sampling kernel, one pair per launch
    static const int kEvRing = 512;
    int log_row = 0;
    PinBuf<double> h_log;     // pinned: mci_integrate's read-back of the iteration log (+ the status word behind it)
    // persistent :vegas iterations (mci_train.h vegas_persist; mci_set_persistent): its own code object (kernel[kPersist]) -- the plain
    // layout at `threads` -- and the two grid-wide counters, which only grow (the host keeps their values)
    bool persist_failed = false;
    // its translation unit takes twice as long to compile as the plain sample kernel (train! comes with it): in automatic mode a code
    // object that is not in the kernel cache is compiled on a thread of its own while the calls go through the launch chain
    struct PersistJob;
    PersistJob *persist_job[2] = {nullptr, nullptr}; // [0] the fixed unit's, [1] the one with a target error
    DevBuf<unsigned long long> d_persist;    // [0] arrived | done << 40, [2] gave up, [3] the turn count a launch with a target stopped at (mci_persist_until.h)
    DevBuf<double> d_persist_sums;           // [2 nobs]: the running sums of that launch's rule
    DevBuf<double> d_edges_backup;           // the map a persistent launch started from (restored when it stalls)
    unsigned long long persist_arrive = 0, persist_done = 0;
    unsigned long long persist_spin_ticks = 200000000ull; // ticks of the 100 MHz wall clock a grid-wide wait may take: 2 s (mci_debug_persist_spin_ticks)
    int persistent = -1;          // -1 automatic (launch-bound :vegas calls of mci_integrate), 0 never, 1 whenever the layout allows
    bool last_persistent = false; // the last mci_integrate ran as one persistent launch
    static const int kGroups = mci::kMergeGroups;
    // Cursor hand-out of big :vegas launches (mci_device.h, the cursor section; mci_iteration_run).  NOT in LaunchState: a self-check
    // never launches through the cursor, and what the device words hold is not rolled back with the host's record.
    static const int kCursorLog2Big = 4, kCursorOnes = 4; // ranges of 16 units, tapering over 8, 4, 2 to 4 single units per wave
    DevBuf<unsigned long long> d_cursor;    // [blocks * kCursorStride]
    int64_t cursor_nblocks = 0;
    unsigned long long cursor_base = 0;     // what the words of blocks 0 .. cursor_nblocks - 1 hold when the queued launches are through
    hipFunction_t cursor_occ_f = nullptr;   // the occupancy query's last answer, and what it was asked about
    int cursor_occ_threads = 0, cursor_occ_resident = 0;
    int64_t cursor_occ_lds = 0;
    static const int64_t kChainFill = 131072; // chains per GPU that keep 2 waves on each of the 1024 SIMDs
    // automatic :mcmc chain lengths (mci_mcmc_auto_chains): measured steps per chain while nothing has been measured | how much longer
    // than the chains that measured the holds a launch's chains may be.  (MCI_MCMC_PILOT / MCI_MCMC_GROW: experiment knobs)
    static int64_t kMcmcPilotSteps, kMcmcGrow;
    static int64_t kMcmcCarryHolds, kMcmcCarryHalfFloors; // carried chains: length in longest holds | minimum length in HALF burn-in floors
    // What a sample launch leaves behind on the host (mci_iteration_run and the functions it calls write it).  VALUES ONLY -- no
    // pointer, capacity, handle or module: spec_self_check copies the record out before its two small launches and back after them,
    // and those launches may create or grow buffers (every d_* / h_* is a DevBuf / PinBuf, which cannot be copied).  Outside it:
    //   resources the check may create -- evs, the kernel units, what describes the speculation trees on the device
    //     (spec_tab_*, spec_ntree, spec_first, spec_accepts);
    //   settings -- spec_lanes, kernel_timing, chain_carry, threads*, ...;
    //   the check's own result -- spec_state, spec_need_check, in_self_check, vegas_check_*, vegas.conservative, check_*;
    //   the merge hand-off -- merge, merge_pending (mci_get_packed flushes it inside the check);
    //   per-call results of mci_integrate -- last_discarded_*, last_persistent, launch_counted, log_row;
    //   the reduce's bookkeeping -- reduces, cev_valid[] (mci_iteration_reduce alone writes them; the check does not reduce).
    struct LaunchState {
        // the last sample launch on this rank
        int last_wg = 0, last_threads = 0, last_nblocks = 0;
        int64_t last_samples = 0;                      // samples (vegas) or chain steps
        int64_t last_nchain = 0;                       // chains per block of the last chain-solver launch
        int last_spec_lanes = 1, last_spec_maxacc = 0; // of the last chain launch (1: one lane per chain)
        bool last_carried = false;                     // the last chain launch continued the one before it
        bool last_cursor = false;                      // the last sample launch handed its ranges out by cursor (mci_debug_vegas_cursor)
        bool last_vegas_big = false;                   // the last :vegas launch ran the big unit (what the reporting calls describe)
        int64_t last_split_chunks = 0, last_split_bytes = 0; // chunks of the last many-grid :vegas launch | bytes of parked stream it held at a time
        // the event ring (evs, d_clocks): sample launches so far, and per slot what its launch left there
        int64_t launches = 0;
        bool time_this_launch = true;
        bool ev_valid[kEvRing] = {};    // the launch of that slot recorded its events
        bool clock_valid[kEvRing] = {}; // ... and stamped its shader clock (timed one-tile :vegas launches only, mci_kernel_clocks)
        // the stored chains (d_chain_x / curr / P): what the launch that wrote them was
        int chain_cur = 0;              // buffer the last launch wrote
        bool chain_valid = false;
        int chain_solver = -1, chain_iteration = -1;
        int64_t chain_lo = 0, chain_hi = 0, chain_nchain = 0;
        int64_t chain_ntrain = 0;       // ntrain when they were launched
        // the block log (d_blocklog): rows logged, their stride and first block
        int64_t blk_rows = 0, blk_stride = 0, blk_lo = -1;
        int blk_carried = 0;            // rows of the log whose launch continued the chains of the one before
        // the :mcmc holding-time hand-over (d_hold -> h_hold / h_hold_d, hold_ev)
        int64_t hold_max = 0;                   // upper edge of the top occupied bucket of the last histogram taken in; 0: none yet
        int64_t hold_len = 0;                   // measured steps per chain of the launch `hold_max` comes from
        int64_t hold_prev = 0;                  // hold_max of the launch before that, once warm
        bool hold_valid = false;                // the launch `hold_max` comes from was long enough for its own holds
        bool hold_measured = false;             // the last :mcmc launch measured its holding times at all (not with a host integrand)
        // Warm-up of the automatic :mcmc chain length: until a launch has run chains long enough for the holds IT measured
        // (mcmc_launch_valid), lengths escalate and mci_integrate repeats an iteration instead of counting it; afterwards a launch is
        // sized from the larger of the last two launches' holds (the longest hold of a launch is an extreme value: it moves by a bucket
        // from launch to launch) and nothing is ever repeated or left out again (no selection on what an iteration measured)
        bool mcmc_warm = false;
        bool hold_inflight = false;             // a histogram is on its way to the host (hold_ev)
        bool hold_from_packed = false;          // ... the summed one (h_hold_d), not this rank's own (h_hold)
        bool hold_deferred = false;             // a communicator is set: the launch's histogram is published behind its packed all-reduce
        bool hold_ext_pending = false;          // no communicator: this rank's counts were published; an external reducer may still sum them (mci_external_reduce_done)
        int64_t hold_launches = 0;              // :mcmc launches that recorded a histogram
        int64_t hold_len_inflight = 0;          // measured steps per chain of the launch whose histogram is in flight
        bool hold_carried_inflight = false;     // that launch continued the chains of the one before (kMcmcCarryHolds x its holds instead of 16 x)
    } launch;
    static_assert(std::is_trivially_copyable<LaunchState>::value, "the launch record holds values only");
    // Stratified :vegas (VEGAS+, mci_set_stratification; mci_strat.h, mci_host_strat.h).  Not part of `config`: a problem keeps the map
    // it trained; the allocation starts uniform in every mci_integrate call unless the problem carries it (mci_set_stratification_carry).
    struct Strat {
        bool on = false;
        std::vector<int> want;        // nstrat the caller asked for, empty = the default plan (mci_strat_plan)
        double beta = 0.75;
        int64_t max_nhcube = (int64_t)1 << 24;
        std::vector<int> nstrat;      // the plan in use (for nsamp samples per iteration), empty = none yet
        int64_t ncube = 0, nsamp = 0;
        DevBuf<long long> d_off;      // [ncube + 1] offsets of the allocation the last run used; the next run overwrites them first
        bool ran = false;             // d_off is the allocation a run of this plan used (mci_get_strat_counts)
        bool alloc_valid = false;     // d_off holds an allocation for this plan (else the next run starts uniform)
        bool alloc_pending = false;   // the next run first turns the d_h the last iteration measured into d_off (adapt)
        DevBuf<double> d_d;           // [ncube] d_h of the next allocation
        // Carry (mci_set_stratification_carry): the d_h of the last finished iteration, or of a state file, with the plan and the beta it
        // was measured under.  c_host empty: the values are d_d's (c_nstrat is then the plan d_d is laid out for); else they wait here
        // for the next run (mci_load_state).  Kept up to date whether or not `carry` is on; consulted only when it is.
        bool carry = false;
        bool c_valid = false;
        std::vector<int> c_nstrat;
        int64_t c_ncube = 0;
        double c_beta = 0.0;
        std::vector<double> c_host;
        int carry_how = 0;            // the last start of an allocation: 0 uniform | 1 from the carried d_h on its own plan | 2 remapped
        DevBuf<double> d_tsum;        // k_strat_alloc scratch
        DevBuf<double> d_part, d_rec_s, d_stat;
        DevBuf<long long> d_rec_h;
        int64_t last_nchunk = 0;
        bool last_run = false;        // the last mci_iteration_run was stratified: mci_iteration_finish reduces it
        int compiled_det = -1;        // the deterministic flag kernel[kStrat] was compiled under
        // test hook (mci_debug_strat_dump): host buffers the next stratified run fills
        double *hx = nullptr, *hy = nullptr, *hjac = nullptr, *hw = nullptr;
        long long *hh = nullptr;
        int64_t hn = 0;
        // test hook (mci_debug_strat_start_d): host buffer the next start of an allocation copies the d_h it allocates from into
        double *hstart = nullptr;
        int64_t hstart_n = 0;
    } strat;
    // Batched parameter sweeps (mci_integrate_sweep, mci_integrate_sweep_strat, mci_integrate_sweep_chains, mci_integrate_sweep_mcmc, mci_integrate_sweep_until; mci_host_sweep.h): the twelve sweep units are
    // kernel[kSweep + which].  A sweep keeps nothing else here: its maps, logs and status words come in and go out through the call's arguments.
    struct Sweep {
        // mci_sweep.h (one Continuous grid) | mci_sweep_leaves.h (any mix of Continuous and Discrete leaves) | mci_sweep_strat.h
        // (stratified points) | mci_sweep_chains.h (:vegasmc points | :mcmc points, fresh | carried chains) | mci_sweep_strat_leaves.h
        // (stratified points, several Continuous leaves) | mci_sweep.h, mci_sweep_leaves.h again (a target error per point:
        // mci_integrate_sweep_until) | mci_sweep_chains.h again (carried chains that go on from the call before:
        // mci_integrate_sweep_chains_resume | mci_integrate_sweep_mcmc_resume): mci_host_sweep.h kSweepUnits describes them in this order
        enum { kOne = 0, kLeaves = 1, kStrat = 2, kChains = 3, kMcmc = 4, kChainsCarry = 5, kMcmcCarry = 6, kStratLeaves = 7, kUntil = 8, kLeavesUntil = 9, kChainsResume = 10, kMcmcResume = 11, kUnits = 12 };
        int grid = 0;                 // csrc/mci_debug.h mci_debug_sweep_workgroups: workgroups of the next sweeps, 0 = the default
        int want_threads = 0;         // ... mci_debug_sweep_threads: 256 | 512 | 1024, 0 = the default (the one-grid unit only)
        int last_grid = 0, last_threads = 0;
        // mci_set_sweep_leaves: MCI_SWEEP_ONE_GRID (a sweep point refines ONE Continuous grid, unit kOne) or MCI_SWEEP_ALL_LEAVES
        // (a problem that is no one-grid layout runs unit kLeaves)
        int leaves_mode = 0;
        // mci_set_sweep_chain_carry: 1 = a :vegasmc | :mcmc sweep point's iterations continue the chains of the one before (units
        // kChainsCarry | kMcmcCarry instead of kChains | kMcmc)
        int chain_carry = 0;
        // mci_set_sweep_strat_leaves: MCI_SWEEP_ALL_LEAVES = a stratified problem of several Continuous leaves runs unit kStratLeaves
        // (an opt-in of its own: leaves_mode does not reach the stratified query)
        int strat_leaves_mode = 0;
    } sweep;
    KernelUnit &sweep_unit(int which) { return kernel[kSweep + which]; }
    static_assert(kVegasBig == kSweep + Sweep::kUnits, "one handle per sweep unit");
};

// The twelve sweep units, in the order of mci_problem::Sweep::unit: everything that tells them apart when they are compiled, loaded and
// named (mci_host_sweep.h compile_sweep_unit; mci_host_jit.h mci_compile_solver, mci_kernel_code_object).  The headers, the kernel symbol
// and the #defines are the JIT unit's row (mci_jit.h kUnits).
struct SweepUnitDesc {
    int jit_unit;         // mcijit::kUnit*
    int32_t solver;       // MCI_VEGAS_SWEEP* | MCI_VEGASMC_SWEEP | MCI_MCMC_SWEEP: the unit's name for mci_compile_solver / mci_kernel_code_object
    int32_t runs;         // the solver its source is generated for (mci_jit.h generate_source)
    const char *tag;      // in messages: "... (sweep kernel, <tag>)", "... code object (<tag>)"
    const char *for_what; // in messages: "the sweep kernel<for_what> ..."
    bool alpha;           // compiled for the one leaf's learning rate (MCI_TRAIN_POWER)
    bool want_threads;    // mci_debug_sweep_threads applies
};
static const SweepUnitDesc kSweepUnits[mci_problem::Sweep::kUnits] = {
    {mcijit::kUnitSweep, MCI_VEGAS_SWEEP, MCI_VEGAS, "", "", true, true},
    {mcijit::kUnitSweepLeaves, MCI_VEGAS_SWEEP_LEAVES, MCI_VEGAS, "several leaves", " for several leaves", false, false},
    {mcijit::kUnitSweepStrat, MCI_VEGAS_SWEEP_STRAT, MCI_VEGAS, "stratified points", " for stratified points", true, false},
    {mcijit::kUnitSweepChains, MCI_VEGASMC_SWEEP, MCI_VEGASMC, ":vegasmc points", " for :vegasmc points", false, false},
    {mcijit::kUnitSweepMcmc, MCI_MCMC_SWEEP, MCI_MCMC, ":mcmc points", " for :mcmc points", false, false},
    {mcijit::kUnitSweepChainsCarry, MCI_VEGASMC_SWEEP_CARRY, MCI_VEGASMC, ":vegasmc points, carried chains", " for :vegasmc points with carried chains", false, false},
    {mcijit::kUnitSweepMcmcCarry, MCI_MCMC_SWEEP_CARRY, MCI_MCMC, ":mcmc points, carried chains", " for :mcmc points with carried chains", false, false},
    {mcijit::kUnitSweepStratLeaves, MCI_VEGAS_SWEEP_STRAT_LEAVES, MCI_VEGAS, "stratified points, several leaves", " for stratified points with several leaves", false, false},
    {mcijit::kUnitSweepUntil, MCI_VEGAS_SWEEP_UNTIL, MCI_VEGAS, "a target error per point", " with a target error per point", true, false},
    {mcijit::kUnitSweepLeavesUntil, MCI_VEGAS_SWEEP_LEAVES_UNTIL, MCI_VEGAS, "several leaves, a target error per point", " for several leaves with a target error per point", false, false},
    {mcijit::kUnitSweepChainsResume, MCI_VEGASMC_SWEEP_RESUME, MCI_VEGASMC, ":vegasmc points, chains of the call before", " for :vegasmc points that continue the chains of the call before", false, false},
    {mcijit::kUnitSweepMcmcResume, MCI_MCMC_SWEEP_RESUME, MCI_MCMC, ":mcmc points, chains of the call before", " for :mcmc points that continue the chains of the call before", false, false},
};
static int sweep_unit_of(int32_t solver) {
    for (int w = 0; w < mci_problem::Sweep::kUnits; ++w)
        if (kSweepUnits[w].solver == solver) return w;
    return -1;
}

// A repeated iteration (the warm-up of automatic :mcmc chain lengths, mci_integrate) draws from the Philox streams of iteration
// i + kRepeatStride * attempt: the iteration index has 17 bits (DESIGN.md "RNG streams"), runs of fewer than 16384 iterations leave the upper ones free
static const int kRepeatStride = 16384, kMaxRepeats = 7;

// (process-wide; csrc/mci_debug.h mci_debug_mcmc_policy moves them for A/B campaigns -- tools/mcmc_policy.py, profiles/r04_mcmc_policy.txt)
int64_t mci_problem::kMcmcPilotSteps = 4096;
int64_t mci_problem::kMcmcGrow = 2;
int64_t mci_problem::kMcmcCarryHolds = 4;
int64_t mci_problem::kMcmcCarryHalfFloors = 2;

// Layout decisions of mci_problem_create that tests and A/B tools force (csrc/mci_debug.h mci_debug_override): process-wide, consulted
// by the NEXT mci_problem_create.  The library itself reads two environment variables and no others: MCI_KERNEL_CACHE (where code objects
// are cached) and MCI_JIT_FLAGS (extra hiprtc options), mci_jit.h.
namespace {
struct Override { bool on = false; int64_t v = 0; };
struct Overrides { Override table_mode, hist_tile_bins, no_split_all, l1_phase, train_walk, hist_copies, fresh_floors, fresh_burnin_pct, spec_self_check, split_chunk, vegas_self_check, vegas_cursor, cursor_log2_big, cursor_ones, vegas_big_unit; } g_over;
Override *override_slot(const char *key) {
    if (!key) return nullptr;
    if (!strcmp(key, "table_mode")) return &g_over.table_mode;
    if (!strcmp(key, "hist_tile_bins")) return &g_over.hist_tile_bins;
    if (!strcmp(key, "no_split_all")) return &g_over.no_split_all;
    if (!strcmp(key, "l1_phase")) return &g_over.l1_phase;
    if (!strcmp(key, "train_walk")) return &g_over.train_walk;
    if (!strcmp(key, "hist_copies")) return &g_over.hist_copies;
    if (!strcmp(key, "fresh_floors")) return &g_over.fresh_floors;
    if (!strcmp(key, "fresh_burnin_pct")) return &g_over.fresh_burnin_pct;
    if (!strcmp(key, "spec_self_check")) return &g_over.spec_self_check;
    if (!strcmp(key, "split_chunk")) return &g_over.split_chunk;
    if (!strcmp(key, "vegas_self_check")) return &g_over.vegas_self_check;
    if (!strcmp(key, "vegas_cursor")) return &g_over.vegas_cursor;
    if (!strcmp(key, "cursor_log2_big")) return &g_over.cursor_log2_big;
    if (!strcmp(key, "cursor_ones")) return &g_over.cursor_ones;
    if (!strcmp(key, "vegas_big_unit")) return &g_over.vegas_big_unit;
    return nullptr;
}
} // namespace

static void persist_job_drop(mci_problem *p);
namespace { void persist_orphans_join(); }
// counters [0..2] of the persistent :vegas kernel + (MCI_PERSIST_TRACE builds) the phase stamps of three workgroups over eight turns
static const size_t kPersistWords = 8 + 3 * 8 * 8 + 16;
static const size_t kPersistCtrWords = 4; // the words that are reset together: counters, gave-up flag, stop word

namespace {

// the parked stream's buffer: from the context's spare one if that is big enough (and not more than twice as big), else hipMalloc
int tile_alloc(mci_problem *p, size_t bytes) {
    mci_ctx *c = p->ctx;
    void *base = nullptr;
    {
        std::lock_guard<std::mutex> g(c->spare_mu);
        if (c->spare && c->spare_bytes >= bytes && c->spare_bytes <= 2 * bytes + ((size_t)64 << 20)) {
            base = c->spare;
            p->tile_bytes = c->spare_bytes;
            c->spare = nullptr;
            c->spare_bytes = 0;
        }
    }
    if (!base) {
        HIPCHK(hipMalloc(&base, bytes));
        p->tile_bytes = bytes;
    }
    p->d_tile_w = (double *)base;
    return MCI_OK;
}
// ... and back: the context keeps the largest buffer it has been handed (work queued on the context's one stream is ordered behind
// the kernels that used it), anything else is freed
void tile_release(mci_problem *p) {
    if (!p->d_tile_w) return;
    mci_ctx *c = p->ctx;
    void *drop = p->d_tile_w;
    {
        std::lock_guard<std::mutex> g(c->spare_mu);
        if (p->tile_bytes > c->spare_bytes) {
            drop = c->spare;
            c->spare = p->d_tile_w;
            c->spare_bytes = p->tile_bytes;
        }
    }
    if (drop) (void)hipFree(drop);
    p->d_tile_w = nullptr;
    p->d_tile_bins = nullptr;
    p->tile_bytes = 0;
    p->cap_tile = 0;
}

int upload(mci_problem *p) {
    if (p->ctx->offline) return MCI_OK;
    auto up = [&](DevBuf<double> &d, const std::vector<double> &h) -> int {
        if (!d) // (sized once: the tables keep their sizes)
            if (int rc = d.reserve(h.size() ? h.size() : 1)) return rc;
        if (h.size()) HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream));
        return MCI_OK;
    };
    int rc;
    if ((rc = up(p->d_edges, p->h_edges))) return rc;
    if ((rc = up(p->d_dacc, p->h_dacc))) return rc;
    if ((rc = up(p->d_ddist, p->h_ddist))) return rc;
    if ((rc = up(p->d_reweight, p->h_reweight))) return rc;
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    return MCI_OK;
}

int ensure_capacity(mci_problem *p, int64_t nwg, int64_t nblocks) {
    const auto &s = p->shape;
    int rc = p->d_part_cols.reserve(nwg * s.ncols);
    if (!rc && (s.table_mode == 0 || s.table_mode == 3)) rc = p->d_part_hist.reserve(nwg * (s.nbin ? s.nbin : 1));
    if (!rc) rc = p->d_scratch.reserve(nblocks * s.ncols);
    return rc;
}

// ---- the argument structs of the launches: each filled from the problem in ONE place; a caller then sets only what differs ----------
// the map and the distributions (BatchArgs, DumpArgs, CheckArgs, TrainArgs)
template <class Args> void fill_tables(const mci_problem *p, Args &a) {
    a.edges = p->d_edges;
    a.dacc = p->d_dacc;
    a.ddist = p->d_ddist;
}
// ... with the reweight factors, the userdata and where a sample launch leaves its sums (where it reports -- BatchArgs::status -- is
// the caller's: the problem's word, a sweep point's own, none for the carry-weights launch)
void fill_batch(const mci_problem *p, mci::BatchArgs &a) {
    fill_tables(p, a);
    a.reweight = p->d_reweight;
    a.ud = p->d_ud;
    a.part_cols = p->d_part_cols;
    a.part_hist = p->d_part_hist;
    a.ghist = p->d_ghist;
}
// the merge of nrows partial rows, wpb per block, into `packed`: a :vegas launch whose histogram rows went through k_hist_stage1
// (use_ghist = 0, no propose | accept tables, no block means, no holding times, the clearStatistics! offsets in place)
mci::MergeArgs merge_args(const mci_problem *p, int64_t nblocks, int wpb, int64_t nrows) {
    const auto &s = p->shape;
    mci::MergeArgs m{};
    m.part_cols = p->d_part_cols;
    m.ncols = s.ncols;
    m.nobs = s.nobs;
    m.ni = s.ni;
    m.nblocks = (int)nblocks;
    m.wg_per_block = wpb;
    m.stage1 = p->d_stage1;
    m.ngroup = (int)mci_problem::kGroups;
    m.ghist = p->d_ghist;
    m.nbin = s.nbin;
    m.packed = p->d_packed;
    m.status = p->d_status;
    m.scratch = p->d_scratch;
    m.npa = p->npa;
    m.nrows = (int)nrows;
    return m;
}
// The launch geometry of the merge kernels (mci_static_kernels.h), in ONE place: the product's launches (queue_merge, strat_run,
// flush_merge, launch_train) and the test hook mci_debug_merge both ask here, so that the hook runs the kernels as the product does.
dim3 hist_stage1_grid(int nbin) { return dim3((unsigned)((nbin + 255) / 256), (unsigned)mci_problem::kGroups); }
dim3 finalize_grid(int nbin, int npa) { return dim3((unsigned)((nbin + 255) / 256 + 1 + (2 * npa + 3) / 4)); } // histogram | statistics | merge_pa
dim3 finish_grid(int nleaf, int npa) { return dim3((unsigned)(nleaf + 1 + (2 * npa + 3) / 4)); }               // leaves | statistics | merge_pa
// two bins per thread for the default 999-bin grids: the rescale (a pow and a log per bin) and the second merge stage are the
// latency chains of a lone workgroup; with four bins per thread (256 threads) a launch-bound iteration took 24.7 us, with two
// 22.2, with one (1024 threads) 22.3 (tools/latency.py, neval = 1e4)
unsigned train_threads(int maxn) { return maxn > 256 ? 512u : 256u; }
// dynamic LDS of k_train | k_finish for a largest leaf of maxn bins: d | sg | wa (train_leaf) | the serial walk's slots and their record,
// where they fit (grids of up to ~2700 increments; *spare = 1), else k_finish's merged histogram alone
size_t train_lds_bytes(int maxn, int *spare) {
    *spare = (size_t)(mci::train_lds_doubles(maxn) + mci::train_spare_doubles(maxn)) * sizeof(double) <= (size_t)kTrainLdsMax ? 1 : 0;
    return (size_t)(mci::train_lds_doubles(maxn) + (*spare ? mci::train_spare_doubles(maxn) : maxn)) * sizeof(double);
}
int max_leaf_bins(const mci_problem *p) {
    int maxn = 1;
    for (auto &L : p->leaves) maxn = L.nbin > maxn ? L.nbin : maxn;
    return maxn;
}
// the problem-wide part of train!'s arguments (what to do, the walk, the log row and the LDS plan are the caller's)
void fill_train(const mci_problem *p, mci::TrainArgs &t) {
    fill_tables(p, t);
    t.leaves = p->d_leaves;
    t.nleaf = p->shape.nleaf;
    t.packed = p->d_packed;
    t.nstat = p->nstat;
    t.reweight = p->d_reweight;
    t.nd = p->shape.ni + 1;
    t.status = p->d_status;
}
// the geometry of the sample launch just queued (mci_kernel_times_ms; launch_train picks train!'s walk by last_samples)
void record_launch(mci_problem *p, int64_t samples, int64_t nwg, int threads, int64_t nblocks) {
    p->launch.last_samples = samples;
    p->launch.last_wg = (int)nwg;
    p->launch.last_threads = threads;
    p->launch.last_nblocks = (int)nblocks;
}

int check_status(mci_problem *p) {
    int st = 0;
    HIPCHK(hipMemcpyAsync(&st, p->d_status, sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    if (!st) return MCI_OK;
    HIPCHK(hipMemsetAsync(p->d_status, 0, sizeof(int), p->ctx->stream));
    if (st & mci::ST_PERSIST_STALL) { // a grid-wide wait of the persistent :vegas launch ran out of time: its counters are void
        // (mci_integrate recovers by itself and never gets here with this bit; this is the message of a stall somebody else finds)
        HIPCHK(hipMemsetAsync(p->d_persist, 0, kPersistCtrWords * sizeof(unsigned long long), p->ctx->stream));
        HIPCHK(hipMemsetAsync(p->d_ghist, 0, 3 * (size_t)(p->shape.nbin ? p->shape.nbin : 1) * sizeof(double), p->ctx->stream));
        p->persist_arrive = p->persist_done = 0;
        p->persist_failed = true; // (later calls take the launch-per-iteration path)
        return fail(MCI_ERR_HIP, "the persistent :vegas launch stalled (is the device shared with other long-running kernels?); "
                                 "the iterations of this call are void -- later calls launch per iteration (mci_set_persistent(prob, 0))");
    }
    if (st & mci::ST_MCMC_INIT) return fail(MCI_ERR_INVALID, "Cannot find the variables that makes the integrand nonzero!"); // mcmc/montecarlo.jl:126
    if (st & mci::ST_NORMALIZATION) return fail(MCI_ERR_NORMALIZATION, "Block normalization is not positively defined!");
    if (st & mci::ST_HIST_NONFINITE) return fail(MCI_ERR_HISTOGRAM, "histogram should be all finite");
    if (st & mci::ST_HIST_NONPOSITIVE) return fail(MCI_ERR_HISTOGRAM, "histogram should be all positive and non-zero");
    return fail(MCI_ERR_HISTOGRAM, "distribution is not all finite");
}

// after a stalled persistent :vegas launch: status word, grid-wide counters and the three histogram buffers back to their idle state
int persist_recover(mci_problem *p) {
    hipStream_t st = p->ctx->stream;
    HIPCHK(hipMemsetAsync(p->d_status, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(p->d_persist, 0, kPersistCtrWords * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(p->d_ghist, 0, 3 * (size_t)(p->shape.nbin ? p->shape.nbin : 1) * sizeof(double), st));
    p->persist_arrive = p->persist_done = 0;
    p->persist_failed = true; // (later calls take the launch-per-iteration path)
    p->merge_pending = false;
    return MCI_OK;
}

// :mcmc holding-time histogram of the launch just queued -> pinned host memory, behind the launch on the stream.  One process: this
// rank's counts, straight from the kernel's buffer (the host later waits for the sample kernel only).  With a communicator every rank
// must size its next chains from the SAME histogram: the 64 counts ride in the iteration's ONE all-reduce -- k_finalize appends them
// to `packed` as exact doubles (MergeArgs::hold), mci_iteration_reduce sums packed_n + 64 doubles and publishes the tail
// (hold_publish_reduced) -- so the launch only notes what it measured with.
int hold_publish(mci_problem *p, int64_t chain_len, bool carried) {
    hipStream_t st = p->ctx->stream;
    if (!p->h_hold) {
        int rc = p->h_hold.reserve(64);
        if (!rc) rc = p->h_hold_d.reserve(64);
        if (rc) return rc;
        HIPCHK(hipEventCreateWithFlags(&p->hold_ev, hipEventDisableTiming));
    }
    p->launch.hold_len_inflight = chain_len;
    p->launch.hold_carried_inflight = carried;
    p->launch.hold_launches += 1;
    if (p->ctx->comm) {
        p->launch.hold_deferred = true;
        return MCI_OK;
    }
    if (p->launch.hold_inflight) HIPCHK(hipEventSynchronize(p->hold_ev)); // (a histogram nobody looked at)
    HIPCHK(hipMemcpyAsync(p->h_hold, p->d_hold, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(p->hold_ev, st));
    p->launch.hold_inflight = true;
    p->launch.hold_from_packed = false;
    p->launch.hold_ext_pending = true;
    return MCI_OK;
}

// ... behind the all-reduce of `packed` (the library's, or an external reducer's: mci_external_reduce_done): the summed counts
int hold_publish_reduced(mci_problem *p) {
    hipStream_t st = p->ctx->stream;
    // (no wait for a copy still in flight -- this rank's own counts published behind the sample kernel when an external reducer sums the
    // packed buffer: the summed counts go to ANOTHER pinned buffer, and the event is simply recorded again behind them)
    HIPCHK(hipMemcpyAsync(p->h_hold_d, p->d_packed + p->packed_n, 64 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(p->hold_ev, st));
    p->launch.hold_inflight = true;
    p->launch.hold_from_packed = true;
    p->launch.hold_deferred = false;
    return MCI_OK;
}

// before an :mcmc launch with an automatic chain count is sized: take in the histogram of the launch before it.  The host waits for
// that launch's sample kernel here (its merge and train! are still running or queued: the next launch is queued behind them while they
// run); what the two-launch lag of the rounds before cost is in profiles/r03_c5_kernel_stats.txt (two more launches sized from the
// untrained map's holding times: 324 ms of a cold BASELINE configs[4] call).
int hold_consume(mci_problem *p) {
    if (!p->launch.hold_inflight) return MCI_OK;
    HIPCHK(hipEventSynchronize(p->hold_ev));
    p->launch.hold_inflight = false;
    int top = -1;
    for (int b = 0; b < 64; ++b)
        if (p->launch.hold_from_packed ? p->h_hold_d[b] > 0.5 : p->h_hold[b] != 0ull) top = b;
    if (top >= 0) {
        p->launch.hold_prev = p->launch.mcmc_warm ? p->launch.hold_max : 0;
        p->launch.hold_max = (int64_t)1 << top; // bucket b holds bit_width(h) == b, i.e. h < 2^b
        p->launch.hold_len = p->launch.hold_len_inflight;
        // was that launch long enough for what it measured itself?  (the rule its successor is sized by, mci_mcmc_auto_chains)
        p->launch.hold_valid = p->launch.hold_len >= (p->launch.hold_carried_inflight ? mci_problem::kMcmcCarryHolds : 16) * p->launch.hold_max;
        if (p->launch.hold_valid) p->launch.mcmc_warm = true;
    }
    return MCI_OK;
}

void drop_modules(mci_problem *p) {
    p->vegas.modules_dropped();
    p->vegas_big.modules_dropped();
    p->launch.last_vegas_big = false; // (the reporting calls describe the standing plan again)
    p->vegas_check_done[0] = p->vegas_check_done[1] = false; // (new code objects: they prove themselves again, or show their markers)
    p->cursor_occ_f = nullptr; // (the occupancy answer belonged to a kernel of the modules that go)
    for (KernelUnit &u : p->kernel) u.drop();
    p->persist_failed = false;
    persist_job_drop(p);
}

} // namespace

static int flush_merge(mci_problem *p);
static int comm_sum_host(mci_problem *p, double *v, int n);

// a log that keeps its rows when it grows: room for `need` rows of `width` doubles, doubling from `first` rows; the new buffer
// first, old -> new, then the old one goes (a copy and a stream synchronisation each time)
static int grow_keeping(mci_problem *p, DevBuf<double> &log, int64_t need, int64_t first, int64_t width) {
    const int64_t have = log.capacity() / width;
    if (need <= have) return MCI_OK;
    int64_t ncap = have ? have : first;
    while (ncap < need) ncap *= 2;
    double *n = nullptr;
    HIPCHK(hipMalloc((void **)&n, (size_t)ncap * width * sizeof(double)));
    if (log) {
        HIPCHK(hipMemcpyAsync(n, log, (size_t)have * width * sizeof(double), hipMemcpyDeviceToDevice, p->ctx->stream));
        HIPCHK(hipStreamSynchronize(p->ctx->stream));
    }
    log.adopt(n, ncap * width);
    return MCI_OK;
}

// room for `rows` rows of [blk_stride] doubles in the block log (grows with a copy and a stream synchronisation; mci_integrate reserves
// its iterations before the loop)
static int grow_block_log(mci_problem *p, int64_t rows) {
    const int64_t need = rows * p->launch.blk_stride;
    return grow_keeping(p, p->d_blocklog, need, 4096, 1);
}

