// cpk_plan.inl -- the launch plan of a batch: LaunchClass and plan_batch(), which decides every launch of a run, its
// kernels as forms of cpk_kernel_table.inl; cpk_device_upload (cpecan_kernels.hip) carries the plan out.
// Part of the single HIP translation unit cpecan_kernels.hip (included there, behind the kernels); not compiled on its own.

constexpr int kMaxClasses = CPK_WIDE_CLASSES + 6;  // wide classes + three packed ones, each of which may run as a split and a whole part

// One kernel launch of a run: the regions [regionBase, regionBase + regionCount) of the device order, which share one
// size class, with LDS, occupancy and per-wave scratch sized for the largest of THEM.
struct LaunchClass {
    bool packed = false;
    int k = 0;           // class index within its kind (wide 0..3, packed 0..2)
    // the kernel of the (first) launch and of the traceback launch of a two-launch class: split, fused, slots and the trace words are read off them
    KernelForm form, formTrace;
    KernelFn fn() const { return kernel_of(form); }
    KernelFn fnTrace() const { return kernel_of(formTrace); }
    CpkGeometry geo{};   // what the kernel reads: the scalar fields describe this class
    int waves = 0;       // workgroups of the launch (a gang: its waves, `gang` to a workgroup)
    // A reserved batch (model slots, KArgs::slotModels): the SLOTS build of the kernel, and the workgroups of a run with
    // t models, 1 <= t <= the reserved count -- `waves` is the most of them, which the per-wave scratch is sized for
    bool slots() const { return form.slots; }
    int wavesFor[CPECAN_MAX_MODEL_SLOTS + 1] = {};
    int wavesWith(int nModels) const { return slots() && wavesFor[nModels] < waves ? wavesFor[nModels] : waves; }
    int threads = CPK_WAVE;  // threads per workgroup: one wave, or the waves of a team
    int64_t subSlots = 0;  // scratch slots: one per wave (sweep) or one per region group of a wave (packed)
    size_t ldsBytes = 0;
    size_t ldsBytesFwd = 0;  // split, two launches: the forward launch's own LDS size (no candidate ring)
    int regionBase = 0, regionCount = 0;
    // A SPLIT class (fewer regions than wave slots): launch 1 = forward sweeps of whole regions into per-REGION rings,
    // launch 2 = one queue item per (region, traceback segment); see kModeForward / kModeTrace in cpk_sweep.inl.
    bool split() const { return form.mode != kModeWhole; }
    bool fused() const { return form.mode == kModeFused; }  // split, as ONE launch: regions and their traceback items in one queue
    bool dense = false;  // the plan's decision: the three-state match kernels allocated for three waves per SIMD (WPS = 3)
    bool abs = false;    // LDS rows for sweeps over absolute positions (set_row_form; cpk_sweep.inl "Absolute-position sweeps"): the ABS of a split class's kernels
    int wavesTrace = 0;
    // Gangs (cpk_sweep.inl "GANG"): waves per workgroup of the forward and of the traceback launch of a two-launch class, 0: one
    // wave per workgroup.  `waves` / `wavesTrace` stay counts of WAVES -- whole gangs --, ldsBytes / ldsBytesFwd the LDS of one.
    int gang = 0, gangTrace = 0;
    int64_t itemBase = 0, itemCount = 0;  // its items in dItems
    // Chains (plan_chains): the forward launch sweeps the first chainFrom segments of a region, a chain item of the traceback
    // launch the later ones of each of the `chains` regions that have more.  0: the forward launch sweeps everything.
    int chainFrom = 0;
    int64_t chains = 0, chainedSegs = 0;  // (chainedSegs: the segments those chains cover)
    bool chainsNeedGang = false;  // its traceback launch is a gang, its forward launch is not: no chains for that alone (the class line says so)
    int64_t ringTotal = 0;                // doubles of all its regions' rings (ringEl is 0 then: nothing per slot)
    int64_t ringEl = 0, candEl = 0, refEl = 0, totEl = 0, bringEl = 0, grollEl = 0;  // elements per scratch slot
    int64_t oRing = 0, oCand = 0, oRef = 0, oTot = 0, oBring = 0, oGroll = 0, oExpect = 0;  // element offsets of the class
    // LDS bytes of the first launch: the forward launch of a two-launch class has a size of its own where the plan set one
    size_t firstLdsBytes() const { return gang_lds_bytes((split() && !fused() && ldsBytesFwd) ? ldsBytesFwd : ldsBytes, gang); }
    size_t traceLdsBytes() const { return gang_lds_bytes(ldsBytes, gangTrace); }
    // the LDS of a workgroup of n waves whose single wave takes waveLds: the tables once, the rest n times
    size_t gang_lds_bytes(size_t waveLds, int n) const {
        const size_t shared = sizeof(double) * lds_header_doubles(geo.emit);
        return n > 1 ? shared + (size_t)n * (waveLds - shared) : waveLds;
    }
    // workgroups and threads per workgroup of the two launches
    unsigned firstGrid(int nModels) const { return (unsigned)(gang > 1 ? (wavesWith(nModels) + gang - 1) / gang : wavesWith(nModels)); }
    unsigned firstThreads() const { return (unsigned)(gang > 1 ? gang * CPK_WAVE : threads); }
    unsigned traceGrid() const { return (unsigned)(gangTrace > 1 ? (wavesTrace + gangTrace - 1) / gangTrace : wavesTrace); }
    unsigned traceThreads() const { return (unsigned)(gangTrace > 1 ? gangTrace * CPK_WAVE : threads); }
    double slotBytes() const {
        return 8.0 * ringEl + (double)sizeof(Candidate) * candEl + 16.0 * refEl + 8.0 * totEl + 8.0 * bringEl + 8.0 * grollEl;
    }
};

// Doubles of the ring a split region keeps its forward values in.  The match emitter stores the match row of every
// diagonal and every state only where the traceback reads it back: diagonal 0, the refresh diagonals of the emitting
// segment (one in CPK_REFRESH_PERIOD) and the two diagonals a forward sweep would resume from -- the table builder lays
// the diagonals end to end with exactly that many doubles each (cpk_table_gather.inl); this is the upper bound it stays
// below.  (Every state of every cell, as the per-wave rings are sized, is 204 GB for BASELINE config B; this is 62.)
static int64_t split_ring_doubles(const CpkRegion &rg, int S) {
    const int64_t N = (int64_t)rg.lX + rg.lY;
    const int64_t fullDiags = N / CPK_REFRESH_PERIOD + 3 * (int64_t)rg.nSeg + 4;  // refresh points + two resume diagonals per segment
    // + one double of padding per diagonal (match rows start and end on even doubles); an even total keeps the next region's ring aligned
    return ((int64_t)rg.cells + (N + 1) + (int64_t)(S - 1) * rg.maxWidth * fullDiags + S + 1) & ~(int64_t)1;
}

// ------------------------------------------------------------------------------------------------
// The launch plan of a batch.  plan_batch() decides, from the batch's geometry and regions, the device's size and free
// memory (PlanDevice) and the planning knobs of the environment (PlanKnobs), the launches of a run: one LaunchClass per
// size class that has regions, with its kernels, form flags, wave counts, LDS and per-slot scratch sizes.  It touches no
// CpkDevice, allocates nothing on the device and queues nothing on a stream; cpk_device_upload carries the plan out.
// ------------------------------------------------------------------------------------------------
// One CU of the chip as the plan sees it (MI355X_MICROARCH.md: 512 VGPRs per lane per SIMD in granules of 8, 4 SIMDs,
// 32 waves, 160 KiB LDS)
constexpr size_t kCuLdsBytes = 160 * 1024;
constexpr size_t kLdsPathMaxBytes = 64 * 1024;  // a wave's LDS on the LDS path (rolling rows + symbols); wider classes roll in global memory
constexpr int kSimdVgprs = 512, kVgprGranule = 8, kSimdsPerCU = 4, kMaxWavesPerCU = 32;
constexpr size_t kThreeWpsLdsWaves = 9;  // a build for three waves per SIMD is tried where the class's LDS lets nine or more waves onto a CU

// A planning knob of the environment, read where it is constructed: unset, 0, or a value.
template <class T>
struct Knob {
    bool set = false;
    T v = 0;
    explicit Knob(const char *name) {
        const char *s = getenv(name);
        set = s != nullptr;
        if (s) v = std::is_floating_point<T>::value ? (T)atof(s) : (T)atoll(s);
    }
    bool off() const { return set && v == 0; }
    bool on() const { return set && v != 0; }
};
// Every environment variable the plan depends on.  Constructing one reads them all: once per upload (tests change them
// between batches), so that every decision of a plan sees the same values.
struct PlanKnobs {
    Knob<int> maxWavesPerCU{"CPECAN_MAX_WAVES_PER_CU"};  // caps the single-wave workgroups per CU (tuning / diagnostics)
    Knob<int> packedSplit{"CPECAN_PACKED_SPLIT"};  // =1 / 0 (tests, A/B runs): every region of every packed class runs split / none
    Knob<int64_t> packedSplitFrom{"CPECAN_PACKED_SPLIT_FROM"};  // =<diagonals>: the packed regions longer than that run split
    Knob<int> packedShare{"CPECAN_PACKED_SHARE"};  // =0: the packed launches never share the wave slots beside a live batch
    Knob<int> abs{"CPECAN_ABS"};  // =0: never the absolute-position sweeps (A/B runs, tests of the other form)
    Knob<int> absWindows{"CPECAN_ABS_WINDOWS"};  // =0: the absolute-position sweeps stage whole strings (diagnostics, tests)
    Knob<int> split{"CPECAN_SPLIT"};  // =1 / 0 (tests, diagnostics): wide classes always / never split; 2 / 1: the one-launch / two-launch form
    Knob<int> expInSweep{"CPECAN_EXP_INSWEEP"};  // =0 (tests, A/B runs): expectation events by the second pass everywhere; 2: inside the traceback whatever the LDS costs
    Knob<int> expOneGroup{"CPECAN_EXP_ONE_GROUP"};  // =0: always the expectation build for two groups per diagonal
    Knob<int> team{"CPECAN_TEAM"};  // =<cells> (tests, diagnostics): a team of waves from that band width; 0: never
    // (the match suite -- tests/match_cases.py -- sets CPECAN_DENSE, CPECAN_FUSED3, CPECAN_TRACE3 and CPECAN_FWD3 to reach every build of the match kernels for two and for three waves per SIMD)
    Knob<int> dense{"CPECAN_DENSE"};  // =1 / 0: the three-state kernels allocated for three waves per SIMD always / never
    Knob<int> fusedSpin{"CPECAN_FUSED_SPIN"};  // polls of a fused item for its region's forward values (tests force the retry with a few)
    Knob<int> fused3{"CPECAN_FUSED3"};  // =0: never the three-waves-per-SIMD build of the one-launch form
    Knob<int> trace3{"CPECAN_TRACE3"};  // =0: never the three-waves-per-SIMD build of the traceback launch
    Knob<int> fwd3{"CPECAN_FWD3"};  // =0: never the three-waves-per-SIMD build of the forward launch
    Knob<int> chain{"CPECAN_CHAIN"};  // =0: no chains; k >= 1 (tests): chains from segment k wherever both launches of a class are gangs
    Knob<int> gang{"CPECAN_GANG"};  // =0: never workgroups of several waves (gangs); n in 2..12: n waves per workgroup wherever the form allows it and n fit
    Knob<double> memBudgetMb{"CPECAN_MEM_BUDGET_MB"};  // the device memory the batch may plan with (test / diagnostic knob)
    Knob<double> splitBudgetFrac{"CPECAN_SPLIT_BUDGET_FRAC"};  // the share of the device the rings of whole regions may take (default 0.45)
    bool traceHost = getenv("CPECAN_TRACE_HOST") != nullptr;  // one line per planned class on stderr
};
// The device as one plan sees it; filled once per upload, so that every decision of a plan rests on the same answers.
struct PlanDevice {
    int numCUs = 0;
    size_t freeBytes = 0, totalBytes = 0;  // hipMemGetInfo
    size_t idleCachedBytes = 0;            // idle blocks of the block cache: ours to reuse or drop
    bool othersAlive = false;              // another batch of this process has run on the device and is not destroyed yet
    // false (planning without a device: the tests of the plan): a kernel is taken to use the registers its build allows
    // it -- 512 / WPS, in granules -- and no static LDS, instead of what the loaded code object reports
    bool queryKernels = true;
};
// What a plan is made from: the planned batch as the host hands it over (CpkBatchPlan, cpecan_internal.h), the device and the knobs.
struct PlanInputs {
    const CpkBatchPlan &batch;
    const PlanDevice &dev;
    const PlanKnobs &knobs;
};

// Resident workgroups of `wavesPerWorkgroup` waves per CU.  hipOccupancyMaxActiveBlocksPerMultiprocessor answers 3 for
// the 64-thread kernels (it reports waves per SIMD), so the bound is computed from the register file and LDS
// directly.  Over-estimating is harmless: surplus workgroups simply queue, every wave exits when the work queue is empty.
// A team of four puts one wave on every SIMD, a team of eight two.  CPECAN_MAX_WAVES_PER_CU counts single waves and has
// never applied to teams.
// Waves per SIMD the registers of a form's kernel allow, and its static LDS.
static int kernel_resources(const PlanDevice &dev, const KernelForm &form, int *perSimdOut, size_t *staticLds) {
    int numRegs = 0;
    *staticLds = 0;
    if (dev.queryKernels) {
        hipFuncAttributes attr;
        HIP_TRY(hipFuncGetAttributes(&attr, (const void *)kernel_of(form)));
        numRegs = attr.numRegs;
        *staticLds = (size_t)attr.sharedSizeBytes;
    } else if (form.family == kFamilySweep && form.wps > 0) numRegs = kSimdVgprs / form.wps / kVgprGranule * kVgprGranule;
    const int vgprAlloc = ((numRegs > 0 ? numRegs : 128) + kVgprGranule - 1) / kVgprGranule * kVgprGranule;
    int perSimd = kSimdVgprs / vgprAlloc;
    if (perSimd > kMaxWavesPerCU / kSimdsPerCU) perSimd = kMaxWavesPerCU / kSimdsPerCU;
    if (perSimd < 1) perSimd = 1;
    *perSimdOut = perSimd;
    return CPECAN_OK;
}
static int waves_per_cu(const KernelForm &form, size_t ldsBytes, int wavesPerWorkgroup, const PlanInputs &in, int *out) {
    const PlanKnobs &knobs = in.knobs;
    int perSimd = 0;
    size_t staticLds = 0;
    if (int rc = kernel_resources(in.dev, form, &perSimd, &staticLds)) return rc;
    int perCU = kSimdsPerCU * perSimd / wavesPerWorkgroup;
    const size_t ldsTotal = ldsBytes + staticLds;
    const int byLds = (int)(kCuLdsBytes / (ldsTotal ? ldsTotal : 1));
    if (byLds < perCU) perCU = byLds;
    if (perCU > kMaxWavesPerCU / wavesPerWorkgroup) perCU = kMaxWavesPerCU / wavesPerWorkgroup;
    if (wavesPerWorkgroup == 1 && knobs.maxWavesPerCU.v >= 1 && knobs.maxWavesPerCU.v < perCU) perCU = knobs.maxWavesPerCU.v;
    *out = perCU;
    return CPECAN_OK;
}
// Even out the rounds: with R = ceil(regions / waves) rounds, ceil(regions / R) waves do the same work in the
// same number of rounds with fewer waves competing per SIMD (10 000 equal pairs: 1667 waves x 6 pairs instead
// of 1792 waves of which 1044 do 6 and 748 do 5).
static int64_t even_rounds(int64_t n, int64_t waves) {
    const int64_t rounds = (n + waves - 1) / waves;
    const int64_t even = (n + rounds - 1) / rounds;
    return (even >= 1 && even < waves) ? even : waves;
}

// The narrow class k (the packed kernel, 64 / GW regions to a wave), its regions from `base` in the device order: the
// first `cut` of them as a split part, the rest as whole regions.
static int plan_packed_class(const PlanInputs &in, int k, int64_t base, std::vector<LaunchClass> *packedSplit,
                             std::vector<LaunchClass> *packedWhole) {
    const CpkGeometry &geo = in.batch.geo;
    const CpkRegion *regions = in.batch.regions;
    const int S = geo.nStates;
    const bool expect = geo.emit == CPECAN_EMIT_EXPECT;
    LaunchClass c;
    c.packed = true;
    c.k = k;
    c.form = packed_form(geo, k, in.batch.dynamic != 0, in.batch.modelSlots > 0);
    if (!c.fn()) {
        cpk_set_error("no packed kernel for emitter %d", geo.emit);
        return CPECAN_EINVAL;
    }
    const int GW = 8 << k, G = CPK_WAVE / GW;
    c.geo = geo;
    c.geo.ringCells = geo.pRingCells[k];
    c.geo.fbCells = geo.pFbCells[k];
    c.geo.maxRefresh = geo.pMaxRefresh[k];
    c.geo.refreshCells = (int64_t)GW * geo.pMaxRefresh[k];
    c.ldsBytes = sizeof(double) * (size_t)(kLdsCubics + kLdsWeights + (expect ? kExpectCopies * 80 : 0)) +
                 (size_t)G * pack_group_bytes(S, GW);
    int perCU = 0;
    if (int rc = waves_per_cu(c.form, c.ldsBytes, 1, in, &perCU)) return rc;
    const int64_t slots = (int64_t)perCU * in.dev.numCUs;
    c.ringEl = c.geo.ringCells * S;
    c.candEl = c.geo.fbCells;
    c.refEl = c.geo.refreshCells;
    c.totEl = c.geo.maxRefresh;
    // B of a segment's emitted cells: the expectation step's second pass, the indel emitter's list pass (cpk_packed.inl)
    c.bringEl = (expect || geo.emit == CPECAN_EMIT_INDEL) ? c.geo.fbCells * S : 0;
    if (geo.emit == CPECAN_EMIT_INDEL) c.candEl = 0;  // no candidates
    // Split (round 4, cpk_packed.inl "MODE"): forward sweeps into rings of the regions' own, then one queue item per
    // (region, traceback segment).  Worth it where ONE group's walk through the longest region -- its forward and its
    // backward steps, one after the other -- is what a launch of whole regions waits for: a realign-style batch of
    // 100-5000 bp alignments took 20 ms with 6 000 pairs and 29 with 50 000 (profiles/r04_config4_chain_bound.txt).
    // Then the LONG regions of the class -- the device order is longest first -- become a split class of their own,
    // launched first: their forward chains (half the steps) run beside the whole-region waves of the shorter ones, and
    // their tracebacks, side by side, behind.  Long: more than half the diagonals of the longest, so that the whole
    // regions' chains (2 N steps) are no longer than the longest forward chain.  CPECAN_PACKED_SPLIT=1 / 0 (tests, A/B
    // runs): every region of every packed class / none; CPECAN_PACKED_SPLIT_FROM=<diagonals>: regions longer than that.
    const int64_t n = geo.nPacked[k];
    int64_t cut = 0;  // the first `cut` regions of the class run split
    {
        int64_t stepsAll = 0, nMax = 0;
        int32_t segMax = 0;
        for (int64_t di = base; di < base + n; di++) {
            const int64_t N = (int64_t)regions[di].lX + regions[di].lY;
            segMax = regions[di].nSeg > segMax ? regions[di].nSeg : segMax;
            stepsAll += 2 * N;
            nMax = N > nMax ? N : nMax;
        }
        const Knob<int> &env = in.knobs.packedSplit;
        const Knob<int64_t> &fromEnv = in.knobs.packedSplitFrom;
        const bool eligible = geo.emit == CPECAN_EMIT_MATCH && !in.batch.dynamic && !geo.debug;
        // (the steps of a wave if the class's steps were dealt out evenly over every wave slot of the chip)
        const int64_t balanced = stepsAll / (G * slots) + 1;
        // ... and only for a batch that has the device to itself: with other batches of the process in flight (a
        // pipeline) their waves fill the slots a chain leaves idle, and the split form -- rings of whole regions in HBM
        // instead of a cache-resident ring per group, six launches instead of two -- costs throughput: config 4 end to end,
        // four batches in flight, 35-37 ms per batch with whole regions against 43 split (profiles/r04_config4_chain_bound.txt)
        const bool lone = !in.dev.othersAlive;
        if (eligible && env.on()) cut = n;
        else if (eligible && !env.off() && (fromEnv.set || (lone && segMax >= 3 && 2 * nMax * 2 >= balanced * 3))) {
            const int64_t from = fromEnv.set ? fromEnv.v : nMax / 2;
            for (int64_t di = base; di < base + n; di++)  // (ordered by cells, not by diagonals: up to the last long one)
                if ((int64_t)regions[di].lX + regions[di].lY > from) cut = di - base + 1;
        }
    }
    for (int part = 0; part < 2; part++) {
        const int64_t pBase = part == 0 ? base : base + cut, pCount = part == 0 ? cut : n - cut;
        if (pCount <= 0) continue;
        LaunchClass cc = c;
        cc.regionBase = (int)pBase;
        cc.regionCount = (int)pCount;
        int64_t waves = (pCount + G - 1) / G;
        if (cc.slots()) {  // t models: t times the groups, up to the wave slots of the chip
            const int64_t groups = waves;
            for (int t = 1; t <= in.batch.modelSlots; t++) {
                cc.wavesFor[t] = (int)(groups * t < slots ? groups * t : slots);
                if (cc.wavesFor[t] > waves) waves = cc.wavesFor[t];
            }
        }
        if (waves > slots) waves = slots;
        cc.waves = (int)waves;
        cc.subSlots = waves * G;
        if (part == 0) {
            int64_t nSegPart = 0;
            for (int64_t di = pBase; di < pBase + pCount; di++) nSegPart += regions[di].nSeg;
            cc.form = with_mode(c.form, kModeForward, false);  // (match emitter, fixed expansion: `eligible` above)
            cc.formTrace = with_mode(c.form, kModeTrace, false);
            int64_t wt = (nSegPart + G - 1) / G;
            if (wt > slots) wt = slots;
            cc.wavesTrace = (int)wt;
            if (wt * G > cc.subSlots) cc.subSlots = wt * G;
            cc.itemCount = nSegPart;
        }
        if (in.knobs.traceHost)
            fprintf(stderr, "cpecan packed class %d: %d regions in groups of %d lanes, LDS %zu B, waves %d / %d, %s\n", k, cc.regionCount, GW,
                    cc.ldsBytes, cc.waves, cc.wavesTrace, form_words(cc.form, false).c_str());
        (part == 0 ? packedSplit : packedWhole)->push_back(cc);
    }
    return CPECAN_OK;
}

// With other batches of the process alive (a pipeline) the packed launches of a batch SHARE the chip's wave slots in
// proportion to what each would ask for alone, instead of each asking for all of them, and one slot per CU in eight
// stays free: the waves are persistent, so fewer of them lose nothing, nothing waits in the hardware queues behind
// them, and the small kernels of the batches around this one (fills, table build, gather, consumers) find a slot
// without waiting for a class to drain.  BASELINE config 4 end to end, six batches in flight, ten runs each over four
// calls: 2.16e10 -> 2.33e10 cells/s on average, single runs spread +-10 % either way
// (profiles/r04_config4_chain_bound.txt).  CPECAN_PACKED_SHARE=0: as before.
static void share_packed_slots(const PlanInputs &in, std::vector<LaunchClass> *packedSplit, std::vector<LaunchClass> *packedWhole) {
    if (in.knobs.packedShare.off() || !in.dev.othersAlive) return;
    int64_t total = 0;
    for (const LaunchClass &cc : *packedSplit) total += cc.waves;
    for (const LaunchClass &cc : *packedWhole) total += cc.waves;
    int perCU0 = 0;  // (of the first class; a failed query leaves 0 and with it every class as it is)
    for (const LaunchClass &cc : *packedSplit) if (!perCU0) (void)waves_per_cu(cc.formTrace, cc.ldsBytes, 1, in, &perCU0);
    for (const LaunchClass &cc : *packedWhole) if (!perCU0) (void)waves_per_cu(cc.form, cc.ldsBytes, 1, in, &perCU0);
    const int64_t room = (int64_t)perCU0 * in.dev.numCUs - in.dev.numCUs / 8;
    if (!(total > room && room > 0)) return;
    for (std::vector<LaunchClass> *part : {packedSplit, packedWhole})
        for (LaunchClass &cc : *part) {
            const int G = CPK_WAVE / (8 << cc.k);
            int64_t w = (int64_t)cc.waves * room / total;
            cc.waves = (int)(w < 1 ? 1 : w);
            if (cc.split()) {
                int64_t wt = (int64_t)cc.wavesTrace * room / total;
                cc.wavesTrace = (int)(wt < cc.waves ? cc.waves : wt);
                if (cc.wavesTrace > (int)((cc.itemCount + G - 1) / G)) cc.wavesTrace = (int)((cc.itemCount + G - 1) / G);
            }
            const int64_t mx = cc.waves > cc.wavesTrace ? cc.waves : cc.wavesTrace;
            cc.subSlots = mx * G;
        }
}

// The LDS of one wave of the class: tables, rolling rows, candidate stage, symbols -- by the form of its sweeps.
// Absolute positions (cpk_sweep.inl): two arrays of S rows with a few positions of slack, a stage of 64
// candidates, and the symbols of one traceback segment at a time instead of both whole strings.
static void set_row_form(LaunchClass &cc, bool abs, const PlanKnobs &knobs) {
    const int S = cc.geo.nStates, emit = cc.geo.emit;
    cc.abs = abs;
    cc.geo.rollStride = cc.geo.maxWidth + (abs ? kAbsSlack : 1);
    cc.geo.absWholeStrings = (abs && knobs.absWindows.off()) ? 1 : 0;
    cc.geo.seqLdsBytes = (abs && !cc.geo.absWholeStrings) ? cc.geo.wWinLdsBytes[cc.k] : cc.geo.wSeqLdsBytes[cc.k];
    cc.geo.rollDoubles = (int64_t)(abs ? 2 * S : 2 * S + 1) * cc.geo.rollStride;
    const size_t header = sizeof(double) * (lds_header_doubles(emit) + lds_stage_doubles(emit, abs));
    cc.ldsBytes = cc.geo.useGlobalRoll ? header
                                       : header + sizeof(double) * (size_t)cc.geo.rollDoubles + (size_t)((cc.geo.seqLdsBytes + 15) / 16 * 16);
}

// Expectation emitter, every diagonal of the class within two 64-lane groups: the events are formed inside the
// traceback (Sweep::tracebackExpect) from three forward diagonals kept in LDS, instead of a second pass over B
// values parked in global memory.  CPECAN_EXP_INSWEEP=0 (tests, A/B runs): the second pass everywhere; 2: inside
// the traceback whatever the LDS costs.
static void plan_expect_in_sweep(LaunchClass &c, const PlanKnobs &knobs) {
    const int S = c.geo.nStates, emit = c.geo.emit;
    const Knob<int> &env = knobs.expInSweep;
    c.geo.expInSweep = emit == CPECAN_EMIT_EXPECT && !c.geo.useGlobalRoll && c.geo.maxWidth <= 2 * CPK_WAVE /* Sweep::kExpGroups */ && !env.off();
    // 1: the build unrolled for ONE group per diagonal (classes up to 64 cells -- the host gives the expectation
    // emitter a size class of its own there, cpecan_host.c); 2: for two.  CPECAN_EXP_ONE_GROUP=0: always the latter.
    if (c.geo.expInSweep) c.geo.expInSweep = (c.geo.maxWidth <= CPK_WAVE && !knobs.expOneGroup.off()) ? 1 : 2;
    if (c.geo.expInSweep) {
        const size_t with = c.ldsBytes + sizeof(double) * (size_t)3 * (c.geo.maxWidth + 1) * S + sizeof(double) * kExpectWinCopies * 80 -
                            sizeof(double) * (size_t)(lds_header_doubles(emit) - lds_header_doubles(emit, true));
        // ... as long as the three forward diagonals in LDS do not cost a resident wave: the kernel's registers
        // allow eight per CU (five-state: bands up to 74 cells, three-state: up to ~120; measured at 66 and 106)
        if (with <= kCuLdsBytes / 8 || (env.set && env.v >= 2)) c.ldsBytes = with;
        else c.geo.expInSweep = 0;
    }
}

// The build of *f for three waves per SIMD, taken where it puts more waves on a CU than *f's perCU: *p3 is its waves per CU then, else 0.
static int take_three_waves(const PlanInputs &in, KernelForm *f, size_t ldsBytes, int perCU, int *p3) {
    KernelForm f3 = *f;
    f3.wps = 3;
    if (int rc = waves_per_cu(f3, ldsBytes, 1, in, p3)) return rc;
    if (*p3 > perCU) *f = f3;
    else *p3 = 0;
    return CPECAN_OK;
}

// The gang a launch of class `c` could run as (`f`: its kernel, waveLds: the LDS of one wave of it): *g waves per workgroup
// and *perCU resident waves per CU, or 0 where the form has no gang build, its registers do not allow three waves per SIMD
// or fewer than two waves fit.  forced: CPECAN_GANG=n, that many waves per workgroup -- as many workgroups per CU as fit --,
// else one workgroup per CU of as many waves as fit, twelve at most.
static int gang_waves(const PlanInputs &in, const LaunchClass &c, KernelForm f, size_t waveLds, int forced, int *g, int *perCU) {
    *g = *perCU = 0;
    f.wps = 3;
    f.gang = true;
    if (!has_kernel(f)) return CPECAN_OK;
    int perSimd = 0;
    size_t staticLds = 0;
    if (int rc = kernel_resources(in.dev, f, &perSimd, &staticLds)) return rc;
    const size_t shared = sizeof(double) * lds_header_doubles(c.geo.emit) + staticLds, own = c.gang_lds_bytes(waveLds, 2) - c.gang_lds_bytes(waveLds, 1);
    if (perSimd < 3 || own == 0 || shared + 2 * own > kCuLdsBytes) return CPECAN_OK;
    int n = (int)((kCuLdsBytes - shared) / own);
    if (n > kGangMaxWaves) n = kGangMaxWaves;
    int groups = 1;
    if (forced) {
        if (forced < 2 || forced > n) return CPECAN_OK;
        n = forced;
        groups = (int)(kCuLdsBytes / (shared + (size_t)n * own));
        if (groups > kGangMaxWaves / n) groups = kGangMaxWaves / n;
    }
    *g = n;
    *perCU = groups * n;
    return CPECAN_OK;
}

// A team of waves per region, or one wave per region -- then, maybe, the build for three waves per SIMD.  Sets the
// class's kernel and *perCUOut, its resident workgroups per CU.
static int plan_team_or_solo(const PlanInputs &in, LaunchClass &c, int *perCUOut) {
    const CpkGeometry &geo = in.batch.geo;
    const int S = geo.nStates, k = c.k;
    const bool expect = geo.emit == CPECAN_EMIT_EXPECT;
    int perCU = 0;
    // Bands of several hundred cells: a team of kTeamWaves waves per region (cpk_team.inl) instead of one wave
    constexpr int kTeamWaves = 4;
    // (the team kernel stages both whole strings and keeps 3 S rows of maxWidth + 1 positions, whatever form of the
    // rows the class would take with one wave per region: NOT c.geo.seqLdsBytes / rollStride, which set_row_form()
    // may have set to the symbol windows and slack of the absolute-position sweeps)
    const int teamStride = c.geo.maxWidth + 1;
    const size_t teamLds = sizeof(double) * ((size_t)team_header_doubles(expect) + (size_t)3 * S * teamStride) +
                           (size_t)((geo.wSeqLdsBytes[k] + 15) / 16 * 16);
    // A class goes to teams where one wave per region is down to three waves per CU or fewer (measured: at four per
    // CU, ~400-cell bands, the single wave still wins by 13 %; at three, ~450 cells, the team wins by 30 %), or on
    // the global-memory variant.  CPECAN_TEAM=<cells> (tests, diagnostics): from that band width instead; 0: never.
    const Knob<int> &teamEnv = in.knobs.team;
    int soloPerCU = 0;
    if (int rc = waves_per_cu(c.form, c.ldsBytes, 1, in, &soloPerCU)) return rc;
    const bool wanted = teamEnv.set ? (teamEnv.v > 0 && c.geo.maxWidth >= teamEnv.v)
                                    : (c.geo.maxWidth > 256 && (soloPerCU <= 3 || c.geo.useGlobalRoll));
    // one workgroup per CU is all the LDS allows from ~660 cells: then eight waves share the region
    const bool big = 2 * teamLds > kCuLdsBytes;
    if (wanted && (geo.emit == CPECAN_EMIT_MATCH || geo.emit == CPECAN_EMIT_INDEL || expect) && !geo.debug &&
        c.geo.maxWidth <= CPK_WAVE * kTeamWaves * (big ? 2 : 1) * kTeamGroups && teamLds <= kCuLdsBytes) {
        // (round 4: the indel emitter's three lists and the expectation emitter -- its second pass shared by the team's waves)
        c.form = team_form(c.form, kTeamWaves * (big ? 2 : 1));
        c.threads = CPK_WAVE * kTeamWaves * (big ? 2 : 1);
        c.geo.useGlobalRoll = 0;
        c.abs = false;
        c.geo.absWholeStrings = 0;
        c.geo.expInSweep = 0;  // (the team's expectation emitter is the second pass: B of the emitted cells in `bring`)
        c.geo.rollStride = teamStride;
        c.geo.seqLdsBytes = geo.wSeqLdsBytes[k];
        c.geo.rollDoubles = (int64_t)(2 * S + 1) * c.geo.rollStride;
        c.ldsBytes = teamLds;
        c.grollEl = 0;
        if (int rc = waves_per_cu(c.form, teamLds, c.threads / CPK_WAVE, in, &perCU)) return rc;
        if (perCU < 1) perCU = 1;
    } else {
        perCU = soloPerCU;
        // Three-state match classes with more regions than two waves per SIMD hold take the kernels allocated for
        // three (168 VGPRs, a handful of spills): 4000 pairs of 1 kb -9 to -19 %, 2500 of 2 kb -17 %, with one wave
        // per region -34 %; a class that leaves slots empty anyway loses 3-10 % to the spills and the fuller SIMDs
        // (config A, 1000 pairs: 3.68 -> 4.07 ms) and keeps the 2-wave kernels.  CPECAN_DENSE=1 / 0: always / never.
        const Knob<int> &denseEnv = in.knobs.dense;
        if (S == 3 && geo.emit == CPECAN_EMIT_MATCH && !geo.debug &&
            (denseEnv.set ? denseEnv.v != 0 : geo.nWide[k] >= (int64_t)soloPerCU * in.dev.numCUs)) {
            int p3 = 0;
            if (int rc = take_three_waves(in, &c.form, c.ldsBytes, perCU, &p3)) return rc;
            c.dense = p3 > 0;
            if (c.dense) perCU = p3;
        }
    }
    *perCUOut = perCU;
    return CPECAN_OK;
}

// Split the class when its regions do not fill the chip and have tracebacks to hand out: the segments of a
// region are independent once its forward values exist.  CPECAN_SPLIT=1 / 0 (tests, diagnostics): always / never.
// `perCU`: the resident waves per CU of the class's one-wave-per-region kernel; nSegClass: its traceback segments.
static void plan_chains(const PlanInputs &in, LaunchClass &c, int64_t nSegClass);  // (below)
static int plan_split_form(const PlanInputs &in, LaunchClass &c, int64_t nSegClass, int perCU) {
    const CpkGeometry &geo = in.batch.geo;
    const int S = geo.nStates, numCUs = in.dev.numCUs;
    const int64_t n = c.regionCount;
    int64_t maxRing = 0;
    for (int64_t di = c.regionBase; di < c.regionBase + c.regionCount; di++) {
        const int64_t rd = split_ring_doubles(in.batch.regions[di], S);
        if (rd > maxRing) maxRing = rd;
    }
    const Knob<int> &env = in.knobs.split;
    const int64_t slots = (int64_t)perCU * numCUs;
    // (debug buffers: split only where CPECAN_SPLIT asks for it -- the per-cell parity tests of the split forms)
    const bool eligible = c.threads == CPK_WAVE && geo.emit == CPECAN_EMIT_MATCH && (!geo.debug || env.set) && nSegClass > 0;
    // Regions with tracebacks to hand out (1.25 segments on average and more) run split whenever their rings fit:
    // measured against one wave per region on 600 to 10 000 pairs of 1-4 kb and bands of 55-124 cells per diagonal,
    // one of the two split forms won every time (tools/split_forms.py, profiles/r02_split_forms.txt).  Which one:
    // the ONE-launch form fills the partly empty last round of forward sweeps with traceback items and wins where a
    // region has many segments (2 kb and longer: -20 to -40 %); with two or three segments per region (1 kb
    // pairs, config A) its device-scope ring accesses and waiting waves cost more than that gains (+7 to +19 %) and the
    // two launches win.  The rings of whole regions are given up first when device memory is short (fit_to_memory).
    const bool manySegs = nSegClass * 4 >= n * 5;
    const bool wanted = env.set ? env.v != 0 : manySegs;
    // ... and up to ~4.5 rounds of forward sweeps: beyond, every region ticket is drawn before the first item anyway,
    // the overlap is down to the seam between the two phases, and the launches' plain ring stores win against
    // the one launch's write-through ones (2 kb pairs, band 100: 5000 / 6500 / 8000 pairs -8 / -8 / -2 % for the one
    // launch, 10 000 pairs -- config B -- +1.7 %: 89.3 against 87.6 ms, and 90.2 against 87.3 ms per pipelined batch)
    // (round 4, both forms at ten waves per CU: 5000 pairs -3 % for the one launch, 7000 pairs +3 %: ~3.25 rounds)
    const bool oneLaunch = nSegClass * 2 >= n * 7 /* 3.5 segments per region and more */ && n * 4 < slots * 13;
    if (!(eligible && wanted)) {
        // one wave per region: the other form of the rows (a class that went to a team of waves keeps the team's LDS)
        if (c.abs) {
            if (c.threads == CPK_WAVE) set_row_form(c, false, in.knobs);
            else c.abs = false;
        }
        return CPECAN_OK;
    }
    c.form.abs = c.abs;  // the sweeps of the split modes follow the rows
    c.itemCount = nSegClass;
    // CPECAN_SPLIT=2 / 1: force the one-launch (kModeFused) / two-launch form
    // (the one-launch form addresses a region's ring with 32-bit byte offsets: Sweep::ringPut)
    if ((env.set ? env.v == 2 : oneLaunch) && maxRing < ((int64_t)1 << 28)) {
        // an item polls this often (s_sleep between polls: seconds in all) for its region's forward values; a
        // count that never comes is reported and the class re-run in two launches (cpk_device_download).
        // CPECAN_FUSED_SPIN: tests force that path with a bound of a few polls.
        c.geo.fusedSpin = in.knobs.fusedSpin.set ? in.knobs.fusedSpin.v : (1 << 24);
        c.form = with_mode(c.form, kModeFused, c.dense);
        int64_t slotsF = slots;
        if (c.abs && S == 5 && !in.knobs.fused3.off() && kCuLdsBytes / c.ldsBytes >= kThreeWpsLdsWaves) {
            int p3 = 0;
            if (int rc = take_three_waves(in, &c.form, c.ldsBytes, perCU, &p3)) return rc;
            if (p3) slotsF = (int64_t)p3 * numCUs;
        }
        // One CU in eight keeps a wave slot (and its 19 KB of LDS) free: a launch that fills every slot to its
        // end starves the small kernels of the batch before it -- the list consumers need a few KB of LDS --
        // until it drains, and a pipeline two batches deep then idles between sweeps (82 ms measured).
        // ... so the slots are left free when another batch of this process has run on the device and is still
        // alive; a batch on its own takes them all (config B: 90.3 -> 89.5 ms).
        const int64_t spare = in.dev.othersAlive ? numCUs / 8 : 0;
        const int64_t room = slotsF - spare > 0 ? slotsF - spare : slotsF;
        int64_t wt = room < n + nSegClass ? room : n + nSegClass;
        c.waves = (int)wt;
        c.subSlots = wt;
        return CPECAN_OK;
    }
    c.formTrace = with_mode(c.form, kModeTrace, c.dense);
    c.form = with_mode(c.form, kModeForward, c.dense);
    int64_t wt = slots < nSegClass ? slots : nSegClass;
    c.wavesTrace = (int)wt;
    if (wt > c.subSlots) c.subSlots = wt;
    int perCUTrace = perCU, perCUFwd = perCU;  // resident waves per CU of either launch
    // the forward launch: no candidate ring in its LDS, and with absolute positions few enough registers
    // for three waves per SIMD -- more waves per CU where that LDS allows them (CPECAN_FWD3=0: never)
    c.ldsBytesFwd = c.geo.useGlobalRoll ? c.ldsBytes : c.ldsBytes - sizeof(double) * lds_stage_doubles(geo.emit, c.abs);
    // ... and so does the traceback launch of a five-state class since round 4 (CPECAN_TRACE3=0: never)
    if (c.abs && S == 5 && !in.knobs.trace3.off() && kCuLdsBytes / c.ldsBytes >= kThreeWpsLdsWaves) {
        int p3 = 0;  // (168 VGPRs)
        if (int rc = take_three_waves(in, &c.formTrace, c.ldsBytes, perCU, &p3)) return rc;
        if (p3) {
            int64_t w3 = (int64_t)p3 * numCUs;
            if (w3 > nSegClass) w3 = nSegClass;
            c.wavesTrace = (int)w3;
            if (w3 > c.subSlots) c.subSlots = w3;
            perCUTrace = p3;
        }
    }
    if (c.abs && !in.knobs.fwd3.off() && kCuLdsBytes / c.ldsBytesFwd >= kThreeWpsLdsWaves) {
        int p3 = 0;  // (no candidate ring and 120 VGPRs or fewer: profiles/r03_occupancy_3_waves_per_simd.txt)
        if (int rc = take_three_waves(in, &c.form, c.ldsBytesFwd, perCU, &p3)) return rc;
        if (p3) {
            int64_t wf = (int64_t)p3 * numCUs;
            if (wf > n) wf = n;
            c.waves = (int)even_rounds(n, wf);  // forward waves touch no per-slot scratch: subSlots stays as it is
            perCUFwd = p3;
        }
    }
    // Gangs: either launch as workgroups of several waves with one copy of the tables (cpk_sweep.inl "GANG").  One workgroup
    // may declare the whole LDS of a CU, so what the tables took in every wave becomes room for one wave more: config B,
    // ten single waves per CU -> one gang of eleven.  Taken (CPECAN_GANG unset) by a launch that already runs the build for
    // three waves per SIMD and whose queue fills every wave of every gang -- with less work than that, gangs would crowd
    // onto few CUs the waves that single-wave workgroups spread over all of them (config A keeps its plan).  Measured at
    // config B (profiles/gang_workgroups_ab.txt): the traceback launch alone 83.3 -> 79.2 ms per step, both launches 76.4.
    if (c.abs && !c.geo.useGlobalRoll && !in.knobs.gang.off()) {
        const int forced = in.knobs.gang.set ? in.knobs.gang.v : 0;
        // The traceback launch: items are handed out longest first to whoever is free, so every wave more per CU counts --
        // a gang where it puts more waves on a CU than single-wave workgroups do.
        int g = 0, perCUGang = 0;
        if (int rc = gang_waves(in, c, c.formTrace, c.ldsBytes, forced, &g, &perCUGang)) return rc;
        if (g > 1 && (forced || (c.formTrace.wps == 3 && perCUGang > perCUTrace && nSegClass >= (int64_t)perCUGang * numCUs))) {
            c.formTrace.wps = 3;
            c.formTrace.gang = true;
            c.gangTrace = g;
            int64_t w = (int64_t)perCUGang * numCUs;
            if (w > nSegClass) w = nSegClass;
            c.wavesTrace = (int)((w + g - 1) / g * g);  // whole gangs: a wave without an item leaves at once
            if (c.wavesTrace > c.subSlots) c.subSlots = c.wavesTrace;
        }
        // The forward launch is quantised -- equal regions run in rounds -- so the rounds, evened out, keep deciding its
        // wave count: the waves a round fewer asks for where the gangs' waves per CU take one off, else the count it has,
        // laid out as whole gangs -- all of them resident at once, or a round would be added.
        if (int rc = gang_waves(in, c, c.form, c.ldsBytesFwd, forced, &g, &perCUGang)) return rc;
        const int64_t cap = (int64_t)perCUGang * numCUs;
        if (g > 1 && (forced || (c.form.wps == 3 && perCUGang > perCUFwd && n >= cap))) {
            int64_t w = c.waves;
            if (!forced && (n + cap - 1) / cap < (n + w - 1) / w) w = even_rounds(n, cap);
            const int64_t groups = (w + g - 1) / g;
            if (forced || groups * g <= cap) {
                c.form.wps = 3;
                c.form.gang = true;
                c.gang = g;
                c.waves = (int)(groups * g);
            }
        }
        plan_chains(in, c, nSegClass);
    }
    return CPECAN_OK;
}

// The cost of a queue item in cells, the measure the item queue is ordered by: a segment's traceback walks the diagonals
// tbPrev + 1 .. dTop; a chain from segment K sweeps the diagonals behind the top of segment K - 1 forward as well.
static int64_t item_cost(const CpkRegion &rg, const CpkSegment &sg) { return (int64_t)(sg.dTop - sg.tbPrev) * rg.maxWidth; }
static int64_t chain_cost(const CpkRegion &rg, const CpkSegment *segs, int K) {
    int64_t cost = (int64_t)(segs[rg.segOff + rg.nSeg - 1].dTop - segs[rg.segOff + K - 1].dTop) * rg.maxWidth;
    for (int32_t si = K; si < rg.nSeg; si++) cost += item_cost(rg, segs[rg.segOff + si]);
    return cost;
}
// Chains: the traceback launch takes over the forward sweep of every region's later segments.  The forward queue of a class
// holds its regions and nothing else; where there are more of them than waves it runs in whole rounds, and with equal
// regions (config B: 10 000 for 2816 slots, 3.55 rounds) the last round is paid in full by a launch that cannot even use
// every CU for it.  The item queue mixes thousands of items of every length, handed out longest first, and ends even.  So
// the forward launch sweeps only the first K segments of a region and ONE item per region -- a chain, cpk_sweep.inl
// "CHAIN" -- sweeps the others forward from the two diagonals the ring holds at the top of segment K - 1 and traces them
// back itself: no wave waits for another.  Taken where both launches are gangs (the builds that exist) and the forward
// launch is quantised.  A region of K or fewer segments is swept wholly by the forward launch and has plain items only.
// K is the smallest for which the chains -- the longest items there are, ceil(chains / waves) of them to a wave -- do not
// stretch the item launch beyond what its work, dealt out evenly, takes:
//     ceil(chains / trace waves) x longest chain <= (cost of all chains + cost of all plain items) / trace waves.
// CPECAN_CHAIN=0: none; CPECAN_CHAIN=k (tests): K = k wherever both launches are gangs, whatever the queue.
static void plan_chains(const PlanInputs &in, LaunchClass &c, int64_t nSegClass) {
    const Knob<int> &env = in.knobs.chain;
    c.chainFrom = 0;
    c.chains = c.chainedSegs = 0;
    c.chainsNeedGang = false;
    if (env.off() || c.gangTrace <= 1 || in.batch.modelSlots > 0 || c.geo.emit != CPECAN_EMIT_MATCH) return;
    if (c.gang <= 1) {  // the CHAIN builds are gangs in both launches
        c.chainsNeedGang = env.set || c.regionCount > c.waves;
        return;
    }
    const bool forced = env.set;
    if (!forced && c.regionCount <= c.waves) return;  // every region has a wave of its own: nothing is quantised
    const CpkRegion *first = in.batch.regions + c.regionBase, *end = first + c.regionCount;
    int32_t segMax = 0;
    int64_t plainAll = 0;
    for (const CpkRegion *rg = first; rg < end; rg++) {
        segMax = rg->nSeg > segMax ? rg->nSeg : segMax;
        for (int32_t si = 0; si < rg->nSeg; si++) plainAll += item_cost(*rg, in.batch.segs[rg->segOff + si]);
    }
    for (int K = forced ? env.v : 1; K >= 1 && K < segMax; K++) {
        int64_t chains = 0, chained = 0, longest = 0, total = plainAll;
        for (const CpkRegion *rg = first; rg < end; rg++) {
            if (rg->nSeg <= K) continue;
            const int64_t cost = chain_cost(*rg, in.batch.segs, K);
            chains++;
            chained += rg->nSeg - K;
            longest = cost > longest ? cost : longest;
            // (the tracebacks of the chained segments are in plainAll already: what a chain adds is its forward sweep)
            total += (int64_t)(in.batch.segs[rg->segOff + rg->nSeg - 1].dTop - in.batch.segs[rg->segOff + K - 1].dTop) * rg->maxWidth;
        }
        const int64_t wt = c.wavesTrace > 0 ? c.wavesTrace : 1;
        if (forced || (chains + wt - 1) / wt * longest * wt <= total) {
            c.chainFrom = K;
            c.chains = chains;
            c.chainedSegs = chained;
            c.itemCount = nSegClass - chained + chains;
            c.form.chain = c.formTrace.chain = true;
            return;
        }
    }
}

// ", gang of n ..." for a class's CPECAN_TRACE_HOST line: the launches that run as gangs, with the LDS of a workgroup
static std::string gang_words(const LaunchClass &c) {
    std::string w;
    if (c.gang > 1) w += ", forward launch: gang of " + std::to_string(c.gang) + " (LDS " + std::to_string(c.firstLdsBytes()) + " B)";
    if (c.gangTrace > 1) w += ", traceback launch: gang of " + std::to_string(c.gangTrace) + " (LDS " + std::to_string(c.traceLdsBytes()) + " B)";
    if (c.chainFrom > 0) w += ", chains from segment " + std::to_string(c.chainFrom) + ": " + std::to_string(c.chains);
    if (c.chainsNeedGang) w += ", no chains: the forward launch is no gang";
    return w;
}

// The wide class k (the sweep kernel, one region per wave or team at a time), its regions from `base` in the device order.
static int plan_wide_class(const PlanInputs &in, int k, int base, LaunchClass *out) {
    const CpkGeometry &geo = in.batch.geo;
    const int S = geo.nStates;
    const bool expect = geo.emit == CPECAN_EMIT_EXPECT;
    LaunchClass c;
    c.k = k;
    c.geo = geo;
    c.geo.maxWidth = geo.wMaxWidth[k];
    c.geo.maxRefresh = geo.wMaxRefresh[k];
    c.geo.ringCells = geo.wRingCells[k];
    c.geo.fbCells = geo.wFbCells[k];
    c.geo.seqLdsBytes = geo.wSeqLdsBytes[k];
    c.geo.rollStride = c.geo.maxWidth + 1;
    // Will the class run split (its tracebacks as queue items; decided in plan_split_form, once the occupancy is known)?
    // Then, with a fixed expansion and bands whose edges move one step per diagonal (CpkRegion::absOk), its sweeps index
    // the rolling rows by absolute position (cpk_sweep.inl): the rows need a few positions of slack.
    // CPECAN_ABS=0: never (A/B runs, tests of the other form).
    int64_t nSegClass = 0;
    bool absOk = geo.emit == CPECAN_EMIT_MATCH && !in.batch.dynamic;
    for (int64_t di = base; di < base + geo.nWide[k]; di++) {
        nSegClass += in.batch.regions[di].nSeg;
        absOk = absOk && in.batch.regions[di].absOk;
    }
    const Knob<int> &splitEnv = in.knobs.split;
    const bool splitLikely = geo.emit == CPECAN_EMIT_MATCH && (!geo.debug || splitEnv.set) && nSegClass > 0 &&
                             (splitEnv.set ? splitEnv.v != 0 : nSegClass * 4 >= (int64_t)geo.nWide[k] * 5);
    const bool absWanted = splitLikely && absOk && !in.knobs.abs.off();
    c.geo.refreshCells = (int64_t)c.geo.maxWidth * c.geo.maxRefresh;
    if (c.geo.refreshCells < 1) c.geo.refreshCells = 1;
    // LDS budget: beyond 64 KiB per wave (rolling buffers + symbol strings, in the form every class can fall back
    // to: one wave per region) the class takes the global-memory path
    c.geo.useGlobalRoll = 0;
    set_row_form(c, false, in.knobs);
    c.geo.useGlobalRoll = c.ldsBytes + 16 > kLdsPathMaxBytes;
    set_row_form(c, absWanted && !c.geo.useGlobalRoll, in.knobs);  // absolute positions are a form of the LDS rows
    plan_expect_in_sweep(c, in.knobs);
    c.form = wide_form(c.geo, in.batch.modelSlots > 0);
    if (!c.fn()) {
        cpk_set_error("no kernel for emitter %d", geo.emit);
        return CPECAN_EINVAL;
    }
    int perCU = 0;
    if (int rc = plan_team_or_solo(in, c, &perCU)) return rc;
    if (perCU < 1) {
        cpk_set_error("kernel does not fit on a CU (LDS %zu bytes)", c.ldsBytes);
        return CPECAN_EHIP;
    }
    const int64_t n = geo.nWide[k];
    int64_t waves = (int64_t)perCU * in.dev.numCUs;
    if (waves > n) waves = n;
    waves = even_rounds(n, waves);
    if (c.slots()) {
        // t models: t x n virtual regions -- an under-subscribed class gets more waves, a saturated one none.  (Rounds are
        // evened out per t, so the count is not monotone in t: the scratch is sized for the most.)
        const int64_t cap = (int64_t)perCU * in.dev.numCUs;
        for (int t = 1; t <= in.batch.modelSlots; t++) {
            const int64_t v = n * t;
            c.wavesFor[t] = (int)even_rounds(v, cap < v ? cap : v);
            if (c.wavesFor[t] > waves) waves = c.wavesFor[t];
        }
    }
    c.waves = (int)waves;
    c.subSlots = waves;
    c.regionBase = base;
    c.regionCount = geo.nWide[k];
    if (int rc = plan_split_form(in, c, nSegClass, perCU)) return rc;
    if (in.knobs.traceHost)
        fprintf(stderr, "cpecan class %d: %d regions, widest diagonal %d, LDS %zu B (forward launch %zu B), waves %d / %d, %s%s\n", k,
                c.regionCount, c.geo.maxWidth, c.ldsBytes, c.ldsBytesFwd, c.waves, c.wavesTrace, form_words(c.form, c.dense).c_str(),
                gang_words(c).c_str());
    c.ringEl = c.geo.ringCells * S;
    c.candEl = c.geo.fbCells * (geo.emit == CPECAN_EMIT_INDEL ? 3 : 1);  // candidate lists
    c.refEl = c.geo.refreshCells;
    c.totEl = c.geo.maxRefresh;
    c.bringEl = expect ? (c.geo.expInSweep ? (int64_t)c.geo.maxRefresh * 96 /* Sweep::kWinDoubles */ : c.geo.fbCells * S) : 0;
    c.grollEl = (c.geo.useGlobalRoll && c.threads == CPK_WAVE) ? c.geo.rollDoubles : 0;
    *out = c;
    return CPECAN_OK;
}

// back to one wave per region (a packed class: whole regions) with a per-wave ring
static void unsplit(LaunchClass &c, const PlanKnobs &knobs) {
    c.form = with_mode(c.form, kModeWhole, c.dense);
    c.formTrace = KernelForm{};
    c.form.gang = c.form.chain = false;
    c.gang = c.gangTrace = 0;
    c.chainFrom = 0;
    c.chains = c.chainedSegs = 0;
    c.chainsNeedGang = false;
    c.itemCount = 0;
    c.ringTotal = 0;
    c.ringEl = c.geo.ringCells * c.geo.nStates;
    if (c.abs) set_row_form(c, false, knobs);
    c.subSlots = c.packed ? (int64_t)c.waves * (CPK_WAVE / (8 << c.k)) : c.waves;
}
// A fused class as two launches -- all forward sweeps, then all items -- which needs no hand-off inside a launch: what
// a class runs as after an item of its one launch gave up waiting (cpk_device_download).  The plain two-launch kernels,
// without the builds for three waves per SIMD, and the launch's waves for both.
static void unfuse(LaunchClass &c) {
    c.formTrace = with_mode(c.form, kModeTrace, c.dense);
    c.form = with_mode(c.form, kModeForward, c.dense);
    c.wavesTrace = c.waves;
    if (c.waves > c.regionCount) c.waves = c.regionCount;
}
// device bytes of the plan as it stands, and with one resident wave per class
static void tally(const std::vector<LaunchClass> &classes, double fixed, double *need, double *floorNeed) {
    *need = *floorNeed = fixed;
    for (const LaunchClass &c : classes) {
        *need += c.slotBytes() * (double)c.subSlots + 8.0 * (double)c.ringTotal;
        *floorNeed += c.slotBytes() * (double)(c.subSlots / (c.waves > 0 ? c.waves : 1)) + 8.0 * (double)c.ringTotal;
    }
}
// Every resident wave owns scratch sized for its class's LARGEST region (forward ring of one traceback segment,
// candidates, refresh series).  One unanchored 3000 x 3000 region (a single segment: 360 MB of ring) in a class of
// its own is one wave's worth; where a class still asks for more than the device has free, it keeps as many
// waves as fit and the rest of its regions queue behind them.
static int fit_to_memory(const PlanInputs &in, std::vector<LaunchClass> &classes) {
    const CpkGeometry &geo = in.batch.geo;
    const CpkBatchPlan &batch = in.batch;
    // the sizes of a batch that no plan changes: what its tables, strings and results take on the device
    const double fixed = (double)sizeof(CpkRegion) * geo.nRegions + (double)(sizeof(CpkDiag) + sizeof(int32_t)) * batch.nDiags +
                         (double)sizeof(CpkSegment) * batch.nSegs + (double)batch.nSymbolBytes + 24.0 * batch.nAnchors +
                         2.0 * 12.0 * batch.nLists * batch.outTriplesPerList /* the triples and their compact copy */;
    double budget = 0.9 * ((double)in.dev.freeBytes + (double)in.dev.idleCachedBytes);  // idle cached blocks are ours to reuse or drop
    if (in.knobs.memBudgetMb.set) budget = 1048576.0 * in.knobs.memBudgetMb.v;
    // split classes keep one ring per REGION (it holds every segment of the region), nothing per slot
    for (LaunchClass &c : classes) {
        if (!c.split()) continue;
        c.ringTotal = 0;
        for (int64_t di = c.regionBase; di < c.regionBase + c.regionCount; di++) c.ringTotal += split_ring_doubles(in.batch.regions[di], geo.nStates);
        c.ringEl = 0;
    }
    // The rings of whole regions are a fixed share of the device at most (CPECAN_SPLIT_BUDGET_FRAC, default 0.45: two
    // pipelined batches fit whatever is free at this moment), so that the same batch always runs in the same form.
    double splitBudget = 0.45 * (double)in.dev.totalBytes;
    if (in.knobs.splitBudgetFrac.set) splitBudget = in.knobs.splitBudgetFrac.v * (double)in.dev.totalBytes;
    double need = 0, floorNeed = 0;
    tally(classes, fixed, &need, &floorNeed);
    if (need > budget || need > splitBudget) {  // whole-region rings are a luxury: give them up before giving up resident waves
        for (LaunchClass &c : classes)
            if (c.split()) unsplit(c, in.knobs);
        tally(classes, fixed, &need, &floorNeed);
    }
    if (floorNeed > budget) {
        cpk_set_error("out of device memory: the batch needs %.0f MB with one resident wave per size class, %.0f MB are free",
                      floorNeed / 1048576.0, budget / 1048576.0);
        return CPECAN_ENOMEM;
    }
    if (need > budget) {
        // the narrow and less wide classes first: they hold most of the regions
        double left = budget - floorNeed;
        for (LaunchClass &c : classes) {
            const int64_t perWave = c.subSlots / c.waves;
            const double waveBytes = c.slotBytes() * (double)perWave;
            int64_t extra = waveBytes > 0 ? (int64_t)(left / waveBytes) : c.waves - 1;
            if (extra > c.waves - 1) extra = c.waves - 1;
            if (extra < 0) extra = 0;
            left -= waveBytes * (double)extra;
            c.waves = (int)(1 + extra);
            c.subSlots = perWave * c.waves;
        }
    }
    return CPECAN_OK;
}

// The launches of a run: one per size class that has regions -- the split parts of the narrow classes, their whole
// parts, then the wide classes -- fitted to the device's memory.
static int plan_batch(const CpkBatchPlan &batch, const PlanDevice &dev, const PlanKnobs &knobs, std::vector<LaunchClass> *out) {
    const PlanInputs in{batch, dev, knobs};
    const CpkGeometry &geo = batch.geo;
    if (batch.modelSlots > 0 && geo.emit != CPECAN_EMIT_EXPECT && geo.emit != kEmitForward) {
        cpk_set_error("model slots: expectation and forward emitters only");
        return CPECAN_EINVAL;
    }
    out->clear();
    int regionAt = 0;
    std::vector<LaunchClass> packedSplit, packedWhole;
    for (int k = 0; k < 3; k++) {  // narrow regions come first in the device order: the packed kernel, 64 / GW to a wave
        if (geo.nPacked[k] <= 0) continue;
        if (int rc = plan_packed_class(in, k, regionAt, &packedSplit, &packedWhole)) return rc;
        regionAt += geo.nPacked[k];
    }
    share_packed_slots(in, &packedSplit, &packedWhole);
    // the split parts first: their forward chains are the longest thing in the batch and start before anything else
    out->insert(out->end(), packedSplit.begin(), packedSplit.end());
    out->insert(out->end(), packedWhole.begin(), packedWhole.end());
    for (int k = 0; k < CPK_WIDE_CLASSES; k++) {  // then the wide ones: the sweep kernel, one region per wave at a time
        if (geo.nWide[k] <= 0) continue;
        LaunchClass c;
        if (int rc = plan_wide_class(in, k, regionAt, &c)) return rc;
        out->push_back(c);
        regionAt += geo.nWide[k];
    }
    if ((int)out->size() > kMaxClasses || regionAt != geo.nRegions) {
        cpk_set_error("internal: the size classes do not cover the regions (%d of %d)", regionAt, geo.nRegions);
        return CPECAN_ESTATE;
    }
    return fit_to_memory(in, *out);
}
