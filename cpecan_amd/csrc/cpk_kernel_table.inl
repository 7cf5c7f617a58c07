// cpk_kernel_table.inl -- the pair-HMM kernel variants of the library as values.  A KernelForm names a variant by its
// template arguments, kKernelTable lists the variants that are built, kernel_of() finds one.  The launch plan
// (cpk_plan.inl) builds and edits forms; this file is the only place where a kernel template is named with arguments.
// Part of the single HIP translation unit cpecan_kernels.hip (included there, behind the kernels); not compiled on its own.

using KernelFn = void (*)(const KArgs);
enum { kNoKernel = 0, kFamilySweep, kFamilyPacked, kFamilyTeam };

// The template arguments of one kernel.  A field its family does not have keeps the value it has here.
struct KernelForm {
    int family = kNoKernel, S = 0, emit = 0, mode = kModeWhole;  // family: cpecan_pairhmm_sweep / _packed / _team
    bool fast = false;  // sweep: LDS rolling rows + LDS symbol strings (FAST); false: the rows roll in global memory
    int wps = 0;        // sweep: waves per SIMD the registers are allocated for (WPS)
    bool abs = false;   // sweep: absolute-position sweeps (ABS)
    int inSweep = 0;    // sweep: expectation events inside the traceback, for one / two groups per diagonal (INSWEEP)
    bool slots = false, dynamic = false;  // dynamic: packed, per-anchor expansions (DYN)
    int width = 0;      // packed: lanes of a group (GW); team: waves (T)
    bool gang = false;  // sweep: workgroups of several waves that share the LDS tables (GANG)
    bool chain = false; // sweep: gangs of a class whose traceback launch sweeps the regions' later segments forward (CHAIN)
};
constexpr bool operator==(const KernelForm &a, const KernelForm &b) {
    return a.family == b.family && a.S == b.S && a.emit == b.emit && a.mode == b.mode && a.fast == b.fast && a.wps == b.wps && a.abs == b.abs &&
           a.inSweep == b.inSweep && a.slots == b.slots && a.dynamic == b.dynamic && a.width == b.width && a.gang == b.gang && a.chain == b.chain;
}
struct KernelEntry { KernelForm form; KernelFn fn; };
// One macro per family builds the key and the pointer of an entry from the same argument list; _F repeats it for LDS and
// global rows, _G / _T for the three group widths / the two team sizes, CPK_BOTH(row macro, ...) for both state counts.
#define CPK_SWEEP_GANG(S, FAST, EMIT, MODE, WPS, ABS, INSWEEP, SLOTS, GANG) \
    {KernelForm{kFamilySweep, S, EMIT, MODE, FAST, WPS, ABS, INSWEEP, SLOTS, false, 0, GANG}, cpecan_pairhmm_sweep<S, FAST, EMIT, MODE, WPS, ABS, INSWEEP, SLOTS, GANG>},
#define CPK_SWEEP(...) CPK_SWEEP_GANG(__VA_ARGS__, false)
#define CPK_SWEEP_CHAIN(S, MODE) \
    {KernelForm{kFamilySweep, S, CPECAN_EMIT_MATCH, MODE, true, 3, true, 0, false, false, 0, true, true}, \
     cpecan_pairhmm_sweep<S, true, CPECAN_EMIT_MATCH, MODE, 3, true, 0, false, true, true>},
#define CPK_PACKED(S, GW, EMIT, DYN, MODE, SLOTS) \
    {KernelForm{kFamilyPacked, S, EMIT, MODE, false, 0, false, 0, SLOTS, DYN, GW}, cpecan_pairhmm_packed<S, GW, EMIT, DYN, MODE, SLOTS>},
#define CPK_TEAM(S, T, EMIT, SLOTS) \
    {KernelForm{kFamilyTeam, S, EMIT, kModeWhole, false, 0, false, 0, SLOTS, false, T}, cpecan_pairhmm_team<S, T, EMIT, SLOTS>},
#define CPK_SWEEP_F(S, ...) CPK_SWEEP(S, true, __VA_ARGS__) CPK_SWEEP(S, false, __VA_ARGS__)
#define CPK_PACKED_G(S, ...) CPK_PACKED(S, 8, __VA_ARGS__) CPK_PACKED(S, 16, __VA_ARGS__) CPK_PACKED(S, 32, __VA_ARGS__)
#define CPK_TEAM_T(S, ...) CPK_TEAM(S, 4, __VA_ARGS__) CPK_TEAM(S, 8, __VA_ARGS__)
#define CPK_BOTH(ROW, ...) ROW(3, __VA_ARGS__) ROW(5, __VA_ARGS__)
constexpr KernelEntry kKernelTable[] = {
    // one wave per region: every emitter; the expectation emitter with its events inside the traceback (LDS rows)
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_MATCH, kModeWhole, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_INDEL, kModeWhole, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP_F, kEmitForward, kModeWhole, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 1, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 2, false)
    // ... of reserved batches (model slots): expectation and forward emitters
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 0, true)
    CPK_BOTH(CPK_SWEEP_F, kEmitForward, kModeWhole, CPK_SWEEP_WAVES, false, 0, true)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 1, true)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_EXPECT, kModeWhole, CPK_SWEEP_WAVES, false, 2, true)
    // split classes (match emitter): forward launch, traceback launch, the one launch of both
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_MATCH, kModeForward, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_MATCH, kModeTrace, CPK_SWEEP_WAVES, false, 0, false)
    CPK_BOTH(CPK_SWEEP_F, CPECAN_EMIT_MATCH, kModeFused, CPK_SWEEP_WAVES, false, 0, false)
    // ... over absolute positions (LDS rows), for two and for three waves per SIMD
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeForward, CPK_SWEEP_WAVES, true, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeTrace, CPK_SWEEP_WAVES, true, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeFused, CPK_SWEEP_WAVES, true, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeForward, 3, true, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeTrace, 3, true, 0, false)
    CPK_BOTH(CPK_SWEEP, true, CPECAN_EMIT_MATCH, kModeFused, 3, true, 0, false)
    // ... the two launches at three waves per SIMD as gangs: workgroups of several waves, one copy of the tables
    CPK_BOTH(CPK_SWEEP_GANG, true, CPECAN_EMIT_MATCH, kModeForward, 3, true, 0, false, true)
    CPK_BOTH(CPK_SWEEP_GANG, true, CPECAN_EMIT_MATCH, kModeTrace, 3, true, 0, false, true)
    // ... and the gangs of a class with chains: a forward launch that stops behind a region's first segments, a traceback
    // launch whose items may sweep the later ones forward before they trace them back
    CPK_BOTH(CPK_SWEEP_CHAIN, kModeForward)
    CPK_BOTH(CPK_SWEEP_CHAIN, kModeTrace)
    // dense classes: the three-state match kernels for three waves per SIMD (the forward launch needs 70 VGPRs: one variant)
    CPK_SWEEP_F(3, CPECAN_EMIT_MATCH, kModeWhole, 3, false, 0, false)
    CPK_SWEEP_F(3, CPECAN_EMIT_MATCH, kModeTrace, 3, false, 0, false)
    CPK_SWEEP_F(3, CPECAN_EMIT_MATCH, kModeFused, 3, false, 0, false)
    // narrow classes, 64 / GW regions to a wave: fixed and per-anchor expansions; reserved batches; the two launches of a split class
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_MATCH, false, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_INDEL, false, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_EXPECT, false, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_MATCH, true, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_INDEL, true, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_EXPECT, true, kModeWhole, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_EXPECT, false, kModeWhole, true)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_EXPECT, true, kModeWhole, true)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_MATCH, false, kModeForward, false)
    CPK_BOTH(CPK_PACKED_G, CPECAN_EMIT_MATCH, false, kModeTrace, false)
    // a team of four or eight waves per region
    CPK_BOTH(CPK_TEAM_T, CPECAN_EMIT_MATCH, false)
    CPK_BOTH(CPK_TEAM_T, CPECAN_EMIT_INDEL, false)
    CPK_BOTH(CPK_TEAM_T, CPECAN_EMIT_EXPECT, false)
    CPK_BOTH(CPK_TEAM_T, CPECAN_EMIT_EXPECT, true)
};
#undef CPK_SWEEP
#undef CPK_SWEEP_GANG
#undef CPK_SWEEP_CHAIN
#undef CPK_PACKED
#undef CPK_TEAM
#undef CPK_SWEEP_F
#undef CPK_PACKED_G
#undef CPK_TEAM_T
#undef CPK_BOTH
// the kernel of a form; nullptr: no such variant is built
constexpr KernelFn kernel_of(const KernelForm &f) {
    for (const KernelEntry &e : kKernelTable)
        if (e.form == f) return e.fn;
    return nullptr;
}
constexpr bool table_lists_no_form_twice() {
    for (const KernelEntry &a : kKernelTable)
        for (const KernelEntry &b : kKernelTable)
            if (&a != &b && a.form == b.form) return false;
    return true;
}
static_assert(table_lists_no_form_twice(), "kKernelTable: a form is listed twice");
// A wide class with one wave per region, from its geometry (slots: a reserved batch; inSweep 1: no diagonal wider than
// one 64-lane group); the narrow class k (groups of 8 << k lanes) as whole regions; a team of waves in place of `solo`.
constexpr KernelForm wide_form(const CpkGeometry &g, bool slots) {
    const bool fast = !g.useGlobalRoll;
    const int inSweep = (g.emit == CPECAN_EMIT_EXPECT && fast && g.expInSweep) ? (g.expInSweep == 1 ? 1 : 2) : 0;
    return KernelForm{kFamilySweep, g.nStates == 5 ? 5 : 3, g.emit, kModeWhole, fast, CPK_SWEEP_WAVES, false, inSweep, slots, false, 0};
}
constexpr KernelForm packed_form(const CpkGeometry &g, int k, bool dynamic, bool slots) {
    return KernelForm{kFamilyPacked, g.nStates == 5 ? 5 : 3, g.emit, kModeWhole, false, 0, false, 0, slots, dynamic, 8 << k};
}
constexpr KernelForm team_form(const KernelForm &solo, int teamWaves) {
    return KernelForm{kFamilyTeam, solo.S, solo.emit, kModeWhole, false, 0, false, 0, solo.slots, false, teamWaves};
}
// `f` in another mode, with the registers that mode takes unless the plan asks for more (take_three_waves): in a dense class the
// three-state kernels are the builds for three waves per SIMD, except the forward launch, which has one build; ABS: split modes only.
constexpr KernelForm with_mode(KernelForm f, int mode, bool dense) {
    f.mode = mode;
    if (f.family == kFamilySweep) f.wps = (dense && f.S == 3 && mode != kModeForward) ? 3 : CPK_SWEEP_WAVES;
    if (mode == kModeWhole) f.abs = false;
    return f;
}
// Every form the plan can ask for has a kernel, or is one of the combinations plan_batch answers "no kernel" to.
constexpr bool has_kernel(const KernelForm &f) { return kernel_of(f) != nullptr; }
constexpr bool split_forms_have_kernels(const KernelForm &whole, bool dense) {  // of a match class
    for (int abs = 0; abs <= (whole.fast ? 1 : 0); abs++)
        for (int mode = kModeForward; mode <= (whole.family == kFamilySweep ? kModeFused : kModeTrace); mode++) {
            KernelForm s = whole;
            s.abs = abs != 0;
            s = with_mode(s, mode, dense);
            if (!has_kernel(s)) return false;
            s.wps = 3;  // the requests for three waves per SIMD: the forward launch; a five-state traceback or one launch
            if (abs && (mode == kModeForward || s.S == 5) && !has_kernel(s)) return false;
            s.gang = true;  // ... and their gangs: the two launches (take_gang)
            if (abs && mode != kModeFused && !has_kernel(s)) return false;
            s.chain = true;  // ... and the chains of those gangs (plan_chains)
            if (abs && mode != kModeFused && !has_kernel(s)) return false;
        }
    return true;
}
constexpr bool planned_forms_have_kernels(int S) {
    for (int e = 0; e < 4 * 12; e++) {  // emitter x model slots x LDS or global rows x in-sweep events 0 / 1 / 2; ... x fixed or per-anchor expansions x narrow class 0..2
        const int emit = e / 12, v = e % 12;
        const bool slots = v >= 6, odd = v & 1;
        CpkGeometry g{};
        g.nStates = S, g.emit = emit, g.useGlobalRoll = odd, g.expInSweep = v % 6 / 2;
        const KernelForm f = wide_form(g, slots), p = packed_form(g, v % 6 / 2, odd, slots);
        // reserved batches: expectation and forward emitters only; no forward-only packed kernel (such a batch has no narrow class)
        const bool built = !slots || emit == CPECAN_EMIT_EXPECT || emit == kEmitForward;
        if (has_kernel(f) != built || has_kernel(p) != (built && emit != kEmitForward)) return false;
        if (built && emit != kEmitForward && !(has_kernel(team_form(f, 4)) && has_kernel(team_form(f, 8)))) return false;
        if (emit != CPECAN_EMIT_MATCH || slots) continue;
        if (!odd && !split_forms_have_kernels(p, false)) return false;
        for (int dense = 0; dense <= (S == 3 ? 1 : 0); dense++)
            if (!has_kernel(with_mode(f, kModeWhole, dense != 0)) || !split_forms_have_kernels(f, dense != 0)) return false;
    }
    return true;
}
static_assert(planned_forms_have_kernels(3) && planned_forms_have_kernels(5), "a form the plan asks for has no kernel in kKernelTable");

// The form words of a class's CPECAN_TRACE_HOST line (tests, tools/soak_*.py and earlier records parse them), from the
// form of its first launch; dense is the plan's decision for the class, not the WPS of one launch.
static std::string form_words(const KernelForm &f, bool dense) {
    const char *launches = f.mode == kModeFused ? "one launch" : f.mode != kModeWhole ? "two launches" : "one wave per region";
    if (f.mode == kModeWhole && f.family == kFamilyPacked) launches = "whole regions";
    if (f.family == kFamilyTeam) launches = f.width > 4 ? "a team of waves per region (eight)" : "a team of waves per region (four)";
    return std::string(launches) + (f.family == kFamilySweep && !f.fast ? ", rolling rows in global memory" : "") + (f.abs ? ", absolute positions" : "") +
           (dense ? ", three waves per SIMD" : "") + (f.inSweep ? ", expectation events inside the traceback" : "");
}
