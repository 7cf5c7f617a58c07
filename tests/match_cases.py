"""The form matrix and the inputs of the match-emitter tests (CPECAN_EMIT_MATCH on the sweep kernel: the headline path),
shared by the CPU suite (tests/test_match_cases_cpu.py: every row plans the kernel it names, the rows cover the kernel
table, the oracle alone meets the caps) and the GPU suite (tests/test_gpu_match.py: every row against the oracle and
against row W1).  Nothing here touches a device.

A row is a set of planning knobs (cpk_plan.inl, PlanKnobs) on top of BASE_ENV and the kernels the plan answers with for
a class of five-state and of three-state regions: the first launch and, for the two-launch form, the traceback launch.
Rows W1..G run with the rolling rows in LDS, rows GW1..GR4 are the same knobs at widths past the LDS edge, where the rows
roll in global memory and absolute positions do not exist.

A problem is (sX, sY, anchors, raggedLeft, raggedRight); a Case is a batch of problems under one model and one set of
parameters, as in indel_cases.py, and the oracle's lists of a problem are computed once per process."""
import collections
import ctypes as C
import functools
import random

import oracle_binding as ob
import table_cases as tc
from cpecan_amd import api
from table_cases import SHORT
from test_gang_plan_cpu import CU_LDS, CUS, FIELDS  # (the record of cpk_plan_describe is named there)

Case = collections.namedtuple("Case", "name mtype problems pkw")
# One kernel: mode (kModeWhole .. kModeFused), waves per SIMD of the build, absolute positions, gang
Kernel = collections.namedtuple("Kernel", "mode wps abs gang")
Row = collections.namedtuple("Row", "name knobs debug five three")  # five / three: (first launch, traceback launch or None)
MODE_WHOLE, MODE_FORWARD, MODE_TRACE, MODE_FUSED = 0, 1, 2, 3
FAMILY_SWEEP = 1
EMIT_MATCH = api.EMIT_MATCH
MTYPES = (0, 2)  # the default five-state and three-state models

BASE_ENV = {"CPECAN_PACKED": "0", "CPECAN_TEAM": "0", "CPECAN_GANG": "0", "CPECAN_TRACE_HOST": "1"}
# every other knob the plan, the table builders or the host's loops read is unset while a row runs
OTHER_KNOBS = ("CPECAN_MAX_WAVES_PER_CU", "CPECAN_PACKED_SPLIT", "CPECAN_PACKED_SPLIT_FROM", "CPECAN_PACKED_SHARE", "CPECAN_ABS",
               "CPECAN_ABS_WINDOWS", "CPECAN_SPLIT", "CPECAN_EXP_INSWEEP", "CPECAN_EXP_ONE_GROUP", "CPECAN_DENSE", "CPECAN_FUSED_SPIN",
               "CPECAN_FUSED3", "CPECAN_TRACE3", "CPECAN_FWD3", "CPECAN_MEM_BUDGET_MB", "CPECAN_SPLIT_BUDGET_FRAC", "CPECAN_FAST_WALK",
               "CPECAN_KEEP_RUNS", "CPECAN_TABLE_WAVE", "CPECAN_THREADS")


def _whole(wps):
    return (Kernel(MODE_WHOLE, wps, 0, 0), None)


def _two(fwd, trace, abs_=0, gang=0):
    return (Kernel(MODE_FORWARD, fwd, abs_, gang), Kernel(MODE_TRACE, trace, abs_, gang))


def _fused(wps, abs_=0):
    return (Kernel(MODE_FUSED, wps, abs_, 0), None)


def _knobs(**kw):
    return {"CPECAN_" + k: str(v) for k, v in kw.items()}


# ---- LDS rows.  debug: the row may run with debug buffers (a dense class cannot: plan_team_or_solo) ----
LDS_ROWS = (
    Row("W1", _knobs(SPLIT=0, DENSE=0), True, _whole(2), _whole(2)),
    Row("W2", _knobs(SPLIT=0, DENSE=1), False, _whole(2), _whole(3)),
    Row("R1", _knobs(SPLIT=1, ABS=0, DENSE=0), True, _two(2, 2), _two(2, 2)),
    Row("R2", _knobs(SPLIT=1, ABS=0, DENSE=1), False, _two(2, 2), _two(2, 3)),
    Row("R3", _knobs(SPLIT=2, ABS=0, DENSE=0), True, _fused(2), _fused(2)),
    Row("R4", _knobs(SPLIT=2, ABS=0, DENSE=1), False, _fused(2), _fused(3)),
    Row("A1", _knobs(SPLIT=1, FWD3=0, TRACE3=0, DENSE=0), True, _two(2, 2, 1), _two(2, 2, 1)),
    Row("A2", _knobs(SPLIT=1), True, _two(3, 3, 1), _two(3, 2, 1)),
    Row("A2d", _knobs(SPLIT=1, DENSE=1), False, _two(3, 3, 1), _two(2, 3, 1)),
    Row("A3", _knobs(SPLIT=2, FUSED3=0, DENSE=0), True, _fused(2, 1), _fused(2, 1)),
    Row("A4", _knobs(SPLIT=2), True, _fused(3, 1), _fused(2, 1)),
    Row("A4d", _knobs(SPLIT=2, DENSE=1), False, _fused(3, 1), _fused(3, 1)),
    Row("G", _knobs(SPLIT=1, GANG=2), True, _two(3, 3, 1, 1), _two(3, 3, 1, 1)),
)
# ---- the same knobs past the LDS edge: rows in global memory, no absolute positions ----
GLOBAL_ROWS = (
    Row("GW1", _knobs(SPLIT=0, DENSE=0), True, _whole(2), _whole(2)),
    Row("GW2", _knobs(SPLIT=0, DENSE=1), False, _whole(2), _whole(3)),
    Row("GR1", _knobs(SPLIT=1, ABS=0, DENSE=0), True, _two(2, 2), _two(2, 2)),
    Row("GR2", _knobs(SPLIT=1, ABS=0, DENSE=1), False, _two(2, 2), _two(2, 3)),
    Row("GR3", _knobs(SPLIT=2, ABS=0, DENSE=0), True, _fused(2), _fused(2)),
    Row("GR4", _knobs(SPLIT=2, ABS=0, DENSE=1), False, _fused(2), _fused(3)),
)
ROWS = {r.name: r for r in LDS_ROWS + GLOBAL_ROWS}
QUEUE_ROWS = ("W1", "W2", "R1", "R2", "R3", "A2", "A2d", "A4d")
# A build for three waves per SIMD of a five-state class is tried where the class's LDS lets nine waves onto a CU
# (cpk_plan.inl, kThreeWpsLdsWaves): a wider five-state class of the same row keeps the builds for two.
THREE_WPS_LDS_WAVES = 9


def states(mtype):
    return 5 if mtype in (0, 1) else 3


def expected(row, mtype):
    r = ROWS[row] if isinstance(row, str) else row
    return r.five if states(mtype) == 5 else r.three


def set_row(monkeypatch, row, **extra):
    """The environment of a row: BASE_ENV, the row's knobs on top, every other knob unset."""
    r = ROWS[row] if isinstance(row, str) else row
    env = dict(BASE_ENV, **r.knobs)
    env.update(extra)
    for k in OTHER_KNOBS + tuple(BASE_ENV):
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- the plan: without a device (cpk_batch_launch_plan) and of an uploaded batch (cpk_batch_launch_forms) ----
def sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


def _records(out, n):
    return [dict(zip(FIELDS, out[i * len(FIELDS):(i + 1) * len(FIELDS)])) for i in range(n)]


def cpu_plan(case):
    """The launch classes cpecan_batch_upload would plan for the case on a device of 256 CUs that is not there."""
    f = api.lib().cpk_batch_launch_plan
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int]
    f.restype = C.c_int
    out = (C.c_int64 * (len(FIELDS) * 16))()
    with api.Batch(sm(case.mtype), api.pairwiseAlignmentBandingParameters_construct(**case.pkw)) as b:
        b.add_many(case.problems)
        n = f(b._h, CUS, 288 << 30, out, 16)
        assert n >= 0, api.lib().cpecan_last_error()
    return _records(out, n)


def uploaded_plan(batch):
    """The launch classes an uploaded batch really got: planned with the registers the loaded kernels report."""
    f = api.lib().cpk_batch_launch_forms
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int]
    f.restype = C.c_int
    out = (C.c_int64 * (len(FIELDS) * 16))()
    n = f(batch._h, out, 16)
    assert n >= 0, api.lib().cpecan_last_error()
    return _records(out, n)


KERNEL_FIELDS = ("family", "S", "emit", "mode", "fast", "wps", "abs", "inSweep", "slots", "dynamic", "width", "gang")


def kernel_table():
    """cpk_kernel_table.inl's kKernelTable as a list of dicts, one per built variant."""
    f = api.lib().cpk_kernel_table_forms
    f.argtypes = [C.POINTER(C.c_int64), C.c_int]
    f.restype = C.c_int
    out = (C.c_int64 * (len(KERNEL_FIELDS) * 1024))()
    n = f(out, 1024)
    assert n > 0
    return [dict(zip(KERNEL_FIELDS, out[i * len(KERNEL_FIELDS):(i + 1) * len(KERNEL_FIELDS)])) for i in range(n)]


def class_kernels(c):
    """(first launch, traceback launch or None) of a class record, as Kernels."""
    first = Kernel(c["mode"], c["wps"], c["abs"], c["gang"])
    return first, (Kernel(MODE_TRACE, c["traceWps"], c["abs"], c["traceGang"]) if c["mode"] == MODE_FORWARD else None)


def class_expectation(row, mtype, c, max_waves_per_cu=None):
    """What the row asks of class c: the row's kernels where the class has room for them.  A build for three waves per
    SIMD is taken only where it puts more waves on a CU than the build for two (cpk_plan.inl, take_three_waves): eight
    by its registers, so the class's LDS -- read off the record -- must let nine on, and so must CPECAN_MAX_WAVES_PER_CU
    where a case sets it.  A class without that room keeps the row's form with the builds for two.  A gang needs no such
    room (CPECAN_GANG=n forces it).  One promotion: in a dense class (three states, CPECAN_DENSE=1) the forward launch,
    which has a single three-wave build, takes it where its smaller LDS puts more waves on a CU than the class has.  (All
    of this is the plan without a device, which takes a build to use the registers it is allowed; DEVICE_EXPECTED names
    the one row the loaded kernels' registers plan otherwise.)"""
    first, trace = expected(row, mtype)
    cap = max_waves_per_cu if max_waves_per_cu else 32

    def waves(wps, lds):
        return min(4 * wps, CU_LDS // lds, cap)

    def room(lds):
        return waves(3, lds) > waves(2, lds)

    if first.gang:
        return first, trace
    lds, lds_fwd = c["ldsBytes"], c["ldsBytesFwd"]
    if trace and trace.wps == 3 and not room(lds):
        trace = trace._replace(wps=2)
    if first.mode == MODE_FORWARD:
        dense = states(mtype) == 3 and trace.wps == 3 and first.wps == 2
        if first.wps == 3 and not room(lds_fwd):
            first = first._replace(wps=2)
        elif dense and first.abs and waves(3, lds_fwd) > waves(3, lds) and CU_LDS // lds_fwd >= THREE_WPS_LDS_WAVES:
            first = first._replace(wps=3)
    elif first.wps == 3 and not room(lds):
        first = first._replace(wps=2)
    return first, trace


# On the device, with no cap on the waves per CU: the loaded forward kernel for three waves per SIMD reports registers for
# four, more waves than a dense three-state class has, so row A2d runs that build in the forward launch of every class as well.
DEVICE_EXPECTED = {("A2d", 3): _two(3, 3, 1)}


def device_expectation(row, mtype, c, max_waves_per_cu=None):
    """class_expectation for the plan of an uploaded batch."""
    name = row if isinstance(row, str) else row.name
    if not max_waves_per_cu and (name, states(mtype)) in DEVICE_EXPECTED:
        return DEVICE_EXPECTED[(name, states(mtype))]
    return class_expectation(row, mtype, c, max_waves_per_cu)


def device_expected(row, mtype, max_waves_per_cu=None):
    """expected() for the plan of an uploaded batch: the row's kernels where a class has room for every build."""
    name = row if isinstance(row, str) else row.name
    return expected(row, mtype) if max_waves_per_cu else DEVICE_EXPECTED.get((name, states(mtype)), expected(row, mtype))


def form_keys(c):
    """The kernel-table keys (S, mode, fast, wps, abs, gang) of the launches of a class record."""
    fast = 0 if c["globalRows"] else 1
    return {(c["nStates"], k.mode, fast, k.wps, k.abs, k.gang) for k in class_kernels(c) if k}


# ---- the oracle's list of a problem: once per (model, problem, parameters), shared by every row, never modified ----
@functools.lru_cache(maxsize=None)
def _oracle(mtype, problem, pkw_items):
    sx, sy, a, rl, rr = problem
    out = ob.aligned_pairs(ob.model(mtype), sx, sy, a, ob.params(**dict(pkw_items)), rl, rr)
    out.setflags(write=False)
    return out


def oracle_lists(case):
    key = tuple(sorted(case.pkw.items()))
    if len(case.problems) > 64:  # the queue sets: the oracle's calls leave the interpreter lock, eight at a time
        import concurrent.futures
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            return list(pool.map(lambda p: _oracle(case.mtype, p, key), case.problems))
    return [_oracle(case.mtype, p, key) for p in case.problems]


def _even_at_least(x):
    return (x + 1) // 2 * 2


def pkw(threshold, widest):
    """A traceback every 42 diagonals (table_cases.SHORT) and an even expansion of at least half the widest diagonal: a
    diagonal is a traceback point only if it has at most 2 * diagonalExpansion + 1 cells (pairwiseAligner.c:792-793)."""
    return dict(threshold=threshold, diagonalExpansion=_even_at_least((widest + 1) // 2), **SHORT)


# ---- the LDS set ----
GAP = 17


@functools.lru_cache(maxsize=None)
def pair(width):
    """A pair of related sequences of width - 1 + GAP and width - 1 bases: sY is sX without GAP bases, one at a time and
    evenly spread, and with every 11th base replaced.  Unanchored, its widest diagonals -- GAP + 1 in a row -- have `width` cells."""
    m = width - 1
    sx = tc.seq(m + GAP, 7)
    drop = {(i + 1) * (m + GAP) // (GAP + 1) for i in range(GAP)}
    assert len(drop) == GAP
    sy = [c for i, c in enumerate(sx) if i not in drop]
    for i in range(5, len(sy), 11):
        sy[i] = "ACGT"[("ACGT".index(sy[i]) + 1) % 4]
    return sx, "".join(sy), ()


LDS_WIDTHS = (9, 64, 65, 129, 193, 257)
DEBUG_WIDTH = 129  # problem 0 of the width-129 batch runs with debug buffers
THRESHOLDS = (0.01, 0.0)
DEGENERATE = (("", "", (), False, False), ("ACGT", "", (), False, False))


def _raggedpair():
    sx, sy, a = pair(100)
    return (sx, sy, a, True, True)


@functools.lru_cache(maxsize=None)
def lds_case(mtype, threshold):
    """One batch per state count: the unanchored pairs of test_gpu_refresh_pass._pair (lX - lY = 17: 18 diagonals in a row
    have the full width) at widths 9, 64, 65, 129, 193 and 257 -- 9, 64 and 1 cells in the last 64-lane group, the 1 as the
    second, third, fourth and fifth group --, an empty problem, a one-sided one and a pair with both ragged ends set."""
    probs = tuple(pair(w) + (False, False) for w in LDS_WIDTHS) + DEGENERATE + (_raggedpair(),)
    return Case("match-lds-%d-%g" % (mtype, threshold), mtype, probs, pkw(threshold, max(LDS_WIDTHS)))


@functools.lru_cache(maxsize=None)
def debug_case(mtype, width, threshold=0.01):
    """A batch of its own whose problem 0 is the pair of `width`: the debug buffers of one problem."""
    return Case("match-debug-%d-%d" % (mtype, width), mtype, (pair(width) + (False, False),), pkw(threshold, width))


# ---- the global set ----
def _globalpair(width):
    return pair(width) + (False, False)


@functools.lru_cache(maxsize=None)
def global_case_at(mtype, width, threshold=0.01, second=True):
    """The pair of `width` cells and, with `second`, the pair 65 cells wider; one expansion, chosen for the wider."""
    probs = (_globalpair(width),) + ((_globalpair(width + 65),) if second else ())
    return Case("match-global-%d-%d-%g-%d" % (mtype, width, threshold, len(probs)), mtype, probs, pkw(threshold, width + 65))


@functools.lru_cache(maxsize=None)
def first_global_width(mtype, plan_whole):
    """The first width at which the whole-form class of one unanchored pair rolls in global memory, found by stepping the
    planner (plan_whole: case -> class records under row GW1's environment; the caller sets that environment)."""
    lo, hi = 256, 2048  # (LDS rows at 256 cells, global rows at 2048: asserted)
    assert not plan_whole(global_case_at(mtype, lo, second=False))[-1]["globalRows"]
    assert plan_whole(global_case_at(mtype, hi, second=False))[-1]["globalRows"]
    while hi - lo > 1:  # the LDS of a class grows with its width: one edge
        mid = (lo + hi) // 2
        if plan_whole(global_case_at(mtype, mid, second=False))[-1]["globalRows"]:
            hi = mid
        else:
            lo = mid
    return hi


# ---- the queue set ----
QUEUE_REGIONS = 320
QUEUE_EXPANSION = 64


def _queue_problems(mtype, n):
    rng = random.Random(5200 + mtype)
    probs = []
    for i in range(n):
        lx, ly = rng.randrange(40, 121), rng.randrange(40, 121)
        sx = tc.seq(lx, 5200 + i)
        sy = "".join(c if rng.random() < 0.85 else rng.choice("ACGT") for c in (sx + tc.seq(120, 9200 + i))[:ly])
        probs.append((sx, sy, (), False, False))
    return tuple(probs)


@functools.lru_cache(maxsize=None)
def queue_case(mtype, threshold=0.01):
    """320 short unanchored regions of 40 to 120 bases, expansion 64 (every diagonal a traceback point): under
    CPECAN_MAX_WAVES_PER_CU=1 a device has fewer waves than regions or items, so every wave takes a second one with the
    state of the first still in its registers and LDS.  With one wave per CU no build for three waves per SIMD puts more
    waves on a CU, so every row of this set runs the builds for two (class_expectation): dense_queue_case is the set
    that queues regions behind the builds for three."""
    return Case("match-queue-%d-%g" % (mtype, threshold), mtype, _queue_problems(mtype, QUEUE_REGIONS),
                dict(threshold=threshold, diagonalExpansion=QUEUE_EXPANSION, **SHORT))


QUEUE_ENV = {"CPECAN_MAX_WAVES_PER_CU": "1"}
# The builds for three waves per SIMD with a second region or item per wave.  The plan takes such a build only where it
# puts a ninth wave on a CU, so the fewest waves a device of 256 CUs gives it are 9 x 256 = 2304 (CPECAN_MAX_WAVES_PER_CU=9):
# 2400 regions of the same family queue 96 and more of them behind a wave that has run one, and three to four items each.
DENSE_QUEUE_REGIONS = 2400
DENSE_QUEUE_ENV = {"CPECAN_MAX_WAVES_PER_CU": "9"}
# (rows A2 and A4 leave CPECAN_DENSE unset, and a three-state class of this many regions is dense by the plan's own choice:
# they would be A2d and A4d, which for five states are A2 and A4 anyway)
DENSE_QUEUE_ROWS = ("W1", "W2", "R2", "R4", "A2d", "A4d")


@functools.lru_cache(maxsize=None)
def dense_queue_case(mtype, threshold=0.01):
    return Case("match-dense-queue-%d-%g" % (mtype, threshold), mtype, _queue_problems(mtype, DENSE_QUEUE_REGIONS),
                dict(threshold=threshold, diagonalExpansion=QUEUE_EXPANSION, **SHORT))
