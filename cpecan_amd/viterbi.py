"""ctypes mirror of include/cpecan_viterbi.h: Viterbi decoding -- the most probable banded state path of two sequences under
a pair-HMM and its log-probability -- on the GPU.

    r = viterbi_path(api.stateMachine5_construct(), sx, sy, anchors, p)
    r.logP                     # the plain sum of the regions' logP
    r.regions                  # Region tuples: x1 y1 x2 y2 logP startState endState opOff nOps
    r.ops                      # int32[nOps, 2]: (state, length), maximal runs, first step first
    pairs_of(r)                # int64[n, 2]: (x, y) of every match step, problem coordinates, 0-based

    with Viterbi(sM, p) as v:  # many problems, as few launches as the budget allows
        v.add_many(problems)   # (sx, sy, anchors[, ragged_left, ragged_right])
        v.run()
        results = [v.result(i) for i in range(v.n)]

Viterbi training's E-step: the transitions and emissions along the decoded paths, counted on the GPU
over inputs that stay there from the first call on; only the model goes down and the bins come up.

    with Viterbi(sM, p) as v:
        v.add_many(problems)
        c = v.run_counts()     # Counts: transitions int64[S, S], emissions int64[S, 16], nSteps, nNoPath, logP
        v.set_model(other)     # same state count; the resident inputs stay
        c = v.run_counts()
    counts_of_ops(S, sx, sy, start_state, ops)   # the same count over one region's ops, on the host
    counts_add_to_hmm(c, hmm)                    # into an api.Hmm accumulator, exactly
"""
import collections
import ctypes as C

import numpy as np

from . import api

# Every symbol include/cpecan_viterbi.h declares (checked by tests/test_viterbi_cpu.py).
EXPORTS = [
    "cpecan_viterbi_create", "cpecan_viterbi_destroy", "cpecan_viterbi_add", "cpecan_viterbi_set_budget",
    "cpecan_viterbi_set_form", "cpecan_viterbi_run", "cpecan_viterbi_launch_forms", "cpecan_viterbi_info",
    "cpecan_viterbi_result", "cpecan_viterbi_kernel_ms", "cpecan_viterbi_replay", "cpecan_viterbi_pairs",
    "cpecan_viterbi_set_model", "cpecan_viterbi_run_counts", "cpecan_viterbi_resident_bytes",
    "cpecan_viterbi_set_keep_problem_counts", "cpecan_viterbi_problem_counts", "cpecan_viterbi_count_ms",
    "cpecan_viterbi_counts_of_ops", "cpecan_viterbi_counts_add_to_hmm",
]

MAX_BYTES = 4 << 30  # CPECAN_VITERBI_MAX_BYTES
FORM_AUTO, FORM_LDS, FORM_GLOBAL = 0, 1, 2  # CPECAN_VITERBI_FORM_*
FORMS = (FORM_LDS, FORM_GLOBAL)
LDS_MAX_WIDTH = 256  # CPECAN_VITERBI_LDS_MAX_WIDTH
# The traceback stages the pointer bytes of this many diagonals in LDS at a time (CPK_VIT_BLOCK_DIAGS).
TRACEBACK_BLOCK_DIAGONALS = 64


class ViterbiInfo(C.Structure):
    """cpecan_viterbi_info_t."""
    _fields_ = [(k, C.c_int64) for k in ("nRegions", "nCells", "nStates", "deviceBytes")]


class ViterbiRegion(C.Structure):
    """cpecan_viterbi_region."""
    _fields_ = [("x1", C.c_int64), ("y1", C.c_int64), ("x2", C.c_int64), ("y2", C.c_int64), ("logP", C.c_double),
                ("startState", C.c_int32), ("endState", C.c_int32), ("opOff", C.c_int64), ("nOps", C.c_int64)]


class ViterbiResult(C.Structure):
    """cpecan_viterbi_result_t: borrowed host pointers."""
    _fields_ = [("logP", C.c_double), ("nRegions", C.c_int64), ("nOps", C.c_int64), ("regions", C.POINTER(ViterbiRegion)),
                ("ops", C.POINTER(C.c_int32))]


class ViterbiCounts(C.Structure):
    """cpecan_viterbi_counts."""
    _fields_ = [("transitions", C.c_int64 * 25), ("emissions", C.c_int64 * 80), ("nSteps", C.c_int64), ("nNoPath", C.c_int64),
                ("nStates", C.c_int64), ("logP", C.c_double)]


# transitions int64[S, S] (from, to); emissions int64[S, 16] (state, cX * 4 + cY)
Counts = collections.namedtuple("Counts", "transitions emissions nSteps nNoPath logP")
Region = collections.namedtuple("Region", "x1 y1 x2 y2 logP startState endState opOff nOps")
Result = collections.namedtuple("Result", "logP regions ops")
LaunchForms = collections.namedtuple("LaunchForms", "launches lds global_")

_bound = False


def _lib():
    global _bound
    L = api.lib()
    if not _bound:
        vp, i64p, i32p, dp = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        L.cpecan_viterbi_create.argtypes = [C.POINTER(vp), C.POINTER(api.StateMachine), C.POINTER(api.PairwiseAlignmentParameters),
                                            C.c_int]
        L.cpecan_viterbi_destroy.argtypes = [vp]
        L.cpecan_viterbi_destroy.restype = None
        L.cpecan_viterbi_add.argtypes = [vp, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, i64p, C.c_int64, C.c_int, C.c_int]
        L.cpecan_viterbi_add.restype = C.c_int64
        L.cpecan_viterbi_set_budget.argtypes = [vp, C.c_int64]
        L.cpecan_viterbi_set_form.argtypes = [vp, C.c_int]
        L.cpecan_viterbi_run.argtypes = [vp]
        L.cpecan_viterbi_launch_forms.argtypes = [vp, i64p, i64p, i64p]
        L.cpecan_viterbi_info.argtypes = [vp, C.c_int64, C.POINTER(ViterbiInfo)]
        L.cpecan_viterbi_result.argtypes = [vp, C.c_int64, C.POINTER(ViterbiResult)]
        L.cpecan_viterbi_kernel_ms.argtypes = [vp, dp, dp]
        L.cpecan_viterbi_replay.argtypes = [C.POINTER(api.StateMachine), C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int, C.c_int,
                                            C.c_int, C.c_int, i32p, C.c_int64, dp]
        L.cpecan_viterbi_pairs.argtypes = [C.POINTER(ViterbiResult), i64p, C.c_int64]
        L.cpecan_viterbi_pairs.restype = C.c_int64
        # a library built before the counts (CPECAN_LIB, the A/B runs of tools/) has the decoding half only: its plain run works
        if hasattr(L, "cpecan_viterbi_run_counts"):
            _bind_counts(L)
        _bound = True
    return L


def _bind_counts(L):
    vp, i64p, i32p, dp = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cp = C.POINTER(ViterbiCounts)
    L.cpecan_viterbi_set_model.argtypes = [vp, C.POINTER(api.StateMachine)]
    L.cpecan_viterbi_run_counts.argtypes = [vp, cp]
    L.cpecan_viterbi_resident_bytes.argtypes = [vp, i64p, i64p]
    L.cpecan_viterbi_set_keep_problem_counts.argtypes = [vp, C.c_int]
    L.cpecan_viterbi_problem_counts.argtypes = [vp, C.c_int64, cp]
    L.cpecan_viterbi_count_ms.argtypes = [vp, dp, dp]
    L.cpecan_viterbi_counts_of_ops.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int, i32p, C.c_int64, cp]
    L.cpecan_viterbi_counts_add_to_hmm.argtypes = [cp, C.POINTER(api.Hmm)]


class Viterbi:
    """cpecan_viterbi: problems added one by one, all of them run in as few launches as the budget allows."""

    def __init__(self, sM, p=None, device=0):
        self._h = C.c_void_p()
        self._sM = sM
        self._p = p or api.pairwiseAlignmentBandingParameters_construct()
        self.n = 0
        api._check(_lib().cpecan_viterbi_create(C.byref(self._h), C.byref(sM), C.byref(self._p), device), "cpecan_viterbi_create")

    def close(self):
        if self._h:
            _lib().cpecan_viterbi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, sx, sy, anchors=(), ragged_left=False, ragged_right=False):
        """Copies the problem; returns its index."""
        x, y = api._bytes(sx), api._bytes(sy)
        a, ptr, n = api._anchor_array(anchors)
        idx = api._check(_lib().cpecan_viterbi_add(self._h, x, len(x), y, len(y), ptr, n, int(ragged_left), int(ragged_right)),
                         "cpecan_viterbi_add")
        self.n += 1
        return idx

    def add_many(self, problems):
        """problems: (sx, sy, anchors[, ragged_left, ragged_right]) each; returns their indices."""
        return [self.add(*q) for q in problems]

    def set_budget(self, nbytes):
        api._check(_lib().cpecan_viterbi_set_budget(self._h, int(nbytes)), "cpecan_viterbi_set_budget")

    def set_form(self, form):
        api._check(_lib().cpecan_viterbi_set_form(self._h, int(form)), "cpecan_viterbi_set_form")

    def run(self):
        api._check(_lib().cpecan_viterbi_run(self._h), "cpecan_viterbi_run")

    def set_model(self, sM):
        """Another model of the same state count for the next run; what run_counts keeps on the device stays."""
        api._check(_lib().cpecan_viterbi_set_model(self._h, C.byref(sM)), "cpecan_viterbi_set_model")
        self._sM = sM

    def set_keep_problem_counts(self, on=True):
        api._check(_lib().cpecan_viterbi_set_keep_problem_counts(self._h, int(bool(on))), "cpecan_viterbi_set_keep_problem_counts")

    def run_counts(self):
        """Decodes every region and counts along the paths on the device (Counts of all problems); the inputs stay there."""
        c = ViterbiCounts()
        api._check(_lib().cpecan_viterbi_run_counts(self._h, C.byref(c)), "cpecan_viterbi_run_counts")
        return _counts(c)

    def problem_counts(self, problem):
        """Counts of one problem of the last run_counts (set_keep_problem_counts must be on)."""
        c = ViterbiCounts()
        api._check(_lib().cpecan_viterbi_problem_counts(self._h, int(problem), C.byref(c)), "cpecan_viterbi_problem_counts")
        return _counts(c)

    def resident_bytes(self):
        """(bytes of the inputs run_counts keeps on the device, bytes of the one scratch beside them)."""
        a, b = C.c_int64(), C.c_int64()
        api._check(_lib().cpecan_viterbi_resident_bytes(self._h, C.byref(a), C.byref(b)), "cpecan_viterbi_resident_bytes")
        return a.value, b.value

    def count_ms(self):
        """(count, reduce) HIP-event milliseconds of the last run_counts."""
        a, b = C.c_double(), C.c_double()
        api._check(_lib().cpecan_viterbi_count_ms(self._h, C.byref(a), C.byref(b)), "cpecan_viterbi_count_ms")
        return a.value, b.value

    def launch_forms(self):
        """Of the last run: LaunchForms(launches, regions run in the LDS form, regions run in the global form)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        api._check(_lib().cpecan_viterbi_launch_forms(self._h, C.byref(a), C.byref(b), C.byref(c)), "cpecan_viterbi_launch_forms")
        return LaunchForms(a.value, b.value, c.value)

    def kernel_ms(self):
        """(sweep, traceback) HIP-event milliseconds of the last run."""
        a, b = C.c_double(), C.c_double()
        api._check(_lib().cpecan_viterbi_kernel_ms(self._h, C.byref(a), C.byref(b)), "cpecan_viterbi_kernel_ms")
        return a.value, b.value

    def info(self, problem):
        i = ViterbiInfo()
        api._check(_lib().cpecan_viterbi_info(self._h, int(problem), C.byref(i)), "cpecan_viterbi_info")
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def _raw(self, problem):
        r = ViterbiResult()
        api._check(_lib().cpecan_viterbi_result(self._h, int(problem), C.byref(r)), "cpecan_viterbi_result")
        return r

    def result(self, problem):
        """Copies of the problem's result (Result)."""
        return _copy(self._raw(problem))

    def pairs(self, problem):
        """cpecan_viterbi_pairs of the problem: int64[n, 2]."""
        r = self._raw(problem)
        n = api._check(_lib().cpecan_viterbi_pairs(C.byref(r), None, 0), "cpecan_viterbi_pairs")
        xy = np.zeros((max(n, 1), 2), dtype=np.int64)
        api._check(_lib().cpecan_viterbi_pairs(C.byref(r), xy.ctypes.data_as(C.POINTER(C.c_int64)), n), "cpecan_viterbi_pairs")
        return xy[:n]


def _copy(r):
    regions = tuple(Region(*(getattr(r.regions[i], k) for k in Region._fields)) for i in range(r.nRegions))
    ops = np.ctypeslib.as_array(r.ops, shape=(2 * r.nOps,)).copy().reshape(-1, 2) if r.nOps else np.zeros((0, 2), np.int32)
    return Result(float(r.logP), regions, ops.astype(np.int32, copy=False))


def _counts(c):
    S = int(c.nStates)
    return Counts(np.array(c.transitions[:S * S], dtype=np.int64).reshape(S, S), np.array(c.emissions[:S * 16], dtype=np.int64).reshape(S, 16),
                  int(c.nSteps), int(c.nNoPath), float(c.logP))


def _raw_counts(counts):
    S = counts.transitions.shape[0]
    c = ViterbiCounts()
    c.transitions[:S * S] = [int(t) for t in np.asarray(counts.transitions).reshape(-1)]
    c.emissions[:S * 16] = [int(t) for t in np.asarray(counts.emissions).reshape(-1)]
    c.nSteps, c.nNoPath, c.nStates, c.logP = int(counts.nSteps), int(counts.nNoPath), S, float(counts.logP)
    return c


def counts_of_ops(n_states, sx, sy, start_state, ops):
    """cpecan_viterbi_counts_of_ops over ONE region (sx, sy: the region's own stretch; ops first step first): Counts with
    logP 0.  Pure host code."""
    x, y = api._bytes(sx), api._bytes(sy)
    o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
    n = o.size // 2
    if n == 0:
        o = np.zeros(2, dtype=np.int32)
    c = ViterbiCounts()
    api._check(_lib().cpecan_viterbi_counts_of_ops(int(n_states), x, len(x), y, len(y), int(start_state),
                                                   o.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(c)), "cpecan_viterbi_counts_of_ops")
    return _counts(c)


def counts_add_to_hmm(counts, hmm):
    """cpecan_viterbi_counts_add_to_hmm: the Counts added to the api.Hmm in place."""
    c = _raw_counts(counts)
    api._check(_lib().cpecan_viterbi_counts_add_to_hmm(C.byref(c), C.byref(hmm)), "cpecan_viterbi_counts_add_to_hmm")
    return hmm


def viterbi_path(sM, sx, sy, anchors=(), p=None, raggedLeft=False, raggedRight=False, device=0):
    """The result of a batch of one (Result)."""
    with Viterbi(sM, p, device) as v:
        v.add(sx, sy, anchors, raggedLeft, raggedRight)
        v.run()
        return v.result(0)


def pairs_of(result):
    """cpecan_viterbi_pairs on a Result: int64[n, 2], the (x, y) of every match step, ascending, problem coordinates."""
    regs = (ViterbiRegion * max(1, len(result.regions)))(*[ViterbiRegion(*r) for r in result.regions])
    ops = np.ascontiguousarray(result.ops, dtype=np.int32).reshape(-1)
    if ops.size == 0:
        ops = np.zeros(2, dtype=np.int32)
    r = ViterbiResult(result.logP, len(result.regions), len(result.ops), regs, ops.ctypes.data_as(C.POINTER(C.c_int32)))
    n = api._check(_lib().cpecan_viterbi_pairs(C.byref(r), None, 0), "cpecan_viterbi_pairs")
    xy = np.zeros((max(n, 1), 2), dtype=np.int64)
    api._check(_lib().cpecan_viterbi_pairs(C.byref(r), xy.ctypes.data_as(C.POINTER(C.c_int64)), n), "cpecan_viterbi_pairs")
    return xy[:n]


def replay(sM, sx, sy, raggedLeft, raggedRight, startState, endState, ops):
    """cpecan_viterbi_replay over ONE region (sx, sy: the region's own stretch): the value of the path, accumulated in path order.
    Pure host code."""
    x, y = api._bytes(sx), api._bytes(sy)
    o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
    n = o.size // 2
    if n == 0:
        o = np.zeros(2, dtype=np.int32)
    v = C.c_double()
    api._check(_lib().cpecan_viterbi_replay(C.byref(sM), x, len(x), y, len(y), int(raggedLeft), int(raggedRight), int(startState),
                                            int(endState), o.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(v)),
               "cpecan_viterbi_replay")
    return v.value
