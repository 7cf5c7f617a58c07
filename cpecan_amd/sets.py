"""ctypes mirror of include/cpecan_sets.h: sets of sequence fragments, every chosen pair of every set aligned in one anchor
batch and one DP batch (the pairwise stage of impl/multipleAligner.c:653-681, :722-770, :903-933).

    with Sets(api.stateMachine5_construct(), p) as s:
        for end, frags in ends:                        # any number of sets
            for seq, left, right in frags:
                s.add_fragment(end, seq, left, right)
        quints, offsets, similarity = s.align(s.pairs(ALL))
"""
import ctypes as C

import numpy as np

from . import api

# Every symbol include/cpecan_sets.h declares (checked by tests/test_sets_cpu.py).
EXPORTS = [
    "cpecan_sets_options_default", "cpecan_sets_create", "cpecan_sets_destroy", "cpecan_sets_add_fragment",
    "cpecan_sets_pairs", "cpecan_sets_align", "cpecan_sets_result_pairs", "cpecan_sets_result_offsets",
    "cpecan_sets_result_similarity", "cpecan_sets_result_timing", "cpecan_sets_result_free", "cpecan_similarity_score",
    "cpecan_batch_set_quintuples", "cpecan_batch_quintuples",
]

ALL, REFERENCE = 0, 1  # CPECAN_SETS_*


class SetsOptions(C.Structure):
    """cpecan_sets_options."""
    _fields_ = [("gapGamma", C.c_float), ("reserved", C.c_int32), ("constraintDiagonalTrim", C.c_int64),
                ("anchorMatrixBiggerThanThis", C.c_int64), ("repeatMaskMatrixBiggerThanThis", C.c_int64)]


class SetsTiming(C.Structure):
    """cpecan_sets_timing (milliseconds)."""
    _fields_ = [(k, C.c_double) for k in ("anchorMs", "packMs", "dpKernelMs", "stageMs", "downloadMs", "totalMs")]

    def as_dict(self):
        return {k: float(getattr(self, k)) for k, _ in self._fields_}


_bound = False


def _lib():
    global _bound
    L = api.lib()
    if not _bound:
        vp, i64p, i32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        L.cpecan_sets_options_default.argtypes = [C.POINTER(SetsOptions)]
        L.cpecan_sets_create.argtypes = [C.POINTER(vp), C.POINTER(api.StateMachine), C.POINTER(api.PairwiseAlignmentParameters),
                                         C.POINTER(SetsOptions), C.c_int]
        L.cpecan_sets_destroy.argtypes = [vp]
        L.cpecan_sets_destroy.restype = None
        L.cpecan_sets_add_fragment.argtypes = [vp, C.c_int64, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
        L.cpecan_sets_add_fragment.restype = C.c_int64
        L.cpecan_sets_pairs.argtypes = [vp, C.c_int, i64p, C.c_int64]
        L.cpecan_sets_pairs.restype = C.c_int64
        L.cpecan_sets_align.argtypes = [vp, i64p, C.c_int64, C.POINTER(vp)]
        L.cpecan_sets_result_pairs.argtypes = [vp, C.POINTER(i32p), i64p]
        L.cpecan_sets_result_offsets.argtypes = [vp, C.POINTER(i64p), i64p]
        L.cpecan_sets_result_similarity.argtypes = [vp, C.POINTER(i64p), i64p]
        L.cpecan_sets_result_timing.argtypes = [vp, C.POINTER(SetsTiming)]
        L.cpecan_sets_result_free.argtypes = [vp]
        L.cpecan_sets_result_free.restype = None
        L.cpecan_batch_set_quintuples.argtypes = [vp, i32p, C.c_int64]
        L.cpecan_batch_quintuples.argtypes = [vp, C.POINTER(i32p), C.POINTER(i64p), C.POINTER(i64p)]
        _bound = True
    return L


def sets_options(**overrides):
    """The reference's defaults (0.5f, 14, 500 * 500, 500 * 500); keyword overrides name fields of cpecan_sets_options."""
    o = SetsOptions()
    api._check(_lib().cpecan_sets_options_default(C.byref(o)), "cpecan_sets_options_default")
    for k, v in overrides.items():
        if k == "reserved" or not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _pair_array(pairs):
    a = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    n = a.shape[0]
    if n == 0:
        a = np.zeros((1, 2), dtype=np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64)), n


class Sets:
    """cpecan_sets.  anchoring: constraintDiagonalTrim, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis."""

    def __init__(self, sM, p=None, gapGamma=0.5, device=0, **anchoring):
        self._h = C.c_void_p()
        self._sM = sM
        self._p = p or api.pairwiseAlignmentBandingParameters_construct()
        self._o = sets_options(gapGamma=gapGamma, **anchoring)
        self.n = 0
        self.timing = None  # of the last align()
        api._check(_lib().cpecan_sets_create(C.byref(self._h), C.byref(sM), C.byref(self._p), C.byref(self._o), device),
                   "cpecan_sets_create")

    def close(self):
        if self._h:
            _lib().cpecan_sets_destroy(self._h)
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

    def add_fragment(self, set_id, seq, leftEndId=0, rightEndId=0):
        """Copies seq as a fragment of set `set_id`; returns its global index."""
        s = api._bytes(seq)
        idx = api._check(_lib().cpecan_sets_add_fragment(self._h, int(set_id), s, len(s), int(leftEndId), int(rightEndId)),
                         "cpecan_sets_add_fragment")
        self.n += 1
        return idx

    def pairs(self, mode=ALL, cap=None):
        """cpecan_sets_pairs: int64[nPairs, 2] of global indices (at most `cap` of them when cap is given)."""
        L = _lib()
        n = api._check(L.cpecan_sets_pairs(self._h, int(mode), None, 0), "cpecan_sets_pairs")
        want = n if cap is None else min(n, int(cap))
        out = np.zeros((max(1, want), 2), dtype=np.int64)
        api._check(L.cpecan_sets_pairs(self._h, int(mode), out.ctypes.data_as(C.POINTER(C.c_int64)), want), "cpecan_sets_pairs")
        return out[:want]

    def align(self, pairs):
        """cpecan_sets_align: (int32[n, 5] records (score, seq1, pos1, seq2, pos2), int64[nPairs + 1] offsets,
        int64[nPairs] similarity scores); pair k is aligned with X = pairs[k][0], Y = pairs[k][1] as given."""
        L = _lib()
        a, ptr, n = _pair_array(pairs)
        r = C.c_void_p()
        api._check(L.cpecan_sets_align(self._h, ptr, n, C.byref(r)), "cpecan_sets_align")
        try:
            q, off, sim = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
            nq, m = C.c_int64(), C.c_int64()
            api._check(L.cpecan_sets_result_pairs(r, C.byref(q), C.byref(nq)), "cpecan_sets_result_pairs")
            api._check(L.cpecan_sets_result_offsets(r, C.byref(off), C.byref(m)), "cpecan_sets_result_offsets")
            api._check(L.cpecan_sets_result_similarity(r, C.byref(sim), C.byref(m)), "cpecan_sets_result_similarity")
            t = SetsTiming()
            api._check(L.cpecan_sets_result_timing(r, C.byref(t)), "cpecan_sets_result_timing")
            self.timing = t.as_dict()
            quints = np.zeros((0, 5), dtype=np.int32)
            if nq.value:
                quints = np.ctypeslib.as_array(q, shape=(nq.value * 5,)).copy().reshape(nq.value, 5)
            offsets = np.ctypeslib.as_array(off, shape=(m.value + 1,)).copy()
            similarity = np.ctypeslib.as_array(sim, shape=(m.value,)).copy() if m.value else np.zeros(0, dtype=np.int64)
            return quints, offsets, similarity
        finally:
            L.cpecan_sets_result_free(r)


def batch_set_quintuples(batch, names):
    """cpecan_batch_set_quintuples on an api.Batch: names int32[nProblems, 2], or None to switch the stage off."""
    if names is None:
        api._check(_lib().cpecan_batch_set_quintuples(batch._h, None, 0), "cpecan_batch_set_quintuples")
        return
    a = np.ascontiguousarray(np.asarray(names, dtype=np.int32).reshape(-1, 2))
    api._check(_lib().cpecan_batch_set_quintuples(batch._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0]),
               "cpecan_batch_set_quintuples")


def batch_quintuples(batch):
    """cpecan_batch_quintuples after download(): (int32[n, 5], int64[nProblems + 1], int64[nProblems] score sums)."""
    q, off, sums = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
    api._check(_lib().cpecan_batch_quintuples(batch._h, C.byref(q), C.byref(off), C.byref(sums)), "cpecan_batch_quintuples")
    m = batch.n
    offsets = np.ctypeslib.as_array(off, shape=(m + 1,)).copy()
    n = int(offsets[m])
    quints = np.ctypeslib.as_array(q, shape=(max(n, 1) * 5,)).copy().reshape(-1, 5)[:n]
    return quints, offsets, (np.ctypeslib.as_array(sums, shape=(m,)).copy() if m else np.zeros(0, dtype=np.int64))
