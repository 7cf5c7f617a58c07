"""ctypes mirror of include/cpecan_dense.h: dense forward / backward rows of a region -- every state of F and B for every band
cell and the total the reference hands its per-diagonal emitter -- computed on the GPU under the reference's traceback
schedule (impl/pairwiseAligner.c:756-877).

    rows = forward_backward(api.stateMachine5_construct(), sx, sy, anchors, p)
    rows.F[rows.cell_off[d] + k]          # the S forward values of cell k of diagonal d

    with Dense(sM, p) as d:                # many regions, one launch sequence
        for sx, sy, anchors in regions:
            d.add(sx, sy, anchors)
        d.run()
        rows = [d.rows(i) for i in range(d.n)]
"""
import collections
import ctypes as C

import numpy as np

from . import api

# Every symbol include/cpecan_dense.h declares (checked by tests/test_dense_cpu.py).
EXPORTS = [
    "cpecan_dense_create", "cpecan_dense_destroy", "cpecan_dense_add", "cpecan_dense_run", "cpecan_dense_info",
    "cpecan_dense_rows", "cpecan_dense_kernel_ms", "cpecan_dense_schedule",
]

MAX_BYTES = 1 << 30  # CPECAN_DENSE_MAX_BYTES


class DenseInfo(C.Structure):
    """cpecan_dense_info_t."""
    _fields_ = [(k, C.c_int64) for k in ("nDiagonals", "nCells", "nSegments", "nStates")]


class DenseRows(C.Structure):
    """cpecan_dense_rows_t: borrowed host pointers."""
    _fields_ = [("diags", C.POINTER(C.c_int32)), ("cellOff", C.POINTER(C.c_int64)), ("F", C.POINTER(C.c_double)),
                ("B", C.POINTER(C.c_double)), ("Bnext", C.POINTER(C.c_double)), ("bnextOff", C.POINTER(C.c_int64)),
                ("totalUsed", C.POINTER(C.c_double)), ("segs", C.POINTER(C.c_int32))]


# diags int32[nDiagonals, 2] (xmyL, width); cell_off int64[nDiagonals + 1]; F, B float64[nCells, S]; b_next float64[*, S]: the
# tracebacks' extra rows one after the other, row k at b_next_off[k]; total_used float64[nDiagonals]; segs int32[nSegments, 3]
# (tbPrev, dTop, tbFrom)
Rows = collections.namedtuple("Rows", "diags cell_off F B b_next total_used segs b_next_off")

# calls int64[nCalls, 8]: xay, seg, fLo, fHi, f2Lo, f2Hi, bLo, bHi (cpecan_dense_call)
Schedule = collections.namedtuple("Schedule", "segs calls")

_bound = False


def _lib():
    global _bound
    L = api.lib()
    if not _bound:
        vp, i64p, i32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        L.cpecan_dense_create.argtypes = [C.POINTER(vp), C.POINTER(api.StateMachine), C.POINTER(api.PairwiseAlignmentParameters),
                                          C.c_int]
        L.cpecan_dense_destroy.argtypes = [vp]
        L.cpecan_dense_destroy.restype = None
        L.cpecan_dense_add.argtypes = [vp, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, i64p, C.c_int64, C.c_int, C.c_int]
        L.cpecan_dense_add.restype = C.c_int64
        L.cpecan_dense_run.argtypes = [vp]
        L.cpecan_dense_info.argtypes = [vp, C.c_int64, C.POINTER(DenseInfo)]
        L.cpecan_dense_rows.argtypes = [vp, C.c_int64, C.POINTER(DenseRows)]
        L.cpecan_dense_kernel_ms.argtypes = [vp]
        L.cpecan_dense_kernel_ms.restype = C.c_double
        L.cpecan_dense_schedule.argtypes = [C.c_int64, C.c_int64, i64p, C.c_int64, C.POINTER(api.PairwiseAlignmentParameters),
                                            i32p, C.c_int64, i64p, i64p, C.c_int64, i64p]
        _bound = True
    return L


def _take(ptr, n, dtype, cols):
    if n == 0:
        return np.zeros((0, cols) if cols else (0,), dtype=dtype)
    a = np.ctypeslib.as_array(ptr, shape=(n * max(cols, 1),)).copy()
    return a.reshape(n, cols) if cols else a


class Dense:
    """cpecan_dense: problems added one by one, all of them run in one launch sequence."""

    def __init__(self, sM, p=None, device=0):
        self._h = C.c_void_p()
        self._sM = sM
        self._p = p or api.pairwiseAlignmentBandingParameters_construct()
        self.n = 0
        api._check(_lib().cpecan_dense_create(C.byref(self._h), C.byref(sM), C.byref(self._p), device), "cpecan_dense_create")

    def close(self):
        if self._h:
            _lib().cpecan_dense_destroy(self._h)
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
        idx = api._check(_lib().cpecan_dense_add(self._h, x, len(x), y, len(y), ptr, n, int(ragged_left), int(ragged_right)),
                         "cpecan_dense_add")
        self.n += 1
        return idx

    def run(self):
        api._check(_lib().cpecan_dense_run(self._h), "cpecan_dense_run")

    @property
    def kernel_ms(self):
        return float(_lib().cpecan_dense_kernel_ms(self._h))

    def info(self, problem):
        i = DenseInfo()
        api._check(_lib().cpecan_dense_info(self._h, int(problem), C.byref(i)), "cpecan_dense_info")
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def rows(self, problem):
        """Copies of the problem's rows as numpy arrays (Rows)."""
        i = self.info(problem)
        r = DenseRows()
        api._check(_lib().cpecan_dense_rows(self._h, int(problem), C.byref(r)), "cpecan_dense_rows")
        nd, nc, ns, S = i["nDiagonals"], i["nCells"], i["nSegments"], i["nStates"]
        if nd == 0:
            z = np.zeros((0, S))
            return Rows(np.zeros((0, 2), np.int32), np.zeros(1, np.int64), z, z.copy(), z.copy(), np.zeros(0),
                        np.zeros((0, 3), np.int32), np.zeros(1, np.int64))
        off = _take(r.bnextOff, ns + 1, np.int64, 0)
        return Rows(_take(r.diags, nd, np.int32, 2), _take(r.cellOff, nd + 1, np.int64, 0), _take(r.F, nc, np.float64, S),
                    _take(r.B, nc, np.float64, S), _take(r.Bnext, int(off[ns]), np.float64, S),
                    _take(r.totalUsed, nd, np.float64, 0), _take(r.segs, ns, np.int32, 3), off)


def forward_backward(sm, sx, sy, anchors=(), p=None, ragged_left=False, ragged_right=False, device=0):
    """The dense rows of one region (Rows)."""
    with Dense(sm, p, device) as d:
        d.add(sx, sy, anchors, ragged_left, ragged_right)
        d.run()
        return d.rows(0)


def schedule(lX, lY, anchors=(), p=None):
    """cpecan_dense_schedule: the tracebacks int32[nSegments, 3] and the emitter calls int64[lX + lY, 8] in the reference's
    order (Schedule).  Pure host code."""
    L = _lib()
    a, ptr, n = api._anchor_array(anchors)
    pp = C.byref(p) if p is not None else None
    ns, nc = C.c_int64(), C.c_int64()
    api._check(L.cpecan_dense_schedule(int(lX), int(lY), ptr, n, pp, None, 0, C.byref(ns), None, 0, C.byref(nc)),
               "cpecan_dense_schedule")
    segs = np.zeros((max(1, ns.value), 3), dtype=np.int32)
    calls = np.zeros((max(1, nc.value), 8), dtype=np.int64)
    api._check(L.cpecan_dense_schedule(int(lX), int(lY), ptr, n, pp, segs.ctypes.data_as(C.POINTER(C.c_int32)), ns.value,
                                       None, calls.ctypes.data_as(C.POINTER(C.c_int64)), nc.value, None),
               "cpecan_dense_schedule")
    return Schedule(segs[:ns.value], calls[:nc.value])
