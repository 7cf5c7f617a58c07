"""A Python restatement of the loop of getPosteriorProbsWithBanding (impl/pairwiseAligner.c:782-867) that does no arithmetic:
it tracks, literally, which rows of the forward and of the backward DpMatrix exist (dpMatrix_createDiagonal /
dpMatrix_deleteDiagonal) and records every call of the emitter with the two live sets at that moment.
cpecan_dense_schedule (include/cpecan_dense.h) is held against it integer for integer by tests/test_dense_cpu.py.

The dense path's contract differs from the reference's state in ONE row: at the call for xay the reference also holds
backward row xay - 2, half-accumulated (it has received the middle terms of xay only); the dense rows do not serve it."""
import collections

Call = collections.namedtuple("Call", "xay seg forward backward")  # forward / backward: frozensets of live rows


def reference_loop(width, min_between, tb_diagonals, expansion):
    """width[d], d = 0 .. N: cells of the band's diagonals.  Returns (segs [(tbPrev, dTop, tbFrom)], calls [Call]); N == 0: no
    rows, no call (:767-770)."""
    N = len(width) - 1
    if N <= 0:
        return [], []
    forward, backward = {0}, set()  # :776
    segs, calls = [], []
    traced_back_to = 0
    total_calculations = 0
    for d in range(1, N + 1):
        forward.add(d)  # :788
        at_end = d == N  # :791
        traceback_point = d >= traced_back_to + min_between and width[d] <= expansion * 2 + 1  # :792-793
        if not (at_end or traceback_point):
            continue
        backward.add(d)  # :798
        if d > traced_back_to + 1:  # :800-804
            assert d - 1 in forward
            backward.add(d - 1)
        traced_back_from = d - (0 if at_end else tb_diagonals + 1)  # :810
        segs.append((traced_back_to, d, traced_back_from))
        this_traceback = 0
        d2 = d
        while d2 > traced_back_to:  # :813
            if d2 > traced_back_to + 2:  # :815-819
                assert d2 - 2 in forward
                backward.add(d2 - 2)
            # :820-822 diagonalCalculationBackward(d2): no rows created or deleted
            if d2 <= traced_back_from:  # :823
                assert d2 in forward and d2 - 1 in forward and d2 in backward  # :824-826
                if d2 != N:
                    assert d2 + 1 in backward  # :827-829
                this_traceback += 1
                calls.append(Call(d2, len(segs) - 1, frozenset(forward), frozenset(backward)))  # :840
                if d2 < traced_back_from or at_end:  # :843-845
                    forward.discard(d2)
            if d2 + 1 <= N:  # :847-849
                backward.discard(d2 + 1)
            d2 -= 1
        traced_back_to = traced_back_from  # :852
        backward.discard(d2 + 1)  # :854
        forward.discard(d2)  # :855
        assert not backward  # :857
        total_calculations += this_traceback
        if not at_end:
            assert len(forward) == tb_diagonals + 2  # :860
    assert total_calculations == N and traced_back_to == N and not backward and not forward  # :868-871
    return segs, calls


def served_backward(call):
    """The backward rows the dense path serves at this call: the reference's, without the half-accumulated xay - 2."""
    return call.backward - {call.xay - 2}


def rows_of_call(c):
    """(forward rows, backward rows) of one record of cpecan_dense_schedule (xay, seg, fLo, fHi, f2Lo, f2Hi, bLo, bHi)."""
    xay, seg, f_lo, f_hi, f2_lo, f2_hi, b_lo, b_hi = (int(v) for v in c)
    return frozenset(range(f_lo, f_hi + 1)) | frozenset(range(f2_lo, f2_hi + 1)), frozenset(range(b_lo, b_hi + 1))
