"""The definition of the Viterbi counts (include/cpecan_viterbi.h) in numpy, over the regions and ops of
tests/viterbi_model.py: what cpecan_viterbi_counts_of_ops and cpk_viterbi.inl's count kernels must equal integer for integer,
and logP bit for bit.  Nothing here touches a GPU or the library.

    region(S, sx, sy, start_state, ops)  -> Counts of ONE region with a path (sx, sy: its own stretch), logP 0.0
    regions(S, model, inputs)            -> [Counts] per region of a viterbi_model.Model; inputs: viterbi_cases.region_inputs;
                                            a region without a path: no counts, nNoPath 1; otherwise logP the region's
    total(S, parts)                      -> Counts: the bins summed, logP = 0.0 + the logP of the parts that have a path, one
                                            after the other in the order given (the plain double sum)
"""
import collections

import numpy as np

import viterbi_model as vm

# transitions int64[S, S] (from, to); emissions int64[S, 16] (state, cX * 4 + cY)
Counts = collections.namedtuple("Counts", "transitions emissions nSteps nNoPath logP")

MOVES_X = (0, 1, 3)  # match, shortGapX, longGapX
MOVES_Y = (0, 2, 4)


def empty(S, n_no_path=0, logP=0.0):
    return Counts(np.zeros((S, S), dtype=np.int64), np.zeros((S, 16), dtype=np.int64), 0, n_no_path, logP)


def region(S, sx, sy, start_state, ops, logP=0.0):
    """updateExpectations with p = 1 for the transition the path took into every cell (impl/pairwiseAligner.c:418-432): the
    transition always, the emission only where both of the CELL's symbols are bases."""
    cx, cy = vm.symbols(sx), vm.symbols(sy)  # 1-based; index 0 is N
    c = empty(S, 0, logP)
    x, y, s, n = 0, 0, int(start_state), 0
    for to, length in np.asarray(ops, dtype=np.int64).reshape(-1, 2):
        to = int(to)
        for _ in range(int(length)):
            x, y = x + (to in MOVES_X), y + (to in MOVES_Y)
            c.transitions[s, to] += 1
            if cx[x] < 4 and cy[y] < 4:
                c.emissions[to, cx[x] * 4 + cy[y]] += 1
            s = to
            n += 1
    assert (x, y) == (len(sx), len(sy))
    return c._replace(nSteps=n)


def steps_without_emission(sx, sy, ops):
    """How many steps of the path end on a cell that sees an N, or lies on row or column 0."""
    cx, cy = vm.symbols(sx), vm.symbols(sy)
    x, y, n = 0, 0, 0
    for to, length in np.asarray(ops, dtype=np.int64).reshape(-1, 2):
        for _ in range(int(length)):
            x, y = x + (int(to) in MOVES_X), y + (int(to) in MOVES_Y)
            n += not (cx[x] < 4 and cy[y] < 4)
    return n


def regions(S, model, inputs):
    out = []
    for r, (sx, sy, _, _) in zip(model.regions, inputs):
        if r.endState < 0:
            out.append(empty(S, 1))
        else:
            out.append(region(S, sx, sy, r.startState, model.ops[r.opOff:r.opOff + r.nOps], r.logP))
    return out


def total(S, parts):
    t, logP = empty(S), 0.0
    for c in parts:
        t.transitions[:] += c.transitions
        t.emissions[:] += c.emissions
        if c.nNoPath == 0:
            logP = logP + c.logP
    return Counts(t.transitions, t.emissions, sum(c.nSteps for c in parts), sum(c.nNoPath for c in parts), logP)


def assert_equal(got, want, what):
    """Integer for integer; logP bit for bit."""
    assert got.transitions.dtype == np.int64 and got.emissions.dtype == np.int64, what
    assert got.transitions.shape == want.transitions.shape and np.array_equal(got.transitions, want.transitions), (what, got.transitions, want.transitions)
    assert got.emissions.shape == want.emissions.shape and np.array_equal(got.emissions, want.emissions), (what, got.emissions, want.emissions)
    assert (got.nSteps, got.nNoPath) == (want.nSteps, want.nNoPath), (what, got.nSteps, got.nNoPath, want.nSteps, want.nNoPath)
    assert np.float64(got.logP).tobytes() == np.float64(want.logP).tobytes(), (what, got.logP, want.logP)
