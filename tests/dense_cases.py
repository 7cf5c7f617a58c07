"""The inputs of the dense-rows tests (tests/test_dense_cpu.py, test_gpu_dense.py, dense_exact_check.py,
test_foreign_emitter_c.py): cases (a)-(f) as one region each, (h) for the splitting entry point.  Nothing here touches a GPU.

    Case.model   "fiveState" | "threeState" | "threeStateAsymInf": model_pair(name) gives (library model, oracle model)
    Case.pkw     keyword overrides of the banding parameters, for both sides
"""
import collections
import functools
import random

import numpy as np

import oracle_binding as ob
from cpecan_amd import api
from cpecan_amd.workload import make_pair

Case = collections.namedtuple("Case", "name model sx sy anchors pkw ragged_left ragged_right")

INF_TRANSITION = (1, 2)  # gapX -> gapY of the three-state model: probability 0, i.e. a -inf switch transition


@functools.lru_cache(maxsize=None)
def inf_hmm():
    """(library Hmm, oracle Hmm): a randomised, normalised three-state asymmetric HMM (as test_gpu_forward._model_pair) with one
    impossible transition."""
    rng = random.Random(977)
    ph, oh = api.hmm_constructEmpty(0.0, api.threeStateAsymmetric), ob.hmm(ob.THREE_STATE_ASYM, 0.0)
    for i in range(9):
        ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
    i = INF_TRANSITION[0] * 3 + INF_TRANSITION[1]
    ph.transitions[i] = oh.T[i] = 0.0
    for i in range(3 * 16):
        ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
    api.hmm_normalise(ph)
    ob.lib().orc_hmm_normalise(oh)
    return ph, oh


@functools.lru_cache(maxsize=None)
def model_pair(name):
    if name == "fiveState":
        return api.stateMachine5_construct(api.fiveState), ob.model(ob.FIVE_STATE)
    if name == "threeState":
        return api.stateMachine3_construct(api.threeState), ob.model(ob.THREE_STATE)
    assert name == "threeStateAsymInf"
    ph, oh = inf_hmm()
    return api.hmm_getStateMachine(ph), ob.model_from_hmm(oh)


def states(name):
    return 5 if name == "fiveState" else 3


def _rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


def _case_b():
    rng = random.Random(7075)
    return Case("b_70x75", "fiveState", _rand_seq(rng, 70), _rand_seq(rng, 75), (), {}, False, False)


def _case_c():
    sx, sy, a = make_pair(3, 1, 600, 10)
    return Case("c_segments", "fiveState", sx, sy, a, dict(diagonalExpansion=10, minDiagsBetweenTraceBack=50, traceBackDiagonals=7),
                False, False)


def _case_d():
    sx, sy, a = make_pair(11, 0, 150, 12, anchor_every=25)
    sx, sy = bytearray(sx), bytearray(sy)
    sx[40:47] = b"N" * 7          # runs of N
    sy[90:93] = b"NNN"
    sx[100:120] = bytes(sx[100:120]).lower()  # lower case
    sy[10:30] = bytes(sy[10:30]).lower()
    return Case("d_inf_ragged", "threeStateAsymInf", bytes(sx), bytes(sy), a,
                dict(diagonalExpansion=12, minDiagsBetweenTraceBack=60, traceBackDiagonals=9), True, True)


def _case_e():
    sx, sy, a = make_pair(4, 0, 300, 20, anchor_every=30)
    a = np.array(a, dtype=np.int64)
    a[:, 2] = [(8, 30, 16, 0, 24)[i % 5] for i in range(len(a))]  # mixed per-anchor expansions, all even
    return Case("e_dynamic", "fiveState", sx, sy, a,
                dict(diagonalExpansion=20, minDiagsBetweenTraceBack=100, traceBackDiagonals=20, dynamicAnchorExpansion=1), False, False)


@functools.lru_cache(maxsize=None)
def cases():
    """(a)-(f), in the order case (g) adds them to one object."""
    return (
        Case("a_tiny5", "fiveState", b"AGCG", b"AGTTCG", (), {}, False, False),
        Case("a_tiny3", "threeState", b"AGCG", b"AGTTCG", (), {}, False, False),
        _case_b(), _case_c(), _case_d(), _case_e(),
        Case("f_x0", "fiveState", b"", b"ACGTA", (), {}, False, False),
        Case("f_y0", "fiveState", b"ACGTA", b"", (), {}, False, False),
        Case("f_both0", "fiveState", b"", b"", (), {}, False, False),
    )


CASE_NAMES = tuple(c.name for c in cases())


def case(name):
    return cases()[CASE_NAMES.index(name)]


# Case (g): the inputs of (a)-(f) together in ONE object and one run.  An object holds one model and one set of parameters, so
# the nine inputs are run under the model and parameters of each of these cases in turn -- many tracebacks, the -inf model
# with ragged ends, per-anchor expansions -- and compared with the same input run alone under the same configuration.
JOINT_CONFIGS = ("c_segments", "d_inf_ragged", "e_dynamic")


def anchors_of(c):
    return [tuple(int(v) for v in t) for t in np.asarray(c.anchors, dtype=np.int64).reshape(-1, 3)] if len(c.anchors) else []


def lib_params(c):
    return api.pairwiseAlignmentBandingParameters_construct(**c.pkw)


def oracle_params(c):
    return ob.params(**c.pkw)


def widths(c):
    p = oracle_params(c)
    if len(c.sx) + len(c.sy) == 0:
        return [1]
    return [(r - l) // 2 + 1 for _, l, r in ob.band(anchors_of(c), len(c.sx), len(c.sy), p.diagonalExpansion, bool(p.dynamicAnchorExpansion))]


_traces = {}


def oracle_trace(c):
    """(pairs, trace) of ob.aligned_pairs_traced; computed once per case, never modified."""
    if c.name not in _traces:
        _traces[c.name] = ob.aligned_pairs_traced(model_pair(c.model)[1], c.sx, c.sy, anchors_of(c), oracle_params(c),
                                                  c.ragged_left, c.ragged_right)
    return _traces[c.name]


# ---- (h): the splitting entry point -- anchors with two gaps wider than a small splitMatrixBiggerThanThis ----
def split_case():
    sx, sy, a = make_pair(13, 0, 420, 10, anchor_every=12)
    a = np.array([t for t in np.asarray(a) if not (100 <= t[0] < 190 or 260 <= t[0] < 340)], dtype=np.int64)
    return Case("h_split", "fiveState", sx, sy, a,
                dict(diagonalExpansion=10, minDiagsBetweenTraceBack=60, traceBackDiagonals=9, splitMatrixBiggerThanThis=50 * 50), False, True)


# ---- the comparison of test_gpu_dense.py and dense_exact_check.py ----
def _close(got, want, tol, what):
    """Infinities in the same places; finite values within tol * max(1, |want|) (test_cell_values_and_totals_match_oracle's
    scale); tol 0: equality.  Returns the largest finite difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (what, "infinities differ")
    diff = np.abs(got[~inf] - want[~inf])
    worst = float(diff.max()) if diff.size else 0.0
    assert np.all(diff <= tol * np.maximum(1.0, np.abs(want[~inf]))), (what, worst)
    return worst


def compare_with_oracle(c, rows, tol):
    """rows: cpecan_amd.dense.Rows of case c against the oracle's trace.  Returns a line of figures."""
    _, tr = oracle_trace(c)
    if len(c.sx) + len(c.sy) == 0:  # no rows
        assert tr == {} and all(len(a) == 0 for a in (rows.diags, rows.F, rows.B, rows.b_next, rows.total_used, rows.segs))
        return "%s: no rows" % c.name
    p = oracle_params(c)
    band = ob.band(anchors_of(c), len(c.sx), len(c.sy), p.diagonalExpansion, bool(p.dynamicAnchorExpansion))
    assert np.array_equal(rows.diags, np.array([(l, (r - l) // 2 + 1) for _, l, r in band], dtype=np.int32)), c.name
    assert np.array_equal(rows.cell_off, tr["cell_offset"]), c.name
    S = states(c.model)
    assert rows.F.shape == rows.B.shape == (tr["n_cells"], S) and len(rows.segs) == tr["n_tracebacks"], c.name
    worst_f = _close(rows.F, tr["forward"], tol, c.name + " F")
    m = ~np.isnan(tr["fb_match"])
    assert m.any() == (len(c.sx) > 0 and len(c.sy) > 0)  # the oracle records it for cells with x > 0 and y > 0
    worst_fb = _close((rows.F[:, 0] + rows.B[:, 0])[m], tr["fb_match"][m], tol, c.name + " F.match + B.match")
    assert np.isnan(rows.total_used[0]) and np.isnan(tr["total_used"][0]) and np.isnan(rows.B[0]).all(), c.name
    worst_t = _close(rows.total_used[1:], tr["total_used"][1:], tol, c.name + " total_used")
    assert not np.isnan(rows.B[1:]).any() and not np.isnan(rows.b_next).any(), c.name
    assert len(rows.b_next) == int(rows.b_next_off[-1]) == sum(int(rows.diags[f + 1][1]) for _, t, f in rows.segs if f < t), c.name
    return "%s: %d cells, %d tracebacks, largest |dF| %.3g, |d(F+B).match| %.3g, |dtotal| %.3g" % (
        c.name, tr["n_cells"], tr["n_tracebacks"], worst_f, worst_fb, worst_t)
