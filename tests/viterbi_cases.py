"""The inputs of the Viterbi tests (tests/test_viterbi_cpu.py, test_gpu_viterbi.py, viterbi_exact_check.py): cases (a)-(f) and
(h) of tests/dense_cases.py, and the smallest inputs at which cpk_viterbi.inl can go wrong -- diagonals wider than one and two
passes of the wave and wider than the LDS rows, empty sequences, regions whose diagonal count sits at a multiple of the
traceback's block, several regions, exact ties, -inf transitions, a problem without a path.  check_preconditions() asserts of
every case the edge it is there for.  The model's results are computed once per case and never modified.  Nothing here touches
a GPU.
"""
import functools
import random

import numpy as np

import dense_cases as dc
import oracle_binding as ob
import viterbi_model as vm
from cpecan_amd import api, viterbi
from cpecan_amd.workload import make_pair

Case = dc.Case
B = viterbi.TRACEBACK_BLOCK_DIAGONALS


def _rand_hmm(lib_type, orc_type, S, seed, zero):
    """(library model, oracle model) of a randomised, normalised HMM whose transitions `zero` [(from, to)] have probability 0."""
    rng = random.Random(seed)
    ph, oh = api.hmm_constructEmpty(0.0, lib_type), ob.hmm(orc_type, 0.0)
    for i in range(S * S):
        ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
    for frm, to in zero:
        ph.transitions[frm * S + to] = oh.T[frm * S + to] = 0.0
    for i in range(S * 16):
        ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
    api.hmm_normalise(ph)
    ob.lib().orc_hmm_normalise(oh)
    return api.hmm_getStateMachine(ph), ob.model_from_hmm(oh)


@functools.lru_cache(maxsize=None)
def model_pair(name):
    """(library model, oracle model)."""
    if name == "fiveStateAsym":
        return api.stateMachine5_construct(api.fiveStateAsymmetric), ob.model(ob.FIVE_STATE_ASYM)
    if name == "threeStateAsym":
        return api.stateMachine3_construct(api.threeStateAsymmetric), ob.model(ob.THREE_STATE_ASYM)
    if name == "fiveStateNoLongOpen":  # the two HMM transitions the model's long-gap opens are loaded from have probability 0
        return _rand_hmm(api.fiveStateAsymmetric, ob.FIVE_STATE_ASYM, 5, 4111, [(0, 3), (0, 2)])  # (check_preconditions holds it to that)
    if name == "threeStateNoEndY":  # gapY -> match has probability 0: the end prior of gapY is -inf
        return _rand_hmm(api.threeStateAsymmetric, ob.THREE_STATE_ASYM, 3, 4112, [(2, 0)])
    return dc.model_pair(name)


MODEL_TYPES = ("fiveState", "fiveStateAsym", "threeState", "threeStateAsym")


def _rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


def _unanchored(name, model, lx, ly, seed):
    rng = random.Random(seed)
    sx = _rand_seq(rng, lx)
    sy = bytearray(_rand_seq(rng, ly))
    n = min(lx, ly)
    for i in range(n):  # mostly X again, so that the best path is no coin toss
        if rng.random() < 0.8:
            sy[i] = sx[i]
    return Case(name, model, sx, bytes(sy), (), {}, False, False)


def _narrow(name, n_diagonals):
    """A band of expansion 8 along the main diagonal whose region has lX + lY == n_diagonals; an insertion and a deletion inside."""
    rng = random.Random(n_diagonals)
    lx = n_diagonals // 2
    sx = _rand_seq(rng, lx)
    sy = sx[:30] + sx[31:60] + b"T" + sx[60:] + b"A" * (n_diagonals - 2 * lx)  # one base of X left out, one put in
    anchors = [(i, i, 8) for i in range(5, lx - 2, 6)]  # they make the band; the path leaves their diagonal by one
    return Case(name, "fiveState", sx, sy, tuple(anchors), dict(diagonalExpansion=8), False, False)


def _three_regions(name, ragged_left):
    sx, sy, a = make_pair(13, 0, 420, 10, anchor_every=12)
    a = np.array([t for t in np.asarray(a) if not (t[0] < 90 or 170 <= t[0] < 250)], dtype=np.int64)
    return Case(name, "fiveState", sx, sy, a, dict(diagonalExpansion=10, splitMatrixBiggerThanThis=50 * 50), ragged_left, False)


@functools.lru_cache(maxsize=None)
def cases():
    return dc.cases() + (
        dc.split_case(),
        _unanchored("u_70x90", "fiveState", 70, 90, 1),
        _unanchored("u_140x150", "threeState", 140, 150, 2),
        _unanchored("u_300x300", "fiveState", 300, 300, 3),
        Case("z_x0_ragged", "threeState", b"", b"ACGTA", (), {}, True, True),
        Case("z_y0_ragged", "fiveStateAsym", b"ACGTA", b"", (), {}, True, False),
        Case("z_both0_ragged", "threeStateAsym", b"", b"", (), {}, False, True),
        _narrow("n_3B_minus1", 3 * B - 1), _narrow("n_3B", 3 * B), _narrow("n_3B_plus1", 3 * B + 1),
        _three_regions("r_three", False), _three_regions("r_three_ragged_left", True),
        Case("t_homopolymer5", "fiveState", b"A" * 9, b"A" * 7, (), {}, False, False),
        Case("t_repeat3", "threeState", b"ACACACACAC", b"ACACACAC", (), {}, False, False),
        _unanchored("i_no_long_open", "fiveStateNoLongOpen", 40, 45, 4),
        Case("p_no_path", "threeStateNoEndY", b"", b"ACG", (), {}, False, False),
    )


CASE_NAMES = tuple(c.name for c in cases())
# the cases every kernel form can run (no diagonal wider than the LDS rows) and that are small: test 3 of test_gpu_viterbi.py
SMALL_CASE_NAMES = tuple(n for n in CASE_NAMES if n not in ("u_300x300", "c_segments", "e_dynamic", "h_split"))


def case(name):
    return cases()[CASE_NAMES.index(name)]


anchors_of = dc.anchors_of
lib_params = dc.lib_params
oracle_params = dc.oracle_params
_models = {}


def model_of(c):
    """viterbi_model.viterbi of the case; computed once, never modified."""
    if c.name not in _models:
        _models[c.name] = vm.viterbi(model_pair(c.model)[1], c.sx, c.sy, anchors_of(c), oracle_params(c), c.ragged_left, c.ragged_right)
    return _models[c.name]


def widest(c):
    """The widest diagonal of any region of the case."""
    p, w = oracle_params(c), 1
    for x1, y1, x2, y2, own, _, _ in vm.regions_of(anchors_of(c), len(c.sx), len(c.sy), p, c.ragged_left, c.ragged_right):
        w = max([w] + [(r - l) // 2 + 1 for _, l, r in vm.band_of(own, x2 - x1, y2 - y1, p)])
    return w


def check_preconditions():
    """Each case is the edge it is there for."""
    assert 65 <= widest(case("u_70x90")) <= 128
    assert 128 < widest(case("u_140x150")) <= viterbi.LDS_MAX_WIDTH
    assert widest(case("u_300x300")) > viterbi.LDS_MAX_WIDTH
    assert all(widest(case(n)) <= viterbi.LDS_MAX_WIDTH for n in SMALL_CASE_NAMES)
    for n, lx, ly in (("f_x0", 0, 5), ("f_y0", 5, 0), ("f_both0", 0, 0), ("z_x0_ragged", 0, 5), ("z_y0_ragged", 5, 0), ("z_both0_ragged", 0, 0)):
        assert (len(case(n).sx), len(case(n).sy)) == (lx, ly)
    for n, want in (("n_3B_minus1", 3 * B - 1), ("n_3B", 3 * B), ("n_3B_plus1", 3 * B + 1)):
        c = case(n)
        assert len(c.sx) + len(c.sy) == want and len(model_of(c).regions) == 1 and widest(c) <= 16, n
        assert {1, 2} & set(int(s) for s in model_of(c).ops[:, 0]), "the path holds a gap"
    r = model_of(case("r_three")).regions
    assert len(r) >= 3 and r[0].x1 == 0 and r[0].y1 == 0
    rl = model_of(case("r_three_ragged_left")).regions
    assert len(rl) == len(r) - 1 and rl[0][:4] == (r[1].x1, r[1].y1, r[1].x2, r[1].y2) and rl[0].x1 > 0 and rl[0].y1 > 0, "the first block is skipped"
    assert len(model_of(dc.split_case()).regions) >= 3
    assert model_of(case("t_homopolymer5")).ties >= 1 and model_of(case("t_repeat3")).ties >= 1
    om = model_pair("fiveStateNoLongOpen")[1]
    opens = [t.tP for t in om.tr[:om.nTransitions] if t.frm == 0 and t.to in (3, 4)]
    assert len(opens) == 2 and all(t == float("-inf") for t in opens)
    assert np.isfinite(model_of(case("i_no_long_open")).logP)
    om = model_pair("threeStateNoEndY")[1]
    assert om.end[2] == float("-inf")
    m = model_of(case("p_no_path"))
    assert m.logP == float("-inf") and m.regions[0].startState == m.regions[0].endState == -1 and m.regions[0].nOps == 0
    assert model_of(case("d_inf_ragged")).logP > float("-inf") and model_of(case("e_dynamic")).logP > float("-inf")


def region_inputs(c):
    """[(sx, sy, ragged_left, ragged_right)] of the case's regions: what replay takes."""
    p = oracle_params(c)
    return [(bytes(c.sx)[x1:x2], bytes(c.sy)[y1:y2], rl, rr)
            for x1, y1, x2, y2, _, rl, rr in vm.regions_of(anchors_of(c), len(c.sx), len(c.sy), p, c.ragged_left, c.ragged_right)]


def assert_equals_model(c, got):
    """got: cpecan_amd.viterbi.Result of case c.  Regions, states and ops integer for integer, every logP bit for bit."""
    want = model_of(c)
    bits = lambda v: np.float64(v).tobytes()  # noqa: E731
    assert len(got.regions) == len(want.regions), c.name
    for k, (g, w) in enumerate(zip(got.regions, want.regions)):
        assert tuple(g[:4]) == tuple(w[:4]) and tuple(g[5:]) == tuple(w[5:]), (c.name, k, g, w)
        assert bits(g.logP) == bits(w.logP), (c.name, k, g.logP, w.logP)
    assert got.ops.dtype == np.int32 and np.array_equal(got.ops, want.ops), c.name
    assert bits(got.logP) == bits(want.logP), (c.name, got.logP, want.logP)
