"""The preconditions that make tests/test_gpu_indel.py meaningful, asserted with the oracle alone (no device): the
asymmetric models really differ between X and Y, the oracle has next to nothing on the threshold, the lists at
threshold 0 hold every cell of their domain, the overflow cases overflow the lists they are meant to, and the widths
around the 64 KB edge are the ones cpk_plan.inl's arithmetic gives."""
import math

import numpy as np
import pytest

import indel_cases as ic
import oracle_binding as ob
from test_gpu_forward import DEGENERATE, RAGGED


@pytest.mark.parametrize("model", ic.ASYMMETRIC)
def test_asymmetric_models_differ_between_x_and_y(model):
    """A list pass that reads state 2 for state 1, or the Y-side weight for gapX, is invisible while the swapped numbers
    are equal: here every X / Y pair of numbers differs (a pair of absent transitions, -inf both, aside)."""
    sm, om = ic.model_pair(model)
    kinds = ["matchFromShortGap", "gapShortOpen", "gapShortExtend", "gapShortSwitchTo"]
    if ic.states(model) == 5:
        kinds += ["matchFromLongGap", "gapLongOpen", "gapLongExtend", "gapLongSwitchTo"]
    compared = 0
    for kind in kinds:
        vx, vy = getattr(sm, kind + "X"), getattr(sm, kind + "Y")
        if math.isinf(vx) and math.isinf(vy):
            continue
        assert vx != vy, (kind, vx)
        compared += 1
    assert compared >= 3
    for i in range(4):
        assert sm.emissionGapX[i] != sm.emissionGapY[i]
        assert om.gapXEm[i] != om.gapYEm[i]
    # the oracle's copy: every transition against its mirror image (short X <-> short Y, long X <-> long Y)
    mirror = {0: 0, 1: 2, 2: 1, 3: 4, 4: 3}
    tP = {(om.tr[k].frm, om.tr[k].to): om.tr[k].tP for k in range(om.nTransitions)}
    mirrored = 0
    for (f, t), v in tP.items():
        other = (mirror[f], mirror[t])
        if other == (f, t) or (math.isinf(v) and math.isinf(tP[other])):
            continue
        assert v != tP[other], ((f, t), v)
        mirrored += 1
    assert mirrored >= 6


def test_the_symmetric_defaults_are_what_the_asymmetric_types_default_to():
    """Why the default models of types 1 and 3 are of no use here: their numbers are the symmetric ones."""
    for asym, sym in ((ob.FIVE_STATE_ASYM, ob.FIVE_STATE), (ob.THREE_STATE_ASYM, ob.THREE_STATE)):
        a, s = ob.model(asym), ob.model(sym)
        assert list(a.gapXEm) == list(a.gapYEm) == list(s.gapXEm)
        assert [a.tr[k].tP for k in range(a.nTransitions)] == [s.tr[k].tP for k in range(s.nTransitions)]


def _check_precondition(case):
    threshold = case.pkw.get("threshold", 0.01)
    assert 0.0 <= threshold <= 0.5  # near PROB_1 the slack excuses everything
    for i, lists in enumerate(ic.oracle_lists(case)):
        for t in lists:
            assert len(np.unique((t[:, 1] + 1) * (1 << 32) + t[:, 2] + 1)) == len(t)  # no coordinate twice
        assert ic.precondition_holds(lists, threshold), (case.name, i, [(ic.near_threshold(t, threshold), len(t)) for t in lists])


@pytest.mark.parametrize("model", ic.MODELS)
def test_little_on_the_threshold_models(model):
    """Per problem and list, at most 0.25 % of the oracle's entries lie within assert_pairs_match's slack of the threshold:
    half of what the GPU test lets be present on one side only."""
    for threshold in ic.THRESHOLDS:
        for case in ic.models_cases(model, threshold):
            _check_precondition(case)


def test_little_on_the_threshold_everywhere_else():
    done = 0
    for case in ic.all_cases():
        if not case.name.startswith("models-"):
            _check_precondition(case)
            done += 1
    assert done >= 50


def _widest(case, i):
    sx, sy, a, _, _ = case.problems[i]
    band = ob.band(a, len(sx), len(sy), case.pkw.get("diagonalExpansion", 20))
    return max((r - l) // 2 + 1 for _, l, r in band)


def _wide_class(width):
    """cpecan_host.c, classify_regions, for the list emitters: classes of up to 128, 192, 256, 384 and 512 cells."""
    for k, edge in enumerate((128, 192, 256, 384, 512)):
        if width <= edge:
            return k
    return 5


@pytest.mark.parametrize("threshold", ic.THRESHOLDS)
def test_models_batches_span_ragged_ends_alphabet_and_classes(threshold):
    first, second = ic.models_cases("fiveStateAsymmetric", threshold)
    for case in (first, second):
        assert {p[3:] for p in case.problems} == set(RAGGED)
        text = [p[0] for p in case.problems if isinstance(p[0], str)]
        assert any("N" in s for s in text) and any(s != s.upper() for s in text)
        assert any(p[2] for p in case.problems)
        if threshold == 0:
            assert max(max(len(p[0]), len(p[1])) for p in case.problems) <= 135
    widths = [_widest(first, i) for i in range(len(first.problems))]
    for n in ic.UNANCHORED:
        assert n + 1 in widths
    # 200 and 300 bases bring the classes of up to 256 and 384 cells; at threshold 0, where a problem has to stay at about
    # 130 bases, 130 cells are the widest diagonal there is: two classes
    assert len({_wide_class(w) for w in widths}) == (2 if threshold == 0 else 4)


@pytest.mark.parametrize("model", ic.EDGE_MODELS)
def test_threshold_zero_lists_hold_every_cell(model):
    """lX lY matches (x > 0 and y > 0), lX (lY + 1) gapX entries (x > 0), (lX + 1) lY gapY entries (y > 0); the row y == 0 of
    gapX and the column x == 0 of gapY are reported as -1: lX and lY entries."""
    case = ic.edges_case(model)
    assert [(len(p[0]), len(p[1])) for p in case.problems[::4]] == list(ic.EDGE_SIZES)
    assert [p[3:] for p in case.problems[:4]] == RAGGED
    for (sx, sy, _, _, _), (m, gx, gy) in zip(case.problems, ic.oracle_lists(case)):
        lX, lY = len(sx), len(sy)
        assert (len(m), len(gx), len(gy)) == (lX * lY, lX * (lY + 1), (lX + 1) * lY)
        assert m[:, 1:].min() >= 0
        assert int((gx[:, 2] == -1).sum()) == lX and gx[:, 1].min() >= 0
        assert int((gy[:, 1] == -1).sum()) == lY and gy[:, 2].min() >= 0


@pytest.mark.parametrize("threshold", [0.0, 0.01])
@pytest.mark.parametrize("model", ic.EDGE_MODELS)
def test_degenerate_problems_have_one_sided_lists(model, threshold):
    case = ic.degenerate_case(model, threshold)
    seen = set()
    for (sx, sy, _, _, _), (m, gx, gy) in zip(case.problems, ic.oracle_lists(case)):
        if (sx, sy) not in DEGENERATE[:3]:
            continue
        seen.add((sx, sy))
        assert len(m) == 0
        if not sx and not sy:
            assert len(gx) == 0 and len(gy) == 0
        elif not sy:
            assert len(gy) == 0 and (gx[:, 2] == -1).all()
        else:
            assert len(gx) == 0 and (gy[:, 1] == -1).all()
        if threshold == 0:  # (at 0.01 the five-state default model gives the overhang to its long-gap states: no entry)
            assert len(gx) == len(sx) and len(gy) == len(sy)
    assert len(seen) == 3


def test_overflow_cases_overflow_the_lists_they_are_meant_to():
    a = ic.overflow_gap_only_case()
    assert ic.default_slice(a, 0) == 6 * (40 + 300) + 64 == 2104
    m, gx, gy = ic.oracle_lists(a)[0]
    assert len(gy) > 2104 and len(m) <= 2104 and len(gx) <= 2104, (len(m), len(gx), len(gy))
    b = ic.overflow_all_case()
    assert (len(b.problems[0][0]), len(b.problems[0][1])) == (64, 64) and ic.default_slice(b, 0) == 832
    assert min(len(t) for t in ic.oracle_lists(b)[0]) > 832
    c = ic.overflow_packed_case()
    overflowing = {a.name: 1, b.name: 1, c.name: 6}
    for i in range(6):
        assert min(len(t) for t in ic.oracle_lists(c)[i]) > ic.default_slice(c, i)
        assert _widest(c, i) <= 32  # narrow enough for the packed kernel
    for case in (a, b, c):  # ... and the problems behind them fit
        n = overflowing[case.name]
        assert len(case.problems) >= n + 4
        for i in range(n, len(case.problems)):
            assert max(len(t) for t in ic.oracle_lists(case)[i]) <= ic.default_slice(case, i)


def test_widths_around_the_64_kb_edge():
    """One wave's LDS by set_row_form: the indel emitter's candidate stage costs 6 KB, so the first width that goes to
    global memory is 646 cells of five states (a forward class: 715) and 1008 of three (1116)."""
    for S, about in ((5, 650), (3, 1010)):
        first = ic.first_global_length(S)
        assert abs(first + 1 - about) <= 8
        assert ic.indel_wave_lds_bytes(S, first, first) + 16 > 65536 >= ic.indel_wave_lds_bytes(S, first - 1, first - 1) + 16
    assert (ic.first_global_length(5), ic.first_global_length(3)) == (645, 1007)
    for model in ic.ASYMMETRIC:
        (n0, g0, c0), (n1, g1, c1) = ic.global_cases(model, 0.01)
        assert (n1, g0, g1) == (n0 + 1, False, True)
        for n, c in ((n0, c0), (n1, c1)):
            assert (len(c.problems[0][0]), len(c.problems[0][1])) == (n, n) and _widest(c, 0) == n + 1


def test_packed_batches_are_as_wide_as_their_groups():
    for model in ic.ASYMMETRIC:
        for lanes, case in ic.packed_cases(model, 0.01):
            widest = max(_widest(case, i) for i in range(len(case.problems)) if case.problems[i][2])
            assert lanes // 2 < widest <= lanes or widest <= lanes == 8, (case.name, widest)


def test_consumer_lists_are_dense():
    """getCumulativeGapProbs sums gap lists that are about as long as the match list, not a few dozen entries."""
    for model in ic.CONSUMER_MODELS:
        case = ic.consumers_case(model, 1e-4)
        m, gx, gy = (sum(len(l[w]) for l in ic.oracle_lists(case)) for w in range(3))
        bases = sum(len(p[0]) + len(p[1]) for p in case.problems)
        assert gx > bases and gy > bases and gx > m // 2 and gy > m // 2, (m, gx, gy, bases)
