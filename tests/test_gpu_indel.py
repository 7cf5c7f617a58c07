"""The indel emitter (CPECAN_EMIT_INDEL: the match, gapX and gapY lists of diagonalCalculationPosteriorProbs,
pairwiseAligner.c:691-733; Batch(..., emit=EMIT_INDEL), result(i, which)) against the CPU oracle on every kernel that
writes the three lists -- the sweep kernel's candidate rings in LDS and with its rows in global memory, the packed
kernel's pass over parked B values in its three group widths, the team kernel of four and of eight waves -- and on the
host rules that treat the three lists together (slices per list, one overflow scan, result(i, which) through the device
order).

Every comparison is per problem and per list: the GPU's list against ob.aligned_pairs_with_indels of the same input
through parity.assert_pairs_match (scores, set and order), and the pairs that gate excuses near the threshold are capped:
at most 0.5 % of the oracle's list, none at threshold 0.  tests/test_indel_cases_cpu.py holds the preconditions (the
oracle itself has at most half of that near the threshold; the asymmetric models differ between X and Y; ...); the
inputs are tests/indel_cases.py's."""
import re
import sys

import numpy as np
import pytest

import indel_cases as ic
import oracle_binding as ob
from cpecan_amd import api
from parity import assert_pairs_match
from test_gpu_forward import DEGENERATE, GLOBAL_MARK

pytestmark = pytest.mark.gpu

ONE_WAVE, TEAM = "one wave per region", "a team of waves per region"


def _run(case, post=None):
    """One EMIT_INDEL batch, the problems through add_many: ([problem][list] triples, stats, scores or None)."""
    sm = ic.model_pair(case.model)[0]
    p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
    with api.Batch(sm, p, emit=api.EMIT_INDEL) as b:
        if post:
            b.set_post(*post)
        b.add_many(case.problems)
        b.upload()
        b.run()
        b.download()
        n = len(case.problems)
        lists = [[b.result(i, which) for which in range(4 if post else 3)] for i in range(n)]
        return lists, b.stats(), ([b.scores(i) for i in range(n)] if post else None)


def _keys(t):
    return (t[:, 1].astype(np.int64) + 1) * (1 << 32) + t[:, 2].astype(np.int64) + 1


def _compare(case, got, which_problems=None):
    """Every problem and list against the oracle; prints and returns (largest score difference, one-sided pairs)."""
    threshold = case.pkw.get("threshold", 0.01)
    want = ic.oracle_lists(case)
    assert len(got) == len(want)
    worst = one_sided = entries = 0
    for i in (which_problems if which_problems is not None else range(len(want))):
        for which in range(3):
            g, w = np.asarray(got[i][which]).reshape(-1, 3), want[i][which]
            what = "%s, problem %d, list %d" % (case.name, i, which)
            if threshold == 0:
                assert len(g) == len(w), what
            _, gi, wi = np.intersect1d(_keys(g), _keys(w), return_indices=True)
            only = len(g) + len(w) - 2 * len(gi)
            if len(gi):
                worst = max(worst, int(np.abs(g[gi, 0].astype(np.int64) - w[wi, 0]).max()))
            one_sided += only
            entries += len(w)
            assert only <= ic.one_sided_allowed(threshold, len(w)), "%s: %d pairs on one side only, oracle has %d" % (what, only, len(w))
            try:
                assert_pairs_match(g, w, threshold=threshold)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (what, e)) from None
    print("%s: %d oracle entries, largest score difference %d (of 1e7), %d pairs on one side only" % (case.name, entries, worst, one_sided))
    return worst, one_sided


def _assert_bit_equal(a, b, what):
    assert len(a) == len(b)
    for i, (la, lb) in enumerate(zip(a, b)):
        for which in range(3):
            assert la[which].shape == lb[which].shape and (la[which] == lb[which]).all(), "%s: problem %d, list %d" % (what, i, which)


def _wide_lines(err):
    return re.findall(r"^cpecan class \d+:.*$", err, re.M)


def _packed_lines(err):
    return re.findall(r"^cpecan packed class \d+:.*$", err, re.M)


def _traced_run(case, capfd, post=None):
    printed = capfd.readouterr().out  # (what the test has printed so far: put back below)
    got, st, scores = _run(case, post)
    err = capfd.readouterr().err
    sys.stdout.write(printed)
    for line in _wide_lines(err) + _packed_lines(err):
        print(line)
    return got, st, scores, err


@pytest.fixture
def trace(monkeypatch):
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    for knob in ("CPECAN_TEAM", "CPECAN_PACKED"):
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


# ---- 1. models, thresholds and ragged ends with one wave per region ----
@pytest.mark.parametrize("threshold", ic.THRESHOLDS)
@pytest.mark.parametrize("model", ic.MODELS)
def test_models_thresholds_and_ragged_ends(model, threshold, trace, capfd):
    """All five models at thresholds {0, 1e-4, 0.01, 0.2} on the mixed batches of indel_cases.models_cases.  At 0 and 1e-4
    every cell, or most, is in all three lists: the x > 0 / y > 0 predicates decide membership and the candidate rings
    wrap many times per segment.  Every class one wave per region, rows in LDS; four wide classes in the first batch --
    two at threshold 0, where a problem stays at about 130 bases and so within 192 cells (test_indel_cases_cpu.py)."""
    first, second = ic.models_cases(model, threshold)
    for case in (first, second):
        got, st, _, err = _traced_run(case, capfd)
        classes = _wide_lines(err)
        assert all(ONE_WAVE in c and GLOBAL_MARK not in c for c in classes) and not _packed_lines(err), classes
        if case is first:
            assert len(classes) >= (2 if threshold == 0 else 3), classes
        assert st.problems == len(case.problems)
        _compare(case, got)


# ---- 2. edges and the -1 coordinates ----
@pytest.mark.parametrize("model", ic.EDGE_MODELS)
def test_threshold_zero_emits_every_cell_of_each_list(model):
    """Unanchored, unbanded, threshold 0: lX lY matches, lX (lY + 1) gapX and (lX + 1) lY gapY entries -- every cell with
    x > 0 and y > 0, with x > 0, with y > 0 (:712, :719, :725) --, lX entries of gapX with y == -1 and lY of gapY with
    x == -1, and the lists equal to the oracle's entry for entry."""
    case = ic.edges_case(model)
    got, st, _ = _run(case)
    for i, ((sx, sy, _, _, _), (m, gx, gy)) in enumerate(zip(case.problems, got)):
        lX, lY = len(sx), len(sy)
        assert (len(m), len(gx), len(gy)) == (lX * lY, lX * (lY + 1), (lX + 1) * lY), i
        assert m[:, 1].min() >= 0 and m[:, 2].min() >= 0, i
        assert int((gx[:, 2] == -1).sum()) == lX and gx[:, 1].min() >= 0 and gx[:, 2].min() >= -1, i
        assert int((gy[:, 1] == -1).sum()) == lY and gy[:, 2].min() >= 0 and gy[:, 1].min() >= -1, i
    worst, one_sided = _compare(case, got)
    assert one_sided == 0
    for i, lists in enumerate(ic.oracle_lists(case)):  # entry for entry: the same coordinates at the same places
        for which in range(3):
            assert (got[i][which][:, 1:] == lists[which][:, 1:]).all(), (i, which)


@pytest.mark.parametrize("threshold", [0.0, 0.01])
@pytest.mark.parametrize("model", ic.EDGE_MODELS)
def test_degenerate_problems_inside_a_batch(model, threshold):
    case = ic.degenerate_case(model, threshold)
    got, st, _ = _run(case)
    assert st.problems == len(case.problems) == 32
    seen = 0
    for (sx, sy, _, _, _), (m, gx, gy) in zip(case.problems, got):
        if (sx, sy) == DEGENERATE[0]:
            assert len(m) == len(gx) == len(gy) == 0
        elif (sx, sy) == DEGENERATE[1]:  # ("ACGT", ""): only a gapX list, y = -1
            assert len(m) == len(gy) == 0 and (gx[:, 2] == -1).all() and (threshold > 0 or sorted(gx[:, 1].tolist()) == [0, 1, 2, 3])
        elif (sx, sy) == DEGENERATE[2]:  # ("", "ACGTN"): only a gapY list, x = -1
            assert len(m) == len(gx) == 0 and (gy[:, 1] == -1).all() and (threshold > 0 or sorted(gy[:, 2].tolist()) == [0, 1, 2, 3, 4])
        else:
            continue
        seen += 1
    assert seen == 12
    _compare(case, got)


# ---- 3. every kernel form with asymmetric models ----
@pytest.mark.parametrize("threshold", ic.FORM_THRESHOLDS)
@pytest.mark.parametrize("model", ic.ASYMMETRIC)
def test_packed_kernel_with_asymmetric_models(model, threshold, trace, capfd):
    """The packed kernel's own list pass (cpk_packed.inl, the kIndel branch) in groups of 8, 16 and 32 lanes: the oracle's
    lists, and bit for bit those of one wave per region (CPECAN_PACKED=0)."""
    for lanes, case in ic.packed_cases(model, threshold):
        trace.setenv("CPECAN_PACKED", "2")
        packed, st_p, _, err = _traced_run(case, capfd)
        assert any("in groups of %d lanes" % lanes in c for c in _packed_lines(err)), err
        trace.setenv("CPECAN_PACKED", "0")
        sweep, st_s, _, err = _traced_run(case, capfd)
        assert not _packed_lines(err) and all(ONE_WAVE in c for c in _wide_lines(err)), err
        assert st_p.cells == st_s.cells and st_p.pairs == st_s.pairs
        _assert_bit_equal(packed, sweep, case.name)
        _compare(case, packed)


@pytest.mark.parametrize("threshold", ic.FORM_THRESHOLDS)
@pytest.mark.parametrize("model", ic.ASYMMETRIC)
def test_team_kernel_with_asymmetric_models(model, threshold, trace, capfd):
    """The team kernel's list pass with four waves (501 cells; the library's own choice for five states, CPECAN_TEAM=500
    for three, where one wave per region still has four waves on a CU), with eight (901 cells of five states) and on a
    multi-segment band (CPECAN_TEAM=100): the oracle's lists, and bit for bit those of one wave per region
    (CPECAN_TEAM=0) -- which for 901 cells of five states is the sweep kernel with its rows in global memory."""
    for words, team, case in ic.team_cases(model, threshold):
        if team:
            trace.setenv("CPECAN_TEAM", team)
        else:
            trace.delenv("CPECAN_TEAM", raising=False)
        teamed, _, _, err = _traced_run(case, capfd)
        classes = _wide_lines(err)
        assert any(TEAM in c and words in c for c in classes) and (team == "100" or len(classes) == 1), classes
        trace.setenv("CPECAN_TEAM", "0")
        solo, _, _, err = _traced_run(case, capfd)
        classes = _wide_lines(err)
        assert classes and all(ONE_WAVE in c for c in classes), classes
        assert all((GLOBAL_MARK in c) == (words == "(eight)") for c in classes), classes
        _assert_bit_equal(teamed, solo, case.name)
        _compare(case, teamed)


@pytest.mark.parametrize("threshold", ic.FORM_THRESHOLDS)
@pytest.mark.parametrize("model", ic.ASYMMETRIC)
def test_one_wave_with_rows_in_global_memory(model, threshold, trace, capfd):
    """CPECAN_TEAM=0 around the 64 KB edge of one wave's LDS (cpk_plan.inl, set_row_form; the candidate stage of the indel
    emitter is 3 x 2 x kStage doubles): the last width that fits keeps its rows in LDS -- the trace line gives the
    computed size --, the first that does not says "rolling rows in global memory".  Both equal the oracle's lists and,
    bit for bit, what the library's own choice of kernel gives."""
    S = ic.states(model)
    for n, in_global, case in ic.global_cases(model, threshold):
        trace.setenv("CPECAN_TEAM", "0")
        solo, _, _, err = _traced_run(case, capfd)
        classes = _wide_lines(err)
        assert len(classes) == 1 and re.search(r": 1 regions, widest diagonal %d,.*%s" % (n + 1, ONE_WAVE), classes[0]), classes
        assert (GLOBAL_MARK in classes[0]) == in_global, classes
        if not in_global:
            assert "LDS %d B" % ic.indel_wave_lds_bytes(S, n, n) in classes[0], classes
        trace.delenv("CPECAN_TEAM")
        own, _, _, err = _traced_run(case, capfd)
        _assert_bit_equal(own, solo, case.name)
        _compare(case, solo)


# ---- 4. the overflow re-run with three lists ----
@pytest.mark.parametrize("which", ["gapY", "all", "packed"])
def test_overflow_rerun_with_three_lists(which, trace, capfd):
    """need is the maximum over the three counts and the slices of the three lists share outOff (cpecan_host.c): a gapY
    list that outgrows its slice while the match list fits, and all three at once (one wave per region; the packed
    kernel), each followed in its batch by problems that fit."""
    case = {"gapY": ic.overflow_gap_only_case, "all": ic.overflow_all_case, "packed": ic.overflow_packed_case}[which]()
    if which == "packed":
        trace.setenv("CPECAN_PACKED", "2")
    got, st, _, err = _traced_run(case, capfd)
    assert (len(_packed_lines(err)) > 0) == (which == "packed"), err
    assert st.launches >= 2
    worst, one_sided = _compare(case, got)


# ---- 5. size classes in one batch ----
def test_size_classes_in_one_batch(trace, capfd):
    """The batch of test_mixed_widths_run_in_size_classes under the random type 3: result(i, which) finds list `which` of
    problem i behind the class sort, and a slice of the batch run alone gives the same lists bit for bit."""
    case = ic.size_classes_case()
    got, st, _, err = _traced_run(case, capfd)
    classes = _wide_lines(err)
    # (three states: 501 cells leave four waves on a CU and 901 are more than a team of four takes -- one wave per region throughout)
    assert len(classes) >= 4 and all(ONE_WAVE in c for c in classes), classes
    assert st.problems == st.regions == len(case.problems)
    _compare(case, got)
    alone, _, _ = _run(ic.Case("size-classes-slice", case.model, case.problems[ic.SIZE_CLASS_SLICE], case.pkw))
    _assert_bit_equal(alone, got[ic.SIZE_CLASS_SLICE], "slice alone")


# ---- 6. the consumers on these lists ----
@pytest.mark.parametrize("threshold", ic.CONSUMER_THRESHOLDS)
@pytest.mark.parametrize("model", ic.CONSUMER_MODELS)
def test_mea_and_left_shift_on_dense_asymmetric_lists(model, threshold, trace, capfd):
    """POST_MEA | POST_LEFT_SHIFT behind the packed kernel, one wave per region and the team in one batch: list 3 and the
    alignment score equal the oracle's getMaximalExpectedAccuracyPairwiseAlignment + leftShiftAlignment of the GPU's own
    three lists -- integer arithmetic, bit-exact."""
    case = ic.consumers_case(model, threshold)
    gamma = float(np.float32(0.5))
    trace.setenv("CPECAN_PACKED", "2")
    trace.setenv("CPECAN_TEAM", "500")  # (501 cells of three states would stay with one wave per region)
    got, st, scores, err = _traced_run(case, capfd, post=(api.POST_MEA | api.POST_LEFT_SHIFT, gamma))
    classes = _wide_lines(err)
    assert _packed_lines(err) and any(ONE_WAVE in c for c in classes) and any(TEAM in c for c in classes), err
    gaps = 0
    for i, (sx, sy, _, _, _) in enumerate(case.problems):
        m, gx, gy, shifted = got[i]
        gaps += len(gx) + len(gy)
        mea, score = ob.mea_alignment(m, gx, gy, len(sx), len(sy), gamma)
        want = ob.left_shift_alignment(mea, sx, sy)
        assert shifted.shape == want.shape and (shifted.astype(np.int64) == want).all(), i
        assert scores[i][2] == score, i
    print("%s: %d gap entries summed" % (case.name, gaps))
