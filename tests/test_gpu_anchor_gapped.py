"""Gapped extension of the chained HSPs (cpecan_anchor_options.gappedExtension) on the GPU
against its definition (tests/anchor_model_gapped.py): runs and statistics integer for integer on the constructed cases,
on random and masked pairs in one batch through the recursion, on both strands, with transition seeds and their
threshold, with the smallest diagonal limit and on the human / dog ENCODE pair; getAlignedPairs with the option against
the anchored call on the model's anchors; and the option off against a call without options."""
import functools

import numpy as np
import pytest

import anchor_cases as ac
import anchor_gapped_cases as gc
import anchor_model as am
import anchor_model_gapped as ag
import reference_cases as rc
import strand_model as sm
from cpecan_amd import api

pytestmark = pytest.mark.gpu

COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")
ON = dict(gapped=1)


def _options(gapped=0, yDrop=0, gappedMaxDiagonals=0, threshold=0):
    return api.anchor_options(threshold, gappedExtension=gapped, yDrop=yDrop, gappedMaxDiagonals=gappedMaxDiagonals)


def _same(got_runs, got_stats, want_runs, want_stats, what):
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, what


@functools.lru_cache(maxsize=None)
def _batch():
    """Three random and three masked pairs of 3000: chains of different lengths in one launch."""
    return tuple(f(index, 3000) for index in (1, 2, 3) for f in (ac.random_pair, ac.masked_pair))


@functools.lru_cache(maxsize=None)
def _batch_model(**kw):
    return tuple(ag.find_anchor_runs(sx, sy, **kw) for sx, sy in _batch())


@pytest.mark.parametrize("case", sorted(gc.CASES))
def test_a_constructed_case_equals_the_model(case):
    sx, sy, kw = gc.CASES[case]
    for softMask in (True, False):
        got = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, softMask=softMask, options=_options(**kw))
        want, _ = ag.anchors_once(sx, sy, 14, softMask, am.default_params(), **kw)
        assert got.tolist() == [[x, y, n, 7] for x, y, n in want], (case, softMask)
    plain = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7)
    assert plain.tolist() == [[x, y, n, 7] for x, y, n in ag.anchors_once(sx, sy, 14, True, am.default_params())[0]]


def test_the_constructed_cases_do_what_they_were_made_for():
    def runs(case):
        sx, sy, kw = gc.CASES[case]
        return api.find_anchor_runs_once(sx, sy, options=_options(**kw)).tolist()
    assert [r[0] - r[1] for r in runs("deletion of 3")] == [0, 3] and [r[0] - r[1] for r in runs("deletion of 31")] == [0, 31]
    assert len(runs("deletion of 32")) == 1 and len(runs("yDrop 100")) == 1
    assert [r[0] - r[1] for r in runs("insertion before")] == [0, -7]
    assert 0 < runs("128 diagonals")[1][2] < runs("deletion of 3")[1][2]
    assert len(runs("both sides")) == 3 and len(runs("touching, n = 0")) == 2 and len(runs("touching, m = 0")) == 2


def test_one_batch_of_six_equals_the_model_through_the_recursion():
    problems = list(_batch())
    runs, stats = api.find_anchor_runs_many(problems, options=_options(1))
    want = _batch_model(**ON)
    for i in range(len(problems)):
        _same(runs[i], stats[i], want[i][0], want[i][1], i)
    assert len({st["chained"] for st in stats}) > 1
    # a limit small enough for step 6 to recurse into the gaps between extended runs
    runs, stats = api.find_anchor_runs_many(problems, anchorMatrixBiggerThanThis=60 * 60, repeatMaskMatrixBiggerThanThis=60 * 60,
                                            options=_options(1))
    for i, (sx, sy) in enumerate(problems):
        want_runs, want_stats = ag.find_anchor_runs(sx, sy, anchorMatrixBiggerThanThis=60 * 60, repeatMaskMatrixBiggerThanThis=60 * 60,
                                                    gapped=1)
        _same(runs[i], stats[i], want_runs, want_stats, i)
    assert sum(st["subProblems"] for st in stats) > 6


def test_the_option_off_is_a_call_without_options():
    problems = list(_batch())
    plain_runs, plain_stats = api.find_anchor_runs_many(problems)
    runs, stats = api.find_anchor_runs_many(problems, options=_options(0))
    want = _batch_model()
    gained = 0
    on_runs, on_stats = api.find_anchor_runs_many(problems, options=_options(1))
    for i in range(len(problems)):
        _same(runs[i], stats[i], want[i][0], want[i][1], i)
        assert np.array_equal(runs[i], plain_runs[i])
        assert {k: stats[i][k] for k in COUNTS} == {k: plain_stats[i][k] for k in COUNTS}
        gained += on_stats[i]["anchorColumns"] > stats[i]["anchorColumns"]
    assert gained >= 3


def test_both_strands_and_a_forced_minus_strand_equal_the_model():
    sx, sy = ac.masked_pair(2, 3001)                                        # an odd length: nibbles straddle bytes
    problems = [(sx, sm.rc(sy)), ac.random_pair(1, 3000)]
    runs, stats, strands = api.find_anchor_runs_many_stranded(problems, strand="both", options=_options(1))
    for i, (a, b) in enumerate(problems):
        want, wst, wstrand = ag.find_anchor_runs_stranded(a, b, "both", gapped=1)
        assert strands[i] == wstrand, i
        _same(runs[i], stats[i], want, wst, i)
    assert [s["strand"] for s in strands] == ["minus", "plus"]
    got, st = api.find_anchor_runs(sx, sm.rc(sy), strand="minus", options=_options(1))
    want, wst, _ = ag.find_anchor_runs_stranded(sx, sm.rc(sy), "minus", gapped=1)
    _same(got, st, want, wst, "minus")


def test_transition_seeds_with_their_threshold_equal_the_model():
    sx, sy = ac.masked_pair(1, 3000)
    got, st = api.find_anchor_runs(sx, sy, params=api.anchor_params_default(seedTransitions=1), options=_options(1, threshold=1200))
    want, wst = ag.find_anchor_runs(sx, sy, seedTransitions=1, threshold=1200, gapped=1)
    _same(got, st, want, wst, "transitions")


def test_64_diagonals_equal_the_model():
    sx, sy = ac.random_pair(2, 3000)
    got, st = api.find_anchor_runs(sx, sy, options=_options(1, gappedMaxDiagonals=64))
    want, wst = ag.find_anchor_runs(sx, sy, gapped=1, gappedMaxDiagonals=64)
    _same(got, st, want, wst, "64 diagonals")
    whole, _ = ag.find_anchor_runs(sx, sy, gapped=1)
    assert not np.array_equal(want, whole)                                  # the limit cuts on this pair


def test_a_y_drop_of_its_own_equals_the_model():
    sx, sy = ac.random_pair(3, 3000)
    got, st = api.find_anchor_runs(sx, sy, options=_options(1, yDrop=600))
    want, wst = ag.find_anchor_runs(sx, sy, gapped=1, yDrop=600)
    _same(got, st, want, wst, "yDrop 600")


def test_the_dog_pair_equals_the_model_end_to_end():
    sx, sy, _, _ = rc.encode_human_other("dog")
    got, st = api.find_anchor_runs(sx, sy, options=_options(1))
    want, wst = ag.find_anchor_runs(sx, sy, gapped=1)
    _same(got, st, want, wst, "dog")
    assert st["runs"] > 162 and st["anchorColumns"] > 8389                  # more than without the option


def test_get_aligned_pairs_with_the_option_is_the_anchored_call_on_the_models_anchors():
    sx, sy = _batch()[0]
    smachine = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    got = api.getAlignedPairs(smachine, sx, sy, p, anchorOptions=_options(1))
    want_runs = _batch_model(**ON)[0][0]
    assert len(want_runs) > len(_batch_model()[0][0])
    assert np.array_equal(got, api.getAlignedPairsUsingAnchors(smachine, sx, sy, np.array(am.runs_to_anchors(want_runs)), p))
