"""A threshold of their own for HSPs that only variant hits seed (cpecan_anchor_options.transitionHspThreshold), on the GPU
against its definition (tests/anchor_model_threshold.py): runs and statistics integer for integer on constructed, random,
masked and ENCODE inputs, through the recursion, the strand pass and the HSP cap; the identities at the two ends of the
threshold's range; getAlignedPairs with the option against the oracle fed the model's anchors."""
import functools
import os

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import anchor_model_threshold as ath
import anchor_threshold_cases as thc
import anchor_transition_cases as tc
import reference_cases as rc
import strand_model as sm
from cpecan_amd import api
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dog_threshold_oracle_pairs.npz")
COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")
T = 1200


def _on(**kw):
    return api.anchor_params_default(seedTransitions=1, **kw)


def _same(got_runs, got_stats, want_runs, want_stats, what, counts=COUNTS):
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in counts} == {k: int(want_stats[k]) for k in counts}, what


def _mixed_problems():
    """The list of test_gpu_anchor_transitions.test_one_call_of_mixed_problems_equals_the_model_problem_by_problem."""
    small = ac.random_pair(41, 300)
    return [ac.random_pair(1, 600), ac.masked_pair(1, 600), ac.random_pair(2, 3000), ac.masked_pair(2, 3000),
            (small[0][:300], small[1][:300]), (b"", b"ACGT"), tc.case("a"), ac.insertion_pair()]


@functools.lru_cache(maxsize=None)
def _dog():
    sx, sy, _, _ = rc.encode_human_other("dog")
    return (sx, sy) + ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=T)


def test_the_smallest_case_stands_and_falls_with_the_threshold():
    sx, sy = tc.case("a")                                       # one HSP, every hit a variant hit
    kept, hits = ath.classed_hsps(sx, sy, True, am.default_params(), 1, 0)
    ((hsp, exact),) = kept.items()
    assert not exact and hits > 100
    score = hsp[3]
    got, st = api.find_anchor_runs(sx, sy, params=_on(), options=api.anchor_options(score + 1))
    want, wst = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=score + 1)
    _same(got, st, want, wst, "one above")
    # `hits` counts every hit whatever becomes of it -- twice here: with no run the whole pair is one gap over the size
    # limit, and step 6 searches it again, soft mask on as at the top level
    assert len(got) == 0 and st["hsps"] == 0 and st["subProblems"] == 1 and st["hits"] == 2 * hits
    got, st = api.find_anchor_runs(sx, sy, params=_on(), options=api.anchor_options(score))
    want, wst = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=score)
    _same(got, st, want, wst, "at the score")
    assert len(got) == 1 and st["hsps"] == 1


def test_mixed_classes_keep_the_exact_and_the_strong():
    sx, sy = thc.mixed_classes()
    got, st = api.find_anchor_runs(sx, sy, params=_on(), options=api.anchor_options(thc.THRESHOLD))
    want, wst = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=thc.THRESHOLD)
    _same(got, st, want, wst, "mixed")
    # A (exact hits, under the threshold) and B (variant hits only, over it) are chained; C (variant only, under) is not
    assert (st["hsps"], st["chained"]) == (2, 2)
    assert [int(r[0]) - 14 for r in got] == [thc.STRETCHES["A"][0], thc.STRETCHES["B"][0]]
    got, st = api.find_anchor_runs(sx, sy, params=_on())
    assert (st["hsps"], st["chained"]) == (3, 3)
    # steps 1-5 alone take the options too
    for softMask in (True, False):
        got = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, softMask=softMask, params=_on(),
                                        options=api.anchor_options(thc.THRESHOLD))
        want, counts = ath.anchors_once(sx, sy, 14, softMask, am.default_params(), 1, thc.THRESHOLD)
        assert counts["chained"] == 2 and got.tolist() == [[x, y, n, 7] for x, y, n in want], softMask


def test_one_call_of_mixed_problems_equals_the_model_and_the_identities_hold():
    problems = _mixed_problems()
    runs, stats = api.find_anchor_runs_many(problems, params=_on(), options=api.anchor_options(T))
    fewer = 0
    for i, (sx, sy) in enumerate(problems):
        want, wst = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=T)
        _same(runs[i], stats[i], want, wst, i)
        fewer += wst["hsps"] < ath.find_anchor_runs(sx, sy, seedTransitions=1)[1]["hsps"]
    assert stats[4]["hits"] == 0 and len(problems[4][0]) * len(problems[4][1]) <= 500 * 500   # under the size limit
    assert stats[5]["hits"] == 0 and stats[7]["subProblems"] > 0
    assert fewer >= 1                                                       # the threshold matters on these inputs
    # T = hspThreshold, and 0 which stands for it, is a call without options
    plain_runs, plain_stats = api.find_anchor_runs_many(problems, params=_on())
    for options in (api.anchor_options(800), api.anchor_options(0)):
        runs, stats = api.find_anchor_runs_many(problems, params=_on(), options=options)
        for i in range(len(problems)):
            _same(runs[i], stats[i], plain_runs[i], plain_stats[i], i)
    # T = INT32_MAX is a seedTransitions = 0 call but for the hits
    off_runs, off_stats = api.find_anchor_runs_many(problems)
    runs, stats = api.find_anchor_runs_many(problems, params=_on(), options=api.anchor_options(2 ** 31 - 1))
    more = 0
    for i in range(len(problems)):
        _same(runs[i], stats[i], off_runs[i], off_stats[i], i, [k for k in COUNTS if k != "hits"])
        more += stats[i]["hits"] > off_stats[i]["hits"]
    assert more >= 6
    # with seedTransitions = 0 the threshold has no effect
    runs, stats = api.find_anchor_runs_many(problems, options=api.anchor_options(2 ** 31 - 1))
    for i in range(len(problems)):
        _same(runs[i], stats[i], off_runs[i], off_stats[i], i)


def test_the_dog_pair_equals_the_model_through_the_recursion():
    sx, sy, want, wst = _dog()
    got, st = api.find_anchor_runs(sx, sy, params=_on(), options=api.anchor_options(T))
    _same(got, st, want, wst, "dog")
    assert (st["runs"], st["anchorColumns"], st["largestGap"]) == (232, 10866, 5028764)
    assert st["hsps"] > 256 and st["subProblems"] >= 17


def test_both_strands_equal_the_model():
    sx, sy = ac.masked_pair(2, 3001)                                        # an odd length: nibbles straddle bytes
    x, ya = tc.case("a")
    (score,) = [h[3] for h in ath.classed_hsps(x, ya, True, am.default_params(), 1, 0)[0]]
    for threshold, want_strands in ((T, ["minus", "plus"]), (score + 1, ["minus", "plus"])):
        problems = [(sx, sm.rc(sy)), (x, ya)]
        runs, stats, strands = api.find_anchor_runs_many_stranded(problems, strand="both", params=_on(),
                                                                  options=api.anchor_options(threshold))
        for i, (a, b) in enumerate(problems):
            want, wst, wstrand = ath.find_anchor_runs_stranded(a, b, "both", seedTransitions=1, threshold=threshold)
            assert strands[i] == wstrand, (threshold, i)
            _same(runs[i], stats[i], want, wst, (threshold, i))
        assert [s["strand"] for s in strands] == want_strands
        # the strand pass runs step 2 with the threshold: case("a") scores on the plus strand only while its HSP is kept
        assert (strands[1]["scorePlus"] > 0) == (threshold <= score)
    # a forced minus strand
    got, st = api.find_anchor_runs(sx, sm.rc(sy), strand="minus", params=_on(), options=api.anchor_options(T))
    want, wst, _ = ath.find_anchor_runs_stranded(sx, sm.rc(sy), "minus", seedTransitions=1, threshold=T)
    _same(got, st, want, wst, "minus")


def test_the_cap_cuts_as_the_model_says():
    sx, sy = ac.masked_pair(5, 4000)
    got, st = api.find_anchor_runs(sx, sy, trim=3, params=_on(maxHsps=5), options=api.anchor_options(T))
    want, wst = ath.find_anchor_runs(sx, sy, trim=3, params=am.default_params(maxHsps=5), seedTransitions=1, threshold=T)
    _same(got, st, want, wst, "cap")
    assert wst["capped"] == 1 and wst["hsps"] > 5


def test_get_aligned_pairs_on_the_dog_pair_equals_the_oracle_fed_the_models_anchors():
    """The oracle's answer is recorded (tests/golden/make_threshold_fixture.py: it takes a third of a minute on this
    pair); the anchors it was fed are recorded with it and must still be the model's."""
    sx, sy, want_runs, _ = _dog()
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["runs"], want_runs)
    smachine = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    got = api.getAlignedPairs(smachine, sx, sy, p, anchorParams=_on(), anchorOptions=api.anchor_options(T))
    assert len(gold["pairs"]) > 60000
    assert_pairs_match(got, gold["pairs"], threshold=p.threshold)
    # the anchors are the model's, so the call is the anchored one on them
    assert np.array_equal(got, api.getAlignedPairsUsingAnchors(smachine, sx, sy, np.array(am.runs_to_anchors(want_runs)), p))
