"""Seed hits that tolerate one transition, on the GPU against their definition (tests/anchor_model_transitions.py): runs
and statistics integer for integer on constructed, random, masked and ENCODE inputs, through the recursion, the strand pass
and the HSP cap; getAlignedPairs with the option against the oracle fed the model's anchors."""
import functools
import os

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import anchor_model_transitions as amt
import anchor_transition_cases as tc
import reference_cases as rc
import strand_model as sm
from cpecan_amd import api
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_transitions_oracle_pairs.npz")
COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")


def _on(**kw):
    return api.anchor_params_default(seedTransitions=1, **kw)


def _same(got_runs, got_stats, want_runs, want_stats, what):
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, what


@functools.lru_cache(maxsize=None)
def _mouse():
    sx, sy, _, _ = rc.encode_human_other("mouse")
    return (sx, sy) + amt.find_anchor_runs(sx, sy, seedTransitions=1)


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_constructed_pairs_equal_the_model(which):
    sx, sy = tc.case(which)
    got, st = api.find_anchor_runs(sx, sy, params=_on())
    want, wst = amt.find_anchor_runs(sx, sy, seedTransitions=1)
    _same(got, st, want, wst, which)
    assert (st["hits"] > 100 and st["runs"] == 1) if which == "a" else st["hits"] == 0
    assert st["kernelMs"] > 0.0
    # without the option, and with it spelled out as 0: no hit in any of the three
    for params in (None, api.anchor_params_default(seedTransitions=0)):
        got0, st0 = api.find_anchor_runs(sx, sy, params=params)
        assert len(got0) == 0 and st0["hits"] == 0


def test_one_call_of_mixed_problems_equals_the_model_problem_by_problem():
    small = ac.random_pair(41, 300)
    problems = [ac.random_pair(1, 600), ac.masked_pair(1, 600), ac.random_pair(2, 3000), ac.masked_pair(2, 3000),
                (small[0][:300], small[1][:300]), (b"", b"ACGT"), tc.case("a"), ac.insertion_pair()]
    runs, stats = api.find_anchor_runs_many(problems, params=_on())
    more = 0
    for i, (sx, sy) in enumerate(problems):
        want, wst = amt.find_anchor_runs(sx, sy, seedTransitions=1)
        _same(runs[i], stats[i], want, wst, i)
        more += wst["hits"] > am.find_anchor_runs(sx, sy)[1]["hits"]
    assert stats[4]["hits"] == 0 and len(problems[4][0]) * len(problems[4][1]) <= 500 * 500   # under the size limit
    assert stats[5]["hits"] == 0 and stats[7]["subProblems"] > 0
    assert more >= 6                                                        # the option matters on these inputs
    # steps 1-5 alone, with and without the soft mask
    sx, sy = problems[3]
    for softMask in (True, False):
        got = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, softMask=softMask, params=_on())
        want, counts = amt.anchors_once(sx, sy, 14, softMask, am.default_params(), 1)
        assert counts["chained"] > 0 and got.tolist() == [[x, y, n, 7] for x, y, n in want], softMask


def test_the_mouse_pair_equals_the_model_through_the_recursion():
    sx, sy, want, wst = _mouse()
    got, st = api.find_anchor_runs(sx, sy, params=_on())
    _same(got, st, want, wst, "mouse")
    assert (st["hits"], st["hsps"], st["runs"], st["anchorColumns"], st["largestGap"]) == (1537, 835, 91, 2378, 6150522)
    assert st["subProblems"] >= 22


def test_both_strands_equal_the_model():
    sx, sy = ac.masked_pair(2, 3001)                                        # an odd length: nibbles straddle bytes
    px, py = ac.random_pair(3, 3000)
    problems = [(sx, sm.rc(sy)), (px, py), tc.case("a")]
    runs, stats, strands = api.find_anchor_runs_many_stranded(problems, strand="both", params=_on())
    for i, (x, y) in enumerate(problems):
        want, wst, wstrand = amt.find_anchor_runs_stranded(x, y, "both", seedTransitions=1)
        assert strands[i] == wstrand, i
        _same(runs[i], stats[i], want, wst, i)
    assert [s["strand"] for s in strands] == ["minus", "plus", "plus"]
    assert all(min(s["scorePlus"], s["scoreMinus"]) >= 0 and max(s["scorePlus"], s["scoreMinus"]) > 0 for s in strands)
    # the scores differ from those without the option: the strand pass runs step 1 as the parameters say
    assert strands[2]["scorePlus"] > sm.strand_score(*tc.case("a")) == 0
    # a forced minus strand
    got, st = api.find_anchor_runs(sx, sm.rc(sy), strand="minus", params=_on())
    want, wst, _ = amt.find_anchor_runs_stranded(sx, sm.rc(sy), "minus", seedTransitions=1)
    _same(got, st, want, wst, "minus")


def test_the_cap_cuts_as_the_model_says():
    sx, sy = ac.masked_pair(5, 4000)
    got, st = api.find_anchor_runs(sx, sy, trim=3, params=_on(maxHsps=5))
    want, wst = amt.find_anchor_runs(sx, sy, trim=3, params=am.default_params(maxHsps=5), seedTransitions=1)
    _same(got, st, want, wst, "cap")
    assert wst["capped"] == 1 and wst["hsps"] > 5


def test_other_seeds_and_several_occurrences_equal_the_model():
    sx, sy = ac.masked_pair(5, 4000)
    for kw in (dict(seed="111111111111", maxSeedOccurrences=3), dict(seed="110110110110110", hspThreshold=1500, xDrop=300)):
        got, st = api.find_anchor_runs(sx, sy, trim=3, params=_on(**kw))
        want, wst = amt.find_anchor_runs(sx, sy, trim=3, params=am.default_params(**kw), seedTransitions=1)
        _same(got, st, want, wst, kw)
        assert wst["hits"] > am.find_anchor_runs(sx, sy, trim=3, params=am.default_params(**kw))[1]["hits"] > 0


def test_get_aligned_pairs_on_the_mouse_pair_equals_the_oracle_fed_the_models_anchors():
    """The oracle's answer is recorded (tests/golden/make_transitions_fixture.py: it takes a quarter of a minute on this
    pair); the anchors it was fed are recorded with it and must still be the model's."""
    sx, sy, want_runs, _ = _mouse()
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["runs"], want_runs)
    smachine = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    got = api.getAlignedPairs(smachine, sx, sy, p, anchorParams=_on())
    assert len(gold["pairs"]) > 60000
    assert_pairs_match(got, gold["pairs"], threshold=p.threshold)
    # the anchors are the model's, so the call is the anchored one on them
    assert np.array_equal(got, api.getAlignedPairsUsingAnchors(smachine, sx, sy, np.array(am.runs_to_anchors(want_runs)), p))
