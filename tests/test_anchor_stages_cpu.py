"""The host stages of the anchor finder without a GPU (tests/anchor_stages.py): check, layout, strand pick, gaps and splice
of cpecan_anchor.c run around the model, which plays cpk_anchor_pass, and the result is strand_model's, integer for
integer -- runs, the nine counts, the strand and both scores.  Every problem list the stages make goes through
cpk_anchor_pass_plan on the way (anchor_stages.check_plan); the plan's contract checks get one hand-made list each."""
import ctypes as C

import pytest

import anchor_cases as ac
import anchor_stages as st
import strand_model as sm
from cpecan_amd import api

COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")


def test_the_mirrors_have_the_sizes_of_the_c_structures():
    assert C.sizeof(st.PassProblem) == 112 and C.sizeof(st.PassParams) == 116 and C.sizeof(st.Pass) == 160
    assert C.sizeof(st.Plan) == 72 and C.sizeof(st.Call) == 96 and C.sizeof(st.List) == 40


def _agree(problems, strand, **kw):
    """run_call against the model on every problem; returns (statistics, strands, facts) of the stages."""
    model_kw = {k: v for k, v in kw.items() if k not in ("once", "softMaskTop")}
    runs, stats, strands, facts = st.run_call(problems, strand, **kw)
    for i, (sx, sy) in enumerate(problems):
        want_runs, want_stats, want_strand = sm.find_anchor_runs_stranded(sx, sy, strand, **model_kw)
        assert runs[i] == [tuple(r) for r in want_runs.tolist()], (i, strand)
        assert {k: stats[i][k] for k in COUNTS} == {k: want_stats[k] for k in COUNTS}, (i, strand)
        assert strands[i] == want_strand, (i, strand)
    return stats, strands, facts


@pytest.mark.parametrize("maskLimit", [500 * 500, 10 ** 9])
def test_insertion_pair_recurses_into_two_gaps(maskLimit):
    stats, _, facts = _agree([ac.insertion_pair()], "plus", repeatMaskMatrixBiggerThanThis=maskLimit)
    assert stats[0]["subProblems"] == 2 and facts["gaps"] == [0, 0]


def test_unrelated_sequences_are_one_gap():
    stats, _, _ = _agree([(ac.random_pair(1, 700)[0], ac.random_pair(2, 700)[0])], "plus")
    assert (stats[0]["subProblems"], stats[0]["runs"], stats[0]["largestGap"]) == (1, 0, 490000)


@pytest.fixture(scope="module")
def stranded_batch():
    return [(sx, sm.rc(sy) if i % 2 else sy) for i, (sx, sy) in enumerate(ac.mixed_batch(48))]


def test_mixed_batch_on_both_strands(stranded_batch):
    _, strands, facts = _agree(stranded_batch, "both")
    small = [i for i, (sx, sy) in enumerate(stranded_batch) if len(sx) * len(sy) <= 500 * 500]
    assert small == [31] and 31 in facts["scored"] and 31 not in facts["searched"]      # the compaction
    assert facts["scored"] == list(range(48)) and facts["searched"] == [i for i in range(48) if i != 31]
    assert sorted(set(facts["gaps"])) == [7]                                            # the recursion
    assert [s["strand"] for s in strands] == ["minus" if i % 2 else "plus" for i in range(48)]     # the twins


@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_mixed_batch_on_a_forced_strand(stranded_batch, strand):
    _, strands, facts = _agree(stranded_batch, strand)
    assert 31 not in facts["scored"] and facts["searched"] == facts["scored"]
    assert all(s["strand"] == strand for s in strands)


def test_edge_cases():
    for strand in ("plus", "minus", "both"):
        _agree([(b"", b"ACGT")], strand)
        _agree([(b"ACGT", b"")], strand)
        assert st.run_call([], strand) == ([], [], [], dict(scored=[], searched=[], gaps=[]))


@pytest.mark.parametrize("softMaskTop", [0, 1])
def test_once_mode(softMaskTop):
    """Steps 1-5 alone: the model's anchors_once with the soft mask the caller chose, whatever the size, no recursion."""
    import anchor_model as am
    sx, sy = ac.masked_pair(1, 2000)
    runs, _, _, facts = st.run_call([(sx, sy)], "plus", expansion=7, anchorMatrixBiggerThanThis=0,
                                    repeatMaskMatrixBiggerThanThis=0, once=True, softMaskTop=softMaskTop)
    want, _ = am.anchors_once(sx, sy, 14, bool(softMaskTop), am.default_params())
    assert runs[0] == [(x, y, length, 7) for x, y, length in want] and len(want) > 0
    assert facts["searched"] == [0] and facts["gaps"] == []


def test_once_mode_masks_differ():
    import anchor_model as am
    sx, sy = ac.masked_pair(1, 2000)
    assert am.anchors_once(sx, sy, 14, True, am.default_params()) != am.anchors_once(sx, sy, 14, False, am.default_params())


# ---- the contract checks of cpk_anchor_pass_plan: no public call can make these lists ----
N_FORWARD, N_SYM = 1000, 1000 + 600


def _problem(**fields):
    p = st.PassProblem(xOff=0, yOff=300, lX=300, lY=200, softMask=1)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _twin(**fields):
    """The minus twin of _problem(): its Y is the reverse complement of the symbols at 300, written to the area."""
    return _problem(**dict(dict(flags=st.RC_Y | st.SHARE_X, yFwd=300, yOff=N_FORWARD), **fields))


def _plan(probs, pass_=None, nSym=N_SYM):
    arr = (st.PassProblem * len(probs))(*probs)
    rc = st.stages().cpk_anchor_pass_plan(C.byref(pass_ or st.default_pass()), arr, len(probs), nSym, N_FORWARD, C.byref(st.Plan()))
    return rc, api.lib().cpecan_last_error().decode()


def test_the_hand_made_lists_are_sound_without_their_fault():
    assert _plan([_problem(), _twin(), _problem(xOff=500, yOff=800)])[0] == st.OK
    assert _plan([_problem(flags=st.RC_Y, yFwd=300, yOff=N_FORWARD + 2)])[0] == st.OK
    st.check_plan(st.default_pass(), (st.PassProblem * 2)(_problem(), _twin()), 2, N_SYM, N_FORWARD)


BAD_LISTS = [
    ("a twin first in the list", [_twin()], "twin"),
    ("a twin behind a twin", [_problem(), _twin(), _twin()], "twin"),
    ("a twin whose lX differs", [_problem(), _twin(lX=299)], "twin"),
    ("a twin whose soft mask differs", [_problem(), _twin(softMask=0)], "twin"),
    ("a reverse complement to an odd offset", [_problem(flags=st.RC_Y, yFwd=300, yOff=N_FORWARD + 1)], "reverse complement"),
    ("a reverse complement inside the forward area", [_problem(flags=st.RC_Y, yFwd=300, yOff=500)], "reverse complement"),
    ("a reverse complement of symbols behind the forward area", [_problem(flags=st.RC_Y, yFwd=900, yOff=N_FORWARD)],
     "reverse complement"),
    ("X reaches past nSym", [_problem(xOff=N_SYM - 299)], "outside the buffer"),
    ("Y reaches past nSym", [_problem(), _twin(yOff=N_SYM - 198)], "outside the buffer"),
    ("a negative offset", [_problem(xOff=-2)], "outside the buffer"),
]


@pytest.mark.parametrize("case", BAD_LISTS, ids=[c[0] for c in BAD_LISTS])
def test_a_list_that_breaks_the_contract_is_refused(case):
    rc, text = _plan(case[1])
    assert rc == st.EINVAL and case[2] in text, text


def test_the_hit_bound_is_2_to_the_30():
    """lY * hitsPerWindow <= 2^30, hitsPerWindow being maxSeedOccurrences, times 1 + the seed's weight with transitions."""
    long_y = [_problem(lY=1 << 20)]
    ok = dict(nSym=1 << 22)
    assert _plan(long_y, st.default_pass(maxSeedOccurrences=1 << 10), **ok)[0] == st.OK           # 2^30 exactly
    rc, text = _plan(long_y, st.default_pass(maxSeedOccurrences=(1 << 10) + 1), **ok)
    assert rc == st.EINVAL and "too many seed occurrences" in text
    assert _plan(long_y, st.default_pass(maxSeedOccurrences=100), **ok)[0] == st.OK
    rc, text = _plan(long_y, st.default_pass(maxSeedOccurrences=100, seedTransitions=1), **ok)  # 100 * 13 per window
    assert rc == st.EINVAL and "too many seed occurrences" in text


BAD_PASSES = [
    ("a seed of 32 characters", dict(seed=b"1" + b"0" * 30 + b"1")),
    ("a seed with 16 ones", dict(seed=b"1" * 16)),
    ("a seed holding a 2", dict(seed=b"11211")),
    ("an empty seed", dict(seed=b"")),
    ("seedTransitions 2", dict(seedTransitions=2)),
    ("a variant threshold under hspThreshold", dict(variantThreshold=799)),
    ("a negative trim", dict(trim=-1)),
]


@pytest.mark.parametrize("case", BAD_PASSES, ids=[c[0] for c in BAD_PASSES])
def test_a_pass_that_breaks_the_contract_is_refused(case):
    assert _plan([_problem()], st.default_pass(seed=b"1" * 15, seedTransitions=1, variantThreshold=800))[0] == st.OK
    rc, text = _plan([_problem()], st.default_pass(**case[1]))
    assert rc == st.EINVAL and "anchor parameters" in text, text
