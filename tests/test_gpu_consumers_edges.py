"""The list consumers (cpk_post.inl) at the chunk, tile and ring edges of the wave kernels: every input of
tests/consumer_cases.py (device-free; tests/test_consumer_cases_cpu.py proves what each is for) through the kernels, in the
wave form (default) and the lane form (CPECAN_POST_LANES=1), against the oracle -- and the ordered filter against the
quadratic model of tests/ordered_model.py as well.  Integer / order-defined arithmetic: the gate is equality everywhere,
lists element for element in order, scores as equal doubles.

No case is kept out of the lane form: its longest quadratic walk (MEA far_predecessor, 2116 pairs that all walk back to the
front of the list, 2.2 M steps of one lane) takes 0.6 s.
"""
import random

import numpy as np
import pytest

import consumer_cases as cc
import oracle_binding as ob
import ordered_model as om
from cpecan_amd import api
from test_gpu_parity import _evolve, _rand_seq, _sm

pytestmark = pytest.mark.gpu

MEA = cc.mea_cases()
ORD = cc.ordered_cases()
SHIFT = cc.shift_cases()
REW = cc.reweight_cases()
MEA_WAVE_ONLY = tuple(k for k in sorted(MEA) if not MEA[k]["lanes"])
FORMS = (None, "1")  # CPECAN_POST_LANES


def _tuples(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def _form(monkeypatch, lanes):
    if lanes:
        monkeypatch.setenv("CPECAN_POST_LANES", lanes)
    else:
        monkeypatch.delenv("CPECAN_POST_LANES", raising=False)


@pytest.mark.parametrize("name", sorted(MEA))
def test_mea_case(name, monkeypatch):
    c = MEA[name]
    want, want_score = ob.mea_alignment(c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"], c["gamma"])
    assert (len(want) == 0) == (name in cc.MEA_EMPTY)
    assert MEA_WAVE_ONLY == ()
    seen = []
    for lanes in FORMS:
        if lanes and name in MEA_WAVE_ONLY:
            continue
        _form(monkeypatch, lanes)
        got, score = api.getMaximalExpectedAccuracyPairwiseAlignment(c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"],
                                                                     gapGamma=c["gamma"])
        assert _tuples(got) == _tuples(want), (name, lanes)
        assert score == want_score, (name, lanes)
        seen.append((_tuples(got), score))
    assert all(s == seen[0] for s in seen)  # the wave and the lane form, bit for bit


@pytest.mark.parametrize("name", sorted(ORD))
def test_ordered_case(name, monkeypatch):
    c = ORD[name]
    want = _tuples(ob.filter_pairs_ordered(c["pairs"], c["lX"], c["lY"], c["gamma"]))
    assert want == om.filter_pairs_ordered(c["pairs"], c["gamma"])
    assert (len(want) == 0) == (name in cc.ORDERED_EMPTY)
    for lanes in FORMS:
        _form(monkeypatch, lanes)
        got = api.filterPairwiseAlignmentToMakePairsOrdered(c["pairs"], "A" * c["lX"], "A" * c["lY"], c["gamma"])
        assert _tuples(got) == want, (name, lanes)


def test_ordered_random_lists_with_ties_against_the_model(monkeypatch):
    for seed in range(0, 300, 5):
        c = cc.ord_random_ties(seed)
        want = om.filter_pairs_ordered(c["pairs"], c["gamma"])
        for lanes in FORMS:
            _form(monkeypatch, lanes)
            got = api.filterPairwiseAlignmentToMakePairsOrdered(c["pairs"], "A" * c["lX"], "A" * c["lY"], c["gamma"])
            assert _tuples(got) == want, (seed, lanes)


@pytest.mark.parametrize("name", sorted(SHIFT))
def test_left_shift_case(name):
    """One lane per problem; POST_LEFT_SHIFT alone, i.e. through cpecan_post_copy_chain."""
    c = SHIFT[name]
    want = _tuples(ob.left_shift_alignment(c["pairs"], c["sx"], c["sy"]))
    assert len(want) >= 2
    assert _tuples(api.leftShiftAlignment(c["pairs"], c["sx"], c["sy"])) == want


@pytest.mark.parametrize("name", sorted(REW))
def test_reweight_and_scores_case(name):
    c = REW[name]
    n, lX, lY = len(c["pairs"]), c["lX"], c["lY"]
    for gamma in c["gammas"]:
        got = api.reweightAlignedPairs2(c["pairs"], lX, lY, gamma)
        want = ob.reweight_aligned_pairs(c["pairs"], lX, lY, gamma)
        assert got.shape == (n, 3) and (got.astype(np.int64) == want).all(), (name, gamma)
        if gamma <= 0:
            assert _tuples(got) == c["pairs"]
        assert api.scoreByPosteriorProbability(lX, lY, want) == ob.score_by_posterior(lX, lY, want)
        by_pairs = api.scoreByPosteriorProbabilityIgnoringGaps(want)
        if n:
            assert by_pairs == ob.score_by_posterior_ignoring_gaps(want)
        else:
            assert np.isnan(by_pairs) and np.isnan(ob.score_by_posterior_ignoring_gaps(want))  # 0 / 0, as in the reference


def test_identity_scores_with_n_and_lower_case():
    c = cc.IDENTITY
    assert api.scoreByIdentity(c["sx"], c["sy"], len(c["sx"]), len(c["sy"]), c["pairs"]) == ob.score_by_identity(c["sx"], c["sy"], c["pairs"])
    assert api.scoreByIdentityIgnoringGaps(c["sx"], c["sy"], c["pairs"]) == ob.score_by_identity_ignoring_gaps(c["sx"], c["sy"], c["pairs"])
    assert api.scoreByIdentityIgnoringGaps(c["sx"], c["sy"], c["pairs"]) == 100.0 * 9 / 13
    assert np.isnan(api.scoreByIdentityIgnoringGaps(c["sx"], c["sy"], []))


# ---- batches: seqOff, chainOff, meaOut and shiftOut of one problem lie behind another's ----
def _batch_problems(count, seed):
    """Problems of 30-200 related bases with, between them, an empty sequence, unrelated short sequences and a pair of
    identical sequences: lists of very different lengths, some empty, side by side in the consumers' buffers."""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        if i % 9 == 4:
            out.append(("", _rand_seq(rng, 7)) if i % 2 else (_rand_seq(rng, 5), ""))
        elif i % 9 == 7:
            out.append((_rand_seq(rng, rng.randrange(1, 4)), _rand_seq(rng, rng.randrange(1, 4))))
        elif i % 9 == 2:
            s = _rand_seq(rng, rng.randrange(30, 90))
            out.append((s, s))
        else:
            sx = _rand_seq(rng, rng.randrange(30, 200))
            out.append((sx, _evolve(rng, sx) or "A"))
    return out


@pytest.mark.parametrize("count", (63, 64, 65))
def test_batch_mea_and_left_shift(count, monkeypatch):
    """63, 64 and 65 problems sit on the `p >= nProblems` guard of the lane kernels (64 lanes a block): the left shift
    always, the MEA chain under CPECAN_POST_LANES.  Every problem against the oracle's chain of the same steps on the lists
    the device emitted; the two forms bit for bit."""
    probs = _batch_problems(count, 700 + count)
    p = api.pairwiseAlignmentBandingParameters_construct()
    gamma = float(np.float32(0.5))
    seen = []
    for lanes in FORMS:
        _form(monkeypatch, lanes)
        with api.Batch(_sm(0), p, emit=api.EMIT_INDEL) as b:
            b.set_post(api.POST_MEA | api.POST_LEFT_SHIFT, gamma)
            for sx, sy in probs:
                b.add(sx, sy, ())
            b.upload()
            b.run()
            b.download()
            outs = []
            empties = chains = 0
            for i, (sx, sy) in enumerate(probs):
                m, gx, gy = b.result(i, 0), b.result(i, 1), b.result(i, 2)
                mea, score = ob.mea_alignment(m, gx, gy, len(sx), len(sy), gamma)
                want = ob.left_shift_alignment(mea, sx, sy)
                got = b.result(i, 3)
                assert _tuples(got) == _tuples(want), (i, lanes)
                assert b.scores(i)[2] == score, (i, lanes)
                empties += len(m) == 0
                chains += len(want) >= 20
                if sx and sx == sy:
                    assert len(want) == len(sx)  # identical sequences: min(lX, lY) entries, the most a left shift writes
                outs.append((_tuples(got), b.scores(i)[2]))
            assert empties >= 5 and chains >= 35
            seen.append(outs)
    assert seen[0] == seen[1]


@pytest.mark.parametrize("count", (63, 64, 65))
def test_batch_reweight_then_ordered(count, monkeypatch):
    probs = _batch_problems(count, 800 + count)
    p = api.pairwiseAlignmentBandingParameters_construct()
    gap_gamma, match_gamma = float(np.float32(0.5)), 0.6
    seen = []
    for lanes in FORMS:
        _form(monkeypatch, lanes)
        with api.Batch(_sm(0), p) as b:
            b.set_post(api.POST_REWEIGHT | api.POST_ORDERED, gap_gamma, match_gamma)
            for sx, sy in probs:
                b.add(sx, sy, (), True, True)
            b.upload()
            b.run()
            b.download()
            outs = []
            kept = 0
            for i, (sx, sy) in enumerate(probs):
                reweighted = b.result(i)  # list 0, as the device reweighted it
                want = ob.filter_pairs_ordered(reweighted, len(sx), len(sy), match_gamma)
                got = b.result(i, 3)
                assert _tuples(got) == _tuples(want), (i, lanes)
                assert _tuples(got) == om.filter_pairs_ordered(_tuples(reweighted), match_gamma), (i, lanes)
                by_post, by_post_ig, _ = b.scores(i)
                by_id, by_id_ig = b.identity_scores(i)
                assert by_post == ob.score_by_posterior(len(sx), len(sy), want)
                assert by_id == ob.score_by_identity(sx, sy, want)
                if len(want):
                    assert by_post_ig == ob.score_by_posterior_ignoring_gaps(want)
                    assert by_id_ig == ob.score_by_identity_ignoring_gaps(sx, sy, want)
                else:
                    assert np.isnan(by_post_ig) and np.isnan(by_id_ig)
                kept += len(want) >= 15
                outs.append(_tuples(got))
            assert kept >= 35
            seen.append(outs)
    assert seen[0] == seen[1]


def test_batch_reweight_is_the_oracle_on_the_plain_lists():
    """POST_REWEIGHT in a batch against the oracle's reweighting of the lists the same batch emits without it."""
    probs = _batch_problems(65, 900)
    p = api.pairwiseAlignmentBandingParameters_construct()
    gamma = cc.F085

    def run(flags):
        with api.Batch(_sm(0), p) as b:
            b.set_post(flags, gamma)
            for sx, sy in probs:
                b.add(sx, sy, ())
            b.upload()
            b.run()
            b.download()
            return [b.result(i) for i in range(len(probs))]

    plain, rew = run(0), run(api.POST_REWEIGHT)
    changed = 0
    for i, (sx, sy) in enumerate(probs):
        want = ob.reweight_aligned_pairs(plain[i], len(sx), len(sy), gamma)
        assert (rew[i].astype(np.int64) == want).all(), i
        changed += bool((want[:, 0] != plain[i][:, 0]).any())
    assert changed >= 35


def test_batch_of_identical_sequences_fills_the_left_shift_outputs():
    """Identical sequences between ordinary problems, MEA and left shift: each identical problem's output has min(lX, lY)
    entries -- all a left shift can write besides the chain it is given, the bound its slice of shiftOut is sized by -- and
    the neighbours' outputs, in the slices before and behind, are still the oracle's."""
    rng = random.Random(77)
    probs = []
    for i in range(12):
        if i % 2:
            s = ("A" * rng.randrange(20, 60)) if i % 4 == 1 else _rand_seq(rng, rng.randrange(20, 60))
            probs.append((s, s))
        else:
            sx = _rand_seq(rng, rng.randrange(30, 120))
            probs.append((sx, _evolve(rng, sx) or "A"))
    p = api.pairwiseAlignmentBandingParameters_construct()
    gamma = float(np.float32(0.5))
    with api.Batch(_sm(0), p, emit=api.EMIT_INDEL) as b:
        b.set_post(api.POST_MEA | api.POST_LEFT_SHIFT, gamma)
        for sx, sy in probs:
            b.add(sx, sy, ())
        b.upload()
        b.run()
        b.download()
        for i, (sx, sy) in enumerate(probs):
            mea, score = ob.mea_alignment(b.result(i, 0), b.result(i, 1), b.result(i, 2), len(sx), len(sy), gamma)
            want = ob.left_shift_alignment(mea, sx, sy)
            got = b.result(i, 3)
            assert _tuples(got) == _tuples(want), i
            if sx == sy:
                assert len(got) == min(len(sx), len(sy))
                assert got[:, 1].tolist() == list(range(len(sx))) and got[:, 2].tolist() == list(range(len(sx)))
            else:
                assert len(got) >= 10
