"""The anchor finder on the GPU against its definition (tests/anchor_model.py): runs and statistics integer for integer;
getAlignedPairs from sequences alone against the anchored path and the oracle; the ENCODE pairs without anchors from the
answer; the cpecan_align command line."""
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import oracle_binding as ob
import reference_cases as rc
from cpecan_amd import api
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")


def _same(got_runs, got_stats, want_runs, want_stats, what):
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, what
    assert 2 * want_stats["hsps"] <= am.default_params()["maxHsps"], "the input comes too close to the HSP cap"
    assert got_stats["kernelMs"] > 0.0 or want_stats["largestGapTop"] <= 500 * 500, what


def _encode(name):
    return rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)


@pytest.mark.parametrize("length", [600, 1500, 5000, 20000])
def test_random_pairs_equal_the_model(length):
    sx, sy = ac.random_pair(length, length)
    got, st = api.find_anchor_runs(sx, sy)
    want, wst = am.find_anchor_runs(sx, sy)
    assert wst["chained"] > 0
    _same(got, st, want, wst, length)


@pytest.mark.parametrize("softMask", [True, False])
def test_masked_pairs_equal_the_model_with_and_without_soft_mask(softMask):
    for index, length in ((1, 2000), (2, 6000)):
        sx, sy = ac.masked_pair(index, length)
        got = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, softMask=softMask)
        want, counts = am.anchors_once(sx, sy, 14, softMask, am.default_params())
        assert counts["chained"] > 0
        assert got.tolist() == [[x, y, n, 7] for x, y, n in want], (index, softMask)
    # the mask matters on these inputs
    sx, sy = ac.masked_pair(2, 6000)
    assert am.anchors_once(sx, sy, 14, True, am.default_params())[1]["hits"] < am.anchors_once(sx, sy, 14, False, am.default_params())[1]["hits"]


@pytest.mark.parametrize("repeatMask", [500 * 500, 10 ** 9])
def test_insertion_pair_recursion_equals_the_model(repeatMask):
    sx, sy = ac.insertion_pair()
    got, st = api.find_anchor_runs(sx, sy, repeatMaskMatrixBiggerThanThis=repeatMask)
    want, wst = am.find_anchor_runs(sx, sy, repeatMaskMatrixBiggerThanThis=repeatMask)
    assert wst["subProblems"] > 0 and wst["largestGapTop"] > 500 * 500
    _same(got, st, want, wst, repeatMask)


def test_other_parameters_equal_the_model():
    """A denser seed, several occurrences, a cap that cuts: the same agreement away from the defaults."""
    sx, sy = ac.masked_pair(5, 4000)
    for kw in (dict(seed="111111111111", maxSeedOccurrences=3), dict(hspThreshold=1500, xDrop=300), dict(maxHsps=5)):
        got, st = api.find_anchor_runs(sx, sy, trim=3, params=api.anchor_params_default(**kw))
        want, wst = am.find_anchor_runs(sx, sy, trim=3, params=am.default_params(**kw))
        assert np.array_equal(got, want), kw
        assert {k: int(st[k]) for k in COUNTS} == {k: int(wst[k]) for k in COUNTS}, kw
    assert wst["capped"] == 1


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_encode_pairs_equal_the_model(name):
    sx, sy, _, _ = _encode(name)
    got, st = api.find_anchor_runs(sx, sy)
    want, wst = am.find_anchor_runs(sx, sy)
    assert wst["subProblems"] > 0
    _same(got, st, want, wst, name)


def test_batch_of_256_mixed_problems_equals_the_model_problem_by_problem():
    problems = ac.mixed_batch(256)
    runs, stats = api.find_anchor_runs_many(problems)
    assert len(runs) == 256
    small = 0
    for i, (sx, sy) in enumerate(problems):
        want, wst = am.find_anchor_runs(sx, sy)
        _same(runs[i], stats[i], want, wst, i)
        small += len(sx) * len(sy) <= 500 * 500
    assert 0 < small < 256


def _model_anchors(sx, sy):
    return np.array(am.runs_to_anchors(am.find_anchor_runs(sx, sy)[0]), dtype=np.int64).reshape(-1, 3)


def test_get_aligned_pairs_equals_the_anchored_path_and_the_oracle():
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    for sx, sy in (ac.random_pair(31, 3000), ac.insertion_pair()):
        anchors = _model_anchors(sx, sy)
        assert len(anchors) > 0
        got = api.getAlignedPairs(sm, sx, sy, p, True, True)
        assert np.array_equal(got, api.getAlignedPairsUsingAnchors(sm, sx, sy, anchors, p, True, True))
        want = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params(), True, True)
        assert_pairs_match(got, want, threshold=p.threshold)
        gi = api.getAlignedPairsWithIndels(sm, sx, sy, p)
        wi = api.getAlignedPairsWithIndelsUsingAnchors(sm, sx, sy, anchors, p)
        for a, b in zip(gi, wi):
            assert np.array_equal(a, b)
        for a, b in zip(gi, ob.aligned_pairs_with_indels(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params())):
            assert_pairs_match(a, b, threshold=p.threshold)
        he, hw = api.hmm_constructEmpty(0.0, api.fiveState), api.hmm_constructEmpty(0.0, api.fiveState)
        api.getExpectations(sm, he, sx, sy, p)
        api.getExpectationsUsingAnchors(sm, hw, sx, sy, anchors, p)
        # The anchors are equal integer for integer (above), so both calls run the same DP.  The expectation emitter adds
        # per-wave partial sums, and which wave takes which stretch of the work is decided at run time: two runs of the SAME
        # anchored call differ in the last bits.  n non-negative doubles summed in two orders differ by at most n * 2^-53
        # relative; n stays under 1e7 events here, so 1e7 * 1.1e-16 = 1.1e-9.
        for g, w in zip(list(he.transitions) + list(he.emissions) + [he.likelihood],
                        list(hw.transitions) + list(hw.emissions) + [hw.likelihood]):
            assert abs(g - w) <= 1.1e-9 * abs(w), (g, w)
        ho = ob.hmm(ob.FIVE_STATE, 0.0)
        ob.expectations(ob.model(ob.FIVE_STATE), ho, sx, sy, anchors, ob.params())
        for g, w in zip(list(he.transitions) + list(he.emissions), list(ho.T)[:25] + list(ho.E)[:80]):
            assert abs(g - w) <= 1e-5 * max(1.0, abs(w))


def test_below_the_size_limit_nothing_changed():
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    sx, sy = ac.random_pair(41, 100)
    sx, sy = sx[:100], sy[:100]
    assert np.array_equal(api.getAlignedPairs(sm, sx, sy, p), api.getAlignedPairsUsingAnchors(sm, sx, sy, (), p))
    runs, st = api.find_anchor_runs(sx, sy)
    assert len(runs) == 0 and st["hits"] == 0


def test_add_many_unanchored_equals_add_many_runs_with_the_model_anchors():
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    problems = ac.mixed_batch(12)
    with api.Batch(sm, p) as a, api.Batch(sm, p) as b:
        _, stats = a.add_many_unanchored([(sx, sy, True, True) for sx, sy in problems])
        b.add_many([(sx, sy, _model_anchors(sx, sy), True, True) for sx, sy in problems])
        for batch in (a, b):
            batch.upload()
            batch.run()
            batch.download()
        for i in range(len(problems)):
            assert np.array_equal(a.result(i), b.result(i)), i
    assert len(stats) == 12


# The bars of tests/test_oracle_golden.py for anchors cut from the answer are chimp 0.99 / 0.99, dog 0.90 / 0.94, mouse
# 0.75 / 0.85.  From the sequences alone the model's anchors through the oracle give (profiles/anchor_quality.txt):
# chimp 0.9997 / 0.9997, dog 0.9277 / 0.9593, mouse 0.7192 / 0.8655.  chimp must clear 0.99 / 0.99 as it stands; dog and
# mouse: the model + oracle figure minus 0.005 (pairs at the 0.01 threshold that GPU and oracle may decide differently).
# The mouse pair's sensitivity stays under the 0.75 it reaches with anchors cut from the answer: its 43 runs lie on the
# embedded alignment (1256 of 1264 columns) but leave gaps of up to 7.9 k x 7.9 k that the DP crosses without a band.
ENCODE_BARS = {"chimp": (0.99, 0.99), "dog": (0.9277 - 0.005, 0.9593 - 0.005), "mouse": (0.7192 - 0.005, 0.8655 - 0.005)}


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_encode_from_sequences_alone(name):
    sx, sy, _, true_pairs = _encode(name)
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=20)
    pairs = api.getAlignedPairs(sm, sx, sy, p)
    assert len({(int(x), int(y)) for _, x, y in pairs}) == len(pairs)
    out = api.filterPairwiseAlignmentToMakePairsOrdered(pairs, sx, sy, 0.5)
    sens, spec = rc.sensitivity_specificity(out, true_pairs)
    print("encode %s from sequences alone: sensitivity %.4f specificity %.4f" % (name, sens, spec))
    assert sens > ENCODE_BARS[name][0] and spec > ENCODE_BARS[name][1], (sens, spec)


def _parse_cigar(line):
    f = line.split()
    assert f[0] == "cigar:" and f[4] == "+" and f[8] == "+"
    ops = [(f[i], int(f[i + 1])) for i in range(10, len(f), 2)]
    return f[1], int(f[2]), int(f[3]), f[5], int(f[6]), int(f[7]), ops


def test_cpecan_align_two_by_two(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    targets = {"t_long": ac.random_pair(51, 1800)[0], "t_short": ac.random_pair(52, 300)[0]}
    queries = {"q_long": ac.random_pair(51, 1800)[1], "q_short": ac.random_pair(52, 300)[1]}
    for name, seqs in (("target.fa", targets), ("query.fa", queries)):
        with open(tmp_path / name, "w") as f:
            for k, s in seqs.items():
                f.write(">%s some description\n" % k)
                s = s.decode()
                for i in range(0, len(s), 70):
                    f.write(s[i:i + 70] + "\n")
    r = subprocess.run([exe, str(tmp_path / "target.fa"), str(tmp_path / "query.fa")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 4
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    order = [(q, t) for q in queries for t in targets]          # cPecanAlign.c:112-118: queries outside, targets inside
    for line, (q, t) in zip(lines, order):
        c2, s2, e2, c1, s1, e1, ops = _parse_cigar(line)
        sx, sy = targets[t], queries[q]                         # contig1 = target = X
        assert (c1, c2) == (t, q) and (s1, e1, s2, e2) == (0, len(sx), 0, len(sy))
        x = y = 0
        got = []
        for op, n in ops:
            if op == "M":
                got += [(x + k, y + k) for k in range(n)]
            x += n if op in "MD" else 0
            y += n if op in "MI" else 0
        assert (x, y) == (len(sx), len(sy))                     # the cigar covers both sequences
        pairs = api.getAlignedPairs(sm, sx, sy, p, True, True)
        pairs = api.reweightAlignedPairs2(pairs, len(sx), len(sy), 0.5)
        want = api.filterPairwiseAlignmentToMakePairsOrdered(pairs, sx, sy, 0.9)
        assert got == sorted((int(a), int(b)) for _, a, b in want), (q, t)
    assert len(targets["t_long"]) * len(queries["q_long"]) > 500 * 500
