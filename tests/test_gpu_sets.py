"""GPU tests of the sets layer (include/cpecan_sets.h) on the cases of tests/set_cases.py, in two layers.

Against a hand-made batch: Sets.align must equal, integer for integer, what an api.Batch of the same problems in the same
order gives (add_many_unanchored + set_post(POST_REWEIGHT, gapGamma)) once its lists are reversed and named on the host,
their scores added up and passed through similarity_score.  Same anchors, same planning, same kernels: exact.  This
isolates the quintuple stage and the glue around it.

Against the oracle: the un-named, un-reversed lists against oracle.aligned_pairs + reweight_aligned_pairs per pair, with
parity.assert_pairs_match as the other suites use it.  With gapGamma > 0 a pair whose probability sits on the emission
threshold and is listed on one side only moves the weight of every pair of its row and column by gapGamma times its own
score, far beyond the match tolerance; a pair of sequences where that happens is left out of this layer.  Only case (c)
-- 30 % / 10 % divergence, many pairs near the threshold, gapGamma 5 -- may be; the test fails if any other case is.
On an MI355X none is: all 339 pairs of the seven cases are compared."""
import functools

import numpy as np
import pytest

import set_cases as sc
from cpecan_amd import api, sets
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in sc.CASES]


def _object(case):
    s = sets.Sets(api.stateMachine5_construct(), gapGamma=case["gapGamma"])
    for set_id, seq, left, right in case["frags"]:
        s.add_fragment(set_id, seq, left, right)
    return s


@functools.lru_cache(maxsize=None)
def _aligned(name, mode=None):
    """(pairs, quints, offsets, similarity) of Sets.align on the case's own pairs (or on those of `mode`); computed once."""
    case = sc.BY_NAME[name]
    want = sc.chosen_pairs(case, mode)
    with _object(case) as s:
        if isinstance(mode or case["pairs"], str):  # the library chooses them
            pairs = [tuple(p) for p in s.pairs(sets.ALL if (mode or case["pairs"]) == "all" else sets.REFERENCE).tolist()]
            assert pairs == want
        return (want,) + s.align(want)


def _hand_made(case, pairs):
    """The same problems through a plain batch: the reweighted list 0 of every problem."""
    p = api.pairwiseAlignmentBandingParameters_construct()
    with api.Batch(api.stateMachine5_construct(), p) as b:
        b.set_post(api.POST_REWEIGHT, float(np.float32(case["gapGamma"])))
        b.add_many_unanchored(sc.problems(case, pairs))
        b.upload()
        b.run()
        b.download()
        return [b.result(i) for i in range(len(pairs))], b.stats()


def _expected(case, pairs, lists):
    quints, offsets, sim = [], [0], []
    for (a, b), t in zip(pairs, lists):
        t = t[::-1].astype(np.int64)  # convertAlignedPairsToMultipleAlignedPairs pops from the end
        quints.append(np.stack([t[:, 0], np.full(len(t), a), t[:, 1], np.full(len(t), b), t[:, 2]], axis=1))
        offsets.append(offsets[-1] + len(t))
        sim.append(api.similarity_score(int(t[:, 0].sum()), len(case["frags"][a][1]), len(case["frags"][b][1])))
    return np.concatenate(quints) if quints else np.zeros((0, 5), dtype=np.int64), offsets, sim


def _assert_equals_hand_made(case, pairs, quints, offsets, sim):
    lists, _ = _hand_made(case, pairs)
    wq, wo, ws = _expected(case, pairs, lists)
    assert quints.dtype == np.int32 and offsets.dtype == np.int64 and sim.dtype == np.int64
    assert offsets.tolist() == wo
    assert quints.shape == wq.shape and (quints.astype(np.int64) == wq).all()
    assert sim.tolist() == ws


@pytest.mark.parametrize("name", NAMES)
def test_align_equals_a_hand_made_batch(name):
    case = sc.BY_NAME[name]
    pairs, quints, offsets, sim = _aligned(name)
    assert len(pairs) == len(sim) == len(offsets) - 1
    _assert_equals_hand_made(case, pairs, quints, offsets, sim)
    if name == "b":
        assert offsets[1] > 256 and int(quints[:, 0].astype(np.int64).sum()) > 2 ** 31
    if name == "c":
        assert int(quints[:, 0].astype(np.int64).sum()) < 0 and sim.tolist() == [0]
    if name == "a":
        assert len(pairs) == 325


def test_align_matches_the_oracle():
    excluded = set()
    p = api.pairwiseAlignmentBandingParameters_construct()
    compared = 0
    for case in sc.CASES:
        pairs, quints, offsets, sim = _aligned(case["name"])
        probs = sc.problems(case, pairs)
        anchors = None
        if case["name"] == "f":  # past anchorMatrixBiggerThanThis: the oracle gets the anchors the library finds
            anchors = [api.runs_to_anchors(api.find_anchor_runs(sx, sy, expansion=p.diagonalExpansion)[0]) for sx, sy, _, _ in probs]
            assert all(len(a) > 0 for a in anchors)
        else:
            assert all(len(sx) * len(sy) <= api.ANCHOR_MATRIX_BIGGER_THAN_THIS for sx, sy, _, _ in probs)
        for k, ((a, b), (plain, rew)) in enumerate(zip(pairs, sc.oracle_lists(case, pairs, anchors))):
            q = quints[offsets[k]:offsets[k + 1]]
            assert (q[:, 1] == a).all() and (q[:, 3] == b).all()
            got = q[::-1][:, [0, 2, 4]]
            if case["gapGamma"] > 0 and {(x, y) for _, x, y in got.tolist()} != {(x, y) for _, x, y in plain.tolist()}:
                excluded.add(case["name"])  # a pair on the threshold, on one side only: every weight of its row and column moved
                continue
            # after reweighting a score says nothing about the emission threshold: the cells are the same on both sides
            # here (or gapGamma is 0 and the scores are the sweep's), so the threshold rule of the gate has nothing to excuse
            assert_pairs_match(got, rew, threshold=p.threshold)
            # the similarity is the sum over min(lX, lY), truncated: every pair may be off by the gate's max(1, 1e-5 w)
            total = int(rew[:, 0].sum())
            lX, lY = len(probs[k][0]), len(probs[k][1])
            # (and, with gapGamma 0, a pair on the threshold that one side alone lists counts in one sum only)
            g = {(x, y): s for s, x, y in got.tolist()}
            w = {(x, y): s for s, x, y in rew.tolist()}
            one_sided = sum(abs(g.get(c, w.get(c))) for c in set(g) ^ set(w))
            slack = (sum(max(1.0, 1e-5 * abs(int(v))) for v in rew[:, 0]) + one_sided) / max(1, min(lX, lY)) + 1
            assert abs(int(sim[k]) - api.similarity_score(total, lX, lY)) <= slack
            compared += 1
    print("oracle layer: %d pairs compared, cases left out: %s" % (compared, sorted(excluded) or "none"))
    assert excluded <= {"c"}, excluded
    assert compared >= 325 + 1 + 3 + 7 + 1 + 1


def test_align_again_on_the_same_object_with_the_reference_pairs():
    for name in ("e", "a"):
        case = sc.BY_NAME[name]
        want = sc.chosen_pairs(case, "reference")
        with _object(case) as s:
            first = s.align(s.pairs(sets.ALL))
            ref = [tuple(p) for p in s.pairs(sets.REFERENCE).tolist()]
            assert ref == want and len(ref) < len(first[2])
            second = s.align(ref)
            _assert_equals_hand_made(case, ref, *second)
            again = s.align(s.pairs(sets.ALL))  # and the first call's pairs give the first call's result
            assert all((x == y).all() for x, y in zip(first, again))
        full = _aligned(name)
        assert all((x == y).all() for x, y in zip(first, full[1:]))
        # every reference pair is one of the ALL pairs: its records are that pair's records
        where = {p: k for k, p in enumerate(full[0])}
        for k, pr in enumerate(ref):
            j = where[pr]
            assert (second[0][second[1][k]:second[1][k + 1]] == full[1][full[2][j]:full[2][j + 1]]).all()
            assert second[2][k] == full[3][j]


def test_a_plain_batch_is_what_it_was():
    """A batch that does not select the stage allocates and launches what it did: the same statistics and lists before
    and after the sets layer has run on the device, and the same as a batch that selects the stage and drops it again."""
    case = sc.BY_NAME["e"]
    pairs = sc.chosen_pairs(case)
    before, st0 = _hand_made(case, pairs)
    with _object(case) as s:
        s.align(pairs)
    after, st1 = _hand_made(case, pairs)
    assert all((x == y).all() for x, y in zip(before, after))
    key = lambda st: (st.problems, st.regions, st.cells, st.pairs, st.launches, st.deviceBytes, st.wavesPerLaunch, st.launchForm)
    assert key(st0) == key(st1) and st0.launches == 1 and st0.deviceBytes > 0
    p = api.pairwiseAlignmentBandingParameters_construct()
    with api.Batch(api.stateMachine5_construct(), p) as b:
        b.set_post(api.POST_REWEIGHT, case["gapGamma"])
        b.add_many_unanchored(sc.problems(case, pairs))
        names = np.array(pairs, dtype=np.int32)
        sets.batch_set_quintuples(b, names)
        b.upload()
        b.run()
        b.download()
        quints, offsets, sums = sets.batch_quintuples(b)
        with pytest.raises(api.CpecanError, match="stayed on the device"):
            b.result(0)
        assert key(b.stats())[:3] == key(st0)[:3] and b.stats().deviceBytes == st0.deviceBytes  # the stage's blocks live for its call only
        wq, wo, _ = _expected(case, pairs, before)
        assert offsets.tolist() == wo and (quints.astype(np.int64) == wq).all()
        assert sums.tolist() == [int(t[:, 0].astype(np.int64).sum()) for t in before]
        sets.batch_set_quintuples(b, None)  # off again: the next download is a plain one
        b.run()
        b.download()
        assert all((b.result(i) == before[i]).all() for i in range(len(pairs)))
        assert key(b.stats()) == key(st0)
