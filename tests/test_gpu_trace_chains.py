"""Chains: an item of the traceback launch that sweeps a region's later segments forward -- from the two diagonals the
region's ring holds at a segment top -- and then traces them back (cpk_sweep.inl "CHAIN"; CPECAN_CHAIN=k forces chains from
segment k wherever both launches of a class are gangs, 0 forbids them).  A chain changes which wave runs the forward sweep
of a segment and nothing else: every case compares what CPECAN_CHAIN=k gives with what CPECAN_CHAIN=0 gives for equality
of bits -- the result list of every problem and the sweeps' debug buffers of problem 0 -- and problem 0 against the oracle,
and reads off the class lines that the chains really ran.  The shapes are those of tests/test_gpu_gang.py."""
import re

import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
import table_model as tm
from cpecan_amd import api
from cpecan_amd.workload import make_pair
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)  # a traceback every 42 diagonals of a narrow band
BASE_ENV = {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1", "CPECAN_TRACE_HOST": "1"}


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


def _problem(p):
    return tuple(p) + (False, False) if len(p) == 3 else tuple(p)


def _chain_words(err):
    """[(K, chains)] of the class lines CPECAN_TRACE_HOST wrote; (0, 0) for a class without chains."""
    out = []
    for line in re.findall(r"^cpecan class \d+:.*$", err, re.M):
        m = re.search(r"chains from segment (\d+): (\d+)", line)
        out.append((int(m.group(1)), int(m.group(2))) if m else (0, 0))
    return out


def _run(monkeypatch, capfd, k, gang, mtype, problems, pkw, cells):
    """(lists, (fb, totals) of problem 0, segments per problem) under CPECAN_CHAIN=k; asserts the chains the plan reports."""
    for name, v in BASE_ENV.items():
        monkeypatch.setenv(name, v)
    monkeypatch.setenv("CPECAN_GANG", str(gang))
    monkeypatch.setenv("CPECAN_CHAIN", str(k))
    capfd.readouterr()
    with api.Batch(_sm(mtype), api.pairwiseAlignmentBandingParameters_construct(**pkw), debug=True) as b:
        for p in problems:
            b.add(*_problem(p))
        b.upload()
        words = _chain_words(capfd.readouterr().err)
        n_seg = [b.table(i)["nSeg"] for i in range(len(problems))]
        b.run()
        b.download()
        out = [b.result(i) for i in range(len(problems))]
        dbg = b.debug_fetch(0, *cells)
    assert words, "no class line"
    want = sum(1 for n in n_seg if n > k) if k else 0
    assert sum(n for _, n in words) == want, (k, words, n_seg)
    assert all(kk == k for kk, n in words if n), (k, words)
    return out, dbg, n_seg


def _check(monkeypatch, capfd, mtype, problems, pkw, ks, gang=3, expect_chains=True):
    """CPECAN_CHAIN=k for every k of ks(segments per problem) against CPECAN_CHAIN=0; problem 0 against the oracle."""
    sx, sy, a, rl, rr = _problem(problems[0])
    want0, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), rl, rr)
    cells = (tr["n_cells"], tr["n_diagonals"])
    want, (fb0, tot0), n_seg = _run(monkeypatch, capfd, 0, gang, mtype, problems, pkw, cells)
    assert any(len(w) for w in want), "nothing was emitted: the case compares empty lists"
    assert np.isfinite(fb0).any() and np.isfinite(tot0).any()
    ks = ks(n_seg) if callable(ks) else ks
    assert not expect_chains or any(n > k for k in ks for n in n_seg), "no k of the case forms a chain"
    for k in ks:
        got, (fb, tot), _ = _run(monkeypatch, capfd, k, gang, mtype, problems, pkw, cells)
        assert len(got) == len(want)
        for i, (x, y) in enumerate(zip(got, want)):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), "chains from %d: problem %d differs" % (k, i)
        assert fb.tobytes() == fb0.tobytes() and tot.tobytes() == tot0.tobytes(), "chains from %d: debug buffers differ" % k
    assert_pairs_match(got[0], want0, threshold=ob.params(**pkw).threshold)


# ---- 1: chains from segment 1, 2, from the last segment, and from behind it (no chain forms); both state counts ----
@pytest.mark.parametrize("gang,mtype", [(2, 0), (3, 2), (11, 0)])
def test_first_second_last_segment_and_none(gang, mtype, monkeypatch, capfd):
    problems = [make_pair(3, i, 150 + 50 * i, 20) for i in range(4)]  # 150 to 300 bases
    _check(monkeypatch, capfd, mtype, problems, dict(diagonalExpansion=20, **SHORT), lambda n: (1, 2, max(n) - 1, max(n)), gang)


def test_behind_the_last_segment_no_chain_forms(monkeypatch, capfd):
    problems = [make_pair(3, i, 200, 20) for i in range(2)]
    _check(monkeypatch, capfd, 0, problems, dict(diagonalExpansion=20, **SHORT), lambda n: (max(n), max(n) + 5), expect_chains=False)


# ---- 2: regions of 1, 2, 3 and many segments in one class ----
def test_one_two_three_and_many_segments_in_one_class(monkeypatch, capfd):
    problems = [make_pair(31, i, length, 10) for i, length in enumerate((320, 20, 45, 70, 22, 48, 75, 260, 330))]

    def ks(n_seg):
        assert {1, 2, 3} <= set(n_seg) and max(n_seg) >= 8, n_seg
        return (1, 2, 3)
    _check(monkeypatch, capfd, 0, problems, dict(diagonalExpansion=10, **SHORT), ks)


# ---- 3: fewer items than waves; about 200 regions -- with chains from segment 16 more items than the 2816 waves ----
def test_fewer_items_than_waves(monkeypatch, capfd):
    problems = [make_pair(3, i, 400, 10) for i in range(2)]
    _check(monkeypatch, capfd, 0, problems, dict(diagonalExpansion=10, **SHORT), (1, 3), gang=11)


def test_two_hundred_regions(monkeypatch, capfd):
    problems = [make_pair(11, i, 400, 20) for i in range(200)]
    _check(monkeypatch, capfd, 0, problems, dict(diagonalExpansion=20, **SHORT), (1, 16), gang=11)


# ---- 4: resume diagonals of 63, 64, 65, 128 and 129 cells ----
def _resume_width_case(width):
    """Unanchored pairs whose 61 (76) widest diagonals in a row have `width` cells; under an expansion of 130 every diagonal
    may be a traceback point, so a segment top and the diagonal below it lie among them.  Returns the problems, the
    parameters and the segments k whose chains resume from two diagonals of `width` cells."""
    m = width - 1
    problems = [(tc.seq(m, 1), tc.seq(m + 60, 2), ()), (tc.seq(m + 75, 3), tc.seq(m, 4), ())]
    pkw = dict(threshold=0.01, diagonalExpansion=130, **SHORT)
    ks = set()
    for p in problems:
        (rg,) = tm.problem_regions(_problem(p), pkw)
        ks |= {si + 1 for si, (_, top, _) in enumerate(rg.segs[:-1]) if rg.width[top] == width and rg.width[top - 1] == width}
    assert ks, "no resume point on the widest diagonals"
    return problems, pkw, tuple(sorted(ks))


@pytest.mark.parametrize("width,mtype", [(63, 0), (64, 2), (65, 0), (128, 2), (129, 0)])
def test_resume_diagonals_around_the_groups(width, mtype, monkeypatch, capfd):
    problems, pkw, ks = _resume_width_case(width)
    _check(monkeypatch, capfd, mtype, problems, pkw, ks)


# ---- 5: a band that turns back: the base moves in front of dTop (k = 1, 4: problem 0) and of dTop + 1 (k = 2: problem 1)
# of a resume point -- tests/test_trace_chains_plan_cpu.py asserts that of the shapes ----
def test_band_that_turns_back(monkeypatch, capfd):
    case = tc.chain_case()
    _check(monkeypatch, capfd, case.mtype, list(case.problems), case.pkw, (1, 2, 4))


# ---- 6: ragged left and right ends ----
@pytest.mark.parametrize("mtype", [0, 2])
def test_ragged_ends(mtype, monkeypatch, capfd):
    pairs = [make_pair(5, i, 250, 20) for i in range(3)]
    problems = [pairs[0] + (True, True), pairs[1] + (True, False), pairs[2] + (False, True)]
    _check(monkeypatch, capfd, mtype, problems, dict(diagonalExpansion=20, **SHORT), lambda n: (1, min(n) - 1))


# ---- 8: threshold 0: every cell is a candidate, more than the stage holds ----
def test_threshold_zero(monkeypatch, capfd):
    problems = [(tc.seq(64, 11), tc.seq(64, 12), ()), (tc.seq(90, 13), tc.seq(80, 14), ())]
    _check(monkeypatch, capfd, 0, problems, dict(threshold=0.0, diagonalExpansion=130, **SHORT), (1, 2))


# ---- 9: a second batch alive beside the first: one with chains, one without ----
def test_a_batch_with_chains_beside_one_without(monkeypatch, capfd):
    pa = [make_pair(21, i, 400, 20) for i in range(12)]
    pb = [make_pair(22, i, 300, 10) for i in range(9)]
    pkw_a, pkw_b = dict(diagonalExpansion=20, **SHORT), dict(diagonalExpansion=10, **SHORT)
    want = []
    for mtype, probs, pkw in ((0, pa, pkw_a), (2, pb, pkw_b)):
        sx, sy, a, rl, rr = _problem(probs[0])
        _, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), rl, rr)
        want.append(_run(monkeypatch, capfd, 0, 11, mtype, probs, pkw, (tr["n_cells"], tr["n_diagonals"]))[0])
    with api.Batch(_sm(0), api.pairwiseAlignmentBandingParameters_construct(**pkw_a)) as a, \
            api.Batch(_sm(2), api.pairwiseAlignmentBandingParameters_construct(**pkw_b)) as b:
        for p in pa:
            a.add(*p)
        for p in pb:
            b.add(*p)
        capfd.readouterr()
        monkeypatch.setenv("CPECAN_CHAIN", "2")  # (the plan reads the environment at upload)
        a.upload()
        assert _chain_words(capfd.readouterr().err) == [(2, len(pa))]
        monkeypatch.setenv("CPECAN_CHAIN", "0")
        b.upload()
        assert _chain_words(capfd.readouterr().err) == [(0, 0)]
        for _ in range(2):  # both in flight, twice: the second round runs over the scratch and the rings of the first
            a.run()
            b.run()
            a.download()
            b.download()
            for batch, probs, w in ((a, pa, want[0]), (b, pb, want[1])):
                for i in range(len(probs)):
                    assert np.array_equal(batch.result(i), w[i]), "problem %d differs" % i
