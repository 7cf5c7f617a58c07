"""The band-edge statistic and the adaptive band without a device: the C statement of the definition
(cpecan_band_edge_of_pairs) against tests/band_edge_model.py on the oracle's lists of every case of
tests/band_edge_cases.py, the margin the GPU tests rely on, the round every cigar of the adaptive set must end on, every
refusal that needs no device, and the two command lines' option checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_edge_cases as bc
import band_edge_model as bm
from cpecan_amd import api, realign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c.name for c in bc.all_cases()]


def _host(case, i, pairs):
    sx, sy, anchors, rl, rr = case.problems[i]
    p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
    return api.band_edge_of_pairs(anchors, len(sx), len(sy), p, pairs, rl, rr)


def test_symbols_and_mirrors():
    L = api.lib()
    for name in ("cpecan_batch_set_band_edge", "cpecan_batch_band_edge", "cpecan_band_edge_of_pairs"):
        assert hasattr(L, name) and name in api.EXPORTS
    realign._lib()
    for name in ("cpecan_realigner_set_adaptive_band", "cpecan_realigner_adaptive_rounds"):
        assert hasattr(L, name) and name in realign.EXPORTS
    assert C.sizeof(api.BandEdge) == 24
    # the library writes 24 bytes and no more: a guard word behind the record survives a call that fills every field
    buf = (C.c_int64 * 4)(-1, -1, -1, 0x5A5A5A5A5A5A5A5A)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=0)
    anchors = np.array([1, 1, 0], dtype=np.int64)
    pairs = np.array([7, 0, 0, 9, 1, 1, 5, 2, 2], dtype=np.int32)
    rc = L.cpecan_band_edge_of_pairs(anchors.ctypes.data_as(C.POINTER(C.c_int64)), 1, 3, 3, C.byref(p), 0, 0,
                                     pairs.ctypes.data_as(C.POINTER(C.c_int32)), 3, C.cast(buf, C.POINTER(api.BandEdge)))
    assert rc == 0 and buf[3] == 0x5A5A5A5A5A5A5A5A
    e = C.cast(buf, C.POINTER(api.BandEdge))[0]
    # E = 0 around the anchor (1, 1): its own diagonal holds that cell alone, cut on both sides and counted once; (0, 0)
    # and (2, 2) sit in the corners' rectangles, which the matrix cuts
    assert (e.edgePairs, e.edgeScoreSum, e.edgeScoreMax, e.reserved) == (1, 9, 9, 0)


@pytest.mark.parametrize("name", CASES)
def test_host_function_equals_the_model(name):
    case = bc.case(name)
    for i, pairs in enumerate(bc.oracle_lists(name)):
        want = bm.band_edge(case.problems[i], case.pkw, pairs)
        assert _host(case, i, pairs) == want, (name, i)
        # the order of the pairs does not matter, and neither does a pair under another's score
        assert _host(case, i, pairs[::-1]) == want, (name, i)


@pytest.mark.parametrize("name", CASES)
def test_margin_precondition(name):
    """A flag is claimed only where the oracle's lists give edgeScoreSum >= 2 S and its absence only where they give
    <= S / 2: the GPU's scores differ from the oracle's by at most one unit a pair."""
    case = bc.case(name)
    for i, pairs in enumerate(bc.oracle_lists(name)):
        got = bm.band_edge(case.problems[i], case.pkw, pairs)
        if case.expect[i] == "flag":
            assert got["edgeScoreSum"] >= 2 * bc.S and got["edgePairs"] > 0, (name, i, got)
        elif case.expect[i] == "clear":
            assert got["edgeScoreSum"] <= bc.S // 2, (name, i, got)
    assert any(e is not None for e in case.expect)


def test_cases_have_the_edges_they_were_built_for():
    # the table of the issue: expansion 4 flags every wrong pair, the right anchors leave no edge pair
    for E in (4, 8):
        case = bc.deletion_case(E)
        stats = [bm.band_edge(pr, case.pkw, l) for pr, l in zip(case.problems, bc.oracle_lists(case.name))]
        assert all(s["edgePairs"] == 0 for s in stats[1::2])
        assert all(len(l) > 300 for l in bc.oracle_lists(case.name)[0::2])  # wrong anchors: twice the pairs of the right ones
    e8 = bc.deletion_case(8)
    miss = bm.band_edge(e8.problems[10], e8.pkw, bc.oracle_lists(e8.name)[10])
    assert miss["edgePairs"] == 0 and len(bc.oracle_lists(e8.name)[10]) == 330  # seed 5: a wrong alignment the flag misses
    # several chunks per region
    chunks = bc.case("del400-chunks")
    assert len(bm.regions(chunks.problems[0], chunks.pkw)) == 1 and chunks.pkw["minDiagsBetweenTraceBack"] == 50
    # two regions, every edge pair in the second, whose origin is not (0, 0)
    two = bc.case("two-regions")
    regs = bm.regions(two.problems[0], two.pkw)
    edges = bm.edge_pairs(two.problems[0], two.pkw, bc.oracle_lists(two.name)[0])
    assert len(regs) == 2 and regs[1].x1 > 0 and regs[1].y1 > 0 and edges and {e[0] for e in edges} == {1}
    # unanchored: pairs on the band's first and last cells exist, and none of them is cut
    un = bc.case("unanchored-team")
    (reg,) = bm.regions(un.problems[0], un.pkw)
    assert all(hi - lo == 2 * min(d, 900 - d) for d, (lo, hi) in enumerate(reg.band))
    assert bm.band_edge(un.problems[0], un.pkw, bc.oracle_lists(un.name)[0])["edgePairs"] == 0
    # per-anchor expansions really differ
    dyn = bc.case("dynamic")
    assert dyn.pkw["dynamicAnchorExpansion"] == 1 and {a[2] for a in dyn.problems[0][2]} == {2, 6}
    assert bc.case("minus").minus and bc.case("indel").emit == bc.EMIT_INDEL


def test_both_sides_count_once_and_matrix_edges_do_not_count():
    """A width-1 diagonal inside the matrix is left- and right-cut at once; the corner cells are cut by the matrix."""
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=0)
    anchors = [(i, i, 0) for i in range(1, 5)]
    pairs = [(100 + i, i, i) for i in range(6)]
    problem = ("A" * 6, "A" * 6, tuple(anchors), False, False)
    want = bm.band_edge(problem, dict(diagonalExpansion=0), pairs)
    assert want == {"edgePairs": 4, "edgeScoreSum": 101 + 102 + 103 + 104, "edgeScoreMax": 104}
    assert api.band_edge_of_pairs(anchors, 6, 6, p, pairs) == want


def test_predicted_rounds_of_the_adaptive_set():
    """The misplaced deletions clear their flag after two doublings, the controls never raise it -- each step with the
    margin, and the host function agrees with the model at every expansion."""
    stats, rounds = bc.adaptive_statistics(), bc.adaptive_predictions()
    inputs = bc.adaptive_inputs()
    assert len(inputs) == 8 and sum(m for *_, m in inputs) == 5
    assert rounds == [2 if misplaced else 0 for *_, misplaced in inputs]
    for row, k in zip(stats, rounds):
        assert all(s["edgeScoreSum"] >= 2 * bc.S for s in row[:k]) and row[k]["edgeScoreSum"] <= bc.S // 2, row
    from cpecan_amd.api import band_edge_of_pairs
    import oracle_binding as ob
    om = ob.model(0)
    for (_, x, _, y, _, misplaced), row in zip(inputs, stats):
        for k, want in enumerate(row):
            E = bc.ADAPTIVE_E << k
            pr, pkw = bc.adaptive_problem(x, y, misplaced, E), bc.adaptive_pkw(E)
            pairs = ob.aligned_pairs(om, x, y, pr[2], ob.params(**pkw), True, True)
            assert band_edge_of_pairs(pr[2], len(x), len(y), api.pairwiseAlignmentBandingParameters_construct(**pkw), pairs, True, True) == want


def test_predicted_rounds_of_the_align_pairs():
    """cpecan_align's pairs (anchors of tests/anchor_model.py): the detour is flagged at expansion 2 and clear at 4, the
    plain query is never flagged -- each with the margin."""
    detour, plain = bc.align_statistics()
    assert detour[0]["edgeScoreSum"] >= 2 * bc.S and detour[1]["edgeScoreSum"] <= bc.S // 2
    assert plain[0]["edgeScoreSum"] <= bc.S // 2


def test_refusals_without_a_device():
    sm = api.stateMachine5_construct()
    for emit in (api.EMIT_EXPECT, api.EMIT_FORWARD):
        with api.Batch(sm, emit=emit) as b:
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                b.set_band_edge(True)
    with api.Batch(sm) as b:
        b.set_band_edge(True)
        b.set_band_edge(False)
        b.set_band_edge(True)
        b.add("ACGT", "ACGT")
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):  # nothing has been downloaded
            b.band_edge(0)
    with api.Batch(sm, emit=api.EMIT_INDEL) as b:
        b.set_band_edge(True)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=4, splitMatrixBiggerThanThis=100)
    L = api.lib()
    e = api.BandEdge()
    one = np.array([5, 0, 0], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.cpecan_band_edge_of_pairs(None, 0, 4, 4, None, 0, 0, one, 1, C.byref(e)) == -1      # no parameters
    assert L.cpecan_band_edge_of_pairs(None, 0, 4, 4, C.byref(p), 0, 0, one, 1, None) == -1      # no output
    assert L.cpecan_band_edge_of_pairs(None, 0, 4, 4, C.byref(p), 0, 0, None, 1, C.byref(e)) == -1  # pairs promised, none given
    assert L.cpecan_band_edge_of_pairs(None, 1, 4, 4, C.byref(p), 0, 0, one, 1, C.byref(e)) == -1   # anchors promised, none given
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # a pair outside the matrix
        api.band_edge_of_pairs((), 4, 4, p, [(5, 4, 0)])
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # a pair between two regions
        api.band_edge_of_pairs([(1, 1, 4), (58, 58, 4)], 60, 60, p, [(5, 30, 30)])
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # anchors that do not increase
        api.band_edge_of_pairs([(3, 3, 4), (2, 5, 4)], 10, 10, p, [(5, 1, 1)])
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # an odd expansion
        api.band_edge_of_pairs((), 4, 4, api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=3), [(5, 1, 1)])


def test_adaptive_band_refusals_without_a_device():
    with realign.Realigner() as r:
        for rounds, score in ((-1, bc.S), (5, bc.S), (1, 0), (4, -3)):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                r.set_adaptive_band(rounds, score)
        r.set_adaptive_band(0)
        r.set_adaptive_band(0, 0)
        for rounds in (1, 2, 3, 4):
            r.set_adaptive_band(rounds, 1)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):  # no realign call yet
            r.adaptive_rounds()
    with realign.Realigner(options=realign.realign_options(rescoreOriginalAlignment=1)) as r:
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            r.set_adaptive_band(2, bc.S)
        r.set_adaptive_band(0)


@pytest.mark.parametrize("binary", ["cpecan_realign", "cpecan_align"])
def test_binaries_refuse_one_option_without_the_other(binary, tmp_path):
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nACGT\n")
    exe = os.path.join(ROOT, "cpecan_amd", binary)
    files = [str(fa)] * (2 if binary == "cpecan_align" else 1)
    for opts in (["--adaptiveBand", "2"], ["--minEdgeScore", "1000000"]):
        done = subprocess.run([exe] + opts + files, stdin=subprocess.DEVNULL, capture_output=True, text=True)
        assert done.returncode == 1 and "need each other" in done.stderr, (opts, done.stderr)
    for opts in (["--adaptiveBand", "0", "--minEdgeScore", "5"], ["--adaptiveBand", "5", "--minEdgeScore", "5"],
                 ["--adaptiveBand", "2", "--minEdgeScore", "0"]):
        done = subprocess.run([exe] + opts + files, stdin=subprocess.DEVNULL, capture_output=True, text=True)
        assert done.returncode == 1 and done.stdout == "", (opts, done.stderr)
