"""Strand without a GPU: the host reverse complement against the model's, the strand rule of DESIGN.md section 7 step 0
on the model (tests/strand_model.py), minus-strand cigars through the realigner's parser and check, and the argument
errors of the new entry points and of cpecan_align --strand."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import reference_cases as rc
import strand_model as sm
from cpecan_amd import api, realign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reverse_complement_in_place(s):
    buf = C.create_string_buffer(bytes(s), len(s))
    assert api.lib().cpecan_reverse_complement(buf, len(s), buf) == 0
    return buf.raw


def test_reverse_complement_equals_the_model_in_place_and_out_of_place():
    rng = random.Random(11)
    alphabet = b"ACGTacgtNnRYKMSWBDHVrykm-*\x00\xff"
    cases = [b"", b"A", b"n", b"AC", b"ACG", b"acgtN", bytes(range(256))]
    cases += [bytes(rng.choice(alphabet) for _ in range(n)) for n in (2, 3, 17, 64, 1001)]
    for s in cases:
        want = sm.rc(s)
        assert api.reverse_complement(s) == want, s
        assert _reverse_complement_in_place(s) == want, s
        assert api.reverse_complement(api.reverse_complement(s)) == s
        assert sm.rc(sm.rc(s)) == s
    assert sm.rc(b"AAcgTNx") == b"xNAcgTT"                          # case survives, other bytes stay
    assert api.lib().cpecan_reverse_complement(None, 3, None) == -1
    assert api.lib().cpecan_reverse_complement(None, 0, None) == 0
    assert C.sizeof(api.StrandResult) == 16


# chain score of (X, Y) and of (X, rc(Y)) with the default parameters, from the model
TABLE = [
    ("random 400", lambda: ac.random_pair(1, 400), 23186, 0),
    ("random 2000", lambda: ac.random_pair(2, 2000), 113751, 0),
    ("random 6000", lambda: ac.random_pair(3, 6000), 327665, 0),
    ("masked 3000", lambda: ac.masked_pair(4, 3000), 128870, 0),
    ("insertion", lambda: ac.insertion_pair(), 254356, 876),
    ("dog", lambda: rc.encode_human_other("dog")[:2], 724288, 23125),
    ("mouse", lambda: rc.encode_human_other("mouse")[:2], 126851, 19316),
]


@pytest.mark.parametrize("case", TABLE, ids=[t[0] for t in TABLE])
def test_the_model_picks_the_strand(case):
    _, make, plus, minus = case
    sx, sy = make()
    assert (sm.strand_score(sx, sy), sm.strand_score(sx, sm.rc(sy))) == (plus, minus)
    limit = 0 if len(sx) * len(sy) <= 500 * 500 else 500 * 500      # the 400-base pair is searched too
    runs, st, res = sm.find_anchor_runs_stranded(sx, sy, "both", anchorMatrixBiggerThanThis=limit)
    assert res == dict(strand="plus", scorePlus=plus, scoreMinus=minus) and plus > 0
    want, wst = am.find_anchor_runs(sx, sy, anchorMatrixBiggerThanThis=limit)
    assert np.array_equal(runs, want) and st == wst
    # the query given on the other strand: the scores swap exactly and the runs are those of the forward pair
    runs, st, res = sm.find_anchor_runs_stranded(sx, sm.rc(sy), "both", anchorMatrixBiggerThanThis=limit)
    assert res == dict(strand="minus", scorePlus=minus, scoreMinus=plus)
    assert np.array_equal(runs, want) and st == wst and len(runs) > 0
    # forced: nothing extra is scored
    runs, st, res = sm.find_anchor_runs_stranded(sx, sm.rc(sy), "minus", anchorMatrixBiggerThanThis=limit)
    assert res == dict(strand="minus", scorePlus=-1, scoreMinus=plus) and np.array_equal(runs, want)
    runs, st, res = sm.find_anchor_runs_stranded(sx, sy, "plus", anchorMatrixBiggerThanThis=limit)
    assert res == dict(strand="plus", scorePlus=plus, scoreMinus=-1) and np.array_equal(runs, want)


def test_a_tie_is_plus():
    sx, sy = ac.random_pair(61, 300)[0], ac.random_pair(62, 300)[1]   # unrelated
    runs, st, res = sm.find_anchor_runs_stranded(sx, sy, "both")
    assert res == dict(strand="plus", scorePlus=0, scoreMinus=0) and len(runs) == 0
    assert sm.find_anchor_runs_stranded(b"", b"ACGT", "both")[2] == dict(strand="plus", scorePlus=0, scoreMinus=0)


def test_a_pair_under_the_size_limit_is_scored_but_gets_no_runs():
    sx, sy = ac.random_pair(1, 400)
    assert len(sx) * len(sy) <= 500 * 500
    runs, st, res = sm.find_anchor_runs_stranded(sx, sm.rc(sy), "both")
    assert res["strand"] == "minus" and res["scoreMinus"] > res["scorePlus"] == 0
    assert len(runs) == 0 and st["runs"] == 0 and st["hits"] == 0
    # forced modes compute nothing for it
    assert sm.find_anchor_runs_stranded(sx, sy, "plus")[2] == dict(strand="plus", scorePlus=-1, scoreMinus=-1)
    assert sm.find_anchor_runs_stranded(sx, sy, "minus")[2] == dict(strand="minus", scorePlus=-1, scoreMinus=-1)


def _cigar_stranded(c1, c2, l1, l2, strand2, xy):
    return realign.Cigar.from_aligned_pairs(c1, c2, 0.0, l1, l2, xy, strand2=bool(strand2))


def test_a_minus_cigar_formats_parses_and_passes_the_cigar_check():
    xy = [(2, 1), (3, 2), (4, 3), (7, 5), (8, 6)]
    plus = _cigar_stranded("target", "query", 12, 9, 1, xy)
    assert plus == realign.Cigar.from_aligned_pairs("target", "query", 0.0, 12, 9, xy) and plus.strand2 is True
    assert realign._lib().cpecan_cigar_from_aligned_pairs_stranded(b"t", b"q", 0.0, 12, 9, 0, None, 1, None) == -1
    minus = _cigar_stranded("target", "query", 12, 9, 0, xy)
    assert (minus.start2, minus.end2, minus.strand2) == (9, 0, False)
    assert (minus.start1, minus.end1, minus.strand1) == (0, 12, True)
    assert minus.ops == plus.ops                                      # the operations in the order of the pairs
    text = minus.format()
    assert text.startswith("cigar: query 9 0 - target 0 12 + ")
    assert realign.Cigar.parse(text) == minus                         # cpecan_cigar_parse runs checkPairwiseAlignment
    pieces = minus.split(10 ** 6)                                     # so does cpecan_cigar_split, the realigner's check
    assert len(pieces) == 1 and pieces[0].strand2 is False and pieces[0].start2 > pieces[0].end2
    with pytest.raises(api.CpecanError):                              # the check does refuse a minus cigar that does not add up
        realign.Cigar("target", 0, 12, True, "query", 8, 0, False, 0.0, minus.ops).split(10 ** 6)


def test_the_new_entry_points_need_a_device_and_refuse_a_bad_strand_mode():
    sx, sy = ac.random_pair(1, 800)
    for mode in (-1, 3, 7):
        with pytest.raises(api.CpecanError) as e:
            api.find_anchor_runs_many_stranded([(sx, sy)], strand=mode)
        assert "(-1)" in str(e.value)
    if api.device_count() > 0:
        return  # with a GPU the calls succeed: tests/test_gpu_strand.py
    smach = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    calls = [lambda m=m: api.find_anchor_runs_many_stranded([(sx, sy)], strand=m) for m in ("plus", "minus", "both", 0, 1, 2)]
    calls += [lambda: api.find_anchor_runs(sx, sy, strand="both"), lambda: api.find_anchor_runs_many([(sx, sy)], strand="minus"),
              lambda: api.getAlignedPairsStranded(smach, sx, sy, p)]
    for call in calls:
        with pytest.raises(api.CpecanError) as e:
            call()
        assert "(-2)" in str(e.value)


def test_batch_add_many_runs_stranded_keeps_the_flag():
    """Adding needs no device: the flag is read back, and the arguments are checked as cpecan_batch_add_many_runs does."""
    smach = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    L = api.lib()
    h = C.c_void_p()
    assert L.cpecan_batch_create(C.byref(h), C.byref(smach), C.byref(p), 0, 0) == 0
    try:
        arr, n, _keep = api.Batch.prepare_problems_runs([(b"ACGTACGTAA", b"ACGTTCGTAA", [(1, 1, 0)]), (b"ACGT", b"ACGA", ())] * 2)
        flags = (C.c_int32 * 4)(0, 1, 1, 0)
        assert L.cpecan_batch_add_many_runs_stranded(h, arr, flags, n) == 0
        assert L.cpecan_batch_add_many_runs_stranded(h, arr, None, n) == 4
        assert [L.cpecan_batch_problem_strand(h, i) for i in range(8)] == [0, 1, 1, 0, 0, 0, 0, 0]
        assert L.cpecan_batch_problem_strand(h, 8) == -1 and L.cpecan_batch_problem_strand(h, -1) == -1
    finally:
        L.cpecan_batch_destroy(h)


def test_cpecan_align_refuses_an_unknown_strand():
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    for args in (["--strand", "sideways", "a.fa", "b.fa"], ["-s", "", "a.fa", "b.fa"]):
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 1 and "target.fa query.fa" in r.stderr and "--strand plus|minus|both" in r.stderr
        assert r.stdout == ""
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--strand" in r.stderr
