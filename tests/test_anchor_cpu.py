"""The anchor finder without a GPU: hand-worked cases for every step of its definition (tests/anchor_model.py), the
model's anchors on random and ENCODE inputs, the parameter struct through the ABI, and the command line's argument errors."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import reference_cases as rc
from cpecan_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = np.array(am.default_params()["scores"], dtype=np.int64)


def _codes(s):
    return am._CODE[np.frombuffer(s.encode(), dtype=np.uint8)]


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def test_a_hit_is_a_pair_of_windows_with_equal_words_at_the_seed_positions():
    seed = "1101"
    #         0123456789
    sx = "TTACGATT"
    sy = "CACTACC"          # window 1 = ACTA: A C . A equals ACGA at X window 2 on the 1 positions; no other word is shared
    assert am.seed_hits(sx, sy, seed, 1, False) == {(2, 1)}
    # a word that occurs twice in X seeds nothing with maxSeedOccurrences 1, and both windows with 2
    sx2 = sx + "ACGA"
    assert am.seed_hits(sx2, sy, seed, 1, False) == set()
    assert am.seed_hits(sx2, sy, seed, 2, False) == {(2, 1), (8, 1)}
    # N at a 1 position skips the window, N at a 0 position does not
    assert am.seed_hits("TTACNATT", sy, seed, 1, False) == {(2, 1)}
    assert am.seed_hits("TTANGATT", sy, seed, 1, False) == set()
    # lower case only matters with softMask, and only at 1 positions
    assert am.seed_hits("TTaCGATT", sy, seed, 1, False) == {(2, 1)}
    assert am.seed_hits("TTaCGATT", sy, seed, 1, True) == set()
    assert am.seed_hits("TTACgATT", sy, seed, 1, True) == {(2, 1)}


def test_extension_stops_on_xdrop_and_takes_the_shortest_prefix():
    # right of a 4-base window: 3 matches (A: +91 each), 2 mismatches A/T (-123 each), 4 matches
    x = "CCCC" + "AAA" + "AA" + "AAAA"
    y = "CCCC" + "AAA" + "TT" + "AAAA"
    cx, cy = _codes(x), _codes(y)
    s0 = 400
    # xDrop 300: after the two mismatches the sum is 273 - 246 = 27, not more than 300 under the best (273): the walk goes on
    assert am.extend_hit(cx, cy, 0, 0, 4, SCORE, 300) == (0, 0, 13, s0 + 3 * 91 - 2 * 123 + 4 * 91)
    # xDrop 200: 273 - 246 = 27 < 273 - 200: stop; the HSP ends after the three matches
    assert am.extend_hit(cx, cy, 0, 0, 4, SCORE, 200) == (0, 0, 7, s0 + 273)
    # a tie: A/G (-31) then G/A... build +91, -91 is impossible with HOXD70, so tie through the matrix: C/C 100, then
    # two columns summing to 0 cannot be made either; use a custom matrix: match +1, mismatch -1
    score = np.where(np.eye(5, dtype=bool), 1, -1).astype(np.int64)
    x = "CCCC" + "A" + "AT" + "G"      # +1, then -1 +1 -> the sum is back at 1 after three columns: the shortest prefix (1) wins
    y = "CCCC" + "A" + "TT" + "C"
    assert am.extend_hit(_codes(x), _codes(y), 0, 0, 4, score, 10) == (0, 0, 5, 4 + 1)
    # nothing positive on either side: the window alone; to the left the walk stops at the start of a sequence
    assert am.extend_hit(_codes("TCCCCA"), _codes("ACCCCT"), 1, 1, 4, score, 10) == (1, 1, 4, 4)
    assert am.extend_hit(_codes("GACCCC"), _codes("ACCCC"), 2, 1, 4, score, 10) == (1, 0, 5, 5)


def test_duplicates_collapse_and_the_threshold_holds():
    rng = random.Random(5)
    core = _rand(rng, 60)
    sx, sy = _rand(rng, 40) + core + _rand(rng, 40), _rand(rng, 30) + core + _rand(rng, 50)
    p = am.default_params(seed="111111", hspThreshold=3000)
    runs, counts = am.anchors_once(sx, sy, 0, False, p)
    # every window of the core is a hit (unless its word repeats), all of them extend to the same HSP
    assert counts["hits"] > 20 and counts["hsps"] == 1 and counts["chained"] == 1
    (x, y, n), = runs
    assert x <= 40 and y == x - 10 and x + n >= 100
    assert am.anchors_once(sx, sy, 0, False, am.default_params(seed="111111", hspThreshold=10 ** 6))[0] == []


def test_chain_tie_breaks():
    # (x, y, length, score), sorted by (x, y, length)
    hsps = [(0, 0, 10, 100), (0, 20, 10, 100), (30, 40, 10, 50), (35, 0, 5, 50), (50, 60, 10, 70)]
    # 2 can follow 0 or 1 (equal best 100): the smallest j, 0.  3 can follow 0 only (y).  4 follows 2 (150) rather than 0 / 1.
    assert am.chain(hsps) == [0, 2, 4]
    # two chains with the same total: the one that ends at the smallest i
    assert am.chain([(0, 0, 10, 100), (5, 50, 10, 100)]) == [0]
    # overlap in one coordinate is not allowed, touching is
    assert am.chain([(0, 0, 10, 100), (9, 20, 10, 100)]) == [0]
    assert am.chain([(0, 0, 10, 100), (10, 10, 10, 100)]) == [0, 1]
    assert am.chain([]) == []


def test_trim_can_empty_a_run_and_the_cap_sets_its_flag():
    rng = random.Random(6)
    a, b = _rand(rng, 30), _rand(rng, 90)
    sx = a + _rand(rng, 50) + b
    sy = a + _rand(rng, 70) + b
    p = am.default_params(seed="111111", hspThreshold=2000)
    runs, counts = am.anchors_once(sx, sy, 14, False, p)
    assert counts["chained"] == 2
    assert len(runs) == 2 and runs[0][2] <= 30 - 28 + 12
    runs, counts = am.anchors_once(sx, sy, 20, False, p)       # 2 * 20 columns and more: the short HSP leaves nothing
    assert counts["chained"] == 2 and len(runs) == 1 and runs[0][0] >= 80
    runs, counts = am.anchors_once(sx, sy, 14, False, am.default_params(seed="111111", hspThreshold=2000, maxHsps=1))
    assert counts["capped"] == 1 and counts["hsps"] == 2 and counts["chained"] == 1 and runs[0][2] > 50   # the better one


def test_one_recursion_with_the_mask_switched_off():
    rng = random.Random(7)
    a, m, b = _rand(rng, 700), _rand(rng, 600), _rand(rng, 700)
    sx = a + m.lower() + b
    sy = a + _rand(rng, 40) + m.lower() + _rand(rng, 40) + b     # the three parts lie on three diagonals
    p = am.default_params()
    top, _ = am.anchors_once(sx, sy, 14, True, p)
    assert len(top) == 2 and top[0][0] + top[0][2] <= 700 + 14 and top[1][0] >= 1300   # the masked middle seeds nothing
    # gap between the two runs: about 630 x 710 > 500 x 500.  With the mask still on nothing is found in it ...
    runs, st = am.find_anchor_runs(sx, sy, repeatMaskMatrixBiggerThanThis=500 * 500)
    assert st["subProblems"] == 1 and st["largestGap"] == st["largestGapTop"] > 500 * 500
    # ... with the mask off (the gap is under repeatMaskMatrixBiggerThanThis) the middle is anchored
    runs2, st2 = am.find_anchor_runs(sx, sy, repeatMaskMatrixBiggerThanThis=10 ** 6)
    assert st2["subProblems"] == 1 and st2["runs"] == st["runs"] + 1 and st2["largestGap"] < 500 * 500
    assert st2["anchorColumns"] > st["anchorColumns"] + 500
    # up to the size limit: nothing
    assert am.find_anchor_runs(sx[:400], sy[:400])[1]["runs"] == 0


def _strictly_increasing(runs, lX, lY):
    pX = pY = 0
    for x, y, n, e in runs.tolist():
        assert x >= pX and y >= pY and n > 0
        pX, pY = x + n, y + n
    assert pX <= lX and pY <= lY


@pytest.mark.parametrize("length", [600, 3000, 8000])
def test_model_anchors_increase_on_random_inputs(length):
    for maker in (ac.random_pair, ac.masked_pair):
        sx, sy = maker(length, length)
        runs, st = am.find_anchor_runs(sx, sy)
        assert st["runs"] == len(runs) > 0 and st["capped"] == 0
        _strictly_increasing(runs, len(sx), len(sy))
        # the pairs differ by point changes only: an anchor is never further from the main diagonal than the indels allow
        assert all(abs(x - y) <= 0.06 * length + 20 for x, y, _, _ in runs.tolist())


@pytest.mark.parametrize("name", ["dog", "mouse", "chimp"])
def test_model_anchors_on_the_encode_pairs(name):
    sx, sy, _, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
    runs, st = am.find_anchor_runs(sx, sy)
    _strictly_increasing(runs, len(sx), len(sy))
    assert st["subProblems"] > 0 and st["capped"] == 0 and 2 * st["hsps"] <= am.default_params()["maxHsps"]
    anchors = am.runs_to_anchors(runs)
    on = sum((x, y) in true_pairs for x, y, _ in anchors)
    assert len(anchors) == st["anchorColumns"] > 1000
    assert on >= 0.98 * len(anchors), (on, len(anchors))     # measured: 0.999 / 0.981 / 0.994 (profiles/anchor_quality.txt)


def test_parameter_defaults_and_struct_sizes_through_the_abi():
    assert C.sizeof(api.AnchorParams) == 152 and C.sizeof(api.AnchorProblem) == 32 and C.sizeof(api.AnchorStats) == 80
    q = api.anchor_params_default()
    want = am.default_params()
    assert q.seed == want["seed"].encode() and q.maxSeedOccurrences == 1
    assert list(q.scores) == [v for row in want["scores"] for v in row]
    assert (q.xDrop, q.hspThreshold, q.maxHsps) == (910, 800, 4096)
    assert list(q.scores)[0 * 5 + 0] == 91 and list(q.scores)[1 * 5 + 2] == -125 and list(q.scores)[4 * 5 + 4] == -100
    assert api.lib().cpecan_anchor_params_default(None) == -1
    assert api.anchor_params_default(seed="1111", maxHsps=7).maxHsps == 7
    a = api.runs_to_anchors(np.array([[3, 5, 2, 20], [9, 9, 1, 20]]))
    assert a.tolist() == [[3, 5, 20], [4, 6, 20], [9, 9, 20]]


def test_find_anchor_runs_needs_a_device():
    if api.device_count() > 0:
        return  # with a GPU the calls succeed: tests/test_gpu_anchor.py
    sx, sy = ac.random_pair(1, 800)
    for call in (lambda: api.find_anchor_runs_many([(sx, sy)]), lambda: api.find_anchor_runs(sx, sy),
                 lambda: api.find_anchor_runs_once(sx, sy)):
        with pytest.raises(api.CpecanError) as e:
            call()
        assert "(-2)" in str(e.value)
    # bad arguments are refused before the device is looked for
    with pytest.raises(api.CpecanError) as e:
        api.find_anchor_runs(sx, sy, trim=-1)
    assert "(-1)" in str(e.value)


def test_cpecan_align_usage_and_argument_errors(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    assert os.path.exists(exe), "build() makes cpecan_align"
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "target.fa query.fa" in r.stderr and r.stdout == ""
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "target.fa query.fa" in r.stderr
    r = subprocess.run([exe, "only_one.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1
    r = subprocess.run([exe, str(tmp_path / "missing.fa"), str(tmp_path / "missing2.fa")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "cannot read" in r.stderr
    r = subprocess.run([exe, "--noSuchOption", "a", "b"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1
    (tmp_path / "empty.fa").write_text("")
    r = subprocess.run([exe, str(tmp_path / "empty.fa"), str(tmp_path / "empty.fa")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout == ""      # no pairs: nothing to align, no device needed
