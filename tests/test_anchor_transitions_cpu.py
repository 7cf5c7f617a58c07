"""Seed hits that tolerate one transition, without a GPU: the model (tests/anchor_model_transitions.py) against
tests/anchor_model.py with the option off, its integers on the ENCODE pairs with the option on, constructed cases that tell a
transition from a transversion and from two transitions, the occurrence filter, and the option through the ABI and the
command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import anchor_model_transitions as amt
import anchor_transition_cases as tc
import reference_cases as rc
from cpecan_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _encode(name):
    return rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_without_transitions_the_model_is_anchor_model_on_the_encode_pairs(name):
    sx, sy, _, _ = _encode(name)
    runs, st = amt.find_anchor_runs(sx, sy, seedTransitions=0)
    want, wst = am.find_anchor_runs(sx, sy)
    assert np.array_equal(runs, want) and st == wst


def test_without_transitions_the_model_is_anchor_model_on_random_pairs():
    for index in (1, 2, 3):
        for maker in (ac.random_pair, ac.masked_pair):
            sx, sy = maker(index, 3000)
            runs, st = amt.find_anchor_runs(sx, sy, seedTransitions=0)
            want, wst = am.find_anchor_runs(sx, sy)
            assert np.array_equal(runs, want) and st == wst and st["runs"] > 0
            assert amt.seed_hits(sx, sy, tc.SEED, 1, True) == am.seed_hits(sx, sy, tc.SEED, 1, True)
            assert amt.anchors_once(sx, sy, 14, False, am.default_params()) == am.anchors_once(sx, sy, 14, False, am.default_params())


# name: hits, hsps, runs, anchor columns, of which on the embedded alignment, largest gap (top level = final)
ENCODE_WITH_TRANSITIONS = {"mouse": (1537, 835, 91, 2378, 2306, 6150522), "dog": (3792, 1510, 233, 10869, 10638, 5028764)}


@pytest.mark.parametrize("name", ["mouse", "dog"])
def test_with_transitions_the_encode_pairs_give_the_recorded_integers(name):
    sx, sy, _, true_pairs = _encode(name)
    runs, st = amt.find_anchor_runs(sx, sy, seedTransitions=1)
    anchors = am.runs_to_anchors(runs)
    on = sum((x, y) in true_pairs for x, y, _ in anchors)
    got = (st["hits"], st["hsps"], st["runs"], st["anchorColumns"], on, st["largestGap"])
    assert got == ENCODE_WITH_TRANSITIONS[name]
    assert st["largestGapTop"] == st["largestGap"] and len(anchors) == st["anchorColumns"] and st["capped"] == 0


def test_the_recorded_oracle_answer_was_fed_the_models_anchors():
    """tests/golden/mouse_transitions_oracle_pairs.npz (tests/test_gpu_anchor_transitions.py compares the GPU with it)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mouse_transitions_oracle_pairs.npz"))
    sx, sy, _, _ = _encode("mouse")
    runs, _ = amt.find_anchor_runs(sx, sy, seedTransitions=1)
    assert np.array_equal(gold["runs"], runs) and gold["pairs"].shape == (61372, 3)


def test_constructed_pairs_tell_one_transition_from_a_transversion_and_from_two():
    x, ya = tc.case("a")
    _, yb = tc.case("b")
    _, yc = tc.case("c")
    # the construction: (a) and (b) change the same positions, no window of the diagonal is unchanged at the compared
    # offsets, some carry one change; in (c) every window carries two or more
    assert [i for i in range(tc.LENGTH) if x[i] != ya[i]] == [i for i in range(tc.LENGTH) if x[i] != yb[i]]
    assert min(tc.changes_per_window(x, ya)) == 1 and tc.changes_per_window(x, ya) == tc.changes_per_window(x, yb)
    assert min(tc.changes_per_window(x, yc)) == 2
    assert all((am._CODE[a] ^ am._CODE[b]) in (0, 2) for a, b in zip(x, ya))
    assert all((am._CODE[a] ^ am._CODE[b]) in (0, 1) for a, b in zip(x, yb))
    assert all((am._CODE[a] ^ am._CODE[b]) in (0, 2) for a, b in zip(x, yc))
    for y in (ya, yb, yc):
        assert amt.seed_hits(x, y, tc.SEED, 1, True, 0) == set() == am.seed_hits(x, y, tc.SEED, 1, True)
    hits = amt.seed_hits(x, ya, tc.SEED, 1, True, 1)
    per_window = tc.changes_per_window(x, ya)
    assert hits == {(i, i) for i in range(len(per_window)) if per_window[i] == 1} and len(hits) > 100
    assert amt.seed_hits(x, yb, tc.SEED, 1, True, 1) == set()
    assert amt.seed_hits(x, yc, tc.SEED, 1, True, 1) == set()
    # through every step: (a) is anchored with the option and not without it
    assert amt.find_anchor_runs(x, ya, seedTransitions=0)[1]["runs"] == 0
    runs, st = amt.find_anchor_runs(x, ya, seedTransitions=1)
    assert st["hits"] == len(hits) and st["hsps"] == 1 and st["anchorColumns"] > 600
    assert amt.find_anchor_runs(x, yb, seedTransitions=1)[1]["hits"] == 0
    assert amt.find_anchor_runs(x, yc, seedTransitions=1)[1]["hits"] == 0


def test_hand_worked_variants_and_the_occurrence_filter():
    seed = "1101"
    #     ACGA at X window 2; Y window 1 = GCTA: G C . A is ACGA's word with the first base's transition
    sx, sy = "TTACGATT", "AGCTAGC"
    assert amt.seed_hits(sx, sy, seed, 1, False, 0) == set()
    assert amt.seed_hits(sx, sy, seed, 1, False, 1) == {(2, 1)}
    assert amt.seed_hits(sx, "ACCTAGC", seed, 1, False, 1) == set()          # C for A: a transversion
    assert amt.seed_hits(sx, "AGTTAGC", seed, 1, False, 1) == set()          # G for A and T for C: two transitions
    assert amt.seed_hits(sx, "AGCTGGC", seed, 1, False, 1) == set()          # two again: first and last compared base
    assert amt.seed_hits(sx, "AGCCAGC", seed, 1, False, 1) == {(2, 1)}       # the 0 position compares nothing
    # a word that occurs twice in Y seeds nothing through a variant either; the count is of exact words, per side
    twice = sy + "AGCTA"
    assert amt.seed_hits(sx, twice, seed, 1, False, 1) == set()
    assert amt.seed_hits(sx, twice, seed, 2, False, 1) == {(2, 1), (2, 8)}
    # ... and so does a word that occurs twice in X
    assert amt.seed_hits(sx + "ACGA", sy, seed, 1, False, 1) == set()
    assert amt.seed_hits(sx + "ACGA", sy, seed, 2, False, 1) == {(2, 1), (8, 1)}
    # ACGA and its variant GCGA once each in X: either is under the limit on its own, and both hit the one Y window ACTA
    assert amt.seed_hits(sx + "GCGA", "AACTATT", seed, 1, False, 0) == {(2, 1)}
    assert {(2, 1), (8, 1)} <= amt.seed_hits(sx + "GCGA", "AACTATT", seed, 1, False, 1)
    # skipped windows stay skipped
    assert amt.seed_hits("TTANGATT", sy, seed, 1, False, 1) == set()
    assert amt.seed_hits("TTaCGATT", sy, seed, 1, False, 1) == {(2, 1)}
    assert amt.seed_hits("TTaCGATT", sy, seed, 1, True, 1) == set()
    with pytest.raises(ValueError):
        amt.seed_hits(sx, sy, seed, 1, False, 2)


def test_the_option_through_the_abi():
    assert C.sizeof(api.AnchorParams) == 152 and api.AnchorParams.seedTransitions.offset == 148
    assert api.anchor_params_default().seedTransitions == 0
    assert api.anchor_params_default(seedTransitions=1).seedTransitions == 1
    sx, sy = tc.case("a")
    for bad in (2, -1):
        for call in (lambda p: api.find_anchor_runs(sx, sy, params=p), lambda p: api.find_anchor_runs_many([(sx, sy)], params=p),
                     lambda p: api.find_anchor_runs_once(sx, sy, params=p),
                     lambda p: api.find_anchor_runs_many_stranded([(sx, sy)], params=p, strand="both")):
            with pytest.raises(api.CpecanError) as e:
                call(api.anchor_params_default(seedTransitions=bad))
            assert "(-1)" in str(e.value)           # refused before a device is looked for: the same with and without one


def test_without_a_device_the_calls_still_answer_no_device():
    if api.device_count() > 0:
        return  # with a GPU the calls succeed: tests/test_gpu_anchor_transitions.py
    sx, sy = tc.case("a")
    p = api.anchor_params_default(seedTransitions=1)
    for call in (lambda: api.find_anchor_runs_many([(sx, sy)], params=p), lambda: api.find_anchor_runs(sx, sy, params=p),
                 lambda: api.find_anchor_runs_once(sx, sy, params=p),
                 lambda: api.find_anchor_runs_many_stranded([(sx, sy)], params=p, strand="both")):
        with pytest.raises(api.CpecanError) as e:
            call()
        assert "(-2)" in str(e.value)


def test_cpecan_align_names_the_option(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--seedTransitions" in r.stderr
    # the option takes no argument: two files still follow it; no pairs, so no device is needed
    (tmp_path / "empty.fa").write_text("")
    for flag in ("--seedTransitions", "-t"):
        r = subprocess.run([exe, flag, str(tmp_path / "empty.fa"), str(tmp_path / "empty.fa")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stdout == ""
    r = subprocess.run([exe, "--seedTransitions", str(tmp_path / "empty.fa")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert r.returncode == 1
