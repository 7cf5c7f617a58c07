"""A threshold of their own for HSPs that only variant hits seed (cpecan_anchor_options.transitionHspThreshold), without a
GPU: the ABI, what is refused before a device is looked for, the model (tests/anchor_model_threshold.py) against the two
models it lies between, its integers and the quality they buy on the ENCODE pairs, and the option on the command line."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import anchor_model_threshold as ath
import anchor_model_transitions as amt
import anchor_threshold_cases as thc
import anchor_transition_cases as tc
import oracle_binding as ob
import reference_cases as rc
from cpecan_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dog_threshold_oracle_pairs.npz")


def _encode(name):
    return rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)


def _inputs():
    """Constructed, random and masked pairs (the ENCODE pairs have tests of their own)."""
    out = [tc.case(which) for which in "abc"] + [thc.mixed_classes()]
    for index in (1, 2, 3):
        out += [ac.random_pair(index, 3000), ac.masked_pair(index, 3000)]
    return out


def _without_hits(st):
    return {k: v for k, v in st.items() if k != "hits"}


def _calls(sx, sy, params, options):
    return (lambda: api.find_anchor_runs(sx, sy, params=params, options=options),
            lambda: api.find_anchor_runs_many([(sx, sy)], params=params, options=options),
            lambda: api.find_anchor_runs_once(sx, sy, params=params, options=options),
            lambda: api.find_anchor_runs_many_stranded([(sx, sy)], params=params, strand="both", options=options))


def test_the_options_through_the_abi():
    assert C.sizeof(api.AnchorOptions) == 32 and C.sizeof(api.AnchorParams) == 152
    o = api.AnchorOptions(transitionHspThreshold=5)
    o.reserved[3] = 7
    assert api.lib().cpecan_anchor_options_default(C.byref(o)) == 0
    assert bytes(o) == bytes(32)
    assert api.lib().cpecan_anchor_options_default(None) == -1
    assert api.anchor_options().transitionHspThreshold == 0
    assert api.anchor_options(transitionHspThreshold=1200).transitionHspThreshold == 1200


def test_bad_options_are_refused_before_a_device_is_looked_for():
    sx, sy = tc.case("a")
    reserved = api.anchor_options(1200)
    reserved.reserved[6] = 1
    for transitions in (0, 1):
        p = api.anchor_params_default(seedTransitions=transitions)       # hspThreshold 800
        for bad in (api.anchor_options(1), api.anchor_options(799), api.anchor_options(-1), api.anchor_options(-2 ** 31),
                    reserved):
            for call in _calls(sx, sy, p, bad):
                with pytest.raises(api.CpecanError) as e:
                    call()
                assert "(-1)" in str(e.value)       # CPECAN_EINVAL: the same with and without a device
    # the bound is the parameters' hspThreshold, not the default's
    with pytest.raises(api.CpecanError) as e:
        api.find_anchor_runs(sx, sy, params=api.anchor_params_default(seedTransitions=1, hspThreshold=1500),
                             options=api.anchor_options(1200))
    assert "(-1)" in str(e.value) and "transitionHspThreshold" in str(e.value)
    # bad parameters are still refused with good options
    with pytest.raises(api.CpecanError) as e:
        api.find_anchor_runs(sx, sy, params=api.anchor_params_default(seedTransitions=2), options=api.anchor_options(1200))
    assert "(-1)" in str(e.value)


def test_without_a_device_valid_options_answer_no_device():
    if api.device_count() > 0:
        return  # with a GPU the calls succeed: tests/test_gpu_anchor_threshold.py
    sx, sy = tc.case("a")
    p = api.anchor_params_default(seedTransitions=1)
    for good in (api.anchor_options(), api.anchor_options(800), api.anchor_options(1200), api.anchor_options(2 ** 31 - 1)):
        for call in _calls(sx, sy, p, good):
            with pytest.raises(api.CpecanError) as e:
                call()
            assert "(-2)" in str(e.value)
    smachine = api.stateMachine5_construct(api.fiveState)
    bp = api.pairwiseAlignmentBandingParameters_construct()
    for call in (lambda: api.getAlignedPairs(smachine, sx, sy, bp, anchorParams=p, anchorOptions=api.anchor_options(1200)),
                 lambda: api.getAlignedPairsWithIndels(smachine, sx, sy, bp, anchorParams=p, anchorOptions=api.anchor_options(1200)),
                 lambda: api.getAlignedPairsStranded(smachine, sx, sy, bp, anchorParams=p, anchorOptions=api.anchor_options(1200))):
        with pytest.raises(api.CpecanError) as e:
            call()
        assert "(-2)" in str(e.value)
    with pytest.raises(api.CpecanError) as e:
        api.getAlignedPairs(smachine, sx, sy, bp, anchorParams=p, anchorOptions=api.anchor_options(799))
    assert "(-1)" in str(e.value)


def test_at_hsp_threshold_the_model_is_the_transitions_model():
    p = am.default_params()
    for sx, sy in _inputs():
        for T in (0, p["hspThreshold"]):
            runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=T)
            want, wst = amt.find_anchor_runs(sx, sy, seedTransitions=1)
            assert np.array_equal(runs, want) and st == wst
        for softMask in (True, False):
            assert ath.anchors_once(sx, sy, 14, softMask, p, 1, 800) == amt.anchors_once(sx, sy, 14, softMask, p, 1)
        assert ath.strand_score(sx, sy, p, 1, 800) == amt.strand_score(sx, sy, p, 1)
        # ... and without seedTransitions there is no variant hit for the threshold to test
        runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=0, threshold=ath.INT32_MAX)
        want, wst = am.find_anchor_runs(sx, sy)
        assert np.array_equal(runs, want) and st == wst


def test_at_int32_max_the_model_is_anchor_model_but_for_hits():
    more = 0
    for sx, sy in _inputs():
        runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=ath.INT32_MAX)
        want, wst = am.find_anchor_runs(sx, sy)
        assert np.array_equal(runs, want) and _without_hits(st) == _without_hits(wst)
        assert st["hits"] >= wst["hits"]
        more += st["hits"] > wst["hits"]
    assert more >= 6


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_the_identities_on_the_encode_pairs(name):
    sx, sy, _, _ = _encode(name)
    runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=800)
    want, wst = amt.find_anchor_runs(sx, sy, seedTransitions=1)
    assert np.array_equal(runs, want) and st == wst
    runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=ath.INT32_MAX)
    want, wst = am.find_anchor_runs(sx, sy)
    assert np.array_equal(runs, want) and _without_hits(st) == _without_hits(wst) and st["hits"] > wst["hits"]


def test_the_threshold_is_refused_below_hsp_threshold_by_the_model_too():
    sx, sy = tc.case("a")
    for bad in (799, 1, -5):
        with pytest.raises(ValueError):
            ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=bad)


def test_the_constructed_pair_has_one_hsp_of_every_class():
    """tests/anchor_threshold_cases.py: what its header promises, by the model."""
    sx, sy = thc.mixed_classes()
    p = am.default_params()
    T = thc.THRESHOLD
    kept, hits = ath.classed_hsps(sx, sy, True, p, 1, 0)
    by_place = {(x, y): (n, score, exact) for (x, y, n, score), exact in kept.items()}
    assert sorted(by_place) == [(a, a) for a, _ in sorted(thc.STRETCHES.values())]      # nothing off the main diagonal
    for which, (a, e) in thc.STRETCHES.items():
        assert by_place[(a, a)][0] == e - a
    (_, sa, ea), (_, sb, eb), (_, sc, ec) = (by_place[(thc.STRETCHES[w][0],) * 2] for w in "ABC")
    assert (ea, eb, ec) == (True, False, False)
    assert 800 <= sa < T <= sb and 800 <= sc < T
    classes = ath.classed_hits(sx, sy, p["seed"], 1, True, 1)
    assert sum(classes.values()) > 0 and sum(not v for v in classes.values()) > 10 and len(classes) == hits
    # all three chain without the threshold; with it exactly A and B
    runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=0)
    assert (st["hsps"], st["chained"]) == (3, 3)
    runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=T)
    assert (st["hsps"], st["chained"], st["hits"]) == (2, 2, hits)
    assert [r[0] - 14 for r in runs.tolist()] == [thc.STRETCHES["A"][0], thc.STRETCHES["B"][0]]
    # the smallest case: every hit of case("a") is a variant hit, and its one HSP stands or falls with the threshold
    x, ya = tc.case("a")
    kept, _ = ath.classed_hsps(x, ya, True, p, 1, 0)
    assert list(kept.values()) == [False]
    (score,) = [h[3] for h in kept]
    assert ath.find_anchor_runs(x, ya, seedTransitions=1, threshold=score)[1]["runs"] == 1
    st = ath.find_anchor_runs(x, ya, seedTransitions=1, threshold=score + 1)[1]
    assert (st["runs"], st["hsps"]) == (0, 0) and st["hits"] > 100


# name: runs, anchor columns, largest gap, at T = 1200 and defaults otherwise
ENCODE_AT_1200 = {"dog": (232, 10866, 5028764), "mouse": (89, 2373, 6150522)}


@functools.lru_cache(maxsize=None)
def _at_1200(name):
    sx, sy, _, true_pairs = _encode(name)
    return (sx, sy, true_pairs) + ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=1200)


@pytest.mark.parametrize("name", ["dog", "mouse"])
def test_at_1200_the_encode_pairs_give_the_recorded_integers(name):
    sx, sy, _, runs, st = _at_1200(name)
    assert (st["runs"], st["anchorColumns"], st["largestGap"]) == ENCODE_AT_1200[name]
    assert st["capped"] == 0 and len(am.runs_to_anchors(runs)) == st["anchorColumns"]
    # the filter the integers come from: in the seedTransitions = 0 HSP set, or score >= T -- on the top-level pass
    p = am.default_params()
    kept, _ = ath.classed_hsps(sx, sy, True, p, 1, 1200)
    every, _ = ath.classed_hsps(sx, sy, True, p, 1, 0)
    exact, _ = ath.classed_hsps(sx, sy, True, p, 0, 0)
    assert set(kept) == {h for h in every if h in exact or h[3] >= 1200}
    assert {h for h, e in every.items() if e} == set(exact)


def test_the_recorded_oracle_answer_was_fed_the_models_anchors():
    """tests/golden/dog_threshold_oracle_pairs.npz (tests/test_gpu_anchor_threshold.py compares the GPU with it)."""
    gold = np.load(GOLDEN)
    _, _, _, runs, _ = _at_1200("dog")
    assert np.array_equal(gold["runs"], runs) and gold["pairs"].shape == (68447, 3)


def _quality(sx, sy, anchors, true_pairs):
    """tools/anchor_transitions_quality.py: the oracle's pairs, ordered filter at 0.5, against the embedded alignment."""
    pairs = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params(diagonalExpansion=20))
    return rc.sensitivity_specificity(ob.filter_pairs_ordered(pairs, len(sx), len(sy), 0.5), true_pairs)


def test_at_1200_the_dog_pair_keeps_the_sensitivity_it_has_without_transitions():
    """profiles/anchor_quality_transition_threshold.txt: 0.9278 at T = 1200 against 0.9277 with seedTransitions = 0 and
    0.9015 with seedTransitions = 1 alone.  0.001: ties in the filter."""
    sx, sy, true_pairs, runs, _ = _at_1200("dog")
    sens, spec = _quality(sx, sy, am.runs_to_anchors(runs), true_pairs)
    sens0, spec0 = _quality(sx, sy, am.runs_to_anchors(am.find_anchor_runs(sx, sy)[0]), true_pairs)
    print("dog T=1200 %.4f / %.4f, seedTransitions=0 %.4f / %.4f" % (sens, spec, sens0, spec0))
    assert sens >= sens0 - 0.001


def test_at_1200_the_mouse_pair_clears_its_bars():
    sx, sy, true_pairs, runs, _ = _at_1200("mouse")
    sens, spec = _quality(sx, sy, am.runs_to_anchors(runs), true_pairs)
    print("mouse T=1200 %.4f / %.4f" % (sens, spec))
    assert sens >= 0.75 and spec >= 0.85


def test_cpecan_align_wants_seed_transitions_with_the_threshold(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--transitionHspThreshold" in r.stderr
    (tmp_path / "empty.fa").write_text("")
    files = [str(tmp_path / "empty.fa"), str(tmp_path / "empty.fa")]
    for flags in (["--transitionHspThreshold", "1200"], ["-T", "1200"], ["--transitionHspThreshold=1200", "--strand", "both"]):
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and "--transitionHspThreshold" in r.stderr and "--seedTransitions" in r.stderr
    # with it: no pairs, so no device is needed
    for flags in (["--seedTransitions", "--transitionHspThreshold", "1200"], ["-T", "1200", "-t"]):
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stdout == ""
    for flags in (["-t", "-T", "x"], ["-t", "-T", "-3"], ["-t", "-T"]):
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0
