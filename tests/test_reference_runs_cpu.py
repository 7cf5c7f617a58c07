"""The oracle against what the reference itself computed (tests/golden/reference_runs.json.gz: the reference's own
impl/pairwiseAligner.c and impl/stateMachine.c built on stand-in headers, oracle/Makefile target `ref`, run on the cases of
tests/reference_run_cases.py).  The oracle claims to be the reference operation for operation and is built with the same
contraction setting and the same libm, so the gate is equality: lists integer for integer and in order, doubles bit for
bit.  No GPU."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import reference_run_cases as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "cpecan_ref_driver")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")

CASES = {c["name"]: c for c in rr.fixture()["cases"]}
DP_NAMES = [n for n, c in CASES.items() if set(c["ops"]) & set(rr.DP_OPS)]
# the records that are empty by design: everything else that is a list must hold something
EMPTY_BY_DESIGN = {("mea-empty_list_with_gaps", "mea"), ("mea-empty_chain", "mea"), ("mea-n0-bare", "mea"),
                   ("reweight-n_0-0.5", "reweighted"), ("reweight-n_0-0", "reweighted"), ("overlap-empty", "non_overlapping")}


def bits(v):
    return struct.pack("<d", v)


def assert_same_double(got, want_hex, what):
    want = float.fromhex(want_hex)
    assert bits(got) == bits(want) or (got != got and want != want), "%s: oracle %s (%r) vs reference %s" % (what, got.hex(), got, want_hex)


def assert_same_list(got, want_flat, what):
    got, want = np.asarray(got, dtype=np.int64).reshape(-1, 3), rr.triples(want_flat)
    assert got.shape == want.shape, "%s: oracle %d entries vs reference %d" % (what, len(got), len(want))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: entry %d: oracle %s vs reference %s" % (what, bad[0], got[bad[0]], want[bad[0]])


def oracle_model(name):
    m = rr.fixture()["models"][name]
    if "T" not in m:
        return ob.model(m["type"])
    h = ob.hmm(m["type"], 0.0)
    for i, v in enumerate(m["T"]):
        h.T[i] = v
    for i, v in enumerate(m["E"]):
        h.E[i] = v
    return ob.model_from_hmm(h)


def oracle_params(c):
    p = c["params"]
    return ob.params(threshold=p["threshold"], minDiagsBetweenTraceBack=p["minDiagsBetweenTraceBack"],
                     traceBackDiagonals=p["traceBackDiagonals"], diagonalExpansion=p["diagonalExpansion"],
                     splitMatrixBiggerThanThis=p["splitMatrixBiggerThanThis"], dynamicAnchorExpansion=p["dynamicAnchorExpansion"])


def test_the_fixture_is_the_case_list():
    """The committed inputs are the ones tests/reference_run_cases.py makes now, in the same order."""
    cases = rr.all_cases()
    assert [c["name"] for c in cases] == list(CASES)
    for c in cases:
        kept = dict(CASES[c["name"]])
        kept.pop("out")
        assert kept == json.loads(json.dumps(c)), c["name"]
    assert rr.fixture()["models"] == json.loads(json.dumps(rr.models()))
    assert 100 <= len(cases) <= 150
    assert all(len(c["sx"]) <= 300 and len(c["sy"]) <= 300 for c in cases)
    assert os.path.getsize(rr.FIXTURE) <= 405 * 1000  # the largest fixture there was before this one


def test_every_record_is_there_and_no_list_is_empty_by_accident():
    keys = {"pairs": ("match",), "indels": ("imatch", "gapx", "gapy"), "forward": ("fwd",), "expect": ("T", "E", "likelihood"),
            "shifted_mea": ("shifted_mea", "shifted_mea_score"), "mea": ("mea", "mea_score"),
            "reweight": ("indel_probs_x", "indel_probs_y", "reweighted"), "shift": ("shifted",),
            "scores": ("identity", "identity_ignoring_gaps", "posterior", "posterior_ignoring_gaps"), "overlap": ("non_overlapping",)}
    seen_ops = set()
    for name, c in CASES.items():
        want = [k for op in c["ops"] for k in keys[op]]
        assert sorted(c["out"]) == sorted(want), name
        seen_ops |= set(c["ops"])
        for k, v in c["out"].items():
            if isinstance(v, list) and (name, k) not in EMPTY_BY_DESIGN:
                assert len(v) > 0, "%s: the recorded %s is empty" % (name, k)
    assert seen_ops == set(keys)
    for name, k in EMPTY_BY_DESIGN:
        assert CASES[name]["out"][k] == [], (name, k)


def test_no_recorded_score_is_near_its_threshold():
    """What tests/golden/make_reference_runs.py saw to at threshold 0, visible in the thresholded lists themselves: every
    recorded score lies above the threshold by more than the margin."""
    for name, c in CASES.items():
        t = c["params"]["threshold"]
        for op in c["ops"]:
            for k in rr.LIST_KEYS.get(op, ()):
                s = rr.triples(c["out"][k])[:, 0]
                if t > 0:
                    assert (s > t * rr.PROB_1 + rr.threshold_margin(t)).all(), (name, k)


def test_closed_form_lengths_of_the_unbanded_pair_at_threshold_zero():
    c = CASES[rr.CLOSED_FORM]
    assert c["params"]["threshold"] == 0 and not c["anchors"] and c["ragged"] == [False, False]
    got = tuple(len(c["out"][k]) // 3 for k in ("imatch", "gapx", "gapy"))
    assert got == rr.closed_form_lengths(len(c["sx"]), len(c["sy"]))


@pytest.mark.parametrize("name", DP_NAMES)
def test_oracle_dp_against_the_reference(name):
    c = CASES[name]
    m, p, (rl, rr_) = oracle_model(c["model"]), oracle_params(c), c["ragged"]
    args = (m, c["sx"], c["sy"], c["anchors"], p, rl, rr_)
    out = c["out"]
    if "pairs" in c["ops"]:
        assert_same_list(ob.aligned_pairs(*args), out["match"], "match list")
    if "indels" in c["ops"]:
        for got, k in zip(ob.aligned_pairs_with_indels(*args), ("imatch", "gapx", "gapy")):
            assert_same_list(got, out[k], k)
    if "forward" in c["ops"]:
        assert_same_double(ob.forward_prob(*args), out["fwd"], "forward probability")
    if "expect" in c["ops"]:
        mtype = rr.fixture()["models"][c["model"]]["type"]
        acc = ob.expectations(m, ob.hmm(mtype, 0.0), *args[1:])
        S = rr.states(c["model"])
        for i in range(S * S):
            assert_same_double(acc.T[i], out["T"][i], "T[%d]" % i)
        for i in range(S * 16):
            assert_same_double(acc.E[i], out["E"][i], "E[%d]" % i)
        assert_same_double(acc.likelihood, out["likelihood"], "likelihood")
    if "shifted_mea" in c["ops"]:
        lists = ob.aligned_pairs_with_indels(*args)
        mea, score = ob.mea_alignment(*lists, len(c["sx"]), len(c["sy"]), c["params"]["gapGamma"])
        assert_same_list(ob.left_shift_alignment(mea, c["sx"], c["sy"]), out["shifted_mea"], "shifted MEA alignment")
        assert_same_double(score, out["shifted_mea_score"], "MEA score")


@pytest.mark.parametrize("name", [n for n in CASES if n not in DP_NAMES])
def test_oracle_consumers_against_the_reference(name):
    c = CASES[name]
    out, pairs = c["out"], rr.triples(c["pairs"])
    if "mea" in c["ops"]:
        got, score = ob.mea_alignment(pairs, rr.triples(c["gx"]), rr.triples(c["gy"]), c["lX"], c["lY"], c["params"]["gapGamma"])
        assert_same_list(got, out["mea"], "MEA alignment")
        assert_same_double(score, out["mea_score"], "MEA score")
    if "reweight" in c["ops"]:
        assert ob.indel_probabilities(pairs, c["lX"], True).tolist() == out["indel_probs_x"]
        assert ob.indel_probabilities(pairs, c["lY"], False).tolist() == out["indel_probs_y"]
        assert_same_list(ob.reweight_aligned_pairs(pairs, c["lX"], c["lY"], c["gamma"]), out["reweighted"], "reweighted list")
    if "shift" in c["ops"]:
        assert_same_list(ob.left_shift_alignment(pairs, c["sx"], c["sy"]), out["shifted"], "left-shifted list")
    if "scores" in c["ops"]:
        assert_same_double(ob.score_by_identity(c["sx"], c["sy"], pairs), out["identity"], "scoreByIdentity")
        assert_same_double(ob.score_by_identity_ignoring_gaps(c["sx"], c["sy"], pairs), out["identity_ignoring_gaps"],
                           "scoreByIdentityIgnoringGaps")
        assert_same_double(ob.score_by_posterior(c["lX"], c["lY"], pairs), out["posterior"], "scoreByPosteriorProbability")
        assert_same_double(ob.score_by_posterior_ignoring_gaps(pairs), out["posterior_ignoring_gaps"],
                           "scoreByPosteriorProbabilityIgnoringGaps")
    if "overlap" in c["ops"]:
        assert_same_list(ob.filter_to_remove_overlap(pairs), out["non_overlapping"], "filterToRemoveOverlap")


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "impl", "pairwiseAligner.c")), reason="needs the reference tree")
def test_the_driver_gives_the_committed_fixture(tmp_path):
    """Runs the reference again on the case file: the committed fixture is what it writes, byte for byte.  Where the tree
    is there the driver has to build: a recipe that stopped compiling fails here, it does not skip."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", "REFERENCE=" + REFERENCE])
    data = rr.fixture_bytes(DRIVER, str(tmp_path))
    committed = open(rr.FIXTURE, "rb").read()
    assert gzip.decompress(data) == gzip.decompress(committed)
    assert data == committed
