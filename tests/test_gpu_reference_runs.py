"""The HIP library against what the reference itself computed (tests/golden/reference_runs.json.gz; see
tests/reference_run_cases.py and tests/test_reference_runs_cpu.py).  The oracle is not in between: every comparison is of
the library's output with a record of the reference's own code.

Match and indel lists: parity.assert_pairs_match, and the coordinate sets are equal -- no recorded score lies within the
margin of its threshold, so the gate's excuse for a one-sided pair is never needed.  Forward probabilities:
parity.assert_log_close.  Expectations: batches of one, at the gates of tests/test_gpu_expect.py (1e-5 relative + 1e-12
on the counts, 1e-9 relative on the likelihood, exactly 0.0 where the record has exactly 0).  Consumers: on the recorded
input lists, in the wave form and under CPECAN_POST_LANES=1, lists equal in order and scores equal doubles.
The cases of one model and one set of parameters run as one batch."""
import collections

import numpy as np
import pytest

import reference_run_cases as rr
from cpecan_amd import api
from parity import assert_log_close, assert_pairs_match

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in rr.fixture()["cases"]}
FORMS = (None, "1")  # CPECAN_POST_LANES
COUNT_RTOL, COUNT_ATOL, LIKELIHOOD_RTOL = 1e-5, 1e-12, 1e-9  # tests/expect_cases.py: ORACLE_RTOL, ORACLE_ATOL, ORACLE_LIKELIHOOD_RTOL


def _machine(name):
    m = rr.fixture()["models"][name]
    if "T" not in m:
        return api.stateMachine5_construct(m["type"]) if m["type"] == api.fiveState else api.stateMachine3_construct(m["type"])
    h = api.hmm_constructEmpty(0.0, m["type"])
    for i, v in enumerate(m["T"]):
        h.transitions[i] = v
    for i, v in enumerate(m["E"]):
        h.emissions[i] = v
    return api.hmm_getStateMachine(h)


def _params(c):
    p = c["params"]
    return api.pairwiseAlignmentBandingParameters_construct(
        threshold=p["threshold"], minDiagsBetweenTraceBack=p["minDiagsBetweenTraceBack"], traceBackDiagonals=p["traceBackDiagonals"],
        diagonalExpansion=p["diagonalExpansion"], splitMatrixBiggerThanThis=p["splitMatrixBiggerThanThis"],
        dynamicAnchorExpansion=bool(p["dynamicAnchorExpansion"]))


def _groups(op):
    """The cases that record `op`, grouped by model and parameters: one batch each."""
    groups = collections.OrderedDict()
    for c in CASES.values():
        if op in c["ops"]:
            key = (c["model"],) + tuple(sorted((k, v) for k, v in c["params"].items() if k != "gapGamma"))
            groups.setdefault(key, []).append(c)
    return list(groups.values())


def _batch(cases, emit):
    b = api.Batch(_machine(cases[0]["model"]), _params(cases[0]), emit=emit)
    for c in cases:
        b.add(c["sx"], c["sy"], [tuple(a) for a in c["anchors"]], *c["ragged"])
    return b


def _run(b):
    b.upload()
    b.run()
    b.download()


def _assert_list(got, want_flat, threshold, what):
    want = rr.triples(want_flat)
    got = np.asarray(got, dtype=np.int64).reshape(-1, 3)
    assert_pairs_match(got, want, threshold=threshold)
    assert {(int(x), int(y)) for _, x, y in got} == {(int(x), int(y)) for _, x, y in want}, "%s: the coordinate sets differ" % what
    assert len(got) == len(want), what


def _tuples(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def _form(monkeypatch, lanes):
    if lanes:
        monkeypatch.setenv("CPECAN_POST_LANES", lanes)
    else:
        monkeypatch.delenv("CPECAN_POST_LANES", raising=False)


def test_match_lists():
    seen = 0
    for cases in _groups("pairs"):
        with _batch(cases, api.EMIT_MATCH) as b:
            _run(b)
            for i, c in enumerate(cases):
                _assert_list(b.result(i), c["out"]["match"], c["params"]["threshold"], c["name"])
                seen += 1
    assert seen == sum("pairs" in c["ops"] for c in CASES.values()) >= 50


def test_indel_lists():
    seen = 0
    for cases in _groups("indels"):
        with _batch(cases, api.EMIT_INDEL) as b:
            _run(b)
            for i, c in enumerate(cases):
                for which, key in enumerate(("imatch", "gapx", "gapy")):
                    _assert_list(b.result(i, which), c["out"][key], c["params"]["threshold"], "%s, %s" % (c["name"], key))
                seen += 1
    assert seen == sum("indels" in c["ops"] for c in CASES.values()) >= 40


def test_forward_probabilities():
    seen = 0
    for cases in _groups("forward"):
        with _batch(cases, api.EMIT_FORWARD) as b:
            _run(b)
            for i, c in enumerate(cases):
                assert_log_close(b.forward_prob(i), float.fromhex(c["out"]["fwd"]), "forward probability of %s" % c["name"])
                seen += 1
    assert seen == sum("forward" in c["ops"] for c in CASES.values()) >= 50


def test_expectations_problem_by_problem():
    worst = 0.0
    cases = [c for c in CASES.values() if "expect" in c["ops"]]
    assert len(cases) >= 50
    for c in cases:
        mtype = rr.fixture()["models"][c["model"]]["type"]
        acc = api.getExpectationsUsingAnchors(_machine(c["model"]), api.hmm_constructEmpty(0.0, mtype), c["sx"], c["sy"],
                                              [tuple(a) for a in c["anchors"]], _params(c), *c["ragged"])
        S = rr.states(c["model"])
        for name, got, want in (("T", np.array(acc.transitions[:S * S]), np.array(rr.hexes(c["out"]["T"]))),
                                ("E", np.array(acc.emissions[:S * 16]), np.array(rr.hexes(c["out"]["E"])))):
            bad = np.nonzero(~(np.abs(got - want) <= COUNT_RTOL * np.abs(want) + COUNT_ATOL))[0]
            assert len(bad) == 0, "%s: %s[%d] is %.17g, the reference has %.17g" % (c["name"], name, bad[0], got[bad[0]], want[bad[0]])
            stray = np.nonzero((want == 0.0) & (got != 0.0))[0]
            assert len(stray) == 0, "%s: %s[%d] is %g where the reference has exactly 0" % (c["name"], name, stray[0], got[stray[0]])
            big = np.abs(want) >= 1e-3
            if big.any():
                worst = max(worst, float((np.abs(got - want)[big] / np.abs(want)[big]).max()))
        want = float.fromhex(c["out"]["likelihood"])
        assert abs(acc.likelihood - want) <= LIKELIHOOD_RTOL * abs(want), "%s: likelihood %.17g, the reference has %.17g" % (
            c["name"], acc.likelihood, want)
        assert want != 0.0 or acc.likelihood == 0.0, c["name"]
    print("largest relative difference of a count of at least 1e-3: %.3g" % worst)


@pytest.mark.parametrize("lanes", FORMS)
def test_shifted_mea_end_to_end(lanes, monkeypatch):
    _form(monkeypatch, lanes)
    cases = [c for c in CASES.values() if "shifted_mea" in c["ops"]]
    assert len(cases) == 3
    for c in cases:
        # On the reference's own three lists the two consumers give the record itself: list and score equal.
        out, lX, lY = c["out"], len(c["sx"]), len(c["sy"])
        mea, mea_score = api.getMaximalExpectedAccuracyPairwiseAlignment(rr.triples(out["imatch"]), rr.triples(out["gapx"]),
                                                                         rr.triples(out["gapy"]), lX, lY, gapGamma=c["params"]["gapGamma"])
        assert _tuples(api.leftShiftAlignment(mea, c["sx"], c["sy"])) == _tuples(out["shifted_mea"]), c["name"]
        assert mea_score == float.fromhex(out["shifted_mea_score"]), c["name"]
        # End to end the lists between the emitter and the chain are the device's own, each entry within max(1, 1e-5 score)
        # of the reference's (the gate of test_indel_lists).  So: the chain's coordinates are the reference's, in order; its
        # scores, borrowed from those lists, meet that gate; and the alignment score -- a sum of chain weights and of
        # gamma times gap entries -- lies within 1e-5 of the recorded score plus one unit for every entry that can go
        # into the sum: the pairs of the MEA chain (no more than of the shifted one) and gamma for each recorded gap entry.
        # The unit per chain pair also covers the int64 truncation of each step of the walk, which can fall the other way
        # once its inputs moved (under one unit a pair): every listed entry is at least threshold * 1e7 = 1e5 here, so
        # its own gate max(1, 1e-5 score) is already inside the relative term.  Nothing further is to be added.
        got, score = api.getShiftedMEAAlignment(c["sx"], c["sy"], [tuple(a) for a in c["anchors"]], _params(c), _machine(c["model"]),
                                                *c["ragged"], gapGamma=c["params"]["gapGamma"])
        want = rr.triples(c["out"]["shifted_mea"])
        assert [(x, y) for _, x, y in _tuples(got)] == [(int(x), int(y)) for _, x, y in want], c["name"]
        assert_pairs_match(got, want, threshold=c["params"]["threshold"])
        want_score = float.fromhex(c["out"]["shifted_mea_score"])
        entries = len(want) + c["params"]["gapGamma"] * (len(c["out"]["gapx"]) + len(c["out"]["gapy"])) / 3
        print("%s: alignment score %.17g, the reference has %.17g, bound %.3g" % (c["name"], score, want_score, 1e-5 * abs(want_score) + entries))
        assert abs(score - want_score) <= 1e-5 * abs(want_score) + entries, c["name"]


@pytest.mark.parametrize("lanes", FORMS)
def test_consumers_on_the_recorded_lists(lanes, monkeypatch):
    _form(monkeypatch, lanes)
    seen = collections.Counter()
    for c in CASES.values():
        out = c["out"]
        if "mea" in c["ops"]:
            got, score = api.getMaximalExpectedAccuracyPairwiseAlignment(c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"],
                                                                         gapGamma=c["params"]["gapGamma"])
            assert _tuples(got) == _tuples(out["mea"]), c["name"]
            assert score == float.fromhex(out["mea_score"]), c["name"]
        if "reweight" in c["ops"]:
            got = api.reweightAlignedPairs2(c["pairs"], c["lX"], c["lY"], c["gamma"])
            assert _tuples(got) == _tuples(out["reweighted"]), c["name"]
        if "shift" in c["ops"]:
            assert _tuples(api.leftShiftAlignment(c["pairs"], c["sx"], c["sy"])) == _tuples(out["shifted"]), c["name"]
        if "scores" in c["ops"]:
            got = (api.scoreByIdentity(c["sx"], c["sy"], c["lX"], c["lY"], c["pairs"]),
                   api.scoreByIdentityIgnoringGaps(c["sx"], c["sy"], c["pairs"]),
                   api.scoreByPosteriorProbability(c["lX"], c["lY"], c["pairs"]),
                   api.scoreByPosteriorProbabilityIgnoringGaps(c["pairs"]))
            want = tuple(float.fromhex(out[k]) for k in ("identity", "identity_ignoring_gaps", "posterior", "posterior_ignoring_gaps"))
            assert got == want, c["name"]
        if "overlap" in c["ops"]:
            assert _tuples(api.filterToRemoveOverlap([tuple(p) for p in rr.triples(c["pairs"]).tolist()])) == _tuples(out["non_overlapping"]), c["name"]
        for op in c["ops"]:
            seen[op] += 1
    assert seen["mea"] >= 18 and seen["reweight"] >= 20 and seen["shift"] >= 7 and seen["scores"] >= 4 and seen["overlap"] >= 3
