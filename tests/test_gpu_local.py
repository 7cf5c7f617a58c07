"""Local chains on the GPU (cpecan_find_local_chains_many, cpk_local.inl) against their definition (tests/local_model.py):
strands, scores, rectangles, runs and counts integer for integer on every case of tests/local_cases.py; the consequences of
DESIGN.md section 7 step 7 on the device's answer; both K = 1 cross-checks against the entry points that were there
before; and the 300-problem batch against the same problems called one at a time."""
import numpy as np
import pytest

import anchor_model as am
import local_cases as lc
import local_model as lm
from cpecan_amd import api, local

pytestmark = pytest.mark.gpu

COUNTS = ("hitsPlus", "hitsMinus", "hspsPlus", "hspsMinus", "capped", "rounds")


def _params(case):
    return api.anchor_params_default(seedTransitions=case["seedTransitions"], **case["params"])


def _find(case, problems=None, **kw):
    options = api.anchor_options(transitionHspThreshold=case["threshold"]) if case["threshold"] else None
    kw.setdefault("options", local.local_options(maxChains=case["K"], minChainScore=case["S"]))
    kw.setdefault("strand", case["strand"])
    return local.find_local_chains(problems if problems is not None else case["problems"], trim=case["trim"], expansion=20,
                                   params=_params(case), anchor_options=options, **kw)


def _consequences(chains, lY, what):
    """Point 5 on one problem's chains: scores do not increase; no two chained runs meet on X or on forward Y."""
    scores = [c["score"] for c in chains]
    assert scores == sorted(scores, reverse=True), what
    xs, ys = [], []
    for c in chains:
        for x, y, length, _ in c["runs"].tolist():
            ix, iy = lm.intervals((x, y, length), c["strand"] == "minus", lY)
            xs.append(ix)
            ys.append(iy)
    for iv in (sorted(xs), sorted(ys)):
        assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:])), what


@pytest.mark.parametrize("name", lc.NAMES)
def test_case_equals_the_model(name):
    case = lc.by_name(name)
    got, stats = _find(case)
    want = lc.model(case)
    assert len(got) == len(want)
    for i, ((wchains, wstats), gchains, gstats) in enumerate(zip(want, got, stats)):
        what = (name, i)
        assert len(gchains) == len(wchains), what
        for g, w in zip(gchains, wchains):
            assert lm.same(g, w), (what, {k: g[k] for k in g if k != "runs"}, {k: w[k] for k in w if k not in ("runs", "hsps")})
        assert {k: int(gstats[k]) for k in COUNTS} == {k: int(wstats[k]) for k in COUNTS}, what
        assert sum(len(c["runs"]) for c in gchains) <= wstats["hspsPlus"] + wstats["hspsMinus"], what
        _consequences(gchains, len(case["problems"][i][1]), what)
        assert gstats["kernelMs"] > 0.0 or all(len(x) == 0 or len(y) == 0 for x, y in case["problems"]), what


def test_one_plus_chain_is_the_anchor_finder_once():
    """K = 1, PLUS, S <= the score: the runs are cpecan_find_anchor_runs_once(..., softMask = 1, ...), integer for integer."""
    for case in (lc.by_name("inversion"), lc.by_name("pool_sizes")):
        for trim in (0, 14):
            one = dict(case, K=1, S=0, trim=trim, strand="plus")
            got, _ = _find(one)
            for (sx, sy), chains in zip(case["problems"], got):
                runs = api.find_anchor_runs_once(sx, sy, trim=trim, expansion=20, softMask=True, params=_params(case))
                assert len(chains) == 1 and np.array_equal(chains[0]["runs"], runs), (case["name"], trim)


def test_one_chain_of_both_is_the_strand_result():
    """K = 1, BOTH: strand and score are what cpecan_find_anchor_runs_many_stranded reports in cpecan_strand_result."""
    for name in ("inversion", "tie", "pool_sizes", "nothing"):
        case = lc.by_name(name)
        got, _ = _find(dict(case, K=1, S=0))
        _, _, strands = api.find_anchor_runs_many_stranded(case["problems"], params=_params(case), strand="both")
        for chains, s in zip(got, strands):
            if max(s["scorePlus"], s["scoreMinus"]) <= 0:
                assert chains == [], name
            else:
                assert len(chains) == 1, name
                assert (chains[0]["strand"], chains[0]["score"]) == (s["strand"], max(s["scorePlus"], s["scoreMinus"])), name


def test_batch_equals_one_at_a_time_and_the_model():
    case = lc.batch_case()
    got, stats = _find(case)
    assert len(got) == 300
    want = lc.model(case)
    kinds = set()
    for i, pr in enumerate(case["problems"]):
        alone, alone_stats = _find(case, problems=[pr])
        assert len(alone[0]) == len(got[i]) == len(want[i][0]), i
        for g, a, w in zip(got[i], alone[0], want[i][0]):
            assert lm.same(g, a) and lm.same(g, w), i
        assert {k: stats[i][k] for k in COUNTS} == {k: alone_stats[0][k] for k in COUNTS} == {k: want[i][1][k] for k in COUNTS}, i
        kinds.add(tuple(c["strand"] for c in got[i]))
    assert got[17] == [] and got[101] == [] and len(kinds) >= 3
