"""Local chains with gapped extension on the GPU (cpecan_find_local_chains_many_gapped, cpk_local_gapped of cpk_local.inl)
against the rule (tests/local_model_gapped.py): records, runs and statistics integer for integer
on every case of tests/local_gapped_cases.py, the consequences of the rule on the device's answer, the batch against its
problems one at a time, and a batch whose first round passes the scratch budget and goes through the sliced launches."""
import random

import numpy as np
import pytest

import anchor_model as am
import anchor_model_gapped as amg
import local_cases as lc
import local_gapped_cases as gc
import local_model as lm
from cpecan_amd import api, local

pytestmark = pytest.mark.gpu

COUNTS = ("hitsPlus", "hitsMinus", "hspsPlus", "hspsMinus", "capped", "rounds")
BUDGET_ROWS = 4 << 20                                      # CPK_ANCHOR_GAPPED_BUDGET_ROWS of cpecan_internal.h


def _params(case):
    return api.anchor_params_default(seedTransitions=case["seedTransitions"], **case["params"])


def _anchor_options(case):
    return api.anchor_options(gappedExtension=case["gapped"], yDrop=case["yDrop"], gappedMaxDiagonals=case["maxDiagonals"])


def _find(case, problems=None, gapped=True, **kw):
    kw.setdefault("options", local.local_options(maxChains=case["K"], minChainScore=case["S"]))
    if gapped:
        kw.setdefault("anchor_options", _anchor_options(case))
    return local.find_local_chains(problems if problems is not None else case["problems"], trim=case["trim"], expansion=20,
                                   params=_params(case), strand=case["strand"], gapped=gapped, **kw)


def _same(got, want, what):
    """One problem's answer against the model's: every chain, every count."""
    (gchains, gstats), (wchains, wstats) = got, want
    assert len(gchains) == len(wchains), what
    for g, w in zip(gchains, wchains):
        assert lm.same(g, w), (what, {k: g[k] for k in g if k != "runs"}, {k: w[k] for k in g if k != "runs"}, g["runs"].tolist(),
                               w["runs"].tolist())
    assert {k: int(gstats[k]) for k in COUNTS} == {k: int(wstats[k]) for k in COUNTS}, what


@pytest.mark.parametrize("name", gc.NAMES)
def test_case_equals_the_model(name):
    case = gc.by_name(name)
    got, stats = _find(case)
    want = gc.model(case)
    assert len(got) == len(want)
    for i in range(len(want)):
        _same((got[i], stats[i]), want[i], (name, i))
        assert stats[i]["kernelMs"] > 0.0


@pytest.mark.parametrize("name", ["inversion", "transposition", "shared_middle", "end_gaps"])
def test_consequences_hold_on_the_device_output(name):
    """Trim 0, so the runs are the untrimmed blocks: disjoint on X and on forward Y over the whole problem; ascending on both
    axes within a chain; the rectangle theirs; every chained HSP (the model's: the records do not list them) inside a block of
    its chain, on its diagonal; and more runs than HSPs somewhere."""
    case = gc.by_name(name)
    assert case["trim"] == 0
    got, _ = _find(case)
    more = 0
    for (sx, sy), chains, (wchains, _) in zip(case["problems"], got, gc.model(case)):
        xs, ys = [], []
        for c, w in zip(chains, wchains):
            runs = c["runs"].tolist()
            assert all(p[0] + p[2] <= q[0] and p[1] + p[2] <= q[1] for p, q in zip(runs, runs[1:])), name
            assert (c["x0"], c["y0"]) == tuple(runs[0][:2]) and (c["x1"], c["y1"]) == (runs[-1][0] + runs[-1][2], runs[-1][1] + runs[-1][2])
            assert 0 <= c["x0"] and c["x1"] <= len(sx) and 0 <= c["y0"] and c["y1"] <= len(sy), name
            for h in w["hsps"]:
                assert any(p[0] <= h[0] and h[0] + h[2] <= p[0] + p[2] and p[0] - p[1] == h[0] - h[1] for p in runs), name
            for x, y, length, _ in runs:
                ix, iy = lm.intervals((x, y, length), c["strand"] == "minus", len(sy))
                xs.append(ix)
                ys.append(iy)
            more += len(runs) > c["nHsps"]
        for iv in (sorted(xs), sorted(ys)):
            assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:])), name
    assert more > 0


def test_one_plus_chain_is_the_gapped_anchor_finder_once():
    """K = 1, PLUS: the runs of cpecan_find_anchor_runs_once(softMask = 1) with the same options, integer for integer."""
    case = gc.by_name("one_chain")
    for trim, kw in ((0, dict()), (14, dict()), (0, dict(yDrop=600, gappedMaxDiagonals=64))):
        ao = api.anchor_options(gappedExtension=1, **kw)
        got, _ = _find(dict(case, trim=trim), anchor_options=ao)
        for (sx, sy), chains in zip(case["problems"], got):
            runs = api.find_anchor_runs_once(sx, sy, trim=trim, expansion=20, softMask=True, params=_params(case), options=ao)
            assert len(chains) == 1 and np.array_equal(chains[0]["runs"], runs), (trim, kw)
            assert len(runs) > chains[0]["nHsps"] or trim


def test_the_option_off_is_the_entry_point_of_before():
    """gappedExtension = 0 through the new entry point, and the old entry point itself: step 7, integer for integer."""
    case = gc.by_name("off")
    assert case["gapped"] == 0
    through, st1 = _find(case)
    before, st2 = _find(case, gapped=False)
    want = gc.model(case)
    for i in range(len(want)):
        _same((through[i], st1[i]), want[i], ("off", i))
        _same((before[i], st2[i]), want[i], ("before", i))
    # and the keyword alone means the extension at its defaults
    on = gc.by_name("inversion")
    alone, _ = local.find_local_chains(on["problems"], trim=0, params=_params(on), strand="both", gapped=True,
                                       options=local.local_options(maxChains=on["K"]))
    assert all(lm.same(g, w) for g, w in zip(alone[0], gc.model(on)[0][0])) and len(alone[0]) >= 2


def test_batch_equals_one_at_a_time_and_the_model():
    case = gc.batch_case()
    got, stats = _find(case)
    assert len(got) == 300
    want = gc.model(case)
    for i, pr in enumerate(case["problems"]):
        _same((got[i], stats[i]), want[i], ("batch", i))
        alone, alone_stats = _find(case, problems=[pr])     # a list of one problem lays its gaps and rows out from 0
        _same((alone[0], alone_stats[0]), want[i], ("alone", i))
    assert got[17] == [] and got[101] == []
    assert any(len(c["runs"]) == 0 for chains in got for c in chains)


# ---- a round over the scratch budget ----
SLICED_TEMPLATES, SLICED_REPEATS = 4, 140


def sliced_template(t):
    """Flanks of 2 kb around an inverted pair of segments: the outward extensions of the first chain have the full 4096 rows
    each, so a few hundred such problems pass the budget in round 1."""
    rng = random.Random(100 + t)
    a, b = lc.rand_seq(rng, 300), lc.rand_seq(rng, 300)
    u = [lc.rand_seq(rng, 2000 + 10 * t) for _ in range(4)]
    return u[0] + a + b + u[1], u[2] + gc.mutate(rng, a) + lc.rc(gc.mutate(rng, b)) + u[3]


def test_a_round_of_two_launches_equals_the_model_and_the_unsliced_call():
    case = gc._case("sliced", [sliced_template(t) for t in range(SLICED_TEMPLATES)], strand="both", K=2)
    want = [gc.model_of(case, sx, sy) for sx, sy in case["problems"]]       # once per template
    unsliced, ustats = _find(case)
    rows = []
    for i, ((sx, sy), (wchains, _)) in enumerate(zip(case["problems"], want)):
        _same((unsliced[i], ustats[i]), want[i], ("unsliced", i))
        assert len(wchains) == 2 and {c["strand"] for c in wchains} == {"plus", "minus"}
        rows.append(amg.gap_rows([h[:3] for h in wchains[0]["hsps"]], len(sx), len(sy)))
    first_round = SLICED_REPEATS * sum(rows)
    assert BUDGET_ROWS < first_round < 2 * BUDGET_ROWS                       # round 1 takes two launches, no more
    assert sum(rows) < BUDGET_ROWS
    problems = case["problems"] * SLICED_REPEATS
    got, stats = _find(case, problems=problems)
    for i in range(len(problems)):
        _same((got[i], stats[i]), want[i % SLICED_TEMPLATES], ("sliced", i))
