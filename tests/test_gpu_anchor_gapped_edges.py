"""The gapped extension (cpk_anchor_chain_untrimmed, cpk_anchor_gapped, cpk_anchor_assemble
and the host's sliced launches) on the GPU against its definition (tests/anchor_model_gapped.py), runs and statistics
integer for integer, on the inputs of tests/anchor_gapped_edge_cases.py: both band edges, N and lower case inside a gap,
long gaps under every option with the two ties, capped chains, passes without scratch rows, and one pass of 280 problems
that takes three launches over the scratch.  What each input is for is asserted in tests/test_anchor_gapped_edges_cpu.py."""
import functools

import numpy as np
import pytest

import anchor_cases as ac
import anchor_gapped_edge_cases as ec
import anchor_model as am
import anchor_model_gapped as ag
import test_gpu_anchor_gapped as base
from cpecan_amd import api

pytestmark = pytest.mark.gpu

COUNTS = base.COUNTS
assert len(COUNTS) == 9


def _options(**kw):
    return api.anchor_options(gappedExtension=1, **kw)


def _same(got_runs, got_stats, want_runs, want_stats, what):
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, what


def _once_equals_the_model(pair, what, softMasks=(True, False), **kw):
    sx, sy = pair
    for softMask in softMasks:
        got = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, softMask=softMask, options=_options(**kw))
        want, _ = ag.anchors_once(sx, sy, 14, softMask, am.default_params(), gapped=1, **kw)
        assert got.tolist() == [[x, y, n, 7] for x, y, n in want], (what, softMask)
    return want


# ---- 1. both band edges ----
@pytest.mark.parametrize("case", sorted(ec.BAND))
def test_both_band_edges_equal_the_model(case):
    want = _once_equals_the_model(ec.BAND[case], case)
    assert len(want) == (1 if "32" in case else 2)


# ---- 2. N and lower case inside a gap ----
@pytest.mark.parametrize("case", sorted(ec.MASKED))
def test_n_and_lower_case_inside_a_gap_equal_the_model(case):
    want = _once_equals_the_model(ec.MASKED[case], case)
    assert len(want) == 2
    sx, sy = ec.MASKED[case]
    plain = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7)
    assert plain.tolist() == [[x, y, n, 7] for x, y, n in ag.anchors_once(sx, sy, 14, True, am.default_params())[0]] and len(plain) == 1


# ---- 3. the long gaps ----
@pytest.mark.parametrize("option", sorted(ec.LONG_OPTIONS))
@pytest.mark.parametrize("pair", ["long_gap", "limit_gap"])
def test_a_long_gap_equals_the_model_under_every_option(pair, option):
    sx, sy = getattr(ec, pair)()
    kw = ec.LONG_OPTIONS[option]
    _once_equals_the_model((sx, sy), (pair, option), softMasks=(True,), **kw)
    got, st = api.find_anchor_runs(sx, sy, options=_options(**kw))
    want, wst = ag.find_anchor_runs(sx, sy, gapped=1, **kw)
    _same(got, st, want, wst, (pair, option))


@pytest.mark.parametrize("pair", ["tie_gap", "source_tie_gap"])
def test_the_ties_go_the_models_way(pair):
    for option, kw in ec.LONG_OPTIONS.items():
        _once_equals_the_model(getattr(ec, pair)(), (pair, option), **kw)


# ---- 4. a capped chain ----
@pytest.mark.parametrize("maxHsps", [5, 1])
def test_a_capped_chain_equals_the_model(maxHsps):
    sx, sy = ac.random_pair(2, 3000)
    got, st = api.find_anchor_runs(sx, sy, params=api.anchor_params_default(maxHsps=maxHsps), options=_options())
    want, wst = ag.find_anchor_runs(sx, sy, params=am.default_params(maxHsps=maxHsps), gapped=1)
    _same(got, st, want, wst, maxHsps)
    assert st["capped"] == 1 and st["runs"] > 30
    once = api.find_anchor_runs_once(sx, sy, trim=14, expansion=7, params=api.anchor_params_default(maxHsps=maxHsps), options=_options())
    want_once, counts = ag.anchors_once(sx, sy, 14, True, am.default_params(maxHsps=maxHsps), gapped=1)
    assert once.tolist() == [[x, y, n, 7] for x, y, n in want_once] and counts["chained"] == maxHsps


# ---- 5. passes without rows ----
@functools.lru_cache(maxsize=None)
def _zero_model():
    return tuple(ag.find_anchor_runs(sx, sy, gapped=1) for sx, sy in ec.zero_row_problems().values())


def test_a_batch_without_rows_equals_the_model():
    problems = list(ec.zero_row_problems().values())
    runs, stats = api.find_anchor_runs_many(problems, options=_options())
    for i, (want, wst) in enumerate(_zero_model()):
        _same(runs[i], stats[i], want, wst, i)
    assert sum(st["runs"] for st in stats) == 1 and sum(st["subProblems"] for st in stats) == 4
    for i, (sx, sy) in enumerate(problems):                                 # and alone: a pass of one problem, no rows at all
        got, st = api.find_anchor_runs(sx, sy, options=_options())
        _same(got, st, _zero_model()[i][0], _zero_model()[i][1], i)


def test_zero_row_problems_between_others_equal_the_model():
    zero, six = list(ec.zero_row_problems().values()), list(base._batch())
    problems, want = [], []
    for i in range(6):
        problems.append(six[i])
        want.append(base._batch_model(**base.ON)[i])
        if i < len(zero):
            problems.append(zero[i])
            want.append(_zero_model()[i])
    runs, stats = api.find_anchor_runs_many(problems, options=_options())
    for i in range(len(problems)):
        _same(runs[i], stats[i], want[i][0], want[i][1], i)
    both_runs, both_stats, strands = api.find_anchor_runs_many_stranded(problems, strand="both", options=_options())
    plus = [i for i in range(len(problems)) if strands[i]["strand"] == "plus"]
    assert len(plus) >= 9                                                   # the six related pairs and what cannot win on minus
    for i in plus:
        _same(both_runs[i], both_stats[i], want[i][0], want[i][1], i)


# ---- 6. a pass over the scratch budget ----
@functools.lru_cache(maxsize=None)
def _template_model(t):
    sx, sy = ec.sliced_template(t)
    return ag.find_anchor_runs(sx, sy, gapped=1)


def test_a_pass_of_three_launches_equals_the_model_and_the_unsliced_call():
    """35 rounds of the eight templates: 8.67 M scratch rows against the 4 Mi of one launch (ec.BUDGET_ROWS, which states
    CPK_ANCHOR_GAPPED_BUDGET_ROWS of cpecan_internal.h), so the top-level pass takes three launches, of which the first
    ends inside a problem (tests/test_anchor_gapped_edges_cpu.py)."""
    templates = [ec.sliced_template(t) for t in range(ec.SLICED_TEMPLATES)]
    runs, stats = api.find_anchor_runs_many(templates, options=_options())   # one launch
    for t in range(ec.SLICED_TEMPLATES):
        _same(runs[t], stats[t], _template_model(t)[0], _template_model(t)[1], t)
        assert stats[t]["runs"] == 9 and stats[t]["subProblems"] == 4
    slots = ec.sliced_slots()
    runs, stats = api.find_anchor_runs_many([templates[t] for t in slots], options=_options())
    assert len(runs) == 280
    for i, t in enumerate(slots):
        _same(runs[i], stats[i], _template_model(t)[0], _template_model(t)[1], (i, t))
