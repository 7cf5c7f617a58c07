"""The expectation emitter (CPECAN_EMIT_EXPECT: the Baum-Welch counts of diagonalCalculationExpectations,
pairwiseAligner.c:735-746; Batch(..., emit=EMIT_EXPECT), expectations(hmm, slot)) against the CPU oracle on every build
that forms the events -- inside the traceback for one and for two 64-lane groups per diagonal, the second pass over
parked B values with rows in LDS and in global memory, the team kernel of four and of eight waves, the packed kernel in
groups of 8, 16 and 32 lanes, and the SLOTS build of each.

A batch pools its counts into one accumulator, so every comparison with the oracle here is of ONE problem, run as a batch
of its own, element by element: |got - want| <= 1e-5 |want| + 1e-12 and 1e-9 relative on the likelihood (DESIGN's gate
for fp32 events; a dropped or doubled event of posterior above ~1e-4 fails it), and exactly 0.0 where the oracle has
exactly 0.  One GPU form against another: rtol 1e-6, atol 1e-12, likelihood 1e-11 (tools/soak_emitters.py: fp32 sums added
in another order).  Every helper prints the largest relative difference it saw -- a record, not a gate.
tests/test_expect_cases_cpu.py holds the preconditions; the inputs are tests/expect_cases.py's."""
import os
import re
import sys

import numpy as np
import pytest

import expect_cases as ec
from cpecan_amd import api
from test_gpu_forward import DEGENERATE, GLOBAL_MARK

pytestmark = pytest.mark.gpu

ONE_WAVE, TEAM, IN_TRACEBACK = "one wave per region", "a team of waves per region", "expectation events inside the traceback"
KNOBS = ("CPECAN_TEAM", "CPECAN_PACKED", "CPECAN_EXP_INSWEEP", "CPECAN_EXP_ONE_GROUP")
FLOOR = 1e-6  # counts below this are left out of the printed relative differences (the gates cover them through atol)


def _counts(h):
    S = h.stateNumber
    return ec.Counts(np.array(h.transitions[:S * S]), np.array(h.emissions[:S * 16]), float(h.likelihood))


def _run(case, problems=None, models=None):
    """One EMIT_EXPECT batch of the case's problems (or of `problems`): the counts it adds to an empty HMM -- with
    `models`, reserved slots and one run: the counts of every slot."""
    sm, mtype = ec.model_pair(case.model)[0], ec.model_type(case.model)
    p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
    with api.Batch(sm, p, emit=api.EMIT_EXPECT) as b:
        if models:
            b.reserve_models(len(models))
        b.add_many(case.problems if problems is None else problems)
        b.upload()
        if models:
            b.set_models(models)
        b.run()
        b.download()
        out = [_counts(b.expectations(api.hmm_constructEmpty(0.0, mtype), k)) for k in range(len(models) if models else 1)]
        return out if models else out[0]


def _wide_lines(err):
    return re.findall(r"^cpecan class \d+:.*$", err, re.M)


def _packed_lines(err):
    return re.findall(r"^cpecan packed class \d+:.*$", err, re.M)


def _traced(capfd, run, *args, **kw):
    """run(...) and the class lines CPECAN_TRACE_HOST wrote meanwhile; what the test has printed so far is put back."""
    printed = capfd.readouterr().out
    got = run(*args, **kw)
    err = capfd.readouterr().err
    sys.stdout.write(printed)
    return got, _wide_lines(err) + _packed_lines(err)


_singles = {}


def _alone(case, capfd, env=()):
    """Every problem of the case as a batch of one under the knobs `env`: ([Counts], [class lines]) per problem.  Run once
    per process and setting: several tests compare the same singletons."""
    key = (case.name, tuple(sorted(dict(env).items())))
    if key not in _singles:
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(dict(env))
        try:
            out = [_traced(capfd, _run, case, [pr]) for pr in case.problems]
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update({k: v for k, v in saved.items() if v is not None})
        _singles[key] = ([c for c, _ in out], [lines for _, lines in out])
    return _singles[key]


def _rel(got, want):
    big = np.abs(want) >= FLOOR
    return float((np.abs(got - want)[big] / np.abs(want)[big]).max()) if big.any() else 0.0


def _report(what, pairs):
    t, e, l = (max([f(g, w) for g, w in pairs] or [0.0]) for f in (
        lambda g, w: _rel(g.T, w.T), lambda g, w: _rel(g.E, w.E),
        lambda g, w: abs(g.likelihood - w.likelihood) / abs(w.likelihood) if w.likelihood else 0.0))
    print("%s: %d comparisons, largest relative difference T %.3g E %.3g likelihood %.3g" % (what, len(pairs), t, e, l))


def _close(got, want, rtol, atol, lrtol, what):
    for name, g, w in (("T", got.T, want.T), ("E", got.E, want.E)):
        bad = np.nonzero(~(np.abs(g - w) <= rtol * np.abs(w) + atol))[0]
        assert len(bad) == 0, "%s: %s[%d] is %.17g, expected %.17g (relative %.3g)" % (
            what, name, bad[0], g[bad[0]], w[bad[0]], abs(g[bad[0]] - w[bad[0]]) / abs(w[bad[0]]) if w[bad[0]] else np.inf)
    assert abs(got.likelihood - want.likelihood) <= lrtol * abs(want.likelihood), "%s: likelihood %.17g, expected %.17g" % (
        what, got.likelihood, want.likelihood)


def _assert_oracle(what, gots, wants):
    """GPU against oracle, one pair of Counts per problem: the gate per element, and exactly 0.0 where the oracle has 0."""
    gots, wants = list(gots), list(wants)
    assert len(gots) == len(wants)
    _report(what + " against the oracle", list(zip(gots, wants)))
    for i, (g, w) in enumerate(zip(gots, wants)):
        _close(g, w, ec.ORACLE_RTOL, ec.ORACLE_ATOL, ec.ORACLE_LIKELIHOOD_RTOL, "%s, problem %d" % (what, i))
        for name, gv, wv in (("T", g.T, w.T), ("E", g.E, w.E)):
            stray = np.nonzero((wv == 0.0) & (gv != 0.0))[0]
            assert len(stray) == 0, "%s, problem %d: %s[%d] is %g where the oracle has exactly 0" % (what, i, name, stray[0], gv[stray[0]])
        assert w.likelihood != 0.0 or g.likelihood == 0.0, (what, i)


def _assert_forms(what, gots, others):
    """One GPU form against another: the same fp32 events, added in another order."""
    gots, others = list(gots), list(others)
    assert len(gots) == len(others)
    _report(what, list(zip(gots, others)))
    for i, (g, o) in enumerate(zip(gots, others)):
        _close(g, o, ec.FORM_RTOL, ec.FORM_ATOL, ec.FORM_LIKELIHOOD_RTOL, "%s, problem %d" % (what, i))


def _widest(lines):
    return max(int(re.search(r"widest diagonal (\d+),", line).group(1)) for line in lines)


@pytest.fixture
def trace(monkeypatch):
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


# ---- 1. every problem alone ----
@pytest.mark.parametrize("model", ec.MODELS)
def test_each_problem_alone_matches_the_oracle(model, trace, capfd):
    """Every problem of the widths case -- and, for the two edge models, of the edges case: 1 x 1 ... 130 x 40 under the four
    ragged combinations, the degenerate problems -- as a batch of one, by the library's own choice of build: one wave per
    region, the widest diagonal the one the problem is named for."""
    case = ec.widths_case(model)
    got, lines = _alone(case, capfd)
    for (kind, w), ls in zip(ec.widths_layout(model), lines):
        assert len(ls) == 1 and ONE_WAVE in ls[0] and ": 1 regions," in ls[0] and GLOBAL_MARK not in ls[0], ls
        assert kind == "banded" or _widest(ls) == w, (kind, w, ls)
    _assert_oracle(case.name, got, ec.oracle_counts(case))
    if model in ec.EDGE_MODELS:
        case = ec.edges_case(model)
        got, lines = _alone(case, capfd)
        for (sx, sy, _, _, _), g, ls in zip(case.problems, got, lines):
            assert all(ONE_WAVE in l for l in ls) and len(ls) <= 1, ls
            if (sx, sy) == DEGENERATE[0]:
                assert not g.T.any() and not g.E.any() and g.likelihood == 0.0
            elif not sx or not sy:
                assert not g.E.any() and g.T.sum() > 0  # (row or column 0 reads as N: transitions only)
        _assert_oracle(case.name, got, ec.oracle_counts(case))


# ---- 2. the in-traceback builds and the second pass ----
SETTINGS = (("in the traceback", {"CPECAN_EXP_INSWEEP": "2"}), ("in the traceback, the build for two groups", {"CPECAN_EXP_INSWEEP": "2", "CPECAN_EXP_ONE_GROUP": "0"}),
            ("second pass", {"CPECAN_EXP_INSWEEP": "0"}))


@pytest.mark.parametrize("model", ec.MODELS)
def test_in_traceback_builds_and_second_pass(model, trace, capfd):
    """The widths problems alone with the events inside the traceback wherever they can be (CPECAN_EXP_INSWEEP=2: the build
    for one group per diagonal up to 64 cells, for two up to 128), with the build for two groups at every width
    (CPECAN_EXP_ONE_GROUP=0) and with the second pass everywhere (CPECAN_EXP_INSWEEP=0): each against the oracle, and
    against one another.  (The class line reads the same for both in-traceback builds: that CPECAN_EXP_ONE_GROUP=0 swapped
    the build is not visible here, only that the setting's counts are right; the two builds add the same events in the same
    order, so their counts are equal as well.)"""
    case = ec.widths_case(model)
    runs = {}
    for name, env in SETTINGS:
        got, lines = _alone(case, capfd, env)
        for ls in lines:
            assert len(ls) == 1 and ONE_WAVE in ls[0], ls
            assert (IN_TRACEBACK in ls[0]) == (name != "second pass" and _widest(ls) <= 128), (name, ls)
        _assert_oracle("%s, %s" % (case.name, name), got, ec.oracle_counts(case))
        runs[name] = got
    names = [name for name, _ in SETTINGS]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            _assert_forms("%s, %s against %s" % (case.name, a, b), runs[a], runs[b])


# ---- 3. the library's own choice where the in-traceback form costs a resident wave ----
def test_the_librarys_own_choice_at_the_lds_edge(trace, capfd):
    """No knob set: 74 cells of five states and 121 of three (against a Y of 1900 bases) still form their events inside the
    traceback, 75 and 122 take the second pass (cpk_plan.inl, plan_expect_in_sweep: the three forward diagonals in LDS
    must not cost a resident wave)."""
    for model in ec.MODELS:
        case = ec.widths_case(model)
        got, lines = _alone(case, capfd)
        narrow, wide = ec.widths_indices(model, "lds-edge")
        last = ec.LAST_IN_TRACEBACK_WIDTH[ec.states(model)]
        assert _widest(lines[narrow]) == last and IN_TRACEBACK in lines[narrow][0], lines[narrow]
        assert _widest(lines[wide]) == last + 1 and IN_TRACEBACK not in lines[wide][0] and ONE_WAVE in lines[wide][0], lines[wide]
        want = ec.oracle_counts(case)
        _assert_oracle("%s, %d and %d cells" % (case.name, last, last + 1), [got[narrow], got[wide]], [want[narrow], want[wide]])


# ---- 4. N and lower case ----
@pytest.mark.parametrize("model", ec.ASYMMETRIC)
def test_n_and_lower_case(model, trace, capfd):
    """The reference counts an event at a cell with an N in the transition counts and not in the emission counts
    (cell_expectation: cX < SYM_N && cY < SYM_N): pairs with a fifth of their bases N or lower case, where those events
    are 10-27 % of all, per problem, inside the traceback and by the second pass."""
    case = ec.n_rich_case(model)
    want = ec.oracle_counts(case)
    for name, env in (("own choice", {}), ("second pass", {"CPECAN_EXP_INSWEEP": "0"})):
        got, lines = _alone(case, capfd, env)
        flat = [l for ls in lines for l in ls]
        assert len(flat) == len(case.problems) and all(ONE_WAVE in l for l in flat), flat
        assert any(IN_TRACEBACK in l for l in flat) == (name == "own choice") and not all(IN_TRACEBACK in l for l in flat), flat
        _assert_oracle("%s, %s" % (case.name, name), got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            left_out, expected = g.T.sum() - g.E.sum(), w.T.sum() - w.E.sum()
            assert expected >= ec.N_RICH_MIN_SHARE * w.T.sum()
            assert abs(left_out - expected) <= ec.ORACLE_RTOL * expected + ec.ORACLE_ATOL, (name, i, left_out, expected)
            for k in ec.absent_transitions(model):
                assert g.T[k] == 0.0, (name, i, k)


# ---- 5. the packed kernel's three group widths ----
@pytest.mark.parametrize("model", ec.ASYMMETRIC)
def test_packed_groups(model, trace, capfd):
    """Each packed batch under CPECAN_PACKED=2, pooled: against the pooled oracle, and against the sum of the same problems
    run alone on the sweep kernel (CPECAN_PACKED=0) at the form-against-form tolerance -- the check that sees a count
    booked to a neighbouring region of a group, or lost with a region that shares its wave."""
    for lanes, case in ec.packed_cases(model):
        trace.setenv("CPECAN_PACKED", "2")
        packed, lines = _traced(capfd, _run, case)
        trace.delenv("CPECAN_PACKED")
        for line in lines:
            print(line)
        assert any("in groups of %d lanes" % lanes in l for l in lines), lines
        _assert_oracle("%s in groups of %d lanes, pooled" % (case.name, lanes), [packed], [ec.pooled(ec.oracle_counts(case))])
        alone, alone_lines = _alone(case, capfd, {"CPECAN_PACKED": "0"})
        assert all(ONE_WAVE in l and "packed" not in l for ls in alone_lines for l in ls), alone_lines
        _assert_oracle("%s alone on the sweep kernel" % case.name, alone, ec.oracle_counts(case))
        _assert_forms("%s packed against the sum of its problems alone" % case.name, [packed], [ec.pooled(alone)])


# ---- 6. the team kernel ----
@pytest.mark.parametrize("model", ec.ASYMMETRIC)
def test_team_of_four_and_eight(model, trace, capfd):
    """The team's second pass with four waves (501 and 509 cells; CPECAN_TEAM=500 for three states, which would keep one wave
    per region), with eight (901 cells of five states), and on two multi-segment bands with short traceback schedules
    (CPECAN_TEAM=100): per problem against the oracle and against one wave per region (CPECAN_TEAM=0) --
    which for 901 cells of five states is the second pass with its rows in global memory."""
    for words, team, case in ec.team_cases(model):
        teamed, lines = _alone(case, capfd, {"CPECAN_TEAM": team} if team else {})
        for ls in lines:
            assert any(TEAM in l and words in l for l in ls) and (team == "100" or len(ls) == 1), ls
            assert not any(IN_TRACEBACK in l for l in ls if TEAM in l), ls
        solo, lines = _alone(case, capfd, {"CPECAN_TEAM": "0"})
        for ls in lines:
            assert ls and all(ONE_WAVE in l for l in ls), ls
            assert all((GLOBAL_MARK in l) == (words == "(eight)") for l in ls), ls
        want = ec.oracle_counts(case)
        _assert_oracle("%s on the team" % case.name, teamed, want)
        _assert_oracle("%s with one wave per region" % case.name, solo, want)
        _assert_forms("%s, the team against one wave per region" % case.name, teamed, solo)


# ---- 7. the second pass with rows in global memory ----
@pytest.mark.parametrize("model", ec.GLOBAL_MODELS)
def test_rows_in_global_memory(model, trace, capfd):
    """CPECAN_TEAM=0 around the 64 KB edge of one wave's LDS (cpk_plan.inl, set_row_form: an expectation class keeps four
    copies of its 80 emission sums in the header and stages no candidates): the last width that fits keeps its rows in
    LDS -- the trace line gives the computed size --, the first that does not says "rolling rows in global memory".  Both
    against the oracle and against the library's own choice, a team of waves."""
    S = ec.states(model)
    for n, in_global, case in ec.global_cases(model):
        solo, lines = _alone(case, capfd, {"CPECAN_TEAM": "0"})
        ls = lines[0]
        assert len(ls) == 1 and re.search(r": 1 regions, widest diagonal %d,.*%s" % (n + 1, ONE_WAVE), ls[0]), ls
        assert (GLOBAL_MARK in ls[0]) == in_global and IN_TRACEBACK not in ls[0], ls
        if not in_global:
            assert "LDS %d B" % ec.expect_wave_lds_bytes(S, n, n) in ls[0], ls
        own, lines = _alone(case, capfd)
        assert len(lines[0]) == 1, lines
        print(lines[0][0])
        want = ec.oracle_counts(case)
        _assert_oracle("%s with one wave per region" % case.name, solo, want)
        _assert_oracle("%s by the library's own choice" % case.name, own, want)
        _assert_forms("%s, one wave per region against the library's own choice" % case.name, solo, own)


# ---- 8. slots against the oracle ----
@pytest.mark.parametrize("form", ec.SLOT_FORMS)
def test_slots_match_the_oracle_under_each_model(form, trace, capfd):
    """reserve_models(3), set_models, one run: expectations(acc, slot=k) is the oracle's pooled count of the batch under
    model k -- not another GPU run's --, for three random models of five and of three states on each form of launch."""
    for S in ec.SLOT_TYPES:
        env, words, cases = ec.slots_case(form, S)
        for k, v in env.items():
            trace.setenv(k, v)
        got, lines = _traced(capfd, _run, cases[0], models=[ec.model_pair(c.model)[0] for c in cases])
        for k in env:
            trace.delenv(k)
        assert any(re.search(words, l) for l in lines), "the %s form did not run: %s" % (form, lines)
        assert len(got) == 3
        _assert_oracle("%s, %d states, slots 0-2, pooled" % (form, S), got, [ec.pooled(ec.oracle_counts(c)) for c in cases])
        for a in range(3):
            for b in range(a + 1, 3):
                assert _rel(got[a].T, got[b].T) > 1e-2 and got[a].likelihood != got[b].likelihood, (a, b)


# ---- 9. the caller's accumulator ----
def test_counts_add_into_the_callers_hmm(trace, capfd):
    """expectations() adds: into an HMM built with pseudo-count 0.5 that already holds another batch's counts the result is
    prior + this batch, element by element with the likelihood -- the very doubles, so equality -- and a second call on the
    same downloaded batch adds the same amounts again."""
    model = "fiveStateAsymmetric"
    first, second = ec.n_rich_case(model), ec.packed_cases(model)[1][1]
    sm, mtype = ec.model_pair(model)[0], ec.model_type(model)
    acc = api.hmm_constructEmpty(0.5, mtype)
    assert all(v == 0.5 for v in acc.transitions) and all(v == 0.5 for v in acc.emissions) and acc.likelihood == 0.0
    states = []
    for case in (first, second):
        with api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**case.pkw), emit=api.EMIT_EXPECT) as b:
            b.add_many(case.problems)
            b.upload()
            b.run()
            b.download()
            fresh = _counts(b.expectations(api.hmm_constructEmpty(0.0, mtype)))
            before = _counts(acc)
            for again in range(2 if case is second else 1):
                b.expectations(acc)
                after = _counts(acc)
                assert (after.T == before.T + fresh.T).all() and (after.E == before.E + fresh.E).all()
                assert after.likelihood == before.likelihood + fresh.likelihood and fresh.likelihood < 0.0
                before = after
            states.append(fresh)
    _assert_oracle("%s, pooled" % second.name, [states[1]], [ec.pooled(ec.oracle_counts(second))])
    total = _counts(acc)
    want = 0.5 + states[0].T + 2 * states[1].T
    assert np.abs(total.T - want).max() <= 1e-12 * want.max()


# ---- 10. batch order and size classes ----
def test_batch_order_and_size_classes(trace, capfd):
    """The widths problems of one model as one batch, in the given and in the reversed order: three size classes and more
    in one launch plan, and both equal to the sum of the singletons -- the counts of a region do not depend on what shares
    its launch."""
    model = "threeStateAsymmetric"
    case = ec.widths_case(model)
    alone, _ = _alone(case, capfd)
    total = ec.pooled(alone)
    for name, problems in (("given order", case.problems), ("reversed", case.problems[::-1])):
        got, lines = _traced(capfd, _run, case, list(problems))
        assert len(lines) >= 3 and all(ONE_WAVE in l for l in lines), lines
        assert sum(int(re.search(r": (\d+) regions", l).group(1)) for l in lines) == len(case.problems)
        _assert_forms("%s as one batch, %s, against the sum of its problems alone" % (case.name, name), [got], [total])
        _assert_oracle("%s as one batch, %s, pooled" % (case.name, name), [got], [ec.pooled(ec.oracle_counts(case))])
