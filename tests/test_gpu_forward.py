"""The forward-probability emitter (CPECAN_EMIT_FORWARD: computeForwardProbability, Batch(..., emit=EMIT_FORWARD),
forward_prob(i, slot)) against the CPU oracle on every path it takes: its own branch of the sweep kernel (start prior,
forwardStream / forward, end-prior dot product, the forwardOut store) and the host rules no other emitter has (a problem
is never split, the band is always the static one, results are read back through the device order).

Every comparison is per problem, GPU value against ob.forward_prob of the same input, through parity.assert_log_close
(LOG_TOL; equality under CPECAN_EXPECT_BIT_EXACT=1 with the exact library; -inf and 0.0 must be equal)."""
import functools
import random
import re

import numpy as np
import pytest

import oracle_binding as ob
from cpecan_amd import api, em
from cpecan_amd.workload import make_pair
from parity import assert_log_close
from test_gpu_parity import _evolve, _rand_seq, _sm

pytestmark = pytest.mark.gpu

TYPES = [api.fiveState, api.fiveStateAsymmetric, api.threeState, api.threeStateAsymmetric]
RAGGED = [(False, False), (True, False), (False, True), (True, True)]
GLOBAL_MARK = "rolling rows in global memory"  # cpk_plan.inl, plan_wide_class: the class runs the !FAST kernel


# ---- models: (library model, the oracle's copy from the same numbers) ----
@functools.lru_cache(maxsize=None)
def _model_pair(mtype):
    """The default model of the symmetric types; the asymmetric ones from a randomised, normalised HMM (as
    test_gpu_parity.test_hmm_loaded_models), so that X and Y gaps really differ."""
    if mtype in (api.fiveState, api.threeState):
        return _sm(mtype), ob.model(mtype)
    rng = random.Random(51 + mtype)
    ph, oh = api.hmm_constructEmpty(0.0, mtype), ob.hmm(mtype, 0.0)
    S = ph.stateNumber
    for i in range(S * S):
        ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
    for i in range(S * 16):
        ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
    api.hmm_normalise(ph)
    ob.lib().orc_hmm_normalise(oh)
    return api.hmm_getStateMachine(ph), ob.model_from_hmm(oh)


@functools.lru_cache(maxsize=None)
def _random_model_pair(mtype, seed):
    """tests/test_gpu_model_slots._random_model, and the oracle's model from the same HMM numbers."""
    h = em.hmm_randomise(api.hmm_constructEmpty(0.0, mtype), seed)
    em.hmm_set_jukes_cantor(h, 0.15)
    oh = ob.hmm(mtype, 0.0)
    for i in range(25):
        oh.T[i] = h.transitions[i]
    for i in range(80):
        oh.E[i] = h.emissions[i]
    return api.hmm_getStateMachine(h), ob.model_from_hmm(oh)


# ---- problems: (sX, sY, anchors, raggedLeft, raggedRight) ----
def _same_length_pair(rng, n):
    """Two related sequences of n and at least n bases: without anchors the widest diagonal has exactly n + 1 cells."""
    sx = _rand_seq(rng, n)
    sy = _evolve(rng, sx)
    return sx, sy + _rand_seq(rng, max(0, n - len(sy)))


def _diagonal_anchors(lX, lY, step, expansion):
    return [(i, i, expansion) for i in range(5, min(lX, lY) - 5, step)]


UNANCHORED = (1, 5, 63, 64, 65, 127, 128, 129, 200, 300)


@functools.lru_cache(maxsize=None)
def _mixed(E):
    """The mixed batch: unanchored pairs with diagonals just under, at and over one, two and several 64-lane groups;
    banded pairs whose anchors carry the expansion E; the per-anchor wide bands of test_random_wide_bands_stream_groups,
    whose expansions of 40-220 a forward batch must ignore; banded pairs with N and lower case.  All four ragged
    combinations go round the list.  Wide classes of <= 128, <= 192, <= 256 and <= 384 cells (cpecan_host.c,
    classify_regions), in an order that is not the device's (by class, then longest first)."""
    rng = random.Random(1000 + E)
    probs = []
    for n in UNANCHORED:
        sx, sy = _same_length_pair(rng, n)
        probs.append((sx, sy, ()))
    for i in range(4):
        probs.append(make_pair(11, i, 600, E))
    for _ in range(6):
        sx = _rand_seq(rng, rng.randrange(150, 520))
        sy = _evolve(rng, sx) or "ACGT"
        anchors, x, y = [], -1, -1
        while True:
            x += rng.randrange(5, 90)
            y += rng.randrange(5, 90)
            if x >= len(sx) or y >= len(sy):
                break
            anchors.append((x, y, 2 * rng.randrange(20, 110)))
        probs.append((sx, sy, anchors))
    for _ in range(4):
        sx = _rand_seq(rng, rng.randrange(200, 320))
        sy = _evolve(rng, sx) or "acgtn"
        probs.append((sx, sy, _diagonal_anchors(len(sx), len(sy), 29, E)))
    return tuple((sx, sy, a) + RAGGED[(i + i // 4) % 4] for i, (sx, sy, a) in enumerate(probs))


# the problems of the mixed batch that share the narrowest wide class at E = 40 (no diagonal over 128 cells)
NARROW = tuple(range(6)) + tuple(range(len(UNANCHORED), len(UNANCHORED) + 4)) + tuple(range(20, 24))


def _run_forward(sm, problems, reserve=0, models=None, **pkw):
    """One forward batch: ([slot][problem] log-probabilities, stats)."""
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    with api.Batch(sm, p, emit=api.EMIT_FORWARD) as b:
        if reserve:
            b.reserve_models(reserve)
        b.add_many(problems)
        b.upload()
        if models:
            b.set_models(models)
        b.run()
        b.download()
        slots = len(models) if models else 1
        return [[b.forward_prob(i, k) for i in range(len(problems))] for k in range(slots)], b.stats()


def _oracle(om, problems, **pkw):
    op = ob.params(**pkw)
    return [ob.forward_prob(om, sx, sy, a, op, rl, rr) for sx, sy, a, rl, rr in problems]


def _assert_all_close(got, want, what):
    assert len(got) == len(want)
    worst = max([abs(g - w) for g, w in zip(got, want) if np.isfinite(w) and np.isfinite(g)] or [0.0])
    print("%s: %d problems, largest difference %.3g" % (what, len(got), worst))
    for i, (g, w) in enumerate(zip(got, want)):
        assert not np.isnan(w), "%s, problem %d: the oracle has no band" % (what, i)
        assert_log_close(g, w, "%s, problem %d" % (what, i))


def _class_lines(err):
    return re.findall(r"^cpecan class \d+:.*$", err, re.M)


# ---- 1. models, ragged ends and widths on the LDS path ----
@pytest.mark.parametrize("E", [2, 10, 40, 100])
@pytest.mark.parametrize("mtype", TYPES)
def test_models_ragged_ends_and_widths_on_the_lds_path(mtype, E, monkeypatch, capfd):
    """The band of a forward batch is the static one: its width is the batch's diagonalExpansion, so the expansions
    {2, 10, 40, 100} are four batches per model type.  At least three wide classes per batch: forward_prob(i) has to
    undo the device order."""
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    sm, om = _model_pair(mtype)
    probs = _mixed(E)
    assert {p[3:] for p in probs} == set(RAGGED)
    text = [p[0] for p in probs if isinstance(p[0], str)]
    assert any("N" in s for s in text) and any(s != s.upper() for s in text)
    capfd.readouterr()
    got, st = _run_forward(sm, probs, diagonalExpansion=E, dynamicAnchorExpansion=0)
    classes = _class_lines(capfd.readouterr().err)
    assert len(classes) >= 3, classes
    assert not any(GLOBAL_MARK in c for c in classes), classes
    assert all("one wave per region" in c for c in classes), classes
    assert st.regions == st.problems == len(probs)
    want = _oracle(om, probs, diagonalExpansion=E)
    assert all(np.isfinite(w) for w in want)
    _assert_all_close(got[0], want, "type %d, expansion %d" % (mtype, E))


# ---- 2. the global-memory kernel ----
def _wave_lds_bytes(states, lX, lY):
    """cpk_plan.inl, set_row_form, for a forward class of one unanchored lX x lY pair: the header of 232 doubles (logAdd
    cubics, emissions, transition weights; no candidate stage), 2 S + 1 rolling rows of maxWidth + 1 doubles, and both
    strings at two symbols a byte."""
    width = min(lX, lY) + 1
    return 8 * (232 + (2 * states + 1) * (width + 1)) + ((lX + 3) // 2 + (lY + 3) // 2 + 15) // 16 * 16


@pytest.mark.parametrize("mtype,length", [(api.fiveState, 700), (api.fiveState, 714), (api.threeState, 1000), (api.threeState, 1115)])
def test_the_global_memory_kernel(mtype, length, monkeypatch, capfd):
    """A class keeps its rolling rows in global memory (the !FAST build: forward() + roll_fence) when one wave's LDS plus
    16 bytes is over 64 KB.  A forward class stages no candidates, so 701 cells of five states (64336 B) and 1001 of
    three (58976 B) still fit: they stay as the widest LDS classes, and the trace line must NOT carry the mark.  715
    cells of five states (65584 B) and 1116 of three (65528 B) are the first that do not fit, and must carry it.  A few
    100-base pairs stand in front, so the wide class is not the only one.  CPECAN_TEAM=100: this emitter has no team
    kernel, the knob changes nothing."""
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    sm, om = _model_pair(mtype)
    rng = random.Random(200 + mtype)
    base = [_same_length_pair(rng, 100) + ((),) for _ in range(3)]
    sx, sy, _ = make_pair(40 + mtype, 0, length, 0)
    sy = (sy + b"A" * length)[:length]  # `length` bases each: the widest diagonal has length + 1 cells
    base.append((sx, sy, ()))
    lds = _wave_lds_bytes(5 if mtype == api.fiveState else 3, length, length)
    in_global = lds + 16 > 64 * 1024
    assert in_global == (length in (714, 1115)), lds
    runs = {}
    for ragged, team in (((True, False), None), ((False, True), None), ((False, True), "100")):
        if team:
            monkeypatch.setenv("CPECAN_TEAM", team)
        probs = [pr + ragged for pr in base]
        capfd.readouterr()
        got, st = _run_forward(sm, probs)
        classes = _class_lines(capfd.readouterr().err)
        assert len(classes) == 2, classes
        wide = [c for c in classes if re.search(r": 1 regions, widest diagonal %d,.*one wave per region" % (length + 1), c)]
        assert len(wide) == 1 and (GLOBAL_MARK in wide[0]) == in_global, classes
        assert sum(GLOBAL_MARK in c for c in classes) == in_global, classes
        if not in_global:
            assert "LDS %d B" % lds in wide[0], (lds, classes)
        assert st.regions == st.problems == len(probs)
        if team:
            assert got[0] == runs[ragged], "CPECAN_TEAM changed a forward batch"
            continue
        runs[ragged] = got[0]
        _assert_all_close(got[0], _oracle(om, probs), "type %d, %d bases, ragged %s" % (mtype, length, ragged))


# ---- 3. a problem is never split ----
@functools.lru_cache(maxsize=None)
def _split_prone():
    rng = random.Random(41)
    probs = []
    for _ in range(12):
        sx = _rand_seq(rng, rng.randrange(300, 500))
        sy = _evolve(rng, sx)
        probs.append((sx, sy, _diagonal_anchors(len(sx), len(sy), 29, 4), True, True))
    return tuple(probs)


def test_a_problem_is_never_split():
    """cPecanRealign-style inputs (sparse anchors every 29 columns, splitMatrixBiggerThanThis = 10, ragged ends) that
    every list emitter cuts into several rectangles: computeForwardProbability never splits
    (pairwiseAligner.c:936-949; cpecan_host.c, problem_rects)."""
    probs = _split_prone()
    pkw = dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10)
    for sx, sy, a, rl, rr in probs:  # the precondition, on the CPU: the other emitters do split every one of these
        assert len(ob.split_points(a, len(sx), len(sy), 10, rl, rr)) > 1
    sm, om = _model_pair(api.fiveState)
    got, st = _run_forward(sm, probs, **pkw)
    assert st.problems == len(probs) and st.regions == st.problems
    _assert_all_close(got[0], _oracle(om, probs, **pkw), "never split")


# ---- 4. always the static band ----
def _band_total(om, sx, sy, a, op, rl, rr):
    """The oracle's total probability on the last diagonal with the band its parameters ask for: what
    getForwardProbWithBanding would give if it took that band (the total the last traceback starts from)."""
    _, tr = ob.aligned_pairs_traced(om, sx, sy, a, op, rl, rr)
    return float(tr["total_used"][len(sx) + len(sy)])


@functools.lru_cache(maxsize=None)
def _diverged():
    """Ten pairs that have diverged twice over, with anchors of expansion 2 on the main diagonal; kept are those whose
    dynamic band differs from the static one of 40 AND loses probability mass a log-space gate sees."""
    rng = random.Random(93)
    om = ob.model(ob.FIVE_STATE)
    static, dynamic = ob.params(diagonalExpansion=40), ob.params(diagonalExpansion=40, dynamicAnchorExpansion=1)
    kept = []
    for i in range(10):
        sx = _rand_seq(rng, rng.randrange(150, 350))
        sy = _evolve(rng, _evolve(rng, sx))
        a = _diagonal_anchors(len(sx), len(sy), 29, 2)
        rl, rr = RAGGED[i % 4]
        if not a or ob.band(a, len(sx), len(sy), 40, dynamic=True) == ob.band(a, len(sx), len(sy), 40, dynamic=False):
            continue
        want = ob.forward_prob(om, sx, sy, a, dynamic, rl, rr)  # (ob.forward_prob forces the static band, as the reference)
        assert want == ob.forward_prob(om, sx, sy, a, static, rl, rr)
        narrow = _band_total(om, sx, sy, a, dynamic, rl, rr)
        if np.isfinite(want) and abs(narrow - want) > 1e-6:
            kept.append((sx, sy, a, rl, rr))
    return tuple(kept)


def test_the_band_is_always_the_static_one():
    """dynamicAnchorExpansion = 1 with anchors of expansion 2 under diagonalExpansion = 40: getForwardProbWithBanding
    builds its band with the static expansion all the same (pairwiseAligner.c:894; cpecan_host.c, hp->dynamic).  The
    preconditions hold for the oracle alone: the two bands differ, and the narrow one changes the total by more than
    1e-6 -- three orders over the gate -- so a kernel on the dynamic band fails."""
    probs = _diverged()
    assert len(probs) >= 8
    pkw = dict(diagonalExpansion=40, dynamicAnchorExpansion=1)
    sm, om = _model_pair(api.fiveState)
    want = _oracle(om, probs, **pkw)
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    single = [api.computeForwardProbability(sx, sy, a, p, sm, rl, rr) for sx, sy, a, rl, rr in probs]
    _assert_all_close(single, want, "computeForwardProbability")
    got, st = _run_forward(sm, probs, **pkw)
    assert st.regions == st.problems == len(probs)
    _assert_all_close(got[0], want, "batch")


# ---- 5. degenerate problems inside a batch ----
DEGENERATE = [("", ""), ("ACGT", ""), ("", "ACGTN"), ("A", "A"), ("N", "T"), ("ACGTACGT", "ACG")]


@pytest.mark.parametrize("mtype", [api.fiveState, api.threeState])
def test_degenerate_problems_inside_a_batch(mtype):
    sm, om = _model_pair(mtype)
    rng = random.Random(300 + mtype)
    ordinary = [make_pair(12, i, 150, 10) for i in range(4)] + [_same_length_pair(rng, 70) + ((),) for _ in range(4)]
    probs, empties = [], []
    for k, ragged in enumerate(RAGGED):
        for j, (sx, sy) in enumerate(DEGENERATE):
            if not sx and not sy:
                empties.append(len(probs))
            probs.append((sx, sy, ()) + ragged)
            if j % 3 == 2:
                probs.append(tuple(ordinary[2 * k + j // 3]) + ragged)
    got, st = _run_forward(sm, probs, diagonalExpansion=10)
    assert st.problems == len(probs) == 32
    assert len(empties) == 4
    for i in empties:
        assert got[0][i] == 0.0  # LOG_ONE for two empty sequences (pairwiseAligner.c:889-891)
    _assert_all_close(got[0], _oracle(om, probs, diagonalExpansion=10), "type %d" % mtype)


# ---- 6. slots against the oracle ----
@pytest.mark.parametrize("mtype", [api.fiveState, api.threeStateAsymmetric])
def test_slots_match_the_oracle(mtype):
    """forward_prob(i, k) of one slotted run is the oracle's value of problem i under model k, for the mixed batch."""
    pairs = [_random_model_pair(mtype, 11 + 7 * k) for k in range(3)]
    probs = _mixed(40)
    got, st = _run_forward(_model_pair(mtype)[0], probs, reserve=3, models=[sm for sm, _ in pairs], diagonalExpansion=40)
    assert st.regions == len(probs)
    for k, (_, om) in enumerate(pairs):
        _assert_all_close(got[k], _oracle(om, probs, diagonalExpansion=40), "type %d, slot %d" % (mtype, k))
    assert got[0] != got[1] and got[1] != got[2]


@pytest.mark.parametrize("mtype", [api.fiveState, api.threeStateAsymmetric])
def test_waves_that_cross_slots_match_the_oracle(mtype, monkeypatch):
    """One single-wave workgroup per CU and 24 copies of the mixed batch's narrow problems: more regions than the launch
    has waves, so every wave goes on from slot 0 into slots 1 and 2."""
    monkeypatch.setenv("CPECAN_MAX_WAVES_PER_CU", "1")
    pairs = [_random_model_pair(mtype, 11 + 7 * k) for k in range(3)]
    narrow = [_mixed(40)[i] for i in NARROW]
    copies = 24
    got, st = _run_forward(_model_pair(mtype)[0], narrow * copies, reserve=3, models=[sm for sm, _ in pairs], diagonalExpansion=40)
    print("regions", st.regions, "waves", st.wavesPerLaunch)
    assert st.regions == len(narrow) * copies and st.regions > st.wavesPerLaunch
    for k, (_, om) in enumerate(pairs):
        want = _oracle(om, narrow, diagonalExpansion=40)
        _assert_all_close(got[k], want * copies, "type %d, slot %d" % (mtype, k))


# ---- 7. the other emitters' total ----
def _single_region_problems():
    return [_mixed(40)[i] for i in (2, 4, 6, 8, 10, 12, 14, 17, 20, 23)]


@pytest.mark.parametrize("mtype", [api.fiveState, api.threeState])
def test_forward_prob_is_the_total_the_last_traceback_starts_from(mtype):
    """The last traceback of getPosteriorProbsWithBanding starts on diagonal N with the end prior in B, and the total it
    uses there is the dot product computeForwardProbability returns.  The sweep kernel's debug buffer holds that total:
    ten single-region problems of every width class, GPU against GPU."""
    sm, _ = _model_pair(mtype)
    probs = _single_region_problems()
    pkw = dict(diagonalExpansion=40, dynamicAnchorExpansion=0)
    got, st = _run_forward(sm, probs, **pkw)
    assert st.regions == len(probs)
    p, op = api.pairwiseAlignmentBandingParameters_construct(**pkw), ob.params(**pkw)
    for i, (sx, sy, a, rl, rr) in enumerate(probs):
        N = len(sx) + len(sy)
        with api.Batch(sm, p, debug=True) as b:
            b.add(sx, sy, a, rl, rr)
            b.upload()
            b.run()
            b.download()
            assert b.stats().regions == 1
            _, tot = b.debug_fetch(0, ob.band_cells(sx, sy, a, op, rl, rr), N + 1)
        assert_log_close(got[0][i], float(tot[N]), "problem %d" % i)


@pytest.mark.parametrize("mtype", [api.fiveState, api.threeState])
def test_expectation_likelihood_is_forward_prob_once_per_diagonal(mtype):
    """diagonalCalculationExpectations adds the total to the HMM's likelihood once per emitted diagonal
    (pairwiseAligner.c:743), and the total is refreshed every tenth diagonal: with at most ten diagonals the one total
    of diagonal N serves them all, and the likelihood an EMIT_EXPECT batch of one problem adds to an empty HMM is
    N x forward_prob (tests/test_oracle_golden.py, test_survey_known_answers, has the property for the oracle)."""
    sm, _ = _model_pair(mtype)
    rng = random.Random(700 + mtype)
    probs = [("AGCG", "AGTTCG", (), False, False)]
    for i, (lx, ly) in enumerate([(1, 1), (5, 5), (3, 7), (7, 3), (2, 8), (9, 1), (4, 4), (6, 2), (6, 3)]):
        probs.append((_rand_seq(rng, lx), _rand_seq(rng, ly), ()) + RAGGED[i % 4])
    got, _ = _run_forward(sm, probs)
    p = api.pairwiseAlignmentBandingParameters_construct()
    for i, (sx, sy, a, rl, rr) in enumerate(probs):
        h = api.getExpectationsUsingAnchors(sm, api.hmm_constructEmpty(0.0, mtype), sx, sy, a, p, rl, rr)
        assert_log_close(h.likelihood, (len(sx) + len(sy)) * got[0][i], "problem %d" % i)


# ---- 8. set_model between runs ----
@pytest.mark.parametrize("mtype", [api.fiveState, api.threeStateAsymmetric])
def test_set_model_between_runs(mtype):
    first, second = _model_pair(mtype), _random_model_pair(mtype, 5)
    probs = _mixed(40)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=40)
    with api.Batch(first[0], p, emit=api.EMIT_FORWARD) as b:
        b.add_many(probs)
        b.upload()
        for round_, (sm, om) in enumerate((first, second)):
            if round_:
                b.set_model(sm)
            b.run()
            b.download()
            got = [b.forward_prob(i) for i in range(len(probs))]
            _assert_all_close(got, _oracle(om, probs, diagonalExpansion=40), "type %d, round %d" % (mtype, round_))
