"""Model slots on the GPU: K models over one resident batch in a single launch.  The check throughout: slot k of a slotted
run gives what cpecan_batch_set_model(model k) plus a run gives on the same resident batch -- expectation sums to
rtol 1e-9 / atol 1e-12 (the same sums added in another order), forward log-probabilities bit for bit."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from cpecan_amd import api, em
from cpecan_amd.realign import Cigar
from cpecan_amd.workload import make_pair, make_realign_batch

pytestmark = pytest.mark.gpu

TYPES = [api.fiveState, api.fiveStateAsymmetric, api.threeState, api.threeStateAsymmetric]


def _random_model(mtype, seed):
    h = em.hmm_randomise(api.hmm_constructEmpty(0.0, mtype), seed)
    em.hmm_set_jukes_cantor(h, 0.15)
    return api.hmm_getStateMachine(h)


def _default(mtype):
    return api.stateMachine5_construct(mtype) if mtype < 2 else api.stateMachine3_construct(mtype)


def _problems(n=12, length=400):
    return [make_pair(seed=5, index=i, length=length + 37 * i, expansion=10) for i in range(n)]


def _batch(sm, emit, problems, reserve=0, ragged=(False, False), **pkw):
    pkw.setdefault("diagonalExpansion", 10)
    b = api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**pkw), emit=emit)
    if reserve:
        b.reserve_models(reserve)
    b.add_many([tuple(p[:3]) + ragged for p in problems])
    b.upload()
    return b


def _expect(b, mtype, slot=0):
    return b.expectations(api.hmm_constructEmpty(0.0, mtype), slot)


def _assert_hmm_close(got, want):
    S = got.stateNumber
    print("max rel diff T %.3g E %.3g L %.3g" % (
        np.max(np.abs(np.array(got.transitions[:S * S]) - want.transitions[:S * S]) / (np.abs(want.transitions[:S * S]) + 1e-300)),
        np.max(np.abs(np.array(got.emissions[:S * 16]) - want.emissions[:S * 16]) / (np.abs(want.emissions[:S * 16]) + 1e-300)),
        abs(got.likelihood - want.likelihood) / abs(want.likelihood)))
    np.testing.assert_allclose(list(got.transitions), list(want.transitions), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(list(got.emissions), list(want.emissions), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got.likelihood, want.likelihood, rtol=1e-9, atol=1e-12)


def _slots_against_sequential(mtype, T, emit, problems, **kw):
    """One slotted run of T different models against T set_model + run rounds on the same resident batch."""
    models = [_random_model(mtype, 11 + 7 * k) for k in range(T)]
    n = len(problems)
    with _batch(_default(mtype), emit, problems, reserve=T, **kw) as b:
        b.set_models(models)
        b.run()
        b.download()
        stats = b.stats()
        if emit == api.EMIT_EXPECT:
            got = [_expect(b, mtype, k) for k in range(T)]
        else:
            got = [np.array([b.forward_prob(i, k) for i in range(n)]) for k in range(T)]
        for bad in (-1, T):
            with pytest.raises(api.CpecanError, match="slot"):
                _expect(b, mtype, bad) if emit == api.EMIT_EXPECT else b.forward_prob(0, bad)
        for k in range(T):
            b.set_model(models[k])
            b.run()
            b.download()
            if emit == api.EMIT_EXPECT:
                _assert_hmm_close(got[k], _expect(b, mtype))
                assert got[k].likelihood != 0.0
            else:
                np.testing.assert_array_equal(got[k], np.array([b.forward_prob(i) for i in range(n)]))
        if T > 1 and emit == api.EMIT_FORWARD:
            assert not np.array_equal(got[0], got[1])  # the models differ: so do the results
    return stats


@pytest.mark.parametrize("mtype", TYPES)
@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("emit", [api.EMIT_EXPECT, api.EMIT_FORWARD])
def test_slot_k_is_set_model_k_plus_a_run(mtype, T, emit):
    _slots_against_sequential(mtype, T, emit, _problems())


# (name, problems, parameters, ragged ends, environment, what CPECAN_TRACE_HOST's plan line must say)
FORMS = [
    ("wide", lambda: [make_pair(3, i, 2000, 100) for i in range(6)], dict(diagonalExpansion=100), {},
     r"cpecan class \d+: 6 regions.*one wave per region(?!.*inside the traceback)"),
    ("insweep_one_group", lambda: [make_pair(5, i, 1000, 10) for i in range(40)], dict(diagonalExpansion=10), {},
     r"cpecan class \d+: 40 regions.*one wave per region.*expectation events inside the traceback"),
    # (CPECAN_EXP_INSWEEP=2, as tests/test_gpu_parity.py pins this build: a five-state band of 94 cells otherwise takes the
    # second pass, its three forward diagonals in LDS would cost a resident wave)
    ("insweep_two_groups", lambda: [make_pair(7, i, 1000, 40) for i in range(20)], dict(diagonalExpansion=40),
     {"CPECAN_EXP_INSWEEP": "2"},
     r"cpecan class \d+: 20 regions, widest diagonal (6[5-9]|[7-9]\d|1[01]\d|12[0-8]),.*expectation events inside the traceback"),
    ("packed", lambda: make_realign_batch(4, 150, 100, 1200, 4), dict(diagonalExpansion=4, splitMatrixBiggerThanThis=100), {},
     r"cpecan packed class \d: \d+ regions in groups of \d+ lanes.*whole regions"),
    ("team", lambda: [make_pair(36, i, 500, 0)[:2] + ((),) for i in range(3)] + [make_pair(34, 0, 900, 0)[:2] + ((),)],
     # (CPECAN_TEAM=100, as tests/test_gpu_parity.py pins the team: a three-state class of this width keeps one wave per
     # region by the library's own choice)
     dict(diagonalExpansion=40), {"CPECAN_TEAM": "100"}, r"a team of waves per region"),
]


@pytest.mark.parametrize("mtype", [api.fiveState, api.threeStateAsymmetric])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_every_launch_form_of_an_expect_batch(form, mtype, monkeypatch, capfd):
    name, make, pkw, env, pattern = form
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    stats = _slots_against_sequential(mtype, 3, api.EMIT_EXPECT, make(), ragged=(True, name == "packed"), **pkw)
    err = capfd.readouterr().err
    assert re.search(pattern, err), "the %s form did not run:\n%s" % (name, err)
    assert stats.launchForm == 0  # CPECAN_FORM_WHOLE: no split form for this emitter


# Waves that CROSS slots with sums in hand: more regions than the launch has waves (CPECAN_MAX_WAVES_PER_CU=1 caps the
# single-wave workgroups; the team's workgroups are capped by its LDS), so every wave draws tickets of several slots and
# takes the flush / reset / refill path of the kernels between them.
# (name, problems, parameters, environment, plan line, regions per launched workgroup must exceed this)
CROSSING = [
    ("wide", lambda: [make_pair(3, i, 1000, 100) for i in range(300)], dict(diagonalExpansion=100), {},
     r"one wave per region(?!.*inside the traceback)", 1),
    ("insweep_one_group", lambda: [make_pair(5, i, 600, 10) for i in range(300)], dict(diagonalExpansion=10), {},
     r"one wave per region.*expectation events inside the traceback", 1),
    ("insweep_two_groups", lambda: [make_pair(7, i, 600, 40) for i in range(300)], dict(diagonalExpansion=40),
     {"CPECAN_EXP_INSWEEP": "2"}, r"widest diagonal (6[5-9]|[7-9]\d|1[01]\d|12[0-8]),.*expectation events inside the traceback", 1),
    ("packed", lambda: make_realign_batch(4, 4000, 100, 300, 4), dict(diagonalExpansion=4, splitMatrixBiggerThanThis=100), {},
     r"cpecan packed class \d: \d+ regions in groups of \d+ lanes.*whole regions", 8),
    ("team", lambda: [make_pair(36, i, 500, 0)[:2] + ((),) for i in range(640)], dict(diagonalExpansion=40),
     {"CPECAN_TEAM": "100"}, r"a team of waves per region", 0.25),
]


@pytest.mark.parametrize("form", CROSSING, ids=[f[0] for f in CROSSING])
def test_waves_that_cross_slots_keep_the_sums_apart(form, monkeypatch, capfd):
    name, make, pkw, env, pattern, per_wave = form
    monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
    monkeypatch.setenv("CPECAN_MAX_WAVES_PER_CU", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    stats = _slots_against_sequential(api.fiveState, 3, api.EMIT_EXPECT, make(), ragged=(True, name == "packed"), **pkw)
    err = capfd.readouterr().err
    assert re.search(pattern, err), "the %s form did not run:\n%s" % (name, err)
    print(name, "regions", stats.regions, "waves", stats.wavesPerLaunch)
    # fewer workgroups than ONE slot has regions (packed: groups of up to 8 regions; team: four waves per workgroup):
    # the workgroups that start in slot 0 go on into slots 1 and 2
    assert stats.regions > per_wave * stats.wavesPerLaunch


def test_forward_waves_that_cross_slots(monkeypatch):
    monkeypatch.setenv("CPECAN_MAX_WAVES_PER_CU", "1")
    problems = [make_pair(5, i, 400, 10) for i in range(600)]
    stats = _slots_against_sequential(api.fiveState, 3, api.EMIT_FORWARD, problems)
    assert stats.regions > stats.wavesPerLaunch


@pytest.mark.parametrize("emit", [api.EMIT_EXPECT, api.EMIT_FORWARD])
def test_the_same_model_in_every_slot(emit):
    problems, mtype, T = _problems(), api.fiveState, 4
    m = _random_model(mtype, 5)
    n = len(problems)
    with _batch(m, emit, problems) as plain:
        plain.run()
        plain.download()
        want = _expect(plain, mtype) if emit == api.EMIT_EXPECT else np.array([plain.forward_prob(i) for i in range(n)])
    with _batch(_default(mtype), emit, problems, reserve=T) as b:
        b.set_models([m] * T)
        b.run()
        b.download()
        for k in range(T):
            if emit == api.EMIT_EXPECT:
                _assert_hmm_close(_expect(b, mtype, k), _expect(b, mtype, 0))
                _assert_hmm_close(_expect(b, mtype, k), want)
            else:
                got = np.array([b.forward_prob(i, k) for i in range(n)])
                np.testing.assert_array_equal(got, want)


def test_a_reserved_batch_before_set_models_runs_its_own_model():
    problems, mtype = _problems(n=6), api.threeState
    m = _random_model(mtype, 2)
    with _batch(m, api.EMIT_EXPECT, problems) as plain, _batch(m, api.EMIT_EXPECT, problems, reserve=3) as b:
        for x in (plain, b):
            x.run()
            x.download()
        _assert_hmm_close(_expect(b, mtype), _expect(plain, mtype))
        with pytest.raises(api.CpecanError, match="after upload"):
            b.reserve_models(2)
        with pytest.raises(api.CpecanError, match="reserved 3"):
            b.set_models([m] * 4)
        with pytest.raises(api.CpecanError, match="reserved 0"):
            plain.set_models([m] * 2)


def test_under_subscription_is_used():
    """300 regions leave most wave slots idle: with n models the launch has n times the waves, up to the chip's capacity.
    The planner evens out the rounds of a queue longer than the chip holds (cpk_plan.inl, even_rounds: a queue of 2400 on
    2048 slots runs as two rounds of 1200 waves), so the waves of a saturated queue depend on its length.  `capacity`
    here is therefore what a large plain batch with a queue as long as the longest slotted one (8 x 300) gets, and
    min(n x 300, capacity) is asserted for n in {1, 2, 3, 8} only: n x 300 either fits the chip or IS that queue.  What
    holds for every n is asserted as well: a run with n models launches exactly the waves a plain batch of n x 300 of the
    same regions launches (n = 5: the queue of 1500)."""
    base = [make_pair(5, i, 600, 10) for i in range(300)]
    mtype, T = api.fiveState, 8
    models = [_random_model(mtype, 30 + k) for k in range(T)]
    with _batch(models[0], api.EMIT_EXPECT, base) as plain:
        unreserved = plain.stats().wavesPerLaunch
    with _batch(models[0], api.EMIT_EXPECT, base * T) as large:
        capacity = large.stats().wavesPerLaunch
    print("unreserved", unreserved, "capacity", capacity)
    assert unreserved == 300 and capacity > unreserved
    with _batch(models[0], api.EMIT_EXPECT, base, reserve=T) as b:
        assert b.stats().wavesPerLaunch == unreserved  # one model until set_models says otherwise
        for n in (2, 3, 8, 1):
            b.set_models(models[:n])
            print("n", n, "waves", b.stats().wavesPerLaunch)
            assert b.stats().wavesPerLaunch == min(n * unreserved, capacity)
            b.run()
            b.download()
            assert b.stats().wavesPerLaunch == min(n * unreserved, capacity)
        with _batch(models[0], api.EMIT_EXPECT, base * 5) as five:
            b.set_models(models[:5])
            assert b.stats().wavesPerLaunch == five.stats().wavesPerLaunch


def test_set_models_between_runs_in_flight_and_fewer_then_more():
    problems, mtype = _problems(n=6), api.fiveState
    a = [_random_model(mtype, 40 + k) for k in range(2)]
    c = [_random_model(mtype, 50 + k) for k in range(4)]
    want = []
    with _batch(_default(mtype), api.EMIT_EXPECT, problems) as plain:
        for m in c:
            plain.set_model(m)
            plain.run()
            plain.download()
            want.append(_expect(plain, mtype))
    with _batch(_default(mtype), api.EMIT_EXPECT, problems, reserve=4) as b:
        b.set_models(a)  # fewer than reserved
        b.run()
        b.set_models(c)  # more, with the first run still queued: it keeps the models it was launched with
        with pytest.raises(api.CpecanError):
            b.download()  # the run of the old models is no longer the batch's result
        b.run()
        b.download()
        for k in range(4):
            _assert_hmm_close(_expect(b, mtype, k), want[k])
        b.set_models(c[2:3])  # and back to one
        b.run()
        b.download()
        _assert_hmm_close(_expect(b, mtype, 0), want[2])
        with pytest.raises(api.CpecanError, match="slot"):
            _expect(b, mtype, 1)


# ---- the trainer: random-restart trials side by side (cpecan_em_trainer_set_concurrent_trials) ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, DX, IY = api.OP_MATCH, api.OP_INDEL_X, api.OP_INDEL_Y


def _world(seed, n=16):
    rng = random.Random(seed)
    seqs, cigars = {}, []
    for k in range(n):
        ops = []
        for i in range(2 * rng.randrange(2, 6) + 1):
            t = M if i % 2 == 0 else rng.choice([DX, IY])
            ops.append((t, rng.randrange(40, 160) if t == M else rng.choice([1, 2, 3, 5, 9])))
        sx, sy = [], []
        for t, ln in ops:
            for _ in range(ln):
                b = rng.choice("ACGT")
                if t != IY:
                    sx.append(b)
                if t != DX:
                    sy.append(b if t != M or rng.random() > 0.1 else rng.choice("ACGT"))
        lx, ly = "".join(rng.choice("ACGT") for _ in range(7)), "".join(rng.choice("ACGT") for _ in range(5))
        seqs["X%d" % k], seqs["Y%d" % k] = lx + "".join(sx) + "GATTACA", ly + "".join(sy) + "CAT"
        cigars.append(Cigar("X%d" % k, len(lx), len(lx) + len(sx), True, "Y%d" % k, len(ly), len(ly) + len(sy), True,
                            1.0, ops))
    return seqs, cigars


def _train(seqs, cigars, out, concurrent, devices=None, **opts):
    t = em.Trainer(em.em_options(**opts), em.em_realign_options(diagonalExpansion=6, splitMatrixBiggerThanThis=100))
    with t:
        for name, s in seqs.items():
            t.add_sequence(name, s)
        if devices:
            t.set_devices(devices)
        t.set_concurrent_trials(concurrent)
        best, running = t.train(cigars, str(out))
    trials = [api.hmm_loadFromFile("%s_%d" % (out, i)) for i in range(opts["trials"])]
    return best, running, trials


def _assert_same_training(a, b):
    (best_a, run_a, trials_a), (best_b, run_b, trials_b) = a, b
    likes_a, likes_b = [h.likelihood for h in trials_a], [h.likelihood for h in trials_b]
    assert len(set(likes_a)) == len(likes_a)  # different random starts
    for ha, hb in zip(trials_a, trials_b):
        np.testing.assert_allclose(list(ha.transitions), list(hb.transitions), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(list(ha.emissions), list(hb.emissions), rtol=1e-9, atol=1e-12)
    assert likes_a.index(max(likes_a)) == likes_b.index(max(likes_b))  # the same best trial
    np.testing.assert_allclose(list(best_a.transitions), list(best_b.transitions), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(run_a, run_b, rtol=1e-9)


@pytest.mark.parametrize("trials,concurrent,devices", [(3, 3, None), (5, 2, None), (3, 3, [0, 0])],
                         ids=["three_in_one_round", "five_in_rounds_of_two", "two_shards"])
def test_concurrent_trials_write_the_models_of_sequential_trials(trials, concurrent, devices, tmp_path):
    seqs, cigars = _world(101, n=14)
    opts = dict(trials=trials, randomStart=1, outputTrialHmms=1, iterations=3, trainEmissions=1, seed=23)
    one = _train(seqs, cigars, tmp_path / "one.txt", 1, devices, **opts)
    many = _train(seqs, cigars, tmp_path / "many.txt", concurrent, devices, **opts)
    _assert_same_training(one, many)
    with em.Trainer() as t:
        for bad in (0, 9):
            with pytest.raises(api.CpecanError, match="concurrent"):
                t.set_concurrent_trials(bad)


def test_command_line_concurrent_trials_end_to_end(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_em")
    seqs, cigars = _world(103, n=12)
    fa = tmp_path / "all.fa"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    cig = tmp_path / "in.cigar"
    cig.write_text("".join(c.format() + "\n" for c in cigars))
    out = tmp_path / "cli.txt"
    res = subprocess.run([exe, "--sequences", str(fa), "--alignments", str(cig), "--outputModel", str(out), "--iterations", "3",
                          "--trainEmissions", "--randomStart", "--trials", "3", "--outputTrialHmms", "--seed", "23",
                          "--concurrentTrials", "3", "--optionsToRealign", "--diagonalExpansion=6 --splitMatrixBiggerThanThis=100"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    opts = dict(trials=3, randomStart=1, outputTrialHmms=1, iterations=3, trainEmissions=1, seed=23)
    best, _, trials = _train(seqs, cigars, tmp_path / "lib.txt", 3, **opts)
    h = api.hmm_loadFromFile(str(out))
    np.testing.assert_allclose(list(h.transitions), list(best.transitions), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(list(h.emissions), list(best.emissions), rtol=1e-9, atol=1e-12)
    for i in range(3):
        hi = api.hmm_loadFromFile("%s_%d" % (out, i))
        np.testing.assert_allclose(list(hi.transitions), list(trials[i].transitions), rtol=1e-9, atol=1e-12)
