"""Viterbi counts and Viterbi training without a GPU: the host functions of include/cpecan_viterbi.h that the feature adds --
counts_of_ops, counts_add_to_hmm, set_model, the refusals of run_counts and problem_counts -- against the numpy definition
(tests/viterbi_counts_model.py) on every case of tests/viterbi_counts_cases.py, on both builds of the library; the trainer's
refusals; the two options of the cpecan_em binary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viterbi_cases as vc
import viterbi_counts_cases as cc
import viterbi_counts_model as cm
from cpecan_amd import api, em, viterbi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(ROOT, "cpecan_amd", "libcpecan_hip_exact.so")
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_em")
NO_DEVICE = 1000


def test_the_cases_are_the_edges_they_claim():
    cc.check_preconditions()


def _exact_counts_of_ops(S, sx, sy, start_state, ops):
    """cpecan_viterbi_counts_of_ops of the exact-logAdd library, called through a handle of its own."""
    L = C.CDLL(EXACT)
    f = L.cpecan_viterbi_counts_of_ops
    f.argtypes = viterbi._lib().cpecan_viterbi_counts_of_ops.argtypes
    o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
    n = o.size // 2
    if n == 0:
        o = np.zeros(2, dtype=np.int32)
    c = viterbi.ViterbiCounts()
    assert f(S, bytes(sx), len(sx), bytes(sy), len(sy), start_state, o.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(c)) == 0
    return viterbi._counts(c)


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_counts_of_ops_equals_the_model_and_the_identities_hold(name):
    """Every region of the case, both libraries; sum(trans) == nSteps, the column sums of trans are the steps per state."""
    c = cc.case(name)
    S, m = cc.n_states(c), vc.model_of(c)
    for r, want, (sx, sy, _, _) in zip(m.regions, cc.region_counts(c), vc.region_inputs(c)):
        if r.endState < 0:
            assert (want.nSteps, want.nNoPath) == (0, 1)
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # no path: no start state, and no ops that reach (lX, lY)
                viterbi.counts_of_ops(S, sx, sy, r.startState, m.ops[r.opOff:r.opOff + r.nOps])
            if len(sx) + len(sy) > 0:
                with pytest.raises(api.CpecanError, match=r"\(-1\).*end at"):
                    viterbi.counts_of_ops(S, sx, sy, 0, m.ops[r.opOff:r.opOff + r.nOps])
            continue
        ops = m.ops[r.opOff:r.opOff + r.nOps]
        want0 = want._replace(logP=0.0)  # the host function knows no logP
        cm.assert_equal(viterbi.counts_of_ops(S, sx, sy, r.startState, ops), want0, (name, r))
        cm.assert_equal(_exact_counts_of_ops(S, sx, sy, r.startState, ops), want0, (name, r, "exact"))
        match_steps = int(ops[ops[:, 0] == 0, 1].sum())  # a match step moves along both sequences
        assert int(want.transitions.sum()) == want.nSteps == len(sx) + len(sy) - match_steps
        steps_in = [int(ops[ops[:, 0] == s, 1].sum()) for s in range(S)]
        assert want.transitions.sum(axis=0).tolist() == steps_in, (name, r)
        assert int(want.emissions.sum()) == want.nSteps - cm.steps_without_emission(sx, sy, ops)
        assert want.emissions.sum(axis=1).tolist() <= steps_in
    pc = cc.problem_counts(c)
    assert int(pc.transitions.sum()) == pc.nSteps and pc.nNoPath == sum(r.endState < 0 for r in m.regions)


def test_counts_of_ops_refuses_ops_that_miss_the_end():
    c = cc.case("a_tiny5")
    m = vc.model_of(c)
    r, ops = m.regions[0], m.ops
    good = lambda o, s0=r.startState, S=5: viterbi.counts_of_ops(S, c.sx, c.sy, s0, np.array(o, dtype=np.int32))  # noqa: E731
    assert good(ops).nSteps == int(ops[:, 1].sum())
    for bad in (ops[:-1], np.concatenate([ops, [[0, 1]]]), [[5, 4]], [[0, -1]], [[1, 0]]):
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            good(bad)
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        good(ops, s0=5)
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        good(ops, S=4)
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        good([[3, len(c.sx)], [4, len(c.sy)]], S=3)  # the long-gap states of a three-state model


@pytest.mark.parametrize("model", ("fiveState", "threeStateAsym"))
def test_counts_add_to_hmm_is_exact(model):
    sm, om = vc.model_pair(model)
    S = om.S
    rng = np.random.default_rng(5)
    counts = viterbi.Counts(rng.integers(0, 2 ** 40, (S, S)), rng.integers(0, 2 ** 40, (S, 16)), 7, 1, -1234.5678)
    h = api.hmm_constructEmpty(0.25, sm.type)
    h.likelihood = -0.125
    viterbi.counts_add_to_hmm(counts, h)
    assert [h.transitions[i] for i in range(S * S)] == [0.25 + float(t) for t in counts.transitions.reshape(-1)]
    assert [h.emissions[i] for i in range(S * 16)] == [0.25 + float(t) for t in counts.emissions.reshape(-1)]
    assert h.likelihood == -0.125 + -1234.5678
    other = api.hmm_constructEmpty(0.0, api.threeState if S == 5 else api.fiveState)
    with pytest.raises(api.CpecanError, match=r"\(-1\).*states"):
        viterbi.counts_add_to_hmm(counts, other)
    assert all(other.transitions[i] == 0.0 for i in range(25))


def test_set_model_run_counts_and_problem_counts_refuse_in_order_without_a_device():
    c = vc.case("u_300x300")
    sm5, sm3 = api.stateMachine5_construct(), api.stateMachine3_construct()
    with viterbi.Viterbi(sm5, vc.lib_params(c), device=NO_DEVICE) as v:
        with pytest.raises(api.CpecanError, match=r"\(-1\).*states"):
            v.set_model(sm3)
        v.set_model(api.stateMachine5_construct(api.fiveStateAsymmetric))  # the state count is what matters
        with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
            v.run_counts()  # no problems: nothing to refuse before the device
        v.add(c.sx, c.sy)
        with pytest.raises(api.CpecanError, match=r"\(-5\).*off"):
            v.problem_counts(0)
        need = v.info(0)["deviceBytes"]
        inputs, scratch = v.resident_bytes()
        assert 0 < inputs < need and inputs + scratch > need  # the slab comes on top of what deviceBytes counts
        v.set_budget(need - 1)
        with pytest.raises(api.CpecanError, match=r"\(-4\).*run_counts.*needs %d bytes" % need):
            v.run_counts()
        with pytest.raises(api.CpecanError, match=r"\(-4\)"):
            v.resident_bytes()
        v.set_budget(need)
        v.set_form(viterbi.FORM_LDS)
        with pytest.raises(api.CpecanError, match=r"\(-1\).*LDS form"):
            v.run_counts()
        v.set_form(viterbi.FORM_AUTO)
        with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
            v.run_counts()
        v.set_keep_problem_counts(True)
        with pytest.raises(api.CpecanError, match=r"\(-5\).*before"):
            v.problem_counts(0)
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            v.problem_counts(1)
        assert v.count_ms() == (0.0, 0.0)
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):
            v.run()  # the plain run is as it was
    assert viterbi._lib().cpecan_viterbi_run_counts(None, None) == -1


def test_trainer_refuses_what_viterbi_training_does_not_go_with_before_any_device():
    with em.Trainer(em.em_options(updateTheBand=1)) as t:
        with pytest.raises(api.CpecanError, match=r"\(-1\).*updateTheBand"):
            t.set_viterbi_training()
    with em.Trainer(em.em_options(randomStart=1, trials=2)) as t:
        t.set_concurrent_trials(2)
        with pytest.raises(api.CpecanError, match=r"\(-1\).*concurrent trials"):
            t.set_viterbi_training()
        t.set_concurrent_trials(1)
        t.set_viterbi_training()
        t.set_concurrent_trials(2)  # switched on first: the training itself refuses
        with pytest.raises(api.CpecanError, match=r"\(-1\).*concurrent trials"):
            t.train([], "unused")
    with em.Trainer(em.em_options()) as t:
        t.set_devices([0, 1])
        with pytest.raises(api.CpecanError, match=r"\(-1\).*2 devices"):
            t.set_viterbi_training()
        t.set_devices([0])
        for bad in (-1.0, float("nan"), float("inf"), -1e-300):
            with pytest.raises(api.CpecanError, match=r"\(-1\).*pseudo-count"):
                t.set_viterbi_training(True, bad)
        t.set_viterbi_training(True, 0.0)
        t.set_viterbi_training(False)
        t.set_viterbi_training(pseudo_count=2.5)
    assert em._lib().cpecan_em_trainer_set_viterbi_training(None, 1, 1.0) == -1


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_command_line_parses_the_two_options_and_refuses_update_the_band(tmp_path):
    assert os.path.exists(EXE), "build the command line with make -C cpecan_amd/csrc"
    files = ["--sequences", str(tmp_path / "a.fa"), "--alignments", "x"]
    res = _run(*files, "--viterbiTraining", "--viterbiPseudoCount", "0.5")
    assert res.returncode != 0 and "cannot open" in res.stderr  # accepted: the files are missing
    res = _run(*files, "--viterbiPseudoCount", "many")
    assert res.returncode != 0 and "--viterbiPseudoCount many" in res.stderr
    res = _run(*files, "--viterbiTraining", "--viterbiPseudoCount", "-1")
    assert res.returncode != 0 and "pseudo-count" in res.stderr and "cannot open" not in res.stderr
    res = _run(*files, "--viterbiTraining", "--updateTheBand")
    assert res.returncode != 0 and "Viterbi training does not go with updateTheBand" in res.stderr and "cannot open" not in res.stderr
    assert "--viterbiTraining" in _run("--help").stderr and "--viterbiPseudoCount" in _run("--help").stderr
