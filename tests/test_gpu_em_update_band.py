"""The trainer's updateTheBand on the GPU (include/cpecan_em.h; cPecanEm.py:205-215): cpecan_em_train with the option against
the same loop written here from Realigner.expectations, the M-step and Realigner.realign -- the realigned cigars replace
the alignments after every iteration but the last.  Eight cigars of 150 .. 300 bases, three with a misplaced deletion
(tests/next_runs_cases.py, whose preconditions tests/test_next_runs_cpu.py asserts on the oracle), five-state model, three
iterations, trainEmissions.  The anchors of cpecan_em_trainer_alignments must be the runs of the loop's last cigars, integer
for integer; transitions, emissions and running likelihoods agree to 1e-6 relative, the figure
test_several_devices_from_one_process uses for a batch that is cut differently."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import next_runs_cases as nc
from cpecan_amd import api, em
from cpecan_amd.realign import Cigar, Realigner

pytestmark = pytest.mark.gpu

RTOL = 1e-6
JOB_PSEUDO = 0.000000000001  # one cPecanRealign --outputExpectations job
THRESHOLD = nc.EM_THRESHOLD  # the posterior threshold of the realign options (one test runs at the default, 0.01)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "em_one_cigar_before_update_band.txt")
# Two trainings of the same sample on the same build do not give the same bytes when the sample is cut into more than one
# region: the EXPECT kernels hand regions to waves through an atomic ticket and add a wave's counts in the order it took
# them.  profiles/em_run_to_run.txt records it on the commit before this option and on this one: eight files of the eight
# cigars below, eight different files, largest relative difference 1.6e-13.  The bound is not that figure but what the
# sums allow: an E-step adds fewer than 1e5 terms per count (band cells of the sample), each reordering moves a sum by at
# most that many roundings of 1.1e-16, so 1e-11.
RUN_TO_RUN = 1e-11


def _options():
    return em.em_realign_options(diagonalExpansion=nc.EM_E, splitMatrixBiggerThanThis=nc.EM_SPLIT, threshold=THRESHOLD)


def _world():
    seqs, cigars = nc.em_world()
    return seqs, [Cigar(*c) for c in cigars]


def _realigner(seqs, h):
    r = Realigner(api.hmm_getStateMachine(h), _options())
    for name, s in seqs.items():
        r.add_sequence(name, s)
    return r


def _start(randomised=None):
    h = randomised if randomised is not None else em.hmm_equalise(api.hmm_constructEmpty(0.0, api.fiveState))
    h.likelihood = 0.0
    return em.hmm_set_jukes_cantor(h, nc.EM_JC)


def _loop(seqs, cigars, h, iterations=nc.EM_ITERATIONS):
    """(model, running likelihoods, the cigars the last E-step ran on)."""
    running, cur = [], list(cigars)
    for it in range(iterations):
        acc = api.hmm_constructEmpty(JOB_PSEUDO, api.fiveState)
        with _realigner(seqs, h) as r:
            r.expectations(cur, acc)
        api.hmm_normalise(acc)  # trainEmissions without tying: the M-step is the normalisation
        running.append(acc.likelihood)
        h = acc
        if it + 1 < iterations:
            with _realigner(seqs, h) as r:
                cur = r.realign(cur)
    return h, running, cur


def _runs_of(seqs, raw, cigars):
    out = []
    for a, c in zip(raw, cigars):
        sx, sy = nc.sub_sequences(seqs, a)
        out.append([tuple(int(v) for v in row) for row in api.anchor_runs_from_alignment(c.ops, 0, 0, 0, nc.EM_E, sx, sy)])
    return out


def _trainer(seqs, devices=None, **opts):
    t = em.Trainer(em.em_options(iterations=nc.EM_ITERATIONS, trainEmissions=1, setJukesCantorStartingEmissions=nc.EM_JC, **opts),
                   _options())
    for name, s in seqs.items():
        t.add_sequence(name, s)
    if devices:
        t.set_devices(devices)
    return t


def _close(got, want):
    np.testing.assert_allclose(list(got.transitions[:25]), list(want.transitions[:25]), rtol=RTOL)
    np.testing.assert_allclose(list(got.emissions[:80]), list(want.emissions[:80]), rtol=RTOL)


@pytest.fixture(scope="module")
def reference_loop():
    seqs, cigars = _world()
    return _loop(seqs, cigars, _start())


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_trainer_equals_the_loop_written_out(tmp_path, reference_loop, devices):
    seqs, cigars = _world()
    want_h, want_running, last = reference_loop
    with _trainer(seqs, devices=devices, updateTheBand=1) as t:
        best, running = t.train(cigars, str(tmp_path / "hmm.txt"))
        anchors = t.alignments()
        tm = t.timing()
    assert [[tuple(int(v) for v in q) for q in a] for a in anchors] == _runs_of(seqs, nc.em_world()[1], last)
    _close(best, want_h)
    np.testing.assert_allclose(running, want_running, rtol=RTOL)
    assert tm.realignMs > 0 and tm.replanMs > 0 and 0 < tm.handoffMs <= tm.realignMs and tm.cigars == 8
    # the option did something: the last anchors are not those of the sampled cigars
    assert _runs_of(seqs, nc.em_world()[1], last) != _runs_of(seqs, nc.em_world()[1], cigars)
    loaded = api.hmm_loadFromFile(str(tmp_path / "hmm.txt"))
    assert list(loaded.transitions[:25]) == list(best.transitions[:25])


def _train_without(tmp_path, seqs, cigars, name, **opts):
    """The model file of a training without the option; no realign, hand-off or re-plan code may have run."""
    with _trainer(seqs, **opts) as t:
        t.train(cigars, str(tmp_path / name))
        tm = t.timing()
        assert (tm.realignMs, tm.replanMs, tm.handoffMs) == (0.0, 0.0, 0.0)
        with pytest.raises(api.CpecanError):
            t.alignments()
    return open(tmp_path / name, "rb").read()


def test_without_the_option_one_cigar_gives_the_bytes_of_the_commit_before(tmp_path):
    """A sample of one cigar is one region and one wave: its training is reproducible, and its model file must be, byte for
    byte, the one the commit before this option wrote for the same call (tests/golden; profiles/em_run_to_run.txt says
    how it was recorded)."""
    seqs, cigars = _world()
    want = open(GOLDEN, "rb").read()
    for k, opts in enumerate((dict(), dict(updateTheBand=0))):
        assert _train_without(tmp_path, seqs, cigars[:1], "one%d.txt" % k, **opts) == want


def test_without_the_option_nothing_changes(tmp_path):
    seqs, cigars = _world()
    files = [_train_without(tmp_path, seqs, cigars, "hmm%d.txt" % k, **opts) for k, opts in enumerate((dict(), dict(updateTheBand=0)))]
    # eight cigars are eight regions: byte equality does not hold between two runs of ANY build (RUN_TO_RUN above)
    a, b = ([[float(v) for v in line.split()] for line in f.decode().split("\n") if line] for f in files)
    assert [len(line) for line in a] == [len(line) for line in b] == [27, 80, 3]
    for la, lb in zip(a, b):
        np.testing.assert_allclose(la, lb, rtol=RUN_TO_RUN)
    # and it is the loop without realignments, E-step for E-step
    h, running = _start(), []
    for _ in range(nc.EM_ITERATIONS):
        acc = api.hmm_constructEmpty(JOB_PSEUDO, api.fiveState)
        with _realigner(seqs, h) as r:
            r.expectations(cigars, acc)
        api.hmm_normalise(acc)
        running.append(acc.likelihood)
        h = acc
    third = [float(v) for v in files[0].decode().split("\n")[2].split("\t")]
    np.testing.assert_allclose(third, running, rtol=RTOL)


def test_trainer_equals_the_loop_at_the_default_threshold(tmp_path, monkeypatch):
    """The same comparison at cPecanRealign's own threshold, 0.01, where list 0 is dense.  The oracle's margin
    (tests/next_runs_cases.py: EM_THRESHOLD) is about kernels against the oracle, one score unit apart; here both sides run
    the same kernels, their models differ by the run-to-run noise of the E-step (RUN_TO_RUN), and a pair would have to lie
    that close to a threshold to flip a cigar."""
    monkeypatch.setattr(sys.modules[__name__], "THRESHOLD", 0.01)
    seqs, cigars = _world()
    want_h, want_running, last = _loop(seqs, cigars, _start())
    with _trainer(seqs, updateTheBand=1) as t:
        best, running = t.train(cigars, str(tmp_path / "hmm.txt"))
        anchors = t.alignments()
    assert [[tuple(int(v) for v in q) for q in a] for a in anchors] == _runs_of(seqs, nc.em_world()[1], last)
    _close(best, want_h)
    np.testing.assert_allclose(running, want_running, rtol=RTOL)


def test_two_trials_each_start_from_the_input_sample(tmp_path):
    seqs, cigars = _world()
    seed = 23
    out = tmp_path / "hmm.txt"
    with _trainer(seqs, updateTheBand=1, randomStart=1, trials=2, outputTrialHmms=1, seed=seed) as t:
        best, _ = t.train(cigars, str(out))
        anchors = t.alignments()
    state = C.c_uint64(seed ^ 0x5DEECE66D)  # the trainer's stream of random starts
    likes = []
    for k in range(2):
        h = api.hmm_constructEmpty(0.0, api.fiveState)
        api._check(em._lib().cpecan_hmm_randomise(C.byref(h), C.byref(state)), "cpecan_hmm_randomise")
        want_h, want_running, last = _loop(seqs, cigars, _start(h))
        got = api.hmm_loadFromFile("%s_%d" % (out, k))
        _close(got, want_h)
        assert got.likelihood == pytest.approx(want_running[-1], rel=RTOL)
        likes.append(got.likelihood)
    assert best.likelihood == max(likes)
    # the anchors are those of the last trial
    assert [[tuple(int(v) for v in q) for q in a] for a in anchors] == _runs_of(seqs, nc.em_world()[1], last)
