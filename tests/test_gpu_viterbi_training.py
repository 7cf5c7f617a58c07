"""Viterbi training (hard EM) on the GPU (cpecan_em_trainer_set_viterbi_training) against a Python
restatement of the trial: the paths of tests/viterbi_model.py under the current model, the counts of
tests/viterbi_counts_model.py, then the trainer's own double operations through the same functions -- api.hmm_normalise, the
emission put-back or em.hmm_tie_emissions, api.hmm_getStateMachine, em.write_model.  Six cigars over sequences of 120-200 bases
(cpecan_amd.workload), small enough for the model on the CPU; three iterations, with and without trainEmissions, a five-state
and a three-state model.  The model file after every iteration and the running likelihoods are compared byte for byte and bit
for bit; the cpecan_em binary writes the same bytes; a Baum-Welch training on a trainer gives the same file before and after a
Viterbi training on it."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import viterbi_counts_model as cm
import viterbi_model as vm
from cpecan_amd import api, em, viterbi
from cpecan_amd.realign import Cigar
from cpecan_amd.workload import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_em")
M, DX, IY = api.OP_MATCH, api.OP_INDEL_X, api.OP_INDEL_Y
E, SPLIT, JC, ITERATIONS, SEED = 6, 40, 0.2, 3, 11
LENGTHS = (120, 136, 152, 168, 184, 200)
ORACLE_TYPE = {api.fiveState: ob.FIVE_STATE, api.threeState: ob.THREE_STATE}


@functools.lru_cache(maxsize=None)
def _world():
    """Six pairs and the cigars of their true alignments' equal columns -- without those of 50 bases of X, a gap large enough
    to cut the cigar into regions there -- and a flank of other bases around each sub-sequence."""
    seqs, cigars = {}, []
    for k, length in enumerate(LENGTHS):
        sx, sy, anchors = make_pair(seed=41, index=k, length=length, expansion=E, anchor_every=1)
        nx, ny = "X%d" % k, "Y%d" % k
        c = Cigar.from_aligned_pairs(nx, ny, 1.0, len(sx), len(sy), [(int(x), int(y)) for x, y, _ in anchors if not 50 <= x < 100])
        seqs[nx], seqs[ny] = "GATTACA" + sx.decode() + "CAT", "TTG" + sy.decode() + "ACCA"
        cigars.append(Cigar(nx, c.start1 + 7, c.end1 + 7, True, ny, c.start2 + 3, c.end2 + 3, True, 1.0, c.ops))
    return seqs, tuple(cigars)


def _problem(seqs, c):
    """cPecanRealign.c:511-529: the sub-sequences and the exact-match anchors of the cigar's match columns."""
    sx, sy = seqs[c.contig1][c.start1:c.end1], seqs[c.contig2][c.start2:c.end2]
    anchors, x, y = [], 0, 0
    for t, ln in c.ops:
        for _ in range(ln):
            if t == M and sx[x].upper() == sy[y].upper() and sx[x].upper() != "N":
                anchors.append((x, y, E))
            x += t != IY
            y += t != DX
    assert (x, y) == (len(sx), len(sy))
    return sx.encode(), sy.encode(), anchors


def _start(mtype):
    h = em.hmm_equalise(api.hmm_constructEmpty(0.0, mtype))
    h.likelihood = 0.0
    return em.hmm_set_jukes_cantor(h, JC)


def _copy(h):
    g = api.Hmm()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(h), ctypes.sizeof(h))
    return g


def _oracle_model(h, mtype):
    S = h.stateNumber
    oh = ob.hmm(ORACLE_TYPE[mtype], 0.0)
    for i in range(S * S):
        oh.T[i] = h.transitions[i]
    for i in range(S * 16):
        oh.E[i] = h.emissions[i]
    return ob.model_from_hmm(oh)


@functools.lru_cache(maxsize=None)
def _restated(mtype, train, tie, pseudo):
    """The trial written out: [(model file bytes after iteration k, with the running likelihoods of iterations 0 .. k)],
    and the running likelihoods.  Computed once per configuration."""
    seqs, cigars = _world()
    order, _, _ = em.sample(cigars, 1000000, 50000000, SEED)
    problems = [_problem(seqs, cigars[i]) for i in order]
    p = ob.params(diagonalExpansion=E, splitMatrixBiggerThanThis=SPLIT * SPLIT)
    h, running, files, steps = _start(mtype), [], [], []
    S = h.stateNumber
    for it in range(ITERATIONS):
        om = _oracle_model(h, mtype)
        parts = []
        for sx, sy, anchors in problems:
            m = vm.viterbi(om, sx, sy, anchors, p, True, True)
            inputs = [(sx[x1:x2], sy[y1:y2], rl, rr) for x1, y1, x2, y2, _, rl, rr in vm.regions_of(anchors, len(sx), len(sy), p, True, True)]
            parts += cm.regions(S, m, inputs)
        counts = cm.total(S, parts)
        acc = api.hmm_constructEmpty(pseudo, mtype)
        viterbi.counts_add_to_hmm(counts, acc)
        api.hmm_normalise(acc)
        running.append(acc.likelihood)
        if not train:
            for i in range(S * 16):
                acc.emissions[i] = h.emissions[i]
        elif tie:
            em.hmm_tie_emissions(acc)
        h = _copy(acc)
        steps.append(counts.nSteps)
        files.append((_copy(h), list(running)))
    assert len(parts) > len(problems), "some cigar is cut into several regions"
    assert all(n > 700 for n in steps)
    return tuple(files), tuple(running)


def _file_bytes(tmp_path, h, running, name="want.txt"):
    em.write_model(h, str(tmp_path / name), running)
    return open(tmp_path / name, "rb").read()


def _trainer(seqs, **opts):
    t = em.Trainer(em.em_options(setJukesCantorStartingEmissions=JC, seed=SEED, **opts),
                   em.em_realign_options(diagonalExpansion=E, splitMatrixBiggerThanThis=SPLIT))
    for name, s in seqs.items():
        t.add_sequence(name, s)
    return t


CONFIGS = [(api.fiveState, 1, 0, 1.0), (api.fiveState, 0, 0, 1.0), (api.threeState, 1, 1, 0.5), (api.threeState, 0, 0, 1.0)]


@pytest.mark.parametrize("mtype,train,tie,pseudo", CONFIGS)
def test_training_equals_the_trial_written_out(tmp_path, mtype, train, tie, pseudo):
    seqs, cigars = _world()
    files, want_running = _restated(mtype, train, tie, pseudo)
    for k in range(1, ITERATIONS + 1):
        out = tmp_path / ("hmm%d.txt" % k)
        with _trainer(seqs, modelType=mtype, iterations=k, trainEmissions=train, tieEmissions=tie) as t:
            t.set_viterbi_training(True, pseudo)
            best, running = t.train(cigars, str(out))
            tm = t.timing()
        want_h, want_run = files[k - 1]
        print("type %d train %d iterations %d: running %r" % (mtype, train, k, running))
        assert np.array(running).tobytes() == np.array(want_run).tobytes(), (running, want_run)
        assert open(out, "rb").read() == _file_bytes(tmp_path, want_h, want_run), k
        S = best.stateNumber
        assert list(best.transitions[:S * S]) == list(want_h.transitions[:S * S]) and best.likelihood == want_h.likelihood
        assert tm.cigars == len(cigars) and tm.iterations == k and tm.setupMs > 0 and tm.iterationsMs > 0
    assert list(want_running) == running
    assert all(v < 0 for v in running)


def test_add_one_smoothing_keeps_unused_transitions_alive(tmp_path):
    """No path of this sample takes a long gap; with the default pseudo-count the long-gap opens keep a probability far above
    the 1e-12 of a Baum-Welch job's pseudo-count, and with 0 they fall to exactly 0."""
    seqs, cigars = _world()
    got = {}
    for pseudo in (1.0, 0.0):
        with _trainer(seqs, modelType=api.fiveState, iterations=1) as t:
            t.set_viterbi_training(True, pseudo)
            got[pseudo], _ = t.train(cigars, str(tmp_path / "hmm.txt"))
    unused = [i for i in range(25) if got[0.0].transitions[i] == 0.0]
    assert unused, "the sample uses every transition: the test shows nothing"
    assert all(got[1.0].transitions[i] > 1e-5 for i in unused)


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for name, s in seqs.items():
            f.write(">%s\n%s\n" % (name, s))


def test_the_binary_writes_the_same_bytes(tmp_path):
    seqs, cigars = _world()
    _write_fasta(tmp_path / "seqs.fa", seqs)
    (tmp_path / "in.cigar").write_text("".join(c.format() + "\n" for c in cigars))
    for mtype, name, train, pseudo in ((api.fiveState, "fiveState", 1, 1.0), (api.threeState, "threeState", 0, 1.0)):
        out = tmp_path / ("cli_%s.txt" % name)
        args = [EXE, "--sequences", str(tmp_path / "seqs.fa"), "--alignments", str(tmp_path / "in.cigar"), "--outputModel", str(out),
                "--iterations", str(ITERATIONS), "--modelType", name, "--seed", str(SEED), "--setJukesCantorStartingEmissions", str(JC),
                "--optionsToRealign", "--diagonalExpansion=%d --splitMatrixBiggerThanThis=%d" % (E, SPLIT), "--viterbiTraining"]
        if train:
            args.append("--trainEmissions")
        res = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        want_h, want_run = _restated(mtype, train, 0, pseudo)[0][ITERATIONS - 1]
        assert open(out, "rb").read() == _file_bytes(tmp_path, want_h, want_run), name
    # another pseudo-count gives another model
    res = subprocess.run(args + ["--outputModel", str(tmp_path / "cli_half.txt"), "--viterbiPseudoCount", "0.5"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert open(tmp_path / "cli_half.txt", "rb").read() != open(out, "rb").read()


def test_the_switch_leaves_nothing_behind(tmp_path):
    """Baum-Welch on one trainer before and after a Viterbi training gives the file it gives on a trainer of its own.  One
    cigar in one region: a Baum-Welch training of more regions is not reproducible to the byte from run to run on any build
    (tests/test_gpu_em_update_band.py says why), so more would show nothing."""
    seqs, cigars = _world()
    one = list(cigars[:1])
    ro_split = 3000  # the cigar is one region

    def trainer():
        t = em.Trainer(em.em_options(setJukesCantorStartingEmissions=JC, seed=SEED, iterations=ITERATIONS, trainEmissions=1),
                       em.em_realign_options(diagonalExpansion=E, splitMatrixBiggerThanThis=ro_split))
        for name, s in seqs.items():
            t.add_sequence(name, s)
        return t

    def train(t, name):
        t.train(one, str(tmp_path / name))
        return open(tmp_path / name, "rb").read()

    with trainer() as t:
        alone = train(t, "alone.txt")
    with trainer() as t:
        before = train(t, "before.txt")
        t.set_viterbi_training(True, 1.0)
        hard = train(t, "viterbi.txt")
        t.set_viterbi_training(False)
        after = train(t, "after.txt")
    assert before == alone and after == alone
    assert hard != alone
