"""CPU checks of the pair-HMM trainer (include/cpecan_em.h): the model operations of cPecanEm.py's Hmm against numbers
worked out by hand, the blast / lastz matrix against a restatement of makeBlastScoringMatrix, the sampling, the model
file, the command line's option handling, and cpecan_batch_set_model's argument checks (no GPU needed for any)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from cpecan_amd import api, em
from cpecan_amd.realign import Cigar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_em")
GOLD_HMM = os.path.join(ROOT, "tests", "golden", "trained_hmm_cPecanEmTest.txt")


def _rows_sum_to_one(h):
    S = h.stateNumber
    for s in range(S):
        assert sum(h.transitions[s * S:(s + 1) * S]) == pytest.approx(1.0, abs=1e-12)
        assert sum(h.emissions[s * 16:(s + 1) * 16]) == pytest.approx(1.0, abs=1e-12)


def test_normalise_by_hand():
    h = api.hmm_constructEmpty(0.0, api.threeState)
    h.transitions[0], h.transitions[1], h.transitions[2] = 1.0, 3.0, 4.0  # row 0: 1/8, 3/8, 4/8
    for i in range(3, 9):
        h.transitions[i] = 2.0
    for i in range(48):
        h.emissions[i] = 1.0 + (i % 16 == 0) * 15.0  # per state: 16 in the first cell, 1 in 15 others: 16/31, 1/31
    api.hmm_normalise(h)
    assert list(h.transitions[:3]) == pytest.approx([0.125, 0.375, 0.5])
    assert list(h.transitions[3:6]) == pytest.approx([1 / 3] * 3)
    assert h.emissions[0] == pytest.approx(16 / 31) and h.emissions[1] == pytest.approx(1 / 31)
    _rows_sum_to_one(h)


def test_equalise_by_hand():
    for t, S in ((api.fiveState, 5), (api.threeStateAsymmetric, 3)):
        h = em.hmm_equalise(api.hmm_constructEmpty(0.3, t))
        assert list(h.transitions[:S * S]) == [1.0 / S] * (S * S)
        assert list(h.emissions[:S * 16]) == [1.0 / 16] * (S * 16)
        _rows_sum_to_one(h)


def test_jukes_cantor_by_hand():
    h = em.hmm_set_jukes_cantor(em.hmm_equalise(api.hmm_constructEmpty(0.0, api.fiveState)), 0.2)
    e = math.exp(-4.0 * 0.2 / 3.0)  # 0.765928...
    same, other = (0.25 + 0.75 * e) / 4, (0.25 - 0.25 * e) / 4
    assert same == pytest.approx(0.2061117, abs=1e-6) and other == pytest.approx(0.0146294, abs=1e-6)
    for s in range(5):
        for x in range(4):
            for y in range(4):
                assert h.emissions[s * 16 + x * 4 + y] == pytest.approx(same if x == y else other, rel=1e-14)
    _rows_sum_to_one(h)
    # divergence 0: the identity
    h = em.hmm_set_jukes_cantor(h, 0.0)
    assert h.emissions[0] == 0.25 and h.emissions[1] == 0.0


def test_tie_emissions_by_hand():
    h = em.hmm_equalise(api.hmm_constructEmpty(0.0, api.threeState))
    a = [0.4, 0.0, 0.0, 0.0, 0.0, 0.2, 0.0, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1, 0.0, 0.0, 0.1]  # identity 0.8
    for s in range(3):
        for i in range(16):
            h.emissions[s * 16 + i] = a[i]
    em.hmm_tie_emissions(h)
    for s in range(3):
        for i in range(16):
            want = 0.2 if i % 4 == i // 4 else 0.2 / 12
            assert h.emissions[s * 16 + i] == pytest.approx(want, rel=1e-14)
    _rows_sum_to_one(h)


def test_randomise_is_seeded_and_normalised():
    a = em.hmm_randomise(api.hmm_constructEmpty(0.0, api.fiveStateAsymmetric), 7)
    b = em.hmm_randomise(api.hmm_constructEmpty(0.0, api.fiveStateAsymmetric), 7)
    c = em.hmm_randomise(api.hmm_constructEmpty(0.0, api.fiveStateAsymmetric), 8)
    assert list(a.transitions) == list(b.transitions) and list(a.emissions) == list(b.emissions)
    assert list(a.transitions) != list(c.transitions)
    assert len(set(a.transitions[:25])) == 25 and min(a.emissions[:80]) > 0
    _rows_sum_to_one(a)


def _load_gold():
    t, e = [l.split() for l in open(GOLD_HMM).read().split("\n") if l.strip()][:2]
    h = api.hmm_constructEmpty(0.0, int(t[0]))
    S = h.stateNumber
    for i in range(S * S):
        h.transitions[i] = float(t[1 + i])
    h.likelihood = float(t[1 + S * S])
    for i in range(S * 16):
        h.emissions[i] = float(e[i])
    return h


def _blast_by_formula(h, seqs):
    """makeBlastScoringMatrix (cPecanEm.py) written out again: a three-state view, base frequencies from the GC content."""
    S = h.stateNumber
    t = [h.transitions[f * S + g] for f in range(3) for g in range(3)]
    t = [v / sum(t[3 * (i // 3):3 * (i // 3) + 3]) for i, v in enumerate(t)]
    em_ = [h.emissions[i] / sum(h.emissions[:16]) for i in range(16)]
    gc = sum(c in "GC" for s in seqs for c in s) / sum(len(s) for s in seqs)
    base = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    probs = [em_[x * 4 + y] / (base[x] * base[y]) for x in range(4) for y in range(4)]
    mc = t[0]
    n = math.sqrt(math.exp((6.94 + sum(math.log(p * mc) for p in probs)) / 16))
    scores = [100 * math.log(p * mc / n ** 2) for p in probs]
    gap_open = 100 * math.log(0.5 * (t[1] / n + t[2] / n) * ((t[3] + t[6]) / (2 * n ** 2)) * (n ** 2 / mc))
    gap_extend = 100 * math.log(0.5 * (t[4] / n + t[8] / n))
    return scores, gap_open, gap_extend


def test_blast_matrix_of_the_trained_model(tmp_path):
    h = _load_gold()
    fa = tmp_path / "s.fa"
    fa.write_text(">s\nTTT\nGG\n")
    gc, total = C.c_int64(0), C.c_int64(0)
    assert em._lib().cpecan_em_fasta_gc(str(fa).encode(), C.byref(gc), C.byref(total)) == 1
    assert (gc.value, total.value) == (2, 5)
    got = em.blast_matrix(h, gc.value / total.value)
    want = _blast_by_formula(h, ["TTTGG"])
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12)
    assert got[1] == pytest.approx(want[1], rel=1e-12) and got[2] == pytest.approx(want[2], rel=1e-12)
    out = tmp_path / "blast.txt"
    em.write_lastz_matrix(str(out), *got)
    lines = out.read_text().split("\n")
    assert lines[0] == "gap_open_penalty = %d" % round(-want[1])
    assert lines[1] == "gap_extend_penalty = %d" % round(-want[2])
    assert lines[2] == "\t\tA\tC\tG\tT"
    for x in range(4):
        assert lines[3 + x] == "\t%s\t%s" % ("ACGT"[x], "\t".join(str(int(round(v))) for v in want[0][4 * x:4 * x + 4]))


def _cigars(lengths):
    return [Cigar("x%d" % i, 0, n, True, "y%d" % i, 0, n + 2, True, 1.0, [(api.OP_MATCH, n), (api.OP_INDEL_Y, 2)])
            for i, n in enumerate(lengths)]


def test_sampling_is_seeded_and_respects_both_limits():
    rng = np.random.default_rng(3)
    lengths = [int(v) for v in rng.integers(50, 400, size=200)]
    cigars = _cigars(lengths)
    alen = [n + 1 for n in lengths]  # (n + n + 2) / 2
    per_job, to_sample = 1000, 9000
    a = em.sample(cigars, per_job, to_sample, 11)
    assert a == em.sample(cigars, per_job, to_sample, 11)
    assert a != em.sample(cigars, per_job, to_sample, 12)
    order, jobs, total = a
    assert len(set(order)) == len(order)
    # the jobs are runs of consecutive cigars; each closes at the first cigar that takes it above per_job
    runs, start = [], 0
    for k in range(1, len(order) + 1):
        if k == len(order) or order[k] != order[k - 1] + 1:
            runs.append(order[start:k])
            start = k
    sizes = []
    for run in runs:  # a run may hold several jobs that happened to be drawn one after the other
        acc = 0
        for i in run:
            acc += alen[i]
            if acc > per_job:
                sizes.append(acc)
                acc = 0
        if acc:
            sizes.append(acc)
    assert all(s - max(alen) <= per_job for s in sizes)
    assert total == pytest.approx(sum(alen[i] for i in order))
    assert total >= to_sample and total - 2 * per_job - max(alen) < to_sample
    # everything when the limit is above the total; nothing drops out of a job
    order, jobs, total = em.sample(cigars, per_job, 10 ** 9, 5)
    assert sorted(order) == list(range(len(cigars))) and total == pytest.approx(sum(alen))


def test_trained_model_file_loads_back(tmp_path):
    h = em.hmm_randomise(api.hmm_constructEmpty(0.0, api.threeStateAsymmetric), 4)
    h.likelihood = -12345.678901234567
    path = tmp_path / "hmm.txt"
    em.write_model(h, str(path), running=[-20000.5, -15000.25, -12345.678901234567])
    lines = path.read_text().split("\n")
    assert len([l for l in lines if l]) == 3 and len(lines[2].split("\t")) == 3
    back = api.hmm_loadFromFile(str(path))
    assert back.type == api.threeStateAsymmetric and back.likelihood == h.likelihood
    assert list(back.transitions[:9]) == list(h.transitions[:9])
    assert list(back.emissions[:48]) == list(h.emissions[:48])
    api.hmm_getStateMachine(back)  # converts without complaint


def test_set_model_argument_checks():
    b = api.Batch(api.stateMachine5_construct(), emit=api.EMIT_EXPECT)
    with pytest.raises(api.CpecanError, match="states"):
        b.set_model(api.stateMachine3_construct())
    with pytest.raises(api.CpecanError, match="before upload"):
        b.set_model(api.stateMachine5_construct(api.fiveStateAsymmetric))
    b.close()


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_command_line_options_and_missing_files(tmp_path):
    assert os.path.exists(EXE), "build the command line with make -C cpecan_amd/csrc"
    assert _run("--help").returncode == 0
    res = _run("--alignments", "x")
    assert res.returncode != 0 and "--sequences" in res.stderr  # usage
    res = _run("--sequences", "a.fa", "--alignments", "x", "--modelType", "sevenState")
    assert res.returncode != 0 and "sevenState" in res.stderr
    res = _run("--sequences", "a.fa", "--alignments", "x", "--updateTheBand")
    assert res.returncode != 0 and "updateTheBand" in res.stderr
    res = _run("--sequences", "a.fa", "--alignments", "x", "--optionsToRealign", "--rescoreByIdentity")
    assert res.returncode != 0 and "optionsToRealign" in res.stderr
    missing = str(tmp_path / "missing.hmm")
    res = _run("--sequences", "a.fa", "--alignments", "x", "--inputModel", missing)
    assert res.returncode != 0 and "cannot load the input model" in res.stderr and missing in res.stderr
    missing_fa = str(tmp_path / "missing.fa")
    res = _run("--sequences", missing_fa, "--alignments", "x")
    assert res.returncode != 0 and "cannot open" in res.stderr and missing_fa in res.stderr
    fa = tmp_path / "a.fa"
    fa.write_text(">x\nACGT\n")
    missing_cigars = str(tmp_path / "missing.cigar")
    res = _run("--sequences", str(fa), "--alignments", missing_cigars)
    assert res.returncode != 0 and missing_cigars in res.stderr
    # a cigar that names a sequence nobody gave: refused before any GPU work
    cig = tmp_path / "in.cigar"
    cig.write_text("not a cigar\n")
    res = _run("--sequences", str(fa), "--alignments", str(cig), "--outputModel", str(tmp_path / "o.hmm"))
    assert res.returncode != 0 and "cigar" in res.stderr
