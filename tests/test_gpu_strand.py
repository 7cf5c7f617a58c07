"""Strand on the GPU against its definition (tests/strand_model.py): runs, statistics, strand and both scores integer for
integer; minus problems against today's forward call on the reverse-complemented query; aligned pairs of a minus pair
against the forward pair, exactly; the ENCODE pairs with the query reverse-complemented; cpecan_align --strand both."""
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import reference_cases as rc
import strand_model as sm
from cpecan_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("hits", "hsps", "chained", "runs", "anchorColumns", "subProblems", "largestGapTop", "largestGap", "capped")


def _same(got_runs, got_stats, got_strand, sx, sy, what, **kw):
    """BOTH on (sx, sy) equals the model; a minus result also equals today's forward call on (sx, rc(sy)): same array."""
    want_runs, want_stats, want_strand = sm.find_anchor_runs_stranded(sx, sy, "both", **kw)
    assert got_strand == want_strand, what
    assert np.array_equal(np.asarray(got_runs, dtype=np.int64).reshape(-1, 4), want_runs), what
    assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, what
    assert 2 * want_stats["hsps"] <= am.default_params()["maxHsps"], "the input comes too close to the HSP cap"
    assert got_stats["kernelMs"] > 0.0, what
    if got_strand["strand"] == "minus":
        fwd, fst = api.find_anchor_runs(sx, sm.rc(sy), **kw)
        assert np.array_equal(got_runs, fwd), what
        assert {k: int(got_stats[k]) for k in COUNTS} == {k: int(fst[k]) for k in COUNTS}, what
    return want_strand


def _both(sx, sy, **kw):
    runs, stats, strands = api.find_anchor_runs_many_stranded([(sx, sy)], strand="both", **kw)
    return runs[0], stats[0], strands[0]


def _encode(name):
    return rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)


@pytest.mark.parametrize("length", [600, 1500, 5000, 20000])
@pytest.mark.parametrize("flip", [False, True])
def test_random_pairs_equal_the_model(length, flip):
    sx, sy = ac.random_pair(length, length)
    sy = sm.rc(sy) if flip else sy
    res = _same(*_both(sx, sy), sx, sy, (length, flip))
    assert res["strand"] == ("minus" if flip else "plus") and max(res["scorePlus"], res["scoreMinus"]) > 0


def test_masked_pairs_equal_the_model():
    for index, length, flip in ((1, 2000, True), (2, 6000, False), (2, 6001, True)):
        sx, sy = ac.masked_pair(index, length)                    # 6001: an odd length, nibbles straddle bytes
        sy = sm.rc(sy) if flip else sy
        res = _same(*_both(sx, sy), sx, sy, (index, length))
        assert res["strand"] == ("minus" if flip else "plus")


@pytest.mark.parametrize("repeatMask", [500 * 500, 10 ** 9])
@pytest.mark.parametrize("flip", [False, True])
def test_insertion_pair_recursion_equals_the_model(repeatMask, flip):
    sx, sy = ac.insertion_pair()
    sy = sm.rc(sy) if flip else sy
    got = _both(sx, sy, repeatMaskMatrixBiggerThanThis=repeatMask)
    res = _same(*got, sx, sy, (repeatMask, flip), repeatMaskMatrixBiggerThanThis=repeatMask)
    assert got[1]["subProblems"] > 0 and res["strand"] == ("minus" if flip else "plus")
    assert min(res["scorePlus"], res["scoreMinus"]) == 876       # the wrong strand chains a little


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_encode_pairs_equal_the_model(name):
    sx, sy, _, _ = _encode(name)
    sy = sm.rc(sy)
    res = _same(*_both(sx, sy), sx, sy, name)
    assert res["strand"] == "minus" and res["scorePlus"] > 0


def test_batch_of_256_mixed_problems_equals_the_model_problem_by_problem():
    problems = [(sx, sm.rc(sy) if i % 2 else sy) for i, (sx, sy) in enumerate(ac.mixed_batch(256))]
    runs, stats, strands = api.find_anchor_runs_many_stranded(problems, strand="both")
    assert len(runs) == len(stats) == len(strands) == 256
    small = 0
    for i, (sx, sy) in enumerate(problems):
        want_runs, want_stats, want_strand = sm.find_anchor_runs_stranded(sx, sy, "both")
        assert strands[i] == want_strand and want_strand["strand"] == ("minus" if i % 2 else "plus"), i
        assert np.array_equal(runs[i], want_runs), i
        assert {k: int(stats[i][k]) for k in COUNTS} == {k: int(want_stats[k]) for k in COUNTS}, i
        assert 2 * want_stats["hsps"] <= am.default_params()["maxHsps"]
        small += len(sx) * len(sy) <= 500 * 500
    assert 0 < small < 256
    # every minus problem: what today's entry point returns for (sX, rc(sY)), in one batch
    minus = [i for i in range(256) if i % 2]
    fwd, fst = api.find_anchor_runs_many([(problems[i][0], sm.rc(problems[i][1])) for i in minus])
    for k, i in enumerate(minus):
        assert np.array_equal(runs[i], fwd[k]), i
        assert {c: int(stats[i][c]) for c in COUNTS} == {c: int(fst[k][c]) for c in COUNTS}, i


def test_plus_through_the_new_entry_point_equals_the_old_one():
    problems = ac.mixed_batch(64) + [ac.insertion_pair(), (b"", b"ACGT")]
    old_runs, old_stats = api.find_anchor_runs_many(problems)
    new_runs, new_stats, strands = api.find_anchor_runs_many_stranded(problems, strand="plus")
    for i, (sx, sy) in enumerate(problems):
        assert np.array_equal(old_runs[i], new_runs[i]), i
        assert {k: old_stats[i][k] for k in COUNTS} == {k: new_stats[i][k] for k in COUNTS}, i
        searched = len(sx) * len(sy) > 500 * 500
        assert strands[i]["strand"] == "plus" and strands[i]["scoreMinus"] == -1
        assert strands[i]["scorePlus"] == (sm.strand_score(sx, sy) if searched else -1), i
    # MINUS forces the orientation and scores only that
    sx, sy = ac.random_pair(5000, 5000)
    runs, stats, strands = api.find_anchor_runs_many_stranded([(sx, sy), (sx, sm.rc(sy))], strand="minus")
    want0, wst0, res0 = sm.find_anchor_runs_stranded(sx, sy, "minus")
    want1, wst1, res1 = sm.find_anchor_runs_stranded(sx, sm.rc(sy), "minus")
    assert strands == [res0, res1] and res0["scorePlus"] == res1["scorePlus"] == -1
    assert np.array_equal(runs[0], want0) and np.array_equal(runs[1], want1) and len(want1) > len(want0)
    assert np.array_equal(api.find_anchor_runs(sx, sm.rc(sy), strand="minus")[0], api.find_anchor_runs(sx, sy)[0])
    assert np.array_equal(api.find_anchor_runs(sx, sm.rc(sy), strand="both")[0], api.find_anchor_runs(sx, sy)[0])


def test_a_tie_and_a_pair_under_the_size_limit():
    sx, sy = ac.random_pair(61, 300)[0], ac.random_pair(62, 300)[1]
    runs, st, res = _both(sx, sy)
    assert res == dict(strand="plus", scorePlus=0, scoreMinus=0) and len(runs) == 0
    sx, sy = ac.random_pair(1, 400)
    runs, st, res = _both(sx, sm.rc(sy))
    assert res == dict(strand="minus", scorePlus=0, scoreMinus=23186) and len(runs) == 0 and st["hits"] == 0
    assert _both(b"", b"ACGT")[2] == dict(strand="plus", scorePlus=0, scoreMinus=0)


def test_get_aligned_pairs_stranded_equals_the_forward_pair_exactly():
    sm5 = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    short = ac.random_pair(41, 400)
    for sx, sy in ((short[0][:380], short[1][:380]), ac.random_pair(31, 5000)):
        want = api.getAlignedPairs(sm5, sx, sy, p, True, True)
        assert len(want) > 100
        got, strand, scores = api.getAlignedPairsStranded(sm5, sx, sm.rc(sy), p, True, True)
        assert strand == "minus" and scores[1] > scores[0] >= 0
        assert np.array_equal(got, want)
        got, strand, scores = api.getAlignedPairsStranded(sm5, sx, sy, p, True, True)
        assert strand == "plus" and np.array_equal(got, want)
        got, strand, scores = api.getAlignedPairsStranded(sm5, sx, sm.rc(sy), p, True, True, strand="minus")
        assert strand == "minus" and np.array_equal(got, want)


def _run(batch):
    batch.upload()
    batch.run()
    batch.download()


def test_add_many_unanchored_both_equals_add_many_runs_on_reverse_complemented_copies():
    sm5 = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    base = ac.mixed_batch(12) + [ac.insertion_pair()]
    given = [(sx, sm.rc(sy) if i % 3 != 1 else sy) for i, (sx, sy) in enumerate(base)]
    # REWEIGHT | ORDERED on the match emitter; MEA | LEFT_SHIFT (getShiftedMEAAlignment: reads the letters) on the indel one
    for emit, flags in ((api.EMIT_MATCH, api.POST_REWEIGHT | api.POST_ORDERED), (api.EMIT_INDEL, api.POST_MEA | api.POST_LEFT_SHIFT)):
        with api.Batch(sm5, p, emit) as a, api.Batch(sm5, p, emit) as b:
            a.set_post(flags, 0.5)
            b.set_post(flags, 0.5)
            _, stats = a.add_many_unanchored([(sx, sy, True, True) for sx, sy in given], strand="both")
            b.add_many_runs([(sx, sy, am.runs_to_anchors(am.find_anchor_runs(sx, sy)[0]), True, True) for sx, sy in base])
            _run(a)
            _run(b)
            for i in range(len(base)):
                assert a.problem_strand(i) == stats[i]["strand"] == ("minus" if i % 3 != 1 else "plus"), i
                for which in ((0, 3) if emit == api.EMIT_MATCH else (0, 1, 2, 3)):
                    assert np.array_equal(a.result(i, which), b.result(i, which)), (i, which)
            assert sum(len(a.result(i, 3)) for i in range(len(base))) > 1000


@pytest.mark.parametrize("name", ["dog", "mouse"])
def test_encode_reverse_complemented_from_sequences_alone(name):
    sx, sy, _, true_pairs = _encode(name)
    sm5 = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=20)
    fwd = api.filterPairwiseAlignmentToMakePairsOrdered(api.getAlignedPairs(sm5, sx, sy, p), sx, sy, 0.5)
    want = rc.sensitivity_specificity(fwd, true_pairs)
    ry = sm.rc(sy)                                               # the query as it lies in memory: the other strand
    pairs, strand, scores = api.getAlignedPairsStranded(sm5, sx, ry, p)
    assert strand == "minus" and scores[1] > scores[0] > 0
    # the pairs are in the coordinates of (sx, rc(ry)); y -> lY - 1 - y takes them, and the true pairs, to those of ry
    out = api.filterPairwiseAlignmentToMakePairsOrdered(pairs, sx, sm.rc(ry), 0.5)
    lY = len(ry)
    mapped = [(s, x, lY - 1 - y) for s, x, y in np.asarray(out).reshape(-1, 3).tolist()]
    got = rc.sensitivity_specificity(mapped, {(x, lY - 1 - y) for x, y in true_pairs})
    print("encode %s reverse-complemented: sensitivity %.4f specificity %.4f (forward %.4f %.4f)" % ((name,) + got + want))
    assert got == want


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for k, s in seqs.items():
            f.write(">%s some description\n" % k)
            s = s.decode()
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")


def test_cpecan_align_strand_both_two_by_two(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    realign_exe = os.path.join(ROOT, "cpecan_amd", "cpecan_realign")
    targets = {"t_long": ac.random_pair(51, 1800)[0], "t_short": ac.random_pair(52, 300)[0]}
    forward = {"q_long": ac.random_pair(51, 1800)[1], "q_short": ac.random_pair(52, 300)[1]}
    queries = {"q_long": sm.rc(forward["q_long"]), "q_short": forward["q_short"]}
    _write_fasta(tmp_path / "target.fa", targets)
    _write_fasta(tmp_path / "query.fa", queries)
    _write_fasta(tmp_path / "forward.fa", forward)

    def run(*args):
        r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return [l for l in r.stdout.splitlines() if l.strip()]

    both = run("--strand", "both", str(tmp_path / "target.fa"), str(tmp_path / "query.fa"))
    plain = run(str(tmp_path / "target.fa"), str(tmp_path / "query.fa"))
    fwd = run(str(tmp_path / "target.fa"), str(tmp_path / "forward.fa"))
    assert plain == run("-s", "plus", str(tmp_path / "target.fa"), str(tmp_path / "query.fa"))
    assert len(both) == len(plain) == len(fwd) == 4
    order = [(q, t) for q in queries for t in targets]
    minus_lines = 0
    for line, plain_line, fwd_line, (q, t) in zip(both, plain, fwd, order):
        f, g = line.split(), fwd_line.split()
        if (q, t) == ("q_long", "t_long"):                       # the one related pair whose query was reverse-complemented
            assert f[1:5] == [q, str(len(queries[q])), "0", "-"] and f[5:9] == [t, "0", str(len(targets[t])), "+"]
            assert f[10:] == g[10:] and g[4] == "+"              # the operations of the forward cigar of (target, rc(query))
            minus_lines += 1
        elif f[4] == "+":
            assert line == plain_line                            # byte-identical to a run without the option
        else:                                                    # an unrelated pair that chains a little more on minus
            assert f[2:5] == [str(len(queries[q])), "0", "-"]
            minus_lines += 1
    assert minus_lines >= 1 and both[3] == plain[3] == fwd[3]    # q_short / t_short: related, forward
    # the whole output goes through cpecan_realign
    r = subprocess.run([realign_exe, str(tmp_path / "target.fa"), str(tmp_path / "query.fa")], input="\n".join(both) + "\n",
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = [l for l in r.stdout.splitlines() if l.startswith("cigar:")]
    assert len(out) == 4 and [l.split()[4] for l in out] == [l.split()[4] for l in both]
