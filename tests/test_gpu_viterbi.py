"""Viterbi decoding on the GPU (cpk_viterbi.inl through cpecan_amd.viterbi) against its definition, tests/viterbi_model.py, on
the cases of tests/viterbi_cases.py: regions, states and ops integer for integer, every logP bit for bit; all cases in one
object and one run, under budgets that cut the run into launches, and under every kernel form, byte for byte; logP against the
forward probability; the exact-logAdd library in one child process; cpecan_align --viterbi."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import anchor_cases as ac
import viterbi_cases as vc
from cpecan_amd import api, realign, viterbi
from parity import LOG_TOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXACT = os.path.join(ROOT, "cpecan_amd", "libcpecan_hip_exact.so")
NEG_INF = float("-inf")


def _alone(c, sm=None, p=None, form=viterbi.FORM_AUTO):
    with viterbi.Viterbi(sm or vc.model_pair(c.model)[0], p or vc.lib_params(c)) as v:
        v.set_form(form)
        v.add(c.sx, c.sy, vc.anchors_of(c), c.ragged_left, c.ragged_right)
        v.run()
        return v.result(0), v.launch_forms()


_results = {}


def _result(c):
    """The case run alone, automatic form, default budget; computed once, never modified."""
    if c.name not in _results:
        _results[c.name] = _alone(c)
    return _results[c.name]


def _same_bytes(a, b, what):
    assert np.float64(a.logP).tobytes() == np.float64(b.logP).tobytes(), what
    assert len(a.regions) == len(b.regions), what
    for r, s in zip(a.regions, b.regions):
        assert tuple(r[:4]) == tuple(s[:4]) and tuple(r[5:]) == tuple(s[5:]), (what, r, s)
        assert np.float64(r.logP).tobytes() == np.float64(s.logP).tobytes(), (what, r, s)
    assert a.ops.dtype == b.ops.dtype and a.ops.tobytes() == b.ops.tobytes(), what


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_case_equals_the_model(name):
    """1: regions, startState, endState and ops integer for integer, every logP bit for bit; every path replayed on the host."""
    c = vc.case(name)
    got, forms = _result(c)
    print("%s: logP %r, %d regions, %d ops, forms %r" % (name, got.logP, len(got.regions), len(got.ops), forms))
    vc.assert_equals_model(c, got)
    sm = vc.model_pair(c.model)[0]
    for r, (sx, sy, rl, rr) in zip(got.regions, vc.region_inputs(c)):
        if r.startState < 0:
            assert r.logP == NEG_INF and r.endState == -1 and r.nOps == 0
            continue
        back = viterbi.replay(sm, sx, sy, rl, rr, r.startState, r.endState, got.ops[r.opOff:r.opOff + r.nOps])
        assert np.float64(back).tobytes() == np.float64(r.logP).tobytes(), (name, r, back)
    assert forms.launches == 1 and forms.lds + forms.global_ == len(got.regions)
    assert forms.global_ == (len(got.regions) if vc.widest(c) > viterbi.LDS_MAX_WIDTH else 0)


@pytest.mark.parametrize("config", ("c_segments", "d_inf_ragged", "e_dynamic", "r_three"))
def test_one_object_one_run_equals_one_at_a_time_under_every_budget(config):
    """2: offsets between problems and between launches.  An object holds one model and one set of parameters, so all inputs run
    under those of `config`; with the default budget, with one that makes at least three launches of the run and with exactly
    the largest region's bytes."""
    cfg = vc.case(config)
    sm, p = vc.model_pair(cfg.model)[0], vc.lib_params(cfg)
    alone = [_alone(c, sm, p)[0] for c in vc.cases()]
    _same_bytes(alone[vc.CASE_NAMES.index(config)], _result(cfg)[0], config)
    with viterbi.Viterbi(sm, p) as v:
        for i, c in enumerate(vc.cases()):
            assert v.add(c.sx, c.sy, vc.anchors_of(c), c.ragged_left, c.ragged_right) == i
        total = sum(v.info(i)["deviceBytes"] for i in range(v.n))
        n_regions = sum(v.info(i)["nRegions"] for i in range(v.n))
        v.run()  # the default budget
        assert v.launch_forms().launches == 1
        for i, c in enumerate(vc.cases()):
            _same_bytes(v.result(i), alone[i], (config, "default", c.name))
        largest = 1  # the largest single region's bytes: the refusals (host only) name them one after the other
        while True:
            v.set_budget(largest)
            try:
                v.run()
                break
            except api.CpecanError as e:
                m = re.search(r"\(-4\).*needs (\d+) bytes", str(e))
                assert m and int(m.group(1)) > largest, str(e)
                largest = int(m.group(1))
        for budget in (largest, max(largest, total // 3)):
            v.set_budget(budget)
            v.run()
            f = v.launch_forms()
            print("%s: budget %d of %d bytes: %r" % (config, budget, total, f))
            assert f.launches >= 3 and f.lds + f.global_ == n_regions, (config, budget, f)
            for i, c in enumerate(vc.cases()):
                _same_bytes(v.result(i), alone[i], (config, budget, c.name))
        v.set_budget(largest - 1)
        with pytest.raises(api.CpecanError, match=r"\(-4\).*needs %d bytes" % largest):
            v.run()


@pytest.mark.parametrize("form", viterbi.FORMS)
def test_every_kernel_form_gives_the_same_bytes(form):
    """3: the form forced on the small cases: launch_forms says it ran, and the bytes are those of the automatic form."""
    for name in vc.SMALL_CASE_NAMES:
        c = vc.case(name)
        got, forms = _alone(c, form=form)
        n = len(got.regions)
        assert forms == ((1, n, 0) if form == viterbi.FORM_LDS else (1, 0, n)), (name, forms)
        _same_bytes(got, _result(c)[0], (name, form))
    wide = vc.case("u_300x300")
    if form == viterbi.FORM_LDS:
        with pytest.raises(api.CpecanError, match=r"\(-1\).*LDS form"):
            _alone(wide, form=form)
    else:
        _same_bytes(_alone(wide, form=form)[0], _result(wide)[0], "u_300x300")


def test_logp_is_at_most_the_forward_probability():
    """4: every unsplit case with the static band: the best path holds no more than the sum over all paths."""
    checked = 0
    for c in vc.cases():
        got = _result(c)[0]
        if len(got.regions) != 1 or c.pkw.get("dynamicAnchorExpansion"):
            continue
        F = api.computeForwardProbability(c.sx, c.sy, vc.anchors_of(c), vc.lib_params(c), vc.model_pair(c.model)[0], c.ragged_left,
                                          c.ragged_right)
        print("%s: logP %r, forward %r" % (c.name, got.logP, F))
        if c.name == "p_no_path":
            assert got.logP == NEG_INF and F == NEG_INF
        else:
            assert np.isfinite(got.logP) and got.logP <= F + LOG_TOL * max(1.0, abs(F)), (c.name, got.logP, F)
        checked += 1
    assert checked >= 15


def test_exact_build_gives_the_same_bytes():
    """5: one child process on the exact-logAdd library."""
    assert os.path.exists(EXACT), "%s is missing: __graft_entry__.build() makes it (`make -C cpecan_amd/csrc exact`)" % EXACT
    env = dict(os.environ, CPECAN_LIB=EXACT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "viterbi_exact_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "viterbi results equal" in r.stdout


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records.items():
            f.write(">%s some description\n" % name)
            s = s.decode()
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")


def test_cpecan_align_viterbi(tmp_path):
    """6: three targets x three queries, one query reverse-complemented, --strand both: the cigars are those built here from
    viterbi.py results on the same anchors; the two refusals."""
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    pairs = [ac.random_pair(61, 700), ac.random_pair(62, 300), ac.random_pair(63, 150)]
    targets = {"t%d" % i: q[0] for i, q in enumerate(pairs)}
    queries = {"q0": api.reverse_complement(pairs[0][1]), "q1": pairs[1][1], "q2": pairs[2][1]}
    _write_fasta(tmp_path / "target.fa", targets)
    _write_fasta(tmp_path / "query.fa", queries)
    files = [str(tmp_path / "target.fa"), str(tmp_path / "query.fa")]
    r = subprocess.run([exe, "--viterbi", "--strand", "both"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    order = [(q, t) for q in queries for t in targets]
    assert len(lines) == 9
    problems = [(targets[t], queries[q]) for q, t in order]
    runs, _, strands = api.find_anchor_runs_many_stranded(problems, strand="both")
    sm, p = api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct()
    minus = [s["strand"] == "minus" for s in strands]
    assert minus[0] and not minus[4] and not minus[8]  # (q0, t0) is the related pair whose query was reverse-complemented
    with viterbi.Viterbi(sm, p) as v:
        for (sx, sy), rr, m in zip(problems, runs, minus):
            anchors = [(int(x) + i, int(y) + i, int(e)) for x, y, n, e in rr for i in range(int(n))]
            v.add(sx, api.reverse_complement(sy) if m else sy, anchors, True, True)
        v.run()
        for i, (line, (q, t)) in enumerate(zip(lines, order)):
            res = v.result(i)
            want = realign.Cigar.from_aligned_pairs(t, q, res.logP, len(targets[t]), len(queries[q]), viterbi.pairs_of(res).tolist(),
                                                    strand2=not minus[i]).format()
            assert line == want, (q, t)
            assert np.array_equal(viterbi.pairs_of(res), v.pairs(i))
    f = lines[0].split()
    assert f[1:5] == ["q0", str(len(queries["q0"])), "0", "-"] and f[5:9] == ["t0", "0", str(len(targets["t0"])), "+"]
    assert sum(int(n) for op, n in zip(f[10::2], f[11::2]) if op == "M") > 500  # the related pair is aligned end to end
    for extra in (["--local"], ["--adaptiveBand", "1", "--minEdgeScore", "100"]):
        r = subprocess.run([exe, "--viterbi"] + extra + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and "--viterbi does not go with" in r.stderr
