"""Gangs: the two launches of a split class as workgroups of several waves that share one copy of the LDS tables
(cpk_sweep.inl "GANG"; CPECAN_GANG=n forces n waves per workgroup, 0 forbids them).  A gang changes which wave runs where
and where its LDS lies, nothing else: every case compares what CPECAN_GANG=n gives with what CPECAN_GANG=0 gives for
equality of bits -- the result list of every problem, and the sweeps' debug buffers where the parity tests read them --
and one problem per shape against the oracle.  The shapes are the smallest at which a gang can go wrong: fewer regions
than waves (most waves of a workgroup find the queue empty at once, while their siblings work on), more items than waves,
every size of the private block around the 64-lane groups, a band that turns back, candidates that bypass the stage, both
state counts, and a batch with gangs alive beside one without."""
import json
import os
import re
import subprocess
import sys

if __name__ == "__main__":  # the child of test_fewer_regions_than_waves
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
from cpecan_amd import api
from cpecan_amd.workload import make_pair
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 11)
SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)  # a traceback every 42 diagonals of a narrow band
# A diagonal is a traceback point only if it has at most 2 * diagonalExpansion + 1 cells (pairwiseAligner.c:792-793).  Under the
# default expansion of 20 an unanchored region wider than 41 cells therefore has two segments, one across all its wide
# diagonals; under 130 every diagonal of the shapes below is a permitted point and a region has a segment every 42 diagonals.
WIDTH_EXPANSIONS = (20, 130)
# every region in a wide class (no packed kernel), every class with a traceback in two launches; CPECAN_ABS at its default
BASE_ENV = {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1", "CPECAN_TRACE_HOST": "1"}


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


def _problem(p):
    return tuple(p) + (False, False) if len(p) == 3 else tuple(p)


def _run(mtype, problems, pkw, debug_cells=None):
    """Results of every problem (and, with debug_cells = (cells, diagonals) of problem 0, its debug buffers)."""
    with api.Batch(_sm(mtype), api.pairwiseAlignmentBandingParameters_construct(**pkw), debug=debug_cells is not None) as b:
        for p in problems:
            b.add(*_problem(p))
        b.upload()
        b.run()
        b.download()
        out = [b.result(i) for i in range(len(problems))]
        dbg = b.debug_fetch(0, *debug_cells) if debug_cells else None
    return out, dbg


def _gang_words(err):
    """[(forward gang, traceback gang)] of the class lines CPECAN_TRACE_HOST wrote: 0 where the launch has one wave per workgroup."""
    out = []
    for line in re.findall(r"^cpecan class \d+:.*$", err, re.M):
        f = re.search(r"forward launch: gang of (\d+)", line)
        t = re.search(r"traceback launch: gang of (\d+)", line)
        out.append((int(f.group(1)) if f else 0, int(t.group(1)) if t else 0))
    return out


def _with_gang(monkeypatch, capfd, n, mtype, problems, pkw, debug_cells=None):
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("CPECAN_GANG", str(n))
    capfd.readouterr()
    out = _run(mtype, problems, pkw, debug_cells)
    words = _gang_words(capfd.readouterr().err)
    assert words, "no class line"
    if n == 0:
        assert all(w == (0, 0) for w in words), words
    else:  # both launches of every class really ran as gangs of n
        assert all(w == (n, n) for w in words), (n, words)
    return out


def _assert_same_lists(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "%s: problem %d differs" % (what, i)


def _check(monkeypatch, capfd, mtype, problems, pkw, sizes=SIZES, oracle=(0,), emits=True):
    """CPECAN_GANG=n against CPECAN_GANG=0, list for list; the problems `oracle` of the last gang against the oracle."""
    (want, _) = _with_gang(monkeypatch, capfd, 0, mtype, problems, pkw)
    assert any(len(w) for w in want) or not emits, "nothing was emitted: the case compares empty lists"
    for n in sizes:
        (got, _) = _with_gang(monkeypatch, capfd, n, mtype, problems, pkw)
        _assert_same_lists(got, want, "gang of %d" % n)
    om, op = ob.model(mtype), ob.params(**pkw)
    for i in oracle:
        sx, sy, a, rl, rr = _problem(problems[i])
        assert_pairs_match(got[i], ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)


def _seq(n, seed):
    return tc.seq(n, seed)


def _width_problems(width):
    """Unanchored pairs (the whole matrix is the band) whose widest diagonal has `width` cells: min(lX, lY) + 1."""
    m = width - 1
    return [(_seq(m, 1), _seq(m, 2), ()), (_seq(m + 17, 3), _seq(m, 4), ()), (_seq(m, 5), _seq(m + 40, 6), ())]


# ---- the private block's size and alignment change with the widest diagonal; both state counts ----
@pytest.mark.parametrize("width,mtype", [(1, 0), (63, 0), (64, 2), (65, 0), (65, 2), (127, 0), (128, 2), (129, 0), (157, 0), (157, 2)])
def test_widest_diagonals_around_the_groups(width, mtype, monkeypatch, capfd):
    """Two runs (WIDTH_EXPANSIONS): two segments per region, whose hand-off lies on a diagonal of at most 41 cells, and many
    segments per region -- at least (lX + lY) / 50, tests/test_match_cases_cpu.py --, which hand over on the widest diagonals."""
    # (diagonals of one cell: one of the two sequences is empty, the sweeps run and there is no match cell to emit)
    for expansion in WIDTH_EXPANSIONS:
        _check(monkeypatch, capfd, mtype, _width_problems(width), dict(threshold=0.01, diagonalExpansion=expansion, **SHORT), oracle=(1,),
               emits=width > 1)


# ---- fewer regions than waves: most waves of the workgroup find the queue empty at once ----
def _few_problems(n_regions):
    return [make_pair(3, i, 600, 10) for i in range(n_regions)]


FEW_PKW = dict(diagonalExpansion=10, **SHORT)


def _child(n_regions):
    """Runs in a process of its own (see below): the lists under gangs of eleven and without gangs, as JSON on stdout."""
    out = {}
    for n in (0, 11):
        os.environ.update(BASE_ENV)
        os.environ["CPECAN_GANG"] = str(n)
        res, _ = _run(0, _few_problems(n_regions), FEW_PKW)
        out[str(n)] = [r.tolist() for r in res]
    sys.stdout.write("RESULT " + json.dumps(out) + "\n")


@pytest.mark.parametrize("n_regions", [1, 5])
def test_fewer_regions_than_waves(n_regions):
    """One region and five, gangs of eleven: in the forward launch ten (six) waves of the workgroup leave at once, and
    must not be waited for by the others at any barrier behind the first.  A wave stuck at a barrier would hang the
    launch, so the batch runs in a child process under a time limit of 60 s; it takes about a second."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(n_regions)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    words = _gang_words(out.stderr)
    assert (11, 11) in words and (0, 0) in words, words
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res["11"]) == n_regions and any(len(r) for r in res["11"])
    assert res["11"] == res["0"]
    om, op = ob.model(0), ob.params(**FEW_PKW)
    sx, sy, a = _few_problems(n_regions)[0]
    assert_pairs_match(np.array(res["11"][0], dtype=np.int32).reshape(-1, 3), ob.aligned_pairs(om, sx, sy, a, op), threshold=op.threshold)


# ---- more items than waves: the waves of one workgroup are at different items ----
def test_more_items_than_waves(monkeypatch, capfd):
    problems = [make_pair(11, i, 300, 20) for i in range(40)]
    _check(monkeypatch, capfd, 0, problems, dict(diagonalExpansion=20, minDiagsBetweenTraceBack=100, traceBackDiagonals=20), oracle=(0, 39))


# ---- a band that turns back: the sweep re-bases its positions (absRebase) inside a gang ----
def test_band_that_turns_back(monkeypatch, capfd):
    case = tc.chain_case()
    _check(monkeypatch, capfd, case.mtype, list(case.problems), case.pkw, oracle=(0, 1))


# ---- threshold 0: every cell is a candidate, more than the stage holds -- they bypass it ----
def test_threshold_zero_bypasses_the_stage(monkeypatch, capfd):
    problems = [(_seq(64, 11), _seq(64, 12), ())]
    _check(monkeypatch, capfd, 0, problems, dict(threshold=0.0, **SHORT))


# ---- the debug buffers: F + B of every emitted cell, the total used on every emitted diagonal ----
@pytest.mark.parametrize("mtype,pair,pkw", [
    (0, (3, 1, 600, 10), dict(diagonalExpansion=10, **SHORT)),
    (2, (2, 0, 1000, 50), dict(diagonalExpansion=50)),
])
def test_debug_buffers_are_the_same_bits(mtype, pair, pkw, monkeypatch, capfd):
    sx, sy, a = make_pair(*pair)
    _, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), False, False)
    cells = (tr["n_cells"], tr["n_diagonals"])
    want, (fb0, tot0) = _with_gang(monkeypatch, capfd, 0, mtype, [(sx, sy, a)], pkw, cells)
    assert np.isfinite(fb0).any() and np.isfinite(tot0).any()
    for n in SIZES:
        got, (fb, tot) = _with_gang(monkeypatch, capfd, n, mtype, [(sx, sy, a)], pkw, cells)
        _assert_same_lists(got, want, "gang of %d" % n)
        assert fb.tobytes() == fb0.tobytes() and tot.tobytes() == tot0.tobytes(), "gang of %d: debug buffers differ" % n


# ---- two batches alive at once, one with gangs and one without: the per-wave scratch slots are disjoint ----
def test_a_gang_batch_beside_a_plain_one(monkeypatch, capfd):
    pa = [make_pair(21, i, 400, 20) for i in range(12)]
    pb = [make_pair(22, i, 500, 10) for i in range(9)]
    pkw_a, pkw_b = dict(diagonalExpansion=20, **SHORT), dict(diagonalExpansion=10, **SHORT)
    (want_a, _) = _with_gang(monkeypatch, capfd, 0, 0, pa, pkw_a)
    (want_b, _) = _with_gang(monkeypatch, capfd, 0, 2, pb, pkw_b)
    with api.Batch(_sm(0), api.pairwiseAlignmentBandingParameters_construct(**pkw_a)) as a, \
            api.Batch(_sm(2), api.pairwiseAlignmentBandingParameters_construct(**pkw_b)) as b:
        for p in pa:
            a.add(*p)
        for p in pb:
            b.add(*p)
        capfd.readouterr()
        monkeypatch.setenv("CPECAN_GANG", "11")  # (the plan reads the environment at upload)
        a.upload()
        assert _gang_words(capfd.readouterr().err) == [(11, 11)]
        monkeypatch.setenv("CPECAN_GANG", "0")
        b.upload()
        assert _gang_words(capfd.readouterr().err) == [(0, 0)]
        for _ in range(2):  # both in flight, twice: the second round runs over the scratch of the first
            a.run()
            b.run()
            a.download()
            b.download()
            _assert_same_lists([a.result(i) for i in range(len(pa))], want_a, "the batch with gangs")
            _assert_same_lists([b.result(i) for i in range(len(pb))], want_b, "the batch without")


if __name__ == "__main__":
    _child(int(sys.argv[1]))
