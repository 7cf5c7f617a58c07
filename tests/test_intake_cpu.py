"""What the add calls pack into a batch (cpecan_host.c: count, reserve, write), pinned without a GPU by
cpk_batch_intake_digest: FNV-1a hashes of (a) the problem records, (b) the region records, (c) the symbols, (d) the anchor or
run values with runForm and anchorStride, (e) the raw letters.  A region's runOff / nRuns exist only in a batch that keeps
runs, so they are hashed into (d), not (b): (b) is then the same whichever form the anchors are held in.

The batches: 70 problems of make_realign_batch(seed, 70, 30, 600) (the OpenMP path) or the first 5 (the serial path), and
behind them a pair with lX == 0, one with lY == 0, one without anchors and one whose anchors start in column 0 and whose
letters are not all upper-case A/C/G/T, and three pairs with an anchor every 50 columns.  splitMatrixBiggerThanThis=10 cuts
the sparsely anchored pairs into many rectangles with anchors on both sides of every cut; of the realign-style problems, whose
anchors leave few gaps of more than 10 cells, the seed is one with which one of the first 5 is cut.

tests/golden/intake_digests.json was made with the library of the commit BEFORE the intake was staged, with only
cpk_batch_intake_digest added to it (the hook reads, and changes nothing):
    CPECAN_LIB=<that library> python tests/test_intake_cpu.py > tests/golden/intake_digests.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpecan_amd import api  # noqa: E402
from cpecan_amd.workload import make_pair, make_realign_batch  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intake_digests.json")
SEED, E, SPLIT = 21, 4, 10
SIZES = (70, 5)


def _extras():
    sx, sy, _ = make_pair(SEED, 1000, 40, E)
    col0 = np.array([(i, i, E) for i in range(12)] + [(20, 21, E), (21, 22, E)], dtype=np.int64)
    return [(b"", b"ACGTTGCA", ()), (b"TTGACA", b"", ()), (sx, sy, ()),
            (b"acgtNnACGTRYacgtACGTACGTAC", b"acgtNnACGTRYacgtACGTAGCGTAC", col0)] + [make_pair(SEED, 2000 + i, 250, E) for i in range(3)]


_PROBLEMS = {}


def problems(n):
    """The n realign-style problems and the seven extras; made once."""
    if n not in _PROBLEMS:
        _PROBLEMS[n] = make_realign_batch(SEED, 70, 30, 600, expansion=E)[:n] + _extras()
    return _PROBLEMS[n]


def _digest(b):
    f = api.lib().cpk_batch_intake_digest
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 5)()
    assert f(b._h, out) == 0, api.lib().cpecan_last_error()
    return [int(x) for x in out]


def _batch(stride3=False):
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=E, splitMatrixBiggerThanThis=SPLIT,
                                                         dynamicAnchorExpansion=int(stride3))
    return api.Batch(api.stateMachine5_construct(), p, emit=api.EMIT_MATCH)


def _is_minus(i):
    return i % 3 == 1


def _add(b, probs, form, first=0):
    """One add call: 'triples' (cpecan_batch_add_many), 'runs' (cpecan_batch_add_many_runs) or 'stranded'
    (cpecan_batch_add_many_runs_stranded, every third problem on the minus strand).  Returns the call's return value."""
    if form == "triples":
        arr, n, _keep = b.prepare_problems(probs)
        return api.lib().cpecan_batch_add_many(b._h, arr, n)
    arr, n, _keep = b.prepare_problems_runs(probs)
    if form == "runs":
        return api.lib().cpecan_batch_add_many_runs(b._h, arr, n)
    minus = (C.c_int32 * max(1, n))(*[int(_is_minus(first + i)) for i in range(n)])
    return api.lib().cpecan_batch_add_many_runs_stranded(b._h, arr, minus, n)


def intake(form, n, stride3=False, calls=None):
    """The five digests of a batch that received problems(n) in `form`, in calls of the given sizes (default: one call)."""
    probs = problems(n)
    with _batch(stride3) as b:
        at = 0
        for size in calls or (len(probs),):
            assert _add(b, probs[at:at + size], form, at) == at, api.lib().cpecan_last_error()
            at += size
        assert at == len(probs)
        return _digest(b)


def all_digests():
    """Every batch of the golden file, in the environment it is read in (CPECAN_KEEP_RUNS unset or 0)."""
    out = {}
    for n in SIZES:
        for form in ("triples", "runs", "stranded"):
            for stride3 in (False, True):
                out["%s_%d%s" % (form, n, "_stride3" if stride3 else "")] = intake(form, n, stride3)
    return out


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("CPECAN_KEEP_RUNS", raising=False)
    monkeypatch.delenv("CPECAN_THREADS", raising=False)


def test_the_matrix_has_what_it_is_meant_to_have():
    probs = problems(70)
    assert len(probs) == 77 and len(problems(5)) == 12  # 77 >= 64: the parallel loops; 12: the serial ones
    assert len(probs[70][0]) == 0 and len(probs[71][1]) == 0 and len(probs[72][2]) == 0 and tuple(probs[73][2][0][:2]) == (0, 0)
    cut = [len(api.getSplitPoints(a, len(sx), len(sy), SPLIT, False, False)) for sx, sy, a in probs]
    assert sum(c > 1 for c in cut[:5]) >= 1 and cut[70] == 1 and cut[71] == 1 and cut[72] == 2 and cut[73] >= 2
    assert all(c >= 4 for c in cut[74:])  # anchors fall on both sides of a cut


def test_digests_are_the_parents():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = all_digests()
    assert sorted(got) == sorted(want["default"])
    assert got == want["default"]


def test_digests_without_kept_runs_are_the_parents(monkeypatch):
    monkeypatch.setenv("CPECAN_KEEP_RUNS", "0")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert all_digests() == want["keep_runs_0"]


@pytest.mark.parametrize("n", SIZES)
def test_runs_and_triples_pack_the_same(n, monkeypatch):
    t, r = intake("triples", n), intake("runs", n)
    assert t[:3] == r[:3] and t[4] == r[4]
    assert t[3] != r[3]  # one batch holds anchors, the other runs
    s = intake("stranded", n)
    monkeypatch.setenv("CPECAN_KEEP_RUNS", "0")
    assert intake("runs", n) == t  # (d) as well: the runs were expanded to the same anchors
    s0 = intake("stranded", n)
    assert s0[:3] == s[:3] and s0[4] == s[4] and s0 != t


@pytest.mark.parametrize("n", SIZES)
def test_stride_three_expands_runs_to_the_triples(n):
    assert intake("runs", n, stride3=True) == intake("triples", n, stride3=True)
    assert intake("runs", n, stride3=True)[3] != intake("triples", n)[3]


@pytest.mark.parametrize("form", ["triples", "runs", "stranded"])
def test_threads_and_calls_do_not_matter(form, monkeypatch):
    want = intake(form, 70)
    for threads in ("1", "16"):
        monkeypatch.setenv("CPECAN_THREADS", threads)
        assert intake(form, 70) == want
        assert intake(form, 70, calls=(30, 47)) == want  # 30 + 40 and the extras: both calls serial
        assert intake(form, 70, calls=(70, 7)) == want  # a parallel call, then a serial one
    assert intake(form, 5, calls=(2, 10)) == intake(form, 5)


def test_a_batch_that_began_with_triples_keeps_anchors():
    probs = problems(70)
    want = intake("triples", 70)
    with _batch() as b:
        assert _add(b, probs[:30], "triples") == 0
        assert _add(b, probs[30:], "runs") == 30
        assert _digest(b) == want  # runForm 0 is part of (d)
    with _batch() as b:  # and the other way round: runs stay runs, a triple is a run of one
        assert _add(b, probs[:30], "runs") == 0
        assert _add(b, probs[30:], "triples") == 30
        got, runs = _digest(b), intake("runs", 70)
        assert got[:3] == runs[:3] and got[4] == runs[4]


@pytest.mark.parametrize("form", ["triples", "runs", "stranded"])
@pytest.mark.parametrize("first,bad", [(30, 17), (4, 40)])  # a serial call of 47 and a parallel one of 73
def test_a_failed_call_names_its_first_bad_problem_and_leaves_the_batch(form, first, bad):
    probs = list(problems(70))
    want = intake(form, 70)
    with _batch() as b:
        assert _add(b, probs[:first], form) == 0
        before = _digest(b)
        call = list(probs[first:])
        for k in (bad, bad + 9):  # two bad problems: anchors that do not increase
            sx, sy, a = call[k]
            call[k] = (sx, sy, np.concatenate([a[:3], a[2:3], a[3:]]))
        assert _add(b, call, form, first) == -1
        assert ("problem %d of the call" % bad) in api.lib().cpecan_last_error().decode()
        assert _digest(b) == before
        assert _add(b, probs[first:], form, first) == first
        assert _digest(b) == want


if __name__ == "__main__":
    os.environ.pop("CPECAN_KEEP_RUNS", None)
    default = all_digests()
    os.environ["CPECAN_KEEP_RUNS"] = "0"
    json.dump({"default": default, "keep_runs_0": all_digests()}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
