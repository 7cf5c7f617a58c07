"""The pass behind every refresh diagonal of the traceback (cpk_sweep.inl: dotGroups / refreshDots in tracebackAbs, the same
pass in traceback): the per-cell dot products that foldTotals() folds into the total probability, and the diagonal's
largest F.m + B.m, which sets the candidate bound.  The groups of a refresh diagonal advance in lock-step and the maximum
is one DPP reduction (wave_max_f32, checked on its own by tools/wave_max_check.hip).

Every case runs under the position-indexed rows and the rank-indexed ones (CPECAN_ABS default / 0), with gangs of eleven
and without (CPECAN_GANG 11 / 0): the result lists, and the debug buffers -- F + B of every emitted cell and the total used
on every emitted diagonal, i.e. the fold of the dot products -- must be the same bits in all four forms, and the lists
agree with the oracle.  The shapes: unanchored pairs, so the whole matrix is the band and a diagonal has up to
min(lX, lY) + 1 cells; lX - lY = 17, so 18 consecutive diagonals have exactly that width and, with a refresh point every
tenth emitted diagonal, at least one of them is a refresh point.  Widths 63, 64, 65 / 127, 128, 129 / 191, 192, 193 put the
refresh diagonals into one, two and three groups of 64 lanes with 63, 0 and 1 cells in the last; 193, 255 and 257 are wider
than the three prefetched groups.  A traceback every 42 diagonals, so every region has many segments; the last segment of
every region starts on a refresh point, and the 8-base region (33 diagonals) is nothing but that segment."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
from cpecan_amd import api
from parity import assert_pairs_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)
# every region in a wide class (no packed kernel), every class with its traceback in a launch of its own
BASE_ENV = {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1"}
FORMS = [(abs_, gang) for abs_ in (None, "0") for gang in ("0", "11")]  # (CPECAN_ABS, CPECAN_GANG); None: the default
WIDTHS = (9, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257)
DEBUG_WIDTHS = (9, 64, 129, 191, 257)
GAP = 17


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


@functools.lru_cache(maxsize=None)
def _pair(width):
    """A pair of related sequences of width - 1 + GAP and width - 1 bases: sY is sX without GAP bases, one at a time and
    evenly spread, and with every 11th base replaced."""
    m = width - 1
    sx = tc.seq(m + GAP, 7)
    drop = {(i + 1) * (m + GAP) // (GAP + 1) for i in range(GAP)}
    assert len(drop) == GAP
    sy = [c for i, c in enumerate(sx) if i not in drop]
    for i in range(5, len(sy), 11):
        sy[i] = "ACGT"[("ACGT".index(sy[i]) + 1) % 4]
    return sx, "".join(sy), ()


def _problems():
    return [_pair(w) for w in WIDTHS]


def _pkw(threshold):
    return dict(threshold=threshold, **SHORT)


@functools.lru_cache(maxsize=None)
def _oracle(mtype, threshold, width):
    sx, sy, a = _pair(width)
    return ob.aligned_pairs(ob.model(mtype), sx, sy, a, ob.params(**_pkw(threshold)))


@pytest.mark.parametrize("mtype", [0, 2])
@pytest.mark.parametrize("threshold", [0.01, 0.0])
def test_every_problem_emits_pairs(mtype, threshold):
    """The oracle alone, on the CPU: no case below can pass on empty lists."""
    for w in WIDTHS:
        sx, sy, _ = _pair(w)
        assert (len(sx), len(sy)) == (w - 1 + GAP, w - 1)
        n = len(_oracle(mtype, threshold, w))
        assert n >= 1 and (w < 60 or n >= (w - 1) // 2), (w, n)


def _set_form(monkeypatch, form):
    abs_, gang = form
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    if abs_ is None:
        monkeypatch.delenv("CPECAN_ABS", raising=False)
    else:
        monkeypatch.setenv("CPECAN_ABS", abs_)
    monkeypatch.setenv("CPECAN_GANG", gang)  # (the plan reads the environment at upload)


def _run(mtype, problems, pkw, debug_cells=None):
    with api.Batch(_sm(mtype), api.pairwiseAlignmentBandingParameters_construct(**pkw), debug=debug_cells is not None) as b:
        for p in problems:
            b.add(*p)
        b.upload()
        b.run()
        b.download()
        out = [b.result(i) for i in range(len(problems))]
        dbg = b.debug_fetch(0, *debug_cells) if debug_cells else None
    return out, dbg


@pytest.mark.gpu
def test_wave_max_program(tmp_path):
    """tools/wave_max_check.hip: the DPP maximum against a shuffle reduction, pattern by pattern (one wave)."""
    exe = str(tmp_path / "wave_max_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "cpecan_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "wave_max_check.hip")],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("wave_max_check: ok"), out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("mtype", [0, 2])
@pytest.mark.parametrize("threshold", [0.01, 0.0])
def test_lists_are_the_same_bits_in_every_form(mtype, threshold, monkeypatch):
    problems, pkw = _problems(), _pkw(threshold)
    want = None
    for form in FORMS:
        _set_form(monkeypatch, form)
        got, _ = _run(mtype, problems, pkw)
        assert all(len(g) for g in got), (form, [len(g) for g in got])
        if want is None:
            want = got
            continue
        for w, a, b in zip(WIDTHS, got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "width %d: %r differs from %r" % (w, form, FORMS[0])
    for w, g in zip(WIDTHS, want):  # one problem per shape -- every one of them -- against the oracle
        assert_pairs_match(g, _oracle(mtype, threshold, w), threshold=threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("mtype", [0, 2])
@pytest.mark.parametrize("width", DEBUG_WIDTHS)
def test_debug_buffers_are_the_same_bits_in_every_form(width, mtype, monkeypatch):
    from parity import LOG_TOL
    sx, sy, a = _pair(width)
    pkw = _pkw(0.01)
    _, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), False, False)
    cells = (tr["n_cells"], tr["n_diagonals"])
    first = None
    for form in FORMS:
        _set_form(monkeypatch, form)
        got, (fb, tot) = _run(mtype, [(sx, sy, a)], pkw, cells)
        if first is None:
            first = (got, fb, tot)
            continue
        assert np.array_equal(got[0], first[0][0]), "%r: the list differs from %r" % (form, FORMS[0])
        assert fb.tobytes() == first[1].tobytes(), "%r: F + B differs from %r" % (form, FORMS[0])
        assert tot.tobytes() == first[2].tobytes(), "%r: the totals differ from %r" % (form, FORMS[0])
    # ... and they are the oracle's totals: the fold of the refresh points' dot products, on every emitted diagonal
    _, _, tot = first
    otot = tr["total_used"]
    mt = ~np.isnan(otot)
    assert mt.any() and np.isfinite(tot[mt]).all()
    assert np.all(np.abs(tot[mt] - otot[mt]) <= LOG_TOL * np.maximum(1.0, np.abs(otot[mt]))), float(np.max(np.abs(tot[mt] - otot[mt])))
