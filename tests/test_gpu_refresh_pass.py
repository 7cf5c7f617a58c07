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
than the three prefetched groups.

Every case runs under two band expansions (EXPANSIONS).  A diagonal is a traceback point only if it has at most
2 * diagonalExpansion + 1 cells (pairwiseAligner.c:792-793), so under the default expansion of 20 no diagonal wider than 41
cells is one: every region from width 25 up has exactly two segments, one of which spans all its wide diagonals, and the
9-cell region has one.  Under an expansion of 130 every diagonal of every region is a permitted traceback point: a
traceback every 42 diagonals, so every region has many segments -- 4, 7, 10, 13 for widths 65, 129, 193, 257
(tests/test_match_cases_cpu.py asserts at least (lX + lY) / 50) --, a segment hands over to the next on diagonals of
63, 64, 65, ... cells, the last segment of every region starts on a refresh point, and the 8-base region (33 diagonals) is
nothing but that segment."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
from cpecan_amd import api
from match_cases import GAP, pair as _pair  # the pair family: shared with the match suite
from parity import assert_pairs_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)
# every region in a wide class (no packed kernel), every class with its traceback in a launch of its own
BASE_ENV = {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1"}
FORMS = [(abs_, gang) for abs_ in (None, "0") for gang in ("0", "11")]  # (CPECAN_ABS, CPECAN_GANG); None: the default
WIDTHS = (9, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257)
DEBUG_WIDTHS = (9, 64, 129, 191, 257)
EXPANSIONS = (20, 130)  # two segments per region (none ends on a diagonal wider than 41 cells) / a segment every 42 diagonals


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


def _problems():
    return [_pair(w) for w in WIDTHS]


def _pkw(threshold, expansion=EXPANSIONS[0]):
    return dict(threshold=threshold, diagonalExpansion=expansion, **SHORT)


@functools.lru_cache(maxsize=None)
def _oracle(mtype, threshold, width, expansion=EXPANSIONS[0]):
    sx, sy, a = _pair(width)
    return ob.aligned_pairs(ob.model(mtype), sx, sy, a, ob.params(**_pkw(threshold, expansion)))


@pytest.mark.parametrize("mtype", [0, 2])
@pytest.mark.parametrize("threshold", [0.01, 0.0])
def test_every_problem_emits_pairs(mtype, threshold):
    """The oracle alone, on the CPU: no case below can pass on empty lists."""
    for w in WIDTHS:
        sx, sy, _ = _pair(w)
        assert (len(sx), len(sy)) == (w - 1 + GAP, w - 1)
        for expansion in EXPANSIONS:
            n = len(_oracle(mtype, threshold, w, expansion))
            assert n >= 1 and (w < 60 or n >= (w - 1) // 2), (w, expansion, n)


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
    """Both expansions: two segments per region, and a segment every 42 diagonals (the module's docstring)."""
    for expansion in EXPANSIONS:
        problems, pkw = _problems(), _pkw(threshold, expansion)
        want = None
        for form in FORMS:
            _set_form(monkeypatch, form)
            got, _ = _run(mtype, problems, pkw)
            assert all(len(g) for g in got), (form, [len(g) for g in got])
            if want is None:
                want = got
                continue
            for w, a, b in zip(WIDTHS, got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), \
                    "width %d, expansion %d: %r differs from %r" % (w, expansion, form, FORMS[0])
        for w, g in zip(WIDTHS, want):  # one problem per shape -- every one of them -- against the oracle
            assert_pairs_match(g, _oracle(mtype, threshold, w, expansion), threshold=threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("mtype", [0, 2])
@pytest.mark.parametrize("width", DEBUG_WIDTHS)
def test_debug_buffers_are_the_same_bits_in_every_form(width, mtype, monkeypatch):
    """Both expansions, as above: with the wider one the segments of a region hand over on its widest diagonals."""
    for expansion in EXPANSIONS:
        _debug_buffers_in_every_form(width, mtype, expansion, monkeypatch)


def _debug_buffers_in_every_form(width, mtype, expansion, monkeypatch):
    from parity import LOG_TOL
    sx, sy, a = _pair(width)
    pkw = _pkw(0.01, expansion)
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
