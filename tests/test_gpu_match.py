"""The match emitter (CPECAN_EMIT_MATCH, the headline path) on every sweep-kernel form against the CPU oracle.

tests/match_cases.py holds the form matrix -- rows of planning knobs and the kernels each must reach: one wave per region,
the two launches and the one launch of a split class with the rows indexed by rank and by absolute position, each in its
builds for two and for three waves per SIMD, gangs, and the same with the rolling rows in global memory -- and the
inputs; tests/test_match_cases_cpu.py asserts the preconditions without a device (every row plans its kernels, the rows
cover the kernel table, the oracle alone meets the caps).  Here every row

1. ran the kernels it names: the plan the uploaded batch really got (cpk_batch_launch_forms: the registers the loaded
   code object reports) is the row's, class by class, the CPECAN_TRACE_HOST line carries the matching words, and the
   plan is the same behind the download -- a one-launch class that was quietly re-run in two launches is not.  Where the
   device declines a build the plan without a device takes, the test fails and says which;
2. gives the oracle's lists, per problem: parity.assert_pairs_match (set, scores, order), the pairs on one side only
   capped by indel_cases.one_sided_allowed -- 0.5 % of the oracle's list, none at threshold 0;
3. gives, bit for bit, the lists of row W1 (GW1 for the global set): a build for three waves per SIMD is the same
   arithmetic in other registers;
4. where the row may run with debug buffers, gives F + B of every emitted cell and the totals used of the oracle's trace
   at parity.LOG_TOL.

The packed kernels, the teams and the gangs of more than two waves have suites of their own: test_gpu_parity.py,
test_gpu_indel.py / test_gpu_expect.py, test_gpu_gang.py."""
import hashlib
import re
import sys
import time

import numpy as np
import pytest

import indel_cases as ic
import match_cases as mc
import oracle_binding as ob
from cpecan_amd import api
from parity import LOG_TOL, assert_pairs_match
from test_gpu_forward import GLOBAL_MARK

pytestmark = pytest.mark.gpu

ONE_WAVE, TWO_LAUNCHES, ONE_LAUNCH = "one wave per region", "two launches", "one launch"
ABS_WORDS, DENSE_WORDS = "absolute positions", "three waves per SIMD"
LAUNCH_WORDS = {mc.MODE_WHOLE: ONE_WAVE, mc.MODE_FORWARD: TWO_LAUNCHES, mc.MODE_FUSED: ONE_LAUNCH}
NAMES = {mc.MODE_WHOLE: "whole", mc.MODE_FORWARD: "fwd", mc.MODE_TRACE: "trace", mc.MODE_FUSED: "fused"}


def _describe(kernels, global_rows=0):
    return " / ".join("%s wps%d%s%s" % (NAMES[k.mode], k.wps, " abs" if k.abs else "", " gang" if k.gang else "") for k in kernels if k) + \
        (" global" if global_rows else "")


def _class_lines(err):
    return re.findall(r"^cpecan class \d+:.*$", err, re.M)


def _run(case, capfd, debug_cells=None):
    """One batch under the environment as it stands: (lists, stats, the uploaded batch's plan, class lines, debug buffers)."""
    printed = capfd.readouterr().out  # (what the test has printed so far: put back below)
    with api.Batch(mc.sm(case.mtype), api.pairwiseAlignmentBandingParameters_construct(**case.pkw), debug=debug_cells is not None) as b:
        b.add_many(case.problems)
        b.upload()
        plan = mc.uploaded_plan(b)
        b.run()
        b.download()
        # A one-launch class whose item gave up waiting is re-run in two launches by the download, quietly, and has the
        # two-launch form from then on (cpk_device_download, unfuse): the plan as it stands behind the download is the one
        # whose kernels produced the lists
        after = mc.uploaded_plan(b)
        assert after == plan, "the plan changed between upload and download: %s, then %s" % (
            [_describe(mc.class_kernels(c), c["globalRows"]) for c in plan], [_describe(mc.class_kernels(c), c["globalRows"]) for c in after])
        lists = [b.result(i) for i in range(len(case.problems))]
        dbg = b.debug_fetch(0, *debug_cells) if debug_cells else None
        st = b.stats()
    err = capfd.readouterr().err
    sys.stdout.write(printed)
    return lists, st, plan, _class_lines(err), dbg


# ---- 1. the form ran ----
def _assert_form_ran(row, case, plan, lines, cap=0, global_rows=0):
    mtype = case.mtype
    assert plan and len(lines) == len(plan), (plan, lines)
    assert sum(c["regions"] for c in plan) == len(case.problems)
    for c, line in zip(plan, lines):
        want = mc.device_expectation(row, mtype, c, cap)
        got = mc.class_kernels(c)
        assert got == want and c["globalRows"] == global_rows, \
            "row %s, %d states, class of %d cells: the device planned %s where the plan without a device takes %s -- " \
            "that variant cannot be reached on this hardware with these knobs" % (
                row, mc.states(mtype), c["maxWidth"], _describe(got, c["globalRows"]), _describe(want, global_rows))
        assert (c["packed"], c["family"], c["threads"]) == (0, mc.FAMILY_SWEEP, 64), c
        assert (c["gangWaves"], c["gangWavesTrace"]) == ((2, 2) if row == "G" else (0, 0)), c
        # the class line: the launches, the rows' memory, the form of the sweeps, the plan's dense decision
        assert LAUNCH_WORDS[want[0].mode] in line, line
        assert (GLOBAL_MARK in line) == bool(global_rows), line
        assert (ABS_WORDS in line) == bool(want[0].abs), line
        dense = mc.states(mtype) == 3 and mc.ROWS[row].knobs.get("CPECAN_DENSE") == "1" and (want[1] or want[0]).wps == 3
        assert (DENSE_WORDS in line) == dense, line
        assert ("gang of 2" in line) == (row == "G"), line
    # the narrowest class has room for every build of the row (with one wave per CU nothing has): nothing demoted there
    if cap != 1:
        assert mc.class_kernels(plan[0]) == mc.device_expected(row, mtype, cap), (row, plan[0])
    print("match plan %s S%d %s: %s" % (row, mc.states(mtype), case.name,
                                        "; ".join("%d cells: %s" % (c["maxWidth"], _describe(mc.class_kernels(c), c["globalRows"])) for c in plan)))


# ---- 2. lists against the oracle, per problem ----
def _keys(t):
    return (t[:, 1].astype(np.int64) + 1) * (1 << 32) + t[:, 2].astype(np.int64) + 1


_compared = {}  # (case, problem, digest of the list) -> (largest score difference, one-sided pairs): the same bytes, the same verdict


def _compare(row, case, got):
    """Every problem against the oracle; prints and returns (largest score difference, pairs on one side only)."""
    threshold = case.pkw["threshold"]
    want = mc.oracle_lists(case)
    assert len(got) == len(want)
    worst = one_sided = entries = 0
    for i, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g).reshape(-1, 3)
        entries += len(w)
        key = (case.name, i, hashlib.sha1(g.tobytes()).hexdigest())
        if key not in _compared:
            what = "row %s, %s, problem %d" % (row, case.name, i)
            if threshold == 0:
                assert len(g) == len(w), what
            _, gi, wi = np.intersect1d(_keys(g), _keys(w), return_indices=True)
            only = len(g) + len(w) - 2 * len(gi)
            diff = int(np.abs(g[gi, 0].astype(np.int64) - w[wi, 0]).max()) if len(gi) else 0
            assert only <= ic.one_sided_allowed(threshold, len(w)), "%s: %d pairs on one side only, oracle has %d" % (what, only, len(w))
            try:
                assert_pairs_match(g, w, threshold=threshold)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (what, e)) from None
            _compared[key] = (diff, only)
        diff, only = _compared[key]
        worst, one_sided = max(worst, diff), one_sided + only
    print("match lists %s S%d %s: %d oracle entries, largest score difference %d (of 1e7), %d pairs on one side only" % (
        row, mc.states(case.mtype), case.name, entries, worst, one_sided))
    return worst, one_sided


# ---- 3. form against form, bit for bit ----
_baseline = {}


def _first_row(case, env, capfd, monkeypatch, row):
    """The lists of row W1 / GW1 for the case, run once per process and never modified."""
    if case.name not in _baseline:
        mc.set_row(monkeypatch, row, **env)
        lists, _, _, _, _ = _run(case, capfd)
        for a in lists:
            a.setflags(write=False)
        _baseline[case.name] = lists
    return _baseline[case.name]


def _assert_bit_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "%s: problem %d differs" % (what, i)


def _check_row(row, case, capfd, monkeypatch, first="W1", env=None, global_rows=0):
    env = env or {}
    t0 = time.time()
    want = _first_row(case, env, capfd, monkeypatch, first)
    mc.set_row(monkeypatch, row, **env)
    got, st, plan, lines, _ = _run(case, capfd)
    for line in lines:
        print(line)
    _assert_form_ran(row, case, plan, lines, int(env.get("CPECAN_MAX_WAVES_PER_CU", 0)), global_rows)
    assert st.problems == len(case.problems)
    _compare(row, case, got)
    _assert_bit_equal(got, want, "row %s against row %s, %s" % (row, first, case.name))
    print("match time %s S%d %s: %.2f s, %d launches" % (row, mc.states(case.mtype), case.name, time.time() - t0, st.launches))
    return st, plan, lines


@pytest.mark.parametrize("threshold", mc.THRESHOLDS)
@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("row", [r.name for r in mc.LDS_ROWS])
def test_lds_rows(row, mtype, threshold, monkeypatch, capfd):
    """Widths 9, 64, 65, 129, 193, 257 with every diagonal a permitted traceback point -- a segment every 42 diagonals, so the
    hand-off between segments lies on diagonals whose last 64-lane group has 9, 0 and 1 cells --, an empty problem, a
    one-sided one and a pair with ragged ends, in four size classes.  At threshold 0 every cell of every band is emitted
    (the candidates bypass the stage), nothing is near the threshold and no pair may stand on one side only."""
    case = mc.lds_case(mtype, threshold)
    _, plan, _ = _check_row(row, case, capfd, monkeypatch)
    assert len(plan) == 4


def _global_width(mtype, monkeypatch):
    mc.set_row(monkeypatch, "GW1")
    return mc.first_global_width(mtype, mc.cpu_plan)


@pytest.mark.parametrize("threshold", mc.THRESHOLDS)
@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("row", [r.name for r in mc.GLOBAL_ROWS])
def test_global_rows(row, mtype, threshold, monkeypatch, capfd):
    """Two unanchored pairs at the first width whose rows roll in global memory and 65 cells past it: every wave of the
    split launches has a slice of the global rows of its own (LaunchClass::subSlots).  At threshold 0 -- every cell of the
    band emitted, no pair on one side only -- the pair at the edge alone: 0.5 million triples of five states, 1.2 of three."""
    case = mc.global_case_at(mtype, _global_width(mtype, monkeypatch), threshold, second=threshold != 0)
    _, plan, _ = _check_row(row, case, capfd, monkeypatch, first="GW1", global_rows=1)
    assert len(plan) == 1


def _assert_waves_queue(case, plan, lines):
    """From the class line's `waves a / b`: fewer waves than regions and, in the traceback launch, than items."""
    (c,), (line,) = plan, lines
    a, b = map(int, re.search(r"waves (\d+) / (\d+)", line).groups())
    assert (a, b) == (c["waves"], c["wavesTrace"]), (line, c)
    assert a < c["regions"] == len(case.problems), line
    if c["mode"] == mc.MODE_FORWARD:
        assert b < c["items"], (line, c["items"])


@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("row", mc.QUEUE_ROWS)
def test_queue_rows(row, mtype, monkeypatch, capfd):
    """320 short regions under CPECAN_MAX_WAVES_PER_CU=1: every wave takes a second region, or item, with the state of the
    first still in its registers and LDS.  (One wave per CU: the builds for two waves per SIMD in every row.)"""
    case = mc.queue_case(mtype)
    _, plan, lines = _check_row(row, case, capfd, monkeypatch, env=mc.QUEUE_ENV)
    _assert_waves_queue(case, plan, lines)


@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("row", mc.DENSE_QUEUE_ROWS)
def test_dense_queue_rows(row, mtype, monkeypatch, capfd):
    """2400 short regions under CPECAN_MAX_WAVES_PER_CU=9: the builds for three waves per SIMD -- 168 registers and a
    handful of spills -- with a second region or item per wave; a spill slot that survived from the first would show."""
    case = mc.dense_queue_case(mtype)
    _, plan, lines = _check_row(row, case, capfd, monkeypatch, env=mc.DENSE_QUEUE_ENV)
    _assert_waves_queue(case, plan, lines)


# ---- 4. cell values ----
DEBUG_LDS = [r.name for r in mc.LDS_ROWS if r.debug]
DEBUG_GLOBAL = [r.name for r in mc.GLOBAL_ROWS if r.debug]


@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("row", DEBUG_LDS + DEBUG_GLOBAL)
def test_cell_values_and_totals_match_oracle(row, mtype, monkeypatch, capfd):
    """F.match + B.match of every emitted cell and the total used on every emitted diagonal (the sweeps' debug buffers) against
    the oracle's trace, at LOG_TOL: the pair of 129 cells for the LDS rows, of the first global width for the global ones."""
    global_rows = 1 if row in DEBUG_GLOBAL else 0
    width = _global_width(mtype, monkeypatch) if global_rows else mc.DEBUG_WIDTH
    case = mc.debug_case(mtype, width)
    (sx, sy, a, rl, rr), = case.problems
    want, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**case.pkw), rl, rr)
    mc.set_row(monkeypatch, row)
    got, _, plan, lines, (fb, tot) = _run(case, capfd, (tr["n_cells"], tr["n_diagonals"]))
    _assert_form_ran(row, case, plan, lines, 0, global_rows)
    assert_pairs_match(got[0], want, threshold=case.pkw["threshold"])
    ofb, otot = tr["fb_match"], tr["total_used"]
    m = ~np.isnan(ofb)
    inf = np.isinf(ofb[m])
    assert m.sum() >= len(want) > 0
    assert np.array_equal(np.isinf(fb[m]), inf) and np.array_equal(fb[m][inf], ofb[m][inf])
    scale = np.maximum(1.0, np.abs(ofb[m][~inf]))
    worst_fb = float(np.max(np.abs(fb[m][~inf] - ofb[m][~inf])))
    mt = ~np.isnan(otot)
    assert mt.any()
    worst_tot = float(np.max(np.abs(tot[mt] - otot[mt])))
    print("match cells %s S%d width %d: %d cells, largest |F+B difference| %.3g, largest |total difference| %.3g" % (
        row, mc.states(mtype), width, int(m.sum()), worst_fb, worst_tot))
    assert np.all(np.abs(fb[m][~inf] - ofb[m][~inf]) <= LOG_TOL * scale), worst_fb
    assert np.all(np.abs(tot[mt] - otot[mt]) <= LOG_TOL * np.maximum(1.0, np.abs(otot[mt]))), worst_tot
