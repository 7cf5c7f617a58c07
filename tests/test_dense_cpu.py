"""CPU tests of the dense-rows layer (include/cpecan_dense.h, cpecan_amd/dense.py): the header against the module and the two
libraries, the argument checks, the cap, and cpecan_dense_schedule -- pure host code -- held integer for integer against
tests/dense_model.py's restatement of the reference's loop (impl/pairwiseAligner.c:782-867), against the traceback segments of
tests/table_model.py and against the oracle's own count of tracebacks.  The values are the GPU's: tests/test_gpu_dense.py."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import dense_cases as dc
import dense_model as dm
import oracle_binding as ob
import table_model as tm
from cpecan_amd import api, dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(ROOT, "cpecan_amd", "libcpecan_hip_exact.so")


def _declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpecan_dense.h")).read(), flags=re.S)
    return set(re.findall(r"\b(cpecan_dense_[a-z_0-9]+)\s*\(", header))


def test_header_declares_what_the_module_exports():
    assert _declared() == set(dense.EXPORTS)
    assert not set(dense.EXPORTS) & set(api.EXPORTS)
    L = api.lib()
    for name in dense.EXPORTS:
        assert hasattr(L, name), name


def test_exact_library_exports_them_too():
    assert os.path.exists(EXACT), "%s is missing: __graft_entry__.build() makes it" % EXACT
    L = C.CDLL(EXACT)
    for name in dense.EXPORTS:
        assert hasattr(L, name), name


# ---- argument errors, before a device is looked for ----
def test_create_refuses_bad_arguments():
    L = dense._lib()
    h = C.c_void_p()
    sm = api.stateMachine5_construct()
    assert L.cpecan_dense_create(None, C.byref(sm), None, 0) == -1
    assert L.cpecan_dense_create(C.byref(h), None, None, 0) == -1
    assert L.cpecan_dense_create(C.byref(h), C.byref(sm), None, -1) == -1
    bad_type = api.stateMachine5_construct()
    bad_type.type = 7
    assert L.cpecan_dense_create(C.byref(h), C.byref(bad_type), None, 0) == -1
    for kw in (dict(traceBackDiagonals=0), dict(diagonalExpansion=3), dict(diagonalExpansion=-2), dict(minDiagsBetweenTraceBack=1),
               dict(traceBackDiagonals=9, minDiagsBetweenTraceBack=10)):  # pairwiseAligner.c:761-765
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            dense.Dense(sm, api.pairwiseAlignmentBandingParameters_construct(**kw), device=1000)


@pytest.mark.parametrize("device", (0, 1000))  # 1000: no such device anywhere, and still the answer is EINVAL
def test_add_refuses_bad_problems_before_it_looks_for_a_device(device):
    with dense.Dense(api.stateMachine5_construct(), device=device) as d:
        for sx, sy, anchors in (("ACGT", "ACGT", [(2, 2, 0), (1, 3, 0)]),  # x not increasing
                                ("ACGT", "ACGT", [(1, 2, 0), (2, 2, 0)]),  # y not increasing
                                ("ACGT", "ACGT", [(4, 1, 0)]),             # outside the matrix
                                ("ACGT", "ACGT", [(-1, 1, 0)]),
                                ("ACGT", "ACGT", [(1, 1, 2 ** 40)])):      # an expansion beyond 32 bits
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                d.add(sx, sy, anchors)
        assert d.n == 0
        L = dense._lib()
        assert L.cpecan_dense_add(d._h, None, 3, b"ACG", 3, None, 0, 0, 0) == -1
        assert L.cpecan_dense_add(d._h, b"ACG", -1, b"ACG", 3, None, 0, 0, 0) == -1
        assert L.cpecan_dense_add(d._h, b"ACG", 3, b"ACG", 3, None, 2, 0, 0) == -1
        assert L.cpecan_dense_add(None, b"ACG", 3, b"ACG", 3, None, 0, 0, 0) == -1
        info = dense.DenseInfo()
        assert L.cpecan_dense_info(d._h, 0, C.byref(info)) == -1  # no such problem
        assert d.add("ACG", "ACGT") == 0
        assert d.info(0) == dict(nDiagonals=8, nCells=20, nSegments=1, nStates=5)
        assert L.cpecan_dense_info(d._h, 1, C.byref(info)) == -1
        rows = dense.DenseRows()
        assert L.cpecan_dense_rows(d._h, 0, C.byref(rows)) == -5  # CPECAN_ESTATE: before a run
        assert L.cpecan_dense_rows(d._h, 3, C.byref(rows)) == -1


def test_dynamic_expansions_must_be_even():
    p = api.pairwiseAlignmentBandingParameters_construct(dynamicAnchorExpansion=1)
    with dense.Dense(api.stateMachine5_construct(), p, device=1000) as d:
        with pytest.raises(api.CpecanError, match=r"\(-1\).*valid band"):
            d.add("ACGTACGT", "ACGTACGT", [(2, 2, 3)])
        assert d.add("ACGTACGT", "ACGTACGT", [(2, 2, 4)]) == 0


def test_run_needs_a_device():
    with dense.Dense(api.stateMachine5_construct(), device=1000) as d:
        d.add("ACGT", "ACGT")
        with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
            d.run()
    if api.device_count() < 1:
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):
            dense.forward_backward(api.stateMachine5_construct(), "ACGT", "ACGT")


def test_the_cap_refuses_with_the_bytes_needed(monkeypatch):
    """A run whose device rows would exceed CPECAN_DENSE_MAX_BYTES is refused; the message names the bytes needed.  The refusal
    needs no device.  20 cells of five states: F and B alone are 1600 bytes."""
    monkeypatch.setenv("CPECAN_DENSE_MAX_BYTES", "1000")
    with dense.Dense(api.stateMachine5_construct(), device=1000) as d:
        d.add("ACG", "ACGT")
        with pytest.raises(api.CpecanError, match=r"\(-4\).*need (\d+) bytes.*allows 1000") as e:
            d.run()
        need = int(re.search(r"need (\d+) bytes", str(e.value)).group(1))
        assert 1600 < need < 4000
        monkeypatch.setenv("CPECAN_DENSE_MAX_BYTES", str(need - 1))
        with pytest.raises(api.CpecanError, match=r"\(-4\)"):
            d.run()
        monkeypatch.setenv("CPECAN_DENSE_MAX_BYTES", str(need))  # fits: now the missing device is what is wrong
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):
            d.run()
    # the default is 1 GiB: an unanchored 6000 x 6000 five-state pair (3.6e7 cells) is over it
    monkeypatch.delenv("CPECAN_DENSE_MAX_BYTES")
    assert dense.MAX_BYTES == 1 << 30
    with dense.Dense(api.stateMachine5_construct(), device=1000) as d:
        d.add("A" * 6000, "A" * 6000)
        with pytest.raises(api.CpecanError, match=r"\(-4\).*allows %d" % (1 << 30)):
            d.run()


def test_a_2kb_pair_needs_about_39_mb(monkeypatch):
    """The scale the header quotes: a 2 kb five-state pair at expansion 100."""
    from cpecan_amd.workload import make_pair
    sx, sy, a = make_pair(3, 0, 2000, 100)
    monkeypatch.setenv("CPECAN_DENSE_MAX_BYTES", "1")
    with dense.Dense(api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=100),
                     device=1000) as d:
        d.add(sx, sy, a)
        with pytest.raises(api.CpecanError) as e:
            d.run()
    need = int(re.search(r"need (\d+) bytes", str(e.value)).group(1))
    assert 35e6 < need < 45e6, need


def test_schedule_refuses_bad_arguments():
    L = dense._lib()
    n = C.c_int64()
    bad = api.pairwiseAlignmentBandingParameters_construct(traceBackDiagonals=0)
    assert L.cpecan_dense_schedule(4, 4, None, 0, C.byref(bad), None, 0, C.byref(n), None, 0, None) == -1
    assert L.cpecan_dense_schedule(-1, 4, None, 0, None, None, 0, C.byref(n), None, 0, None) == -1
    assert L.cpecan_dense_schedule(4, 4, None, 0, None, None, 2, C.byref(n), None, 0, None) == -1  # a capacity without an array
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        dense.schedule(4, 4, [(3, 1, 0), (2, 2, 0)])


# ---- the schedule against the restated loop ----
def _check_schedule(lX, lY, anchors, p, what):
    """p: oracle_binding.Params.  Returns the segments."""
    lp = api.pairwiseAlignmentBandingParameters_construct(
        minDiagsBetweenTraceBack=p.minDiagsBetweenTraceBack, traceBackDiagonals=p.traceBackDiagonals,
        diagonalExpansion=p.diagonalExpansion, dynamicAnchorExpansion=p.dynamicAnchorExpansion)
    got = dense.schedule(lX, lY, anchors, lp)
    N = lX + lY
    if N == 0:
        assert len(got.segs) == 0 and len(got.calls) == 0, what
        return []
    width = [(r - l) // 2 + 1 for _, l, r in ob.band(anchors, lX, lY, p.diagonalExpansion, bool(p.dynamicAnchorExpansion))]
    segs, calls = dm.reference_loop(width, p.minDiagsBetweenTraceBack, p.traceBackDiagonals, p.diagonalExpansion)
    assert [tuple(int(v) for v in s) for s in got.segs] == segs, what
    assert segs == [tuple(s) for s in tm.schedule(np.asarray(width), p.minDiagsBetweenTraceBack, p.traceBackDiagonals, p.diagonalExpansion)], what
    assert len(got.calls) == len(calls) == N, what
    for c, want in zip(got.calls, calls):
        assert (int(c[0]), int(c[1])) == (want.xay, want.seg), (what, want.xay)
        forward, backward = dm.rows_of_call(c)
        assert forward == want.forward, (what, want.xay, sorted(forward), sorted(want.forward))
        assert backward == dm.served_backward(want), (what, want.xay, sorted(backward), sorted(want.backward))
        tb_prev, d_top, tb_from = segs[want.seg]
        if want.xay == tb_prev + 1 and tb_prev >= 1:
            assert want.xay - 2 not in forward, (what, want.xay)  # the freed-F[d - 2] quirk, SURVEY 8a row a11
        assert want.xay == N or want.xay + 1 in backward, (what, want.xay)
    assert sorted(int(c[0]) for c in got.calls) == list(range(1, N + 1)), what  # every diagonal exactly once
    return segs


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_schedule_of_the_cases(name):
    c = dc.case(name)
    segs = _check_schedule(len(c.sx), len(c.sy), dc.anchors_of(c), dc.oracle_params(c), name)
    _, trace = dc.oracle_trace(c)
    assert trace.get("n_tracebacks", 0) == len(segs)
    with dense.Dense(dc.model_pair(c.model)[0], dc.lib_params(c), device=1000) as d:  # the object plans the same, without a device
        d.add(c.sx, c.sy, dc.anchors_of(c), c.ragged_left, c.ragged_right)
        info = d.info(0)
    assert info["nSegments"] == len(segs) and info["nStates"] == dc.states(c.model)
    assert info["nDiagonals"] == trace.get("n_diagonals", 0) and info["nCells"] == trace.get("n_cells", 0)


def test_schedule_of_random_small_parameter_sets():
    """200 parameter sets in the ranges of the reference's test_getAlignedPairsWithBanding (tests/pairwiseAlignerTest.c:403-438),
    anchors as its getRandomAnchorPairs draws them (:326-342)."""
    rng = random.Random(403)
    multi = 0
    for trial in range(200):
        lX = rng.randint(0, 100)
        lY = max(0, lX + rng.randint(-10, 10))
        tbd = rng.randint(1, 10)
        p = ob.params(traceBackDiagonals=tbd, minDiagsBetweenTraceBack=tbd + rng.randint(2, 10), diagonalExpansion=2 * rng.randint(0, 10),
                      dynamicAnchorExpansion=int(rng.random() > 0.5))
        anchors, x, y = [], -1, -1
        while True:
            x += rng.randint(1, 20)
            y += rng.randint(1, 20)
            e = 2 * rng.randint(0, 5)
            if x >= lX or y >= lY:
                break
            anchors.append((x, y, e))
        multi += len(_check_schedule(lX, lY, anchors, p, "trial %d" % trial)) > 2
    assert multi >= 100  # most of them trace back several times


# ---- the case module's preconditions ----
def test_the_cases_are_what_they_claim():
    w = {c.name: dc.widths(c) for c in dc.cases()}
    assert max(w["b_70x75"]) == 71 > 64  # more than one 64-lane group
    c = dc.case("c_segments")
    segs, calls = dm.reference_loop(w[c.name], 50, 7, 10)
    assert len(segs) >= 5
    for tb_prev, d_top, tb_from in segs[:-1]:
        assert tb_from - tb_prev > 10  # the refreshes restart inside every traceback: more than one per traceback
        assert d_top - tb_from == 8
    assert sum(1 for k in calls if k.xay == segs[k.seg][0] + 1 and segs[k.seg][0] >= 1) == len(segs) - 1  # the quirk, at every bottom
    d = dc.case("d_inf_ragged")
    assert (len(d.sx), d.ragged_left, d.ragged_right) == (150, True, True)
    assert b"NNN" in d.sx and b"NNN" in d.sy and d.sx != d.sx.upper() and d.sy != d.sy.upper()
    lib_m, orc_m = dc.model_pair(d.model)
    assert lib_m.type == api.threeStateAsymmetric and lib_m.gapShortSwitchToY == -np.inf and np.isfinite(lib_m.gapShortSwitchToX)
    assert sum(1 for i in range(orc_m.nTransitions) if orc_m.tr[i].tP == -np.inf) == 1
    assert max(w[d.name]) < 64 and len(dm.reference_loop(w[d.name], 60, 9, 12)[0]) >= 3
    e = dc.case("e_dynamic")
    assert e.pkw["dynamicAnchorExpansion"] == 1 and len({int(t[2]) for t in e.anchors}) >= 4
    assert len(dm.reference_loop(w[e.name], 100, 20, 20)[0]) >= 2
    assert [(len(dc.case(n).sx), len(dc.case(n).sy)) for n in ("f_x0", "f_y0", "f_both0")] == [(0, 5), (5, 0), (0, 0)]
    h = dc.split_case()
    rects = ob.split_points(dc.anchors_of(h), len(h.sx), len(h.sy), h.pkw["splitMatrixBiggerThanThis"], h.ragged_left, h.ragged_right)
    assert len(rects) >= 3


def test_no_oracle_pair_sits_at_the_threshold():
    """The foreign-emitter test excuses pairs within 1e-5 * threshold of the threshold; for these cases the oracle's lists have
    none that close (scores are floors of p * 1e7: one unit of slack for the floor)."""
    for c in dc.cases() + (dc.split_case(),):
        om, p = dc.model_pair(c.model)[1], dc.oracle_params(c)
        lists = ob.aligned_pairs_with_indels(om, c.sx, c.sy, dc.anchors_of(c), p, c.ragged_left, c.ragged_right)
        t = p.threshold * ob.PROB_1
        for l in lists:
            s = np.asarray(l, dtype=np.int64).reshape(-1, 3)[:, 0]
            assert not np.any(np.abs(s - t) <= 1e-5 * t + 1), c.name
