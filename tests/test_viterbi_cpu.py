"""Viterbi decoding without a GPU: the numpy model (tests/viterbi_model.py) against exhaustive enumeration; the host functions
of include/cpecan_viterbi.h -- replay, info, the argument checks, pairs -- against the model on every case of
tests/viterbi_cases.py; the header against the module."""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest

import oracle_binding as ob
import viterbi_cases as vc
import viterbi_model as vm
from cpecan_amd import api, viterbi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(ROOT, "cpecan_amd", "libcpecan_hip_exact.so")
NO_DEVICE = 1000


def _bits(v):
    return np.float64(v).tobytes()


def test_header_declares_what_the_module_exports():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpecan_viterbi.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(cpecan_viterbi_[a-z_0-9]+)\s*\(", header)) == set(viterbi.EXPORTS)
    assert not set(viterbi.EXPORTS) & set(api.EXPORTS)
    for L in (api.lib(), C.CDLL(EXACT)):
        for name in viterbi.EXPORTS:
            assert hasattr(L, name), name
    assert "cpecan_viterbi" not in open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    internal = open(os.path.join(ROOT, "cpecan_amd", "csrc", "cpecan_internal.h")).read()
    assert int(re.search(r"#define CPK_VIT_BLOCK_DIAGS (\d+)", internal).group(1)) == viterbi.TRACEBACK_BLOCK_DIAGONALS
    assert int(re.search(r"#define CPK_VIT_LDS_MAX_WIDTH (\d+)", internal).group(1)) == viterbi.LDS_MAX_WIDTH


def test_the_cases_are_the_edges_they_claim():
    vc.check_preconditions()


# ---- the model against exhaustive enumeration ----
@pytest.mark.parametrize("model", vc.MODEL_TYPES)
def test_model_equals_exhaustive_enumeration(model):
    """Every state path of pairs of every length 0 .. 3 x 0 .. 3, all four ragged combinations, the band the whole matrix: the
    model's logP is the maximum to the bit, its path replays to it, and is the enumerated one wherever the maximum is unique."""
    om = vc.model_pair(model)[1]
    p = ob.params(diagonalExpansion=20)
    rng = random.Random(31)
    unique = 0
    for lx, ly in itertools.product(range(4), range(4)):
        for sx, sy in ((b"A" * lx, b"A" * ly), (vc._rand_seq(rng, lx), vc._rand_seq(rng, ly))):
            for rl, rr in itertools.product((False, True), (False, True)):
                paths = vm.enumerate_paths(om, sx, sy, rl, rr)
                best = max(v for v, _, _ in paths)
                logP, s0, s1, ops, n_cells, _ = vm.region(om, sx, sy, (), p, rl, rr)
                assert n_cells == (lx + 1) * (ly + 1)
                assert _bits(logP) == _bits(best), (model, sx, sy, rl, rr, logP, best)
                assert np.isfinite(best)
                assert _bits(vm.replay(om, sx, sy, rl, rr, s0, s1, ops)) == _bits(logP)
                winners = [(a, st) for v, a, st in paths if v == best]
                if len(winners) == 1:
                    unique += 1
                    steps = tuple(s for s, n in ops for _ in range(n))
                    assert winners[0] == (s0, steps), (model, sx, sy, rl, rr)
                    assert (steps[-1] if steps else s0) == s1
    assert unique >= 16


# ---- the host functions against the model ----
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_host_replay_of_the_models_paths_gives_its_logp_to_the_bit(name):
    c = vc.case(name)
    sm, om = vc.model_pair(c.model)
    m = vc.model_of(c)
    total = None
    for r, (sx, sy, rl, rr) in zip(m.regions, vc.region_inputs(c)):
        if r.nOps == 0 and r.startState < 0:
            assert r.logP == float("-inf")
        else:
            ops = m.ops[r.opOff:r.opOff + r.nOps]
            assert _bits(viterbi.replay(sm, sx, sy, rl, rr, r.startState, r.endState, ops)) == _bits(r.logP), (name, r)
            assert _bits(vm.replay(om, sx, sy, rl, rr, r.startState, r.endState, ops)) == _bits(r.logP), (name, r)
            assert all(a[0] != b[0] for a, b in zip(ops[:-1], ops[1:])) and (ops[:, 1] >= 1).all(), "maximal runs"
        total = r.logP if total is None else total + r.logP
    assert _bits(total) == _bits(m.logP)


def test_replay_refuses_malformed_ops():
    sm = api.stateMachine5_construct()
    c = vc.case("a_tiny5")
    r = vc.model_of(c).regions[0]
    ops = vc.model_of(c).ops
    good = lambda o, s0=r.startState, s1=r.endState: viterbi.replay(sm, c.sx, c.sy, False, False, s0, s1, o)  # noqa: E731
    assert _bits(good(ops)) == _bits(r.logP)
    for bad in (ops[:-1],                                       # ends short of (lX, lY)
                np.concatenate([ops, [[0, 1]]]),                # leaves the matrix
                [[1, 4], [2, 6]],                               # shortX -> shortY: the five-state model has no switch
                [[3, 4], [1, 0], [2, 6]], [[5, 4], [2, 6]], [[0, -1]]):
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            good(np.array(bad, dtype=np.int32))
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        good(ops, s1=(r.endState + 1) % 5)                      # the path ends in another state
    with pytest.raises(api.CpecanError, match=r"\(-1\)"):
        good(ops, s0=5)
    # the three-state model has the switch
    sm3 = api.stateMachine3_construct()
    assert np.isfinite(viterbi.replay(sm3, c.sx, c.sy, False, False, 0, 2, np.array([[1, 4], [2, 6]], dtype=np.int32)))


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_info_equals_the_models_regions_and_cells(name):
    c = vc.case(name)
    m = vc.model_of(c)
    with viterbi.Viterbi(vc.model_pair(c.model)[0], vc.lib_params(c), device=NO_DEVICE) as v:
        assert v.add(c.sx, c.sy, vc.anchors_of(c), c.ragged_left, c.ragged_right) == 0
        i = v.info(0)
        assert (i["nRegions"], i["nCells"], i["nStates"]) == (len(m.regions), m.n_cells, dc_states(c)), (name, i)
        assert i["deviceBytes"] > m.n_cells
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            v.result(0)
        with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
            v.run()
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            v.info(1)


def dc_states(c):
    return vc.model_pair(c.model)[1].S


def test_bad_arguments_are_refused_before_any_device():
    sm = api.stateMachine5_construct()
    L, h = viterbi._lib(), C.c_void_p()
    assert L.cpecan_viterbi_create(C.byref(h), None, None, 0) == -1
    assert L.cpecan_viterbi_create(C.byref(h), C.byref(sm), None, -1) == -1
    bad = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=3)
    assert L.cpecan_viterbi_create(C.byref(h), C.byref(sm), C.byref(bad), 0) == -1
    with viterbi.Viterbi(sm, device=NO_DEVICE) as v:
        for sx, sy, anchors in (("ACGT", "ACGT", [(2, 2, 0), (1, 3, 0)]),  # x not increasing
                                ("ACGT", "ACGT", [(1, 2, 0), (2, 2, 0)]),  # y not increasing
                                ("ACGT", "ACGT", [(4, 1, 0)]),             # outside the matrix
                                ("ACGT", "ACGT", [(1, 4, 0)]),
                                ("ACGT", "ACGT", [(-1, 1, 0)])):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                v.add(sx, sy, anchors)
        assert v.n == 0 and L.cpecan_viterbi_info(v._h, 0, C.byref(viterbi.ViterbiInfo())) == -1  # nothing was added
        for b in (0, -1):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                v.set_budget(b)
        for f in (-1, 3):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                v.set_form(f)
        for f in (viterbi.FORM_AUTO,) + viterbi.FORMS:
            v.set_form(f)
        v.set_budget(1)
        assert v.launch_forms() == (0, 0, 0) and v.kernel_ms() == (0.0, 0.0)
    p = api.pairwiseAlignmentBandingParameters_construct(dynamicAnchorExpansion=1)
    with viterbi.Viterbi(sm, p, device=NO_DEVICE) as v:
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            v.add("ACGTACGT", "ACGTACGT", [(3, 3, 5)])  # an odd expansion


def test_a_region_above_the_budget_and_a_forced_form_that_cannot_hold_it_are_refused_without_a_device():
    c = vc.case("u_300x300")
    with viterbi.Viterbi(vc.model_pair(c.model)[0], vc.lib_params(c), device=NO_DEVICE) as v:
        v.add(c.sx, c.sy)
        need = v.info(0)["deviceBytes"]
        v.set_budget(need - 1)
        with pytest.raises(api.CpecanError, match=r"\(-4\).*needs %d bytes" % need):
            v.run()
        v.set_budget(need)
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):
            v.run()
        v.set_form(viterbi.FORM_LDS)
        with pytest.raises(api.CpecanError, match=r"\(-1\).*LDS form"):
            v.run()


def test_config_b_needs_about_600_kb_a_pair_on_the_device():
    """The scale DESIGN.md section 12 quotes: a 2 kb pair at band 100."""
    from cpecan_amd.workload import make_pair
    sx, sy, a = make_pair(3, 0, 2000, 100)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=100)
    with viterbi.Viterbi(api.stateMachine5_construct(), p, device=NO_DEVICE) as v:
        v.add(sx, sy, a)
        i = v.info(0)
    assert 0.4e6 < i["nCells"] < 0.6e6 and 0.5e6 < i["deviceBytes"] < 0.7e6 and i["deviceBytes"] < 1.3 * i["nCells"], i


@pytest.mark.parametrize("name", ("a_tiny5", "r_three", "r_three_ragged_left", "p_no_path", "f_both0", "n_3B"))
def test_pairs_are_the_match_steps_in_problem_coordinates(name):
    c = vc.case(name)
    m = vc.model_of(c)
    want = []
    for r in m.regions:
        x, y = r.x1, r.y1
        for s, n in m.ops[r.opOff:r.opOff + r.nOps]:
            for _ in range(n):
                if s == 0:
                    want.append((x, y))
                x, y = x + (s in (0, 1, 3)), y + (s in (0, 2, 4))
        assert r.nOps == 0 or (x, y) == (r.x2, r.y2)
    got = viterbi.pairs_of(viterbi.Result(m.logP, m.regions, m.ops))
    assert got.dtype == np.int64 and got.tolist() == [list(t) for t in want]
    assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(want[:-1], want[1:]))
