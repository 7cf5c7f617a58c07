"""Gapped extension of the chained HSPs (cpecan_anchor_options.gappedExtension, yDrop, gappedMaxDiagonals; DESIGN.md section
7, step 5b) without a GPU: the ABI, what is refused before a device is looked for, the model (tests/anchor_model_gapped.py)
on the constructed cases and its properties on random, masked and ENCODE pairs, the device-free sizing of the pass, and the
option on the command line."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_gapped_cases as gc
import anchor_model as am
import anchor_model_gapped as ag
import anchor_model_threshold as ath
import anchor_stages as st
import reference_cases as rc
from cpecan_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = am.default_params()
SCORE = np.array(P["scores"], dtype=np.int64).reshape(5, 5)


def _calls(sx, sy, params, options):
    return (lambda: api.find_anchor_runs(sx, sy, params=params, options=options),
            lambda: api.find_anchor_runs_many([(sx, sy)], params=params, options=options),
            lambda: api.find_anchor_runs_once(sx, sy, params=params, options=options),
            lambda: api.find_anchor_runs_many_stranded([(sx, sy)], params=params, strand="both", options=options))


def _once(case, **kw):
    sx, sy, options = gc.CASES[case] if case in gc.CASES else case
    return ag.anchors_once(sx, sy, 14, True, P, **dict(options, **kw))


def _columns(runs):
    return {(x + k, y + k) for x, y, n in runs for k in range(n)}


# ---- the ABI ----
def test_the_options_through_the_abi():
    assert C.sizeof(api.AnchorOptions) == 32
    o = api.AnchorOptions(transitionHspThreshold=5)
    o.gappedExtension, o.yDrop, o.gappedMaxDiagonals = 1, 77, 64
    assert list(o.reserved) == [1, 77, 64, 0, 0, 0, 0]                  # the properties lie over words 0 to 2
    assert api.lib().cpecan_anchor_options_default(C.byref(o)) == 0
    assert bytes(o) == bytes(32)
    d = api.anchor_options()
    assert (d.transitionHspThreshold, d.gappedExtension, d.yDrop, d.gappedMaxDiagonals) == (0, 0, 0, 0) and bytes(d) == bytes(32)
    o = api.anchor_options(1200, gappedExtension=1, yDrop=500, gappedMaxDiagonals=128)
    assert np.frombuffer(bytes(o), dtype=np.int32).tolist() == [1200, 1, 500, 128, 0, 0, 0, 0]


def _bad_options():
    out = [api.anchor_options(gappedExtension=2), api.anchor_options(gappedExtension=-1),
           api.anchor_options(gappedExtension=1, yDrop=-1), api.anchor_options(gappedExtension=1, yDrop=-2 ** 31),
           api.anchor_options(gappedExtension=1, gappedMaxDiagonals=63), api.anchor_options(gappedExtension=1, gappedMaxDiagonals=4097),
           api.anchor_options(gappedExtension=1, gappedMaxDiagonals=-64),
           api.anchor_options(yDrop=9400), api.anchor_options(gappedMaxDiagonals=4096)]          # without gappedExtension
    for word in (3, 4, 5, 6):                                            # the four that stay reserved
        o = api.anchor_options(gappedExtension=1)
        o.reserved[word] = 1
        out.append(o)
    return out


def test_bad_options_are_refused_before_a_device_is_looked_for():
    sx, sy, _ = gc.CASES["deletion of 3"]
    for transitions in (0, 1):
        p = api.anchor_params_default(seedTransitions=transitions)
        for bad in _bad_options():
            for call in _calls(sx, sy, p, bad):
                with pytest.raises(api.CpecanError) as e:
                    call()
                assert "(-1)" in str(e.value), bytes(bad).hex()          # CPECAN_EINVAL: the same with and without a device


def test_without_a_device_valid_options_answer_no_device():
    if api.device_count() > 0:
        return  # with a GPU the calls succeed: tests/test_gpu_anchor_gapped.py
    sx, sy, _ = gc.CASES["deletion of 3"]
    good = (api.anchor_options(gappedExtension=1), api.anchor_options(gappedExtension=1, yDrop=1),
            api.anchor_options(gappedExtension=1, yDrop=2 ** 31 - 1, gappedMaxDiagonals=64),
            api.anchor_options(1200, gappedExtension=1, gappedMaxDiagonals=4096))
    for transitions in (0, 1):
        p = api.anchor_params_default(seedTransitions=transitions)
        for o in good:
            for call in _calls(sx, sy, p, o):
                with pytest.raises(api.CpecanError) as e:
                    call()
                assert "(-2)" in str(e.value)
    smachine = api.stateMachine5_construct(api.fiveState)
    bp = api.pairwiseAlignmentBandingParameters_construct()
    with pytest.raises(api.CpecanError) as e:
        api.getAlignedPairs(smachine, sx * 2, sy * 2, bp, anchorOptions=good[0])
    assert "(-2)" in str(e.value)


# ---- the model on the constructed cases (tests/anchor_gapped_cases.py) ----
def test_a_deletion_of_3_is_crossed_only_with_the_option():
    off, counts_off = _once("deletion of 3", gapped=0)
    on, counts_on = _once("deletion of 3")
    assert len(off) == 1 and counts_off == counts_on
    assert len(on) == 2 and on[0] == off[0] and on[1][0] - on[1][1] == 3
    # the walk goes to the end of the sequences; its best cell lies two columns before, the last but one being a transversion
    assert on[1][0] + on[1][2] == 500 - 2 - 14


def test_the_band_ends_at_31():
    on, _ = _once("deletion of 31")
    assert len(on) == 2 and on[1][0] - on[1][1] == 31
    on, _ = _once("deletion of 32")
    off, _ = _once("deletion of 32", gapped=0)
    assert on == off and len(on) == 1


def test_an_insertion_before_the_exact_part_is_gained_by_a_left_extension():
    off, _ = _once("insertion before", gapped=0)
    on, _ = _once("insertion before")
    assert len(off) == 1 and len(on) == 2 and on[1] == off[0]
    assert on[0][0] - on[0][1] == 0 and off[0][0] - off[0][1] == -7


def test_the_diagonal_limit_cuts_the_second_run_short():
    whole, _ = _once("deletion of 3")
    cut, _ = _once("128 diagonals")
    assert len(cut) == 2 and cut[0] == whole[0] and cut[1][:2] == whole[1][:2] and 0 < cut[1][2] < whole[1][2]
    # 128 anti-diagonals hold at most 64 aligned columns, of which the deletion's three diagonals take none
    assert cut[1][2] <= 64 - 2 * 14


def test_a_small_y_drop_removes_the_second_run():
    on, _ = _once("yDrop 100")
    off, _ = _once("yDrop 100", gapped=0, yDrop=0)
    assert on == off and len(on) == 1


def test_two_extensions_into_one_short_gap_and_the_overlap_rule():
    sx, sy, _ = gc.CASES["both sides"]
    hsps, _, _ = ath._hsps(sx, sy, True, P, 0, 0)
    chain = [hsps[i][:3] for i in am.chain(hsps)]
    assert len(chain) == 2
    cx, cy = am._CODE[am._bytes(sx)], am._CODE[am._bytes(sy)]
    lower, upper = (chain[0][0] + chain[0][2], chain[0][1] + chain[0][2]), chain[1][:2]
    gx, gy = cx[lower[0]:upper[0]], cy[lower[1]:upper[1]]
    bestR, (iR, jR), blocksR = ag.right_extension(gx, gy, SCORE)
    bestL, (iL, jL), blocksL = ag.right_extension(gx[::-1], gy[::-1], SCORE)
    assert blocksR and blocksL and iR + iL > len(gx) and bestR != bestL   # both reach the middle: they overlap
    keptR, keptL = ag.gap_extensions(cx, cy, lower, upper, True, True, SCORE, ag.Y_DROP, ag.MAX_DIAGONALS)
    assert (keptR == [], keptL != []) if bestR < bestL else (keptR != [], keptL == [])
    on, _ = _once("both sides")
    off, _ = _once("both sides", gapped=0)
    assert len(off) == 2 and len(on) == 3 and (on[0], on[2]) == (off[0], off[1])
    assert all(a[0] + a[2] <= b[0] and a[1] + a[2] <= b[1] for a, b in zip(on, on[1:]))


def test_a_tie_in_the_overlap_rule_drops_the_left_extension():
    """A palindromic gap: X and Y of the gap are one string s with s == s reversed, so both extensions have the same best
    and the same reach."""
    half = gc.random_bases(5, 30)
    s = am._CODE[am._bytes(half + half[::-1])]
    bestR, reachR, blocksR = ag.right_extension(s, s, SCORE)
    bestL, reachL, blocksL = ag.right_extension(s[::-1], s[::-1], SCORE)
    assert (bestR, reachR) == (bestL, reachL) and reachR == (60, 60)
    keptR, keptL = ag.gap_extensions(s, s, (0, 0), (60, 60), True, True, SCORE, ag.Y_DROP, ag.MAX_DIAGONALS)
    assert keptR == [(0, 0, 60)] and keptL == []


@pytest.mark.parametrize("case", ["touching, n = 0", "touching, m = 0"])
def test_a_gap_with_an_empty_side_has_no_extension(case):
    on, counts = _once(case)
    off, _ = _once(case, gapped=0)
    assert counts["chained"] == 2 and on == off
    empty = np.zeros(0, dtype=np.int64)
    assert ag.right_extension(empty, am._CODE[am._bytes("ACG")], SCORE) == (0, (0, 0), [])
    assert ag.right_extension(am._CODE[am._bytes("ACG")], empty, SCORE) == (0, (0, 0), [])
    assert ag.right_extension(empty, empty, SCORE) == (0, (0, 0), [])


def test_bad_options_are_refused_by_the_model_too():
    sx, sy, _ = gc.CASES["deletion of 3"]
    for bad in (dict(gapped=2), dict(gapped=1, yDrop=-1), dict(gapped=1, gappedMaxDiagonals=63), dict(gapped=1, gappedMaxDiagonals=4097),
                dict(yDrop=5), dict(gappedMaxDiagonals=64)):
        with pytest.raises(ValueError):
            ag.find_anchor_runs(sx, sy, **bad)


# ---- the model's properties ----
def _properties(sx, sy, **kw):
    """Option off is the model below; the runs increase strictly inside the sequences; steps 1-4 do not see the option; for
    steps 1-5 alone the anchor columns with the option are a superset."""
    off, st_off = ag.find_anchor_runs(sx, sy, **kw)
    want, st_want = ath.find_anchor_runs(sx, sy, **kw)
    assert np.array_equal(off, want) and st_off == st_want
    on, st_on = ag.find_anchor_runs(sx, sy, gapped=1, **kw)
    r = on.tolist()
    assert all(x >= 0 and y >= 0 and n > 0 and x + n <= len(sx) and y + n <= len(sy) for x, y, n, _ in r)
    assert all(a[0] + a[2] <= b[0] and a[1] + a[2] <= b[1] for a, b in zip(r, r[1:]))
    assert st_on["runs"] == len(r) and st_on["anchorColumns"] == sum(q[2] for q in r)
    once_kw = dict(seedTransitions=kw.get("seedTransitions", 0), threshold=kw.get("threshold", 0))
    for softMask in (True, False):
        a, ca = ag.anchors_once(sx, sy, 14, softMask, P, gapped=0, **once_kw)
        b, cb = ag.anchors_once(sx, sy, 14, softMask, P, gapped=1, **once_kw)
        assert ca == cb and _columns(a) <= _columns(b)
        assert (a, ca) == ath.anchors_once(sx, sy, 14, softMask, P, **once_kw)
    return st_off, st_on


@pytest.mark.parametrize("index", [1, 2, 3])
def test_the_properties_on_random_and_masked_pairs(index):
    more = 0
    for sx, sy in (ac.random_pair(index, 3000), ac.masked_pair(index, 3000)):
        st_off, st_on = _properties(sx, sy)
        more += st_on["anchorColumns"] > st_off["anchorColumns"]
        _properties(sx, sy, seedTransitions=1, threshold=1200)
    assert more >= 1


def test_the_strand_scores_do_not_see_the_option():
    import strand_model as sm
    sx, sy = ac.masked_pair(2, 3001)
    for strand in ("both", "minus"):
        _, _, off = ath.find_anchor_runs_stranded(sx, sm.rc(sy), strand)
        runs, stats, on = ag.find_anchor_runs_stranded(sx, sm.rc(sy), strand, gapped=1)
        assert on == off and on["strand"] == "minus"
        want, wst = ag.find_anchor_runs(sx, sy, gapped=1)
        assert np.array_equal(runs, want) and stats == wst


# name: (runs, anchor columns, columns off the embedded alignment, largest gap, cells of all gap rectangles), off and on
ENCODE = {"dog": ((162, 8389, 157, 5773131, 36.1e6), (406, 15107, 224, 4676660, 18.7e6)),
          "mouse": ((43, 1264, 8, 61984896, 106.9e6), (129, 3061, 70, 59128170, 90.5e6))}


@functools.lru_cache(maxsize=None)
def _encode(name, gapped):
    sx, sy, _, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
    return (sx, sy, true_pairs) + ag.find_anchor_runs(sx, sy, gapped=gapped)


@pytest.mark.parametrize("name", ["chimp", "dog", "mouse"])
def test_the_properties_on_the_encode_pairs(name):
    sx, sy, _, off, st_off = _encode(name, 0)
    want, st_want = am.find_anchor_runs(sx, sy)
    assert np.array_equal(off, want) and st_off == st_want
    _, _, _, on, st_on = _encode(name, 1)
    r = on.tolist()
    assert all(x >= 0 and y >= 0 and n > 0 and x + n <= len(sx) and y + n <= len(sy) for x, y, n, _ in r)
    assert all(a[0] + a[2] <= b[0] and a[1] + a[2] <= b[1] for a, b in zip(r, r[1:]))
    assert st_on["anchorColumns"] > st_off["anchorColumns"] and st_on["capped"] == 0
    top_off, c_off = ag.anchors_once(sx, sy, 14, True, P)
    top_on, c_on = ag.anchors_once(sx, sy, 14, True, P, gapped=1)
    assert c_off == c_on and _columns(top_off) <= _columns(top_on)


@pytest.mark.parametrize("name", ["dog", "mouse"])
@pytest.mark.parametrize("gapped", [0, 1])
def test_the_encode_pairs_give_the_recorded_integers(name, gapped):
    """profiles/anchor_quality_gapped.txt: the table the feature was proposed with."""
    sx, sy, true_pairs, runs, stats = _encode(name, gapped)
    anchors = am.runs_to_anchors(runs)
    off_alignment = sum((x, y) not in true_pairs for x, y, _ in anchors)
    cells = sum((x - pX) * (y - pY) for pX, pY, x, y in am._gaps([q[:3] for q in runs.tolist()], len(sx), len(sy)))
    want = ENCODE[name][gapped]
    print(name, gapped, stats, off_alignment, cells)
    assert (stats["runs"], stats["anchorColumns"], off_alignment, stats["largestGap"]) == want[:4]
    assert abs(cells - want[4]) <= 0.05e6                                # the table gives it to 0.1 M


# ---- the pass's device-free sizing (cpecan_internal.h) ----
class GappedPlan(C.Structure):
    _fields_ = [("nRows", C.c_int64), ("nRuns", C.c_int64), ("maxGaps", C.c_int32), ("pad", C.c_int32)]


GAPPED = 4


def _gapped_flags(diags=4096):
    return GAPPED | (diags << 8)


def test_the_sizing_of_a_gapped_pass():
    L = st.stages()
    L.cpk_anchor_gapped_size.restype = None
    L.cpk_anchor_gapped_size.argtypes = [C.POINTER(st.PassProblem), C.c_int64, st.i64p, st.i64p, C.POINTER(GappedPlan)]
    probs = (st.PassProblem * 4)()
    for i, (flags, rows, chained, nRuns) in enumerate([(_gapped_flags(), 1000, 3, 0), (0, 555, 7, 5), (_gapped_flags(64), 0, 0, 0),
                                                       (_gapped_flags(), 128, 40, 0)]):
        probs[i].flags, probs[i].columns, probs[i].chained, probs[i].nRuns = flags, rows, chained, nRuns
    rowBase, runBase, plan = (C.c_int64 * 5)(), (C.c_int64 * 5)(), GappedPlan()
    L.cpk_anchor_gapped_size(probs, 4, rowBase, runBase, C.byref(plan))
    assert list(rowBase) == [0, 1000, 1000, 1000, 1128] and list(runBase) == [0, 1003, 1008, 1008, 1176]
    assert (plan.nRows, plan.nRuns, plan.maxGaps) == (1128, 1176, 41)


def test_the_launches_of_a_pass_over_the_budget_end_at_gap_boundaries():
    L = st.stages()
    L.cpk_anchor_gapped_slice_end.restype = C.c_int64
    L.cpk_anchor_gapped_slice_end.argtypes = [st.i64p, C.c_int64, C.c_int64, C.c_int64]
    rows = [0, 8192, 100, 0, 0, 8000, 192, 8192, 1, 0]                   # rows per gap; some have none
    bounds = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    arr = (C.c_int64 * len(bounds))(*bounds.tolist())
    for budget in (8192, 8292, 10000, 16384, 10 ** 9):
        lo, cuts = 0, []
        while lo < bounds[-1]:
            hi = L.cpk_anchor_gapped_slice_end(arr, len(bounds), lo, budget)
            assert lo < hi <= lo + budget and hi in bounds               # it advances, fits and ends at a boundary
            assert hi == max(b for b in bounds if b <= lo + budget)      # and is the farthest such
            cuts.append(hi)
            lo = hi
        assert cuts[-1] == bounds[-1]
    assert L.cpk_anchor_gapped_slice_end(arr, len(bounds), 0, 8191) == 0   # a gap that does not fit: no progress, an error


def test_the_plan_checks_the_gapped_values_of_a_problem():
    def plan(**fields):
        p = st.PassProblem(xOff=0, yOff=300, lX=300, lY=200, softMask=1)
        for k, v in fields.items():
            setattr(p, k, v)
        arr = (st.PassProblem * 1)(p)
        rc_ = st.stages().cpk_anchor_pass_plan(C.byref(st.default_pass()), arr, 1, 1000, 1000, C.byref(st.Plan()))
        return rc_, api.lib().cpecan_last_error().decode(), arr[0]
    rc_, _, p = plan(flags=_gapped_flags(64), pad=9400)                  # `pad` is yDrop in the C struct
    assert rc_ == st.OK and (p.flags, p.pad) == (_gapped_flags(64), 9400)
    assert plan(flags=_gapped_flags(4096), pad=1)[0] == st.OK
    for bad in (dict(flags=_gapped_flags(64), pad=0), dict(flags=_gapped_flags(63), pad=5), dict(flags=_gapped_flags(4097), pad=5),
                dict(flags=GAPPED, pad=5), dict(flags=0, pad=5), dict(flags=64 << 8, pad=0)):
        rc_, text, _ = plan(**bad)
        assert rc_ == st.EINVAL and "gapped extension" in text, bad


# ---- the command line ----
def test_cpecan_align_wants_gapped_with_y_drop(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--gapped" in r.stderr and "--yDrop" in r.stderr
    (tmp_path / "empty.fa").write_text("")
    files = [str(tmp_path / "empty.fa"), str(tmp_path / "empty.fa")]
    for flags in (["--yDrop", "5000"], ["-Y", "5000"], ["--yDrop=5000", "--strand", "both"]):
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and "--yDrop" in r.stderr and "--gapped" in r.stderr
    for flags in (["--gapped"], ["--gapped", "--yDrop", "5000"], ["-G", "-Y", "5000", "-t", "-T", "1200"]):   # no pairs: no device
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stdout == ""
    for flags in (["-G", "-Y", "x"], ["-G", "-Y", "0"], ["-G", "-Y", "-3"], ["-G", "-Y"]):
        r = subprocess.run([exe] + flags + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0
