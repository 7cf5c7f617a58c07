"""The preconditions that make tests/test_gpu_table.py meaningful, asserted without a device: every case of
tests/table_cases.py really has the edge it was built for -- an anchor on a lane's first diagonal, a ring that wraps, a band
edge that turns back on a chunk's first and last diagonal -- as tests/table_model.py sees it; the model agrees with the
oracle's cell offsets and traceback counts and with what host planning counts; and the model's own checks see the faults
they are there for.  A case that silently stops exercising its edge fails here, not on the GPU."""
import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
import table_model as tm
from cpecan_amd import api

ALL = [c.name for c in tc.all_cases()]


def _flat(name):
    return [r for regs in tc.regions(name) for r in regs]


def _diagonal_of(anchor):
    return anchor[0] + anchor[1] + 2  # matrix coordinates are sequence coordinates + 1


@pytest.mark.parametrize("name", ALL)
def test_the_model_agrees_with_the_oracle_trace_and_with_host_planning(name):
    """cellOff is the oracle trace's cell_offset and the schedule has the oracle's number of tracebacks on every
    single-region problem; the host plans the model's regions, diagonals and cells (planning runs without a device)."""
    case = tc.case(name)
    om, op = ob.model(case.mtype), ob.params(**case.pkw)
    for (sx, sy, a, rl, rr), regs in zip(case.problems, tc.regions(name)):
        if len(regs) != 1 or len(sx) + len(sy) == 0:
            continue
        _, info = ob.aligned_pairs_traced(om, sx, sy, a, op, rl, rr)
        assert np.array_equal(info["cell_offset"], regs[0].cell_off), name
        assert info["n_tracebacks"] == len(regs[0].segs), name
    sm = api.stateMachine5_construct(case.mtype) if case.mtype in (0, 1) else api.stateMachine3_construct(case.mtype)
    with api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**case.pkw)) as b:
        b.add_many(case.problems)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):  # CPECAN_ESTATE: no table before upload
            b.table(0)
        try:
            b.upload()
        except api.CpecanError:
            pass  # no device here: planning has run
        st = b.stats()
    flat = _flat(name)
    if case.positions:  # what admits every class of the batch to the absolute-position sweeps
        assert all(r.smooth for r in flat) and not case.pkw.get("dynamicAnchorExpansion")
    assert (st.regions, st.diagonals, st.cells) == (len(flat), sum(r.lX + r.lY + 1 for r in flat), sum(r.cells for r in flat))


def test_chunk_case_has_every_chunk_shape():
    regs = _flat("chunks")
    assert sorted(r.lX + r.lY + 1 for r in regs) == [1, 2, 63, 64, 65, 127, 128, 129, 200, 1000]
    assert any(r.lX == 0 and r.lY > 0 for r in regs) and any(r.lY == 0 and r.lX > 0 for r in regs)
    assert any(len(tm.lane_starts(r.lX + r.lY + 1)) < tm.WAVE for r in regs)  # lanes without a diagonal
    n = 1000
    assert n - tm.lane_starts(n)[-1] < tm.chunk_of(n)  # the last lane with diagonals has a short chunk
    assert tm.lane_starts(129) == list(range(0, 129, 3)) and tm.lane_starts(64) == list(range(64))


def test_search_case_puts_anchors_around_lane_starts():
    regs = _flat("search")
    assert [len(r.anchors) for r in regs[:2]] == [0, 1]
    starts = tm.lane_starts(2 * tc.SEARCH_L + 1)
    assert _diagonal_of(regs[1].anchors[0]) in starts
    diags = [_diagonal_of(a) for a in regs[2].anchors]
    assert diags == list(tc.SEARCH_DIAGONALS)
    for off in (-1, 0, 1):
        assert any(d - off in starts for d in diags), off
    assert any(d - 1 in starts for d in diags if d - 2 in diags)                  # anchors on both sides of one lane's start
    assert sum(s + tm.chunk_of(321) <= diags[0] for s in starts) >= 2            # chunks entirely before the first anchor
    assert sum(s > diags[-1] for s in starts) >= 2                               # ... and behind the last
    assert all(_diagonal_of(a) in starts for a in regs[3].anchors) and len(regs[3].anchors) >= 50
    assert all(_diagonal_of(a) + 1 in starts for a in regs[4].anchors)


def test_dynamic_case_changes_expansion_at_lane_starts():
    r = _flat("dynamic")[0]
    starts = tm.lane_starts(r.lX + r.lY + 1)
    a = r.anchors
    # an anchor ON a lane's first diagonal whose successor has another expansion: a search that takes the successor's
    # interval there builds the diagonal with the wrong expansion
    assert sum(_diagonal_of(p) in starts and p[2] != q[2] for p, q in zip(a, a[1:])) >= 3
    assert any(p[2] == 0 and q[2] >= 20 for p, q in zip(a, a[1:])) and any(p[2] >= 20 and q[2] == 0 for p, q in zip(a, a[1:]))
    assert a[-1][2] >= 20 and sum(s > _diagonal_of(a[-1]) for s in starts) >= 20  # chunks behind the last anchor
    # the last anchor's expansion is in force there: the band behind it is wider than with expansion 0
    zero = tm.region_of(0, 0, r.lX, r.lY, [(x, y, 0) for x, y, _ in a], ob.params(**tc.case("dynamic").pkw))
    assert r.width[_diagonal_of(a[-1]) + 10] > zero.width[_diagonal_of(a[-1]) + 10]
    assert not r.smooth and tc.case("dynamic").positions is False


@pytest.mark.parametrize("name", ["queue", "queue-dynamic"])
def test_queue_cases_straddle_the_queue_depth(name):
    regs = _flat(name)
    assert [len(r.anchors) for r in regs] == list(tc.QUEUE_COUNTS) and {7, 8, 9, 16, 17} <= set(tc.QUEUE_COUNTS)
    for r in regs:  # no diagonal neighbours: the run shortcut is not what these walk through
        assert not any(q[0] == p[0] + 1 and q[1] == p[1] + 1 for p, q in zip(r.anchors, r.anchors[1:]))
    assert (len({a[2] for r in regs for a in r.anchors}) > 1) == (name == "queue-dynamic")


def _run_intervals(r, E):
    """(first diagonal, x - y, clear of the matrix edges) of every interval between two diagonal-neighbour anchors."""
    out, h = [], E // 2
    for p, q in zip(r.anchors, r.anchors[1:]):
        if q[0] == p[0] + 1 and q[1] == p[1] + 1:
            pX, pY = p[0] + 1, p[1] + 1
            out.append((pX + pY + 1, pX - pY, pX - h >= 0 and pY - h >= 0 and pX + 1 + h <= r.lX and pY + 1 + h <= r.lY))
    return out


@pytest.mark.parametrize("E", tc.RUN_EXPANSIONS)
def test_run_cases_have_every_run_and_the_shortcut_is_the_oracles_band(E):
    regs = _flat("runs-E%d" % E)
    assert [(r.lX, r.lY, len(r.anchors)) for r in regs[:4]] == [(n, n, n) for n in (1, 2, 3, 40)]  # corner to corner
    lengths = lambda r: [int(v) for v in api.anchor_runs(r.anchors)[:, 2]]
    assert lengths(regs[4]) == [1, 2, 3, 10] and lengths(regs[7]) == [10, 10]
    assert regs[5].anchors[0][0] == 0 and regs[6].anchors[0][1] == 0                     # a run from column 0 / row 0
    assert regs[4].anchors[-1][:2] == (regs[4].lX - 1, regs[4].lY - 1)                   # a run into the far corner
    assert regs[7].anchors[10][0] - regs[7].anchors[9][0] == 1 and regs[7].anchors[10][1] - regs[7].anchors[9][1] == 2
    taken = skipped = 0
    for r in regs:
        for d, xmy, clear in _run_intervals(r, E):
            want = [(xmy - E - 1, E + 2), (xmy - E, E + 1)]
            got = [(int(r.lo[d]), int(r.width[d])), (int(r.lo[d + 1]), int(r.width[d + 1]))]
            if clear:  # what cpk_band_in_run promises, held against the oracle's band
                assert got == want, (E, d)
                taken += 1
            else:
                skipped += got != want
    assert taken >= 40
    # at the far corner (and, from expansion 4 on, at column 0) the rectangle is cut by the matrix edge: the two
    # diagonals are NOT the shortcut's there
    assert (skipped > 0) == (E > 0)
    corner = [iv for iv in _run_intervals(regs[4], E) if iv[0] + 1 == regs[4].lX + regs[4].lY]
    assert len(corner) == 1 and corner[0][2] == (E == 0)


def _wraps_and_exact_fits(r):
    pos, wraps, exact = 0, 0, []
    for d, w in enumerate(int(v) for v in r.width):
        if pos + w > r.ring_cap:
            pos, wraps = 0, wraps + 1
        if pos + w == r.ring_cap:
            exact.append(d)
        pos += w
    return wraps, exact


def test_ring_whole_case_wraps_and_fills_the_ring_to_its_last_cell():
    regs = _flat("ring-whole")
    for r in regs:
        wraps, _ = _wraps_and_exact_fits(r)
        assert wraps >= 2 and len(r.segs) >= 3
        ring = tm.ring_whole(r.width, r.ring_cap)
        assert tm.ring_overlaps(ring, r.width, r.segs, r.ring_cap) is None  # the written rule passes the independent check
    # a diagonal that ends exactly on the ring's last cell: it stays where it is (pos + width > ringCap, not >=)
    assert sum(len(_wraps_and_exact_fits(r)[1]) > 0 for r in regs) >= 2


@pytest.mark.parametrize("name", ["ring-split-S5", "ring-split-S3"])
def test_ring_split_cases_have_segments_refresh_diagonals_and_lane_boundaries(name):
    regs = _flat(name)
    for r in regs:
        assert len(r.segs) >= 3
        for prev, top, frm in r.segs:  # a refresh diagonal that is neither of the two below the segment's top
            assert any((frm - d) % tm.REFRESH_PERIOD == 0 and d < top - 1 for d in range(prev + 1, frm + 1)), (prev, top, frm)
        S = 5 if name.endswith("S5") else 3
        off, end = tm.ring_split(r.width, r.segs, S)
        assert all(o % 2 == 0 for o in off) and end > r.cells
        kept = [tm.stores_every_state(d, r.segs) for d in range(len(r.width))]
        assert kept[0] and 0.1 < sum(kept) / len(kept) < 0.25  # every tenth diagonal and two per segment, not all
    r = regs[0]
    starts = tm.lane_starts(r.lX + r.lY + 1)
    assert r.segs == [(0, 50, 42), (42, 92, 84), (84, 120, 120)]
    assert all(top in starts and frm in starts for _, top, frm in r.segs[:2])


def test_chain_case_turns_back_on_every_part_of_a_chunk():
    regs = _flat("chains")
    assert all(r.smooth for r in regs)
    for r in regs[:2]:
        nD = r.lX + r.lY + 1
        chunk = tm.chunk_of(nD)
        hi = r.lo + 2 * (r.width - 1)
        assert any(r.lo[d] < r.lo[d - 1] > r.lo[d - 2] for d in range(2, nD))  # the low edge rises, then falls
        assert any(hi[d] > hi[d - 1] < hi[d - 2] for d in range(2, nD))        # the high edge falls, then rises
        for backward in (False, True):
            turns = [d for d in tm.danger_diagonals(r.lo, r.width, backward) if 0 < d < nD - 1]
            assert {0, chunk - 1} < {d % chunk for d in turns} and len({d % chunk for d in turns}) == chunk
    # smooth stretches: the replay of a lane reaches back (forward chain) or ahead (backward chain) over many chunks
    assert tm.danger_diagonals(regs[2].lo, regs[2].width) == [0] and tm.danger_diagonals(regs[2].lo, regs[2].width, True) == [200]
    for r, backward in ((regs[3], False), (regs[4], True)):
        d = tm.danger_diagonals(r.lo, r.width, backward)
        gaps = np.abs(np.diff(d + [0 if backward else r.lX + r.lY]))
        assert gaps.max() >= 40 * tm.chunk_of(r.lX + r.lY + 1)


def test_multi_region_case_cuts_problems_and_keeps_anchors_relative():
    per_problem = tc.regions("multi-region")
    assert max(len(regs) for regs in per_problem) >= 3 and sum(len(regs) > 1 for regs in per_problem) >= 1
    for (sx, sy, a, _, _), regs in zip(tc.case("multi-region").problems, per_problem):
        assert sum(len(r.anchors) for r in regs) == len(a)
        for r in regs:
            assert all(0 <= x < r.lX and 0 <= y < r.lY for x, y, _ in r.anchors)
            assert r.x1 + r.lX <= len(sx) and r.y1 + r.lY <= len(sy)
    assert sum(r.x1 > 0 and len(r.anchors) > 0 for regs in per_problem for r in regs) >= 3  # anchors moved to their rectangle


def test_mixed_case_spans_the_packed_and_the_wide_classes():
    regs = _flat("mixed")
    widest = [r.max_width for r in regs if r.lX + r.lY > 0]
    assert any(w <= 8 for w in widest) and any(8 < w <= 16 for w in widest) and any(16 < w <= 32 for w in widest)
    assert sum(w > 32 for w in widest) >= 5
    assert any(len(p) > 1 for p in tc.regions("mixed")) and any(r.lX + r.lY == 0 for r in regs)
    assert len({tuple(c.pkw.items()) for c in tc.all_cases()}) > 3  # (the other cases keep their own parameters)


# ---- the model's checks see what they are there for ----
def test_the_ring_check_sees_a_consistent_wrong_rule():
    r = _flat("ring-whole")[0]
    tight = tm.ring_whole(r.width, r.ring_cap - int(r.width.max()))  # laid out for a ring that is one diagonal short
    assert tm.ring_overlaps(tight, r.width, r.segs, r.ring_cap - int(r.width.max())) is not None
    shifted = [o + 1 for o in tm.ring_whole(r.width, r.ring_cap)]
    assert tm.ring_overlaps(shifted, r.width, r.segs, r.ring_cap) is not None  # leaves the ring at its end


def _chain(lo, width, max_width, backward, turn_back=True):
    """The position words of one direction by the documented procedure: re-base where the contract demands it or the
    three live diagonals no longer fit, centred in the slack."""
    hi = lo + 2 * (width - 1)
    P, n = max_width + tm.ABS_SLACK, len(lo)
    order = list(range(n))[::-1] if backward else list(range(n))
    must = set(tm.danger_diagonals(lo, width, backward)) if turn_back else {order[0]}
    out, B = {}, 0
    for k, d in enumerate(order):
        live = order[max(0, k - 2):k + 1]
        need_lo, need_hi = min(int(lo[q]) for q in live), max(int(hi[q]) for q in live)
        flag = d in must or (need_lo - B) >> 1 < 1 or (need_hi - B) >> 1 > P - 2
        if flag:
            span = ((need_hi - need_lo) >> 1) + 2
            B = (need_lo - 2 * (1 + max(0, P - 2 - span) // 2)) & ~1
        out[d] = ((int(lo[d]) - B) >> 1) | (int(flag) << 15)
    return out


def test_the_position_check_sees_a_missed_re_base_and_a_stale_base():
    r = _flat("chains")[0]
    fwd, bwd = _chain(r.lo, r.width, r.max_width, False), _chain(r.lo, r.width, r.max_width, True)
    words = np.array([fwd[d] | (bwd[d] << 16) for d in range(len(r.lo))], dtype=np.uint32).astype(np.int32)
    assert tm.check_dpos(r.lo, r.width, words, r.max_width) == []
    lazy = _chain(r.lo, r.width, r.max_width, False, turn_back=False)  # re-bases only when the rows are left
    words = np.array([lazy[d] | (bwd[d] << 16) for d in range(len(r.lo))], dtype=np.uint32).astype(np.int32)
    errs = tm.check_dpos(r.lo, r.width, words, r.max_width)
    assert errs and all("forward" in e and "must re-base" in e for e in errs)
    d = tm.danger_diagonals(r.lo, r.width)[3]
    stale = dict(fwd)
    stale[d + 1] ^= 1  # one position off under an unchanged flag: the base moved without a re-base
    words = np.array([stale[q] | (bwd[q] << 16) for q in range(len(r.lo))], dtype=np.uint32).astype(np.int32)
    assert any("diagonal %d has flag 0" % (d + 1) in e for e in tm.check_dpos(r.lo, r.width, words, r.max_width))


def test_first_difference_names_the_diagonal_and_the_field():
    r = _flat("ring-split-S5")[0]
    want = tm.expected_table(r, True, 5, 0)
    got = want.copy()
    got[17, 2] += 2
    assert tm.first_difference(want, want) is None
    assert tm.first_difference(got, want) == "diagonal 17 field ringOff: got %d, want %d" % (got[17, 2], want[17, 2])
