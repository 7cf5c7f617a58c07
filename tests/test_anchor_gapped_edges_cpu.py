"""What the inputs of tests/anchor_gapped_edge_cases.py are for, asserted with the model alone (tests/anchor_model_gapped.py;
no device): the runs at both band edges, the gaps with N and lower case, the long gaps with their options, the tie, the
capped chains, the passes without rows and the launches of the pass over the scratch budget.  Every figure here is the
model's; tests/test_gpu_anchor_gapped_edges.py holds the kernels to the same model on the same inputs, and is vacuous
wherever one of these assertions would fail."""
import ctypes as C
import functools

import numpy as np
import pytest

import anchor_cases as ac
import anchor_gapped_edge_cases as ec
import anchor_model as am
import anchor_model_gapped as ag
import anchor_model_threshold as ath
import anchor_stages as st

P = am.default_params()
SCORE = np.array(P["scores"], dtype=np.int64).reshape(5, 5)


def _once(pair, softMask=True, params=P, **kw):
    return ag.anchors_once(pair[0], pair[1], 14, softMask, params, **kw)


def _diagonals(runs):
    return [(x - y, n) for x, y, n in runs]


def _columns(runs):
    return sum(r[2] for r in runs)


def _chain(pair, softMask=True, params=P):
    hsps, _, _ = ath._hsps(pair[0], pair[1], softMask, params, 0, 0)
    return [hsps[i][:3] for i in am.chain(hsps)]


def _codes(pair):
    return am._CODE[am._bytes(pair[0])], am._CODE[am._bytes(pair[1])]


def _gap(pair, g=1):
    """(lower corner, upper corner) of gap g of the pair's chain."""
    chain = _chain(pair)
    corners = [(0, 0)] + [(x + n, y + n) for x, y, n in chain]
    starts = [(x, y) for x, y, n in chain] + [(len(pair[0]), len(pair[1]))]
    return corners[g], starts[g]


def _walks(pair, g=1, maxDiagonals=ag.MAX_DIAGONALS):
    """Both extensions of gap g before the overlap rule, and (m, n)."""
    (ax, ay), (bx, by) = _gap(pair, g)
    cx, cy = _codes(pair)
    gx, gy = cx[ax:bx], cy[ay:by]
    return (ag.right_extension(gx, gy, SCORE, ag.Y_DROP, maxDiagonals),
            ag.right_extension(gx[::-1], gy[::-1], SCORE, ag.Y_DROP, maxDiagonals), (len(gx), len(gy)))


# ---- 1. both band edges ----
BAND_RUNS = {
    "insertion of 3": [(0, 222), (-3, 222)],
    "insertion of 31": [(0, 222), (-31, 222)],
    "insertion of 32": [(0, 222)],
    "deletion of 31, swapped": [(0, 229), (-31, 184)],
    "deletion of 32, swapped": [(0, 222)],
}


@pytest.mark.parametrize("case", sorted(ec.BAND))
def test_the_band_ends_at_minus_31_too(case):
    assert sorted(ec.BAND) == sorted(BAND_RUNS)
    for softMask in (True, False):
        on, _ = _once(ec.BAND[case], softMask, gapped=1)
        assert _diagonals(on) == BAND_RUNS[case], softMask
    off, _ = _once(ec.BAND[case])
    assert _diagonals(off) == BAND_RUNS[case][:1]


def test_the_insertion_of_31_runs_along_the_last_diagonal_that_is_a_cell():
    """The I chain of 31 goes down the first column of the gap: cell (i, 0) is on diagonal i, and the last of them, i = 31,
    has no cell on the diagonal below it."""
    (best, (i, j), blocks), _, _ = _walks(ec.BAND["deletion of 31, swapped"])
    assert blocks[0][0] - blocks[0][1] == -31 and best > 0
    (best, (i, j), blocks), _, _ = _walks(ec.BAND["insertion of 31"])
    assert [b[0] - b[1] for b in blocks] == [-31]


# ---- 2. N and lower case inside a gap ----
@pytest.mark.parametrize("case", sorted(ec.MASKED))
def test_n_and_lower_case_inside_a_gap_are_crossed(case):
    sx, sy = ec.MASKED[case]
    assert b"N" in sx + sy or sy != sy.upper()
    for softMask in (True, False):
        on, _ = _once((sx, sy), softMask, gapped=1)
        off, _ = _once((sx, sy), softMask)
        assert _diagonals(on) == [(0, 222), (3, 217)] and _diagonals(off) == [(0, 222)], softMask
    # the masked columns lie inside the second run: one block crosses them
    (x, y, n) = on[1]
    masked = [k for k in range(len(sy)) if sy[k:k + 1] in (b"N", b"a", b"c", b"g", b"t")]
    assert masked and all(y <= k < y + n for k in masked)


# ---- 3. the long gaps ----
LONG_RUNS = {   # option: (runs, anchor columns) of long_gap and of limit_gap, steps 1-5b
    "default": ((13, 1755), (16, 1957)),
    "64 diagonals": ((3, 416), (4, 338)),
    "1000 diagonals": ((10, 1169), (10, 1091)),
    "yDrop 1": ((2, 413), (2, 334)),
    "yDrop 2^31 - 1": ((13, 1755), (16, 1957)),
}


@functools.lru_cache(maxsize=None)
def _long(which, option):
    pair = ec.long_gap() if which == 0 else ec.limit_gap()
    return tuple(_once(pair, gapped=1, **ec.LONG_OPTIONS[option])[0])


@pytest.mark.parametrize("which", [0, 1])
def test_the_options_of_a_long_gap_all_matter(which):
    assert sorted(LONG_RUNS) == sorted(ec.LONG_OPTIONS)
    for option in ec.LONG_OPTIONS:
        runs = _long(which, option)
        assert (len(runs), _columns(runs)) == LONG_RUNS[option][which], option
    default = _long(which, "default")
    for option in ("64 diagonals", "1000 diagonals", "yDrop 1"):
        assert _long(which, option) != default
        for other in ("64 diagonals", "1000 diagonals", "yDrop 1"):
            assert option == other or _long(which, option) != _long(which, other)
    assert _long(which, "yDrop 2^31 - 1") == default
    pair = ec.long_gap() if which == 0 else ec.limit_gap()
    assert list(_long(which, "yDrop 1")) == _once(pair)[0]                # nothing survives the first transversion
    assert len(_chain(pair)) == 2 and len(set(r[0] - r[1] for r in default)) >= 9


def test_the_long_gap_has_many_blocks_on_the_way_back():
    (ax, ay), (bx, by) = _gap(ec.long_gap())
    assert (bx - ax) + (by - ay) == 3356                                   # under the limit: an extension may cross it all
    (bestR, _, blocksR), (bestL, _, blocksL), _ = _walks(ec.long_gap())
    assert len(blocksR) == 11 and len(blocksL) == 12                       # slots cap - 1 downwards, and 0 upwards
    assert bestR > bestL                                                   # the right one stays: eleven blocks from the top


def test_the_limit_binds_on_both_extensions_of_one_gap():
    pair = ec.limit_gap()
    (ax, ay), (bx, by) = _gap(pair)
    m, n = bx - ax, by - ay
    assert (m, n) == (2250, 2258) and m + n > ag.MAX_DIAGONALS
    (bestR, (iR, jR), blocksR), (bestL, (iL, jL), blocksL), _ = _walks(pair)
    assert iR + jR <= 4096 and iL + jL <= 4096 and iR + jR > 4000 and iL + jL > 4000
    # the overlap rule fires: both are there before it, one after it
    assert blocksR and blocksL and (iR + iL > m or jR + jL > n) and bestR != bestL
    cx, cy = _codes(pair)
    keptR, keptL = ag.gap_extensions(cx, cy, (ax, ay), (bx, by), True, True, SCORE, ag.Y_DROP, ag.MAX_DIAGONALS)
    assert (keptR == [], len(keptL)) == (True, len(blocksL)) if bestR < bestL else (len(keptR), keptL == []) == (len(blocksR), True)
    # with room for the whole gap the result is another one
    wide = ag.extend_chain(cx, cy, _chain(pair), SCORE, ag.Y_DROP, 8192)
    wide = [(x + 14, y + 14, length - 28) for x, y, length in wide if length > 28]
    assert wide != list(_long(1, "default")) and _columns(wide) > 1957


def test_the_tie_gap_ties_and_the_rule_shows_in_the_runs():
    pair = ec.tie_gap()
    (bestR, reachR, blocksR), (bestL, reachL, blocksL), (m, n) = _walks(pair)
    assert bestR == bestL > 0 and reachR == reachL and 2 * reachR[0] > m
    (ax, ay), (bx, by) = _gap(pair)
    right = [(ax + i, ay + j, length) for i, j, length in blocksR]
    left = sorted((bx - i - length, by - j - length, length) for i, j, length in blocksL)
    assert right != left                                                   # the homopolymer: each walk drops another A
    cx, cy = _codes(pair)
    keptR, keptL = ag.gap_extensions(cx, cy, (ax, ay), (bx, by), True, True, SCORE, ag.Y_DROP, ag.MAX_DIAGONALS)
    assert keptR == right and keptL == []
    on, _ = _once(pair, gapped=1)
    assert _diagonals(on) == [(0, 122), (3, 30), (4, 37), (7, 122)]
    # had the rule kept the left one, the trimmed runs would differ
    other = [(x + 14, y + 14, length - 28) for x, y, length in left if length > 28]
    assert other != on[1:3] and len(other) == 2


def _path_score(cx, cy, blocks):
    """What an alignment scores whose aligned columns are `blocks` [(i, j, length)], from the corner to its last column."""
    total, i, j = 0, 0, 0
    for bi, bj, length in blocks:
        for skipped in (bi - i, bj - j):
            total -= ag.GAP_OPEN + skipped * ag.GAP_EXTEND if skipped else 0
        total += int(sum(SCORE[cx[bi + k], cy[bj + k]] for k in range(length)))
        i, j = bi + length, bj + length
    return total


def test_the_source_tie_gap_has_two_ways_back_of_one_score():
    pair = ec.source_tie_gap()
    (ax, ay), (bx, by) = _gap(pair)
    assert (ax, ay, bx - ax, by - ay) == (150, 150, 48, 45)                # the HSPs end where the N begin
    cx, cy = _codes(pair)
    gx, gy = cx[ax:bx], cy[ay:by]
    (bestR, reachR, blocksR), (bestL, _, blocksL), _ = _walks(pair)
    assert blocksR == [(0, 0, 19), (21, 19, 3), (25, 22, 13)] and reachR == (38, 35)
    other = [(0, 0, 22), (25, 22, 13)]                                     # the gap of 3 in one piece, the column (G, G) not won
    assert _path_score(gx, gy, blocksR) == _path_score(gx, gy, other) == bestR
    # the first run is the HSP and the block of 19 behind it; the other way back would make it 150 + 22 - 28 long
    on, _ = _once(pair, gapped=1)
    assert on == [(14, 14, 150 + 19 - 28), (212, 209, 122)]


# ---- 4. a capped chain ----
@pytest.mark.parametrize("maxHsps, chained, runs, columns, plain", [(5, 5, 36, 1283, (5, 517)), (1, 1, 37, 1198, (1, 164))])
def test_a_capped_chain_leaves_gaps_thousands_of_cells_wide(maxHsps, chained, runs, columns, plain):
    pair = ac.random_pair(2, 3000)
    params = am.default_params(maxHsps=maxHsps)
    on, counts = _once(pair, params=params, gapped=1)
    off, counts_off = _once(pair, params=params)
    assert counts == counts_off == dict(hits=872, hsps=46, chained=chained, capped=1)
    assert (len(on), _columns(on)) == (runs, columns) and (len(off), _columns(off)) == plain and len(on) > len(off)
    rows = ag.gap_rows_each(_chain(pair, params=params), len(pair[0]), len(pair[1]))
    assert max(rows) >= 2 * 1000                                           # a gap with m + n in the thousands
    for g in range(1, chained + 1):
        if rows[g] >= 2000:
            (_, _, blocksR), (_, _, blocksL), _ = _walks_of(pair, params, g)
            assert max(len(blocksR), len(blocksL)) >= 12                   # dozens of blocks, one extension alone a dozen
            break
    else:
        raise AssertionError("no wide gap between two HSPs")


def _walks_of(pair, params, g):
    chain = _chain(pair, params=params)
    corners = [(0, 0)] + [(x + n, y + n) for x, y, n in chain]
    starts = [(x, y) for x, y, n in chain] + [(len(pair[0]), len(pair[1]))]
    cx, cy = _codes(pair)
    gx, gy = cx[corners[g][0]:starts[g][0]], cy[corners[g][1]:starts[g][1]]
    return ag.right_extension(gx, gy, SCORE), ag.right_extension(gx[::-1], gy[::-1], SCORE), (len(gx), len(gy))


def test_the_recursion_on_a_capped_chain_gives_the_recorded_integers():
    pair = ac.random_pair(2, 3000)
    for maxHsps, want in ((5, (14, 929)), (1, (3, 340))):
        _, stats = ag.find_anchor_runs(pair[0], pair[1], params=am.default_params(maxHsps=maxHsps))
        assert (stats["runs"], stats["anchorColumns"], stats["capped"]) == want + (1,)


# ---- 5. passes without rows ----
def test_the_zero_row_problems_have_no_rows():
    for name, (sx, sy) in ec.zero_row_problems().items():
        assert len(sx) * len(sy) > 500 * 500, name
        runs, stats = ag.find_anchor_runs(sx, sy, gapped=1)
        chain = _chain((sx, sy))
        assert ag.gap_rows(chain, len(sx), len(sy)) == 0, name
        if name == "identical":
            assert chain == [(0, 0, 1500)] and runs.tolist() == [[14, 14, 1472, 20]] and stats["subProblems"] == 0
        else:
            assert chain == [] and (stats["hsps"], stats["runs"], stats["subProblems"]) == (0, 0, 1), name
            # the sub-pass is the same problem again, soft mask on as well: no rows there either
        _, _, strand = ag.find_anchor_runs_stranded(sx, sy, "both", gapped=1)
        assert strand["strand"] == "plus" and strand["scoreMinus"] == 0, name     # strand "both" searches the same problem


# ---- 6. a pass over the scratch budget ----
@functools.lru_cache(maxsize=None)
def _template_rows(t):
    sx, sy = ec.sliced_template(t)
    return tuple(ag.gap_rows_each(_chain((sx, sy)), len(sx), len(sy)))


SLICED_ROWS = (32292, 29440, 32404, 29596, 32372, 29644, 32456, 29548)     # scratch rows of the eight templates


def test_the_templates_of_the_sliced_batch():
    for t in range(ec.SLICED_TEMPLATES):
        sx, sy = ec.sliced_template(t)
        rows = _template_rows(t)
        assert (len(sx), len(sy)) == ((8800, 8790) if t % 2 == 0 else (8100, 8090))
        assert sum(rows) == SLICED_ROWS[t] == ag.gap_rows(_chain((sx, sy)), len(sx), len(sy))
        assert len(rows) - 1 in (5, 6, 7) and rows[0] == rows[-1] == 0 and sum(rows) % 8192 != 0
        on, _ = _once((sx, sy), gapped=1)
        off, _ = _once((sx, sy))
        assert (len(on), len(off)) == (9, 5), t                            # every conserved stretch is won, deletion crossed
    assert sum(SLICED_ROWS) == 247752


def test_the_templates_recurse():
    """Cached by the GPU file as well; here once, for the sub-problems that make the second pass of the sliced batch."""
    for t in (0, 1):
        sx, sy = ec.sliced_template(t)
        _, stats = ag.find_anchor_runs(sx, sy, gapped=1)
        assert (stats["runs"], stats["subProblems"]) == (9, 4)


def test_the_sliced_batch_takes_three_launches_and_one_ends_inside_a_problem():
    slots = ec.sliced_slots()
    assert len(slots) == 280
    orders = [tuple(o) for o in ec.sliced_orders()]
    assert all(sorted(o) == list(range(8)) for o in orders) and len(set(orders)) == ec.SLICED_ROUNDS
    assert all(a != b for a, b in zip(slots, slots[1:]))                   # neighbouring slots differ
    total = sum(SLICED_ROWS[t] for t in slots)
    assert 2 * ec.BUDGET_ROWS < total < 3 * ec.BUDGET_ROWS and total == 35 * 247752
    # the gap boundaries as anchor_pass_gapped collects them: rowBase of the problem plus the rows in front of the gap
    bounds, starts, at = [], set(), 0
    for t in slots:
        starts.add(at)
        for rows in _template_rows(t):
            bounds.append(at)
            at += rows
    bounds.append(at)
    starts.add(at)
    assert at == total
    L = st.stages()
    L.cpk_anchor_gapped_slice_end.restype = C.c_int64
    L.cpk_anchor_gapped_slice_end.argtypes = [st.i64p, C.c_int64, C.c_int64, C.c_int64]
    arr = (C.c_int64 * len(bounds))(*bounds)
    lo, cuts = 0, []
    while lo < total:
        hi = L.cpk_anchor_gapped_slice_end(arr, len(bounds), lo, ec.BUDGET_ROWS)
        assert lo < hi <= lo + ec.BUDGET_ROWS
        cuts.append(hi)
        lo = hi
    assert len(cuts) == 3 and cuts[-1] == total
    assert cuts[0] > ec.BUDGET_ROWS - 8192 and cuts[1] - cuts[0] > ec.BUDGET_ROWS - 8192     # the first two are full
    assert any(cut not in starts for cut in cuts[:2])                      # a launch ends between two gaps of one problem


def test_gap_rows_restates_the_sizing_of_the_pass():
    assert ag.gap_rows_each([], 300, 200) == [0] and ag.gap_rows([], 300, 200) == 0
    chain = [(10, 20, 50), (60, 70, 5), (3000, 4000, 100)]
    assert ag.gap_rows_each(chain, 3200, 4100) == [30, 0, 2 * 4096, 100]
    assert ag.gap_rows_each(chain, 3200, 4100, 64) == [30, 0, 128, 64] and ag.gap_rows(chain, 3200, 4100, 64) == 222
