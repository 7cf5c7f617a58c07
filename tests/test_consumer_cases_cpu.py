"""What every input of tests/consumer_cases.py is for, proved without a device: with the oracle's traces
(ob.mea_alignment_traced, ob.filter_pairs_ordered_traced), the quadratic model of the ordered filter
(tests/ordered_model.py) and plain arithmetic.  A case that loses the property it is named for fails here, so
tests/test_gpu_consumers_edges.py cannot quietly stop walking an edge; and no expected output is empty or trivial but
the ones named empty.  The oracle's ordered filter is held to the model list for list as well, on every ordered case and on
300 random small lists with many exact ties.  The two refusals of the library (a repeated cell, a row mass beyond the
int32 range) are made by the host before a device is looked for, so they are tested here."""
import numpy as np
import pytest

import consumer_cases as cc
import oracle_binding as ob
import ordered_model as om
from cpecan_amd import api

MEA = cc.mea_cases()
ORD = cc.ordered_cases()
SHIFT = cc.shift_cases()
REW = cc.reweight_cases()


def _tuples(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


# ------------------------------------------------------------------------------------------------ MEA chain
def _mea_trace(c):
    return ob.mea_alignment_traced(c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"], c["gamma"])


@pytest.mark.parametrize("name", sorted(MEA))
def test_mea_case_has_its_named_walks_predecessors_and_records(name):
    c = MEA[name]
    al, score, tr = _mea_trace(c)
    for i, (visited, ended) in c["walks"].items():
        assert (int(tr["visited"][i]), int(tr["ended"][i])) == (visited, ended), (name, i)
    for i, p in c["prev"].items():
        assert int(tr["prev"][i]) == p, (name, i)
    for i, r in c["record"].items():
        assert int(tr["record"][i]) == r, (name, i)
    if c["count"] is not None:
        assert len(al) == c["count"], name
    if name in cc.MEA_EMPTY:
        assert len(al) == 0
    else:
        assert len(al) >= 1 and score > 0.0
    # every coordinate is one the host accepts
    assert all(0 <= x < c["lX"] and 0 <= y < c["lY"] for _, x, y in c["pairs"])
    assert all(0 <= x < c["lX"] for _, x, _ in c["gx"]) and all(0 <= y < c["lY"] for _, _, y in c["gy"])


def test_mea_walks_end_on_the_named_places_of_the_window_and_the_fetched_chunks():
    """The walk of one pair and of the sentinel ends on a dominated record at exactly the 1st, 64th, 65th, 128th, 129th and
    193rd most recent pair; the stopping record is the best predecessor (the stop lane itself takes part)."""
    for k1 in (1, 64, 65, 128, 129, 193):
        for who in ("pair", "sentinel"):
            c = MEA["walk_%d_%s" % (k1, who)]
            _, _, tr = _mea_trace(c)
            i = len(c["pairs"]) - (1 if who == "pair" else 0)
            assert int(tr["visited"][i]) == k1 and int(tr["ended"][i]) == 1
            assert int(tr["prev"][i]) == i - k1  # the record the walk ended on
            assert not tr["record"][i - k1 + 1:i].any()  # nothing in between is a record


def test_mea_walks_run_off_the_front():
    for name, targets in (("runoff_64_65_66", (64, 65, 66)), ("runoff_128_129_130", (128, 129, 130))):
        c = MEA[name]
        _, _, tr = _mea_trace(c)
        for i in targets:
            assert int(tr["visited"][i]) == i and int(tr["ended"][i]) == 0 and int(tr["prev"][i]) >= 1


def test_mea_ties():
    # two fan pairs of the best weight in different lanes of one chunk: 3 and 10 pairs back from pair f + 1
    c = MEA["runoff_64_65_66"]
    f = 63
    best = [i for i in range(1, f + 1) if c["pairs"][i][0] == 6000000]
    assert best == [f - 9, f - 2] and max(p[0] for p in c["pairs"][1:f + 1]) == 6000000
    al, _, tr = _mea_trace(c)
    assert int(tr["prev"][f + 1]) == f - 2 and _tuples(al)[0] == c["pairs"][f - 2]  # the more recent; visible in the alignment
    # ... and exactly 64 apart: the same lane of the register window and of the first fetched chunk
    c = MEA["tie_64_apart"]
    f = 100
    best = [i for i in range(1, f + 1) if c["pairs"][i][0] == 6000000]
    assert best == [f - 69, f - 5] and best[1] - best[0] == cc.WAVE
    al, _, tr = _mea_trace(c)
    for t in (f + 1, f + 2, f + 3):
        assert int(tr["prev"][t]) == f - 5
        assert (t - 1 - (f - 5)) % cc.WAVE == (t - 1 - (f - 69)) % cc.WAVE and (t - 1 - (f - 5)) < cc.WAVE <= (t - 1 - (f - 69))
    assert _tuples(al)[0] == c["pairs"][f - 5]
    # a candidate equal to the from-the-start score does not replace it
    c = MEA["tie_start_score"]
    al, _, tr = _mea_trace(c)
    assert c["pairs"][0][0] == 0 and int(tr["prev"][1]) == -1 and _tuples(al) == [c["pairs"][1]]


def test_mea_record_on_an_equal_end_score_where_the_float_casts_round():
    c = MEA["tie_record_rounding"]
    (wA, _, _), (wB, _, _), (wC, _, _) = c["pairs"]
    big = c["gx"][0][0]
    f32 = np.float32
    half = f32(0.5)
    assert big > 1 << 24 and float(f32(big)) != big  # the cast rounds
    end_a = float(f32(wA)) + float(f32(2) * half)
    end_b = float(f32(wB)) + float(f32(big + 2) * half)
    assert float(f32(wA)) == wA and end_a == end_b  # B's end score EQUALS the running top A set
    via_b = int(wC + float(wB) + float(f32(big) * half))
    via_a = int(wC + float(wA) + 0.0)
    assert via_a > via_b  # what a walk that went on to A would have preferred
    al, score, tr = _mea_trace(c)
    assert [int(v) for v in tr["record"][:2]] == [1, 1] and int(tr["prev"][2]) == 1 and int(tr["visited"][2]) == 1
    assert _tuples(al) == [c["pairs"][1], c["pairs"][2]]


def test_mea_hand_off_places():
    for lane in (0, 63):
        c = MEA["handoff_lane_%d" % lane]
        i = len(c["pairs"]) - 1
        _, _, tr = _mea_trace(c)
        assert i % cc.WAVE == lane and i >= cc.WAVE and int(tr["visited"][i]) == 101 > cc.WAVE


def test_mea_lengths_and_sentinel_places():
    ns = sorted(len(MEA[k]["pairs"]) for k in MEA if k.startswith("length_")) + [len(MEA["empty_list_with_gaps"]["pairs"])]
    assert sorted(ns) == [0, 1, 63, 64, 65, 127, 128, 129]
    assert MEA["empty_list_with_gaps"]["gx"] and MEA["empty_list_with_gaps"]["gy"]
    for k in MEA:
        if k.startswith("length_"):
            c = MEA[k]
            assert all(y == -1 for _, _, y in c["gx"]) and all(x == -1 for _, x, _ in c["gy"])  # as the indel emitter writes them
            assert c["gamma"] == cc.F085 != 0.85
            if len(c["pairs"]) >= 63:
                assert sum(g[0] for g in c["gx"]) > 1 << 24  # cumulative masses beyond the float's integers
                al, _, tr = _mea_trace(c)
                assert len(al) >= 3 and int(tr["visited"].max()) >= 4  # chains, with walks over several pairs
    assert MEA["gamma_zero"]["gamma"] == 0.0 and MEA["gamma_zero"]["gx"]
    assert not MEA["no_gap_lists"]["gx"] and not MEA["no_gap_lists"]["gy"]
    assert (MEA["one_by_one"]["lX"], MEA["one_by_one"]["lY"]) == (1, 1)


def test_mea_tile_cases():
    for n1 in (2048, 2049, 4097):
        c = MEA["diagonal_%d" % n1]
        n = len(c["pairs"])
        al, _, tr = _mea_trace(c)
        assert n + 1 == n1 and len(al) == n and int(tr["visited"].max()) == 1  # every pair chained, walks of one
    c = MEA["far_predecessor"]
    n = len(c["pairs"])
    al, _, tr = _mea_trace(c)
    assert int(tr["prev"][n]) == n - 1 and int(tr["prev"][n - 1]) == 0 and n - 1 > cc.TILE
    assert _tuples(al) == [c["pairs"][0], c["pairs"][n - 1]]
    c = MEA["empty_chain"]
    al, score, tr = _mea_trace(c)
    assert len(c["pairs"]) == 70 and len(al) == 0 and int(tr["prev"][70]) == -1 and score == 0.0


# ------------------------------------------------------------------------------------------------ ordered filter
def _ord_trace(c):
    return ob.filter_pairs_ordered_traced(c["pairs"], c["lX"], c["lY"], c["gamma"])


def _places(c):
    """Place of every qualifying pair in the order the wave kernel sorts them into: by column, list order inside."""
    q = om.qualifying(c["pairs"], c["gamma"])
    order = sorted(q, key=lambda i: (c["pairs"][i][1], i))
    return {i: k for k, i in enumerate(order)}


@pytest.mark.parametrize("name", sorted(ORD))
def test_ordered_case_oracle_equals_model_and_is_not_trivial(name):
    c = ORD[name]
    want, tr = _ord_trace(c)
    assert _tuples(want) == om.filter_pairs_ordered(c["pairs"], c["gamma"])
    assert _tuples(want) == _tuples(ob.filter_pairs_ordered(c["pairs"], c["lX"], c["lY"], c["gamma"]))
    assert tr["m"] == len(om.qualifying(c["pairs"], c["gamma"]))
    if "m" in c:
        assert tr["m"] == c["m"]
    for x, k in c.get("columns", {}).items():
        assert sum(1 for i in om.qualifying(c["pairs"], c["gamma"]) if c["pairs"][i][1] == x) == k
    cells = [(x, y) for _, x, y in c["pairs"]]
    assert len(set(cells)) == len(cells) and all(0 <= x < c["lX"] and 0 <= y < c["lY"] for x, y in cells)
    if name in cc.ORDERED_EMPTY:
        assert len(want) == 0 and len(c["pairs"]) > 0
    else:
        assert len(want) >= 1
        if tr["m"] >= 3 and name not in cc.ORDERED_SINGLE:
            assert len(want) >= 2


def test_oracle_filter_equals_model_on_random_lists_with_ties():
    kept = 0
    for seed in range(300):
        c = cc.ord_random_ties(seed)
        want = _tuples(ob.filter_pairs_ordered(c["pairs"], c["lX"], c["lY"], c["gamma"]))
        assert want == om.filter_pairs_ordered(c["pairs"], c["gamma"]), seed
        kept += len(want)
    assert kept > 600


def test_ordered_qualifying_counts_and_gamma():
    assert [ORD["m_%d" % m]["m"] for m in (0, 1, 63, 64, 65, 128, 129)] == [0, 1, 63, 64, 65, 128, 129]
    for m in (1, 63, 64, 65, 128, 129):
        c = ORD["m_%d" % m]
        assert len(c["pairs"]) > m  # pairs that take no part are interleaved
        ws = {w for w, _, _ in c["pairs"]}
        assert m < 63 or (ws & {0} and ws & {-5} and ws & {4999999})
    c = ORD["m_0"]
    assert {w <= 0 for w, _, _ in c["pairs"]} == {True, False}
    c = ORD["gamma_085"]
    q = om.qualifying(c["pairs"], c["gamma"])
    assert {c["pairs"][i][0] for i in q} == {8500001} and {w for w, _, _ in c["pairs"]} == {8500000, 8500001}
    assert 8500000 / cc.PROB_1 >= 0.85 and not 8500000 / cc.PROB_1 >= float(np.float32(0.85))


def test_ordered_column_counter_cases():
    for lX in (2047, 2048, 2049, 1):
        c = ORD["columns_%d" % lX]
        xs = {c["pairs"][i][1] for i in om.qualifying(c["pairs"], c["gamma"])}
        assert c["lX"] == lX and 0 in xs and lX - 1 in xs
    assert cc.TILE == 2048


def test_ordered_column_sizes_and_places():
    assert [ORD["column_of_%d" % k]["columns"][1] for k in (1, 2, 63, 64, 65, 66, 130)] == [1, 2, 63, 64, 65, 66, 130]
    for k in (63, 130):  # list order inside the column is not y order
        ys = [y for _, x, y in ORD["column_of_%d" % k]["pairs"] if x == 1]
        assert ys != sorted(ys)
    c = ORD["column_equal_weights"]
    assert len({w for w, x, _ in c["pairs"] if x == 1}) == 1
    ys = [y for _, x, y in c["pairs"] if x == 1]
    assert ys != sorted(ys) and ys[0] != min(ys)
    want, tr = _ord_trace(c)
    assert (6000000, 1, min(ys)) in _tuples(want)  # of equal scores the smaller y is the end later pairs chain from
    c = ORD["column_10_at_place_60"]
    pl = _places(c)
    col = sorted(pl[i] for i, p in enumerate(c["pairs"]) if p[1] == 60)
    assert col == list(range(60, 70))  # straddles the chunk edge at 64
    c = ORD["column_fills_chunk"]
    pl = _places(c)
    col = sorted(pl[i] for i, p in enumerate(c["pairs"]) if p[1] == 64)
    assert col == list(range(64, 128))  # places 0 .. 63 of the second chunk


def test_ordered_staircase_cases():
    for a in (63, 64, 65, 128, 129):
        c = ORD["monotone_%d" % a]
        _, tr = _ord_trace(c)
        assert tr["extended"][:a].all() and (tr["query"][:a] == 1).all()  # a entries appended
        assert int(tr["query"][a]) == 0 and c["pairs"][a][1:] == (a, a // 2)  # then a search inside
    c = ORD["staircase_moves"]
    _, tr = _ord_trace(c)
    d, e = tr["dropped"], tr["extended"]
    assert int(d[20]) == 9 and not e[20]      # drops several: the tail moves left
    assert int(d[21]) == 0 and not e[21]      # into the middle, drops none: the tail moves right
    assert int(d[22]) == -1                   # the same y, lower score: redundant
    assert int(d[23]) == 1 and not e[23]      # the same y, equal score: the later column replaces
    assert int(d[24]) == 1 and not e[24]      # the same y, higher score
    q, pred, score, _ = om.chain(c["pairs"], c["gamma"])
    assert score[22] < score[17] and c["pairs"][22][2] == c["pairs"][17][2]
    assert score[23] == score[16] and c["pairs"][23][2] == c["pairs"][16][2]
    assert score[24] > score[15] and c["pairs"][24][2] == c["pairs"][15][2]
    # one column, listed lower y first: the second pair is dominated by the entry the first has just become
    assert c["pairs"][25][1] == c["pairs"][26][1] and c["pairs"][25][2] < c["pairs"][26][2] and score[25] > score[26]
    c = ORD["descending_y"]
    _, tr = _ord_trace(c)
    assert len(c["pairs"]) == 100 and (tr["dropped"][1:] == 0).all() and not tr["extended"][1:].any()


def _pred_sources(c):
    """Where the wave kernel finds the predecessor's score: 'registers' (the last staircase entry), 'readlane' (a place of
    the current chunk), 'memory' (a place of an earlier chunk)."""
    _, tr = _ord_trace(c)
    pl = _places(c)
    kinds = {}
    for i, k in pl.items():
        p = int(tr["pred"][i])
        if p < 0:
            continue
        if tr["query"][i]:
            kinds[i] = "registers"
        else:
            kinds[i] = "readlane" if pl[p] >= k - k % cc.WAVE else "memory"
    return kinds


def test_ordered_predecessor_score_sources():
    c = ORD["pred_sources"]
    kinds = _pred_sources(c)
    assert kinds[100] == "readlane" and kinds[101] == "memory" and kinds[50] == "registers"
    assert set(kinds.values()) == {"registers", "readlane", "memory"}
    assert set(_pred_sources(ORD["many_4097"]).values()) == {"registers", "readlane", "memory"}


def test_ordered_ties():
    c = ORD["tie_smaller_y"]
    q, pred, score, _ = om.chain(c["pairs"], c["gamma"])
    assert score[1] == score[2] and score[4] == score[5]
    assert int(pred[3]) == 2 and int(pred[6]) == 4  # the end at the smaller y, whichever was listed first
    want, _ = _ord_trace(c)
    assert _tuples(want) == [c["pairs"][i] for i in (6, 4, 3, 2, 0)]
    c = ORD["tie_later_column"]
    q, pred, score, _ = om.chain(c["pairs"], c["gamma"])
    assert score[1] == score[2] and c["pairs"][1][2] == c["pairs"][2][2] and int(pred[3]) == 2
    want, _ = _ord_trace(c)
    assert _tuples(want) == [c["pairs"][i] for i in (3, 2, 0)]


def test_ordered_walk_back_cases():
    for m in (2048, 2049, 4097):
        c = ORD["many_%d" % m]
        want, tr = _ord_trace(c)
        assert tr["m"] == m and c["lX"] <= 2049 and len(want) > 1000
    c = ORD["far_predecessor"]
    want, tr = _ord_trace(c)
    pl = _places(c)
    last = len(c["pairs"]) - 1
    assert int(tr["pred"][last]) == 0 and pl[last] - pl[0] > cc.TILE
    assert _tuples(want) == [c["pairs"][last], c["pairs"][0]]


# ------------------------------------------------------------------------------------------------ the two refusals
def test_repeated_cell_is_refused_before_a_device_is_looked_for():
    """the oracle keeps the copy with the lower index, the kernels the one with the higher, and the
    reference every copy; the library refuses the list."""
    c = cc.REPEATED_CELL
    cells = [(x, y) for _, x, y in c["pairs"]]
    assert len(set(cells)) == len(cells) - 1
    with pytest.raises(api.CpecanError, match="more than once"):
        api.filterPairwiseAlignmentToMakePairsOrdered(c["pairs"], "A" * c["lX"], "A" * c["lY"], c["gamma"])
    with pytest.raises(api.CpecanError, match="more than once"):  # also when the copies differ in weight or take no part
        api.filterPairwiseAlignmentToMakePairsOrdered([(1, 0, 0), (9000000, 0, 0)], "A", "A", 0.5)


def test_row_mass_bound_of_the_reweighting():
    """The kernel keeps PROB_1 minus the listed mass in an int32.  At the bound the int32 is INT32_MIN, which floors at 0
    like the oracle's int64; one unit beyond it wraps to INT32_MAX and would read as unaligned mass: refused."""
    at, beyond = REW["mass_at_bound"], cc.MASS_BEYOND
    assert sum(w for w, _, _ in at["pairs"]) == cc.MASS_MAX == cc.PROB_1 + 2 ** 31
    assert sum(w for w, _, _ in beyond["pairs"]) == cc.MASS_MAX + 1
    wrap = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    assert wrap(cc.PROB_1 - cc.MASS_MAX) == -2 ** 31 and wrap(cc.PROB_1 - cc.MASS_MAX - 1) == 2 ** 31 - 1
    assert cc.MASS_MAX // cc.PROB_1 == 215
    with pytest.raises(api.CpecanError, match="mass"):
        api.reweightAlignedPairs2(beyond["pairs"], beyond["lX"], beyond["lY"], 0.5)
    with pytest.raises(api.CpecanError, match="mass"):  # the lower end: negative weights
        api.reweightAlignedPairs2([(-2 ** 31, 0, 0), (-2 ** 31, 0, 1)], 1, 2, 0.5)
    # the oracle at the bound: the row has no unaligned mass left, each column has PROB_1 minus its pair
    got = ob.reweight_aligned_pairs(at["pairs"], at["lX"], at["lY"], 0.5)
    assert [int(w) for w in got[:, 0]] == [int(w - 0.5 * (cc.PROB_1 - w)) for w, _, _ in at["pairs"]]


# ------------------------------------------------------------------------------------------------ left shift
def _left_shift(pairs, sx, sy):
    """impl/pairwiseAligner.c:1726-1762 in plain Python; also returns the smallest index it read the sequences at."""
    out, low = [], 1 << 30
    x, y = len(sx), len(sy)
    sx, sy = sx.upper(), sy.upper()
    for w, x2, y2 in reversed(pairs):
        while x - x2 > 1 or y - y2 > 1:
            low = min(low, x - 1, y - 1)
            if sx[x - 1] != sy[y - 1]:
                break
            out.append((w, x - 1, y - 1))
            x, y = x - 1, y - 1
            if x2 == x or y2 == y:
                break
        if x2 < x and y2 < y:
            out.append((w, x2, y2))
            x, y = x2, y2
    while x > 0 and y > 0 and sx[x - 1] == sy[y - 1]:
        out.append((pairs[0][0] if pairs else 1, x - 1, y - 1))
        x, y = x - 1, y - 1
    return out[::-1], low


@pytest.mark.parametrize("name", sorted(SHIFT))
def test_left_shift_case(name):
    c = SHIFT[name]
    want, low = _left_shift(c["pairs"], c["sx"], c["sy"])
    assert low >= 0  # (a list that is no chain can send the reference's loop in front of the sequence: not this one)
    assert _tuples(ob.left_shift_alignment(c["pairs"], c["sx"], c["sy"])) == want
    assert len(want) >= 2 and len(want) <= len(c["pairs"]) + min(len(c["sx"]), len(c["sy"]))
    chain = all(u[1] < v[1] and u[2] < v[2] for u, v in zip(c["pairs"], c["pairs"][1:]))
    assert chain == c.get("chain", True)


def test_left_shift_named_properties():
    want, _ = _left_shift(**SHIFT["homopolymer"])
    assert len(want) == 8 and want[0] == (5, 0, 0)
    assert [t[1] - t[2] for t in want] == [0] + [3] * 7  # the gap of three has travelled to the left end of the run
    want, _ = _left_shift(**SHIFT["homopolymer_to_the_end"])
    assert want[0] == (8, 3, 0) and len(want) == 6  # travelled to the left end of Y, score borrowed from the first pair
    c = SHIFT["break_on_row"]
    want, _ = _left_shift(**c)
    assert want == [(4, 4, 1), (6, 5, 2), (7, 6, 3)]  # one step, then y2 == y: the slide stops on the row of the pair in front
    c = SHIFT["empty_on_identical"]
    want, _ = _left_shift(**c)
    assert want == [(1, i, i) for i in range(len(c["sx"]))] and len(want) == min(len(c["sx"]), len(c["sy"]))  # shiftCap's bound
    c = SHIFT["lower_case_and_n"]
    assert any(ch.islower() for ch in c["sx"]) and "N" in c["sx"].upper() and "N" in c["sy"].upper()
    want, _ = _left_shift(**c)
    assert len(want) > len(c["pairs"])


# ------------------------------------------------------------------------------------------------ reweighting, scores
def test_reweight_cases():
    assert sorted(len(REW["n_%d" % n]["pairs"]) for n in (0, 255, 256, 257, 1000)) == [0, 255, 256, 257, 1000]
    c = REW["floor_at_zero"]
    rows = {}
    for w, x, _ in c["pairs"]:
        rows[x] = rows.get(x, 0) + w
    assert [rows[x] / cc.PROB_1 for x in range(4)] == [1.0, 1.5, 3.0, 0.25]
    got = ob.reweight_aligned_pairs(c["pairs"], c["lX"], c["lY"], 0.5)
    assert int(got[0, 0]) == cc.PROB_1 and int(got[3, 0]) == cc.PROB_1  # rows and columns at or over PROB_1: nothing unaligned
    assert int(got[6, 0]) == 2500000 - int(0.5 * (7500000 + 7500000))  # negative: truncated towards zero
    for name, c in REW.items():
        assert 0.0 in c["gammas"]
        if name != "mass_at_bound":
            assert -1.0 in c["gammas"] and 50.0 in c["gammas"] and cc.F085 in c["gammas"] and 0.85 in c["gammas"]
            if len(c["pairs"]) >= 255:
                got = ob.reweight_aligned_pairs(c["pairs"], c["lX"], c["lY"], 50.0)
                assert (got[:, 0] < 0).any() and (got[:, 0] > -2 ** 31).all()
                a = ob.reweight_aligned_pairs(c["pairs"], c["lX"], c["lY"], cc.F085)
                b = ob.reweight_aligned_pairs(c["pairs"], c["lX"], c["lY"], 0.85)
                assert (a[:, 0] != b[:, 0]).any()  # float32 against double gamma
    assert np.isnan(ob.score_by_posterior_ignoring_gaps([]))
    c = cc.IDENTITY
    assert ob.score_by_identity(c["sx"], c["sy"], c["pairs"]) == 100.0 * 2 * 9 / 26  # N = N does not count, lower case does
