"""Constructed inputs of the list consumers (cpk_post.inl) at the chunk, tile and ring edges of the wave kernels.

Device-free: nothing here imports the library.  tests/test_consumer_cases_cpu.py proves with the oracle's traces and the
quadratic model what every input is for; tests/test_gpu_consumers_edges.py runs them through the kernels.

A pair is a (weight, x, y) tuple.  The figures the wave kernels turn on:
  WAVE  = 64    pairs per chunk of the MEA chain and of the ordered filter, entries of the register window, of the
                staircase buffer and of the column ring;
  TILE  = 2048  words of LDS: column counters of the ordered filter up to that many columns, places per step of the
                walks back along the predecessors.
"""
import random

import numpy as np

PROB_1 = 10000000
WAVE = 64
TILE = 2048
F085 = float(np.float32(0.85))


def anti_diagonal_order(cells):
    """The order the emitters list cells in: by anti-diagonal, then by x - y descending."""
    return sorted(cells, key=lambda c: (c[0] + c[1], -(c[0] - c[1])))


# ------------------------------------------------------------------------------------------------
# MEA chain.  A case: dict(pairs, gx, gy, lX, lY, gamma) + what the CPU file asserts about it:
#   walks:  {pair index (n = the sentinel): (visited, ended)}   by the oracle's trace
#   prev:   {pair index: predecessor}
#   record: {pair index: flag}
#   count:  length of the alignment (None: only "not empty")
#   lanes:  False where the lane kernel's quadratic walk would take seconds and the GPU file keeps to the wave form (none:
#           the longest, far_predecessor with 2.2 M steps of one lane, takes 0.6 s on the MI355X)
# ------------------------------------------------------------------------------------------------
def _mea(pairs, lX, lY, gx=(), gy=(), gamma=0.5, **expect):
    c = dict(pairs=[tuple(p) for p in pairs], gx=[tuple(g) for g in gx], gy=[tuple(g) for g in gy], lX=lX, lY=lY,
             gamma=float(np.float32(gamma)), walks={}, prev={}, record={}, count=None, lanes=True)
    c.update(expect)
    return c


def _fan(k, first=1):
    """k cells on one anti-diagonal, x = first .. first + k - 1: none dominates another."""
    return [(first + t, first + k - 1 - t) for t in range(k)]


def mea_fan(k, prefix=0, with_target=True):
    """A record R = (0, 0) of weight 9e6, a fan of k pairs of negative weight behind it (each chains from R and stays under
    the top, so none is a record), and -- with_target -- one pair P that dominates them all: P's walk (or the sentinel's)
    passes the k fan pairs and ends on R, the (k + 1)-th most recent pair, which is also its best predecessor.
    prefix: pairs in front of R that nothing but the sentinel dominates (they move P along the chunks)."""
    lX = lY = k + 2 + prefix
    pre = [(1, lX - 1 - t, 0) for t in range(prefix)]  # y = 0: dominated by the sentinel alone; R is not dominated by them
    fan = []
    for t, (x, y) in enumerate(_fan(k)):
        fan.append((-3 - (t % 5), x, y))
    pairs = pre + [(9000000, 0, 0)] + fan
    r = prefix
    c = _mea(pairs, lX, lY)
    if with_target:
        pairs.append((4000000, k + 1, k + 1))
        c = _mea(pairs, lX, lY)
        i = len(pairs) - 1
        c["walks"] = {i: (k + 1, 1), len(pairs): (1, 1)}
        c["prev"] = {i: r, len(pairs): i}
        c["count"] = 2
    else:
        c["walks"] = {len(pairs): (k + 1, 1)}
        c["prev"] = {len(pairs): r}
        c["count"] = 1
    for t in range(k):
        c["record"][r + 1 + t] = 0
    c["record"][r] = 1
    return c


def mea_runoff(f, tie=(2, 9)):
    """Pair 0 a record nothing but the sentinel dominates; a fan of f pairs of coarse weights that start chains of their
    own and stay under the top (no records); then three pairs on a further anti-diagonal that dominate the whole fan: pairs
    f + 1, f + 2, f + 3 walk back over every earlier pair and run off the front.  The fan's best weight sits on the two
    pairs `tie` (places back from pair f, 0 the most recent) -- the more recent is the predecessor -- and on nothing else.
    The three targets set records, so the sentinel takes the last of them: the tie-break shows in the alignment."""
    lX = lY = f + 8
    pairs = [(9000000, lX - 1, 0)]
    for t, (x, y) in enumerate(_fan(f, 1)):
        pairs.append((6000000 if f - 1 - t in tie else 2000000 * (1 + t % 2), x, y))
    for t in range(3):  # x > f, y > f: above the whole fan; one anti-diagonal: none dominates another
        pairs.append((4000000, f + 1 + t, f + 3 - t))
    c = _mea(pairs, lX, lY)
    for t in range(3):
        i = f + 1 + t
        c["walks"][i] = (i, 0)
        c["prev"][i] = f - min(tie)
        c["record"][i] = 1
    c["walks"][len(pairs)] = (1, 1)
    c["prev"][len(pairs)] = f + 3
    c["count"] = 2
    return c


def mea_tie_64_apart():
    """The fan's best weight on two pairs exactly 64 places apart -- the same lane of the register window and of the first
    fetched chunk: the more recent one is the predecessor."""
    return mea_runoff(100, tie=(5, 69))


def mea_tie_start():
    """A candidate equal to the from-the-start score does not replace it: pair 0 has weight 0 (chain score 0, a record by
    `>=`), pair 1 dominates it and scores w + 0 == w either way: it keeps no predecessor, and the alignment is pair 1 alone."""
    c = _mea([(0, 0, 0), (5000000, 1, 1)], 2, 2)
    c.update(prev={1: -1, 2: 1}, record={0: 1, 1: 1}, walks={1: (1, 1)}, count=1)
    return c


def mea_tie_record_rounding():
    """An end score EQUAL to the running top is a record (`>=`), and the walk of a later pair stops there -- shown on gap
    masses beyond 2^24, where the float casts round and stopping is not lossless, so the rule is visible in the alignment.
    gamma 0.5.  gapX: 2^25 + 2 on row 1, 2 on row 2.
      pair 0 = A (17777216, 1, 1): from the start, no mass in front: 17777216; behind it 2 -> end score 17777217, a record.
      pair 1 = B (999999, 0, 0):   999999; behind it 2^25 + 4 (exact in float) -> + 2^24 + 2 = 17777217 == top: a record.
      pair 2 = C (2000000, 2, 2):  walks back to B first: the mass between is 2^25 + 2, which the float cast rounds to 2^25:
                                   2000000 + 999999 + 2^24 = 19777215; B is a record, so the walk ends and A -- which
                                   would give 2000000 + 17777216 + 0 = 19777216 -- is never looked at.
    Alignment B, C.  With `>` for `>=` B is no record and C chains from A."""
    big = (1 << 25) + 2
    c = _mea([(17777216, 1, 1), (999999, 0, 0), (2000000, 2, 2)], 3, 3, gx=[(big, 1, -1), (2, 2, -1)])
    c.update(prev={2: 1, 3: 2}, record={0: 1, 1: 1}, walks={2: (1, 1)}, count=2)
    return c


def mea_handoff(lane):
    """A walk of 101 pairs from the pair at place `lane` (0 or 63) of a chunk: beyond the register window it reads the
    best / record / H words the wave stored at the end of the chunk before."""
    k = 100
    prefix = (lane - (1 + k)) % WAVE  # P's index is prefix + 1 + k
    c = mea_fan(k, prefix=prefix)
    assert (prefix + 1 + k) % WAVE == lane
    return c


def mea_diagonal(n, gamma=0.5, gaps=False):
    """n pairs (i, i), every one in the chain: walks of one, so the lane kernel stays linear."""
    rng = random.Random(n)
    pairs = [(rng.randrange(1000000, 9000001), i, i) for i in range(n)]
    # (light gap masses: no pair is worth skipping)
    gx = [(rng.randrange(1, 1000), rng.randrange(n), -1) for _ in range(n // 3)] if gaps and n else []
    gy = [(rng.randrange(1, 1000), -1, rng.randrange(n)) for _ in range(n // 3)] if gaps and n else []
    c = _mea(pairs, max(n, 1), max(n, 1), gx, gy, gamma)
    c["count"] = n
    c["walks"] = {n: (1, 1)} if n else {}
    return c


def mea_length(n, seed):
    """A list of n pairs in emitter order around a noisy diagonal, weights and dense gap lists with the -1 coordinate the
    indel emitter writes, gamma float32(0.85).  The sentinel is entry n: the last lane of a chunk at n = 63, lane 0 of a
    chunk of its own at n = 64."""
    rng = random.Random(seed)
    L = max(4, (2 * n) // 3 + 3)
    cells = set()
    while len(cells) < n:
        i = rng.randrange(L)
        cells.add((i, min(L - 1, max(0, i + rng.randrange(-2, 3)))))
    pairs = [(rng.randrange(1, PROB_1 + 1), x, y) for x, y in anti_diagonal_order(cells)]
    gx = [(rng.randrange(100000, 2500000), x, -1) for x in range(L) for _ in range(2)]
    gy = [(rng.randrange(100000, 2500000), -1, y) for y in range(L) for _ in range(2)]
    return _mea(pairs, L, L, gx, gy, F085)


def mea_far_predecessor():
    """The chain's predecessor more than a tile back: E = (0, 0), a block of 46 x 46 cells of weight -1 in emitter order
    (2116 pairs: each chains from E or from a block pair and stays under the top, none is a record, none is chosen), then
    L = (47, 47): its walk passes the whole block, ends on E, and E is its best predecessor."""
    block = anti_diagonal_order([(x, y) for x in range(1, 47) for y in range(1, 47)])
    pairs = [(9000000, 0, 0)] + [(-1, x, y) for x, y in block] + [(4000000, 47, 47)]
    c = _mea(pairs, 48, 48)
    i = len(pairs) - 1
    c.update(walks={i: (i, 1), i + 1: (1, 1)}, prev={i: 0, i + 1: i}, count=2)
    return c


def mea_empty_chain():
    """n = 70 pairs of negative weight: the sentinel's from-the-start score 0 beats every chain: count 0 with n > 0."""
    pairs = [(-1000 - i, i, i) for i in range(70)]
    c = _mea(pairs, 70, 70)
    c.update(prev={70: -1}, count=0)
    return c


def mea_empty_list():
    """n = 0 with gap lists: the sentinel alone; the score is the whole gap mass times gamma."""
    c = _mea([], 5, 4, gx=[(3000000, 1, -1), (2000000, 4, -1)], gy=[(1000000, -1, 0)])
    c.update(count=0)
    return c


def mea_cases():
    cases = {}
    for k1 in (1, 64, 65, 128, 129, 193):  # the walk ends on the k1-th most recent pair
        cases["walk_%d_pair" % k1] = mea_fan(k1 - 1)
        cases["walk_%d_sentinel" % k1] = mea_fan(k1 - 1, with_target=False)
    cases["runoff_64_65_66"] = mea_runoff(63)
    cases["runoff_128_129_130"] = mea_runoff(127)
    cases["tie_64_apart"] = mea_tie_64_apart()
    cases["tie_start_score"] = mea_tie_start()
    cases["tie_record_rounding"] = mea_tie_record_rounding()
    cases["handoff_lane_0"] = mea_handoff(0)
    cases["handoff_lane_63"] = mea_handoff(63)
    for n in (1, 63, 64, 65, 127, 128, 129):
        cases["length_%d" % n] = mea_length(n, 100 + n)
    cases["empty_list_with_gaps"] = mea_empty_list()
    cases["empty_chain"] = mea_empty_chain()
    cases["one_by_one"] = _mea([(7000000, 0, 0)], 1, 1, count=1)
    cases["gamma_zero"] = mea_diagonal(40, gamma=0.0, gaps=True)
    cases["no_gap_lists"] = mea_diagonal(90)
    for n1 in (2048, 2049, 4097):  # n + 1 entries with the sentinel
        cases["diagonal_%d" % n1] = mea_diagonal(n1 - 1, gamma=F085 if n1 == 2049 else 0.5, gaps=n1 != 2048)
    cases["far_predecessor"] = mea_far_predecessor()
    return cases


MEA_EMPTY = ("empty_list_with_gaps", "empty_chain")  # the cases whose alignment is empty by design


# ------------------------------------------------------------------------------------------------
# Ordered filter.  A case: dict(pairs, lX, lY, gamma) + what the CPU file asserts:
#   m:       pairs that take part
#   columns: {x: qualifying pairs in that column}
#   other keys are read by the test of the same name in the CPU file
# ------------------------------------------------------------------------------------------------
def _ord(pairs, lX, lY, gamma=0.5, **expect):
    c = dict(pairs=[tuple(p) for p in pairs], lX=lX, lY=lY, gamma=gamma, lanes=True)
    c.update(expect)
    return c


def ord_diagonal(m, interleave=True, seed=0):
    """m qualifying pairs (i, i) of random weight >= 0.5 and, interleaved, pairs under matchGamma, of weight 0 and of
    negative weight at other cells: m != n."""
    rng = random.Random(1000 + m + seed)
    pairs = []
    for i in range(m):
        pairs.append((rng.randrange(5000000, PROB_1 + 1), i, i))
        if interleave:
            pairs.append((rng.choice([4999999, 0, -5, 1200000]), i, (i + 1 + rng.randrange(3)) % max(m, 2) if m > 1 else 1))
    if m == 0:
        pairs = [(4999999, 0, 0), (0, 1, 1), (-7, 2, 2), (1, 0, 2), (3000000, 2, 0)]
    L = max(m, 3)
    cells = set()
    out = []
    for p in pairs:  # distinct cells only
        if (p[1], p[2]) not in cells:
            cells.add((p[1], p[2]))
            out.append(p)
    return _ord(out, L, L, 0.5, m=m)


def ord_gamma85():
    """matchGamma = float32(0.85) = 0.85000002...: weight 8 500 000 is out, 8 500 001 is in."""
    pairs = []
    for i in range(40):
        pairs.append((8500001 if i % 2 else 8500000, i, i))
    return _ord(pairs, 40, 40, 0.85, m=20)


def ord_columns(lX):
    """Qualifying pairs in column 0 and in column lX - 1 (and a few between): lX <= 2048 counts the columns in LDS, beyond
    in global memory."""
    rng = random.Random(lX)
    lY = 50
    xs = sorted({0, lX - 1} | {rng.randrange(lX) for _ in range(30)})
    pairs = []
    for x in xs:
        for y in sorted({rng.randrange(lY) for _ in range(2)}):
            pairs.append((rng.randrange(5000000, PROB_1), x, y))
    pairs.append((9999999, 0, 0) if (0, 0) not in {(p[1], p[2]) for p in pairs} else (1, 0, lY - 1))
    rng.shuffle(pairs)
    cells, out = set(), []
    for p in pairs:
        if (p[1], p[2]) not in cells:
            cells.add((p[1], p[2]))
            out.append(p)
    return _ord(out, lX, lY, 0.3)


def ord_column_of(c, shuffled=True, equal=False):
    """One column (x = 1) of c qualifying pairs between a pair at (0, 0) and pairs at (2, c + 1), (3, c + 2): the ring of a
    column's scores holds 64.  equal: one weight throughout the column -- every pair of it scores the same."""
    rng = random.Random(c)
    col = [(6000000 if equal else rng.randrange(5000000, PROB_1), 1, 1 + j) for j in range(c)]
    if shuffled:
        rng.shuffle(col)
    pairs = [(7000000, 0, 0)] + col + [(6000000, 2, c + 1), (5000000, 3, c + 2)]
    return _ord(pairs, 4, c + 3, 0.5, m=c + 3, columns={1: c})


def ord_column_at(start, c):
    """`start` pairs (i, i), then a column of c pairs: it begins at place `start` of the sorted order."""
    rng = random.Random(start * 131 + c)
    pairs = [(rng.randrange(5000000, PROB_1), i, i) for i in range(start)]
    ys = list(range(start, start + c))
    rng.shuffle(ys)
    pairs += [(rng.randrange(5000000, PROB_1), start, y) for y in ys]
    pairs += [(6000000, start + 1, start + c)]
    return _ord(pairs, start + 2, start + c + 1, 0.5, m=start + c + 1, columns={start: c}, first_place=start)


def ord_monotone(a):
    """a pairs (i, i) append a entries to the staircase; directly behind them a pair that does not extend the alignment
    (column a, y = a // 2): a binary search right after the register buffer of 64 entries is full, or empty again."""
    rng = random.Random(a)
    pairs = [(rng.randrange(5000000, PROB_1), i, i) for i in range(a)]
    pairs.append((5500000, a, a // 2))
    pairs.append((6000000, a + 1, a + 1))
    return _ord(pairs, a + 2, a + 2, 0.5, m=a + 2, inside=a)


def ord_staircase_moves():
    """On 20 entries (i, 2 i) of score 0.1 (i + 1), in later columns:
      pair 20 (9e6, y 5):    scores 0.3 + 0.9: the entries at y = 6 .. 22 (scores 0.4 .. 1.2) go, the tail moves left;
      pair 21 (0.5e6, y 25): 1.3 + 0.05 under the 1.4 at y 26: goes into the middle, drops none, the tail moves right;
      pair 22 (0.5e6, y 34): the same y as an entry (1.8) with a lower score 1.7 + 0.05: redundant;
      pair 23 (1e6, y 32):   the same y with an EQUAL score (the same sum of seventeen 0.1): the later column replaces;
      pair 24 (1.5e6, y 30): the same y with a higher score 1.5 + 0.15 (under the 1.7 above): replaces that entry alone;
      pair 25 (9e6, y 39), pair 26 (1e6, y 40) in ONE column, listed in that order: pair 26 is dominated by the entry below."""
    pairs = [(1000000, i, 2 * i) for i in range(20)]
    pairs += [(9000000, 20, 5), (500000, 21, 25), (500000, 22, 34), (1000000, 23, 32), (1500000, 24, 30),
              (9000000, 25, 39), (1000000, 25, 40), (4000000, 26, 41)]
    return _ord(pairs, 27, 42, 0.0, m=28)


def ord_descending(k=100):
    """x ascending, y strictly descending, weights descending: every insert goes to position 0 and drops nothing."""
    pairs = [(9000000 - 50000 * i, i, k - 1 - i) for i in range(k)]
    return _ord(pairs, k, k, 0.0, m=k)


def ord_pred_sources():
    """100 pairs (i, i), then (100, 98) -- predecessor at place 97, in the current chunk of 64 places: readlane -- and
    (101, 10) -- predecessor at place 9, a chunk the wave stored long ago: memory; the diagonal's own pairs take theirs from
    the last entry: registers."""
    rng = random.Random(5)
    pairs = [(rng.randrange(5000000, PROB_1), i, i) for i in range(100)]
    pairs += [(5000000, 100, 98), (5000000, 101, 10), (5000000, 102, 102)]
    return _ord(pairs, 103, 103, 0.5, m=103)


def ord_tie_smaller_y():
    """Two ends of one column with equal chain scores: (1, 5) listed before (1, 2) and the other way round in column 3;
    the end at the smaller y is the one later pairs chain from."""
    pairs = [(5000000, 0, 0), (6000000, 1, 5), (6000000, 1, 2), (5000000, 2, 7),
             (6000000, 3, 9), (6000000, 3, 12), (5000000, 4, 14)]
    return _ord(pairs, 5, 15, 0.5, m=7)


def ord_tie_later_column():
    """Equal chain scores at the SAME y in a later column: (1, 3) and (2, 3) both score 0.5 + 0.6; the later column's pair
    replaces the earlier one's and is what (3, 4) chains from."""
    pairs = [(5000000, 0, 0), (6000000, 1, 3), (6000000, 2, 3), (5000000, 3, 4)]
    return _ord(pairs, 4, 5, 0.5, m=4)


def ord_many(m):
    """m qualifying pairs on at most 2049 columns, two to a column at (x, x) and (x, x + 1): the walk back along the
    predecessors takes more than one tile of 2048 places."""
    rng = random.Random(m)
    pairs = []
    x = 0
    while len(pairs) < m:
        pairs.append((rng.randrange(5000000, PROB_1), x, x))
        if len(pairs) < m:
            pairs.append((rng.randrange(5000000, PROB_1), x, x + 1))
        x += 1
    return _ord(pairs, x, x + 1, 0.5, m=m)


def ord_far_predecessor():
    """(0, 0), then 1050 columns of two light pairs above y = 1, then (1051, 1) with a weight that makes it the best end:
    its only possible predecessor is place 0, 2101 places back -- more than a tile."""
    pairs = [(9000000, 0, 0)]
    for x in range(1, 1051):
        pairs += [(1, x, x + 1), (1, x, x + 2)]
    pairs.append((9000000, 1051, 1))
    return _ord(pairs, 1052, 1053, 0.0, m=2102)


def ord_random_ties(seed):
    rng = random.Random(seed)
    lX, lY = rng.randrange(1, 14), rng.randrange(1, 14)
    cells = list({(rng.randrange(lX), rng.randrange(lY)) for _ in range(rng.randrange(0, 60))})
    rng.shuffle(cells)
    pairs = [(rng.randrange(-1, 5) * 2500000, x, y) for x, y in cells]
    return _ord(pairs, lX, lY, rng.choice([0.0, 0.25, 0.5]))


def ordered_cases():
    cases = {}
    for m in (0, 1, 63, 64, 65, 128, 129):
        cases["m_%d" % m] = ord_diagonal(m)
    cases["gamma_085"] = ord_gamma85()
    for lX in (1, 2047, 2048, 2049):
        cases["columns_%d" % lX] = ord_columns(lX)
    for c in (1, 2, 63, 64, 65, 66, 130):
        cases["column_of_%d" % c] = ord_column_of(c)
    cases["column_equal_weights"] = ord_column_of(12, equal=True)
    cases["column_10_at_place_60"] = ord_column_at(60, 10)
    cases["column_fills_chunk"] = ord_column_at(64, 64)
    for a in (63, 64, 65, 128, 129):
        cases["monotone_%d" % a] = ord_monotone(a)
    cases["staircase_moves"] = ord_staircase_moves()
    cases["descending_y"] = ord_descending()
    cases["pred_sources"] = ord_pred_sources()
    cases["tie_smaller_y"] = ord_tie_smaller_y()
    cases["tie_later_column"] = ord_tie_later_column()
    for m in (2048, 2049, 4097):
        cases["many_%d" % m] = ord_many(m)
    cases["far_predecessor"] = ord_far_predecessor()
    return cases


ORDERED_EMPTY = ("m_0",)
ORDERED_SINGLE = ("columns_1", "descending_y")  # a chain of one pair by design: one column; no pair below another
REPEATED_CELL = dict(pairs=[(6000000, 0, 0), (7000000, 1, 1), (5000000, 2, 2), (7000000, 1, 1), (5000000, 3, 3)], lX=4, lY=4,
                     gamma=0.5)  # refused: cell (1, 1) twice


# ------------------------------------------------------------------------------------------------
# Left shift: dict(pairs, sx, sy); `chain` False where list 0 is not a chain.
# ------------------------------------------------------------------------------------------------
def shift_cases():
    cases = {}
    # a gap inside a homopolymer: the shift travels to the left end of the run
    cases["homopolymer"] = dict(pairs=[(5, 0, 0), (6, 1, 1), (7, 2, 2), (8, 9, 6), (9, 10, 7)], sx="CAAAAAAAAAG", sy="CAAAAAAG")
    # the run reaches the left end of both sequences
    cases["homopolymer_to_the_end"] = dict(pairs=[(8, 7, 4), (9, 8, 5)], sx="AAAAAAAAG", sy="AAAAAG")
    # the slide meets the row of the pair in front: the `x2 == x || y2 == y` break
    cases["break_on_row"] = dict(pairs=[(4, 1, 1), (6, 5, 2), (7, 6, 3)], sx="CAAAAAG", sy="CAAG")
    # the empty alignment on identical sequences: min(lX, lY) entries of score 1
    cases["empty_on_identical"] = dict(pairs=[], sx="ACGTTGCAAC" * 3, sy="ACGTTGCAAC" * 3)
    cases["empty_on_prefix"] = dict(pairs=[], sx="GATTACA", sy="GATTACA")
    # lower case and N: compared in upper case, N equals N
    cases["lower_case_and_n"] = dict(pairs=[(3, 0, 0), (9, 8, 5)], sx="caaNnaaag", sy="CAnNAG")
    # list 0 is no chain: (3, 6) is followed by (5, 2), which is skipped over by the pairs behind it
    cases["not_a_chain"] = dict(pairs=[(2, 0, 0), (3, 3, 6), (4, 5, 2), (5, 7, 8), (6, 9, 9)], sx="ACGTACGTAC", sy="ACGTTCGTAC",
                                chain=False)
    return cases


# ------------------------------------------------------------------------------------------------
# Reweighting and scores: dict(pairs, lX, lY, gammas)
# ------------------------------------------------------------------------------------------------
MASS_MAX = PROB_1 + (1 << 31)  # the largest listed mass of a row or column the library takes


def _row_of_mass(total, lY_extra=0):
    """One row (x = 0) whose pairs list exactly `total`, at most PROB_1 a pair, each in a column of its own."""
    ws = [PROB_1] * (total // PROB_1) + ([total % PROB_1] if total % PROB_1 else [])
    return dict(pairs=[(w, 0, j) for j, w in enumerate(ws)], lX=1, lY=len(ws) + lY_extra)


def reweight_cases():
    cases = {}
    for n in (0, 255, 256, 257, 1000):  # the stride loop and the 256-wide reduction
        rng = random.Random(n)
        L = max(4, n // 2)
        cells = set()
        while len(cells) < n:
            cells.add((rng.randrange(L), rng.randrange(L)))
        cases["n_%d" % n] = dict(pairs=[(rng.randrange(1, 4000000), x, y) for x, y in sorted(cells)], lX=L, lY=L)
    # rows that list 1x, 1.5x and 3x PROB_1: the unaligned mass floors at 0
    pairs = [(PROB_1, 0, 0), (PROB_1, 1, 1), (5000000, 1, 2), (PROB_1, 2, 3), (PROB_1, 2, 4), (PROB_1, 2, 5), (2500000, 3, 6)]
    cases["floor_at_zero"] = dict(pairs=pairs, lX=4, lY=7)
    cases["mass_at_bound"] = _row_of_mass(MASS_MAX)
    for c in cases.values():
        c["gammas"] = (0.5, F085, 0.85, 2.0, 50.0, 0.0, -1.0)  # 50: weights go negative (truncation towards zero)
    cases["mass_at_bound"]["gammas"] = (0.5, 0.0)
    return cases


MASS_BEYOND = _row_of_mass(MASS_MAX + 1)  # refused
IDENTITY = dict(sx="ACGTNnacgtNAC", sy="ACGTNNACGANaC",
                pairs=[(5, i, i) for i in range(13)])  # N = N does not count, lower case does
