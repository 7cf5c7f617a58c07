"""Inputs of the next-runs tests (the hand-off of the trainer's updateTheBand; include/cpecan_realign.h), shared by the CPU
suite (tests/test_next_runs_cpu.py) and the GPU suites (tests/test_gpu_next_runs.py, tests/test_gpu_em_update_band.py).
Nothing here touches a device.

HAND: lists worked out by hand -- (name, pairs, sX, sY, trim, expected runs without the expansion).
random_chains(): 500 random chains.
CASES: realign-style inputs for the batch stage.  A case is sequences by name, cigars as the arguments of realign.Cigar and
the realign options; problems(case) are the problems cPecanRealign makes of them (cPecanRealign.c:511-529).
em_world(): the inputs of the trainer tests."""
import collections
import functools
import random

import numpy as np

import oracle_binding as ob

M, DX, IY = 0, 1, 2  # CPECAN_OP_MATCH, _INDEL_X (bases of X only), _INDEL_Y
PROB_1 = 10000000
GAP_GAMMA, MATCH_GAMMA = 0.5, float(np.float32(0.85))  # cPecanRealign's defaults (the latter a float there)
MARGIN = 1e-4  # no reweighted weight this close to matchGamma, no posterior this close to the threshold

_X10 = "ACGTACGTAC"
HAND = (
    ("empty", (), _X10, _X10, 0, ()),
    ("one-pair", ((2, 2),), _X10, _X10, 0, ((2, 2, 1),)),
    ("one-pair-trimmed", ((2, 2),), _X10, _X10, 1, ()),
    ("block-of-6-trim-3", tuple((i, i) for i in range(6)), _X10, _X10, 3, ()),  # shorter than 2 * trim + 1
    ("block-of-7-trim-3", tuple((i, i) for i in range(7)), _X10, _X10, 3, ((3, 3, 1),)),
    ("block-of-10-trim-0", tuple((i, i) for i in range(10)), _X10, _X10, 0, ((0, 0, 10),)),
    ("block-of-10-trim-3", tuple((i, i) for i in range(10)), _X10, _X10, 3, ((3, 3, 4),)),
    ("mismatch-in-the-middle", tuple((i, i) for i in range(10)), _X10, "ACGTTCGTAC", 0, ((0, 0, 4), (5, 5, 5))),
    ("mismatch-in-the-middle-trim-2", tuple((i, i) for i in range(10)), _X10, "ACGTTCGTAC", 2, ((2, 2, 2), (5, 5, 3))),
    ("n-against-n", tuple((i, i) for i in range(10)), "ACGTNCGTAC", "ACGTNCGTAC", 0, ((0, 0, 4), (5, 5, 5))),
    ("lower-against-upper", tuple((i, i) for i in range(10)), "acgtacgtac", _X10, 0, ((0, 0, 10),)),
    ("lower-n-against-n", tuple((i, i) for i in range(10)), "acgtncgtac", "ACGTNCGTAC", 0, ((0, 0, 4), (5, 5, 5))),
    ("block-ends-at-the-corner", ((6, 5), (7, 6), (8, 7), (9, 8)), _X10, "AAAAAGTAC", 0, ((6, 5, 4),)),
    ("x-gap", ((0, 0), (1, 1), (2, 2), (5, 3), (6, 4), (7, 5), (8, 6), (9, 7)), "ACGTTACGTA", "ACGACGTA", 0,
     ((0, 0, 3), (5, 3, 5))),
    ("y-gap", ((0, 0), (1, 1), (2, 2), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9)), "ACGACGTA", "ACGTTACGTA", 0,
     ((0, 0, 3), (3, 5, 5))),
    ("both-gaps", ((0, 0), (1, 1), (2, 2), (5, 4), (6, 5), (7, 6), (8, 7), (9, 8)), "ACGTTACGTA", "ACGTACGTA", 0,
     ((0, 0, 3), (5, 4, 5))),
    ("both-gaps-trim-1", ((0, 0), (1, 1), (2, 2), (5, 4), (6, 5), (7, 6), (8, 7), (9, 8)), "ACGTTACGTA", "ACGTACGTA", 1,
     ((1, 1, 1), (6, 5, 3))),
    # a step of one in x and two in y is a y-gap, not a block
    ("step-one-and-two", ((0, 0), (1, 2), (2, 3)), "ACG", "AACG", 0, ((0, 0, 1), (1, 2, 2))),
)


def random_chain(rng):
    """(pairs, sX, sY, trim): a chain of a few blocks over sequences of up to 200 letters, Y a noisy copy of X along it."""
    letters = "ACGTacgtNn"
    pairs, x, y = [], 0, 0
    for _ in range(rng.randrange(0, 7)):
        x += rng.choice((0, 0, 1, 2, 5))
        y += rng.choice((0, 0, 1, 3))
        if pairs and pairs[-1] == (x - 1, y - 1):
            x += 1  # a new block: it must not continue the one before
        for _ in range(rng.randrange(1, 30)):
            pairs.append((x, y))
            x, y = x + 1, y + 1
    lX, lY = x + rng.randrange(0, 4), y + rng.randrange(0, 4)
    sx = [rng.choice(letters) for _ in range(lX)]
    sy = [rng.choice(letters) for _ in range(lY)]
    for px, py in pairs:
        if rng.random() < 0.8:
            sy[py] = sx[px] if rng.random() < 0.7 else sx[px].swapcase()
    return tuple(pairs), "".join(sx), "".join(sy), rng.randrange(0, 5)


@functools.lru_cache(maxsize=None)
def random_chains(n=500, seed=20260101):
    rng = random.Random(seed)
    return tuple(random_chain(rng) for _ in range(n))


# ---- realign-style inputs ----
Case = collections.namedtuple("Case", "name seqs cigars opts")  # opts: diagonalExpansion, constraintDiagonalTrim


def bases(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def reverse_complement(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def noisy(x, rate, seed):
    rng = random.Random(seed)
    return "".join(c if rng.random() > rate else rng.choice("ACGT") for c in x)


def _gapless(name, x, y, E=4, trim=0):
    n = min(len(x), len(y))
    ops = [(M, n)] + ([(DX, len(x) - n)] if len(x) > n else []) + ([(IY, len(y) - n)] if len(y) > n else [])
    return Case(name, {"X": x, "Y": y}, (("X", 0, len(x), True, "Y", 0, len(y), True, 1.0, tuple(ops)),), dict(diagonalExpansion=E, constraintDiagonalTrim=trim))


def identical_case(n):
    """X against itself: every column ends up in list 3, so the list and the columns of X hold n entries -- one short of a
    chunk of 64 lanes, exactly one, one more, four and one."""
    x = bases(n, 100 + n)
    return _gapless("identical-%d" % n, x, x)


def straddle_case():
    """130 bases with base 66 missing in Y and trim 3: the first block ends at column 65, so its trimmed columns 63 .. 65
    lie on both sides of the chunk edge at 64, and the second block's trimmed start lies behind it."""
    x = bases(130, 7)
    y = x[:66] + x[67:]
    ops = ((M, 66), (DX, 1), (M, 63))
    return Case("straddle", {"X": x, "Y": y}, (("X", 0, 130, True, "Y", 0, 129, True, 1.0, ops),), dict(diagonalExpansion=4, constraintDiagonalTrim=3))


def empty_case():
    """Nothing aligns: no anchors, no pair reaches matchGamma, list 3 is empty."""
    return _gapless("empty", "A" * 40, "C" * 40)


def many_case():
    """300 cigars of 30 .. 70 bases in one batch, number 137 of them the empty one."""
    seqs, cigars = {}, []
    rng = random.Random(300)
    for k in range(300):
        n = rng.randrange(30, 71)
        x = bases(n, 1000 + k)
        y = noisy(x, 0.06, 5000 + k)
        if k == 137:
            x, y = "A" * n, "C" * n
        seqs["X%d" % k], seqs["Y%d" % k] = x, y
        cigars.append(("X%d" % k, 0, n, True, "Y%d" % k, 0, n, True, 1.0, ((M, n),)))
    return Case("many-300", seqs, tuple(cigars), dict(diagonalExpansion=4, constraintDiagonalTrim=0))


def minus_case():
    """The second sequence on its minus strand: the cigar reads "Y 190 5 -" and the aligner sees rc(Y[5:190])."""
    x = bases(190, 41)
    piece = noisy(x[:90] + x[95:], 0.05, 42)  # 185 bases, five of X deleted
    y = "GATTA" + reverse_complement(piece) + "CATCAT"
    ops = ((M, 90), (DX, 5), (M, 95))
    return Case("minus", {"X": x, "Y": y}, (("X", 0, 190, True, "Y", 5 + 185, 5, False, 1.0, ops),), dict(diagonalExpansion=4, constraintDiagonalTrim=1))


def long_case():
    """One 1200 bp pair at expansion 4: 2400 diagonals, several traceback segments, and list 3 arrives in their order."""
    x = bases(1200, 51)
    y = noisy(x[:500] + x[503:900] + "AC" + x[900:], 0.04, 52)
    ops = ((M, 500), (DX, 3), (M, 397), (IY, 2), (M, 300))
    return Case("long-1200", {"X": x, "Y": y}, (("X", 0, 1200, True, "Y", 0, 1199, True, 1.0, ops),), dict(diagonalExpansion=4, constraintDiagonalTrim=0))


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = tuple(identical_case(n) for n in (63, 64, 65, 257)) + (straddle_case(), empty_case(), many_case(), minus_case(), long_case())
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in all_cases() if c.name == name)


def sub_sequences(seqs, cigar):
    """getSubSequence (cPecanRealign.c:245-253) of both sides of a cigar."""
    c1, s1, e1, f1, c2, s2, e2, f2 = cigar[:8]
    sx = seqs[c1][s1:e1] if f1 else reverse_complement(seqs[c1][e1:s1])
    sy = seqs[c2][s2:e2] if f2 else reverse_complement(seqs[c2][e2:s2])
    return sx, sy


def cigar_anchors(sx, sy, ops, trim, expansion):
    """cPecanRealign.c:525-529: every match column but `trim` at either end of its operation, exact matches only."""
    anchors, x, y = [], 0, 0
    for t, n in ops:
        if t == M:
            for k in range(trim, n - trim):
                a, b = sx[x + k].upper(), sy[y + k].upper()
                if a == b and a != "N":
                    anchors.append((x + k, y + k, expansion))
        x += n if t != IY else 0
        y += n if t != DX else 0
    return anchors


def problems(c):
    """[(sX, sY, anchors)] of a case, both ends ragged (cPecanRealign.c:537)."""
    out = []
    for cigar in c.cigars:
        sx, sy = sub_sequences(c.seqs, cigar)
        out.append((sx, sy, cigar_anchors(sx, sy, cigar[9], c.opts["constraintDiagonalTrim"], c.opts["diagonalExpansion"])))
    return out


REALIGN_SPLIT = 10  # cPecanRealign's default splitMatrixBiggerThanThis (cells)


def oracle_realign(om, sx, sy, anchors, pkw, check=None):
    """cPecanRealign.c:537-553 on the CPU oracle: the ordered alignment (list 3), sorted, as (x, y) pairs.  check: a list that
    receives the margins of this problem -- the smallest distance of a posterior to the threshold and of a reweighted weight
    to matchGamma."""
    p = ob.params(**pkw)
    pairs = ob.aligned_pairs(om, sx, sy, anchors, p, True, True)
    rw = ob.reweight_aligned_pairs(pairs, len(sx), len(sy), GAP_GAMMA)
    if check is not None:
        low = dict(pkw)
        low["threshold"] = p.threshold - 2 * MARGIN  # the pairs just under the threshold too
        near = ob.aligned_pairs(om, sx, sy, anchors, ob.params(**low), True, True)
        d_thr = min([abs(s / PROB_1 - p.threshold) for s in near[:, 0]], default=1.0)
        d_gamma = min([abs(w / PROB_1 - MATCH_GAMMA) for w in rw[:, 0]], default=1.0)
        check.append((d_thr, d_gamma))
    ordered = ob.filter_pairs_ordered(rw, len(sx), len(sy), MATCH_GAMMA)
    return sorted((int(x), int(y)) for _, x, y in ordered)


def case_pkw(c):
    return dict(diagonalExpansion=c.opts["diagonalExpansion"], splitMatrixBiggerThanThis=REALIGN_SPLIT)


@functools.lru_cache(maxsize=None)
def oracle_lists(name):
    """Per problem of the case: (sorted list 3 of the oracle, margins).  Computed once per process and shared."""
    c = case(name)
    om, out = ob.model(0), []
    for sx, sy, anchors in problems(c):
        margins = []
        out.append((tuple(oracle_realign(om, sx, sy, anchors, case_pkw(c), margins)), margins[0]))
    return tuple(out)


# ---- the trainer: 8 cigars of 150 .. 300 bases, three with a misplaced deletion (as tests/band_edge_cases.py) ----
EM_E, EM_SPLIT, EM_ITERATIONS, EM_JC = 4, 100, 3, 0.2
# The posterior threshold of the trainer tests' realign options.  At the default 0.01 no world meets the margin: away from an
# indel the posteriors of the shifted alignments fall off geometrically, and in 16 realignments one of them always lands
# within 1e-4 -- 1 % -- of 0.01 (3400 seeds tried on the oracle, none passed; 7 of 16 realignments miss it in this world).
# Around 0.2 the posteriors are sparse and 1e-4 is 0.05 %.
EM_THRESHOLD = 0.2
EM_SEEDS = ((0, 150, True), (1, 180, False), (2, 210, True), (3, 240, False), (4, 270, True), (5, 300, False), (6, 165, False),
            (7, 225, False))  # (seed, length of X, misplaced deletion)


def em_world():
    """(seqs, cigars): X of the given length, Y a noisy copy without 10 bases in the middle; the cigar has the deletion where
    it is, or -- misplaced -- is gapless with the deletion pushed to the end."""
    seqs, cigars = {}, []
    for seed, n, misplaced in EM_SEEDS:
        x = bases(n, 500 + seed)
        at = n // 2
        y = noisy(x[:at] + x[at + 10:], 0.08, 600 + seed)
        ops = ((M, n - 10), (DX, 10)) if misplaced else ((M, at), (DX, 10), (M, n - 10 - at))
        seqs["x%d" % seed], seqs["y%d" % seed] = "GATTACA" + x + "TTG", y + "CA"
        cigars.append(("x%d" % seed, 7, 7 + n, True, "y%d" % seed, 0, n - 10, True, 1.0, ops))
    return seqs, tuple(cigars)


def em_pkw():
    return dict(diagonalExpansion=EM_E, splitMatrixBiggerThanThis=EM_SPLIT * EM_SPLIT, threshold=EM_THRESHOLD)


def m_step(acc, S):
    """calculateMaximisation with trainEmissions and no tying: rows normalised."""
    t = np.array(acc.T[:S * S]).reshape(S, S)
    t /= t.sum(axis=1, keepdims=True)
    e = np.array(acc.E[:S * 16]).reshape(S, 16)
    e /= e.sum(axis=1, keepdims=True)
    return t, e


@functools.lru_cache(maxsize=None)
def oracle_em_update_band(iterations=EM_ITERATIONS):
    """The updateTheBand loop on the CPU oracle: five-state model, equal transitions, Jukes-Cantor emissions, one job.
    Returns (margins of every realignment, blocks of the last anchors per cigar, running likelihoods)."""
    import next_runs_model as nm
    seqs, cigars = em_world()
    S, h = 5, ob.hmm(0)
    e = np.exp(-4.0 * EM_JC / 3.0)
    for i in range(S * S):
        h.T[i] = 1.0 / S
    for s in range(S):
        for i in range(16):
            h.E[s * 16 + i] = (0.25 + 0.75 * e) / 4 if i % 4 == i // 4 else (0.25 - 0.25 * e) / 4
    subs = [sub_sequences(seqs, c) for c in cigars]
    anchors = [cigar_anchors(sx, sy, c[9], 0, EM_E) for (sx, sy), c in zip(subs, cigars)]
    p, margins, running = ob.params(**em_pkw()), [], []
    for it in range(iterations):
        m = ob.model_from_hmm(h)
        acc = ob.hmm(0, 0.000000000001)
        for (sx, sy), a in zip(subs, anchors):
            ob.expectations(m, acc, sx, sy, a, p, True, True)
        t, em_ = m_step(acc, S)
        for i in range(S * S):
            h.T[i] = t.flat[i]
        for i in range(S * 16):
            h.E[i] = em_.flat[i]
        h.likelihood = acc.likelihood
        running.append(acc.likelihood)
        if it + 1 < iterations:
            m = ob.model_from_hmm(h)
            new = []
            for (sx, sy), a in zip(subs, anchors):
                chain = oracle_realign(m, sx, sy, a, em_pkw(), margins)
                new.append(runs_to_anchors(nm.next_runs(chain, sx, sy, 0, EM_E)))
            anchors = new
    return tuple(margins), tuple(tuple(a) for a in anchors), tuple(running)


def runs_to_anchors(runs):
    return [(int(x) + k, int(y) + k, int(e)) for x, y, n, e in runs for k in range(int(n))]
