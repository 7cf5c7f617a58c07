"""Constructed inputs of the band-edge tests, shared by the CPU suite (tests/test_band_edge_cpu.py: the host function
against tests/band_edge_model.py on the oracle's lists, and every case really has the edge it was built for) and the GPU
suites (tests/test_gpu_band_edge.py, tests/test_gpu_realign_adaptive.py).  Nothing here touches a device.

A problem is (sX, sY, anchors, raggedLeft, raggedRight) with anchors (x, y, expansion).  A Case is one batch: model type,
parameters, problems, emitter, the planning knobs that put it on the kernel it is built for, `minus` (the problems go in
through cpecan_batch_add_many_runs_stranded with Y on the minus strand: sY here is already the reverse complement the batch
aligns, and the anchors are in its coordinates) and `expect`, per problem: "flag" (the oracle's lists must give
edgeScoreSum >= 2 S), "clear" (<= S / 2) or None (no claim)."""
import collections
import functools
import random

import oracle_binding as ob

Case = collections.namedtuple("Case", "name mtype pkw problems emit env minus expect")

S = 1000000            # minEdgeScore of the tests: a pair at the 0.01 threshold is worth 100 000 units
EMIT_MATCH, EMIT_INDEL = 0, 1
KNOBS = ("CPECAN_SPLIT", "CPECAN_PACKED", "CPECAN_PACKED_SPLIT", "CPECAN_TEAM", "CPECAN_ABS", "CPECAN_DENSE", "CPECAN_TABLE_WAVE",
         "CPECAN_KEEP_RUNS", "CPECAN_POST_LANES")
SEEDS = (0, 1, 2, 3, 4, 5)


def bases(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def reverse_complement(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def deletion_pair(n, at, length, seed):
    """X: n random bases; Y: X without X[at:at + length]."""
    x = bases(n, seed)
    return x, x[:at] + x[at + length:]


def wrong_anchors(x, y, E):
    """A gapless cigar, filtered to the columns whose letters agree: what cPecanRealign keeps of it."""
    return tuple((i, i, E) for i in range(min(len(x), len(y))) if x[i] == y[i])


def right_anchors(y, at, length, E):
    return tuple((i if i < at else i + length, i, E) for i in range(len(y)))


def _problem(x, y, anchors):
    return (x, y, tuple(anchors), True, True)


def deletion_case(E):
    """The 150-base pairs of the issue's table, seeds 0..5: wrong anchors, then right ones.  Packed classes."""
    probs, expect = [], []
    for seed in SEEDS:
        x, y = deletion_pair(150, 75, 10, seed)
        probs += [_problem(x, y, wrong_anchors(x, y, E)), _problem(x, y, right_anchors(y, 75, 10, E))]
        expect += [None if (E, seed) == (8, 5) else "flag", "clear"]  # seed 5 at E = 8: wrong, and not flagged
    return Case("del150-E%d" % E, 0, dict(diagonalExpansion=E), tuple(probs), EMIT_MATCH, {"CPECAN_PACKED": "2"}, False, tuple(expect))


def _long_problems(E=20):
    x, y = deletion_pair(400, 200, 30, 7)
    return (_problem(x, y, wrong_anchors(x, y, E)), _problem(x, y, right_anchors(y, 200, 30, E)))


def sweep_case():
    """400 bases with a 30-base deletion at E = 20, one wave per region."""
    return Case("del400-sweep", 0, dict(diagonalExpansion=20), _long_problems(), EMIT_MATCH, {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "0"},
                False, ("flag", "clear"))


def chunks_case():
    """The same with a traceback every 44 diagonals: several chunks per region, gathered in descending segment order."""
    pkw = dict(diagonalExpansion=20, minDiagsBetweenTraceBack=50, traceBackDiagonals=5)
    return Case("del400-chunks", 0, pkw, _long_problems(), EMIT_MATCH, {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "0"}, False, ("flag", "clear"))


TWO_REGIONS_SPLIT = 900


def two_regions_case():
    """One problem cut in two by a 40 x 40 gap without anchors: right anchors in front of it, a misplaced 10-base deletion
    behind it.  Edge pairs lie in the second region only, so every one of them has its dx, dy undone."""
    E = 4
    x = bases(300, 11)
    y = x[:220] + x[230:]
    anchors = [(i, i, E) for i in range(100)] + [(i, i, E) for i in range(140, len(y)) if x[i] == y[i]]
    pkw = dict(diagonalExpansion=E, splitMatrixBiggerThanThis=TWO_REGIONS_SPLIT)
    return Case("two-regions", 0, pkw, (_problem(x, y, anchors),), EMIT_MATCH, {}, False, ("flag",))


def unanchored_case():
    """450 x 450 without anchors: the band is the matrix, only the matrix cuts it, and the statistic is 0.  Team kernel."""
    x = bases(450, 21)
    rng = random.Random(22)
    y = "".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in x)
    return Case("unanchored-team", 0, dict(diagonalExpansion=20), ((x, y, (), True, True),), EMIT_MATCH, {"CPECAN_TEAM": "400"}, False, ("clear",))


def dynamic_case():
    """Per-anchor expansions: the wrong anchors of seed 0 carry 2 in front of column 60 and 6 behind it, the right ones 4."""
    x, y = deletion_pair(150, 75, 10, 0)
    wrong = tuple((i, j, 2 if i < 60 else 6) for i, j, _ in wrong_anchors(x, y, 0))
    pkw = dict(diagonalExpansion=30, dynamicAnchorExpansion=1)
    return Case("dynamic", 0, pkw, (_problem(x, y, wrong), _problem(x, y, right_anchors(y, 75, 10, 4))), EMIT_MATCH, {}, False,
                ("flag", "clear"))


def minus_case():
    """The pairs of seeds 1 and 2 at E = 4 as minus-strand problems: the caller holds the reverse complement of Y."""
    probs = deletion_case(4).problems[2:6]
    return Case("minus", 0, dict(diagonalExpansion=4), probs, EMIT_MATCH, {}, True, ("flag", "clear", "flag", "clear"))


def indel_case():
    """An INDEL batch: three lists per problem, and only list 0 counts."""
    probs = deletion_case(4).problems[6:10]
    return Case("indel", 0, dict(diagonalExpansion=4), probs, EMIT_INDEL, {}, False, ("flag", "clear", "flag", "clear"))


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = (deletion_case(4), deletion_case(8), sweep_case(), chunks_case(), two_regions_case(), unanchored_case(), dynamic_case(),
             minus_case(), indel_case())
    assert len({c.name for c in cases}) == len(cases)
    return cases


def case(name):
    return next(c for c in all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def oracle_lists(name):
    """List 0 of every problem of the case from the oracle: computed once per process and shared (read-only)."""
    c = case(name)
    om, op = ob.model(c.mtype), ob.params(**c.pkw)
    out = []
    for sx, sy, a, rl, rr in c.problems:
        if c.emit == EMIT_INDEL:
            out.append(ob.aligned_pairs_with_indels(om, sx, sy, a, op, rl, rr)[0])
        else:
            out.append(ob.aligned_pairs(om, sx, sy, a, op, rl, rr))
    for t in out:
        t.setflags(write=False)
    return tuple(out)


# ---- the adaptive band of the realign flow: eight cigars of about 150 bases at E = 4 ----
ADAPTIVE_E, ADAPTIVE_ROUNDS = 4, 3
ADAPTIVE_CIGARS = ((0, True), (1, True), (2, False), (4, True), (5, False), (6, True), (7, False), (8, True))  # (seed, misplaced deletion)
REALIGN_SPLIT = 10  # cPecanRealign's splitMatrixBiggerThanThis: a cigar is cut wherever its anchors leave more than 10 cells


def adaptive_inputs():
    """[(name of X, X, name of Y, Y, cigar operations, misplaced)]: the cigar is "M 140 D 10" (gapless, the deletion pushed to
    the end) where the deletion is misplaced and "M 75 D 10 M 65" where it is right.  Operations are (op, length) with
    0 = match, 1 = X only."""
    out = []
    for seed, misplaced in ADAPTIVE_CIGARS:
        x, y = deletion_pair(150, 75, 10, seed)
        ops = ((0, 140), (1, 10)) if misplaced else ((0, 75), (1, 10), (0, 65))
        out.append(("x%d" % seed, x, "y%d" % seed, y, ops, misplaced))
    return out


def adaptive_problem(x, y, misplaced, E):
    """The problem the realign flow makes of such a cigar at expansion E: exact-match anchors, both ends ragged."""
    return _problem(x, y, wrong_anchors(x, y, E) if misplaced else right_anchors(y, 75, 10, E))


def adaptive_pkw(E):
    return dict(diagonalExpansion=E, splitMatrixBiggerThanThis=REALIGN_SPLIT)


@functools.lru_cache(maxsize=None)
def adaptive_statistics():
    """Per cigar, the model's statistic of the oracle's list at E * 2^k, k = 0 .. ADAPTIVE_ROUNDS: computed once and shared."""
    import band_edge_model as bm
    om, out = ob.model(0), []
    for _, x, _, y, _, misplaced in adaptive_inputs():
        row = []
        for k in range(ADAPTIVE_ROUNDS + 1):
            E = ADAPTIVE_E << k
            pr, pkw = adaptive_problem(x, y, misplaced, E), adaptive_pkw(E)
            row.append(bm.band_edge(pr, pkw, ob.aligned_pairs(om, x, y, pr[2], ob.params(**pkw), True, True)))
        out.append(tuple(row))
    return tuple(out)


def adaptive_predictions():
    """The round every cigar ends on with maxRounds = ADAPTIVE_ROUNDS and minEdgeScore = S."""
    import band_edge_model as bm
    return [bm.predicted_round(lambda k, row=row: row[k], ADAPTIVE_ROUNDS, S) for row in adaptive_statistics()]


# ---- cpecan_align --adaptiveBand: anchors from the anchor finder, so a flag needs an alignment that leaves an HSP ----
ALIGN_E = 2


def align_inputs():
    """(target, [queries]): 700 bases; the first query carries two inserted bases and, eight columns on, two deleted ones.
    The ungapped HSP runs through the eight shifted columns, the anchors follow it, and at expansion 2 the alignment's detour
    two diagonals off is the band's last cell; at expansion 4 it is inside.  The second query is the target with a few
    substitutions: no detour, no flag."""
    x = bases(700, 31)
    detour = x[:300] + "GT" + x[300:308] + x[310:]
    rng = random.Random(32)
    plain = "".join(c if rng.random() > 0.03 else rng.choice("ACGT") for c in x)
    return x, [detour, plain]


@functools.lru_cache(maxsize=None)
def align_statistics():
    """Per query, the model's statistic at ALIGN_E and at twice that, on the anchors of tests/anchor_model.py."""
    import anchor_model as am
    import band_edge_model as bm
    x, queries = align_inputs()
    om, out = ob.model(0), []
    for y in queries:
        row = []
        for E in (ALIGN_E, 2 * ALIGN_E):
            runs, _ = am.find_anchor_runs(x, y, expansion=E)
            anchors = tuple(am.runs_to_anchors(runs))
            pkw = dict(diagonalExpansion=E)
            row.append(bm.band_edge((x, y, anchors, True, True), pkw, ob.aligned_pairs(om, x, y, anchors, ob.params(**pkw), True, True)))
        out.append(tuple(row))
    return tuple(out)
