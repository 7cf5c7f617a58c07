"""Seeded models and problems of the expectation-emitter tests (CPECAN_EMIT_EXPECT: the Baum-Welch counts of
diagonalCalculationExpectations, pairwiseAligner.c:735-746), shared by the CPU suite (tests/test_expect_cases_cpu.py: the
preconditions, with the oracle alone) and the GPU suite (tests/test_gpu_expect.py: every build of the emitter against
the oracle, problem by problem).  Nothing here touches a device.

A problem is (sX, sY, anchors, raggedLeft, raggedRight); a Case is a batch of problems under one model and one set of
parameters (tests/indel_cases.py).  Case names are unique: the oracle's counts of a case are computed once per process and
shared.  Only finite models: every transition a model has carries a probability above zero."""
import collections
import functools
import random

import numpy as np

import indel_cases as ic
import oracle_binding as ob
from cpecan_amd import api
from cpecan_amd.workload import make_pair
from indel_cases import ASYMMETRIC, MODELS, Case, states
from test_gpu_forward import DEGENERATE, RAGGED, _random_model_pair, _same_length_pair
from test_gpu_parity import _evolve, _rand_seq

Counts = collections.namedtuple("Counts", "T E likelihood")

# ---- tolerances: the project's, not new measurements ----
ORACLE_RTOL, ORACLE_ATOL, ORACLE_LIKELIHOOD_RTOL = 1e-5, 1e-12, 1e-9  # test_gpu_parity._assert_hmm_close, the team test's likelihood bound
FORM_RTOL, FORM_ATOL, FORM_LIKELIHOOD_RTOL = 1e-6, 1e-12, 1e-11       # tools/soak_emitters.py: fp32 sums added in another order

# ---- models: the five of indel_cases, and three random ones per state count for the slots ----
SLOT_TYPES = {5: api.fiveState, 3: api.threeStateAsymmetric}
SLOT_MODELS = {"slot%d-%d" % (S, k): (mtype, 11 + 7 * k) for S, mtype in SLOT_TYPES.items() for k in range(3)}


def slot_models(S):
    return tuple("slot%d-%d" % (S, k) for k in range(3))


def model_type(name):
    return SLOT_MODELS[name][0] if name in SLOT_MODELS else ic.TYPE_OF[name]


def model_pair(name):
    """(library model, the oracle's model from the same numbers): indel_cases.model_pair, and for the slots
    test_gpu_forward._random_model_pair -- what test_gpu_model_slots._random_model makes, with the oracle's copy."""
    return _random_model_pair(*SLOT_MODELS[name]) if name in SLOT_MODELS else ic.model_pair(name)


def n_states(name):
    return 5 if model_type(name) in (api.fiveState, api.fiveStateAsymmetric) else 3


def present_transitions(name):
    """The indices from * S + to of the transitions the model has."""
    om, S = model_pair(name)[1], n_states(name)
    return tuple(sorted({om.tr[k].frm * S + om.tr[k].to for k in range(om.nTransitions)}))


def absent_transitions(name):
    """The indices of T the oracle leaves at exactly 0 on every problem: state pairs without a transition (a five-state
    model has none between the short and the long gaps, nor between the two long gaps)."""
    S = n_states(name)
    return tuple(i for i in range(S * S) if i not in present_transitions(name))


# ---- the oracle's counts, per problem ----
_oracle_cache = {}


def _counts_of(model, problem, pkw):
    sx, sy, a, rl, rr = problem
    acc = ob.hmm(model_type(model), 0.0)
    ob.expectations(model_pair(model)[1], acc, sx, sy, a, ob.params(**pkw), rl, rr)
    S = n_states(model)
    T, E = np.array(acc.T[:S * S]), np.array(acc.E[:S * 16])
    T.setflags(write=False)
    E.setflags(write=False)
    return Counts(T, E, float(acc.likelihood))


def oracle_counts(case):
    """[Counts(T[S * S], E[S * 16], likelihood)] of every problem of the case: ob.expectations into a fresh ob.hmm(type, 0.0);
    computed once, never modified."""
    if case.name not in _oracle_cache:
        _oracle_cache[case.name] = (case, tuple(_counts_of(case.model, pr, case.pkw) for pr in case.problems))
    kept, out = _oracle_cache[case.name]
    assert kept is case or kept == case, "two cases share the name %s" % case.name
    return out


def pooled(counts):
    """The sum of a list of Counts."""
    counts = list(counts)
    return Counts(sum(c.T for c in counts), sum(c.E for c in counts), sum(c.likelihood for c in counts))


# ---- what a problem must bring for the gates to mean something (tests/test_expect_cases_cpu.py asserts each) ----
MIN_COUNT = 1e-3


def covers_every_transition(counts, model):
    """Every transition of the model has a count of at least MIN_COUNT: the relative gate then tests each element."""
    return all(counts.T[i] >= MIN_COUNT for i in present_transitions(model))


def transposed_pairs_differ(counts, model):
    """T[a * S + b] and T[b * S + a] differ by more than 1 % (of the larger) for some pair of states, and so do the sums
    over the four X rows of the gapX and the gapY emission blocks, row by row: from and to swapped in the transition index,
    or the emissions of the two gap states swapped, then move a count far outside the gate."""
    S = n_states(model)
    T = counts.T.reshape(S, S)
    pairs = [(T[a, b], T[b, a]) for a in range(S) for b in range(a + 1, S) if max(T[a, b], T[b, a]) >= MIN_COUNT]
    rows_x, rows_y = counts.E[16:32].reshape(4, 4).sum(axis=1), counts.E[32:48].reshape(4, 4).sum(axis=1)
    return (any(abs(u - v) > 0.01 * max(u, v) for u, v in pairs) and
            any(abs(u - v) > 0.01 * max(u, v) for u, v in zip(rows_x, rows_y)))


def well_covered(counts, model):
    return covers_every_transition(counts, model) and (model not in ASYMMETRIC or transposed_pairs_differ(counts, model))


def n_share(counts):
    """(sum(T) - sum(E)) / sum(T): the share of the events at cells with an N on either side -- a cell of row or column 0
    counts as one (pairwiseAligner.c:597-607) --, which are in the transition counts and not in the emission counts."""
    return (counts.T.sum() - counts.E.sum()) / counts.T.sum()


def _drawn(model, draw, ragged, holds, **pkw):
    """draw(0), draw(1), ... until the oracle's counts of the problem meet holds(counts, model)."""
    for k in range(100):
        sx, sy, a = draw(k)
        pr = (sx, sy, tuple(map(tuple, a))) + tuple(ragged)
        if holds is None or holds(_counts_of(model, pr, pkw), model):
            return pr
    raise AssertionError("no problem meets the precondition under %s, %r" % (model, pkw))


# ---- the LDS a wave of an expectation class takes (cpk_plan.inl) ----
LDS_PATH_MAX_BYTES = 64 * 1024
IN_SWEEP_MAX_BYTES = 160 * 1024 // 8


def expect_wave_lds_bytes(S, lX, lY):
    """set_row_form for an expectation class of one unanchored lX x lY pair with one wave per region: the header of 552
    doubles (logAdd cubics, emission + transition weights, four copies of the 80 emission sums; no candidate stage),
    2 S + 1 rolling rows of maxWidth + 1 doubles, and both strings at two symbols a byte."""
    width = min(lX, lY) + 1
    return 8 * (552 + (2 * S + 1) * (width + 1)) + ((lX + 3) // 2 + (lY + 3) // 2 + 15) // 16 * 16


def in_sweep_lds_bytes(S, lX, lY):
    """plan_expect_in_sweep: with the events formed inside the traceback the wave keeps three forward diagonals of S
    rows and two copies of a window's emission sums as well, and one copy of the kernel's sums instead of four."""
    return expect_wave_lds_bytes(S, lX, lY) + 8 * (3 * (min(lX, lY) + 2) * S + 2 * 80 - 3 * 80)


def in_global_memory(S, n):
    """plan_wide_class: the rolling rows of the class go to global memory when one wave's LDS plus 16 bytes is over 64 KB."""
    return expect_wave_lds_bytes(S, n, n) + 16 > LDS_PATH_MAX_BYTES


# What the CPECAN_TRACE_HOST class lines gave: the first unanchored n x n pair (n + 1 cells on the widest diagonal) whose
# rows no longer fit.  An expectation class stages no candidates but keeps 320 doubles of sums: between the indel
# emitter's 645 / 1007 bases and the forward emitter's 714 / 1115.
FIRST_GLOBAL_LENGTH = {5: 685, 3: 1071}
# ... and the widest diagonal at which the library's own choice still forms the events inside the traceback, for X against
# a Y of at least LDS_EDGE_LY bases: 74 cells of five states, 121 of three; one cell more takes the second pass.
LDS_EDGE_LY = 1900
LAST_IN_TRACEBACK_WIDTH = {5: 74, 3: 121}


# ---- a pair with one long gap on each side ----
OVERHANG_X, OVERHANG_Y = 8, 6


def _planted(rng, seg, gap_x, gap_y, seq=_rand_seq):
    """X = a + gx + b + c + tx and Y = hy + a' + b' + gy + c': three related stretches of `seg` bases, gap_x bases only X has
    and gap_y only Y has, OVERHANG_Y bases of Y in front and OVERHANG_X of X behind.  The long-gap states of the five-state
    models, which related sequences without such gaps leave at counts of 1e-4 and less, get counts of the order of the
    gap lengths.  The overhangs are there for the transposed counts: every gap an alignment opens inside the matrix it
    closes as well, so T[match, gap] and T[gap, match] differ only by the alignments that begin or end in a gap state."""
    a, b, c = (seq(rng, seg) for _ in range(3))
    near = lambda s: "".join(ch if rng.random() < 0.9 else seq(rng, 1) for ch in s)
    return a + seq(rng, gap_x) + b + c + seq(rng, OVERHANG_X), seq(rng, OVERHANG_Y) + near(a) + near(b) + seq(rng, gap_y) + near(c)


# ---- 1. widths ----
UNANCHORED_WIDTHS = (1, 5, 63, 64, 65, 127, 128, 129)
BANDED_EXPANSIONS = (10, 40)
PLANTED = {64: (12, 19, 28), 114: (25, 30, 39)}  # cells: (seg, gap_x, gap_y); X is the shorter, 3 seg + gap_x + OVERHANG_X + 1 cells
WidthsProblem = collections.namedtuple("WidthsProblem", "kind width")
WIDTHS_PKW = dict(diagonalExpansion=40, dynamicAnchorExpansion=1)


def widths_layout(model):
    """What problem i of widths_case(model) is: ("unanchored", cells), ("lds-edge", cells), ("banded", expansion) or
    ("planted", cells)."""
    last = LAST_IN_TRACEBACK_WIDTH[states(model)]
    return (tuple(WidthsProblem("unanchored", w) for w in UNANCHORED_WIDTHS) +
            (WidthsProblem("lds-edge", last), WidthsProblem("lds-edge", last + 1)) +
            tuple(WidthsProblem("banded", E) for E in BANDED_EXPANSIONS) +
            tuple(WidthsProblem("planted", w) for w in PLANTED))


def widths_indices(model, kind):
    return tuple(i for i, wp in enumerate(widths_layout(model)) if wp.kind == kind)


def _of_width(rng, w, ly=0):
    """An unanchored related pair whose widest diagonal has w cells: w - 1 bases of X against at least as many of Y (ly: at
    least that many).  One cell: no X at all."""
    if w == 1:
        return "", _rand_seq(rng, 7), ()
    sx, sy = _same_length_pair(rng, w - 1)
    return sx, sy + _rand_seq(rng, max(0, ly - len(sy))), ()


@functools.lru_cache(maxsize=None)
def widths_case(model):
    """Unanchored related pairs whose widest diagonal is just under, at and over one and two 64-lane groups -- where the
    library goes from the build for one group per diagonal to the build for two and on to the second pass --, a pair each
    side of the width at which its own choice gives up the in-traceback form for its LDS, two banded pairs of several
    traceback segments (dynamicAnchorExpansion: the anchors of make_pair carry their own expansion), and two pairs with planted gaps, one per
    in-traceback build, the second drawn until its counts are well_covered.  The ragged combinations go round the list."""
    rng = random.Random(5000 + MODELS.index(model))
    draws = []
    for kind, w in widths_layout(model):
        if kind == "unanchored":
            draws.append((lambda k, w=w: _of_width(rng, w), None))
        elif kind == "lds-edge":
            draws.append((lambda k, w=w: _of_width(rng, w, LDS_EDGE_LY), None))
        elif kind == "banded":
            draws.append((lambda k, E=w: tuple(make_pair(11, E + 2 * k, 600, E)), None))
        else:
            draws.append((lambda k, t=PLANTED[w]: _planted(rng, *t) + ((),), well_covered if w == max(PLANTED) else None))
    probs = tuple(_drawn(model, draw, RAGGED[(i + i // 4) % 4], holds, **WIDTHS_PKW) for i, (draw, holds) in enumerate(draws))
    return Case("expect-widths-%s" % model, model, probs, dict(WIDTHS_PKW))


# ---- 2. edges ----
EDGE_SIZES, EDGE_MODELS = ic.EDGE_SIZES, ic.EDGE_MODELS


@functools.lru_cache(maxsize=None)
def edges_case(model):
    """One pair of each of indel_cases.EDGE_SIZES (1 x 1 ... 130 x 40, unanchored) under all four ragged combinations --
    problems 4 k ... 4 k + 3 share their sequences --, then test_gpu_forward.DEGENERATE (empty X, empty Y, both, ...) under
    every ragged combination with an ordinary problem after every third; the first of these has planted gaps and is drawn
    until its counts are well_covered."""
    rng = random.Random(5100 + MODELS.index(model))
    probs = []
    for lX, lY in EDGE_SIZES:
        pair = ic._pair_of_lengths(rng, lX, lY)
        probs += [pair + ((),) + ragged for ragged in RAGGED]
    ordinary = [lambda k: _planted(rng, 30, 35, 45) + ((),)]
    ordinary += [lambda k, i=i: tuple(make_pair(12, i, 100, 10)) for i in range(1, 4)]
    ordinary += [lambda k: _same_length_pair(rng, 70) + ((),) for _ in range(4)]
    for k, ragged in enumerate(RAGGED):
        for j, (sx, sy) in enumerate(DEGENERATE):
            probs.append((sx, sy, ()) + ragged)
            if j % 3 == 2:
                i = 2 * k + j // 3
                probs.append(_drawn(model, ordinary[i], ragged, None if i else well_covered, diagonalExpansion=10))
    return Case("expect-edges-%s" % model, model, tuple(probs), dict(diagonalExpansion=10))


# ---- 3. N-rich ----
N_RICH_MIN_SHARE = 0.10


def _n_rich_seq(rng, n):
    """A tenth of the bases N, another tenth lower case (one of each at the least)."""
    s = [rng.choice("ACGT") for _ in range(n)]
    k = max(1, round(0.1 * n))
    marked = rng.sample(range(n), min(n, 2 * k))
    for j, i in enumerate(marked):
        s[i] = "N" if j < (len(marked) + 1) // 2 else s[i].lower()
    return "".join(s)


def _n_rich_pair(rng, n):
    sx = _n_rich_seq(rng, n)
    sy = "".join(ch if rng.random() < 0.85 else _n_rich_seq(rng, rng.randrange(0, 3)) for ch in sx)
    return sx, sy or "N"


def _n_rich_enough(counts, model):
    return n_share(counts) >= N_RICH_MIN_SHARE


@functools.lru_cache(maxsize=None)
def n_rich_case(model):
    """Pairs in which a fifth of the bases are N or lower case: one with planted gaps (well_covered), two banded, five
    unanchored of 10-129 bases (both in-traceback builds and the second pass); every one drawn until the events at N cells
    are N_RICH_MIN_SHARE of all."""
    rng = random.Random(5200 + MODELS.index(model))

    def banded(k):
        sx, sy = _n_rich_pair(rng, 300)
        return sx, sy, [(i, i, 24) for i in range(5, min(len(sx), len(sy)) - 5, 29)]

    draws = [lambda k: _planted(rng, 30, 35, 45, _n_rich_seq) + ((),), banded, banded]
    draws += [lambda k, n=n: _n_rich_pair(rng, n) + ((),) for n in (10, 40, 63, 90, 129)]
    first = lambda c, m: _n_rich_enough(c, m) and well_covered(c, m)
    probs = [_drawn(model, draw, RAGGED[i % 4], _n_rich_enough if i else first, diagonalExpansion=24) for i, draw in enumerate(draws)]
    return Case("expect-nrich-%s" % model, model, tuple(probs), dict(diagonalExpansion=24))


# ---- 4. packed ----
PACKED_EXPANSIONS = ic.PACKED_EXPANSIONS  # (expansion, lanes of a group, splitMatrixBiggerThanThis)


@functools.lru_cache(maxsize=None)
def _packed_batch(model, E, split):
    """The batch of indel_cases._packed_batch with seeds of its own.  In the widest of the three bands the first problem has
    planted gaps of 9 and 10 bases between runs of anchors on one diagonal each -- they widen that band of 27 cells to 32 -- and is drawn until its counts are
    well_covered; the narrower bands have no room for such gaps (their problems cover every transition all the same)."""
    rng = random.Random(5300 + 10 * MODELS.index(model) + E)
    pkw = dict(diagonalExpansion=E, minDiagsBetweenTraceBack=rng.randrange(40, 200), traceBackDiagonals=rng.randrange(3, 30),
               splitMatrixBiggerThanThis=split)

    def dense(sx, sy):
        anchors, x, y = [], -1, -1
        while True:
            x += rng.randrange(1, 5)
            y += rng.randrange(1, 5)
            if x >= len(sx) or y >= len(sy):
                return sx, sy, anchors
            anchors.append((x, y, E))

    def draw(k):
        sx = _rand_seq(rng, rng.randrange(1, 400))
        return dense(sx, _evolve(rng, sx) or "C")

    def planted(k):
        sx, sy = _planted(rng, 60, 9, 10)
        anchors = [(i, OVERHANG_Y + i, E) for i in range(2, 58)] + [(69 + i, OVERHANG_Y + 60 + i, E) for i in range(2, 58)]
        return sx, sy, anchors + [(129 + i, OVERHANG_Y + 130 + i, E) for i in range(2, 58)]

    ragged = lambda: (rng.random() > 0.5, rng.random() > 0.5)
    probs = [_drawn(model, planted, ragged(), well_covered, **pkw)] if E == 26 else []
    probs += [_drawn(model, draw, ragged(), None, **pkw) for _ in range(16 - len(probs))]
    probs += [("A", "A", (), False, False), ("ACGTAC", "", (), False, True), ("", "GGT", (), True, True)]
    return tuple(probs), pkw


@functools.lru_cache(maxsize=None)
def packed_cases(model):
    """(lanes of a group, case): dense random anchors, one batch per group width of the packed kernel (expansions 2, 6 and
    26), short traceback schedules, split rectangles in two of the three, ("A", "A") and the one-sided problems at the
    end: 16 + 3 problems each."""
    out = []
    for E, lanes, split in PACKED_EXPANSIONS:
        probs, pkw = _packed_batch(model, E, split)
        out.append((lanes, Case("expect-packed-%s-E%d" % (model, E), model, probs, pkw)))
    return tuple(out)


# ---- 5. team ----
@functools.lru_cache(maxsize=None)
def team_cases(model):
    """(words the trace line of the class must carry, CPECAN_TEAM, case): the three shapes of indel_cases.team_cases -- 500 x
    500 unanchored (four waves), 900 x 900 unanchored (eight; five states only), the 1500-base band of ~157 cells under
    CPECAN_TEAM=100 --, the class with a short traceback schedule that test_expectation_emitter_on_the_team_kernel forces
    onto the team with CPECAN_TEAM=100 (the team's second pass needs B of the emitted cells), and a pair of
    500 and 510 bases with planted gaps (four waves), drawn until its counts are well_covered."""
    out = [(words, team, Case("expect-" + c.name, model, c.problems, {k: v for k, v in c.pkw.items() if k != "threshold"}))
           for words, team, c in ic.team_cases(model, 0.01)]
    narrow = []
    for i in range(2):
        sx, sy, a = make_pair(8, i, 700, 60, anchor_every=150)
        narrow.append((sx, sy, tuple(map(tuple, a)), True, False))
    out.append(("a team of waves", "100", Case("expect-team-narrow-%s" % model, model, tuple(narrow),
                                               dict(diagonalExpansion=60, traceBackDiagonals=12, minDiagsBetweenTraceBack=300))))
    rng = random.Random(5400 + MODELS.index(model))
    gaps = _drawn(model, lambda k: _planted(rng, 150, 50, 60) + ((),), (False, True), well_covered, diagonalExpansion=40)
    out.append(("(four)", None if states(model) == 5 else "500", Case("expect-team4-planted-%s" % model, model, (gaps,),
                                                                        dict(diagonalExpansion=40))))
    return tuple(out)


# ---- 6. rows in global memory ----
GLOBAL_MODELS = ("fiveStateAsymmetric", "threeStateAsymmetric")


@functools.lru_cache(maxsize=None)
def global_cases(model):
    """(length, in global memory, case) for the last length that keeps its rows in LDS under CPECAN_TEAM=0 and the first
    that does not."""
    first = FIRST_GLOBAL_LENGTH[states(model)]
    out = []
    for n in (first - 1, first):
        sx, sy, _ = make_pair(50 + MODELS.index(model), 0, n, 0)
        sy = (sy + b"A" * n)[:n]  # n bases each: the widest diagonal has n + 1 cells
        out.append((n, n == first, Case("expect-global-%s-%d" % (model, n), model, ((sx, sy, (), n == first, n != first),), {})))
    return tuple(out)


# ---- 7. slots ----
SLOT_FORMS = ("in_traceback_one_group", "in_traceback_two_groups", "second_pass", "packed", "team")


@functools.lru_cache(maxsize=None)
def slots_case(form, S):
    """(environment, what a trace line must say, [the same small batch as a Case under each of the three slot models])."""
    rng = random.Random(5500 + SLOT_FORMS.index(form))
    pkw = {}
    if form == "in_traceback_one_group":
        probs, env, words = [_of_width(rng, w) for w in (20, 50, 64)], {}, r"widest diagonal 64,.*inside the traceback"
    elif form == "in_traceback_two_groups":
        probs, env = [_of_width(rng, w) for w in (70, 100, 128)], {"CPECAN_EXP_INSWEEP": "2"}
        words = r"widest diagonal 128,.*inside the traceback"
    elif form == "second_pass":
        probs, env = [_of_width(rng, w) for w in (129, 150, 200)], {}
        words = r"widest diagonal 200,.*one wave per region(?!.*inside the traceback)"
    elif form == "packed":
        probs = [make_pair(8, 20 + i, 150 + 40 * i, 12, anchor_every=3) for i in range(4)]
        env, words, pkw = {"CPECAN_PACKED": "2"}, r"cpecan packed class \d+: 4 regions in groups of \d+ lanes", dict(diagonalExpansion=12)
    else:
        probs, env, words = [ic._unanchored(36, 2, 500), ic._unanchored(36, 3, 400)], {"CPECAN_TEAM": "100"}, r"a team of waves per region"
    probs = tuple((sx, sy, tuple(map(tuple, a)), i % 2 == 0, i % 3 == 0) for i, (sx, sy, a) in enumerate(probs))
    return env, words, tuple(Case("expect-slots-%s-%s" % (form, m), m, probs, pkw) for m in slot_models(S))


# ---- the cases by what they are for ----
def categories(model):
    """{category: cases} of one model of MODELS: tests/test_expect_cases_cpu.py asks of every category that one of its
    problems is well_covered."""
    out = {"widths": [widths_case(model)]}
    if model in EDGE_MODELS:
        out["edges"] = [edges_case(model)]
    if model in ASYMMETRIC:
        out["n-rich"] = [n_rich_case(model)]
        out["packed"] = [c for _, c in packed_cases(model)]
        out["team"] = [c for _, _, c in team_cases(model)]
    if model in GLOBAL_MODELS:
        out["global rows"] = [c for _, _, c in global_cases(model)]
    return out


def all_cases():
    """Every case a GPU test compares with the oracle's counts."""
    out = [c for m in MODELS for cases in categories(m).values() for c in cases]
    for form in SLOT_FORMS:
        for S in SLOT_TYPES:
            out += slots_case(form, S)[2]
    return out
