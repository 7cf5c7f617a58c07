"""Seeded models and problems of the indel-emitter tests (CPECAN_EMIT_INDEL: the match, gapX and gapY lists of
diagonalCalculationPosteriorProbs, pairwiseAligner.c:691-733), shared by the CPU suite (tests/test_indel_cases_cpu.py:
the preconditions, with the oracle alone) and the GPU suite (tests/test_gpu_indel.py: the kernels against the oracle).
Nothing here touches a device.

A problem is (sX, sY, anchors, raggedLeft, raggedRight); a Case is a batch of problems under one model and one set of
parameters.  Case names are unique: the oracle's lists of a case are computed once per process and shared."""
import collections
import functools
import random

import numpy as np

import oracle_binding as ob
import reference_cases as rc
from cpecan_amd import api
from cpecan_amd.workload import make_pair
from test_gpu_forward import DEGENERATE, RAGGED, _diagonal_anchors, _model_pair, _same_length_pair
from test_gpu_parity import _evolve, _rand_seq

PROB_1 = 10000000
Case = collections.namedtuple("Case", "name model problems pkw")

# ---- models: name -> (library model, the oracle's model from the same numbers) ----
TYPE_OF = {"fiveState": api.fiveState, "fiveStateAsymmetric": api.fiveStateAsymmetric, "threeState": api.threeState,
           "threeStateAsymmetric": api.threeStateAsymmetric, "trained": api.fiveStateAsymmetric}
MODELS = tuple(TYPE_OF)
ASYMMETRIC = ("fiveStateAsymmetric", "threeStateAsymmetric", "trained")


@functools.lru_cache(maxsize=None)
def model_pair(name):
    """The default model of the two symmetric types; types 1 and 3 from the randomised, normalised HMM of
    test_gpu_forward._model_pair; "trained": the five-state-asymmetric HMM cPecanEm trained in the reference's own test
    (tests/golden/trained_hmm_cPecanEmTest.txt), loaded as test_trained_hmm_of_the_reference_through_the_gpu loads it."""
    if name != "trained":
        return _model_pair(TYPE_OF[name])
    mtype, T, _, E = rc.trained_hmm_numbers()
    assert mtype == api.fiveStateAsymmetric
    oh = ob.hmm(ob.FIVE_STATE_ASYM, 0.0)
    for i, v in enumerate(T):
        oh.T[i] = v
    for i, v in enumerate(E):
        oh.E[i] = v
    return api.hmm_getStateMachine(api.hmm_loadFromFile(rc.TRAINED_HMM)), ob.model_from_hmm(oh)


def states(name):
    return 5 if TYPE_OF[name] in (api.fiveState, api.fiveStateAsymmetric) else 3


# ---- the threshold excuse of parity.assert_pairs_match, and its cap ----
def slack(threshold):
    """parity.assert_pairs_match excuses a pair present on one side only when its score is this close to the threshold."""
    return max(2.0, 2e-5 * threshold * PROB_1)


def near_threshold(triples, threshold):
    """How many entries of a list lie within the slack of the threshold: the pairs a correct kernel may lose or gain."""
    s = np.asarray(triples, dtype=np.int64).reshape(-1, 3)[:, 0]
    return int((np.abs(s - threshold * PROB_1) <= slack(threshold)).sum())


def one_sided_allowed(threshold, oracle_len):
    """Pairs on one side only: at most 0.5 % of the oracle's list, none at threshold 0 (nothing is near that threshold:
    every cell of the list's domain is emitted)."""
    return 0 if threshold == 0 else int(0.005 * oracle_len)


_oracle_cache = {}


def oracle_lists(case):
    """[(match, gapX, gapY)] of every problem of the case from the oracle; computed once, never modified."""
    if case.name not in _oracle_cache:
        om, op = model_pair(case.model)[1], ob.params(**case.pkw)
        out = []
        for sx, sy, a, rl, rr in case.problems:
            lists = ob.aligned_pairs_with_indels(om, sx, sy, a, op, rl, rr)
            for t in lists:
                t.setflags(write=False)
            out.append(lists)
        _oracle_cache[case.name] = (case, tuple(out))
    kept, out = _oracle_cache[case.name]
    assert kept is case or kept == case, "two cases share the name %s" % case.name
    return out


def _tname(threshold):
    return "%g" % threshold


# ---- 1. models, thresholds and ragged ends with one wave per region ----
UNANCHORED = (1, 5, 63, 64, 65, 127, 128, 129)
UNANCHORED_ABOVE_ZERO = (200, 300)
THRESHOLDS = (0.0, 1e-4, 0.01, 0.2)


def precondition_holds(lists, threshold):
    """What makes the cap on one-sided pairs meaningful, for the oracle alone: of each list at most 0.25 % of the entries
    lie within the slack of the threshold.  (Nothing to ask at threshold 0: p >= 0 holds for every cell.)"""
    return threshold == 0 or all(near_threshold(t, threshold) <= 0.0025 * len(t) for t in lists)


def _drawn(model, draw, ragged, thresholds, **pkw):
    """draw(0), draw(1), ... until the oracle's lists of the problem meet precondition_holds at every threshold."""
    om = model_pair(model)[1]
    for k in range(100):
        sx, sy, a = draw(k)
        pr = (sx, sy, tuple(map(tuple, a))) + tuple(ragged)
        if all(precondition_holds(ob.aligned_pairs_with_indels(om, *pr[:3], ob.params(threshold=t, **pkw), *ragged), t) for t in thresholds):
            return pr
    raise AssertionError("no problem meets the precondition under %s, %r" % (model, pkw))


@functools.lru_cache(maxsize=None)
def _models_problems(model, E, zero):
    """The problems of one batch of models_cases.  The same problems serve every threshold above 0, and a problem is drawn
    again (the next numbers of the same generator) until the oracle's lists of it meet precondition_holds at each of them:
    under the default models a list at 1e-4 has a few hundred entries, one of which may sit on the threshold."""
    rng = random.Random(4000 + 10 * MODELS.index(model) + E)
    length, most = (120, 135) if zero else (600, 10 ** 9)  # (at threshold 0 no sequence over 135 bases)
    draws = []
    if E == 10:
        for n in UNANCHORED + (() if zero else UNANCHORED_ABOVE_ZERO):
            draws.append(lambda k, n=n: tuple(s[:most] for s in _same_length_pair(rng, n)) + ((),))
    for i in range(2):
        draws.append(lambda k, i=i: tuple(make_pair(11, E + i + 2 * k, length, E)))
    for _ in range(3):
        def masked(k):
            sx = _rand_seq(rng, rng.randrange(90, 130) if zero else rng.randrange(200, 320))
            sy = (_evolve(rng, sx) or "acgtn")[:most]
            return sx, sy, _diagonal_anchors(len(sx), len(sy), 29, E)
        draws.append(masked)
    return tuple(_drawn(model, draw, RAGGED[(i + i // 4 + E // 40) % 4], () if zero else THRESHOLDS, diagonalExpansion=E)
                 for i, draw in enumerate(draws))


@functools.lru_cache(maxsize=None)
def models_cases(model, threshold):
    """Two batches, one per band expansion (the expansion is a parameter of the batch).  The first holds the unanchored
    pairs -- related sequences whose widest diagonal is just under, at and over one and two 64-lane groups, and at
    thresholds above 0 four and five groups -- next to banded pairs of expansion 10; the second banded pairs of expansion
    40.  Both hold banded pairs with N and lower case (the unanchored ones are from that alphabet as well).  At threshold
    0 every problem stays at about 130 bases: a list then holds every cell of the band.  All four ragged combinations go
    round each list."""
    return tuple(Case("models-%s-%s-E%d" % (model, _tname(threshold), E), model, _models_problems(model, E, threshold == 0),
                      dict(threshold=threshold, diagonalExpansion=E)) for E in (10, 40))


# ---- 2. edges and the -1 coordinates ----
EDGE_SIZES = ((1, 1), (1, 7), (7, 1), (5, 5), (64, 3), (3, 64), (65, 65), (130, 40))
EDGE_MODELS = ("fiveState", "threeStateAsymmetric")


def _pair_of_lengths(rng, lX, lY):
    sx = _rand_seq(rng, lX)
    sy = "".join(ch if rng.random() < 0.8 else _rand_seq(rng, 1) for ch in sx)
    return sx, (sy + _rand_seq(rng, lY))[:lY]


@functools.lru_cache(maxsize=None)
def edges_case(model):
    """Threshold 0, unanchored, unbanded: every size with all four ragged combinations."""
    rng = random.Random(4100 + MODELS.index(model))
    probs = []
    for lX, lY in EDGE_SIZES:
        for ragged in RAGGED:
            probs.append(_pair_of_lengths(rng, lX, lY) + ((),) + ragged)
    return Case("edges-%s" % model, model, tuple(probs), dict(threshold=0.0))


@functools.lru_cache(maxsize=None)
def degenerate_case(model, threshold):
    """test_gpu_forward.DEGENERATE under every ragged combination, an ordinary problem after every third."""
    rng = random.Random(4200 + MODELS.index(model))
    ordinary = []
    for i in range(4):
        sx, sy, a = make_pair(12, i, 100, 10)
        ordinary.append((sx, sy, tuple(map(tuple, a))))
    ordinary += [_same_length_pair(rng, 70) + ((),) for _ in range(4)]
    probs = []
    for k, ragged in enumerate(RAGGED):
        for j, (sx, sy) in enumerate(DEGENERATE):
            probs.append((sx, sy, ()) + ragged)
            if j % 3 == 2:
                probs.append(tuple(ordinary[2 * k + j // 3]) + ragged)
    return Case("degenerate-%s-%s" % (model, _tname(threshold)), model, tuple(probs), dict(threshold=threshold, diagonalExpansion=10))


# ---- 3. every kernel form with asymmetric models ----
FORM_THRESHOLDS = (1e-3, 0.01)
PACKED_EXPANSIONS = ((2, 8, 10), (6, 16, 10 ** 12), (26, 32, 10))  # (expansion, lanes of a group, splitMatrixBiggerThanThis)


@functools.lru_cache(maxsize=None)
def _packed_batch(model, E, split):
    rng = random.Random(4300 + 10 * MODELS.index(model) + E)
    pkw = dict(diagonalExpansion=E, minDiagsBetweenTraceBack=rng.randrange(40, 200), traceBackDiagonals=rng.randrange(3, 30),
               splitMatrixBiggerThanThis=split)

    def draw(k):
        sx = _rand_seq(rng, rng.randrange(1, 400))
        sy = _evolve(rng, sx) or "C"
        anchors, x, y = [], -1, -1
        while True:
            x += rng.randrange(1, 5)
            y += rng.randrange(1, 5)
            if x >= len(sx) or y >= len(sy):
                return sx, sy, anchors
            anchors.append((x, y, E))

    probs = [_drawn(model, draw, (rng.random() > 0.5, rng.random() > 0.5), FORM_THRESHOLDS, **pkw) for _ in range(16)]
    probs += [("A", "A", (), False, False), ("ACGTAC", "", (), False, True), ("", "GGT", (), True, True)]
    return tuple(probs), pkw


@functools.lru_cache(maxsize=None)
def packed_cases(model, threshold):
    """(lanes of a group, case): the dense random anchors of test_packed_kernel_indel_emitter, a batch per group width of
    the packed kernel, short traceback schedules, split rectangles in two of the three, one-base and one-sided problems
    at the end; the same problems at both thresholds, drawn as those of models_cases."""
    out = []
    for E, lanes, split in PACKED_EXPANSIONS:
        probs, pkw = _packed_batch(model, E, split)
        out.append((lanes, Case("packed-%s-%s-E%d" % (model, _tname(threshold), E), model, probs, dict(pkw, threshold=threshold))))
    return tuple(out)


def _unanchored(seed, index, length):
    sx, sy, _ = make_pair(seed, index, length, 0)
    return sx, sy, ()


@functools.lru_cache(maxsize=None)
def team_cases(model, threshold):
    """(words the trace line of the class must carry, CPECAN_TEAM, case): unanchored 500 x 500 (501 cells: four waves), five
    states only 900 x 900 (eight waves, by the library's own choice), and a multi-segment band of ~157 cells that
    CPECAN_TEAM=100 forces onto the team."""
    # (501 cells of three states leave one wave per region four waves on a CU, and the library keeps it: CPECAN_TEAM=500
    # puts the class on the team all the same; with five states the team is the library's own choice)
    out = [("(four)", None if states(model) == 5 else "500", Case("team4-%s-%s" % (model, _tname(threshold)), model, (_unanchored(36, 0, 500) + (True, False),),
                                 dict(threshold=threshold, diagonalExpansion=40)))]
    if states(model) == 5:
        out.append(("(eight)", None, Case("team8-%s-%s" % (model, _tname(threshold)), model, (_unanchored(34, 0, 900) + (False, True),),
                                          dict(threshold=threshold, diagonalExpansion=40))))
    sx, sy, a = make_pair(3, 5, 1500, 100)
    out.append(("a team of waves", "100", Case("team100-%s-%s" % (model, _tname(threshold)), model,
                                               ((sx, sy, tuple(map(tuple, a)), True, True),),
                                               dict(threshold=threshold, diagonalExpansion=100))))
    return tuple(out)


LDS_PATH_MAX_BYTES = 64 * 1024


def indel_wave_lds_bytes(S, lX, lY):
    """cpk_plan.inl, set_row_form, for an indel class of one unanchored lX x lY pair with one wave per region: the header
    of 232 doubles (logAdd cubics, emission + transition weights), the candidate stage of 3 lists x 2 doubles x kStage
    (128) slots, 2 S + 1 rolling rows of maxWidth + 1 doubles, and both strings at two symbols a byte."""
    width = min(lX, lY) + 1
    return 8 * (232 + 3 * 2 * 128 + (2 * S + 1) * (width + 1)) + ((lX + 3) // 2 + (lY + 3) // 2 + 15) // 16 * 16


def in_global_memory(S, n):
    """plan_wide_class: the rolling rows of the class go to global memory when one wave's LDS plus 16 bytes is over 64 KB."""
    return indel_wave_lds_bytes(S, n, n) + 16 > LDS_PATH_MAX_BYTES


def first_global_length(S):
    """The smallest n whose unanchored n x n pair (n + 1 cells on the widest diagonal) no longer fits."""
    n = 1
    while not in_global_memory(S, n):
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def global_cases(model, threshold):
    """(length, in global memory, case) for the last length that keeps its rows in LDS and the first that does not."""
    S = states(model)
    first = first_global_length(S)
    out = []
    for n in (first - 1, first):
        sx, sy, _ = make_pair(40 + MODELS.index(model), 0, n, 0)
        sy = (sy + b"A" * n)[:n]  # n bases each: the widest diagonal has n + 1 cells
        out.append((n, n == first, Case("global-%s-%s-%d" % (model, _tname(threshold), n), model, ((sx, sy, (), n == first, n != first),),
                                        dict(threshold=threshold))))
    return tuple(out)


# ---- 4. the overflow re-run with three lists ----
OVERFLOW_THRESHOLD = 1e-4


def default_slice(case, i):
    """cpecan_host.c, default_out_cap, for problem i as one region: 6 (lX + lY) + 64 triples per list, or every cell of
    the band where that is fewer (or the threshold is 0)."""
    sx, sy, a, rl, rr = case.problems[i]
    cells = ob.band_cells(sx, sy, a, ob.params(**case.pkw), rl, rr)
    cap = 6 * (len(sx) + len(sy)) + 64
    return cells if case.pkw.get("threshold", 0.01) <= 0 or cap > cells else cap


def _followers(rng):
    """Problems that cannot overflow -- their slice is every cell of the band: they follow the overflowing ones in the batch."""
    return [_pair_of_lengths(rng, 5, 5) + ((), False, False), _pair_of_lengths(rng, 1, 7) + ((), True, False),
            _pair_of_lengths(rng, 12, 12) + ((), False, False), _pair_of_lengths(rng, 14, 9) + ((), False, True),
            ("ACGT", "", (), False, True)]


@functools.lru_cache(maxsize=None)
def overflow_gap_only_case():
    """(a) X: 40 random bases; Y: 130 random bases + X + 130 random bases, three-state default model, unanchored: the
    gapY list of the first problem outgrows its slice, the match list does not."""
    rng = random.Random(4400)
    sx = _rand_seq(rng, 40)
    sy = _rand_seq(rng, 130) + sx + _rand_seq(rng, 130)
    return Case("overflow-gapY", "threeState", tuple([(sx, sy, (), False, False)] + _followers(rng)), dict(threshold=OVERFLOW_THRESHOLD))


@functools.lru_cache(maxsize=None)
def overflow_all_case():
    """(b) unanchored 64 x 64 under the random type 1: all three lists of the first problem outgrow the slice of 832."""
    rng = random.Random(4401)
    sx, sy = _same_length_pair(rng, 64)
    return Case("overflow-all", "fiveStateAsymmetric", tuple([(sx, sy[:64], (), False, False)] + _followers(rng)),
                dict(threshold=OVERFLOW_THRESHOLD))


@functools.lru_cache(maxsize=None)
def overflow_packed_case():
    """(b) on the packed kernel: the dense anchors and narrow bands of test_packed_kernel_output_overflow_rerun."""
    probs = []
    for i in range(6):
        sx, sy, a = make_pair(8, i, 200 + 30 * i, 12, anchor_every=3)
        probs.append((sx, sy, tuple(map(tuple, a)), False, False))
    probs += _followers(random.Random(4402))
    return Case("overflow-packed", "fiveStateAsymmetric", tuple(probs), dict(threshold=OVERFLOW_THRESHOLD, diagonalExpansion=12))


# ---- 5. size classes in one batch ----
SIZE_CLASS_SLICE = slice(46, 53)


@functools.lru_cache(maxsize=None)
def size_classes_case():
    """The batch of test_mixed_widths_run_in_size_classes under the random type 3: regions of every wide class, in an order
    that is not the device's (by class, then longest first)."""
    probs = [make_pair(31, i, 400, 40) for i in range(40)]                # <= 128 cells
    probs += [_unanchored(32, i, 150) for i in range(6)]                  # <= 256
    probs += [_unanchored(33, i, 300) for i in range(4)]                  # fits the LDS
    probs += [_unanchored(36, i, 500) for i in range(2)]                  # 501 cells
    probs += [_unanchored(34, 0, 900)]                                    # 901 cells
    probs += [make_pair(35, i, 200, 40) for i in range(80)]               # more of the first class, behind the wide ones
    probs = [(sx, sy, tuple(map(tuple, a)), False, False) for sx, sy, a in probs]
    return Case("size-classes", "threeStateAsymmetric", tuple(probs), dict(diagonalExpansion=40))


# ---- 6. the consumers on these lists ----
CONSUMER_MODELS = ("threeStateAsymmetric", "fiveStateAsymmetric")
CONSUMER_THRESHOLDS = (1e-4, 0.01)


@functools.lru_cache(maxsize=None)
def consumers_case(model, threshold):
    """Problems for all three kernels in one batch (under CPECAN_PACKED=2): dense anchors of expansion 12 (13-cell bands:
    packed), unanchored pairs of 20-160 bases (one wave per region) and one unanchored 500 x 500 pair (a team of four)."""
    rng = random.Random(4600 + MODELS.index(model))
    probs = []
    for i in range(6):
        sx, sy, a = make_pair(8, 10 + i, 150 + 40 * i, 12, anchor_every=3)
        probs.append((sx, sy, tuple(map(tuple, a))))
    for _ in range(8):
        sx = _rand_seq(rng, rng.randrange(20, 160))
        probs.append((sx, _evolve(rng, sx) or "A", ()))
    probs.append(_unanchored(36, 1, 500))
    return Case("consumers-%s-%s" % (model, _tname(threshold)), model, tuple(p + (False, False) for p in probs),
                dict(threshold=threshold, diagonalExpansion=12))


def all_cases():
    """Every case a GPU test compares with the oracle's lists."""
    out = []
    for model in MODELS:
        for threshold in THRESHOLDS:
            out += models_cases(model, threshold)
    for model in EDGE_MODELS:
        out.append(edges_case(model))
        out += [degenerate_case(model, t) for t in (0.0, 0.01)]
    for model in ASYMMETRIC:
        for threshold in FORM_THRESHOLDS:
            out += [c for _, c in packed_cases(model, threshold)]
            out += [c for _, _, c in team_cases(model, threshold)]
            out += [c for _, _, c in global_cases(model, threshold)]
    out += [overflow_gap_only_case(), overflow_all_case(), overflow_packed_case(), size_classes_case()]
    return out
