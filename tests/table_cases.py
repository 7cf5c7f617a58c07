"""Constructed inputs of the band-table tests, shared by the CPU suite (tests/test_table_cases_cpu.py: every case really has
the edge it was built for, asserted with tests/table_model.py alone) and the GPU suite (tests/test_gpu_table.py: the table
the device built, entry by entry against the model).  Nothing here touches a device.

A problem is (sX, sY, anchors, raggedLeft, raggedRight) with anchors (x, y, expansion); a Case is a batch of problems under
one model and one set of parameters, and names the launch plans (PLANS) it is built for; `positions`: under its split plans
the batch must carry position words (a fixed expansion and every band smooth, so every class runs under absolute positions).
The sequences' letters do not matter to the table: only their lengths and the anchors do."""
import collections
import functools
import random

import table_model as tm

Case = collections.namedtuple("Case", "name mtype pkw problems plans positions")

# The planning knobs of a launch plan.  CPECAN_PACKED=0: every region in a wide class, one wave each; CPECAN_SPLIT=0 keeps
# them whole (rings of cells that wrap, the serial builder), 1 / 2 split every class that has a traceback (rings of
# doubles, the wave builder) in the two-launch / one-launch form.  "mixed": narrow regions packed and whole, wide ones split.
PLANS = {
    "whole": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "0"},
    "split1": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1"},
    "split2": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "2"},
    "mixed": {"CPECAN_PACKED": "2", "CPECAN_PACKED_SPLIT": "0", "CPECAN_SPLIT": "1"},
}
# every other knob the plan or the builders read is unset while a case runs
OTHER_KNOBS = ("CPECAN_ABS", "CPECAN_ABS_WINDOWS", "CPECAN_TABLE_WAVE", "CPECAN_KEEP_RUNS", "CPECAN_FAST_WALK", "CPECAN_TEAM",
               "CPECAN_DENSE", "CPECAN_PACKED_SPLIT_FROM", "CPECAN_MEM_BUDGET_MB", "CPECAN_SPLIT_BUDGET_FRAC",
               "CPECAN_MAX_WAVES_PER_CU", "CPECAN_FUSED_SPIN", "CPECAN_THREADS")
SPLIT_PLANS = ("split1", "split2")
SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)  # a traceback every 42 diagonals of a narrow band


def seq(n, seed=0):
    rng = random.Random(1000 * n + seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def problem(lX, lY, anchors=(), expansion=0, seed=0):
    return (seq(lX, seed), seq(lY, seed + 1), tuple((x, y, e[0] if e else expansion) for x, y, *e in anchors), False, False)


def path(lX, lY, seed, lo=3, hi=12):
    """Anchors that wander from corner to corner in steps of lo .. hi - 1 columns and rows."""
    rng, out, x, y = random.Random(seed), [], -1, -1
    while True:
        x += rng.randrange(lo, hi)
        y += rng.randrange(lo, hi)
        if x >= lX or y >= lY:
            return out
        out.append((x, y))


def on_diagonals(diagonals, lean=0):
    """One anchor on each of the given matrix diagonals (x + y + 2, ascending and at least 2 apart), near the main diagonal."""
    out = []
    for d in diagonals:
        s = d - 2
        x = s // 2 + lean
        out.append((x, s - x))
    assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(out, out[1:])), out
    return out


# ---- wave builder: chunking ----
CHUNK_SIZES = ((0, 0), (1, 0), (31, 31), (0, 63), (64, 0), (63, 63), (64, 63), (64, 64), (100, 99), (500, 499))


def _chunk_problems(E):
    return [problem(lX, lY, path(lX, lY, 7 + lX) if lX + lY > 150 else (), E, seed=lX) for lX, lY in CHUNK_SIZES]


def chunk_case():
    """lX + lY + 1 in {1, 2, 63, 64, 65, 127, 128, 129, 200, 1000}: lanes without a diagonal, a short last chunk, lX or lY 0."""
    E = 10
    return Case("chunks", 0, dict(diagonalExpansion=E, **SHORT), _chunk_problems(E), ("whole",) + SPLIT_PLANS, True)


# ---- wave builder: the binary search that sets a lane's iterator ----
SEARCH_L = 160  # 321 diagonals: chunks of 6, the last lane with diagonals (53) holds 3
SEARCH_DIAGONALS = (29, 60, 91, 119, 121, 150, 180)  # d0 - 1, d0, d0 + 1 of lanes 5, 10, 15; both sides of lane 20; d0 of 25, 30


def search_case():
    E = 4
    probs = [problem(SEARCH_L, SEARCH_L, (), E), problem(SEARCH_L, SEARCH_L, on_diagonals((120,)), E, seed=1),
             problem(SEARCH_L, SEARCH_L, on_diagonals(SEARCH_DIAGONALS), E, seed=2),
             problem(SEARCH_L, SEARCH_L, on_diagonals(range(6, 318, 6)), E, seed=3),   # an anchor on every lane's first diagonal
             problem(SEARCH_L, SEARCH_L, on_diagonals(range(11, 318, 12)), E, seed=4)]  # ... on every other lane's last
    return Case("search", 0, dict(diagonalExpansion=E, **SHORT), probs, ("whole",) + SPLIT_PLANS, True)


# ---- wave builder: per-anchor expansions ----
DYNAMIC_L = 150  # 301 diagonals: chunks of 5
DYNAMIC_ANCHORS = tuple((x, y, e) for (x, y), e in zip(on_diagonals((30, 55, 80, 101, 124, 150, 170)), (0, 24, 0, 20, 2, 30, 24)))


def dynamic_case():
    """Anchors on the first diagonals of lanes 6, 11, 16, 30 and 34 (and one off lanes 20's and 25's), neighbours with
    expansions 0 and 20 or more, and 26 lanes behind the last anchor, whose expansion of 24 stays in force."""
    pkw = dict(dynamicAnchorExpansion=1, diagonalExpansion=30, minDiagsBetweenTraceBack=60, traceBackDiagonals=7)
    rng = random.Random(5)
    fuzz = tuple((x, y, 2 * rng.randrange(0, 12)) for x, y in path(120, 130, 9))
    probs = [problem(DYNAMIC_L, DYNAMIC_L, DYNAMIC_ANCHORS), problem(120, 130, fuzz, seed=1), problem(90, 70, (), seed=2),
             problem(100, 100, ((50, 50, 0),), seed=3), problem(100, 100, ((49, 49, 40),), seed=4)]
    return Case("dynamic", 0, pkw, probs, ("whole",) + SPLIT_PLANS, False)


# ---- serial builder: the anchor queue ----
QUEUE_COUNTS = (1, 2, 7, 8, 9, 16, 17)  # around the queue's depth of 8 and twice that


def _queue_problems(dynamic, E=6):
    probs = []
    for n in QUEUE_COUNTS:
        anchors = [(3 + 5 * i + (i % 2), 2 + 5 * i + 2 * (i % 3 == 0), 2 * (i % 4)) for i in range(n)]
        probs.append(problem(95, 97, anchors if dynamic else [a[:2] for a in anchors], E, seed=n))
    return probs


def queue_case(dynamic=False):
    pkw = dict(diagonalExpansion=6, dynamicAnchorExpansion=int(dynamic), **SHORT)
    return Case("queue-dynamic" if dynamic else "queue", 0, pkw, _queue_problems(dynamic), ("whole", "split1"), not dynamic)


# ---- the run shortcut ----
RUN_EXPANSIONS = (0, 2, 4, 10)


def _diag(x, y, n):
    return [(x + k, y + k) for k in range(n)]


def run_problems(E):
    probs = []
    for n in (1, 2, 3, 40):  # identical sequences: one run from corner to corner
        s = seq(n, n)
        probs.append((s, s, tuple((k, k, E) for k in range(n)), False, False))
    probs.append(problem(50, 50, _diag(5, 6, 1) + _diag(10, 12, 2) + _diag(20, 22, 3) + _diag(40, 40, 10), E, seed=50))  # lengths 1, 2, 3; ends in the corner
    probs.append(problem(60, 64, _diag(0, 3, 30), E, seed=60))                        # starts at column 0
    probs.append(problem(64, 60, _diag(3, 0, 30), E, seed=61))                        # ... at row 0
    probs.append(problem(45, 46, _diag(10, 10, 10) + _diag(20, 21, 10), E, seed=45))  # two runs one indel apart
    probs.append(problem(46, 45, _diag(10, 10, 10) + _diag(21, 20, 10), E, seed=46))
    return probs


def run_case(E):
    return Case("runs-E%d" % E, 0, dict(diagonalExpansion=E, **SHORT), run_problems(E), ("whole", "split1"), True)


# ---- rings ----
RING_WHOLE_SEEDS = (3, 4, 5, 6)


def ring_whole_case():
    """Whole regions under a short schedule: rings of cells that wrap many times."""
    probs = [problem(300 + 7 * s, 310 - 5 * s, path(300 + 7 * s, 310 - 5 * s, s, 2, 9), 6, seed=s) for s in RING_WHOLE_SEEDS]
    return Case("ring-whole", 0, dict(diagonalExpansion=6, **SHORT), probs, ("whole",), False)


def ring_split_case(mtype):
    """Split regions, S = 5 (mtype 0) and S = 3 (mtype 2).  The 60-base identical pair has 121 diagonals in chunks of 2 and
    tracebacks from 50 and 92 that emit from 42 and 84: every one of them a lane's first diagonal."""
    E = 4
    s60 = seq(60, 60)
    probs = [(s60, s60, tuple((i, i, E) for i in range(60)), False, False),
             problem(200, 210, path(200, 210, 21, 2, 9), E, seed=21), problem(230, 190, path(230, 190, 22, 2, 9), E, seed=22)]
    return Case("ring-split-S%d" % (5 if mtype == 0 else 3), mtype, dict(diagonalExpansion=E, **SHORT), probs, SPLIT_PLANS, True)


# ---- position chains ----
CHAIN_L = 100  # 201 diagonals: chunks of 4


def _zigzag(lX, lY, first, second, turn_every):
    """Anchors that step by `first` (dx, dy) turn_every times, then by `second`, and so on: the band leans to one side
    and then to the other."""
    out, x, y, k = [], 1, 1, 0
    while x < lX - 2 and y < lY - 2:
        out.append((x, y))
        dx, dy = first if (k // turn_every) % 2 == 0 else second
        x, y, k = x + dx, y + dy, k + 1
    return out


def chain_case():
    E = 4
    probs = [problem(CHAIN_L, CHAIN_L, _zigzag(CHAIN_L, CHAIN_L, (7, 2), (2, 7), 3), E),
             problem(CHAIN_L, CHAIN_L, _zigzag(CHAIN_L, CHAIN_L, (3, 8), (9, 2), 2), E, seed=1),
             problem(CHAIN_L, CHAIN_L, (), E, seed=2),                                 # one smooth stretch, corner to corner
             problem(120, 120, ((3, 4), (9, 8), (14, 15)), E, seed=3),                 # anchors at the start, smooth behind
             problem(120, 120, ((104, 105), (110, 109), (115, 116)), E, seed=4)]       # ... at the end, smooth in front
    return Case("chains", 0, dict(diagonalExpansion=E, **SHORT), probs, SPLIT_PLANS, True)


# ---- problems cut into several regions ----
def _clusters(starts, n, step=3):
    """n anchors from each start, `step` apart and wobbling: between the clusters the matrix is cut."""
    return [(x0 + step * k, y0 + step * k + k % 2) for x0, y0 in starts for k in range(n)]


def multi_region_case():
    E = 4
    probs = [problem(260, 265, _clusters(((5, 5), (70, 75), (140, 150), (210, 215)), 8), E, seed=31),
             problem(200, 210, path(200, 210, 31, 3, 30), E, seed=32), problem(150, 150, ((20, 20), (130, 131)), E, seed=33)]
    return Case("multi-region", 0, dict(diagonalExpansion=E, splitMatrixBiggerThanThis=900, **SHORT), probs, ("whole", "split1"), True)


# ---- one batch of everything that shares a fixed expansion ----
def mixed_case():
    """Narrow regions (packed, whole) beside wide ones (split) in one batch: the host reorders the regions by class and
    size, and every region must still find its own slice of the table."""
    E = 4
    probs = (run_problems(E) + search_case().problems + chain_case().problems + ring_split_case(0).problems +
             multi_region_case().problems + _chunk_problems(E) + _queue_problems(False, E))
    return Case("mixed", 0, dict(diagonalExpansion=E, splitMatrixBiggerThanThis=2500, **SHORT), probs, ("mixed",), False)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [chunk_case(), search_case(), dynamic_case(), queue_case(False), queue_case(True)]
    cases += [run_case(E) for E in RUN_EXPANSIONS]
    cases += [ring_whole_case(), ring_split_case(0), ring_split_case(2), chain_case(), multi_region_case(), mixed_case()]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case(name):
    return next(c for c in all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def regions(name):
    """The model's regions of every problem of the case: computed once per process and shared (read-only)."""
    c = case(name)
    return tuple(tuple(tm.problem_regions(p, c.pkw)) for p in c.problems)
