"""The inputs of the Viterbi count tests (tests/test_viterbi_counts_cpu.py, test_gpu_viterbi_counts.py): every case of
tests/viterbi_cases.py -- the empty sequences with a path of zero steps, p_no_path, the three-region cases, the ties, the -inf
transitions, all four model types -- and the smallest inputs at which the count kernel of cpk_viterbi.inl can go wrong: paths
whose run count sits at the kernel's pass of 64 runs (63, 64, 65) and past two passes (129), one run longer than four passes
of the wave over its steps, N bases in the middle of both sequences, a path that starts with a gap run along row 0.
check_preconditions() asserts of every new case the edge it is there for.  The model's counts are computed once per case and
never modified.  Nothing here touches a GPU.
"""
import functools
import random

import viterbi_cases as vc
import viterbi_counts_model as cm

Case = vc.Case
PASS = 64  # runs a pass of cpecan_viterbi_count lays out, and steps it spreads over the lanes at a time (CPK_WAVE)


def _anchored(name, sx, sy, model="fiveState", ragged_left=False, ragged_right=False):
    """A band of expansion 8 around anchors on the main diagonal, as viterbi_cases._narrow makes it."""
    n = min(len(sx), len(sy))
    anchors = tuple((i, i, 8) for i in range(5, n - 2, 6))
    return Case(name, model, sx, sy, anchors, dict(diagonalExpansion=8), ragged_left, ragged_right)


def _runs(name, n_indels, end_on_gap, seed):
    """X against X with, every 10 bases, in turn one base left out and one base put in, so that the path leaves the anchors'
    diagonal by one and comes back: 2 * n_indels + 1 runs, match runs and one-step gap runs alternating.  end_on_gap: the last
    block of matches is left out and the path ends on the last indel, a base put in: one run fewer.  Where a block of random
    bases happens to fit its shifted copy, mismatches are cheaper than the two gaps around it and the path loses runs: the seeds
    used are ones at which it does not, and check_preconditions holds the model's path to the run count."""
    rng = random.Random(seed)
    sx, sy = bytearray(), bytearray()
    for k in range(n_indels):
        block = bytearray(vc._rand_seq(rng, 10))
        sx += block
        if k % 2 == 0:  # the block's last base is missing in Y; it differs from its neighbours, so the gap has one place
            while block[-1] == block[-2]:
                block[-1] = rng.choice(b"ACGT")
            sx[-1] = block[-1]
            sy += block[:-1]
        else:  # a base put into Y that differs from both neighbours
            sy += block
            sy.append(next(b for b in b"ACGT" if b != block[-1]))
    if not end_on_gap:
        block = vc._rand_seq(rng, 10)
        while sy and block[0] in (sy[-1], sx[-1]):
            block = vc._rand_seq(rng, 10)
        sx += block
        sy += block
    return _anchored(name, bytes(sx), bytes(sy))


def _long_run():
    s = vc._rand_seq(random.Random(77), 300)
    return _anchored("k_one_run_300", s, s)


def _n_in_the_middle():
    s = bytearray(vc._rand_seq(random.Random(78), 90))
    sx, sy = bytearray(s), bytearray(s)
    sx[40:45] = b"NNNNN"
    sy[43:47] = b"NNNN"
    return _anchored("k_n_middle", bytes(sx), bytes(sy), model="threeState")


def _leading_gap():
    rng = random.Random(79)
    common = vc._rand_seq(rng, 40)
    return Case("k_leading_gap", "fiveState", b"GGGGGGGGGGGG" + common, common, (), {}, True, False)


@functools.lru_cache(maxsize=None)
def new_cases():
    return (_runs("k_runs_63", 31, False, 7031), _runs("k_runs_64", 32, True, 7032), _runs("k_runs_65", 32, False, 7032),
            _runs("k_runs_129", 64, False, 7078),
            _long_run(), _n_in_the_middle(), _leading_gap())


@functools.lru_cache(maxsize=None)
def cases():
    return vc.cases() + new_cases()


CASE_NAMES = tuple(c.name for c in cases())
# the cases every kernel form can run and that are small (viterbi_cases.SMALL_CASE_NAMES), and the new ones, all narrow
SMALL_CASE_NAMES = vc.SMALL_CASE_NAMES + tuple(c.name for c in new_cases())


def case(name):
    return cases()[CASE_NAMES.index(name)]


def n_states(c):
    return vc.model_pair(c.model)[1].S


_counts = {}


def region_counts(c):
    """[Counts] per region of the case, from the model's path; computed once, never modified."""
    if c.name not in _counts:
        _counts[c.name] = tuple(cm.regions(n_states(c), vc.model_of(c), vc.region_inputs(c)))
    return _counts[c.name]


def problem_counts(c):
    return cm.total(n_states(c), region_counts(c))


def check_preconditions():
    """Each new case is the edge it is there for."""
    for name, want in (("k_runs_63", 63), ("k_runs_64", 64), ("k_runs_65", 65), ("k_runs_129", 129)):
        c = case(name)
        m = vc.model_of(c)
        assert len(m.regions) == 1 and vc.widest(c) <= 16, name
        assert len(m.ops) == want, (name, len(m.ops))
        assert {int(s) for s in m.ops[:, 0]} >= {0, 1, 2}, "match runs and gap runs of both kinds"
    assert PASS - 1 == 63 and 2 * PASS + 1 == 129
    assert int(vc.model_of(case("k_runs_64")).ops[-1, 0]) != 0, "the path ends on a gap run"
    m = vc.model_of(case("k_one_run_300"))
    assert len(m.regions) == 1 and m.ops.tolist() == [[0, 300]] and 300 > 4 * PASS and m.regions[0].startState == 0
    c = case("k_n_middle")
    m, pc = vc.model_of(c), problem_counts(c)
    assert b"N" in c.sx[30:60] and b"N" in c.sy[30:60] and len(m.regions) == 1
    lost = cm.steps_without_emission(c.sx, c.sy, m.ops)
    assert lost >= 5 and int(pc.emissions.sum()) < pc.nSteps and pc.nSteps - int(pc.emissions.sum()) == lost
    assert int(pc.transitions.sum()) == pc.nSteps
    c = case("k_leading_gap")
    m, pc = vc.model_of(c), problem_counts(c)
    assert len(m.regions) == 1 and c.ragged_left and int(m.ops[0, 0]) in (1, 3) and int(m.ops[0, 1]) >= 10, m.ops[:2]
    assert pc.nSteps - int(pc.emissions.sum()) == int(m.ops[0, 1]) == cm.steps_without_emission(c.sx, c.sy, m.ops), "row 0 sees N"
    # the edges that come with viterbi_cases
    for name in ("f_both0", "z_both0_ragged"):
        pc = problem_counts(case(name))
        assert (pc.nSteps, pc.nNoPath) == (0, 0) and pc.logP == vc.model_of(case(name)).logP and pc.logP > float("-inf")
    pc = problem_counts(case("p_no_path"))
    assert (pc.nSteps, pc.nNoPath, pc.logP) == (0, 1, 0.0)
    assert len(region_counts(case("r_three"))) >= 3
    assert {case(n).model for n in CASE_NAMES} >= set(vc.MODEL_TYPES)
