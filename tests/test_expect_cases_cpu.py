"""The preconditions that make tests/test_gpu_expect.py meaningful, asserted with the oracle alone (no device): every
transition of a model gets a count the relative gate can test, the asymmetric models give counts a transposed index
would move, the N-rich problems really leave events out of the emission counts, the widths are the ones the cases are
named for, the ragged flags change the counts, and the oracle's counts of a batch are the sum of its problems'.

Coverage and asymmetry are asserted for every batch (Case) on its own, with two short lists of exceptions, each a
single-problem batch whose shape the team tests fix: NOT_COVERED and NOT_TRANSPOSED below name them, the tests assert that
they are exceptions indeed, and the kind they belong to (team) holds a planted problem that does meet the condition."""
import numpy as np
import pytest

import expect_cases as ec
import oracle_binding as ob
from cpecan_amd import api
from test_gpu_forward import DEGENERATE, RAGGED


def _all_counts(cases):
    return [(case, i, c) for case in cases for i, c in enumerate(ec.oracle_counts(case))]


# Related 500-, 900- and 700-base pairs without a long gap leave the long-gap transitions of the trained model (opened with
# probability 2e-4 to 5e-4) at counts of 4e-5 to 1e-4: on these batches the relative gate tests those four elements through
# its absolute part only.  expect-team4-planted-trained is the batch of the kind that covers them.
NOT_COVERED = ("expect-team4-trained-0.01", "expect-team8-trained-0.01", "expect-team-narrow-trained")


@pytest.mark.parametrize("model", ec.MODELS)
def test_every_case_has_a_problem_that_covers_every_transition(model):
    """... with a count of at least 1e-3: otherwise the relative gate tests nothing on that element."""
    for kind, cases in ec.categories(model).items():
        for case in cases:
            best = max(min(c.T[i] for i in ec.present_transitions(model)) for c in ec.oracle_counts(case))
            assert (best >= ec.MIN_COUNT) == (case.name not in NOT_COVERED), (case.name, best)
        assert any(ec.covers_every_transition(c, model) for _, _, c in _all_counts(cases)), kind
    assert all(name.endswith("trained") or "-trained-" in name for name in NOT_COVERED)


@pytest.mark.parametrize("form", ec.SLOT_FORMS)
def test_every_slots_batch_covers_every_transition(form):
    for S in ec.SLOT_TYPES:
        for case in ec.slots_case(form, S)[2]:
            assert any(ec.covers_every_transition(c, case.model) for c in ec.oracle_counts(case)), case.name


def test_finite_models_only():
    """No transition a model has is at probability zero, and no emission: -inf models are not this suite's."""
    for name in ec.MODELS + tuple(ec.SLOT_MODELS):
        om = ec.model_pair(name)[1]
        assert all(np.isfinite(om.tr[k].tP) for k in range(om.nTransitions)), name
        assert all(np.isfinite(v) for v in list(om.matchEm) + list(om.gapXEm) + list(om.gapYEm)), name
        assert len(ec.present_transitions(name)) == om.nTransitions == (13 if ec.n_states(name) == 5 else 9)
        assert len(ec.absent_transitions(name)) == (12 if ec.n_states(name) == 5 else 0)


def test_the_transposition_predicate_sees_a_transposition():
    T = np.array([[50.0, 7.0, 3.0], [6.0, 2.0, 1.0], [3.0, 1.0, 2.0]]).reshape(-1)
    E = np.concatenate([np.ones(16), np.arange(16.0), np.arange(16.0)])
    same = ec.Counts(T, E, -1.0)
    assert not ec.transposed_pairs_differ(same, "threeStateAsymmetric")  # gapX and gapY emissions equal
    E2 = E.copy()
    E2[32:48] *= 1.5
    assert ec.transposed_pairs_differ(ec.Counts(T, E2, -1.0), "threeStateAsymmetric")
    sym = T.reshape(3, 3)
    assert not ec.transposed_pairs_differ(ec.Counts(((sym + sym.T) / 2).reshape(-1), E2, -1.0), "threeStateAsymmetric")


# One long pair each, whose alignment begins and ends in the match state: the counts into and out of every gap state agree
# to 1 %.  The other batches of the team kind (501 and 509 cells, the short traceback schedule) do differ.
NOT_TRANSPOSED = ("expect-team8-fiveStateAsymmetric-0.01", "expect-team100-fiveStateAsymmetric-0.01")


@pytest.mark.parametrize("model", ec.ASYMMETRIC)
def test_asymmetric_models_give_counts_a_transposed_index_would_move(model):
    """In at least one problem per batch T[a * S + b] and T[b * S + a] differ by more than 1 % for some pair of states, and
    the sums over the X rows of the gapX and gapY emission blocks likewise: 1000 times the gate.  (Every gap opened inside
    the matrix is closed there too: the difference comes from alignments that begin or end in a gap state, which is what
    the overhangs of expect_cases._planted are for.)"""
    for kind, cases in ec.categories(model).items():
        for case in cases:
            differ = any(ec.transposed_pairs_differ(c, model) for c in ec.oracle_counts(case))
            assert differ == (case.name not in NOT_TRANSPOSED), case.name
        assert any(ec.transposed_pairs_differ(c, model) for _, _, c in _all_counts(cases)), kind
    # ... and in every problem drawn for it
    assert ec.well_covered(ec.oracle_counts(ec.widths_case(model))[ec.widths_indices(model, "planted")[-1]], model)


@pytest.mark.parametrize("model", ec.ASYMMETRIC)
def test_n_rich_problems_leave_a_tenth_of_the_events_out_of_the_emissions(model):
    """sum(T) - sum(E) is at least 10 % of sum(T) in every problem: a kernel that counts the emission at an N cell -- there
    is no slot for it, it would land in a neighbour's -- moves sum(E) by that much.  The transitions the models do not
    have are the elements the oracle leaves at exactly 0."""
    case = ec.n_rich_case(model)
    assert len(case.problems) == 8
    for (sx, sy, _, _, _), c in zip(case.problems, ec.oracle_counts(case)):
        both = sx + sy
        assert 0.12 <= sum(ch == "N" or ch.islower() for ch in both) / len(both) <= 0.30
        assert "N" in sx and "N" in sy and any(ch.islower() for ch in both)
        assert ec.n_share(c) >= ec.N_RICH_MIN_SHARE
        assert all(c.T[i] == 0.0 for i in ec.absent_transitions(model)) and all(c.T[i] > 0.0 for i in ec.present_transitions(model))
    assert {p[3:] for p in case.problems} == set(RAGGED)


def _widest(case, i):
    """The widest diagonal of problem i from the host's own band (api.band_construct); the problem is one rectangle."""
    sx, sy, a, rl, rr = case.problems[i]
    p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
    assert len(api.getSplitPoints(a, len(sx), len(sy), p.splitMatrixBiggerThanThis, rl, rr)) == 1, (case.name, i)
    band = api.band_construct(a, len(sx), len(sy), p.diagonalExpansion, dynamic=bool(p.dynamicAnchorExpansion))
    assert band == ob.band(a, len(sx), len(sy), p.diagonalExpansion, dynamic=bool(p.dynamicAnchorExpansion))
    return max((r - l) // 2 + 1 for _, l, r in band)


@pytest.mark.parametrize("model", ec.MODELS)
def test_widths_are_the_ones_the_problems_are_named_for(model):
    case, layout = ec.widths_case(model), ec.widths_layout(model)
    assert len(case.problems) == len(layout) == 14
    assert {p[3:] for p in case.problems} == set(RAGGED)
    named = set()
    for i, (kind, w) in enumerate(layout):
        got = _widest(case, i)
        if kind == "banded":  # several traceback segments; expansion 10 within one 64-lane group, 40 within two
            lo, hi = {10: (21, 64), 40: (81, 128)}[w]
            assert lo <= got <= hi, (kind, w, got)
            assert len(case.problems[i][0]) + len(case.problems[i][1]) > 1000
        else:
            assert got == w, (kind, w, got)
            named.add(w)
    assert {1, 5, 63, 64, 65, 127, 128, 129} <= named
    S = ec.states(model)
    assert {w for kind, w in layout if kind == "lds-edge"} == ({74, 75} if S == 5 else {121, 122})


def test_widths_at_the_lds_edges():
    """cpk_plan.inl's arithmetic: plan_expect_in_sweep keeps the in-traceback form while it leaves eight waves on a CU (20 KB
    each), plan_wide_class keeps the rows in LDS up to 64 KB less 16 bytes."""
    for S in (5, 3):
        last = ec.LAST_IN_TRACEBACK_WIDTH[S]
        for model in [m for m in ec.MODELS if ec.states(m) == S]:
            case = ec.widths_case(model)
            (sx0, sy0, *_), (sx1, sy1, *_) = (case.problems[i] for i in ec.widths_indices(model, "lds-edge"))
            assert (len(sx0), len(sx1)) == (last - 1, last) and min(len(sy0), len(sy1)) >= ec.LDS_EDGE_LY
            assert ec.in_sweep_lds_bytes(S, len(sx0), len(sy0)) <= ec.IN_SWEEP_MAX_BYTES < ec.in_sweep_lds_bytes(S, len(sx1), len(sy1))
        first = ec.FIRST_GLOBAL_LENGTH[S]
        assert ec.in_global_memory(S, first) and not ec.in_global_memory(S, first - 1)
    for model in ec.GLOBAL_MODELS:
        (n0, g0, c0), (n1, g1, c1) = ec.global_cases(model)
        assert (n1, g0, g1) == (n0 + 1, False, True)
        for n, c in ((n0, c0), (n1, c1)):
            assert (len(c.problems[0][0]), len(c.problems[0][1])) == (n, n) and _widest(c, 0) == n + 1


# Where raggedRight changes the end prior and nothing else the counts see: one base against one, and 65 against 65 bases of
# a pair that ends in aligned bases, under the five-state default model -- the posterior of ending in a gap state is 4e-6
# there.  The likelihood moves by 4 % and more all the same, and raggedLeft moves the counts at both sizes.
RIGHT_FLAG_MOVES_THE_LIKELIHOOD_ALONE = {("fiveState", (1, 1)), ("fiveState", (65, 65))}


@pytest.mark.parametrize("model", ec.EDGE_MODELS)
def test_the_four_ragged_combinations_give_different_counts(model):
    """Problems 4 k ... 4 k + 3 of the edges case are one pair under the four combinations: pairwise, their likelihoods
    differ by 1e5 times the gate and their transition counts by ten times the gate at the least (most by 100 to 1e5
    times), at every size and for every pair of combinations but the two named above, so a kernel that drops a flag fails."""
    case = ec.edges_case(model)
    counts = ec.oracle_counts(case)
    assert [(len(p[0]), len(p[1])) for p in case.problems[:32:4]] == list(ec.EDGE_SIZES)
    for k, size in enumerate(ec.EDGE_SIZES):
        group = range(4 * k, 4 * k + 4)
        assert len({case.problems[i][:2] for i in group}) == 1 and [case.problems[i][3:] for i in group] == RAGGED
        for i in group:
            for j in group:
                if i < j:
                    rel_t = np.abs(counts[i].T - counts[j].T).max() / max(counts[i].T.max(), counts[j].T.max())
                    rel_l = abs(counts[i].likelihood - counts[j].likelihood) / abs(counts[i].likelihood)
                    assert rel_l > 1e5 * ec.ORACLE_LIKELIHOOD_RTOL, (size, i, j, rel_l)
                    right_flag_only = case.problems[i][3] == case.problems[j][3]
                    if (model, size) in RIGHT_FLAG_MOVES_THE_LIKELIHOOD_ALONE and right_flag_only:
                        assert rel_t <= 10 * ec.ORACLE_RTOL, (size, i, j, rel_t)  # (an exception indeed)
                    else:
                        assert rel_t > 10 * ec.ORACLE_RTOL, (size, i, j, rel_t)
    # the degenerate problems: nothing at all for two empty sequences, gap states only for a one-sided one
    seen = 0
    for (sx, sy, _, _, _), c in zip(case.problems[32:], counts[32:]):
        if (sx, sy) == DEGENERATE[0]:
            assert not c.T.any() and not c.E.any() and c.likelihood == 0.0
        elif (sx, sy) in DEGENERATE[1:3]:
            S = ec.n_states(model)
            assert c.T.reshape(S, S)[0, 0] == 0.0 and c.T.sum() > 0 and not c.E.any()  # (row or column 0: an N cell)
        else:
            continue
        seen += 1
    assert seen == 12 and len(case.problems) == 64


def test_packed_batches_are_as_wide_as_their_groups():
    for model in ec.ASYMMETRIC:
        for lanes, case in ec.packed_cases(model):
            assert len(case.problems) == 19
            widest = 0
            for sx, sy, a, rl, rr in case.problems:
                if a:
                    band = ob.band(a, len(sx), len(sy), case.pkw["diagonalExpansion"])
                    widest = max(widest, max((r - l) // 2 + 1 for _, l, r in band))
            assert lanes // 2 < widest <= lanes or widest <= lanes == 8, (case.name, widest)


def test_oracle_counts_are_additive():
    """ob.expectations over a whole case into one accumulator equals the sum of oracle_counts to 1e-12 relative: the pooled
    comparisons of the packed and slot tests may use either."""
    done = 0
    for case in ec.all_cases():
        if len(case.problems) < 2:
            continue
        acc = ob.hmm(ec.model_type(case.model), 0.0)
        om, op = ec.model_pair(case.model)[1], ob.params(**case.pkw)
        for sx, sy, a, rl, rr in case.problems:
            ob.expectations(om, acc, sx, sy, a, op, rl, rr)
        want = ec.pooled(ec.oracle_counts(case))
        S = ec.n_states(case.model)
        np.testing.assert_allclose(np.array(acc.T[:S * S]), want.T, rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.array(acc.E[:S * 16]), want.E, rtol=1e-12, atol=0)
        np.testing.assert_allclose(acc.likelihood, want.likelihood, rtol=1e-12, atol=0)
        done += 1
    assert done >= 40


def test_case_names_are_unique_and_counts_read_only():
    cases = ec.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    c = ec.oracle_counts(cases[0])[1]
    with pytest.raises(ValueError):
        c.T[0] = 1.0
    assert ec.oracle_counts(cases[0]) is ec.oracle_counts(cases[0])
