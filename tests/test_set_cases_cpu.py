"""The inputs of tests/test_gpu_sets.py are what they are meant to be: every case of tests/set_cases.py has the property it
is in the suite for, asserted with the oracle on the CPU."""
import numpy as np

import set_cases as sc
import set_model as sm
from cpecan_amd import api, sets


def _sums(case):
    return [int(rew[:, 0].sum()) for _, rew in sc.oracle_lists(case)]


def test_the_cases_are_the_seven():
    assert [c["name"] for c in sc.CASES] == list("abcdefg")
    for c in sc.CASES:
        assert float(np.float32(c["gapGamma"])) == c["gapGamma"]  # the float of the options is the double of the oracle


def test_library_chooses_the_pairs_of_every_case():
    """cpecan_sets_pairs on the real fragments, both modes, against the model: host code, no GPU."""
    for c in sc.CASES:
        with sets.Sets(api.stateMachine5_construct(), gapGamma=c["gapGamma"]) as s:
            for i, (set_id, seq, left, right) in enumerate(c["frags"]):
                assert s.add_fragment(set_id, seq, left, right) == i
            for mode, name in ((sets.ALL, "all"), (sets.REFERENCE, "reference")):
                assert [tuple(p) for p in s.pairs(mode).tolist()] == sc.chosen_pairs(c, name)


def test_case_a_is_more_than_one_block_of_problems():
    c = sc.BY_NAME["a"]
    lengths = [len(f[1]) for f in c["frags"]]
    assert len(lengths) == 26 and lengths.count(0) == 1 and all(8 <= n <= 14 for n in lengths if n)
    assert len({f[0] for f in c["frags"]}) == 1
    pairs = sc.chosen_pairs(c)
    assert len(pairs) == 325 > 256
    lists = sc.oracle_lists(c)
    empty = [k for k, (a, b) in enumerate(pairs) if 7 in (a, b)]
    assert len(empty) == 25 and all(len(lists[k][1]) == 0 for k in empty)  # nothing aligns to the empty fragment
    assert sum(len(rew) > 0 for _, rew in lists) >= 256  # and the other lists are not empty


def test_case_b_sums_past_32_bits_in_a_long_list():
    c = sc.BY_NAME["b"]
    assert len(c["frags"][0][1]) == 300 and len(sc.chosen_pairs(c)) == 1
    (plain, rew), = sc.oracle_lists(c)
    assert len(rew) > 256
    total = _sums(c)[0]
    assert total > 2 ** 31 and int(rew[:, 0].astype(np.int32).sum(dtype=np.int32)) != total  # 32 bits would wrap
    lX, lY = (len(f[1]) for f in c["frags"])
    assert 0 < sm.similarity_score(total, lX, lY) < sm.PROB_1


def test_case_c_has_a_negative_sum():
    c = sc.BY_NAME["c"]
    assert c["gapGamma"] == 5.0 and len(c["frags"][0][1]) == 60
    (plain, rew), = sc.oracle_lists(c)
    total = _sums(c)[0]
    assert len(rew) > 0 and total < -2 ** 31
    lX, lY = (len(f[1]) for f in c["frags"])
    assert sm.similarity_score(total, lX, lY) == 0


def test_case_d_is_not_reweighted():
    c = sc.BY_NAME["d"]
    assert c["gapGamma"] == 0.0 and len(sc.chosen_pairs(c)) == 3
    for plain, rew in sc.oracle_lists(c):
        assert len(plain) > 0 and (plain == rew).all()


def test_case_e_has_interleaved_sets_and_every_ragged_combination():
    c = sc.BY_NAME["e"]
    ids = [f[0] for f in c["frags"]]
    sizes = sorted(ids.count(i) for i in set(ids))
    assert sizes == [1, 2, 4]
    assert any(ids[i] != ids[i + 1] and ids[i] in ids[i + 2:] for i in range(len(ids) - 2))  # a set comes back after another
    assert {(rl, rr) for _, _, rl, rr in sc.problems(c)} == {(False, False), (False, True), (True, False), (True, True)}
    assert len(sc.chosen_pairs(c)) == 0 + 1 + 6 and len(sc.chosen_pairs(c, "reference")) == 0 + 1 + 3
    # the ragged flags matter to the result: the same two sequences with the flags cleared give another list
    import oracle_binding as ob
    changed = 0
    for (sx, sy, rl, rr), (plain, _) in zip(sc.problems(c), sc.oracle_lists(c)):
        if rl or rr:
            other = np.asarray(ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, (), ob.params(), False, False)).reshape(-1, 3)
            changed += other.shape != plain.shape or not (other == plain).all()
    assert changed > 0


def test_case_f_is_past_the_anchor_threshold():
    c = sc.BY_NAME["f"]
    lX, lY = (len(f[1]) for f in c["frags"])
    assert lX * lY > api.ANCHOR_MATRIX_BIGGER_THAN_THIS == 250000 and 550 <= min(lX, lY)


def test_case_g_is_given_backwards():
    c = sc.BY_NAME["g"]
    assert c["pairs"] == [(1, 0)] and sc.chosen_pairs(c, "all") == [(0, 1)]
    (sx, sy, rl, rr), = sc.problems(c)
    assert sx == c["frags"][1][1] and sy == c["frags"][0][1] and len(sx) != len(sy) and (rl, rr) == (True, False)
    (plain, rew), = sc.oracle_lists(c)
    (fplain, frew), = sc.oracle_lists(c, [(0, 1)])
    # X and Y swapped is another list, not the same list with the columns exchanged read in the same order
    assert len(rew) > 0 and rew[:, [0, 2, 1]].tolist() != frew.tolist()
