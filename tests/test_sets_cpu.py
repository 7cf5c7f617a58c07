"""CPU-side checks of the sets layer (include/cpecan_sets.h): the choice of pairs and the similarity score against
tests/set_model.py on hand-worked and random sets, the argument checks, and the header against sets.EXPORTS.  Nothing here
needs a GPU; cpecan_sets_align must say so when there is none."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import set_model as sm
from cpecan_amd import api, sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _object(frags, device=0):
    """frags: (set_id, length, leftEndId, rightEndId); the bases do not matter to the choice of pairs."""
    s = sets.Sets(api.stateMachine5_construct(), device=device)
    for i, (set_id, length, left, right) in enumerate(frags):
        assert s.add_fragment(set_id, "A" * length, left, right) == i
    return s


def _both(frags, mode):
    with _object(frags) as s:
        got = [tuple(r) for r in s.pairs(mode).tolist()]
    assert got == sm.pairs(frags, mode)
    return got


def test_header_declares_what_the_module_exports():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpecan_sets.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpecan_[a-z_0-9]+)\s*\(", header))
    L = api.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert declared == set(sets.EXPORTS)
    # the new declarations stay out of cpecan_hip.h, whose every `cpecan_xxx(` is an export of api.EXPORTS
    assert not set(sets.EXPORTS) & set(api.EXPORTS)


def test_options_defaults():
    o = sets.sets_options()
    assert (o.gapGamma, o.constraintDiagonalTrim, o.anchorMatrixBiggerThanThis, o.repeatMaskMatrixBiggerThanThis) == \
        (0.5, 14, 250000, 250000)


def test_pairs_hand_worked():
    assert _both([], sm.ALL) == [] and _both([], sm.REFERENCE) == []
    assert _both([(0, 5, 1, 2)], sm.ALL) == [] and _both([(0, 5, 1, 2)], sm.REFERENCE) == []
    # one rightEndId: sorted by length the indices are 1 3 0 4 2; the median, place (0 + 5) / 2 = 2, is fragment 0: a star on it
    star = [(0, 30, 0, 7), (0, 10, 0, 7), (0, 50, 0, 7), (0, 20, 0, 7), (0, 40, 0, 7)]
    assert _both(star, sm.REFERENCE) == [(0, 1), (0, 2), (0, 3), (0, 4)]
    assert _both(star, sm.ALL) == [(a, b) for a in range(5) for b in range(a + 1, 5)]
    # two runs.  Sorted: (1,5,#1) (1,9,#3) | (2,8,#2) (2,10,#0) (2,12,#4); references #3 (place 1) and #0 (place 3); of the two
    # references [#3, #0] place 1 is #0: the link (0, 3)
    two = [(0, 10, 0, 2), (0, 5, 0, 1), (0, 8, 0, 2), (0, 9, 0, 1), (0, 12, 0, 2)]
    assert _both(two, sm.REFERENCE) == [(0, 2), (0, 3), (0, 4), (1, 3)]
    # three runs.  Sorted: (1,4,#1) (1,6,#3) | (2,1,#5) (2,4,#2) | (3,2,#4) (3,4,#0); references #3, #2, #0; the median of
    # those three is #2: links (2, 3) and (0, 2)
    three = [(0, 4, 0, 3), (0, 4, 0, 1), (0, 4, 0, 2), (0, 6, 0, 1), (0, 2, 0, 3), (0, 1, 0, 2)]
    assert _both(three, sm.REFERENCE) == [(0, 2), (0, 4), (1, 3), (2, 3), (2, 5)]
    # equal lengths: the index breaks the tie, place (0 + 4) / 2 = 2 is fragment 2
    assert _both([(0, 10, 0, 0)] * 4, sm.REFERENCE) == [(0, 2), (1, 2), (2, 3)]
    # three interleaved sets, 9 = {0, 2, 5}, 4 = {1, 4}, 7 = {3}: sets in the order of their first fragment
    inter = [(9, 5, 0, 0), (4, 5, 0, 0), (9, 6, 0, 0), (7, 5, 0, 0), (4, 4, 0, 0), (9, 7, 0, 0)]
    assert _both(inter, sm.ALL) == [(0, 2), (0, 5), (2, 5), (1, 4)]
    assert _both(inter, sm.REFERENCE) == [(0, 2), (2, 5), (1, 4)]
    # negative and large ids are ids like any other
    assert _both([(-3, 1, 0, -5), (2 ** 40, 1, 0, 0), (-3, 2, 0, 2 ** 40)], sm.REFERENCE) == [(0, 2)]


def test_pairs_random_sets():
    rng = random.Random(2024)
    n_sets = 0
    for trial in range(40):
        sizes = [rng.randrange(1, 13) for _ in range(5)]
        n_sets += len(sizes)
        tags = [k for k, size in enumerate(sizes) for _ in range(size)]
        rng.shuffle(tags)  # interleaved
        ids = [rng.randrange(-50, 50) * 5 + k for k in range(5)]  # distinct set ids in no particular order
        frags = [(ids[k], rng.randrange(0, 6), rng.randrange(3), rng.randrange(4)) for k in tags]
        members = {}
        for i, f in enumerate(frags):
            members.setdefault(f[0], []).append(i)
        assert len(_both(frags, sm.ALL)) == sum(len(m) * (len(m) - 1) // 2 for m in members.values())
        got = _both(frags, sm.REFERENCE)
        at = 0
        for m in sorted(members.values(), key=lambda m: m[0]):
            mine = got[at:at + len(m) - 1]  # n - 1 pairs
            at += len(m) - 1
            assert mine == sorted(mine) and all(a < b and a in m and b in m for a, b in mine)
            reach, grew = {m[0]}, True  # connected: n - 1 edges that reach every member are a spanning tree
            while grew:
                grew = False
                for a, b in mine:
                    if (a in reach) != (b in reach):
                        reach |= {a, b}
                        grew = True
            assert reach == set(m)
        assert at == len(got)
    assert n_sets == 200


def test_pairs_cap_contract():
    frags = [(0, 3, 0, 0)] * 5
    with _object(frags) as s:
        L = api.lib()
        full = s.pairs(sm.ALL)
        assert len(full) == 10
        buf = np.full((10, 2), -7, dtype=np.int64)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_int64))
        assert L.cpecan_sets_pairs(s._h, sm.ALL, ptr, 3) == 10  # the count there are, whatever the room
        assert buf[:3].tolist() == full[:3].tolist() and (buf[3:] == -7).all()
        assert L.cpecan_sets_pairs(s._h, sm.ALL, None, 0) == 10
        assert L.cpecan_sets_pairs(s._h, sm.ALL, ptr, 100) == 10 and buf.tolist() == full.tolist()
        assert s.pairs(sm.ALL, cap=4).tolist() == full[:4].tolist()
        assert L.cpecan_sets_pairs(s._h, 2, ptr, 10) == -1 and L.cpecan_sets_pairs(s._h, sm.ALL, ptr, -1) == -1


def test_similarity_score():
    P = sm.PROB_1
    cases = [(0, 0, 0), (5 * P, 0, 7), (P // 2, 0, 0),  # j == 0 counts as 1
             (-1, 10, 10), (-3 * 10 ** 12, 5, 9),  # a negative sum: 0
             (10 * P + 1, 10, 12), (2 ** 62, 300, 300),  # above j * 1e7: 1e7
             (10 * P, 10, 10), (10 * P - 1, 10, 10), (2900000123, 300, 310), (1, 3, 3), (29, 3, 4), (31, 4, 3),  # truncation
             (2 ** 31, 300, 300), (2 ** 31 + 12345, 215, 300)]
    rng = random.Random(5)
    cases += [(rng.randrange(-10 ** 9, 4 * 10 ** 10), rng.randrange(0, 4000), rng.randrange(0, 4000)) for _ in range(2000)]
    for total, lX, lY in cases:
        assert api.similarity_score(total, lX, lY) == sm.similarity_score(total, lX, lY), (total, lX, lY)
    assert api.similarity_score(5 * P, 0, 7) == P and api.similarity_score(P // 2, 0, 0) == P // 2
    assert api.similarity_score(-1, 10, 10) == 0 and api.similarity_score(10 * P + 1, 10, 12) == P
    assert api.similarity_score(10 * P - 1, 10, 10) == 9999999  # 0.99999999 * 1e7 = 9999999.9, truncated
    assert api.similarity_score(29, 3, 4) == 9 and api.similarity_score(31, 4, 3) == 10  # 29 / 3 = 9.67, 31 / 3 = 10.3
    assert api.lib().cpecan_similarity_score(1, -1, 3) == -1


def test_align_refuses_bad_pairs_before_it_looks_for_a_device():
    frags = [(0, 4, 0, 0), (0, 4, 0, 0), (1, 4, 0, 0)]
    for device in (0, 1000):  # 1000: no such device anywhere, and still the answer is EINVAL
        with _object(frags, device) as s:
            for bad, what in (([(1, 1)], "itself"), ([(0, 2)], "different sets"), ([(0, 3)], "names fragment"),
                              ([(-1, 0)], "names fragment"), ([(0, 1), (2, 0)], "different sets")):
                with pytest.raises(api.CpecanError, match=r"\(-1\).*" + what):
                    s.align(bad)


def test_align_needs_a_device():
    frags = [(0, 4, 0, 0), (0, 4, 0, 0)]
    with _object(frags, 1000) as s:
        with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
            s.align([(0, 1)])
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):
            s.align([])  # even an empty call does not pretend it ran
    if api.device_count() == 0:
        with _object(frags) as s:
            with pytest.raises(api.CpecanError, match=r"\(-2\).*no usable HIP device"):
                s.align(s.pairs(sm.ALL))


def test_batch_switch_argument_checks():
    """cpecan_batch_set_quintuples on a batch: host-side state only."""
    with api.Batch(api.stateMachine5_construct()) as b:
        b.add("ACGT", "ACGT")
        b.add("ACGT", "AGT")
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            sets.batch_set_quintuples(b, [(0, 1)])  # one pair of names for two problems
        sets.batch_set_quintuples(b, [(0, 1), (0, 2)])
        sets.batch_set_quintuples(b, None)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            sets.batch_quintuples(b)  # nothing was downloaded
    with api.Batch(api.stateMachine5_construct(), emit=api.EMIT_FORWARD) as b:
        b.add("ACGT", "ACGT")
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            sets.batch_set_quintuples(b, [(0, 1)])
