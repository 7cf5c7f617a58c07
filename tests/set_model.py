"""The sets layer's host logic in plain Python (include/cpecan_sets.h): which pairs of a set the reference aligns
(impl/multipleAligner.c:668-681 and :722-770) and its similarity score (:604-619).  No library, no GPU.

A fragment is (set_id, length, leftEndId, rightEndId); its global index is its place in the list."""
import struct

PROB_1 = 10000000
ALL, REFERENCE = 0, 1


def _sets_in_order(frags):
    """[(members ascending)] of every set, the sets by the global index of their first fragment."""
    groups = {}
    for i, f in enumerate(frags):
        groups.setdefault(f[0], []).append(i)
    return sorted(groups.values(), key=lambda m: m[0])


def _star(l, i, j, chosen):
    """getReferencePairwiseAlignmentsP (:722-733): l[(i + j) // 2] pairs with every other element of l[i:j]."""
    ref = l[(i + j) // 2]
    for t in l[i:j]:
        if t[2] != ref[2]:
            chosen.append((min(ref[2], t[2]), max(ref[2], t[2])))
    return ref


def reference_pairs_of_set(frags, members):
    """getReferencePairwiseAlignments (:735-770) on the fragments `members`, sorted as makeAlignment iterates them."""
    if not members:
        return []
    l = sorted((frags[m][3], frags[m][1], m) for m in members)  # (rightEndId, length, index), :746-750
    chosen, refs, i = [], [], 0
    for j in range(1, len(l) + 1):
        if j == len(l) or l[j][0] != l[i][0]:
            refs.append(_star(l, i, j, chosen))
            i = j
    _star(refs, 0, len(refs), chosen)  # :765
    assert len(chosen) == len(members) - 1  # :768
    return sorted(chosen)


def pairs(frags, mode):
    out = []
    for members in _sets_in_order(frags):
        if mode == ALL:
            out += [(a, b) for k, a in enumerate(members) for b in members[k + 1:]]
        else:
            out += reference_pairs_of_set(frags, members)
    return out


def _f64(v):
    """An int64 converted to double as C converts it (round to nearest even); exact below 2^53."""
    return struct.unpack("d", struct.pack("d", float(v)))[0]


def similarity_score(score_sum, lX, lY):
    """getAlignmentScore (:613-618) from the sum of the scores."""
    j = min(lX, lY)
    j = 1 if j == 0 else j
    d = _f64(score_sum) / _f64(j * PROB_1)
    d = 1.0 if d > 1.0 else d
    d = 0.0 if d < 0.0 else d
    return int(d * PROB_1)  # truncation towards zero
