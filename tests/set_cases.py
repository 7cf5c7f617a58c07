"""Inputs of the GPU tests of the sets layer (tests/test_gpu_sets.py), with the property each of them is there for.
tests/test_set_cases_cpu.py asserts those properties with the oracle, so a case cannot quietly stop being the case it
is meant to be.  Seeded: the same fragments everywhere.

A case: name, gapGamma, frags [(set_id, seq, leftEndId, rightEndId)], pairs ("all" | "reference" | explicit list)."""
import random

import numpy as np

import oracle_binding as ob
import set_model as sm


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s, sub, indel):
    out = []
    for ch in s:
        r = rng.random()
        if r < sub:
            out.append(rng.choice([b for b in "ACGT" if b != ch]))
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out.append(ch)
            out.append(rng.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


def _case_a():
    rng = random.Random(101)
    root = _seq(rng, 14)
    frags = []
    for i in range(26):
        n = 0 if i == 7 else rng.randrange(8, 15)
        frags.append((0, _mutate(rng, root, 0.15, 0.0)[:n], i % 2, i % 3))
    return dict(name="a", gapGamma=0.5, frags=frags, pairs="all")


def _two(seed, n, sub, indel, gamma, name, left=(0, 0), right=(0, 0)):
    rng = random.Random(seed)
    x = _seq(rng, n)
    return dict(name=name, gapGamma=gamma, frags=[(0, x, left[0], right[0]), (0, _mutate(rng, x, sub, indel), left[1], right[1])],
                pairs="all")


def _case_d():
    rng = random.Random(104)
    root = _seq(rng, 40)
    return dict(name="d", gapGamma=0.0, frags=[(3, _mutate(rng, root, 0.1, 0.04), 0, k % 2) for k in range(3)], pairs="all")


def _case_e():
    rng = random.Random(105)
    root = _seq(rng, 30)
    m = lambda: _mutate(rng, root, 0.1, 0.05)
    # sets 30 (four fragments), 10 (two), 20 (one), interleaved.  Set 10's pair has both ends in common; in set 30 pair
    # (0, 3) is ragged on the right, (0, 4) on the left and (0, 6) on both
    frags = [(30, m(), 1, 1), (10, m(), 7, 7), (20, m(), 0, 0), (30, m(), 1, 2), (30, m(), 2, 1), (10, m(), 7, 7), (30, m(), 2, 2)]
    return dict(name="e", gapGamma=0.5, frags=frags, pairs="all")


def _case_g():
    rng = random.Random(107)
    x = _seq(rng, 50)
    return dict(name="g", gapGamma=0.5, frags=[(0, x, 0, 0), (0, _mutate(rng, x[8:43], 0.08, 0.04), 1, 0)], pairs=[(1, 0)])


CASES = [
    _case_a(),                                # 325 problems: past one 256-wide block of problems; one fragment of length 0
    _two(102, 300, 0.03, 0.01, 0.5, "b"),     # a list of more than 256 triples whose sum is above 2^31
    _two(116, 60, 0.30, 0.10, 5.0, "c"),      # a negative sum (below -2^31 even): similarity 0
    _case_d(),                                # gapGamma 0: not reweighted, the stage still runs
    _case_e(),                                # interleaved sets, every ragged combination
    _two(106, 600, 0.05, 0.0, 0.5, "f"),      # lX * lY > 250000: the anchor finder is on the path
    _case_g(),                                # X = b, Y = a with b > a, as given
]
BY_NAME = {c["name"]: c for c in CASES}


def model_frags(case):
    return [(s, len(seq), left, right) for s, seq, left, right in case["frags"]]


def chosen_pairs(case, mode=None):
    """The pairs of the case (or of `mode`, "all" / "reference") as tests/set_model.py chooses them."""
    mode = mode or case["pairs"]
    if not isinstance(mode, str):
        return [tuple(p) for p in mode]
    return sm.pairs(model_frags(case), sm.ALL if mode == "all" else sm.REFERENCE)


def problems(case, pairs=None):
    """(sX, sY, raggedLeft, raggedRight) of every pair: X = a, Y = b as given (impl/multipleAligner.c:658-661)."""
    f = case["frags"]
    return [(f[a][1], f[b][1], f[a][2] != f[b][2], f[a][3] != f[b][3]) for a, b in (pairs if pairs is not None else chosen_pairs(case))]


_oracle = {}


def oracle_lists(case, pairs=None, anchors=None):
    """Per pair (plain, reweighted): oracle.aligned_pairs and reweight_aligned_pairs of it, int64[n, 3].  anchors: one
    anchor list per pair, or None for none.  Computed once per (case, pairs) and shared; callers must not write to it."""
    pairs = pairs if pairs is not None else chosen_pairs(case)
    key = (case["name"], tuple(pairs), anchors is not None)
    if key not in _oracle:
        out = []
        for k, (sx, sy, rl, rr) in enumerate(problems(case, pairs)):
            plain = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors[k] if anchors is not None else (), ob.params(), rl, rr)
            plain = np.asarray(plain, dtype=np.int64).reshape(-1, 3)
            out.append((plain, ob.reweight_aligned_pairs(plain, len(sx), len(sy), case["gapGamma"]).reshape(-1, 3)))
        _oracle[key] = out
    return _oracle[key]
