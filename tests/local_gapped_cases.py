"""Inputs of the tests of local chains with gapped extension: pairs of 1-1.5 kb built as
tests/local_cases.py builds its own, each there for one edge of the rule.  A case is a local_cases case with three keys
more -- gapped, yDrop, maxDiagonals, as cpecan_anchor_options holds them -- and model(case) is the answer of
tests/local_model_gapped.py, computed once per process.  What each case must show on the model is asserted in
tests/test_local_gapped_cases_cpu.py."""
import random

import anchor_model as am
import local_cases as lc
import local_model_gapped as lmg

SEG = 400
SUB = 0.06
PARAMS = dict(xDrop=150)


def mutate(rng, s, sub=SUB):
    """Substitutions at rate `sub`, and a 2-base deletion 45 bases from either end and every 130 bases."""
    out = [rng.choice(lc._OTHER[ch]) if rng.random() < sub else ch for ch in s]
    cuts = sorted(set([45, len(s) - 47] + list(range(130, len(s) - 47, 130))), reverse=True)
    for at in cuts:
        del out[at:at + 2]
    return "".join(out)


def _case(name, problems, strand="both", K=4, trim=0, params=None, gapped=1, yDrop=0, maxDiagonals=0):
    return dict(lc._case(name, problems, strand=strand, K=K, trim=trim, params=dict(PARAMS, **(params or {}))), gapped=gapped,
                yDrop=yDrop, maxDiagonals=maxDiagonals)


def _segments(seed):
    rng = random.Random(seed)
    return rng, [lc.rand_seq(rng, SEG) for _ in range(3)]


def inversion_pair(seed=1):
    rng, (a, b, c) = _segments(seed)
    return a + b + c, mutate(rng, a) + lc.rc(mutate(rng, b)) + mutate(rng, c)


def transposition_pair(seed=1):
    rng, (a, b, c) = _segments(seed)
    return a + b + c, mutate(rng, b) + mutate(rng, c) + mutate(rng, a)


def shared_middle_pair(seed=5):
    """X = A + M + B; Y = M' + B'[2:] + J + A' + M', M' being M without bases 20-21: both A and B can grow into M on X."""
    rng = random.Random(seed)
    a, m, b, j = lc.rand_seq(rng, 500), lc.rand_seq(rng, 40), lc.rand_seq(rng, 300), lc.rand_seq(rng, 200)
    m2 = m[:20] + m[22:]
    return a + m + b, m2 + lc.mutate(rng, b, 0.05)[2:] + j + lc.mutate(rng, a, 0.05) + m2


def end_gap_pairs(seed=3):
    """The homology in the middle of both sequences; and a pair that is homologous to both ends, with an indel near each."""
    rng = random.Random(seed)
    h, g = lc.rand_seq(rng, 600), lc.rand_seq(rng, 500)
    h2 = mutate(rng, h)
    h2 = h2[:16] + h2[18:-18] + h2[-16:]                     # no seed fits between an end of the homology and its first indel
    inner = (lc.rand_seq(rng, 150) + h + lc.rand_seq(rng, 170), lc.rand_seq(rng, 120) + h2 + lc.rand_seq(rng, 140))
    g2 = lc.mutate(rng, g, SUB)
    return [inner, (g, g2[:30] + g2[32:460] + g2[462:])]


def narrow_pair(seed=1):
    """A stretch with a 2-base deletion every 15 bases, where no seed fits and the extension has far to walk; near its upper
    end a 20-base deletion, which costs more than the y-drop of the case, with a dozen columns behind it."""
    rng = random.Random(seed)
    h = lc.rand_seq(rng, 1000)
    y = list(lc.mutate(rng, h, 0.04))
    for at in [482, 450] + list(range(435, 290, -15)):
        del y[at:at + (20 if at == 450 else 2)]
    return h, "".join(y)


def _batch_problems():
    rng = random.Random(777)
    out = []
    for i in range(300):
        if i == 17:
            out.append(("", lc.rand_seq(rng, 200)))
        elif i == 101:
            out.append((lc.rand_seq(rng, 12), lc.rand_seq(rng, 300)))       # shorter than the seed's span
        else:
            a, b = lc.rand_seq(rng, 150 + rng.randrange(100)), lc.rand_seq(rng, 150 + rng.randrange(100))
            kind = i % 3
            a2, b2 = lc.mutate(rng, a, 0.08, 60), lc.mutate(rng, b, 0.08, 60)
            y = a2 + (lc.rc(b2) if kind == 0 else b2)
            if kind == 2:
                y = b2 + a2
            out.append((a + b, y))
    return out


BATCH_TRIM = 29                     # twice it is the longest block of the shortest chains: they keep no run


def cases():
    return [
        _case("inversion", [inversion_pair()]),
        _case("transposition", [transposition_pair()], strand="plus"),
        _case("shared_middle", [shared_middle_pair()], strand="plus"),
        _case("end_gaps", end_gap_pairs(), strand="plus", K=2),
        _case("narrow", [narrow_pair()], strand="plus", K=2, yDrop=600, maxDiagonals=64),
        _case("one_chain", [inversion_pair(), transposition_pair()], strand="plus", K=1),
        _case("off", [inversion_pair()], gapped=0),
    ]


def batch_case():
    return _case("batch", _batch_problems(), K=16, trim=BATCH_TRIM)


NAMES = ["inversion", "transposition", "shared_middle", "end_gaps", "narrow", "one_chain", "off"]


def by_name(name):
    if name == "batch":
        return batch_case()
    return next(c for c in cases() if c["name"] == name)


_models = {}


def model_of(case, sx, sy, **kw):
    params = am.default_params(**case["params"])
    return lmg.local_chains(sx, sy, case["strand"], case["K"], case["S"], case["trim"], 20, params, case["seedTransitions"],
                            case["threshold"], case["gapped"], case["yDrop"], case["maxDiagonals"], **kw)


def model(case):
    """[(chains, statistics)] per problem of the case, from tests/local_model_gapped.py; computed once."""
    key = (case["name"], case["K"], case["trim"], case["strand"], case["gapped"])
    if key not in _models:
        _models[key] = [model_of(case, x, y) for x, y in case["problems"]]
    return _models[key]
