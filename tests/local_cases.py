"""Inputs of the local-chain tests: small pairs, each there for one rule of the definition.
A case is a dict: problems [(sX, sY)], strand, K (maxChains), S (minChainScore), trim, params (overrides of
anchor_model.default_params), seedTransitions, threshold (transitionHspThreshold).  model(case) is the model's answer,
computed once per process and shared by every test that needs it."""
import random

import anchor_model as am
import local_model as lm
import strand_model as sm

_OTHER = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, sub=0.10, indel_every=0):
    """Substitutions at rate `sub`; with indel_every, a one-base deletion or insertion about every so many bases."""
    out = []
    for i, ch in enumerate(s):
        if indel_every and i % indel_every == indel_every - 1:
            if rng.random() < 0.5:
                continue
            out.append(rng.choice("ACGT"))
        out.append(rng.choice(_OTHER[ch]) if rng.random() < sub else ch)
    return "".join(out)


def rc(s):
    return sm.rc(s).decode()


def _case(name, problems, strand="both", K=4, S=0, trim=0, params=None, seedTransitions=0, threshold=0):
    return dict(name=name, problems=problems, strand=strand, K=K, S=S, trim=trim, params=params or {},
                seedTransitions=seedTransitions, threshold=threshold)


SEG = 1200
_rng = random.Random(20240607)
A, B, Cc = (rand_seq(_rng, SEG) for _ in range(3))
INVERSION_X = A + B + Cc
INVERSION_Y = mutate(_rng, A) + rc(mutate(_rng, B)) + mutate(_rng, Cc)
TRANSPOSITION_X = A + B
TRANSPOSITION_Y = mutate(_rng, B) + mutate(_rng, A)
TIE_S = rand_seq(_rng, 900)
UNRELATED = (rand_seq(_rng, 1500), rand_seq(_rng, 1400))

# pool sizes: a short seed, a low threshold and an x-drop under one mismatch cut the diagonals into many short HSPs, and an
# indel every ~100 bases spreads them over neighbouring diagonals.  The plus pools hold fewer than 64, 65 .. 256 and more than
# 256 HSPs (tests/test_local_cases_cpu.py holds that): under one wave, under the workgroup's stride of 256, beyond it.
POOL_PARAMS = dict(seed="11111111", maxSeedOccurrences=3, xDrop=60, hspThreshold=700)


def _pool_pair(n):
    rng = random.Random(n)
    x = rand_seq(rng, n)
    return x, mutate(rng, x, sub=0.10, indel_every=100)


POOL_PAIRS = [_pool_pair(500), _pool_pair(1500), _pool_pair(5000)]


def _batch_problems():
    rng = random.Random(4242)
    out = []
    for i in range(300):
        if i == 17:
            out.append(("", rand_seq(rng, 200)))
        elif i == 101:
            out.append((rand_seq(rng, 12), rand_seq(rng, 300)))          # shorter than the seed's span
        else:
            a, b = rand_seq(rng, 150 + rng.randrange(120)), rand_seq(rng, 150 + rng.randrange(120))
            kind = i % 3
            y = mutate(rng, a, 0.08) + (rc(mutate(rng, b, 0.08)) if kind == 0 else mutate(rng, b, 0.08))
            if kind == 2:
                y = mutate(rng, b, 0.08) + mutate(rng, a, 0.08)
            out.append((a + b, y))
    return out


CAP_MAX_HSPS = 6
# With the default x-drop a segment of 1.2 kb at 10 % substitutions is ONE HSP, which runs a few chance matches into its
# neighbour, and the kill rule then removes the whole inverted segment with it.  A smaller x-drop cuts every segment into
# several HSPs: the one at the junction dies, the rest of the segment chains.
SEGMENT_PARAMS = dict(xDrop=150)


def inversion(params=None, **kw):
    return _case("inversion", [(INVERSION_X, INVERSION_Y)], params=dict(SEGMENT_PARAMS, **(params or {})), **kw)


def cases():
    """Every single-call case but the threshold one, which needs the model's scores (threshold_case)."""
    return [
        inversion(),
        _case("transposition", [(TRANSPOSITION_X, TRANSPOSITION_Y)], strand="plus", params=SEGMENT_PARAMS),
        _case("tie", [(TIE_S, TIE_S + rc(TIE_S))]),
        _case("nothing", [UNRELATED]),
        _case("short", [("ACGTACGTAC", INVERSION_Y[:500])]),
        _case("empty", [("", INVERSION_Y[:300]), (INVERSION_X[:300], "")]),
        dict(inversion(K=1), name="k_cut"),
        dict(inversion(params=dict(maxHsps=CAP_MAX_HSPS)), name="cap"),
        _case("pool_sizes", POOL_PAIRS, K=4, params=POOL_PARAMS),
        dict(inversion(trim=trim_of_trim_case()), name="trim"),
        dict(inversion(seedTransitions=1, threshold=1200), name="transitions"),
        dict(inversion(strand="minus"), name="minus_only"),
    ]


def batch_case():
    return _case("batch", _batch_problems(), K=16)


_models = {}


def model(case):
    """[(chains, statistics)] per problem of the case, from tests/local_model.py; computed once."""
    key = (case["name"], case["K"], case["S"], case["trim"], case["strand"])
    if key not in _models:
        params = am.default_params(**case["params"])
        _models[key] = [lm.local_chains(x, y, case["strand"], case["K"], case["S"], case["trim"], 20, params,
                                        case["seedTransitions"], case["threshold"]) for x, y in case["problems"]]
    return _models[key]


def threshold_case():
    """S between the model's first and second chain score on the inversion: the second round ends the call."""
    chains, _ = model(inversion())[0]
    first, second = chains[0]["score"], chains[1]["score"]
    assert first > second + 1
    return dict(inversion(S=second + (first - second) // 2), name="threshold")


def by_name(name):
    if name == "threshold":
        return threshold_case()
    if name == "batch":
        return batch_case()
    return next(c for c in cases() if c["name"] == name)


NAMES = ["inversion", "transposition", "tie", "nothing", "short", "empty", "k_cut", "cap", "pool_sizes", "trim", "transitions",
         "minus_only", "threshold"]


def trim_of_trim_case():
    """A trim that removes every run of one chain of the `trim` case and leaves runs in another: half the longest HSP of the
    model's shortest-HSP chain, found on the model."""
    chains, _ = model(inversion())[0]
    longest = sorted(max(h[2] for h in c["hsps"]) for c in chains)
    return (longest[0] + 1) // 2
