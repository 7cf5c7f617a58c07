"""The local-chain cases (tests/local_cases.py) on the model (tests/local_model.py), no GPU: every case is there for the
rule its name says, and the consequences of the definition (point 5) hold on every case and on
100 random pairs."""
import random

import numpy as np

import anchor_model as am
import local_cases as lc
import local_model as lm
import strand_model as sm


def _check_consequences(chains, st, lY, K, what):
    scores = [c["score"] for c in chains]
    assert scores == sorted(scores, reverse=True), what                         # scores do not increase
    assert len(chains) <= K and len(chains) <= st["rounds"] <= len(chains) + 1, what
    xs, ys, n = [], [], 0
    for c in chains:
        assert c["nHsps"] == len(c["hsps"]) >= 1 and (c["x0"], c["y0"]) == c["hsps"][0][:2], what
        assert c["score"] == sum(h[3] for h in c["hsps"]), what
        for h in c["hsps"]:
            ix, iy = lm.intervals(h, c["strand"] == "minus", lY)
            xs.append(ix)
            ys.append(iy)
            n += 1
    for iv in (sorted(xs), sorted(ys)):                                         # pairwise disjoint on X and on forward Y
        assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:])), what
    assert n <= min(st["hspsPlus"], _cap(what)) + min(st["hspsMinus"], _cap(what)), what   # at most the pools


_caps = {}


def _cap(what):
    return _caps.get(what[0], 4096)


def _all_cases():
    return [lc.by_name(n) for n in lc.NAMES] + [lc.batch_case()]


def test_consequences_hold_on_every_case():
    for case in _all_cases():
        _caps[case["name"]] = am.default_params(**case["params"])["maxHsps"]
        for i, ((chains, st), (sx, sy)) in enumerate(zip(lc.model(case), case["problems"])):
            _check_consequences(chains, st, len(sy), case["K"], (case["name"], i))


def _strands(name, problem=0):
    return [c["strand"] for c in lc.model(lc.by_name(name))[problem][0]]


def test_every_case_is_the_case_it_is_named_for():
    inv = lc.model(lc.by_name("inversion"))[0][0]
    assert "plus" in _strands("inversion") and "minus" in _strands("inversion")
    minus = next(c for c in inv if c["strand"] == "minus")                      # it covers more than half of B on X
    covered = sum(min(h[0] + h[2], 2 * lc.SEG) - max(h[0], lc.SEG) for h in minus["hsps"] if h[0] < 2 * lc.SEG and h[0] + h[2] > lc.SEG)
    assert covered > lc.SEG // 2 and minus["x0"] >= lc.SEG - 50 and minus["x1"] <= 2 * lc.SEG + 50
    assert _strands("transposition") == ["plus", "plus"]
    t = lc.model(lc.by_name("transposition"))[0][0]
    assert t[0]["x1"] <= t[1]["x0"] and t[1]["y1"] <= t[0]["y0"] or t[1]["x1"] <= t[0]["x0"] and t[0]["y1"] <= t[1]["y0"]   # not colinear
    tie = lc.by_name("tie")
    (sx, sy), = tie["problems"]
    assert sm.rc(sy).decode() == sy and sm.strand_score(sx, sy) == sm.strand_score(sx, sm.rc(sy)) > 0
    assert _strands("tie") == ["plus"]                                          # plus wins the tie; nothing is left for round 2
    for name in ("nothing", "short"):
        chains, st = lc.model(lc.by_name(name))[0]
        assert chains == [] and st["rounds"] == 0
    assert [c for c, _ in lc.model(lc.by_name("empty"))] == [[], []]
    thr = lc.by_name("threshold")
    chains, st = lc.model(thr)[0]
    assert len(chains) == 1 and st["rounds"] == 2 and inv[1]["score"] < thr["S"] < inv[0]["score"]
    assert len(lc.model(lc.by_name("k_cut"))[0][0]) == 1 and len(inv) >= 2
    cap = lc.model(lc.by_name("cap"))[0][1]
    assert cap["capped"] == 3 and min(cap["hspsPlus"], cap["hspsMinus"]) > lc.CAP_MAX_HSPS
    sizes = [st["hspsPlus"] for _, st in lc.model(lc.by_name("pool_sizes"))]
    assert sizes[0] < 64 and 65 <= sizes[1] <= 256 and sizes[2] > 256, sizes
    trimmed = lc.model(lc.by_name("trim"))[0][0]
    assert any(len(c["runs"]) == 0 for c in trimmed) and any(len(c["runs"]) > 0 for c in trimmed)
    plain, seeded = lc.model(lc.by_name("inversion"))[0][1], lc.model(lc.by_name("transitions"))[0][1]
    assert seeded["hitsPlus"] > plain["hitsPlus"] and seeded["hitsMinus"] > plain["hitsMinus"]
    assert _strands("minus_only") == ["minus"]
    batch = lc.model(lc.batch_case())
    assert len(batch) == 300 and batch[17][0] == [] and batch[101][0] == []
    assert {tuple(c["strand"] for c in chains) for chains, _ in batch} >= {("plus",), ("plus", "minus"), ("plus", "plus")}


def test_one_plus_chain_is_anchors_once_and_one_of_both_is_the_strand_score():
    """The K = 1 consequences on the model: the runs of anchors_once, strand and score of the strand model."""
    for name in ("inversion", "pool_sizes", "tie"):
        case = lc.by_name(name)
        params = am.default_params(**case["params"])
        for sx, sy in case["problems"]:
            for trim in (0, 14):
                chains, _ = lm.local_chains(sx, sy, "plus", 1, 0, trim, 20, params)
                runs, _ = am.anchors_once(sx, sy, trim, True, params)
                assert [tuple(r[:3]) for r in chains[0]["runs"].tolist()] == runs
            chains, _ = lm.local_chains(sx, sy, "both", 1, 0, 0, 20, params)
            plus, minus = sm.strand_score(sx, sy, params), sm.strand_score(sx, sm.rc(sy), params)
            assert (chains[0]["strand"], chains[0]["score"]) == ("minus" if minus > plus else "plus", max(plus, minus))


def test_consequences_hold_on_random_pairs():
    rng = random.Random(99)
    params = am.default_params(xDrop=150)
    kinds = set()
    for k in range(100):
        parts = [lc.rand_seq(rng, 120 + rng.randrange(200)) for _ in range(3)]
        sx = "".join(parts)
        order = list(range(3))
        rng.shuffle(order)
        sy = "".join(lc.rc(lc.mutate(rng, parts[j], 0.08)) if rng.random() < 0.4 else lc.mutate(rng, parts[j], 0.08) for j in order)
        strand = ("both", "plus", "minus")[k % 3]
        chains, st = lm.local_chains(sx, sy, strand, 1 + k % 5, 0, 0, 20, params)
        _check_consequences(chains, st, len(sy), 1 + k % 5, ("random", k))
        kinds.add(len(chains))
    assert max(kinds) >= 3
