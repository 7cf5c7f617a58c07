"""The cases of tests/local_gapped_cases.py on the model (tests/local_model_gapped.py), no GPU: every case shows the edge of
DESIGN.md section 7 step 7b it is named for, so one that stops exercising it fails here; and the consequences of the rule
hold on every case and on random pairs."""
import random

import numpy as np

import anchor_model as am
import anchor_model_gapped as amg
import local_cases as lc
import local_gapped_cases as gc
import local_model as lm
import local_model_gapped as lmg
import strand_model as sm


def _check_consequences(chains, lY, what):
    assert lmg.disjoint(chains, lY), what                                       # disjoint on X and on forward Y
    for c in chains:
        b = c["blocks"]
        assert all(p[0] + p[2] <= q[0] and p[1] + p[2] <= q[1] for p, q in zip(b, b[1:])), what   # ascending on both axes
        for h in c["hsps"]:                                                     # every chained HSP inside a block of its chain
            assert any(p[0] <= h[0] and h[0] + h[2] <= p[0] + p[2] and p[0] - p[1] == h[0] - h[1] for p in b), what
        assert (c["x0"], c["y0"]) == b[0][:2] and (c["x1"], c["y1"]) == (b[-1][0] + b[-1][2], b[-1][1] + b[-1][2]), what
        assert c["nHsps"] == len(c["hsps"]) and c["score"] == sum(h[3] for h in c["hsps"]), what  # the peel's, unchanged


def test_consequences_hold_on_every_case():
    for case in [gc.by_name(n) for n in gc.NAMES if n != "off"] + [gc.batch_case()]:
        for i, ((chains, _), (sx, sy)) in enumerate(zip(gc.model(case), case["problems"])):
            _check_consequences(chains, len(sy), (case["name"], i))


def _gaps(chains):
    return [(r, c, g) for r, c in enumerate(chains) for g in c["gaps"]]


def test_inversion():
    chains, _ = gc.model(gc.by_name("inversion"))[0]
    assert any(c["strand"] == "minus" and c["kept"] for c in chains)
    assert any(len(c["runs"]) > c["nHsps"] for c in chains)
    assert any(g["dropped"] and g["reach"]["R"][0] + g["reach"]["L"][0] > g["m"] and min(g["best"].values()) > 0 for _, _, g in _gaps(chains))


def test_transposition():
    chains, _ = gc.model(gc.by_name("transposition"))[0]
    assert [c["strand"] for c in chains] == ["plus", "plus"]
    seen = False
    for _, _, g in _gaps(chains):
        for side, other in (("R", "L"), ("L", "R")):
            (ms, ns), (i, j) = g["sides"][side], g["reach"][side]
            fenced_x, fenced_y = ms < g["m"], ns < g["n"]
            kept = g["kept"][side] > 0
            seen |= kept and fenced_x != fenced_y and ((fenced_x and i == ms) or (fenced_y and j == ns))
    assert seen


def test_shared_middle():
    case = gc.by_name("shared_middle")
    (sx, sy), = case["problems"]
    chains, _ = gc.model(case)[0]
    loose, _ = gc.model_of(case, sx, sy, hsp_fences_only=True)
    assert len(chains) == len(loose) >= 2
    # some gap of a later round is fenced by a block an earlier round kept: without those blocks its sides are wider ...
    assert any(g["sides"] != h["sides"] for (r, _, g), (_, _, h) in zip(_gaps(chains), _gaps(loose)) if r >= 1)
    # ... and then two chains overlap on X: round order decides the result
    assert lmg.disjoint(chains, len(sy)) and not lmg.disjoint(loose, len(sy))
    xs = sorted((b[0], b[0] + b[2]) for c in loose for b in c["blocks"])
    assert any(a[1] > b[0] for a, b in zip(xs, xs[1:]))


def test_end_gaps():
    case = gc.by_name("end_gaps")
    (inner, _), (whole, _) = gc.model(case)
    first, last = inner[0]["gaps"][0], inner[0]["gaps"][-1]
    assert first["kept"]["L"] > 0 and last["kept"]["R"] > 0                     # both end gaps extend outwards ...
    assert first["reach"]["L"][0] < first["m"] and first["reach"]["L"][1] < first["n"]   # ... and end inside the sequences
    assert last["reach"]["R"][0] < last["m"] and last["reach"]["R"][1] < last["n"]
    c = whole[0]
    assert (c["x0"], c["y0"]) == (0, 0) or (c["x1"], c["y1"]) == tuple(len(s) for s in case["problems"][1])
    assert any(g["kept"][s] and g["reach"][s] == (g["m"], g["n"]) for g in (c["gaps"][0], c["gaps"][-1]) for s in "RL")


def _again(case, sx, sy, g, side, yDrop, maxDiagonals):
    """The walk of one extension of a gap record once more, with another y-drop or diagonal limit: (best, reach)."""
    params = am.default_params(**case["params"])
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    cx, cy = am._CODE[am._bytes(sx)], am._CODE[am._bytes(sy)]
    (x, y), (ms, ns) = g["corner"][side], g["sides"][side]
    gx, gy = (cx[x:x + ms], cy[y:y + ns]) if side == "R" else (cx[x - ms:x][::-1], cy[y - ns:y][::-1])
    best, reach, _ = amg.right_extension(gx, gy, score, yDrop, maxDiagonals)
    return best, reach


def test_narrow():
    case = gc.by_name("narrow")
    assert (case["yDrop"], case["maxDiagonals"]) == (600, 64)
    (sx, sy), = case["problems"]
    chains, _ = gc.model(case)[0]
    assert [c["strand"] for c in chains][:1] == ["plus"]
    cut = dropped = False
    for _, _, g in _gaps(chains):
        for side in "RL":
            if not g[{"R": "right", "L": "left"}[side]]:
                continue
            here = (g["best"][side], g["reach"][side])
            assert here == _again(case, sx, sy, g, side, 600, 64)
            ms, ns = g["sides"][side]
            if ms + ns <= 64 or here[0] == 0:
                continue
            unlimited = _again(case, sx, sy, g, side, 600, 4096)
            cut |= here != unlimited                                             # the 64 anti-diagonals cut it
            # the limit did not, and a larger y-drop carries it further: the y-drop ended it
            dropped |= here == unlimited and here != _again(case, sx, sy, g, side, 9400, 4096)
    assert cut and dropped


def test_one_chain_is_the_gapped_anchor_finder_once():
    case = gc.by_name("one_chain")
    params = am.default_params(**case["params"])
    for trim in (0, 14):
        for sx, sy in case["problems"]:
            (c,), _ = gc.model_of(dict(case, trim=trim), sx, sy)
            runs, _ = amg.anchors_once(sx, sy, trim, True, params, gapped=1)
            assert [tuple(r[:3]) for r in c["runs"].tolist()] == runs
            assert c["blocks"] == amg.extend_chain(am._CODE[am._bytes(sx)], am._CODE[am._bytes(sy)], [h[:3] for h in c["hsps"]],
                                                   np.array(params["scores"], dtype=np.int64).reshape(5, 5))


def test_off_is_the_local_model():
    case = gc.by_name("off")
    (sx, sy), = case["problems"]
    got, st = gc.model(case)[0]
    want, wst = lm.local_chains(sx, sy, case["strand"], case["K"], 0, case["trim"], 20, am.default_params(**case["params"]))
    assert st == wst and len(got) == len(want) >= 2 and all(lm.same(g, w) for g, w in zip(got, want))


def test_batch():
    case = gc.batch_case()
    batch = gc.model(case)
    assert len(batch) == 300 and batch[17][0] == [] and batch[101][0] == []
    assert {tuple(c["strand"] for c in chains) for chains, _ in batch} >= {("plus",), ("plus", "minus"), ("plus", "plus")}
    every = [c for chains, _ in batch for c in chains]
    assert any(len(c["runs"]) == 0 for c in every) and any(len(c["runs"]) > c["nHsps"] for c in every)
    assert any(c["kept"] for c in every if c["strand"] == "minus")


def test_consequences_hold_on_random_pairs():
    rng = random.Random(7)
    params = am.default_params(xDrop=150)
    more = 0
    for k in range(40):
        parts = [lc.rand_seq(rng, 120 + rng.randrange(200)) for _ in range(3)]
        order = list(range(3))
        rng.shuffle(order)
        sx = "".join(parts)
        sy = "".join(lc.rc(lc.mutate(rng, parts[j], 0.07, 50)) if rng.random() < 0.4 else lc.mutate(rng, parts[j], 0.07, 50) for j in order)
        chains, _ = lmg.local_chains(sx, sy, ("both", "plus", "minus")[k % 3], 1 + k % 5, 0, 0, 20, params)
        _check_consequences(chains, len(sy), ("random", k))
        more += sum(len(c["blocks"]) > c["nHsps"] for c in chains)
    assert more >= 10
