"""The anchor finder's definition with seedTransitions in plain Python: tests/anchor_model.py
with another step 1 and every other step reused from there.  With seedTransitions == 0 it is that model.

    seed_hits(sX, sY, seed, maxSeedOccurrences, softMask, seedTransitions)   the set of (x, y) window pairs
    anchors_once(sX, sY, trim, softMask, params, seedTransitions)            steps 1-5
    find_anchor_runs(sX, sY, ..., params, seedTransitions)                   step 6 around them
    strand_score / find_anchor_runs_stranded                                 tests/strand_model.py's step 0 around this model

anchor_model.default_params refuses keys it does not know, so seedTransitions travels beside the parameter dict.
"""
import numpy as np

import anchor_model as am
import strand_model as sm


def seed_hits(sX, sY, seed, maxSeedOccurrences, softMask, seedTransitions=0):
    """Step 1.  Words, skipped windows and the occurrence filter as in anchor_model (exact words, counted per side).  A hit
    is an X window with word w and a Y window with word v, both words surviving the filter, with v == w or, with
    seedTransitions == 1, v == w ^ (2 << 2k) for one k in 0 .. weight-1: in the codes a c g t = 0 1 2 3, XOR 2 swaps a
    with g and c with t."""
    if seedTransitions not in (0, 1):
        raise ValueError(seedTransitions)
    weight = seed.count("1")
    wx, wy = am.seed_words(sX, seed, softMask), am.seed_words(sY, seed, softMask)
    wx = {w: xs for w, xs in wx.items() if len(xs) <= maxSeedOccurrences}
    wy = {w: ys for w, ys in wy.items() if len(ys) <= maxSeedOccurrences}
    hits = set()
    for v, ys in wy.items():
        for w in [v] + ([v ^ (2 << (2 * k)) for k in range(weight)] if seedTransitions else []):
            for x in wx.get(w, ()):
                for y in ys:
                    assert (x, y) not in hits          # two windows match by at most one variant
                    hits.add((x, y))
    return hits


def _hsps(sX, sY, softMask, params, seedTransitions):
    """Steps 1-3: (HSPs sorted by (x, y, length), hits, HSPs found before the cap)."""
    span = len(params["seed"])
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    hits = seed_hits(sX, sY, params["seed"], params["maxSeedOccurrences"], softMask, seedTransitions)
    cx, cy = am._CODE[am._bytes(sX)], am._CODE[am._bytes(sY)]
    hsps = set()
    for x, y in hits:
        h = am.extend_hit(cx, cy, x, y, span, score, params["xDrop"])
        if h[3] >= params["hspThreshold"]:
            hsps.add(h)
    found = len(hsps)
    if found > params["maxHsps"]:
        hsps = sorted(hsps, key=lambda h: (-h[3], h[0], h[1], h[2]))[:params["maxHsps"]]
    return sorted(hsps, key=lambda h: (h[0], h[1], h[2])), len(hits), found


def anchors_once(sX, sY, trim, softMask, params, seedTransitions=0):
    """Steps 1-5: (runs [(x, y, length)], counts dict)."""
    hsps, hits, found = _hsps(sX, sY, softMask, params, seedTransitions)
    picked = am.chain(hsps)
    runs = [(hsps[i][0] + trim, hsps[i][1] + trim, hsps[i][2] - 2 * trim) for i in picked if hsps[i][2] - 2 * trim > 0]
    return runs, dict(hits=hits, hsps=found, chained=len(picked), capped=int(found > params["maxHsps"]))


def find_anchor_runs(sX, sY, trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                     repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0):
    """Step 6 around steps 1-5, as anchor_model.find_anchor_runs."""
    params = params or am.default_params()
    lX, lY = len(sX), len(sY)
    st = dict(hits=0, hsps=0, chained=0, runs=0, anchorColumns=0, subProblems=0, largestGapTop=lX * lY, largestGap=lX * lY,
              capped=0)
    if lX * lY <= anchorMatrixBiggerThanThis or lX == 0 or lY == 0:
        return np.zeros((0, 4), dtype=np.int64), st

    def add(c):
        for k in ("hits", "hsps", "chained"):
            st[k] += c[k]
        st["capped"] |= c["capped"]

    top, c = anchors_once(sX, sY, trim, True, params, seedTransitions)
    add(c)
    st["largestGapTop"] = max((x - pX) * (y - pY) for pX, pY, x, y in am._gaps(top, lX, lY))
    out = []
    for j, (pX, pY, x, y) in enumerate(am._gaps(top, lX, lY)):
        matrix = (x - pX) * (y - pY)
        if matrix > anchorMatrixBiggerThanThis:
            sub, c = anchors_once(sX[pX:x], sY[pY:y], trim, matrix > repeatMaskMatrixBiggerThanThis, params, seedTransitions)
            add(c)
            st["subProblems"] += 1
            out += [(pX + a, pY + b, length) for a, b, length in sub]
        if j < len(top):
            out.append(top[j])
    st["runs"] = len(out)
    st["anchorColumns"] = sum(r[2] for r in out)
    st["largestGap"] = max((x - pX) * (y - pY) for pX, pY, x, y in am._gaps(out, lX, lY))
    runs = np.array([(x, y, length, expansion) for x, y, length in out], dtype=np.int64).reshape(-1, 4)
    return runs, st


def strand_score(sX, sY, params=None, seedTransitions=0):
    """strand_model.strand_score: the chain score of one top-level pass (steps 1-4, soft mask on) on the whole pair."""
    params = params or am.default_params()
    if len(sX) == 0 or len(sY) == 0:
        return 0
    hsps, _, _ = _hsps(sX, sY, True, params, seedTransitions)
    return int(sum(hsps[i][3] for i in am.chain(hsps)))


def find_anchor_runs_stranded(sX, sY, strand="both", trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                              repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0):
    """strand_model.find_anchor_runs_stranded with this model's step 1 in every pass."""
    params = params or am.default_params()
    res = dict(strand="plus", scorePlus=-1, scoreMinus=-1)
    searched = len(sX) * len(sY) > anchorMatrixBiggerThanThis and len(sX) > 0 and len(sY) > 0
    if strand == "both":
        res["scorePlus"] = strand_score(sX, sY, params, seedTransitions)
        res["scoreMinus"] = strand_score(sX, sm.rc(sY), params, seedTransitions)
        res["strand"] = "minus" if res["scoreMinus"] > res["scorePlus"] else "plus"
    elif strand == "minus":
        res["strand"] = "minus"
        if searched:
            res["scoreMinus"] = strand_score(sX, sm.rc(sY), params, seedTransitions)
    elif searched:
        res["scorePlus"] = strand_score(sX, sY, params, seedTransitions)
    y = sm.rc(sY) if res["strand"] == "minus" else sY
    runs, st = find_anchor_runs(sX, y, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params,
                                seedTransitions)
    return runs, st, res
