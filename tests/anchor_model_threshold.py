"""The anchor finder's definition with a threshold of their own for HSPs that only variant hits seed (DESIGN.md section 7,
steps 1-2; cpecan_anchor_options.transitionHspThreshold) in plain Python: tests/anchor_model_transitions.py with a class per
hit and another test in step 2, every other step reused from there and from tests/anchor_model.py.

    classed_hits(sX, sY, seed, maxSeedOccurrences, softMask, seedTransitions)      {(x, y): the two words are equal}
    classed_hsps(sX, sY, softMask, params, seedTransitions, threshold)             {(x, y, length, score): an exact hit extends to it}
    anchors_once(sX, sY, trim, softMask, params, seedTransitions, threshold)       steps 1-5
    find_anchor_runs(sX, sY, ..., params, seedTransitions, threshold)              step 6 around them
    strand_score / find_anchor_runs_stranded                                       step 0 around this model

threshold: 0 stands for params["hspThreshold"], as in the C struct; otherwise it is at least that.  It travels beside the
parameter dict, as seedTransitions does.
"""
import numpy as np

import anchor_model as am
import anchor_model_transitions as amt
import strand_model as sm

INT32_MAX = 2 ** 31 - 1


def _threshold(params, threshold):
    t = threshold or params["hspThreshold"]
    if t < params["hspThreshold"]:
        raise ValueError(threshold)
    return t


def classed_hits(sX, sY, seed, maxSeedOccurrences, softMask, seedTransitions=0):
    """Step 1 with the class of every hit: exact (True) when the two words are equal, variant (False) otherwise.  The
    occurrence filter counts exact words per side with and without the option, so the exact hits are the hits without it."""
    exact = amt.seed_hits(sX, sY, seed, maxSeedOccurrences, softMask, 0)
    hits = amt.seed_hits(sX, sY, seed, maxSeedOccurrences, softMask, seedTransitions)
    assert exact <= hits
    return {h: h in exact for h in hits}


def classed_hsps(sX, sY, softMask, params, seedTransitions=0, threshold=0):
    """Steps 1-2: ({kept HSP (x, y, length, score): at least one exact hit extends to it}, hits).  An HSP is kept iff it
    scores hspThreshold and (it scores `threshold` or an exact hit extends to it)."""
    t = _threshold(params, threshold)
    span = len(params["seed"])
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    hits = classed_hits(sX, sY, params["seed"], params["maxSeedOccurrences"], softMask, seedTransitions)
    cx, cy = am._CODE[am._bytes(sX)], am._CODE[am._bytes(sY)]
    reached = {}
    for (x, y), exact in hits.items():
        h = am.extend_hit(cx, cy, x, y, span, score, params["xDrop"])
        reached[h] = reached.get(h, False) or exact
    return {h: e for h, e in reached.items() if h[3] >= params["hspThreshold"] and (h[3] >= t or e)}, len(hits)


def _hsps(sX, sY, softMask, params, seedTransitions, threshold):
    """Steps 1-3: (HSPs sorted by (x, y, length), hits, HSPs kept before the cap)."""
    kept, hits = classed_hsps(sX, sY, softMask, params, seedTransitions, threshold)
    hsps, found = set(kept), len(kept)
    if found > params["maxHsps"]:
        hsps = sorted(hsps, key=lambda h: (-h[3], h[0], h[1], h[2]))[:params["maxHsps"]]
    return sorted(hsps, key=lambda h: (h[0], h[1], h[2])), hits, found


def anchors_once(sX, sY, trim, softMask, params, seedTransitions=0, threshold=0):
    """Steps 1-5: (runs [(x, y, length)], counts dict)."""
    hsps, hits, found = _hsps(sX, sY, softMask, params, seedTransitions, threshold)
    picked = am.chain(hsps)
    runs = [(hsps[i][0] + trim, hsps[i][1] + trim, hsps[i][2] - 2 * trim) for i in picked if hsps[i][2] - 2 * trim > 0]
    return runs, dict(hits=hits, hsps=found, chained=len(picked), capped=int(found > params["maxHsps"]))


def find_anchor_runs(sX, sY, trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                     repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0, threshold=0):
    """Step 6 around steps 1-5, as anchor_model.find_anchor_runs: the threshold holds in the gaps too."""
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

    top, c = anchors_once(sX, sY, trim, True, params, seedTransitions, threshold)
    add(c)
    st["largestGapTop"] = max((x - pX) * (y - pY) for pX, pY, x, y in am._gaps(top, lX, lY))
    out = []
    for j, (pX, pY, x, y) in enumerate(am._gaps(top, lX, lY)):
        matrix = (x - pX) * (y - pY)
        if matrix > anchorMatrixBiggerThanThis:
            sub, c = anchors_once(sX[pX:x], sY[pY:y], trim, matrix > repeatMaskMatrixBiggerThanThis, params, seedTransitions,
                                  threshold)
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


def strand_score(sX, sY, params=None, seedTransitions=0, threshold=0):
    """The chain score of one top-level pass (steps 1-4, soft mask on) on the whole pair."""
    params = params or am.default_params()
    if len(sX) == 0 or len(sY) == 0:
        return 0
    hsps, _, _ = _hsps(sX, sY, True, params, seedTransitions, threshold)
    return int(sum(hsps[i][3] for i in am.chain(hsps)))


def find_anchor_runs_stranded(sX, sY, strand="both", trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                              repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0, threshold=0):
    """anchor_model_transitions.find_anchor_runs_stranded with the threshold in every pass, both orientations included."""
    params = params or am.default_params()
    res = dict(strand="plus", scorePlus=-1, scoreMinus=-1)
    searched = len(sX) * len(sY) > anchorMatrixBiggerThanThis and len(sX) > 0 and len(sY) > 0
    if strand == "both":
        res["scorePlus"] = strand_score(sX, sY, params, seedTransitions, threshold)
        res["scoreMinus"] = strand_score(sX, sm.rc(sY), params, seedTransitions, threshold)
        res["strand"] = "minus" if res["scoreMinus"] > res["scorePlus"] else "plus"
    elif strand == "minus":
        res["strand"] = "minus"
        if searched:
            res["scoreMinus"] = strand_score(sX, sm.rc(sY), params, seedTransitions, threshold)
    elif searched:
        res["scorePlus"] = strand_score(sX, sY, params, seedTransitions, threshold)
    y = sm.rc(sY) if res["strand"] == "minus" else sY
    runs, st = find_anchor_runs(sX, y, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params,
                                seedTransitions, threshold)
    return runs, st, res
