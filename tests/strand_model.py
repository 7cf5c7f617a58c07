"""Strand of a pair, as DESIGN.md section 7 step 0 defines it, in plain Python on top of tests/anchor_model.py: the model
the GPU result is compared with, integer for integer.

    rc(s)                               the reverse complement, bytes
    strand_score(sX, sY, params)        chain score of ONE top-level pass (steps 1-4, soft mask on) on the whole pair
    find_anchor_runs_stranded(sX, sY, strand, ...)
        -> (runs int64[n, 4], statistics dict, {"strand", "scorePlus", "scoreMinus"})
"""
import numpy as np

import anchor_model as am

_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s):
    """Bytes reversed, A<->T, C<->G, a<->t, c<->g; every other byte stays as it is.  Position y' of rc(Y) is position
    lY - 1 - y' of Y."""
    s = s.encode() if isinstance(s, str) else bytes(s)
    return s[::-1].translate(_COMPLEMENT)


def strand_score(sX, sY, params=None):
    """anchors_once (steps 1-4, softMask on, whatever the size) with the chain's score kept: the sum of the chained HSPs'
    scores, 0 when there is no HSP."""
    params = params or am.default_params()
    if len(sX) == 0 or len(sY) == 0:
        return 0
    seed, span = params["seed"], len(params["seed"])
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    cx, cy = am._CODE[am._bytes(sX)], am._CODE[am._bytes(sY)]
    hsps = set()
    for x, y in am.seed_hits(sX, sY, seed, params["maxSeedOccurrences"], True):
        h = am.extend_hit(cx, cy, x, y, span, score, params["xDrop"])
        if h[3] >= params["hspThreshold"]:
            hsps.add(h)
    if len(hsps) > params["maxHsps"]:
        hsps = sorted(hsps, key=lambda h: (-h[3], h[0], h[1], h[2]))[:params["maxHsps"]]
    hsps = sorted(hsps, key=lambda h: (h[0], h[1], h[2]))
    return int(sum(hsps[i][3] for i in am.chain(hsps)))


def find_anchor_runs_stranded(sX, sY, strand="both", trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                              repeatMaskMatrixBiggerThanThis=500 * 500, params=None):
    """strand "plus" / "minus" force the orientation and score only what the forward call computes anyway (the top-level
    pass of a pair beyond the size limit); "both" scores both orientations and takes minus iff scoreMinus > scorePlus.
    The chosen orientation then goes on as am.find_anchor_runs on (sX, sY) or on (sX, rc(sY))."""
    params = params or am.default_params()
    res = dict(strand="plus", scorePlus=-1, scoreMinus=-1)
    searched = len(sX) * len(sY) > anchorMatrixBiggerThanThis and len(sX) > 0 and len(sY) > 0
    if strand == "both":
        res["scorePlus"], res["scoreMinus"] = strand_score(sX, sY, params), strand_score(sX, rc(sY), params)
        res["strand"] = "minus" if res["scoreMinus"] > res["scorePlus"] else "plus"
    elif strand == "minus":
        res["strand"] = "minus"
        if searched:
            res["scoreMinus"] = strand_score(sX, rc(sY), params)
    elif searched:
        res["scorePlus"] = strand_score(sX, sY, params)
    y = rc(sY) if res["strand"] == "minus" else sY
    runs, st = am.find_anchor_runs(sX, y, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params)
    return runs, st, res
