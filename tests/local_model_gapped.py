"""Local chains with gapped extension (cpecan_find_local_chains_many_gapped) in plain Python:
tests/local_model.py, whose chains carry their HSPs, with the extension of tests/anchor_model_gapped.py run into every gap
of every chain between fences.  Written from the rule: an occupied set, gaps, fences, the walk of step 5b as it is, the
overlap test, assembly, trim.  Loops over sets; nothing about lanes, scratch rows or launches.

    local_chains(sX, sY, strand, maxChains, minChainScore, trim, expansion, params, seedTransitions, transitionHspThreshold,
                 gapped, yDrop, gappedMaxDiagonals)  -> (chains [dict], statistics dict)

A chain is local_model's with `runs` replaced by the trimmed merged blocks, the rectangle by theirs, and three keys only the
model has: `blocks` (the merged blocks, untrimmed), `kept` (the extension blocks it kept, untrimmed, in its orientation) and
`gaps` (one record per gap: what the walks saw and what became of them), which tests/test_local_gapped_cases_cpu.py reads.
With gapped == 0 this is local_model.local_chains, integer for integer.
"""
import numpy as np

import anchor_model as am
import anchor_model_gapped as amg
import local_model as lm
import strand_model as sm


def _flip(iv, lY):
    return (lY - iv[1], lY - iv[0])


def _extend(cx, cy, chain, occupied, score, yDrop, maxDiagonals):
    """Step 7b on one chain.  chain: its HSPs (x, y, length) in its own orientation; occupied: [(X interval, Y interval)] in
    that orientation.  Returns (merged blocks, kept extension blocks, gap records)."""
    lX, lY = len(cx), len(cy)
    c = len(chain)
    lower = [(0, 0)] + [(x + n, y + n) for x, y, n in chain]
    upper = [(x, y) for x, y, n in chain] + [(lX, lY)]
    out, kept, records = [], [], []
    for g in range(c + 1):
        (ax, ay), (bx, by) = lower[g], upper[g]
        m, n = bx - ax, by - ay
        right, left = g >= 1, g < c
        # fences: the smallest occupied start at or behind the lower corner, the largest occupied end at or before the upper
        fxR = min([ix[0] for ix, _ in occupied if ax <= ix[0] < bx] + [bx])
        fyR = min([iy[0] for _, iy in occupied if ay <= iy[0] < by] + [by])
        fxL = max([ix[1] for ix, _ in occupied if ax < ix[1] <= bx] + [ax])
        fyL = max([iy[1] for _, iy in occupied if ay < iy[1] <= by] + [ay])
        mR, nR, mL, nL = fxR - ax, fyR - ay, bx - fxL, by - fyL
        R = amg.right_extension(cx[ax:ax + mR], cy[ay:ay + nR], score, yDrop, maxDiagonals) if right else (0, (0, 0), [])
        L = amg.right_extension(cx[bx - mL:bx][::-1], cy[by - nL:by][::-1], score, yDrop, maxDiagonals) if left else (0, (0, 0), [])
        (bestR, (iR, jR), blocksR), (bestL, (iL, jL), blocksL) = R, L
        dropped = None
        if iR + iL > m or jR + jL > n:                       # 5b's test on the whole gap
            if bestR < bestL:
                blocksR, dropped = [], "right"
            else:
                blocksL, dropped = [], "left"
        outR = [(ax + i, ay + j, k) for i, j, k in blocksR]
        outL = sorted((bx - i - k, by - j - k, k) for i, j, k in blocksL)
        records.append(dict(g=g, m=m, n=n, right=right, left=left, sides=dict(R=(mR, nR), L=(mL, nL)), best=dict(R=bestR, L=bestL),
                            reach=dict(R=(iR, jR), L=(iL, jL)), dropped=dropped, kept=dict(R=len(outR), L=len(outL)),
                            corner=dict(R=(ax, ay), L=(bx, by))))
        kept += outR + outL
        out += outR + outL
        if g < c:
            out.append(tuple(chain[g]))
    merged = []
    for x, y, k in out:
        if merged and merged[-1][0] + merged[-1][2] == x and merged[-1][1] + merged[-1][2] == y:
            merged[-1][2] += k
        else:
            merged.append([x, y, k])
    return [tuple(b) for b in merged], kept, records


def local_chains(sX, sY, strand="both", maxChains=1, minChainScore=0, trim=14, expansion=20, params=None, seedTransitions=0,
                 transitionHspThreshold=0, gapped=1, yDrop=0, gappedMaxDiagonals=0, hsp_fences_only=False):
    """hsp_fences_only: the occupied set without the blocks that earlier rounds kept -- NOT the rule; the case tests use it to
    show that round order decides a result."""
    params = params or am.default_params()
    gapped, yDrop, maxDiagonals = amg._options(gapped, yDrop, gappedMaxDiagonals)
    chains, st = lm.local_chains(sX, sY, strand, maxChains, minChainScore, trim, expansion, params, seedTransitions,
                                 transitionHspThreshold)
    if not gapped:
        return chains, st
    lY = len(sY)
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    cx = am._CODE[am._bytes(sX)]
    cys = {"plus": am._CODE[am._bytes(sY)], "minus": am._CODE[am._bytes(sm.rc(sY))]}
    kept_forward = []                                        # (X interval, forward-Y interval) of the blocks kept so far
    for r, ch in enumerate(chains):
        minus = ch["strand"] == "minus"
        occupied = [lm.intervals(h, o["strand"] == "minus", lY) for q, o in enumerate(chains) if q != r for h in o["hsps"]]
        if not hsp_fences_only:
            occupied += kept_forward
        if minus:
            occupied = [(ix, _flip(iy, lY)) for ix, iy in occupied]
        merged, kept, records = _extend(cx, cys[ch["strand"]], [h[:3] for h in ch["hsps"]], occupied, score, yDrop, maxDiagonals)
        kept_forward += [lm.intervals(b, minus, lY) for b in kept]
        runs = [(x + trim, y + trim, k - 2 * trim, expansion) for x, y, k in merged if k - 2 * trim > 0]
        ch.update(runs=np.array(runs, dtype=np.int64).reshape(-1, 4), blocks=merged, kept=kept, gaps=records, x0=merged[0][0],
                  y0=merged[0][1], x1=merged[-1][0] + merged[-1][2], y1=merged[-1][1] + merged[-1][2])
    return chains, st


def disjoint(chains, lY):
    """Consequence 1: all untrimmed blocks of a problem are pairwise disjoint on X and on forward Y."""
    xs, ys = [], []
    for c in chains:
        for b in c["blocks"]:
            ix, iy = lm.intervals(b, c["strand"] == "minus", lY)
            xs.append(ix)
            ys.append(iy)
    return all(a[1] <= b[0] for iv in (sorted(xs), sorted(ys)) for a, b in zip(iv, iv[1:]))
