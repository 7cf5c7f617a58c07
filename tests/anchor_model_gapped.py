"""The anchor finder's definition with gapped extension of the chain (DESIGN.md section 7, step 5b;
cpecan_anchor_options.gappedExtension, yDrop, gappedMaxDiagonals) in plain Python / numpy: tests/anchor_model_threshold.py
-- which is anchor_model_transitions and anchor_model at its defaults -- with a step between the chain and the trim, every
other step reused from there.  Written from the definition: cells, three states, sequential anti-diagonals.

    right_extension(cx, cy, score, yDrop, maxDiagonals)     (best, (i*, j*), blocks [(i, j, length)]) of one gap corner
    extend_chain(cx, cy, chain, score, yDrop, maxDiagonals) the merged, untrimmed blocks of a chain [(x, y, length)]
    anchors_once(sX, sY, trim, softMask, params, seedTransitions, threshold, gapped, yDrop, gappedMaxDiagonals)
    find_anchor_runs(...) / find_anchor_runs_stranded(...)  step 6 and step 0 around them
    gap_rows(chain, lX, lY, maxDiagonals)                   the scratch rows a chain's extensions take in a pass

gapped, yDrop and gappedMaxDiagonals travel beside the parameter dict as the C struct holds them: 0 / 1, 0 for 9400, 0 for
4096.  With gapped == 0 this is anchor_model_threshold, integer for integer.
"""
import numpy as np

import anchor_model as am
import anchor_model_threshold as ath
import strand_model as sm

GAP_OPEN, GAP_EXTEND = 400, 30                 # lastz's for HOXD70: a gap of L columns costs GAP_OPEN + L * GAP_EXTEND
Y_DROP = GAP_OPEN + 300 * GAP_EXTEND           # 9400
MAX_DIAGONALS = 4096
BAND = 31                                      # cells with |i - j| <= BAND
NONE = -(1 << 60)                              # "no path": far under every sum a path can have, and it stays there


def _options(gapped, yDrop, gappedMaxDiagonals):
    """The three values as the kernels get them; ValueError for what the C entry points refuse."""
    if gapped not in (0, 1) or yDrop < 0 or (gappedMaxDiagonals != 0 and not 64 <= gappedMaxDiagonals <= 4096):
        raise ValueError((gapped, yDrop, gappedMaxDiagonals))
    if not gapped and (yDrop or gappedMaxDiagonals):
        raise ValueError((gapped, yDrop, gappedMaxDiagonals))
    return gapped, yDrop or Y_DROP, gappedMaxDiagonals or MAX_DIAGONALS


def right_extension(cx, cy, score, yDrop=Y_DROP, maxDiagonals=MAX_DIAGONALS):
    """The right extension over the codes cx[0..m), cy[0..n): (best, (i*, j*), blocks), blocks being (i, j, length) of
    the runs of aligned columns, ascending, relative to the corner.  Empty: (0, (0, 0), [])."""
    m, n = len(cx), len(cy)
    dMax = min(m + n, maxDiagonals)
    W = 2 * BAND + 1                           # index k + BAND stands for the matrix diagonal k = i - j
    k = np.arange(-BAND, BAND + 1, dtype=np.int64)
    none = np.full(W, NONE, dtype=np.int64)
    M, I, D = [none.copy()], [none.copy()], [none.copy()]     # per anti-diagonal
    M[0][BAND] = 0
    srcM, srcI, srcD = [None], [None], [None]
    best, best_at = 0, (0, 0)
    top = [0]
    for d in range(1, dMax + 1):
        i2 = d + k
        i, j = i2 // 2, (d - k) // 2
        cell = (i2 % 2 == 0) & (i >= 0) & (i <= m) & (j >= 0) & (j <= n)
        # M: from (i - 1, j - 1), two anti-diagonals back on the same k; among equal values M, then I, then D
        m_new, m_src = none.copy(), np.zeros(W, dtype=np.int8)
        if d >= 2:
            can = cell & (i >= 1) & (j >= 1)
            three = np.stack([M[d - 2], I[d - 2], D[d - 2]])
            which = np.argmax(three, axis=0)                 # the first of equal maxima
            prev = three.max(axis=0)
            can &= prev > NONE // 2
            s = np.zeros(W, dtype=np.int64)
            s[can] = score[cx[i[can] - 1], cy[j[can] - 1]]
            m_new[can] = prev[can] + s[can]
            m_src[can] = which[can]
        # I: from (i - 1, j), the diagonal k - 1 of the anti-diagonal before; a tie goes to M
        i_new, i_src = none.copy(), np.zeros(W, dtype=np.int8)
        fromM = np.concatenate([[NONE], M[d - 1][:-1]])
        fromI = np.concatenate([[NONE], I[d - 1][:-1]])
        a, b = fromM - GAP_OPEN - GAP_EXTEND, fromI - GAP_EXTEND
        can = cell & (i >= 1) & (np.maximum(fromM, fromI) > NONE // 2)
        i_new[can] = np.maximum(a, b)[can]
        i_src[can] = (b > a)[can]
        # D: from (i, j - 1), the diagonal k + 1
        d_new, d_src = none.copy(), np.zeros(W, dtype=np.int8)
        fromM = np.concatenate([M[d - 1][1:], [NONE]])
        fromD = np.concatenate([D[d - 1][1:], [NONE]])
        a, b = fromM - GAP_OPEN - GAP_EXTEND, fromD - GAP_EXTEND
        can = cell & (j >= 1) & (np.maximum(fromM, fromD) > NONE // 2)
        d_new[can] = np.maximum(a, b)[can]
        d_src[can] = (b > a)[can]
        for new in (m_new, i_new, d_new):
            new[new < NONE // 2] = NONE
        M.append(m_new), I.append(i_new), D.append(d_new)
        srcM.append(m_src), srcI.append(i_src), srcD.append(d_src)
        if int(m_new.max()) > best:                          # the smallest d, then the smallest i - j
            best = int(m_new.max())
            at = int(np.argmax(m_new))
            best_at = (int(i[at]), int(j[at]))
        t = int(max(m_new.max(), i_new.max(), d_new.max()))
        top.append(t)
        if t < best - yDrop and top[d - 1] < best - yDrop:
            break
    if best == 0:
        return 0, (0, 0), []
    # the way back from the best cell in state M; every M step is the aligned column (i - 1, j - 1)
    columns = []
    (i, j), state = best_at, 0
    while (i, j, state) != (0, 0, 0):
        d, at = i + j, i - j + BAND
        if state == 0:
            columns.append((i - 1, j - 1))
            state = int(srcM[d][at])
            i, j = i - 1, j - 1
        elif state == 1:
            state = 1 if srcI[d][at] else 0
            i -= 1
        else:
            state = 2 if srcD[d][at] else 0
            j -= 1
        assert i >= 0 and j >= 0
    blocks = []
    for x, y in reversed(columns):
        if blocks and blocks[-1][0] + blocks[-1][2] == x and blocks[-1][1] + blocks[-1][2] == y:
            blocks[-1][2] += 1
        else:
            blocks.append([x, y, 1])
    return best, best_at, [tuple(b) for b in blocks]


def gap_extensions(cx, cy, lower, upper, right, left, score, yDrop, maxDiagonals):
    """The blocks of one gap, the rectangle from its lower corner to its upper one, in the problem's coordinates:
    (right blocks, left blocks), each ascending, after the overlap rule."""
    (ax, ay), (bx, by) = lower, upper
    gx, gy = cx[ax:bx], cy[ay:by]
    m, n = len(gx), len(gy)
    bestR, (iR, jR), blocksR = right_extension(gx, gy, score, yDrop, maxDiagonals) if right else (0, (0, 0), [])
    bestL, (iL, jL), blocksL = right_extension(gx[::-1], gy[::-1], score, yDrop, maxDiagonals) if left else (0, (0, 0), [])
    if iR + iL > m or jR + jL > n:                           # they overlap: the smaller best goes, the left one on a tie
        if bestR < bestL:
            blocksR = []
        else:
            blocksL = []
    outR = [(ax + i, ay + j, length) for i, j, length in blocksR]
    outL = sorted((bx - i - length, by - j - length, length) for i, j, length in blocksL)
    return outR, outL


def extend_chain(cx, cy, chain, score, yDrop=Y_DROP, maxDiagonals=MAX_DIAGONALS):
    """Step 5b: the chained HSPs [(x, y, length)] in chain order with the extensions of every gap between them, neighbours
    that continue each other merged.  Untrimmed."""
    c = len(chain)
    corners = [(0, 0)] + [(x + length, y + length) for x, y, length in chain]        # lower corner of gap g
    starts = [(x, y) for x, y, length in chain] + [(len(cx), len(cy))]               # upper corner of gap g
    out = []
    for g in range(c + 1):
        blocksR, blocksL = gap_extensions(cx, cy, corners[g], starts[g], g >= 1, g < c, score, yDrop, maxDiagonals)
        out += blocksR + blocksL
        if g < c:
            out.append(tuple(chain[g]))
    merged = []
    for x, y, length in out:
        if merged and merged[-1][0] + merged[-1][2] == x and merged[-1][1] + merged[-1][2] == y:
            merged[-1][2] += length
        else:
            merged.append([x, y, length])
    return [tuple(b) for b in merged]


def gap_rows_each(chain, lX, lY, maxDiagonals=MAX_DIAGONALS):
    """anchor_gap_rows of cpk_anchor.inl for every gap g = 0 .. len(chain) of a chain [(x, y, length)]: the scratch rows of
    its extensions, min(m + n, maxDiagonals) for the right one (g >= 1) and as many for the left one (g < len(chain))."""
    c = len(chain)
    corners = [(0, 0)] + [(x + length, y + length) for x, y, length in chain]
    starts = [(x, y) for x, y, length in chain] + [(lX, lY)]
    return [((g >= 1) + (g < c)) * min(starts[g][0] - corners[g][0] + starts[g][1] - corners[g][1], maxDiagonals)
            for g in range(c + 1)]


def gap_rows(chain, lX, lY, maxDiagonals=MAX_DIAGONALS):
    """The scratch rows of a problem in a pass with step 5b: anchor_gap_rows summed over the gaps of its chain."""
    return sum(gap_rows_each(chain, lX, lY, maxDiagonals))


def anchors_once(sX, sY, trim, softMask, params, seedTransitions=0, threshold=0, gapped=0, yDrop=0, gappedMaxDiagonals=0):
    """Steps 1-5 with 5b: (runs [(x, y, length)], counts dict).  The counts are those of steps 1-4."""
    gapped, yDrop, maxDiagonals = _options(gapped, yDrop, gappedMaxDiagonals)
    if not gapped:
        return ath.anchors_once(sX, sY, trim, softMask, params, seedTransitions, threshold)
    hsps, hits, found = ath._hsps(sX, sY, softMask, params, seedTransitions, threshold)
    picked = am.chain(hsps)
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    cx, cy = am._CODE[am._bytes(sX)], am._CODE[am._bytes(sY)]
    blocks = extend_chain(cx, cy, [hsps[i][:3] for i in picked], score, yDrop, maxDiagonals)
    runs = [(x + trim, y + trim, length - 2 * trim) for x, y, length in blocks if length - 2 * trim > 0]
    return runs, dict(hits=hits, hsps=found, chained=len(picked), capped=int(found > params["maxHsps"]))


def find_anchor_runs(sX, sY, trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                     repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0, threshold=0, gapped=0, yDrop=0,
                     gappedMaxDiagonals=0):
    """Step 6 around steps 1-5b, as anchor_model.find_anchor_runs: the gaps are those between the extended runs, and the
    extension holds inside them too."""
    params = params or am.default_params()
    _options(gapped, yDrop, gappedMaxDiagonals)
    lX, lY = len(sX), len(sY)
    st = dict(hits=0, hsps=0, chained=0, runs=0, anchorColumns=0, subProblems=0, largestGapTop=lX * lY, largestGap=lX * lY,
              capped=0)
    if lX * lY <= anchorMatrixBiggerThanThis or lX == 0 or lY == 0:
        return np.zeros((0, 4), dtype=np.int64), st

    def add(c):
        for k in ("hits", "hsps", "chained"):
            st[k] += c[k]
        st["capped"] |= c["capped"]

    top, c = anchors_once(sX, sY, trim, True, params, seedTransitions, threshold, gapped, yDrop, gappedMaxDiagonals)
    add(c)
    st["largestGapTop"] = max((x - pX) * (y - pY) for pX, pY, x, y in am._gaps(top, lX, lY))
    out = []
    for j, (pX, pY, x, y) in enumerate(am._gaps(top, lX, lY)):
        matrix = (x - pX) * (y - pY)
        if matrix > anchorMatrixBiggerThanThis:
            sub, c = anchors_once(sX[pX:x], sY[pY:y], trim, matrix > repeatMaskMatrixBiggerThanThis, params, seedTransitions,
                                  threshold, gapped, yDrop, gappedMaxDiagonals)
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


def find_anchor_runs_stranded(sX, sY, strand="both", trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                              repeatMaskMatrixBiggerThanThis=500 * 500, params=None, seedTransitions=0, threshold=0, gapped=0,
                              yDrop=0, gappedMaxDiagonals=0):
    """anchor_model_threshold.find_anchor_runs_stranded with step 5b in every pass.  The strand score is the chain score
    of step 4: the extension does not change it."""
    params = params or am.default_params()
    res = dict(strand="plus", scorePlus=-1, scoreMinus=-1)
    searched = len(sX) * len(sY) > anchorMatrixBiggerThanThis and len(sX) > 0 and len(sY) > 0
    if strand == "both":
        res["scorePlus"] = ath.strand_score(sX, sY, params, seedTransitions, threshold)
        res["scoreMinus"] = ath.strand_score(sX, sm.rc(sY), params, seedTransitions, threshold)
        res["strand"] = "minus" if res["scoreMinus"] > res["scorePlus"] else "plus"
    elif strand == "minus":
        res["strand"] = "minus"
        if searched:
            res["scoreMinus"] = ath.strand_score(sX, sm.rc(sY), params, seedTransitions, threshold)
    elif searched:
        res["scorePlus"] = ath.strand_score(sX, sY, params, seedTransitions, threshold)
    y = sm.rc(sY) if res["strand"] == "minus" else sY
    runs, st = find_anchor_runs(sX, y, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params,
                                seedTransitions, threshold, gapped, yDrop, gappedMaxDiagonals)
    return runs, st, res
