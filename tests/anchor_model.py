"""The anchor finder's definition (include/cpecan_hip.h) in plain Python / numpy: the model the GPU
result is compared with, integer for integer.  Written from the definition, not from the kernels: sets, sorted orders and
sequential loops, nothing about lanes or launches.

    find_anchor_runs(sX, sY, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params)
        -> (runs int64[n, 4] of (x, y, length, expansion), statistics dict)
"""
import numpy as np

HOXD70 = [[91, -114, -31, -123], [-114, 100, -125, -31], [-31, -125, 100, -114], [-123, -31, -114, 91]]


def default_params(**overrides):
    scores = [[HOXD70[a][b] if a < 4 and b < 4 else -100 for b in range(5)] for a in range(5)]
    p = dict(seed="1110100110010101111", maxSeedOccurrences=1, scores=scores, xDrop=910, hspThreshold=800, maxHsps=4096)
    for k, v in overrides.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


_CODE = np.full(256, 4, dtype=np.int64)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _i
    _CODE[ord(_ch.lower())] = _i
_LOWER = np.zeros(256, dtype=bool)
for _ch in "acgt":
    _LOWER[ord(_ch)] = True


def _bytes(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8)


def seed_words(seq, seed, softMask):
    """Step 1, one sequence: {word: [window positions]} over the windows that are not skipped."""
    raw = _bytes(seq)
    code, lower = _CODE[raw], _LOWER[raw]
    span = len(seed)
    n = len(raw) - span + 1
    if n <= 0:
        return {}
    word = np.zeros(n, dtype=np.int64)
    ok = np.ones(n, dtype=bool)
    for k, ch in enumerate(seed):
        if ch != "1":
            continue
        c = code[k:k + n]
        ok &= c < 4
        if softMask:
            ok &= ~lower[k:k + n]
        word = word * 4 + (c & 3)
    out = {}
    for pos in np.nonzero(ok)[0].tolist():
        out.setdefault(int(word[pos]), []).append(pos)
    return out


def seed_hits(sX, sY, seed, maxSeedOccurrences, softMask):
    """Step 1: the set of (x, y) window pairs with equal words, without the words that occur too often on either side."""
    wx, wy = seed_words(sX, seed, softMask), seed_words(sY, seed, softMask)
    hits = set()
    for word, xs in wx.items():
        ys = wy.get(word)
        if ys is None or len(xs) > maxSeedOccurrences or len(ys) > maxSeedOccurrences:
            continue
        for x in xs:
            for y in ys:
                hits.add((x, y))
    return hits


def _extend(col_scores, xDrop):
    """(best sum, columns) of the shortest prefix of the column scores that reaches the best running sum, walking until
    the sum falls more than xDrop below its best.  col_scores: a function (start, stop) -> scores of columns start..stop-1,
    shorter at the end of a sequence."""
    best, best_len, total, at, chunk = 0, 0, 0, 0, 64
    while True:
        s = col_scores(at, at + chunk)
        if len(s) == 0:
            return best, best_len
        c = total + np.cumsum(s)
        peak = np.maximum(np.maximum.accumulate(c), best)   # best after each column
        stop = np.nonzero(c < peak - xDrop)[0]
        upto = int(stop[0]) if len(stop) else len(c)         # the column that stops the walk can never be the best
        if upto > 0:
            m = int(c[:upto].max())
            if m > best:
                best, best_len = m, at + int(np.argmax(c[:upto])) + 1   # argmax: the first, i.e. the shortest prefix
        if len(stop) or len(s) < chunk:
            return best, best_len
        total = int(c[-1])
        at += chunk
        chunk = min(chunk * 2, 4096)


def extend_hit(cx, cy, x, y, span, score, xDrop):
    """Step 2 for one hit: (x, y, length, score) of the HSP.  cx, cy: symbol codes 0..4."""
    lX, lY = len(cx), len(cy)
    s0 = int(score[cx[x:x + span], cy[y:y + span]].sum())

    def right(a, b):
        b = min(b, lX - (x + span), lY - (y + span))
        return score[cx[x + span + a:x + span + b], cy[y + span + a:y + span + b]] if b > a else np.zeros(0, dtype=np.int64)

    def left(a, b):
        b = min(b, x, y)
        if b <= a:
            return np.zeros(0, dtype=np.int64)
        return score[cx[x - b:x - a][::-1], cy[y - b:y - a][::-1]]

    bestR, lenR = _extend(right, xDrop)
    bestL, lenL = _extend(left, xDrop)
    return x - lenL, y - lenL, span + lenL + lenR, s0 + bestL + bestR


def chain(hsps):
    """Step 4 on HSPs sorted by (x, y, length): the indices of the chain, in increasing order."""
    n = len(hsps)
    if n == 0:
        return []
    a = np.array(hsps, dtype=np.int64)
    ex, ey = a[:, 0] + a[:, 2], a[:, 1] + a[:, 2]
    best = np.zeros(n, dtype=np.int64)
    pred = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        can = (ex[:i] <= a[i, 0]) & (ey[:i] <= a[i, 1])
        best[i] = a[i, 3]
        if can.any():
            m = best[:i][can].max()
            pred[i] = int(np.nonzero(can & (best[:i] == m))[0][0])    # among equal maxima the smallest j
            best[i] += m
    i = int(np.argmax(best))                                         # the smallest i with the largest best
    out = []
    while i >= 0:
        out.append(i)
        i = int(pred[i])
    return out[::-1]


def anchors_once(sX, sY, trim, softMask, params):
    """Steps 1-5: (runs [(x, y, length)], counts dict)."""
    seed, span = params["seed"], len(params["seed"])
    score = np.array(params["scores"], dtype=np.int64).reshape(5, 5)
    hits = seed_hits(sX, sY, seed, params["maxSeedOccurrences"], softMask)
    cx, cy = _CODE[_bytes(sX)], _CODE[_bytes(sY)]
    hsps = set()
    for x, y in hits:
        h = extend_hit(cx, cy, x, y, span, score, params["xDrop"])
        if h[3] >= params["hspThreshold"]:
            hsps.add(h)                                   # (x, y, length) decides the score: exact duplicates collapse
    found = len(hsps)
    capped = found > params["maxHsps"]
    if capped:                                            # step 3
        hsps = sorted(hsps, key=lambda h: (-h[3], h[0], h[1], h[2]))[:params["maxHsps"]]
    hsps = sorted(hsps, key=lambda h: (h[0], h[1], h[2]))
    picked = chain(hsps)
    runs = [(hsps[i][0] + trim, hsps[i][1] + trim, hsps[i][2] - 2 * trim) for i in picked if hsps[i][2] - 2 * trim > 0]
    return runs, dict(hits=len(hits), hsps=found, chained=len(picked), capped=int(capped))


def _gaps(runs, lX, lY):
    """(pX, pY, x, y) of the rectangle in front of every run and behind the last."""
    pX = pY = 0
    for x, y, length in list(runs) + [(lX, lY, 0)]:
        yield pX, pY, x, y
        pX, pY = x + length, y + length


def find_anchor_runs(sX, sY, trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
                     repeatMaskMatrixBiggerThanThis=500 * 500, params=None):
    """Step 6 around steps 1-5 (impl/pairwiseAligner.c:1162-1196 with this finder in lastz's place)."""
    params = params or default_params()
    lX, lY = len(sX), len(sY)
    st = dict(hits=0, hsps=0, chained=0, runs=0, anchorColumns=0, subProblems=0, largestGapTop=lX * lY, largestGap=lX * lY,
              capped=0)
    if lX * lY <= anchorMatrixBiggerThanThis or lX == 0 or lY == 0:
        return np.zeros((0, 4), dtype=np.int64), st
    top, c = anchors_once(sX, sY, trim, True, params)
    for k in ("hits", "hsps", "chained"):
        st[k] += c[k]
    st["capped"] |= c["capped"]
    st["largestGapTop"] = max((x - pX) * (y - pY) for pX, pY, x, y in _gaps(top, lX, lY))
    out = []
    for j, (pX, pY, x, y) in enumerate(_gaps(top, lX, lY)):
        matrix = (x - pX) * (y - pY)
        if matrix > anchorMatrixBiggerThanThis:
            sub, c = anchors_once(sX[pX:x], sY[pY:y], trim, matrix > repeatMaskMatrixBiggerThanThis, params)
            for k in ("hits", "hsps", "chained"):
                st[k] += c[k]
            st["capped"] |= c["capped"]
            st["subProblems"] += 1
            out += [(pX + a, pY + b, length) for a, b, length in sub]
        if j < len(top):
            out.append(top[j])
    st["runs"] = len(out)
    st["anchorColumns"] = sum(r[2] for r in out)
    st["largestGap"] = max((x - pX) * (y - pY) for pX, pY, x, y in _gaps(out, lX, lY))
    runs = np.array([(x, y, length, expansion) for x, y, length in out], dtype=np.int64).reshape(-1, 4)
    return runs, st


def runs_to_anchors(runs):
    return [(int(x) + k, int(y) + k, int(e)) for x, y, length, e in np.asarray(runs).reshape(-1, 4) for k in range(int(length))]
