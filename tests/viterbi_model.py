"""The definition of Viterbi decoding (include/cpecan_viterbi.h) in numpy, one diagonal at a time: what
cpk_viterbi.inl must equal bit for bit.  The band and the split points are the oracle's (oracle_binding.band, split_points); the
transition list, the emissions and the start / end vectors are those of the oracle's Model, om.tr in list order.  Only IEEE
double additions and comparisons.  Nothing here touches a GPU or the library.

    viterbi(om, sx, sy, anchors, p, ragged_left, ragged_right) -> Model(logP, regions, ops, n_cells, ties)
        regions  Region tuples as cpecan_amd.viterbi gives them; ops int32[n, 2]; n_cells: band cells of all regions;
        ties: band cells in which a candidate equalled the best so far exactly (both finite)
    enumerate_paths(om, sx, sy, ragged_left, ragged_right) -> [(value, start_state, (state, ...))] of ONE region, every path
    replay(om, sx, sy, ragged_left, ragged_right, start_state, end_state, ops) -> the value accumulated in path order
"""
import collections

import numpy as np

import oracle_binding as ob

Region = collections.namedtuple("Region", "x1 y1 x2 y2 logP startState endState opOff nOps")
Model = collections.namedtuple("Model", "logP regions ops n_cells ties")

NEG_INF = float("-inf")
DX = (1, 1, 0)  # the step of a gap-X (block 0), match (1), gap-Y (2) transition
DY = (0, 1, 1)


def symbols(s):
    return np.array([4] + [ob.symbol(chr(c)) for c in bytes(s)], dtype=np.int64)  # 1-based: cell (x, y) sees s[x - 1]


def transitions(om):
    return [(t.block, t.frm, t.to, t.tP) for t in om.tr[:om.nTransitions]]


def block_of_state(om):
    """state -> block of the transitions that enter it (every state is entered by one kind of step)."""
    out = {}
    for block, _, to, _ in transitions(om):
        assert out.setdefault(to, block) == block
    return out


def vectors(om, ragged_left, ragged_right):
    S = om.S
    return (np.array((om.raggedStart if ragged_left else om.start)[:S]), np.array((om.raggedEnd if ragged_right else om.end)[:S]))


def band_of(anchors, lX, lY, p):
    if lX + lY == 0:
        return [(0, 0, 0)]
    return ob.band(anchors, lX, lY, p.diagonalExpansion, bool(p.dynamicAnchorExpansion))


def region(om, sx, sy, anchors, p, ragged_left, ragged_right):
    """One region: (logP, startState, endState, ops as a list of [state, length], n_cells, ties)."""
    S, lX, lY = om.S, len(sx), len(sy)
    N = lX + lY
    cx, cy = symbols(sx), symbols(sy)
    mE, xE, yE = np.array(om.matchEm[:]), np.array(om.gapXEm[:]), np.array(om.gapYEm[:])
    tr = transitions(om)
    startvec, endvec = vectors(om, ragged_left, ragged_right)
    band = band_of(anchors, lX, lY, p)
    assert band[0][1:] == (0, 0) and band[N][1:] == (lX - lY, lX - lY), "the first and last diagonal hold one cell"
    V, P = [startvec.reshape(1, S).copy()], [np.full((1, S), -1, dtype=np.int64)]
    n_cells, ties = 1, 0
    with np.errstate(invalid="raise"):
        for d in range(1, N + 1):
            _, lo, hi = band[d]
            xmy = np.arange(lo, hi + 1, 2)
            x, y = (d + xmy) // 2, (d - xmy) // 2
            assert x.min() >= 0 and y.min() >= 0 and x.max() <= lX and y.max() <= lY
            w = len(xmy)
            best = np.full((w, S), NEG_INF)
            ptr = np.full((w, S), -1, dtype=np.int64)
            tied = np.zeros(w, dtype=bool)
            em = (xE[cx[x]], mE[cx[x] * 5 + cy[y]], yE[cy[y]])
            for block, frm, to, tP in tr:  # in list order
                sd = d - (2 if block == 1 else 1)
                if sd < 0:
                    continue
                _, slo, shi = band[sd]
                sxmy = xmy + (-1, 0, 1)[block]
                k = (sxmy - slo) // 2
                ok = (sxmy >= slo) & (sxmy <= shi)  # a source outside the matrix or the band is skipped
                src = np.where(ok, V[sd][np.clip(k, 0, len(V[sd]) - 1), frm], NEG_INF)
                cand = src + (em[block] + tP)
                tied |= ok & (cand == best[:, to]) & (cand > NEG_INF)
                take = ok & (cand > best[:, to])  # strict: the first transition in list order wins a tie
                best[:, to] = np.where(take, cand, best[:, to])
                ptr[:, to] = np.where(take, frm, ptr[:, to])
            V.append(best)
            P.append(ptr)
            n_cells += w
            ties += int(tied.sum())
    logP, end_state = NEG_INF, -1
    for s in range(S):
        c = V[N][0, s] + endvec[s]
        if c > logP:
            logP, end_state = float(c), s
    if logP == NEG_INF:
        return NEG_INF, -1, -1, [], n_cells, ties
    blk = block_of_state(om)
    steps, s, x, y = [], end_state, lX, lY
    while x + y > 0:
        d = x + y
        frm = int(P[d][(x - y - band[d][1]) // 2, s])
        assert frm >= 0
        steps.append(s)
        x, y = x - DX[blk[s]], y - DY[blk[s]]
        s = frm
    assert (x, y) == (0, 0)
    steps.reverse()
    ops = []
    for t in steps:
        if ops and ops[-1][0] == t:
            ops[-1][1] += 1
        else:
            ops.append([t, 1])
    return logP, s, end_state, ops, n_cells, ties


def regions_of(anchors, lX, lY, p, ragged_left, ragged_right):
    """[(x1, y1, x2, y2, own anchors shifted, ragged_left, ragged_right)] as
    getPosteriorProbsWithBandingSplittingAlignmentsByLargeGaps cuts the problem (impl/pairwiseAligner.c:1273-1326)."""
    anchors = [tuple(int(v) for v in t) for t in anchors]
    rects = ob.split_points(anchors, lX, lY, p.splitMatrixBiggerThanThis, ragged_left, ragged_right)
    out, j = [], 0
    for i, (x1, y1, x2, y2) in enumerate(rects):
        own = []
        while j < len(anchors) and anchors[j][0] + anchors[j][1] < x2 + y2:
            a = anchors[j]
            assert x1 <= a[0] < x2 and y1 <= a[1] < y2
            own.append((a[0] - x1, a[1] - y1, a[2] if len(a) > 2 else 0))
            j += 1
        out.append((x1, y1, x2, y2, own, ragged_left or i > 0, ragged_right or i < len(rects) - 1))
    assert j == len(anchors)
    return out


def viterbi(om, sx, sy, anchors, p, ragged_left=False, ragged_right=False):
    sx, sy = bytes(sx), bytes(sy)
    total, regs, ops, n_cells, ties = None, [], [], 0, 0
    for x1, y1, x2, y2, own, rl, rr in regions_of(anchors, len(sx), len(sy), p, ragged_left, ragged_right):
        logP, s0, s1, rops, nc, nt = region(om, sx[x1:x2], sy[y1:y2], own, p, rl, rr)
        regs.append(Region(x1, y1, x2, y2, logP, s0, s1, len(ops), len(rops)))
        ops += rops
        total = logP if total is None else total + logP  # the plain double sum, region order
        n_cells += nc
        ties += nt
    return Model(total, tuple(regs), np.array(ops, dtype=np.int32).reshape(-1, 2), n_cells, ties)


def replay(om, sx, sy, ragged_left, ragged_right, start_state, end_state, ops):
    """v = startvec[start]; v = v + (e + tP) per step; v + endvec[end]: the additions of the recurrence along the path."""
    cx, cy = symbols(sx), symbols(sy)
    startvec, endvec = vectors(om, ragged_left, ragged_right)
    tP = {(frm, to): (block, t) for block, frm, to, t in transitions(om)}
    v, s, x, y = float(startvec[start_state]), start_state, 0, 0
    for to, length in np.asarray(ops).reshape(-1, 2):
        for _ in range(int(length)):
            block, t = tP[(s, int(to))]
            x, y = x + DX[block], y + DY[block]
            e = (om.gapXEm[cx[x]], om.matchEm[cx[x] * 5 + cy[y]], om.gapYEm[cy[y]])[block]
            v = v + (e + t)
            s = int(to)
    assert (x, y, s) == (len(sx), len(sy), end_state)
    return v + float(endvec[end_state])


def enumerate_paths(om, sx, sy, ragged_left, ragged_right):
    """Every state path of one region whose band is the whole matrix: (value accumulated in path order, end prior included; start
    state; the states of the steps).  Paths through -inf are included: their value is -inf."""
    lX, lY = len(sx), len(sy)
    cx, cy = symbols(sx), symbols(sy)
    startvec, endvec = vectors(om, ragged_left, ragged_right)
    tr = transitions(om)
    out = []

    def walk(v, s, x, y, s0, steps):
        if (x, y) == (lX, lY):
            out.append((v + float(endvec[s]), s0, tuple(steps)))
            return
        for block, frm, to, t in tr:
            nx, ny = x + DX[block], y + DY[block]
            if frm != s or nx > lX or ny > lY:
                continue
            e = (om.gapXEm[cx[nx]], om.matchEm[cx[nx] * 5 + cy[ny]], om.gapYEm[cy[ny]])[block]
            steps.append(to)
            walk(v + (e + t), to, nx, ny, s0, steps)
            steps.pop()

    for s0 in range(om.S):
        walk(float(startvec[s0]), s0, 0, 0, s0, [])
    return out
