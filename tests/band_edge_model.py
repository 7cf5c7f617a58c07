"""The band-edge statistic (cpecan_band_edge, include/cpecan_hip.h) stated in Python over the
oracle's band and split points, for tests/test_band_edge_cpu.py, tests/test_gpu_band_edge.py and
tests/test_gpu_realign_adaptive.py.  Integers only, so every comparison is exact.  Nothing here touches a device.

A region is a rectangle of the oracle's split points with the anchors in front of its far corner's diagonal that no
earlier rectangle took (pairwiseAligner.c:1296-1308); its band is oracle_binding.band on those anchors.  A pair
(score, x, y) in problem coordinates lies in the one region whose rectangle holds it; it is cell (xs + 1, ys + 1) of that
region, on anti-diagonal d = xs + ys + 2 with x - y = xs - ys.  The cell is left-cut iff it is the band's first cell of d
and (x - 1, y + 1) is in the matrix, right-cut iff it is the last and (x + 1, y - 1) is in the matrix."""
import collections

import oracle_binding as ob

Region = collections.namedtuple("Region", "x1 y1 lX lY band")  # band[d] = (xmyL, xmyR)


def regions(problem, pkw):
    """The regions of (sX, sY, anchors, raggedLeft, raggedRight) under the parameters pkw."""
    sx, sy, anchors, rl, rr = problem
    p = ob.params(**pkw)
    anchors = [tuple(int(v) for v in a) + ((0,) if len(a) == 2 else ()) for a in anchors]
    out, at = [], 0
    for x1, y1, x2, y2 in ob.split_points(anchors, len(sx), len(sy), p.splitMatrixBiggerThanThis, rl, rr):
        own = []
        while at < len(anchors) and anchors[at][0] + anchors[at][1] < x2 + y2:
            own.append((anchors[at][0] - x1, anchors[at][1] - y1, anchors[at][2]))
            at += 1
        band = ob.band(own, x2 - x1, y2 - y1, p.diagonalExpansion, bool(p.dynamicAnchorExpansion))
        assert [d for d, _, _ in band] == list(range(x2 - x1 + y2 - y1 + 1))
        out.append(Region(x1, y1, x2 - x1, y2 - y1, tuple((lo, hi) for _, lo, hi in band)))
    assert at == len(anchors)
    return out


def is_cut(region, xs, ys):
    """Cell (xs + 1, ys + 1) of the region, for a pair (xs, ys) in region coordinates."""
    x, y = xs + 1, ys + 1
    lo, hi = region.band[x + y]
    assert lo <= x - y <= hi and (x - y - lo) % 2 == 0, "a pair outside its band"
    left = x - y == lo and x - 1 >= 0 and y + 1 <= region.lY
    right = x - y == hi and x + 1 <= region.lX and y - 1 >= 0
    return left or right


def edge_pairs(problem, pkw, pairs):
    """[(region index, score, x, y)] of the edge pairs among `pairs`, rows (score, x, y) in problem coordinates."""
    regs = regions(problem, pkw)
    out = []
    for s, x, y in ((int(v) for v in row) for row in pairs):
        inside = [k for k, r in enumerate(regs) if r.x1 <= x < r.x1 + r.lX and r.y1 <= y < r.y1 + r.lY]
        assert len(inside) == 1, "pair (%d, %d) lies in %d regions" % (x, y, len(inside))
        r = regs[inside[0]]
        if is_cut(r, x - r.x1, y - r.y1):
            out.append((inside[0], s, x, y))
    return out


def band_edge(problem, pkw, pairs):
    """{"edgePairs", "edgeScoreSum", "edgeScoreMax"} of a problem's list 0."""
    edges = edge_pairs(problem, pkw, pairs)
    return {"edgePairs": len(edges), "edgeScoreSum": sum(e[1] for e in edges), "edgeScoreMax": max([e[1] for e in edges], default=0)}


def predicted_round(stats_of_round, max_rounds, min_edge_score):
    """The round a cigar ends on: stats_of_round(k) is its statistic at expansion E * 2^k; round k + 1 runs iff round k left
    edgeScoreSum >= min_edge_score."""
    k = 0
    while k < max_rounds and stats_of_round(k)["edgeScoreSum"] >= min_edge_score:
        k += 1
    return k
