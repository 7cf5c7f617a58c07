"""A plain model of the per-diagonal band table the device builds (cpecan_build_diag_table and
cpecan_build_diag_table_wave, cpk_table_gather.inl), for tests/test_table_cases_cpu.py and tests/test_gpu_table.py.
Integers only, so every comparison is exact.  Nothing here touches a device.

The band comes from the oracle (oracle_binding.band on a region's own anchors), the regions from the oracle's split
points; everything else is derived here from the written rules:

  xmyL, width, cellOff   the oracle's band, and the running sum of its widths;
  segments               the traceback schedule of the reference (pairwiseAligner.c:791-810): a traceback starts on the
                         first diagonal d >= tracedBackTo + minDiagsBetweenTraceBack that is at most 2 E + 1 cells wide,
                         and on the last one; it emits down to tracedBackTo + 1 from d - (traceBackDiagonals + 1), from d
                         itself on the last diagonal;
  ringOff, whole region  cells: the diagonals are laid end to end and start again at 0 when pos + width > ringCap;
                         independently of that rule, the diagonals tbPrev .. dTop of every segment -- what the traceback
                         loop of Sweep::traceback walks (d2 = dTop down to tbPrev + 1, each step prefetching the ring row
                         of d2 - 1) and what host planning counts as live (plan_region, liveMax) -- must lie in pairwise
                         disjoint intervals inside [0, ringCap);
  ringOff, split region  doubles: every diagonal starts on an even double, its match row is padded to an even count, and
                         the S - 1 other rows are kept only on diagonal 0, on the refresh diagonals of the segment that
                         emits the diagonal ((tbFrom - d) % 10 == 0) and from one diagonal below the top of the segment
                         that covers it (d >= dTop - 1);
  dpos                   never computed here: checked against the contract in the header comment of
                         cpk_table_gather.inl (check_dpos below)."""
import collections

import numpy as np

import oracle_binding as ob

WAVE = 64            # CPK_WAVE
REFRESH_PERIOD = 10  # CPK_REFRESH_PERIOD
ABS_SLACK = 6        # CPK_ABS_SLACK
FIELDS = ("xmyL", "width", "ringOff", "cellOff")

# One DP region as the model sees it: its place in the problem, its own anchors (relative, (x, y, expansion)), the
# oracle's band as arrays over the diagonals, and what planning derives from the band.
Region = collections.namedtuple("Region", "x1 y1 lX lY anchors lo width cell_off segs max_width cells ring_cap smooth")


def schedule(width, min_between, tb_diagonals, expansion):
    """The traceback segments (tbPrev, dTop, tbFrom) of a band with these widths."""
    N, segs, traced_back_to = len(width) - 1, [], 0
    for d in range(1, N + 1):
        at_end = d == N
        if at_end or (d >= traced_back_to + min_between and width[d] <= 2 * expansion + 1):
            tb_from = d if at_end else d - (tb_diagonals + 1)
            segs.append((traced_back_to, d, tb_from))
            traced_back_to = tb_from
    return segs


def region_of(x1, y1, lX, lY, anchors, p):
    """anchors: relative to the region.  p: oracle_binding.Params."""
    band = ob.band(anchors, lX, lY, p.diagonalExpansion, bool(p.dynamicAnchorExpansion))
    assert [xay for xay, _, _ in band] == list(range(lX + lY + 1))
    lo = np.array([l for _, l, _ in band], dtype=np.int64)
    hi = np.array([r for _, _, r in band], dtype=np.int64)
    width = (hi - lo) // 2 + 1
    cell_off = np.concatenate([[0], np.cumsum(width)])
    segs = schedule(width, p.minDiagsBetweenTraceBack, p.traceBackDiagonals, p.diagonalExpansion)
    live = max([int(cell_off[top + 1] - cell_off[prev]) for prev, top, _ in segs], default=0)
    steps = [abs(int(v)) for v in np.diff(lo)] + [abs(int(v)) for v in np.diff(hi)]
    return Region(x1, y1, lX, lY, tuple(anchors), lo, width, cell_off, segs, int(width.max()), int(cell_off[-1]),
                  live + int(width.max()), not p.dynamicAnchorExpansion and all(s == 1 for s in steps))


def problem_regions(problem, pkw):
    """The regions of (sX, sY, anchors, raggedLeft, raggedRight): the rectangles of the oracle's split points, each with
    the anchors in front of its far corner's diagonal that no earlier rectangle took (pairwiseAligner.c:1296-1308)."""
    sx, sy, anchors, rl, rr = problem
    p = ob.params(**pkw)
    anchors = [tuple(int(v) for v in a) + ((0,) if len(a) == 2 else ()) for a in anchors]
    rects = ob.split_points(anchors, len(sx), len(sy), p.splitMatrixBiggerThanThis, rl, rr)
    out, at = [], 0
    for x1, y1, x2, y2 in rects:
        own = []
        while at < len(anchors) and anchors[at][0] + anchors[at][1] < x2 + y2:
            own.append((anchors[at][0] - x1, anchors[at][1] - y1, anchors[at][2]))
            at += 1
        out.append(region_of(x1, y1, x2 - x1, y2 - y1, own, p))
    assert at == len(anchors)
    return out


# ---- the two ring rules ----
def ring_whole(width, ring_cap):
    off, pos = [], 0
    for w in width:
        w = int(w)
        if pos + w > ring_cap:
            pos = 0
        off.append(pos)
        pos += w
    return off


def stores_every_state(d, segs):
    """A split region's diagonal d keeps all S rows, not the match row alone."""
    if d == 0:
        return True
    if not segs:
        return False
    emit_from = next((f for _, _, f in segs if f >= d), segs[-1][2])  # the segment that emits d
    cov_top = next((t for _, t, _ in segs if t >= d), segs[-1][1])    # the segment whose forward sweep covers d
    return (emit_from - d) % REFRESH_PERIOD == 0 or d >= cov_top - 1


def ring_split(width, segs, S):
    """(ringOff per diagonal, end of the last one), in doubles."""
    off, pos = [], 0
    for d, w in enumerate(width):
        w = int(w)
        off.append(pos)
        even = (w + 1) // 2 * 2
        pos += even + (w * (S - 1) if stores_every_state(d, segs) else 0)
    return off, pos


def ring_overlaps(ring_off, width, segs, ring_cap):
    """The first (segment, diagonal, diagonal) whose ring intervals collide or leave [0, ringCap) among the diagonals
    tbPrev .. dTop of a segment; None when every segment's live diagonals are apart."""
    for si, (prev, top, _) in enumerate(segs):
        spans = sorted((int(ring_off[d]), int(ring_off[d]) + int(width[d]), d) for d in range(prev, top + 1))
        if spans and (spans[0][0] < 0 or max(e for _, e, _ in spans) > ring_cap):
            return (si, spans[0][2], spans[-1][2])
        for (_, e0, d0), (b1, _, d1) in zip(spans, spans[1:]):
            if b1 < e0:
                return (si, d0, d1)
    return None


# ---- the lanes of the wave builder ----
def chunk_of(n_diagonals):
    return (n_diagonals + WAVE - 1) // WAVE


def lane_starts(n_diagonals):
    """First diagonal of every lane that has one."""
    c = chunk_of(n_diagonals)
    return [l * c for l in range(WAVE) if l * c < n_diagonals]


# ---- the position words ----
def danger_diagonals(lo, width, backward=False):
    """Where the contract demands a new base: the sweep's first diagonal, an edge that moved by other than one x-y step,
    an edge that turned back over positions it had left (low edge falls after rising, high edge rises after falling)."""
    hi = lo + 2 * (width - 1)
    order = list(range(len(lo)))[::-1] if backward else list(range(len(lo)))
    out = []
    for k, d in enumerate(order):
        must = k == 0
        if k >= 1:
            p1 = order[k - 1]
            must = must or abs(int(lo[d] - lo[p1])) != 1 or abs(int(hi[d] - hi[p1])) != 1
        if k >= 2:
            p2 = order[k - 2]
            must = must or (lo[d] < lo[p1] and lo[p1] > lo[p2]) or (hi[d] > hi[p1] and hi[p1] < hi[p2])
        if must:
            out.append(d)
    return out


def check_dpos(lo, width, dpos, max_width, fits=True):
    """The contract of dpos[d] = posF | flagF << 15 | posB << 16 | flagB << 31, per sweep direction.  With the even base
    B in force at d (B = lo - 2 pos, rounded down to even): (fits) the cells of d and of the one or two diagonals before
    it in sweep order sit at positions 1 .. P - 2, P = maxWidth + CPK_ABS_SLACK; flag 0 means the base of the diagonal
    before; the flag is set wherever danger_diagonals says so.  Returns a list of messages, empty when it holds.
    fits=False for a band whose edges jump (CpkRegion::absOk == 0: no sweep reads its positions, and three of its
    diagonals need not fit the rows)."""
    hi = lo + 2 * (width - 1)
    P, n, errs = max_width + ABS_SLACK, len(lo), []
    for name, shift, backward in (("forward", 0, False), ("backward", 16, True)):
        order = list(range(n))[::-1] if backward else list(range(n))
        must = set(danger_diagonals(lo, width, backward))
        base_before = None
        for k, d in enumerate(order):
            word = (int(dpos[d]) >> shift) & 0xffff
            pos, flag = word & 0x7fff, word >> 15
            B = (int(lo[d]) - 2 * pos) & ~1
            if fits:
                for q in order[max(0, k - 2):k + 1]:
                    first, last = (int(lo[q]) - B) >> 1, (int(hi[q]) - B) >> 1
                    if first < 1 or last > P - 2:
                        errs.append("%s dpos: diagonal %d under the base of diagonal %d sits at %d..%d, outside 1..%d"
                                    % (name, q, d, first, last, P - 2))
            if not flag and B != base_before:
                errs.append("%s dpos: diagonal %d has flag 0 but base %d after %s" % (name, d, B, base_before))
            if d in must and not flag:
                errs.append("%s dpos: diagonal %d must re-base (first, jump or turn-back) and has flag 0" % (name, d))
            base_before = B
    return errs


# ---- the whole table of a region, and the comparison ----
def expected_table(rg, split, S, ring_cap):
    """int64[nDiagonals, 4] of (xmyL, width, ringOff, cellOff) for the region as it was planned: split or whole, with
    the ring capacity the host gave a whole region."""
    ring = ring_split(rg.width, rg.segs, S)[0] if split else ring_whole(rg.width, ring_cap)
    return np.stack([rg.lo, rg.width, np.array(ring, dtype=np.int64), rg.cell_off[:-1]], axis=1)


def first_difference(got, want):
    """"diagonal d field f: got x, want y" for the first differing entry, or None."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    if got.shape != want.shape:
        return "table of %s entries, want %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    d, f = (int(v) for v in bad[0])
    return "diagonal %d field %s: got %d, want %d" % (d, FIELDS[f], got[d, f], want[d, f])


def check_region(rg, t, check_positions=True):
    """Everything the suite holds of one fetched table t (api.Batch.table) against the model's region rg.  Returns a list
    of messages, each naming the diagonal it is about; empty when the table is right."""
    errs = []
    S, split = t["nStates"], bool(t["split"])
    facts = dict(x1=rg.x1, y1=rg.y1, lX=rg.lX, lY=rg.lY, cells=rg.cells, maxWidth=rg.max_width, nSeg=len(rg.segs),
                 absOk=int(rg.smooth))
    if not split:
        facts["ringCap"] = rg.ring_cap
    for k, v in facts.items():
        if t[k] != v:
            errs.append("region fact %s: got %d, want %d" % (k, t[k], v))
    if [tuple(int(v) for v in s) for s in t["segs"]] != list(rg.segs):
        errs.append("segments: got %s, want %s" % (t["segs"].tolist(), rg.segs))
    if errs:
        return errs
    diff = first_difference(t["diags"], expected_table(rg, split, S, t["ringCap"]))
    if diff:
        errs.append(diff)
    ring_off = t["diags"][:, 2]
    if split:
        end = ring_split(rg.width, rg.segs, S)[1]
        if end > t["ringDoubles"]:
            errs.append("diagonal %d: the split ring ends at double %d, %d are reserved" % (rg.lX + rg.lY, end, t["ringDoubles"]))
        odd = np.flatnonzero(ring_off % 2)
        if len(odd):
            errs.append("diagonal %d: split ringOff %d is odd" % (odd[0], ring_off[odd[0]]))
    else:
        hit = ring_overlaps(ring_off, t["diags"][:, 1], rg.segs, t["ringCap"])
        if hit:
            errs.append("segment %d: diagonals %d and %d collide in the ring or leave it" % hit)
    if check_positions and t["dpos"] is not None:
        errs += check_dpos(rg.lo, rg.width, t["dpos"], rg.max_width, fits=rg.smooth)
    return errs
