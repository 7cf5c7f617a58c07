"""The hand-off from an ordered alignment to the anchor runs of the next E-step (include/cpecan_realign.h,
cpecan_batch_set_next_runs), stated in plain Python: what cpecan_next_runs_of_pairs and the kernel must equal.  Nothing here
touches the library."""


def blocks(pairs):
    """pairs: (x, y) of a chain in any order -> [(x0, y0, length)]: the maximal runs of consecutive pairs, sorted ascending,
    in which both coordinates step by one -- the match operations convertAlignedPairsToPairwiseAlignment makes."""
    xy = sorted((int(x), int(y)) for x, y in pairs)
    for (x1, y1), (x2, y2) in zip(xy, xy[1:]):
        assert x1 < x2 and y1 < y2, "not a chain"
    out = []
    for x, y in xy:
        if out and (out[-1][0] + out[-1][2], out[-1][1] + out[-1][2]) == (x, y):
            out[-1][2] += 1
        else:
            out.append([x, y, 1])
    return [tuple(b) for b in out]


def keeps(a, b):
    """matchFn (cPecanRealign.c:277-281): equal letters, case-insensitive, not N."""
    return a.upper() == b.upper() and a.upper() != "N"


def next_runs(pairs, sx, sy, trim, expansion):
    """[(x, y, length, expansion)]: per block, `trim` columns dropped at both ends, the columns with unequal letters or N
    dropped, and the kept columns that follow each other joined."""
    runs = []
    for x0, y0, n in blocks(pairs):
        run = None
        for k in range(trim, n - trim):
            if keeps(sx[x0 + k], sy[y0 + k]):
                if run is None:
                    run = [x0 + k, y0 + k, 0, expansion]
                    runs.append(run)
                run[2] += 1
            else:
                run = None
    return [tuple(r) for r in runs]
