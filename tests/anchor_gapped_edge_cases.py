"""Inputs that take the gapped extension to its edges, shared by the CPU suite
(tests/test_anchor_gapped_edges_cpu.py: what every input is for, asserted with the model alone) and the GPU suite
(tests/test_gpu_anchor_gapped_edges.py: the kernels against the model).  Nothing here touches a device.

    BAND        both edges of the band: insertions (lane 1's side, diagonal -31) and deletions (lane 63's side, +31)
    MASKED      N and lower case inside a gap that only an extension crosses
    long_gap    one gap with an indel every 150 bases: many blocks on the way back, the diagonal limit, yDrop at its ends
    limit_gap   the same with m + n > 4096: the limit binds on both extensions of one gap and the overlap rule decides
    tie_gap     a gap that reads the same from both ends around a homopolymer: equal bests, different columns
    source_tie_gap  a gap whose way back passes an I cell with two equal sources
    ZERO_ROWS   problems whose pass has no scratch rows
    sliced_*    a batch whose top-level pass needs three launches over the scratch

A case of BAND and MASKED is (sX, sY) as bytes; the options travel in the tests."""
import functools

import numpy as np

import anchor_gapped_cases as gc
from anchor_gapped_cases import X, conserved, random_bases
from cpecan_amd.workload import splitmix64

# cpecan_internal.h: CPK_ANCHOR_GAPPED_BUDGET_ROWS, the scratch rows of one launch (256 MiB of 64-byte rows).  This is the
# one place the tests state it; the launches the library makes with it are what test_gpu_anchor_gapped_edges.py checks.
BUDGET_ROWS = 4 << 20


# ---- 1. both band edges ----
def insertion(k):
    """Y has k bases X does not, then the conserved copy of the rest: crossing them puts the rest on diagonal -k, the side
    of the band whose outermost cell (lane 1) has no neighbour below."""
    return X.encode(), (X[:250] + random_bases(900 + k, k) + conserved(X[250:])).encode()


def swapped(pair):
    return pair[1], pair[0]


BAND = {
    "insertion of 3": insertion(3),
    "insertion of 31": insertion(31),
    "insertion of 32": insertion(32),
    "deletion of 31, swapped": swapped(gc.deletion(31)),
    "deletion of 32, swapped": swapped(gc.deletion(32)),
}

# ---- 2. N and lower case inside a gap ----
_C = conserved(X[253:])
MASKED = {
    "N in Y": (X.encode(), (X[:250] + _C[:100] + "N" * 10 + _C[110:]).encode()),
    "lower case in Y": (X.encode(), (X[:250] + _C[:60] + _C[60:160].lower() + _C[160:]).encode()),
    "N in X, lower case in Y": ((X[:300] + "N" * 5 + X[305:]).encode(), (X[:250] + _C[:80] + _C[80:120].lower() + _C[120:]).encode()),
}


# ---- 3. a long gap ----
def _indel_middle(seed, s, every=150):
    """The conserved copy of s, cut every `every` bases by an indel of 1 to 8: a deletion (bases of s left out), then an
    insertion (bases s does not have), in turn.  The sizes keep every piece within a few diagonals of the first."""
    out, at, k = [], 0, 0
    while at < len(s):
        out.append(conserved(s[at:at + every]))
        at += every
        size = 1 + (5 * k) % 8
        if k % 2 == 0:
            at += size
        else:
            out.append(random_bases(seed + 100 + k, size))
        k += 1
    return "".join(out)


@functools.lru_cache(maxsize=None)
def long_gap(seed=777, middle=1900):
    """An exact head and tail of 120 around `middle` conserved bases with an indel every 150: one gap whose extensions
    cross a dozen indels, with m + n under 4096."""
    s = random_bases(seed, 240 + middle)
    head, mid, tail = s[:120], s[120:120 + middle], s[120 + middle:]
    return s.encode(), (head + _indel_middle(seed, mid) + tail).encode()


def limit_gap():
    """The same with a middle of 2400: m + n > 4096, so neither extension crosses the gap and they meet inside it."""
    return long_gap(778, 2400)


def tie_gap():
    """A gap both of whose strings read the same from either end, so that the two extensions are one walk and tie: in X
    u H AAA H' u', in Y the conserved copy of H, AA, and its reverse (H' and u' being H and u reversed).  The flanks lie on
    the diagonals 0 and +7 and the two halves on +3 and +4.  Which A has no partner is open: each walk leaves out the one
    it meets first, so the right extension's blocks are not the left one's, and the rule's choice shows in the runs."""
    left, right, u = random_bases(31, 150), random_bases(32, 150), "GCA"
    h = random_bases(33, 61)
    hc = conserved(h)
    gx = u + h + "AAA" + h[::-1] + u[::-1]
    gy = hc + "AA" + hc[::-1]
    assert gx == gx[::-1] and gy == gy[::-1]
    return (left + gx + right).encode(), (left + gy + right).encode()


def source_tie_gap():
    """A gap in which the I state of a cell on the way back has two sources of one value, opening a gap there or extending
    the one opened earlier: the blocks (0, 0, 19), (21, 19, 3), (25, 22, 13) and (0, 0, 22), (25, 22, 13) score the same.
    The tie goes to M, which gives the first.  Found by a search over short strings with N.  Ten N in X on either side of
    the gap end the two HSPs at its corners (ten columns of -100 pass the x-drop), so the gap is exactly these strings."""
    left, right = random_bases(41, 150), random_bases(42, 150)
    gx = "N" * 10 + "TACCCTCCCNNCGCGGANTAGCTAAACA" + "N" * 10
    gy = "AATAATTAGC" + "TACCCTCCCCGCGAGTAGCTAAACA" + "CCGCCTTCAT"
    return (left + gx + right).encode(), (left + gy + right).encode()


LONG_OPTIONS = {"default": {}, "64 diagonals": dict(gappedMaxDiagonals=64), "1000 diagonals": dict(gappedMaxDiagonals=1000),
                "yDrop 1": dict(yDrop=1), "yDrop 2^31 - 1": dict(yDrop=2 ** 31 - 1)}


# ---- 5. passes without rows ----
def zero_row_problems():
    """All beyond 500 x 500, so they are searched.  Only the identical pair has an HSP, and its two gaps are 0 x 0."""
    a, b = random_bases(5007, 1500), random_bases(5008, 1500)
    return {"unrelated": (a.encode(), b.encode()),
            "identical": (a.encode(), a.encode()),
            "shorter than the seed": (random_bases(5003, 15).encode(), random_bases(5004, 40000).encode()),
            "all N": (b"N" * 1500, b.encode()),
            "lower case": (a.lower().encode(), a.lower().encode())}


# ---- 6. a pass over the scratch budget ----
@functools.lru_cache(maxsize=None)
def sliced_template(t):
    """Five exact 80-base parts with four gaps of 2100 between them (gap 1 of an odd template: 1400).  A gap starts with
    160 conserved bases that lose g + 1 of them on the way, the rest is unrelated.  The HSP of a part runs on into the
    stretch up to the deletion, so a gap between two parts has m + n of about 4050 (2650 in the short one), twice that in
    scratch rows, and a right extension that crosses the deletion to win."""
    seed = 6000 + 100 * t
    x, y = [], []
    for g in range(5):
        part = random_bases(seed + g, 80)
        x.append(part)
        y.append(part)
        if g == 4:
            break
        width = 1400 if t % 2 == 1 and g == 1 else 2100
        stretch = random_bases(seed + 10 + g, 160)
        x.append(stretch + random_bases(seed + 20 + g, width - 160))
        y.append(conserved(stretch[:70] + stretch[70 + g + 1:]) + random_bases(seed + 30 + g, width - 160))
    return "".join(x).encode(), "".join(y).encode()


SLICED_TEMPLATES = 8
SLICED_ROUNDS = 35


def sliced_orders(rounds=SLICED_ROUNDS):
    """The order of the eight templates in every round: a permutation of its own per round, turned by one where it would
    start with the template the round before ended with."""
    out = []
    for r in range(rounds):
        order = [int(v) for v in np.argsort(splitmix64(9100 + r, np.arange(SLICED_TEMPLATES, dtype=np.uint64)), kind="stable")]
        if out and out[-1][-1] == order[0]:
            order = order[1:] + order[:1]
        out.append(order)
    return out


def sliced_slots(rounds=SLICED_ROUNDS):
    """The template of every slot of the batch."""
    return [t for order in sliced_orders(rounds) for t in order]
