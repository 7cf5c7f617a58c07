"""Constructed inputs of the gapped-extension tests, shared by the CPU suite (model only) and
the GPU suite (model against the kernels).  X is 500 random bases.  A CONSERVED copy of a stretch has every fifth base
replaced by a transversion: it scores about +50 a column under HOXD70 but holds no window of the 12-of-19 seed, so no HSP
starts there and only an extension can win it.  Every case is (sX, sY, options of the model as keywords)."""
import numpy as np

from cpecan_amd.workload import splitmix64

TRANSVERSION = {"A": "C", "C": "A", "G": "T", "T": "G"}


def random_bases(seed, n):
    u = splitmix64(seed, np.arange(n, dtype=np.uint64))
    return "".join("ACGT"[int(v % np.uint64(4))] for v in u)


def conserved(s, phase=0):
    """s with the bases at phase, phase + 5, ... transverted."""
    return "".join(TRANSVERSION[ch] if i % 5 == phase else ch for i, ch in enumerate(s))


X = random_bases(20250, 500)


def deletion(k):
    """Y = X[:250], then the conserved copy of X[250 + k:]: crossing the k-base deletion puts the rest on diagonal +k."""
    return X.encode(), (X[:250] + conserved(X[250 + k:])).encode()


def insertion_before():
    """The conserved part first, then 7 bases X does not have, then the exact part: a left extension crosses them."""
    return X.encode(), (conserved(X[:250]) + random_bases(7, 7) + X[250:]).encode()


def both_sides():
    """Two exact parts on different diagonals around a conserved middle that lies on a third: X[:200], 3 bases gone, the
    conserved copy of X[203:263], 2 bases gone, X[265:].  Both HSPs reach the middle with an extension of their own, and
    the overlap rule keeps one."""
    return X.encode(), (X[:200] + conserved(X[203:263]) + X[265:]).encode()


def touching(swap=False):
    """Y = X[:255] + X[258:], both parts exact: the two HSPs stop at the deletion (at 255 the bases next to it mismatch on
    either diagonal, so neither x-drop walk goes on and both are chained) and the gap between them is 3 x 0; swapped,
    0 x 3."""
    sx, sy = X.encode(), (X[:255] + X[258:]).encode()
    return (sy, sx) if swap else (sx, sy)


CASES = {
    "deletion of 3": deletion(3) + (dict(gapped=1),),
    "deletion of 31": deletion(31) + (dict(gapped=1),),
    "deletion of 32": deletion(32) + (dict(gapped=1),),
    "insertion before": insertion_before() + (dict(gapped=1),),
    "128 diagonals": deletion(3) + (dict(gapped=1, gappedMaxDiagonals=128),),
    "yDrop 100": deletion(3) + (dict(gapped=1, yDrop=100),),
    "both sides": both_sides() + (dict(gapped=1),),
    "touching, n = 0": touching() + (dict(gapped=1),),
    "touching, m = 0": touching(True) + (dict(gapped=1),),
}
