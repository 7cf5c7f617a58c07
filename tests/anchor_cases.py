"""Seeded inputs of the anchor-finder tests, shared by the CPU (model only) and GPU (model against the kernels) suites."""
import numpy as np

from cpecan_amd.workload import make_pair, splitmix64


def random_pair(index, length):
    """A seeded pair of cpecan_amd/workload.py: 5 % substitutions, 2 % deletions, 2 % insertions."""
    sx, sy, _ = make_pair(seed=1234, index=index, length=length, expansion=20)
    return sx, sy


def _stretches(seed, n, count, lo, hi):
    u = splitmix64(seed, np.arange(2 * count, dtype=np.uint64))
    for k in range(count):
        a = int(u[2 * k] % np.uint64(max(1, n - hi)))
        yield a, min(n, a + lo + int(u[2 * k + 1] % np.uint64(hi - lo + 1)))


def masked_pair(index, length):
    """The same with lower-case stretches (20-200 bases) and runs of N (1-30) laid over both sequences."""
    out = []
    for which, s in enumerate(random_pair(index, length)):
        b = bytearray(s)
        for a, e in _stretches(77 + 2 * index + which, len(b), max(2, len(b) // 400), 20, 200):
            b[a:e] = bytes(b[a:e]).lower()
        for a, e in _stretches(99 + 2 * index + which, len(b), max(1, len(b) // 1500), 1, 30):
            b[a:e] = b"N" * (e - a)
        out.append(bytes(b))
    return tuple(out)


def insertion_pair(index=7, flank=2500, insert=3000):
    """X = A + U + B, Y = A' + V + B' with U (1 kb) and V (`insert`) unrelated, and a 600-base lower-case stretch inside A
    and A': the top level (soft mask on) leaves gaps beyond 500 x 500, so the recursion fires."""
    ax, ay = random_pair(100 + index, flank)
    bx, by = random_pair(200 + index, flank)
    ux, _ = random_pair(300 + index, 1000)
    vy, _ = random_pair(400 + index, insert)
    ax = ax[:900] + ax[900:1500].lower() + ax[1500:]
    ay = ay[:900] + ay[900:1500].lower() + ay[1500:]
    return ax + ux + bx, ay + vy + by


def mixed_batch(n=256):
    """n problems of 300 to 3000 bases (the short ones stay under 500 x 500), every fourth one masked."""
    lengths = 300 + (splitmix64(4321, np.arange(n, dtype=np.uint64)) % np.uint64(2701)).astype(np.int64)
    return [(masked_pair if i % 4 == 3 else random_pair)(1000 + i, int(lengths[i])) for i in range(n)]
