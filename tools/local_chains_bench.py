"""Anchor-kernel time (kernelMs) of cpecan_find_local_chains_many against the path that was
there before it, cpecan_find_anchor_runs_many_stranded with BOTH, on the same problems in the same process, alternating:

    pairs     256 pairs of 3 kb (cpecan_amd/workload.py: 5 % substitutions, 2 % + 2 % indels), default parameters
    inversion X = A B C, Y = A' rc(B') C' at 10 % substitutions, scaled to 100 kb, default parameters
    pool      one 60 kb pair at 10 % substitutions with an indel every ~100 bases, under parameters that fill the pool to the
              maxHsps cap of 4096 (short seed, x-drop under one mismatch): the chain recurrence at its largest

K = 1 is the yardstick (same pools, one chain per orientation there, one round here); then K = 4 and K = 16.  Every figure is
the median of REPEATS calls; the two entry points alternate call by call.  Usage: python tools/local_chains_bench.py > profiles/local_chains.txt"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpecan_amd import api, local  # noqa: E402
from cpecan_amd.workload import make_pair  # noqa: E402

REPEATS = 7
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def mutate(rng, s, sub=0.10, indel_every=0):
    s = s.copy()
    hit = rng.random(len(s)) < sub
    s[hit] = ACGT[(np.searchsorted(ACGT, s[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    if indel_every:
        keep = np.ones(len(s), dtype=bool)
        keep[indel_every - 1::2 * indel_every] = False                  # a deletion, then an insertion, in turn
        s = s[keep]
        at = np.arange(2 * indel_every - 1, len(s), 2 * indel_every)
        s = np.insert(s, at, ACGT[rng.integers(0, 4, len(at))])
    return s


def workloads():
    rng = np.random.default_rng(11)
    pairs = [make_pair(seed=77, index=i, length=3000, expansion=20)[:2] for i in range(256)]
    seg = 100000 // 3
    a, b, c = (rand_seq(rng, seg) for _ in range(3))
    x = np.concatenate([a, b, c]).tobytes()
    y = mutate(rng, a).tobytes() + mutate(rng, b).tobytes().translate(COMP)[::-1] + mutate(rng, c).tobytes()
    px = rand_seq(rng, 60000)
    pool = (px.tobytes(), mutate(rng, px, 0.10, 100).tobytes())
    pool_params = api.anchor_params_default(seed="11111111", maxSeedOccurrences=3, xDrop=60, hspThreshold=700)
    return [("pairs: 256 x 3 kb", pairs, None), ("inversion: 100 kb", [(x, y)], None), ("pool: 60 kb, capped", [pool], pool_params)]


def main():
    if api.device_count() < 1:
        raise SystemExit("needs a GPU")
    print("local chains: anchor-kernel time, median of %d calls, ms" % REPEATS)
    for name, problems, params in workloads():
        old, new = [], {1: [], 4: [], 16: []}
        chains = {}
        api.find_anchor_runs_many_stranded(problems, trim=0, params=params, strand="both")       # warm-up: caches, code objects
        for _ in range(REPEATS):
            _, stats, _ = api.find_anchor_runs_many_stranded(problems, trim=0, params=params, strand="both",
                                                             anchorMatrixBiggerThanThis=10 ** 15)
            old.append(stats[0]["kernelMs"])
            for k in new:
                got, st = local.find_local_chains(problems, trim=0, params=params, options=local.local_options(maxChains=k),
                                                  strand="both")
                new[k].append(st[0]["kernelMs"])
                chains[k] = (sum(len(c) for c in got), max(s["hspsPlus"] for s in st), max(s["hspsMinus"] for s in st),
                             max(s["rounds"] for s in st))
        base = statistics.median(old)
        print("%s" % name)
        print("  stranded BOTH (one chain per orientation, the path before)   %9.3f" % base)
        for k in new:
            m = statistics.median(new[k])
            print("  local K = %-2d  %9.3f   x %.2f   chains %d, largest pools %d / %d, most rounds %d"
                  % (k, m, m / base, chains[k][0], chains[k][1], chains[k][2], chains[k][3]))


if __name__ == "__main__":
    main()
