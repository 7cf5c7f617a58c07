#!/usr/bin/env python3
"""Where the time of the multiple aligner's pairwise stage goes (profiles/set_alignment.txt).

Workload: --sets seeded sets (cpecan_amd.workload.make_fragment_set) of 8 fragments of 300 to 600 bp, every pair of every
set (impl/multipleAligner.c:668-681): 2000 sets are 56 000 problems.  One Sets.align over all of them -- one anchor batch,
one DP batch, the quintuple stage, one download -- against today's route for the first --single of the same pairs:
api.getAlignedPairs + api.reweightAlignedPairs2, one pair at a time, as multipleAligner.c:660-662 calls them.

    python tools/set_alignment_profile.py [--sets 2000] [--single 1000] [--seed 7]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cpecan_amd import api, sets  # noqa: E402
from cpecan_amd.workload import make_fragment_set  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=2000)
    ap.add_argument("--single", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    sM = api.stateMachine5_construct()
    p = api.pairwiseAlignmentBandingParameters_construct()
    t0 = time.perf_counter()
    frags = []  # (set, seq, left, right)
    for e in range(a.sets):
        frags += [(e, seq, left, right) for seq, left, right in make_fragment_set(a.seed, e)]
    t_gen = time.perf_counter() - t0
    lengths = [len(f[1]) for f in frags]
    print("workload: %d sets of 8 fragments, %d fragments of %d .. %d bp (mean %.0f), seed %d; generated in %.2f s"
          % (a.sets, len(frags), min(lengths), max(lengths), sum(lengths) / len(lengths), a.seed, t_gen))

    def run():
        with sets.Sets(sM, p, device=a.device) as s:
            t0 = time.perf_counter()
            for set_id, seq, left, right in frags:
                s.add_fragment(set_id, seq, left, right)
            pairs = s.pairs(sets.ALL)
            t1 = time.perf_counter()
            quints, offsets, sim = s.align(pairs)
            t2 = time.perf_counter()
            return pairs, quints, offsets, sim, s.timing, t1 - t0, t2 - t1

    run_small = a.sets > 20
    if run_small:  # the first call of a process pays for the runtime, the code objects and the memory pools
        keep, frags = frags, frags[:8 * 20]
        run()
        frags = keep
    pairs, quints, offsets, sim, tm, t_add, t_align = run()
    n = len(pairs)
    anchored = sum(1 for x, y in pairs.tolist() if lengths[x] * lengths[y] > api.ANCHOR_MATRIX_BIGGER_THAN_THIS)
    print("Sets.align: %d problems (%d past anchorMatrixBiggerThanThis), %d records, mean similarity %.4f"
          % (n, anchored, len(quints), float(sim.mean()) / api.PAIR_ALIGNMENT_PROB_1))
    print("  add_fragment + pairs (host, Python)   %9.1f ms" % (1e3 * t_add))
    print("  align, wall (Python call)             %9.1f ms   %8.2f us per pair" % (1e3 * t_align, 1e6 * t_align / n))
    print("    cpecan_sets_align, wall             %9.1f ms" % tm["totalMs"])
    print("      anchor batch, wall                %9.1f ms" % tm["anchorMs"])
    print("      add as runs + plan + upload, wall %9.1f ms" % tm["packMs"])
    print("      run + download, wall              %9.1f ms" % tm["downloadMs"])
    print("        DP kernels (HIP events)         %9.1f ms" % tm["dpKernelMs"])
    print("        quintuple stage (HIP events)    %9.3f ms" % tm["stageMs"])
    print("    numpy copies of the result          %9.1f ms" % (1e3 * t_align - tm["totalMs"]))

    m = min(a.single, n)
    by = [(frags[x], frags[y]) for x, y in pairs[:m].tolist()]
    api.reweightAlignedPairs2(api.getAlignedPairs(sM, by[0][0][1], by[0][1][1], p), len(by[0][0][1]), len(by[0][1][1]), 0.5)
    t0 = time.perf_counter()
    records = 0
    for fx, fy in by:
        l = api.getAlignedPairs(sM, fx[1], fy[1], p, fx[2] != fy[2], fx[3] != fy[3])
        l = api.reweightAlignedPairs2(l, len(fx[1]), len(fy[1]), 0.5)
        records += len(l)
    t_single = time.perf_counter() - t0
    print("one pair at a time (getAlignedPairs + reweightAlignedPairs2), the first %d of the same pairs:" % m)
    print("  wall                                  %9.1f ms   %8.2f us per pair" % (1e3 * t_single, 1e6 * t_single / m))
    print("  records of those pairs                %9d one at a time, %d in the batch" % (records, int(offsets[m])))
    print("per pair: %.2f us in one batch, %.2f us one at a time, ratio %.1f"
          % (1e6 * t_align / n, 1e6 * t_single / m, (t_single / m) / (t_align / n)))


if __name__ == "__main__":
    main()
