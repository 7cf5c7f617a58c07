"""What the gapped extension of the local chains (cpecan_find_local_chains_many_gapped) costs
and what it buys, on the problems of tools/local_chains_bench.py (whose figures at K = 1, 4 and 16 are in
profiles/local_chains.txt): per case and K

    anchor-kernel time (kernelMs) of a call with the option off and on, alternating in one process, median of REPEATS calls;
    the chains' runs, aligned columns and largest gap rectangle (between two consecutive runs of a chain) off and on;
    the DP kernel time of the batch that realigns the chains: every chain with runs is one problem, the sub-sequences from
    the start of its first run to the end of its last (what cpecan_cigar_from_local_chain spans) banded on its runs at
    expansion 20, as the realigner bands on the cigar -- cpecan_stats.kernelMs of one run, median of REPEATS runs.

Usage: python tools/local_chains_gapped_bench.py > profiles/local_chains_gapped.txt"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cpecan_amd import api, local  # noqa: E402
import local_chains_bench as base  # noqa: E402

REPEATS = 7
EXPANSION = 20


def shape(chains):
    """(chains, runs, aligned columns, largest gap rectangle) over all problems."""
    runs = cols = gap = n = 0
    for mine in chains:
        for c in mine:
            r = c["runs"]
            n += 1
            runs += len(r)
            cols += int(r[:, 2].sum()) if len(r) else 0
            for a, b in zip(r, r[1:]):
                gap = max(gap, int((b[0] - a[0] - a[2]) * (b[1] - a[1] - a[2])))
    return n, runs, cols, gap


def dp_problems(problems, chains):
    """The DP problems of the realign batch: per chain with runs (sub X, sub Y in the chain's orientation, anchors)."""
    out = []
    for (sx, sy), mine in zip(problems, chains):
        sx, sy = api._bytes(sx), api._bytes(sy)
        rc = None
        for c in mine:
            r = c["runs"].copy()
            if not len(r):
                continue
            if c["strand"] == "minus" and rc is None:
                rc = api.reverse_complement(sy)
            y = rc if c["strand"] == "minus" else sy
            x0, y0, x1, y1 = int(r[0][0]), int(r[0][1]), int(r[-1][0] + r[-1][2]), int(r[-1][1] + r[-1][2])
            r[:, 0] -= x0
            r[:, 1] -= y0
            r[:, 3] = EXPANSION
            out.append((sx[x0:x1], y[y0:y1], api.runs_to_anchors(r)))
    return out


def dp_kernel_ms(dp):
    if not dp:
        return 0.0, 0
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=EXPANSION)
    with api.Batch(api.stateMachine5_construct(api.fiveState), p) as b:
        b.add_many(dp)
        b.upload()
        times = []
        for k in range(REPEATS + 1):                                        # the first run warms up
            b.run()
            b.download()                                                    # the kernel time is read behind the download
            s = b.stats()
            times.append(s.kernelMs)
    return statistics.median(times[1:]), s.cells


def main():
    if api.device_count() < 1:
        raise SystemExit("needs a GPU")
    print("local chains, gapped extension off / on: anchor-kernel time and DP kernel time of the realign batch,")
    print("median of %d, ms; trim 0, strand both, expansion %d" % (REPEATS, EXPANSION))
    for name, problems, params in base.workloads():
        print(name)
        for k in (1, 4, 16):
            o = local.local_options(maxChains=k)
            times, got = {False: [], True: []}, {}
            for g in (False, True):                                         # warm-up
                local.find_local_chains(problems, trim=0, params=params, options=o, strand="both", gapped=g)
            for _ in range(REPEATS):
                for g in (False, True):
                    got[g], st = local.find_local_chains(problems, trim=0, params=params, options=o, strand="both", gapped=g)
                    times[g].append(st[0]["kernelMs"])
            off, on = statistics.median(times[False]), statistics.median(times[True])
            print("  K = %-2d  anchor kernels: off %9.3f   on %9.3f   x %.2f" % (k, off, on, on / off))
            for g in (False, True):
                print("          %s  chains %d, runs %d, aligned columns %d, largest gap rectangle %d; DP kernel %9.3f, band cells %d"
                      % (("on " if g else "off",) + shape(got[g]) + dp_kernel_ms(dp_problems(problems, got[g]))))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
