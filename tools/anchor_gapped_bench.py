"""Kernel time of the anchor stage with gappedExtension off and on in one process (cpecan_anchor_stats.kernelMs: HIP events
around the anchor kernels of both passes), and the DP kernels' time and band cells of a getAlignedPairs-style call on the
anchors either gives (Batch.add_many_unanchored + upload + run + download), on the three ENCODE pairs and on 256 seeded
3 kb pairs.  Every anchor figure: smallest, median and largest of `repeats` calls, off and on interleaved.
Usage: python tools/anchor_gapped_bench.py [repeats]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_cases as ac  # noqa: E402
import reference_cases as rc  # noqa: E402
from cpecan_amd import api  # noqa: E402


def spread(v):
    return "%8.3f %8.3f %8.3f" % (min(v), statistics.median(v), max(v))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    options = {0: None, 1: api.anchor_options(gappedExtension=1)}
    cases = [("ENCODE human / chimp", [rc.encode_human_chimp()[:2]]), ("ENCODE human / dog", [rc.encode_human_other("dog")[:2]]),
             ("ENCODE human / mouse", [rc.encode_human_other("mouse")[:2]]),
             ("256 seeded 3 kb pairs", [ac.random_pair(1000 + i, 3000) for i in range(256)])]
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    for g in (0, 1):
        api.find_anchor_runs_many(cases[1][1], options=options[g])  # first calls: module load, pools
    print("library %s; ms as min median max of %d calls" % (api.LIB_PATH, repeats))
    for name, problems in cases:
        ms, st = {0: [], 1: []}, {}
        for _ in range(repeats):
            for g in (0, 1):
                _, stats = api.find_anchor_runs_many(problems, options=options[g])
                ms[g].append(stats[0]["kernelMs"])
                st[g] = stats
        for g in (0, 1):
            print("%-22s problems %4d  gappedExtension %d  anchor kernels %s ms  chained %d  runs %d  anchor columns %d  "
                  "gaps searched %d" % (name, len(problems), g, spread(ms[g]), sum(s["chained"] for s in st[g]),
                                        sum(s["runs"] for s in st[g]), sum(s["anchorColumns"] for s in st[g]),
                                        sum(s["subProblems"] for s in st[g])), flush=True)
        for g in (0, 1):
            anchor, dp, cells = [], [], 0
            for _ in range(3):
                with api.Batch(sm, p) as b:
                    _, stats = b.add_many_unanchored([(sx, sy, True, True) for sx, sy in problems], options=options[g])
                    b.upload()
                    b.run()
                    b.download()
                    s = b.stats()
                    anchor.append(stats[0]["kernelMs"])
                    dp.append(s.kernelMs)
                    cells = s.cells
            print("%-22s problems %4d  gappedExtension %d  in a call: anchor kernels %8.3f ms  DP kernels %9.3f ms  share %5.1f %%  "
                  "band cells %d" % (name, len(problems), g, min(anchor), min(dp), 100.0 * min(anchor) / (min(anchor) + min(dp)),
                                     cells), flush=True)


if __name__ == "__main__":
    main()
