"""Kernel time of the anchor stage with seedTransitions off and on in one process (cpecan_anchor_stats.kernelMs: HIP events
around the anchor kernels of both passes), and the stage's share of a getAlignedPairs-style call (Batch.add_many_unanchored
+ upload + run + download: anchor kernels beside the DP kernels, as profiles/anchor_stage.txt), on the three ENCODE pairs
and on 256 seeded 3 kb pairs.  Every figure: smallest, median and largest of `repeats` calls, off and on interleaved.
Usage: python tools/anchor_transitions_bench.py [repeats] [off] [--transitionHspThreshold N]
off: only the off case, for a library without the option.  --transitionHspThreshold N: a third case, mode 2, which is
seedTransitions 1 with cpecan_anchor_options.transitionHspThreshold = N."""
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
    argv = list(sys.argv[1:])
    threshold = None
    if "--transitionHspThreshold" in argv:
        at = argv.index("--transitionHspThreshold")
        threshold = int(argv[at + 1])
        del argv[at:at + 2]
    repeats = int(argv[0]) if argv else 7
    modes = (0,) if "off" in argv[1:] else (0, 1) if threshold is None else (0, 1, 2)
    params = {0: api.anchor_params_default()}
    options = {0: None, 1: None}
    if 1 in modes:
        params[1] = api.anchor_params_default(seedTransitions=1)
    if 2 in modes:
        params[2] = params[1]
        options[2] = api.anchor_options(transitionHspThreshold=threshold)
    cases = [("ENCODE human / chimp", [rc.encode_human_chimp()[:2]]), ("ENCODE human / dog", [rc.encode_human_other("dog")[:2]]),
             ("ENCODE human / mouse", [rc.encode_human_other("mouse")[:2]]),
             ("256 seeded 3 kb pairs", [ac.random_pair(1000 + i, 3000) for i in range(256)])]
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct()
    api.find_anchor_runs_many(cases[1][1])  # first call: module load, pools
    print("library %s; ms as min median max of %d calls" % (api.LIB_PATH, repeats))
    if threshold is not None:
        print("seedTransitions 2 stands for seedTransitions 1 with transitionHspThreshold %d" % threshold)
    for name, problems in cases:
        ms = {t: [] for t in modes}
        st = {}
        for _ in range(repeats):
            for t in modes:
                _, stats = api.find_anchor_runs_many(problems, params=params[t], options=options[t])
                ms[t].append(stats[0]["kernelMs"])
                st[t] = stats
        for t in modes:
            print("%-22s problems %4d  seedTransitions %d  anchor kernels %s ms  hits %d  hsps %d  runs %d  anchor columns %d  "
                  "gaps searched %d" % (name, len(problems), t, spread(ms[t]), sum(s["hits"] for s in st[t]),
                                        sum(s["hsps"] for s in st[t]), sum(s["runs"] for s in st[t]),
                                        sum(s["anchorColumns"] for s in st[t]), sum(s["subProblems"] for s in st[t])), flush=True)
        for t in modes:
            anchor, dp, cells = [], [], 0
            for _ in range(3):
                with api.Batch(sm, p) as b:
                    _, stats = b.add_many_unanchored([(sx, sy, True, True) for sx, sy in problems], params=params[t],
                                                          options=options[t])
                    b.upload()
                    b.run()
                    b.download()
                    s = b.stats()
                    anchor.append(stats[0]["kernelMs"])
                    dp.append(s.kernelMs)
                    cells = s.cells
            print("%-22s problems %4d  seedTransitions %d  in a call: anchor kernels %8.3f ms  DP kernels %9.3f ms  share %5.1f %%  "
                  "band cells %d" % (name, len(problems), t, min(anchor), min(dp), 100.0 * min(anchor) / (min(anchor) + min(dp)),
                                     cells), flush=True)


if __name__ == "__main__":
    main()
