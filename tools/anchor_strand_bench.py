"""Kernel time of the anchor stage with strand BOTH against PLUS in one process (cpecan_anchor_stats.kernelMs: HIP events
around the anchor kernels of both passes), best of `repeats` calls each, on the three ENCODE pairs and on the 256 mixed
problems of tests/anchor_cases.py.  Usage: python tools/anchor_strand_bench.py [repeats]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_cases as ac  # noqa: E402
import reference_cases as rc  # noqa: E402
from cpecan_amd import api  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cases = [("ENCODE human / chimp", [rc.encode_human_chimp()[:2]]), ("ENCODE human / dog", [rc.encode_human_other("dog")[:2]]),
             ("ENCODE human / mouse", [rc.encode_human_other("mouse")[:2]]), ("mixed_batch(256)", ac.mixed_batch(256))]
    api.find_anchor_runs_many_stranded(cases[1][1], strand="both")  # first call: module load, pools
    for name, problems in cases:
        ms = {}
        for strand in ("plus", "both", "plus", "both"):
            for _ in range(repeats):
                _, stats, _ = api.find_anchor_runs_many_stranded(problems, strand=strand)
                ms[strand] = min(ms.get(strand, 1e30), stats[0]["kernelMs"])
        print("%-22s problems %4d  anchor kernels PLUS %8.3f ms  BOTH %8.3f ms  ratio %.2f" %
              (name, len(problems), ms["plus"], ms["both"], ms["both"] / ms["plus"]), flush=True)


if __name__ == "__main__":
    main()
