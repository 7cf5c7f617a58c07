"""What the band-edge statistic (cpecan_batch_set_band_edge) costs at download: a BASELINE config-4-like
batch (cPecanRealign mode: mixed lengths, expansion 4, split at 10, ragged ends, REWEIGHT | ORDERED) is uploaded and run once,
then run + download is repeated with the switch off and on, alternating, in ONE process.  Prints the median and range of the
download stage's wall time for either setting, their difference, and the pairs and problems the kernel saw; checks that the
lists are the same bytes with and without the switch.
Usage: python tools/band_edge_bench.py [pairs] [repeats] >> profiles/band_edge.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpecan_amd import api, workload  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    problems = workload.config_problems("4", range(n))
    cfg = workload.CONFIGS["4"]
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"], splitMatrixBiggerThanThis=cfg.get("split", 10))
    times = {False: [], True: []}
    with api.Batch(api.stateMachine5_construct(), p) as b:
        b.set_post(api.POST_REWEIGHT | api.POST_ORDERED, 0.5, 0.85)
        b.add_many_runs(problems)
        b.upload()
        b.run()
        b.download()  # warm: result buffers, consumer scratch
        first = b.result(n // 2).copy()
        flagged = pairs = 0
        for rep in range(repeats):
            for on in (False, True):
                b.set_band_edge(on)
                b.run()
                t0 = time.perf_counter()
                b.download()
                times[on].append(1e3 * (time.perf_counter() - t0))
                assert (b.result(n // 2) == first).all()
        st = b.stats()
        edges = [b.band_edge(i) for i in range(n)]
        flagged = sum(e["edgeScoreSum"] >= 10 ** 6 for e in edges)
        pairs = sum(e["edgePairs"] for e in edges)
    off, on = statistics.median(times[False]), statistics.median(times[True])
    print("band_edge_bench: config 4, %d problems, %d regions, %d emitted pairs, %d edge pairs, %d problems with edgeScoreSum >= 1e6; "
          "wall time of download(), which first waits for the sweep, over %d repeats: switch off median %.2f ms (%.2f .. %.2f), on median %.2f ms (%.2f .. %.2f), "
          "difference %.2f ms (kernel time of the sweeps %.2f ms)" %
          (n, st.regions, st.pairs, pairs, flagged, repeats, off, min(times[False]), max(times[False]), on, min(times[True]),
           max(times[True]), on - off, st.kernelMs), flush=True)


if __name__ == "__main__":
    main()
