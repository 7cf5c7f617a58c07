"""What Viterbi decoding costs at BASELINE config B -- 10 000 pairs of 2 kb, five-state, band 100, built with
cpecan_amd/workload.py as bench.py builds them -- beside the kernel time of a CPECAN_EMIT_MATCH batch over the same problems
in the same process on the same commit.  The sweep and the traceback are timed by their HIP events (cpecan_viterbi_kernel_ms),
the match batch by events on its launch stream as bench.py does; after warm-up, the median of --runs runs (at least five).

    python tools/viterbi_profile.py [--pairs N] [--runs 5] [--out profiles/viterbi.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpecan_amd import api, viterbi, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=0, help="override config B's number of pairs")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi.txt"))
    args = ap.parse_args()
    assert args.runs >= 5, "the median of at least five runs"
    cfg = dict(workload.CONFIGS["B"])
    n = args.pairs or cfg["n_pairs"]
    problems = workload.config_problems("B", range(n))
    sm = api.stateMachine5_construct(api.fiveState)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"], splitMatrixBiggerThanThis=cfg.get("split", 10 ** 15))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("Viterbi decoding at config B: %d pairs of %d bp, five-state, band %d; commit %s; %s" % (
        n, cfg["length"], cfg["expansion"], commit, torch.cuda.get_device_name(0)))
    say("warm-up %d, then the median of %d runs; [min .. max] beside it" % (args.warmup, args.runs))

    def med(v):
        return "%.3f ms [%.3f .. %.3f]" % (statistics.median(v), min(v), max(v))

    for form, name in ((viterbi.FORM_AUTO, "automatic (LDS rows)"), (viterbi.FORM_GLOBAL, "global rows, forced")):
        with viterbi.Viterbi(sm, p) as v:
            t0 = time.perf_counter()
            v.add_many(problems)
            add_s = time.perf_counter() - t0
            info = [v.info(i) for i in range(v.n)]
            cells = sum(i["nCells"] for i in info)
            v.set_form(form)
            sweep, trace, wall = [], [], []
            for k in range(args.warmup + args.runs):
                t0 = time.perf_counter()
                v.run()
                if k >= args.warmup:
                    wall.append(1e3 * (time.perf_counter() - t0))
                    s, t = v.kernel_ms()
                    sweep.append(s)
                    trace.append(t)
            forms = v.launch_forms()
            n_ops = sum(len(v.result(i).ops) for i in range(0, v.n, max(1, v.n // 100)))
            say("")
            say("form: %s" % name)
            say("  sweep      %s" % med(sweep))
            say("  traceback  %s" % med(trace))
            total = [a + b for a, b in zip(sweep, trace)]
            say("  both       %s  = %.3g band cells/s (%d band cells; sweep alone %.3g cells/s)" % (
                med(total), cells / (1e-3 * statistics.median(total)), cells, cells / (1e-3 * statistics.median(sweep))))
            say("  pointer bytes %d (one per band cell), device bytes of all regions %d, default budget %d: %d launches (%d regions in "
                "LDS form, %d in global form)" % (cells, sum(i["deviceBytes"] for i in info), viterbi.MAX_BYTES, forms.launches,
                                                  forms.lds, forms.global_))
            say("  a whole run on the host's clock (tables, copies, kernels, ops back): %s; adding the problems: %.2f s; every 100th "
                "problem holds %d ops" % (med(wall), add_s, n_ops))
        api.cache_trim()

    prepared, n_prepared, _keep = api.Batch.prepare_problems(problems)
    b = api.Batch(sm, p, emit=api.EMIT_MATCH, device=0)
    b.add_prepared(prepared, n_prepared)
    b.upload()
    stream = torch.cuda.Stream()
    ms = []
    for k in range(args.warmup + args.runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        b.run(stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    mcells = b.stats().cells
    say("")
    say("CPECAN_EMIT_MATCH batch over the same problems (forward, backward, posterior lists), kernel time of a run:")
    say("  %s  = %.3g band cells/s (%d band cells)" % (med(ms), mcells / (1e-3 * statistics.median(ms)), mcells))
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
