"""What a Viterbi-training E-step costs: cpecan_viterbi_run_counts over a resident Viterbi object on
BASELINE config 5's sample (100 000 pairs of 1 kb, five-state, band 10: the trainer's workload) and on config B's problems
(10 000 pairs of 2 kb, band 100: the workload profiles/viterbi.txt measured), built with cpecan_amd/workload.py as bench.py
builds them.  One process, one GPU.  Per iteration the sweep, traceback, count and reduce kernels by their HIP events
(cpecan_viterbi_kernel_ms, cpecan_viterbi_count_ms) and the whole call on the host's clock; the first call, which plans and
uploads, apart; beside them a plain cpecan_viterbi_run over the same object and, for config 5, the kernel and wall time of a
CPECAN_EMIT_EXPECT batch over the same sample, as the Baum-Welch trainer runs it.  After warm-up, the median of --runs runs
(at least five), [min .. max] beside it.

    python tools/viterbi_training_profile.py [--pairs5 N] [--pairsB N] [--runs 5] [--out profiles/viterbi_training.txt]
    CPECAN_LIB=<library of the commit before> python tools/viterbi_training_profile.py --plain-only --append

--plain-only measures cpecan_viterbi_run alone, with whatever library CPECAN_LIB names: that is how the parent commit's
figures get into the same file (--append).
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


def med(v):
    return "%.3f ms [%.3f .. %.3f]" % (statistics.median(v), min(v), max(v))


def params_of(cfg):
    return api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"],
                                                            splitMatrixBiggerThanThis=cfg.get("split", 10 ** 15))


def plain_runs(v, warmup, runs):
    sweep, trace, wall = [], [], []
    for k in range(warmup + runs):
        t0 = time.perf_counter()
        v.run()
        if k >= warmup:
            wall.append(1e3 * (time.perf_counter() - t0))
            s, t = v.kernel_ms()
            sweep.append(s)
            trace.append(t)
    return sweep, trace, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs5", type=int, default=0, help="override config 5's number of pairs")
    ap.add_argument("--pairsB", type=int, default=0, help="override config B's number of pairs")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--plain-only", action="store_true", help="cpecan_viterbi_run alone (any library of the plain ABI)")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_training.txt"))
    args = ap.parse_args()
    assert args.runs >= 5, "the median of at least five runs"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert args.plain_only or hasattr(viterbi._lib(), "cpecan_viterbi_run_counts"), "a library from before the counts: --plain-only"
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("%s; library %s; working tree of commit %s; %s" % ("cpecan_viterbi_run alone" if args.plain_only else "Viterbi training's E-step",
                                                           os.path.relpath(api.LIB_PATH, ROOT), commit, torch.cuda.get_device_name(0)))
    say("warm-up %d, then the median of %d runs; [min .. max] beside it" % (args.warmup, args.runs))
    sm = api.stateMachine5_construct(api.fiveState)
    for name, pairs in (("5", args.pairs5), ("B", args.pairsB)):
        cfg = dict(workload.CONFIGS[name])
        n = pairs or cfg["n_pairs"]
        problems = workload.config_problems(name, range(n))
        p = params_of(cfg)
        say("")
        say("config %s: %d pairs of %d bp, five-state, band %d" % (name, n, cfg["length"], cfg["expansion"]))
        with viterbi.Viterbi(sm, p) as v:
            v.add_many(problems)
            cells = sum(v.info(i)["nCells"] for i in range(v.n))
            if not args.plain_only:
                inputs, scratch = v.resident_bytes()
                t0 = time.perf_counter()
                first = v.run_counts()
                first_ms = 1e3 * (time.perf_counter() - t0)
                rows = {k: [] for k in ("sweep", "traceback", "count", "reduce", "wall")}
                for k in range(args.warmup + args.runs):
                    v.set_model(sm)  # as an iteration of the trainer does
                    t0 = time.perf_counter()
                    c = v.run_counts()
                    wall = 1e3 * (time.perf_counter() - t0)
                    assert c.nSteps == first.nSteps and c.logP == first.logP
                    if k >= args.warmup:
                        (s, t), (cn, rd) = v.kernel_ms(), v.count_ms()
                        for key, val in zip(rows, (s, t, cn, rd, wall)):
                            rows[key].append(val)
                f = v.launch_forms()
                say("  %d band cells, %d steps on the paths, %d regions without a path; %d launches (%d regions in LDS form, %d in global "
                    "form)" % (cells, first.nSteps, first.nNoPath, f.launches, f.lds, f.global_))
                say("  resident inputs %d bytes beside %d bytes of scratch; the first run_counts (plan, pack, upload, run): %.1f ms" % (
                    inputs, scratch, first_ms))
                say("  run_counts from its second call on, per call:")
                for key in ("sweep", "traceback", "count", "reduce"):
                    say("    %-10s %s" % (key, med(rows[key])))
                kernels = [sum(x) for x in zip(rows["sweep"], rows["traceback"], rows["count"], rows["reduce"])]
                say("    kernels    %s  = %.3g band cells/s" % (med(kernels), cells / (1e-3 * statistics.median(kernels))))
                say("    wall       %s" % med(rows["wall"]))
                say("    outside the kernels (wall - kernels) %s" % med([w - k for w, k in zip(rows["wall"], kernels)]))
            sweep, trace, wall = plain_runs(v, args.warmup, args.runs)
            both = [a + b for a, b in zip(sweep, trace)]
            say("  cpecan_viterbi_run over the same problems, per call:")
            say("    sweep      %s" % med(sweep))
            say("    traceback  %s" % med(trace))
            say("    wall       %s" % med(wall))
            say("    outside the kernels (wall - sweep - traceback) %s" % med([w - k for w, k in zip(wall, both)]))
        api.cache_trim()
        if name == "5" and not args.plain_only:
            prepared, n_prepared, _keep = api.Batch.prepare_problems(problems)
            b = api.Batch(sm, p, emit=api.EMIT_EXPECT, device=0)
            b.add_prepared(prepared, n_prepared)
            b.upload()
            stream = torch.cuda.Stream()
            ms, wall = [], []
            for k in range(args.warmup + args.runs):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.set_model(sm)
                t0 = time.perf_counter()
                e0.record(stream)
                b.run(stream.cuda_stream)
                e1.record(stream)
                b.download()
                acc = api.hmm_constructEmpty(0.0, api.fiveState)
                b.expectations(acc)
                w = 1e3 * (time.perf_counter() - t0)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
                    wall.append(w)
            say("  CPECAN_EMIT_EXPECT batch over the same sample (the Baum-Welch E-step), per run:")
            say("    kernels    %s  = %.3g band cells/s (%d band cells)" % (med(ms), b.stats().cells / (1e-3 * statistics.median(ms)), b.stats().cells))
            say("    wall       %s  (set_model, run, download, expectations)" % med(wall))
            b.close()
            api.cache_trim()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
