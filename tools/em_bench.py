"""Cost of one EM iteration on a resident batch against one full expectation call on the same data.

One full call is what `cpecan_realign --outputExpectations` pays per iteration when a script drives the EM loop: add the
problems, plan, upload, run, download, destroy.  An iteration of cpecan_em is cpecan_batch_set_model + run + download on a
batch that stays uploaded.  The problems are BASELINE config 5's (workload.CONFIGS["5"]: expectation emitter, 1000 bp,
expansion 10) or a smaller set; the model of each iteration is a different random five-state model, as in random-restart
trials.  Prints one JSON line.

    python tools/em_bench.py [--pairs 100000] [--iterations 10] [--trials 3] [--full-calls 2]

--models T measures model slots instead (cpecan_batch_reserve_models): T models in one launch of a reserved batch against
the same T models one after another (set_model + run + download each) on a plain resident batch, rounds alternating.

    python tools/em_bench.py --models 3 [--pairs 1000] [--iterations 15]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpecan_amd import api, em  # noqa: E402
from cpecan_amd.workload import CONFIGS, config_problems  # noqa: E402


def slots_bench(a, p, arr, n, models):
    T = a.models
    pool = models  # at least T + 1 different models (main)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    with api.Batch(models[0], p, emit=api.EMIT_EXPECT, device=a.device) as plain, \
            api.Batch(models[0], p, emit=api.EMIT_EXPECT, device=a.device) as slotted:
        plain.add_prepared(arr, n)
        plain.upload()
        slotted.reserve_models(T)
        slotted.add_prepared(arr, n)
        slotted.upload()
        seq_s, seq_ms, slot_s, slot_ms = [], [], [], []
        for it in range(a.iterations + 2):  # two warm rounds
            ms_ = [pool[(it * T + k) % len(pool)] for k in range(T)]
            t = time.perf_counter()
            kms = 0.0
            for m in ms_:
                plain.set_model(m)
                plain.run()
                plain.download()
                plain.expectations(api.hmm_constructEmpty(0.0, api.fiveState))
                kms += plain.stats().kernelMs
            ts = time.perf_counter() - t
            waves_seq = plain.stats().wavesPerLaunch
            t = time.perf_counter()
            slotted.set_models(ms_)
            slotted.run()
            slotted.download()
            for k in range(T):
                slotted.expectations(api.hmm_constructEmpty(0.0, api.fiveState), k)
            tl = time.perf_counter() - t
            if it >= 2:
                seq_s.append(ts)
                seq_ms.append(kms)
                slot_s.append(tl)
                slot_ms.append(slotted.stats().kernelMs)
        st, ss = plain.stats(), slotted.stats()
    print(json.dumps({
        "what": "T models in one launch (model slots) vs T models one after another, same resident problems",
        "models": T, "pairs": a.pairs, "regions": st.regions, "cells": st.cells, "rounds": a.iterations,
        "sequential_s_median": med(seq_s), "sequential_s_min": min(seq_s), "sequential_s_max": max(seq_s),
        "sequential_kernel_ms_median": med(seq_ms), "sequential_kernel_ms_min": min(seq_ms), "sequential_kernel_ms_max": max(seq_ms),
        "sequential_waves_per_launch": waves_seq,
        "slotted_s_median": med(slot_s), "slotted_s_min": min(slot_s), "slotted_s_max": max(slot_s),
        "slotted_kernel_ms_median": med(slot_ms), "slotted_kernel_ms_min": min(slot_ms), "slotted_kernel_ms_max": max(slot_ms),
        "slotted_waves_per_launch": ss.wavesPerLaunch,
        "sequential_over_slotted": med(seq_s) / med(slot_s),
        "sequential_over_slotted_kernel": med(seq_ms) / med(slot_ms),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=CONFIGS["5"]["n_pairs"])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--full-calls", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--models", type=int, default=0, help="T: model slots, T in one launch against T in a row")
    a = ap.parse_args()
    cfg = CONFIGS["5"]
    t0 = time.perf_counter()
    problems = config_problems("5", range(a.pairs))
    arr, n, keep = api.Batch.prepare_problems(problems)
    gen_s = time.perf_counter() - t0
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"])
    models = [api.hmm_getStateMachine(em.hmm_set_jukes_cantor(em.hmm_randomise(
        api.hmm_constructEmpty(0.0, api.fiveState), 100 + k), 0.1)) for k in range(max(a.iterations * a.trials, a.models) + 1)]

    if a.models:
        return slots_bench(a, p, arr, n, models)

    def full_call(sm):
        t = time.perf_counter()
        with api.Batch(sm, p, emit=api.EMIT_EXPECT, device=a.device) as b:
            b.add_prepared(arr, n)
            b.upload()
            b.run()
            b.download()
            acc = api.hmm_constructEmpty(0.0, api.fiveState)
            b.expectations(acc)
            st = b.stats()
        return time.perf_counter() - t, acc.likelihood, st

    full_call(models[0])  # warm: block caches, kernels loaded
    full = [full_call(models[k % len(models)]) for k in range(a.full_calls)]
    full_s = sorted(f[0] for f in full)[len(full) // 2]
    kernel_ms_full = full[-1][2].kernelMs

    with api.Batch(models[0], p, emit=api.EMIT_EXPECT, device=a.device) as b:
        t = time.perf_counter()
        b.add_prepared(arr, n)
        b.upload()
        setup_s = time.perf_counter() - t
        b.run()
        b.download()
        iters, kernel_ms = [], []
        for k in range(a.iterations * a.trials):
            t = time.perf_counter()
            b.set_model(models[k + 1])
            b.run()
            b.download()
            acc = api.hmm_constructEmpty(0.0, api.fiveState)
            b.expectations(acc)
            iters.append(time.perf_counter() - t)
            kernel_ms.append(b.stats().kernelMs)
        st = b.stats()
    iters.sort()
    kernel_ms.sort()
    out = {
        "what": "EM iteration on a resident batch vs one full expectation call",
        "pairs": a.pairs, "regions": st.regions, "cells": st.cells, "launchForm": st.launchForm,
        "wavesPerLaunch": st.wavesPerLaunch,
        "iterations": a.iterations * a.trials,
        "iteration_s_median": iters[len(iters) // 2], "iteration_s_min": iters[0], "iteration_s_max": iters[-1],
        "iteration_kernel_ms_median": kernel_ms[len(kernel_ms) // 2],
        "full_call_s_median": full_s, "full_call_kernel_ms": kernel_ms_full,
        "resident_setup_s": setup_s, "problem_generation_s": gen_s,
        "full_call_over_iteration": full_s / iters[len(iters) // 2],
        "iteration_over_kernel": iters[len(iters) // 2] / (kernel_ms[len(kernel_ms) // 2] / 1e3),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
