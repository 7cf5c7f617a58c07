"""What an EM iteration with updateTheBand costs: writes profiles/em_update_band.txt.

Per size (pairs of ~1 kb, five-state model, diagonalExpansion 10, split at 3000 x 3000 as cPecanEm passes them, three
iterations, so two realignments), in alternating runs as the measuring guide asks:
  A  em.train(updateTheBand=1): E-step, realign batch (of which the hand-off stage on the device) and re-plan per iteration,
     from cpecan_em_timing;
  B  em.train(updateTheBand=0): the resident iteration of profiles/em_iteration_vs_full_call.txt;
  C  the same loop through Realigner.expectations + Realigner.realign: every list 3 downloaded, cigars built on the host and
     their operations walked again -- what the trainer would do without the stage, and what the commit before could do.
Medians over the repeats; every run is printed as it ends, so a run that is cut short still leaves its figures.

    python tools/em_update_band_bench.py [--pairs 1000,100000] [--repeats 3] [--out profiles/em_update_band.txt]
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpecan_amd import api, em  # noqa: E402
from cpecan_amd.realign import Cigar, Realigner  # noqa: E402

M, DX, IY = api.OP_MATCH, api.OP_INDEL_X, api.OP_INDEL_Y
ITERATIONS = 3


def world(n, length=1000, seed=5):
    """n pairs: X random, Y a copy with 8 % substitutions and an indel of 1-6 bases about every 120 columns; the cigar is
    the true alignment."""
    rng = random.Random(seed)
    seqs, cigars = {}, []
    for k in range(n):
        ops, sx, sy = [], [], []
        while len(sx) < length:
            run = rng.randrange(60, 180)
            ops.append((M, run))
            for _ in range(run):
                b = rng.choice("ACGT")
                sx.append(b)
                sy.append(b if rng.random() > 0.08 else rng.choice("ACGT"))
            t, g = rng.choice((DX, IY)), rng.randrange(1, 7)
            ops.append((t, g))
            (sx if t == DX else sy).extend(rng.choice("ACGT") for _ in range(g))
        seqs["x%d" % k], seqs["y%d" % k] = "".join(sx), "".join(sy)
        cigars.append(Cigar("x%d" % k, 0, len(sx), True, "y%d" % k, 0, len(sy), True, 0.0, ops))
    return seqs, cigars


def options():
    return em.em_realign_options(diagonalExpansion=10, splitMatrixBiggerThanThis=3000)


def trained(seqs, cigars, update, path):
    t0 = time.perf_counter()
    with em.Trainer(em.em_options(iterations=ITERATIONS, trainEmissions=1, setJukesCantorStartingEmissions=0.2,
                                  updateTheBand=int(update)), options()) as t:
        for name, s in seqs.items():
            t.add_sequence(name, s)
        t.train(cigars, path)
        tm = t.timing()
    wall = 1e3 * (time.perf_counter() - t0)
    e_step = (tm.iterationsMs - tm.realignMs - tm.replanMs) / ITERATIONS
    rounds = max(1, ITERATIONS - 1)
    return dict(wall=wall, setup=tm.setupMs, iterations=tm.iterationsMs, e_step=e_step, realign=tm.realignMs / rounds,
                handoff=tm.handoffMs / rounds, replan=tm.replanMs / rounds)


def written_out(seqs, cigars):
    """The loop of tests/test_gpu_em_update_band.py; the realigners are made once (adding the sequences is no part of an
    iteration)."""
    h = em.hmm_set_jukes_cantor(em.hmm_equalise(api.hmm_constructEmpty(0.0, api.fiveState)), 0.2)
    r = Realigner(api.hmm_getStateMachine(h), options())
    for name, s in seqs.items():
        r.add_sequence(name, s)
    cur, e_ms, r_ms = list(cigars), [], []
    t_all = time.perf_counter()
    for it in range(ITERATIONS):
        t0 = time.perf_counter()
        r.set_model(api.hmm_getStateMachine(h))
        acc = api.hmm_constructEmpty(1e-12, api.fiveState)
        r.expectations(cur, acc)
        api.hmm_normalise(acc)
        h = acc
        e_ms.append(1e3 * (time.perf_counter() - t0))
        if it + 1 < ITERATIONS:
            t0 = time.perf_counter()
            r.set_model(api.hmm_getStateMachine(h))
            cur = r.realign(cur)
            r_ms.append(1e3 * (time.perf_counter() - t0))
    r.close()
    return dict(iterations=1e3 * (time.perf_counter() - t_all), e_step=statistics.median(e_ms), realign=statistics.median(r_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1000,100000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "em_update_band.txt"))
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU")
    out = open(a.out, "w")

    def say(text):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say("tools/em_update_band_bench.py: pairs of ~1 kb, fiveState, diagonalExpansion 10, %d iterations (%d realignments), ms"
        % (ITERATIONS, ITERATIONS - 1))
    say("A = em.train(updateTheBand=1); B = em.train(updateTheBand=0), the resident iteration; C = the loop through")
    say("Realigner.expectations + Realigner.realign (list 3 downloaded, cigars built and walked on the host).  Alternating runs.")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hmm.txt")
        for n in [int(v) for v in a.pairs.split(",")]:
            seqs, cigars = world(n)
            say("")
            say("%d pairs" % n)
            runs = {"A": [], "B": [], "C": []}
            for k in range(a.repeats):
                runs["A"].append(trained(seqs, cigars, True, path))
                say("  run %d A: %s" % (k, "  ".join("%s %.1f" % kv for kv in runs["A"][-1].items())))
                runs["B"].append(trained(seqs, cigars, False, path))
                say("  run %d B: %s" % (k, "  ".join("%s %.1f" % kv for kv in runs["B"][-1].items())))
                runs["C"].append(written_out(seqs, cigars))
                say("  run %d C: %s" % (k, "  ".join("%s %.1f" % kv for kv in runs["C"][-1].items())))
            med = {w: {f: statistics.median(r[f] for r in rs) for f in rs[0]} for w, rs in runs.items()}
            say("  medians per iteration: A E-step %.1f, realign batch %.1f (hand-off stage %.2f), re-plan %.1f" %
                (med["A"]["e_step"], med["A"]["realign"], med["A"]["handoff"], med["A"]["replan"]))
            say("                         B E-step %.1f (resident, nothing re-planned)" % med["B"]["e_step"])
            say("                         C E-step call %.1f, realign call %.1f" % (med["C"]["e_step"], med["C"]["realign"]))
    out.close()


if __name__ == "__main__":
    main()
