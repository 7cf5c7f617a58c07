"""The band-edge statistic (cpecan_band_edge) as a sign of a band that was too narrow, on the CPU: the
oracle's aligned pairs, the statistic of cpecan_band_edge_of_pairs on them, and what doubling the expansion does.
 1. The three ENCODE pairs with the anchor finder's default anchors and with seedTransitions = 1 (the human / dog case of
    DESIGN.md section 7): per round k (expansion 20 * 2^k) the statistic, whether the pair is flagged under a few values of
    minEdgeScore, and sensitivity / specificity after the ordered filter at 0.5.
 2. Synthetic realign sets at expansion 4, cPecanRealign's parameters: cigars with a misplaced indel (the input cigar is
    gapless, the true alignment has one deletion) and correct cigars of the same pairs; the share of each flagged per round
    and minEdgeScore, and the share of misplaced cigars a round leaves unflagged although they still emit far more pairs
    than the correct cigar (misses of the flag).
Needs no GPU.  Usage: python tools/band_edge_quality.py >> profiles/band_edge_quality.txt"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_model as am  # noqa: E402
import anchor_model_transitions as amt  # noqa: E402
import oracle_binding as ob  # noqa: E402
import reference_cases as rc  # noqa: E402
from cpecan_amd import api  # noqa: E402

SCORES = (10 ** 6, 10 ** 7, 10 ** 8)
ROUNDS = 3


def statistic(sx, sy, anchors, pkw, pairs, ragged):
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    return api.band_edge_of_pairs(anchors, len(sx), len(sy), p, pairs, ragged, ragged)


def encode():
    om = ob.model(ob.FIVE_STATE)
    for name in ("chimp", "dog", "mouse"):
        sx, sy, _, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
        for t in (0, 1):
            runs, _ = amt.find_anchor_runs(sx, sy, seedTransitions=t)
            for k in range(ROUNDS):
                E = 20 << k
                anchors = [(x, y, E) for x, y, _ in am.runs_to_anchors(runs)]
                t0 = time.time()
                pkw = dict(diagonalExpansion=E)
                pairs = ob.aligned_pairs(om, sx, sy, anchors, ob.params(**pkw))
                e = statistic(sx, sy, anchors, pkw, pairs, False)
                sens, spec = rc.sensitivity_specificity(ob.filter_pairs_ordered(pairs, len(sx), len(sy), 0.5), true_pairs)
                print("%s seedTransitions=%d round=%d expansion=%d pairs=%d edgePairs=%d edgeScoreSum=%d edgeScoreMax=%d flagged=%s "
                      "sens=%.4f spec=%.4f oracle %.0f s" % (name, t, k, E, len(pairs), e["edgePairs"], e["edgeScoreSum"], e["edgeScoreMax"],
                                                             "/".join("%d:%s" % (s, "yes" if e["edgeScoreSum"] >= s else "no") for s in SCORES),
                                                             sens, spec, time.time() - t0), flush=True)


def synthetic(n=200, seed=1):
    rng = random.Random(seed)
    om = ob.model(ob.FIVE_STATE)
    rows = []
    for _ in range(n):
        lX, cut = rng.randrange(150, 300), rng.randrange(5, 16)
        x = "".join(rng.choice("ACGT") for _ in range(lX))
        at = rng.randrange(40, lX - 40 - cut)
        y = "".join(c if rng.random() > 0.05 else rng.choice("ACGT") for c in x[:at] + x[at + cut:])
        per_round = []
        for k in range(ROUNDS):
            E = 4 << k
            pkw = dict(diagonalExpansion=E, splitMatrixBiggerThanThis=10)
            wrong = [(i, i, E) for i in range(len(y)) if x[i] == y[i]]
            right = [(i if i < at else i + cut, i, E) for i in range(len(y)) if x[i if i < at else i + cut] == y[i]]
            out = []
            for anchors in (wrong, right):
                pairs = ob.aligned_pairs(om, x, y, anchors, ob.params(**pkw), True, True)
                out.append((statistic(x, y, anchors, pkw, pairs, True)["edgeScoreSum"], len(pairs)))
            per_round.append(out)
        rows.append(per_round)
    for s in SCORES:
        alive = list(range(n))  # misplaced cigars still flagged, as the adaptive band would run them
        for k in range(ROUNDS):
            flagged = [i for i in alive if rows[i][k][0][0] >= s]
            missed = [i for i in alive if i not in flagged and rows[i][k][0][1] > 1.3 * rows[i][k][1][1]]
            correct = sum(rows[i][k][1][0] >= s for i in range(n))
            print("synthetic n=%d minEdgeScore=%d round=%d expansion=%d: misplaced in the round %d, flagged %d (%.1f %% of all), "
                  "unflagged with over 1.3 x the correct cigar's pairs %d; correct cigars flagged %d (%.1f %%)" %
                  (n, s, k, 4 << k, len(alive), len(flagged), 100.0 * len(flagged) / n, len(missed), correct, 100.0 * correct / n), flush=True)
            alive = flagged


if __name__ == "__main__":
    print("# tools/band_edge_quality.py", flush=True)
    synthetic()
    encode()
