"""The anchor finder with and without seedTransitions on the ENCODE pairs, on the CPU: the model's statistics
(tests/anchor_model_transitions.py), the anchor columns that lie on the embedded alignment, and sensitivity / specificity
of the oracle's aligned pairs after the ordered filter at 0.5, beside the same figures for anchors cut from the embedded
alignment.  Needs no GPU.  Usage: python tools/anchor_transitions_quality.py > profiles/anchor_quality_transitions.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_model as am  # noqa: E402
import anchor_model_transitions as amt  # noqa: E402
import oracle_binding as ob  # noqa: E402
import reference_cases as rc  # noqa: E402


def quality(sx, sy, anchors, true_pairs):
    pairs = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params(diagonalExpansion=20))
    return rc.sensitivity_specificity(ob.filter_pairs_ordered(pairs, len(sx), len(sy), 0.5), true_pairs)


def main():
    for name in ("chimp", "dog", "mouse"):
        sx, sy, answer, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
        for t in (0, 1):
            runs, st = amt.find_anchor_runs(sx, sy, seedTransitions=t)
            anchors = am.runs_to_anchors(runs)
            on = sum((x, y) in true_pairs for x, y, _ in anchors)
            t0 = time.time()
            sens, spec = quality(sx, sy, anchors, true_pairs)
            print("%s seedTransitions=%d stats=%s on_alignment=%d (%.1f %%) from_sequences sens=%.4f spec=%.4f oracle %.0f s" %
                  (name, t, st, on, 100.0 * on / max(1, len(anchors)), sens, spec, time.time() - t0), flush=True)
        print("%s from_the_answer sens=%.4f spec=%.4f" % ((name,) + quality(sx, sy, answer, true_pairs)), flush=True)


if __name__ == "__main__":
    main()
