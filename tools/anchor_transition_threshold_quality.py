"""The anchor finder with seedTransitions = 1 and a threshold T of their own for HSPs that only variant hits seed
(cpecan_anchor_options.transitionHspThreshold), on the ENCODE pairs, on the CPU: the model's statistics
(tests/anchor_model_threshold.py), the anchor columns on and off the embedded alignment, and sensitivity / specificity of
the oracle's aligned pairs as tools/anchor_transitions_quality.py computes them.  Needs no GPU.
Usage: python tools/anchor_transition_threshold_quality.py > profiles/anchor_quality_transition_threshold.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import anchor_model as am  # noqa: E402
import anchor_model_threshold as ath  # noqa: E402
import reference_cases as rc  # noqa: E402
from anchor_transitions_quality import quality  # noqa: E402

THRESHOLDS = (800, 1000, 1200, 1600, 2400)


def main():
    for name in ("chimp", "dog", "mouse"):
        sx, sy, _, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
        for T in THRESHOLDS:
            runs, st = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=T)
            anchors = am.runs_to_anchors(runs)
            on = sum((x, y) in true_pairs for x, y, _ in anchors)
            t0 = time.time()
            sens, spec = quality(sx, sy, anchors, true_pairs)
            print("%s seedTransitions=1 T=%d stats=%s on_alignment=%d off_alignment=%d sens=%.4f spec=%.4f oracle %.0f s" %
                  (name, T, st, on, len(anchors) - on, sens, spec, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
