"""The anchor finder with gapped extension of the chained HSPs (cpecan_anchor_options.gappedExtension; DESIGN.md section 7,
step 5b) on the ENCODE pairs, on the CPU: the model's statistics (tests/anchor_model_gapped.py) with the option off and
on, the anchor columns on and off the embedded alignment, the cells of the gap rectangles the DP crosses without a band,
and sensitivity / specificity of the oracle's aligned pairs as tools/anchor_transitions_quality.py computes them -- with
the default seeds and with seedTransitions = 1 and transitionHspThreshold = 1200.  Needs no GPU.
Usage: python tools/anchor_gapped_quality.py >> profiles/anchor_quality_gapped.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import anchor_model as am  # noqa: E402
import anchor_model_gapped as ag  # noqa: E402
import reference_cases as rc  # noqa: E402
from anchor_transitions_quality import quality  # noqa: E402


def main():
    for name in ("chimp", "dog", "mouse"):
        sx, sy, _, true_pairs = rc.encode_human_chimp() if name == "chimp" else rc.encode_human_other(name)
        for seedTransitions, T in ((0, 0), (1, 1200)):
            for gapped in (0, 1):
                runs, st = ag.find_anchor_runs(sx, sy, seedTransitions=seedTransitions, threshold=T, gapped=gapped)
                anchors = am.runs_to_anchors(runs)
                on = sum((x, y) in true_pairs for x, y, _ in anchors)
                cells = sum((x - pX) * (y - pY) for pX, pY, x, y in am._gaps([r[:3] for r in runs.tolist()], len(sx), len(sy)))
                t0 = time.time()
                sens, spec = quality(sx, sy, anchors, true_pairs)
                print("%s seedTransitions=%d T=%d gappedExtension=%d stats=%s on_alignment=%d off_alignment=%d gap_cells=%d "
                      "sens=%.4f spec=%.4f oracle %.0f s" % (name, seedTransitions, T, gapped, st, on, len(anchors) - on, cells,
                                                             sens, spec, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
