"""Writes tests/golden/dog_threshold_oracle_pairs.npz: the CPU oracle's aligned pairs of the ENCODE human / dog pair
(five-state model, default parameters, no ragged ends) fed the anchors that tests/anchor_model_threshold.py finds with
seedTransitions = 1 and transitionHspThreshold = 1200, and those anchors.  The oracle takes a third of a minute on this
pair, too long for a test, so tests/test_gpu_anchor_threshold.py reads its recorded answer;
tests/test_anchor_threshold_cpu.py checks that the recorded anchors are still the model's.  Needs no GPU.
Usage: python tests/golden/make_threshold_fixture.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import anchor_model as am  # noqa: E402
import anchor_model_threshold as ath  # noqa: E402
import oracle_binding as ob  # noqa: E402
import reference_cases as rc  # noqa: E402

THRESHOLD = 1200


def main():
    sx, sy, _, _ = rc.encode_human_other("dog")
    runs, _ = ath.find_anchor_runs(sx, sy, seedTransitions=1, threshold=THRESHOLD)
    anchors = np.array(am.runs_to_anchors(runs), dtype=np.int64).reshape(-1, 3)
    pairs = np.asarray(ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params()), dtype=np.int64).reshape(-1, 3)
    assert pairs.max() < 2 ** 31 and pairs.min() >= 0
    np.savez_compressed(os.path.join(HERE, "dog_threshold_oracle_pairs.npz"), runs=runs.astype(np.int32),
                        pairs=pairs.astype(np.int32))
    print("%d runs, %d pairs" % (len(runs), len(pairs)))


if __name__ == "__main__":
    main()
