"""A constructed input of the transitionHspThreshold tests, shared by the CPU (model only) and GPU (model against the
kernels) suites: three HSPs of different classes on the main diagonal of one pair.

X is random; Y is X with every base replaced by a transversion (score <= -114: nine such columns end an x-drop walk, and a
window that reaches into them has a compared transversion, so it is no hit), except in three stretches:
  A  36 columns, unchanged: exact hits, scores about 3400;
  B  150 columns, a transition at every 6th base as in anchor_transition_cases.case("a"): variant hits only, about 11 000;
  C  31 columns, the same pattern: variant hits only, about 2300.
With THRESHOLD between the scores of A and B, A is kept for its exact hits, B for its score, and C is dropped.
"""
import random

import anchor_transition_cases as tc

LENGTH = 800
THRESHOLD = 4000
STRETCHES = {"A": (100, 136), "B": (200, 350), "C": (420, 451)}   # [start, end) on both sequences


def mixed_classes():
    rng = random.Random(11)   # a generator seed at which nothing off the main diagonal reaches hspThreshold
                              # (tests/test_anchor_threshold_cpu.py checks that with the model)
    x = bytes(rng.choice(b"ACGT") for _ in range(LENGTH))
    y = bytearray(x.translate(tc._TRANSVERSION))
    a, e = STRETCHES["A"]
    y[a:e] = x[a:e]
    for a, e in (STRETCHES["B"], STRETCHES["C"]):
        y[a:e] = tc._changed(x[a:e], 6, tc._TRANSITION)
    return x, bytes(y)
