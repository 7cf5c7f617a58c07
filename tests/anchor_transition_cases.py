"""Constructed inputs of the seedTransitions tests, shared by the CPU (model only) and GPU (model against the kernels) suites.

One random X of 700 bases and three Y made from it by point changes at every `period`-th position.  The seed
1110100110010101111 compares window offsets 0 1 2 4 7 8 11 13 15 16 17 18.  A window that starts c positions before a changed
base carries the changes at offsets c, c + period, ...:
  period 6: compared changes per window = 2 3 2 1 2 2 for c = 0 .. 5: never none, and one in the windows with c = 3;
  period 4: 4 3 2 3 for c = 0 .. 3: two or more in every window.
"""
import random

SEED = "1110100110010101111"
LENGTH = 700
COMPARED = [k for k, ch in enumerate(SEED) if ch == "1"]
_TRANSITION = bytes.maketrans(b"ACGT", b"GTAC")      # code ^ 2
_TRANSVERSION = bytes.maketrans(b"ACGT", b"CATG")    # code ^ 1


def _x():
    rng = random.Random(4)   # a generator seed at which no two windows off the main diagonal match by chance
                             # (tests/test_anchor_transitions_cpu.py checks that with the model)
    return bytes(rng.choice(b"ACGT") for _ in range(LENGTH))


def _changed(x, period, table):
    y = bytearray(x)
    for i in range(3, len(y), period):
        y[i:i + 1] = bytes(y[i:i + 1]).translate(table)
    return bytes(y)


def changes_per_window(x, y):
    """Bases that differ at the compared offsets, for every window of the main diagonal."""
    return [sum(x[i + k] != y[i + k] for k in COMPARED) for i in range(len(x) - len(SEED) + 1)]


def case(which):
    """(a) one transition every 6 bases; (b) transversions at the same positions; (c) one transition every 4 bases."""
    x = _x()
    return x, {"a": _changed(x, 6, _TRANSITION), "b": _changed(x, 6, _TRANSVERSION), "c": _changed(x, 4, _TRANSITION)}[which]
