"""The next-runs stage on the GPU (cpecan_post_next_runs behind CPECAN_POST_ORDERED; include/cpecan_realign.h): for the
cases of tests/next_runs_cases.py the runs a batch downloads equal cpecan_next_runs_of_pairs on the downloaded list 3 of a
twin batch without the stage, integer for integer, and the exact-match anchor runs of the cigars Realigner.realign returns;
Realigner.reanchor returns the same, on one device and cut into shards.  A batch that switches the stage on and off again is
the plain batch."""
import numpy as np
import pytest

import next_runs_cases as nc
from cpecan_amd import api, realign
from cpecan_amd.realign import Cigar, Realigner, realign_options

pytestmark = pytest.mark.gpu


def _batch(c, stage, toggle=False):
    E, trim = c.opts["diagonalExpansion"], c.opts["constraintDiagonalTrim"]
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=E, splitMatrixBiggerThanThis=nc.REALIGN_SPLIT)
    b = api.Batch(api.stateMachine5_construct(), p, emit=api.EMIT_MATCH)
    b.set_post(api.POST_REWEIGHT | api.POST_ORDERED, nc.GAP_GAMMA, 0.85)
    if stage or toggle:
        realign.batch_set_next_runs(b, trim, E)
    if toggle:
        realign.batch_set_next_runs(b, 0, realign.NEXT_RUNS_OFF)
    b.add_many_runs([(sx, sy, anchors, True, True) for sx, sy, anchors in nc.problems(c)])
    b.upload()
    b.run()
    b.download()
    return b


def _realigner(c):
    r = Realigner(options=realign_options(**c.opts))
    for name, s in c.seqs.items():
        r.add_sequence(name, s)
    return r


def _rows(a):
    return [tuple(int(v) for v in row) for row in a]


@pytest.mark.parametrize("name", [c.name for c in nc.all_cases()])
def test_stage_equals_the_host_function_and_the_realigned_cigars(name):
    c = nc.case(name)
    E, trim = c.opts["diagonalExpansion"], c.opts["constraintDiagonalTrim"]
    probs = nc.problems(c)
    cigars = [Cigar(*a) for a in c.cigars]
    with _batch(c, False) as twin, _batch(c, True) as staged, _realigner(c) as r:
        with pytest.raises(api.CpecanError):
            staged.result(0, 3)  # the triples of such a batch stay on the device
        with pytest.raises(api.CpecanError):
            realign.batch_set_next_runs(staged, trim, E)  # after upload
        with pytest.raises(api.CpecanError):
            realign.batch_next_runs(twin, 0)  # not asked for
        realigned = r.realign(cigars)
        reanchored = r.reanchor(cigars)
        assert len(realigned) == len(reanchored) == len(probs)
        unsorted = 0
        for i, (sx, sy, _) in enumerate(probs):
            got = _rows(realign.batch_next_runs(staged, i))
            list3 = twin.result(i, 3)
            assert _rows(realign.next_runs_of_pairs(list3, sx, sy, trim, E)) == got, (name, i)
            assert _rows(api.anchor_runs_from_alignment(realigned[i].ops, 0, 0, trim, E, sx, sy)) == got, (name, i)
            assert _rows(reanchored[i]) == got, (name, i)
            np.testing.assert_array_equal(staged.scores(i)[:2], twin.scores(i)[:2])  # (nan for an empty list, in both)
            np.testing.assert_array_equal(staged.identity_scores(i), twin.identity_scores(i))
            unsorted += bool(len(list3) > 1 and np.any(np.diff(list3[:, 1]) < 0))
            if name == "empty" or (name == "many-300" and i == 137):
                assert len(list3) == 0 and got == []
            else:
                assert len(got) > 0
        assert unsorted > 0 or name == "empty"  # list 3 arrives in reverse input order: the stage cannot take it as sorted
    if name == "many-300":
        with _realigner(c) as r:
            r.set_devices([0, 0, 0])  # three logical shards on device 0, joined in input order
            sharded = r.reanchor(cigars)
        assert [_rows(a) for a in sharded] == [_rows(a) for a in reanchored]


def test_reanchoring_on_given_runs_is_realigning_the_realigned_cigars():
    c = nc.case("long-1200")
    cigars = [Cigar(*a) for a in c.cigars]
    with _realigner(c) as r:
        first = r.reanchor(cigars)
        second = r.reanchor(cigars, runs_in=first)
        once = r.realign(cigars)
        twice = r.realign(once)
    sx, sy, _ = nc.problems(c)[0]
    E, trim = c.opts["diagonalExpansion"], c.opts["constraintDiagonalTrim"]
    assert _rows(api.anchor_runs_from_alignment(twice[0].ops, 0, 0, trim, E, sx, sy)) == _rows(second[0])


def test_stage_switched_on_and_off_again_is_the_plain_batch():
    c = nc.case("straddle")
    with _batch(c, False) as plain, _batch(c, False, toggle=True) as toggled:
        a, b = plain.stats(), toggled.stats()
        for f in ("problems", "regions", "cells", "diagonals", "pairs", "deviceBytes", "launches", "wavesPerLaunch", "launchForm"):
            assert getattr(a, f) == getattr(b, f), f
        for i in range(len(c.cigars)):
            for which in (0, 3):
                np.testing.assert_array_equal(plain.result(i, which), toggled.result(i, which))
            np.testing.assert_array_equal(plain.scores(i), toggled.scores(i))
        with pytest.raises(api.CpecanError):
            realign.batch_next_runs(toggled, 0)
