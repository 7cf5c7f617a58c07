"""Model slots (cpecan_batch_reserve_models / set_models / the _slot getters) without a GPU: argument checks, call order,
and that reserving changes nothing the host plans."""
import ctypes as C
import json
import os
import subprocess

import pytest

from cpecan_amd import api, em, realign
from cpecan_amd.workload import make_pair, make_realign_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests_unreserved.json")


def _batch(emit=api.EMIT_EXPECT, sm=None):
    return api.Batch(sm or api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=10),
                     emit=emit)


def test_slot_count_limits():
    assert api.MAX_MODEL_SLOTS == 8
    with _batch() as b:
        for n in (0, 9, -1):
            with pytest.raises(api.CpecanError, match="slots"):
                b.reserve_models(n)
        for n in (1, 3, 8):
            b.reserve_models(n)


@pytest.mark.parametrize("emit", [api.EMIT_MATCH, api.EMIT_INDEL])
def test_list_emitters_take_no_slots(emit):
    with _batch(emit) as b:
        with pytest.raises(api.CpecanError, match=r"\(-1\).*EMIT_EXPECT"):
            b.reserve_models(2)
    with _batch(api.EMIT_FORWARD) as b:
        b.reserve_models(2)


def test_call_order_and_state_count():
    five, three = api.stateMachine5_construct(), api.stateMachine3_construct()
    with _batch() as b:
        b.reserve_models(3)
        with pytest.raises(api.CpecanError, match=r"\(-5\).*before upload"):
            b.set_models([five, five])
        with pytest.raises(api.CpecanError, match=r"\(-1\).*3 states for a batch planned for 5"):
            b.set_models([five, three])
    with _batch() as b:
        b.add(*make_pair(1, 0, 200, 10))
        with pytest.raises(api.CpecanError, match=r"\(-2\)"):  # CPECAN_ENODEVICE: no compute without a GPU
            b.upload()
        b.reserve_models(2)  # the upload failed: the batch is not frozen


def test_reserve_on_an_unfrozen_batch_and_without_one():
    # (a batch freezes only where there is a device: reserve after upload, CPECAN_ESTATE, is asserted on the GPU --
    # tests/test_gpu_model_slots.py, test_a_reserved_batch_before_set_models_runs_its_own_model)
    lib = api.lib()
    with _batch() as b:
        assert lib.cpecan_batch_reserve_models(b._h, 2) == 0
        assert lib.cpecan_batch_reserve_models(None, 2) == -1


def test_slot_getters_check_state_and_arguments():
    lib = api.lib()
    h = api.hmm_constructEmpty(0.0, api.fiveState)
    v = C.c_double()
    with _batch() as b:
        assert lib.cpecan_batch_expectations_slot(b._h, 0, C.byref(h)) == -5  # nothing downloaded
        assert lib.cpecan_batch_expectations_slot(None, 0, C.byref(h)) == -5
    with _batch(api.EMIT_FORWARD) as b:
        assert lib.cpecan_batch_forward_prob_slot(b._h, 0, 0, C.byref(v)) == -5
        assert lib.cpecan_batch_forward_prob_slot(None, 0, 0, C.byref(v)) == -5


def _plan_digest(b):
    f = api.lib().cpk_batch_plan_digest
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    assert f(b._h, out) == 0, api.lib().cpecan_last_error()
    return [int(x) for x in out]


def _fixed_batches():
    yield "expect_1kb_x10", api.EMIT_EXPECT, [make_pair(5, i, 1000, 10) for i in range(24)], dict(diagonalExpansion=10)
    yield "expect_realign", api.EMIT_EXPECT, make_realign_batch(4, 40, 100, 1500, 4), dict(diagonalExpansion=4, splitMatrixBiggerThanThis=100)
    yield "forward_wide", api.EMIT_FORWARD, [make_pair(3, i, 700, 60) for i in range(8)], dict(diagonalExpansion=60)


def digests(reserve):
    out = {}
    for name, emit, problems, pkw in _fixed_batches():
        with api.Batch(api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct(**pkw), emit=emit) as b:
            if reserve:
                b.reserve_models(reserve)
            b.add_many(problems)
            out[name] = _plan_digest(b)
    return out


def test_plan_digest_of_an_unreserved_batch_is_the_parents():
    """tests/golden/plan_digests_unreserved.json: the four hashes of three fixed batches, taken with the library of the
    commit before model slots.  A reserved batch plans the same regions, order, segments and geometry."""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert digests(0) == want
    assert digests(1) == want
    assert digests(8) == want
    with _batch() as b:  # the symbols exist at all (this file fails as a whole on a library without them)
        b.reserve_models(2)


EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpecan_amd", "cpecan_em")


def _em(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_command_line_concurrent_trials_option(tmp_path):
    assert os.path.exists(EXE), "build the command line with make -C cpecan_amd/csrc"
    res = _em("--help")
    assert res.returncode == 0 and "--concurrentTrials" in res.stderr
    for bad in ("0", "9", "x"):
        res = _em("--sequences", "a.fa", "--alignments", "x", "--concurrentTrials", bad)
        assert res.returncode != 0 and "--concurrentTrials" in res.stderr and "1 to 8" in res.stderr
    # a good value is parsed and the run goes on to its files: the fasta that is not there is what fails
    missing = str(tmp_path / "missing.fa")
    res = _em("--sequences", missing, "--alignments", "x", "--concurrentTrials", "3")
    assert res.returncode != 0 and "concurrentTrials" not in res.stderr and missing in res.stderr


def test_trainer_and_expect_set_argument_checks():
    with em.Trainer() as t:
        for bad in (0, 9):
            with pytest.raises(api.CpecanError, match="concurrent trials"):
                t.set_concurrent_trials(bad)
        t.set_concurrent_trials(1)
        t.set_concurrent_trials(8)
    L = realign._lib()
    assert L.cpecan_expect_set_reserve_models(None, 2) == -1
    assert L.cpecan_expect_set_run_models(None, None, 1, None) == -1
    assert "cpecan_em_trainer_set_concurrent_trials" in em.EXPORTS
    assert {"cpecan_expect_set_reserve_models", "cpecan_expect_set_run_models"} <= set(realign.EXPORTS)


def test_set_models_checks_the_count_before_it_reads_the_models():
    one = (api.StateMachine * 1)(api.stateMachine5_construct())
    with _batch() as b:
        assert api.lib().cpecan_batch_set_models(b._h, one, 1000) == -1
        assert api.lib().cpecan_batch_set_models(b._h, one, 0) == -1
