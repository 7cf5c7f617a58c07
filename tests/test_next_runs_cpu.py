"""CPU checks of the hand-off from an ordered alignment to the anchor runs of the next E-step (the trainer's updateTheBand;
include/cpecan_realign.h, include/cpecan_em.h): cpecan_next_runs_of_pairs against tests/next_runs_model.py and against
the composition of cpecan_cigar_from_aligned_pairs and cpecan_anchor_runs_from_alignment on lists worked out by hand and on
500 random chains; the argument checks; headers against their EXPORTS; the command line; and, with the CPU oracle, the
preconditions of the GPU cases (tests/test_gpu_next_runs.py, tests/test_gpu_em_update_band.py).  No GPU needed for any."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import next_runs_cases as nc
import next_runs_model as nm
from cpecan_amd import api, em, realign
from cpecan_amd.realign import Cigar, Realigner, realign_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_em")
E = 6


def _host(pairs, sx, sy, trim, expansion=E):
    return [tuple(r) for r in realign.next_runs_of_pairs([(7, x, y) for x, y in pairs], sx, sy, trim, expansion).tolist()]


def _composition(pairs, sx, sy, trim, expansion=E):
    """The cigar convertAlignedPairsToPairwiseAlignment makes of the sorted pairs, then the anchors cPecanRealign makes of
    that cigar's operations."""
    c = Cigar.from_aligned_pairs("x", "y", 0.0, len(sx), len(sy), sorted(pairs))
    assert (c.start1, c.end1, c.start2, c.end2) == (0, len(sx), 0, len(sy))
    return [tuple(r) for r in api.anchor_runs_from_alignment(c.ops, 0, 0, trim, expansion, sx, sy).tolist()]


@pytest.mark.parametrize("name", [h[0] for h in nc.HAND])
def test_hand_worked_lists(name):
    _, pairs, sx, sy, trim, want = next(h for h in nc.HAND if h[0] == name)
    want = [w + (E,) for w in want]
    assert nm.next_runs(pairs, sx, sy, trim, E) == want
    assert _composition(pairs, sx, sy, trim) == want
    assert _host(pairs, sx, sy, trim) == want
    assert _host(tuple(reversed(pairs)), sx, sy, trim) == want  # the device's list 3 arrives in reverse input order
    assert _host(pairs[1::2] + pairs[0::2], sx, sy, trim) == want


def test_random_chains():
    chains = nc.random_chains()
    assert len(chains) == 500
    kinds = set()
    for pairs, sx, sy, trim in chains:
        want = nm.next_runs(pairs, sx, sy, trim, E)
        assert _host(tuple(reversed(pairs)), sx, sy, trim) == want
        assert _composition(pairs, sx, sy, trim) == want
        kinds.add((len(pairs) == 0, len(want) == 0, trim == 0, len(nm.blocks(pairs)) > 2))
    assert len(kinds) >= 8  # empty and full lists, with and without trim, few and many blocks


def test_host_function_cap_and_argument_checks():
    L = realign._lib()
    pairs, sx, sy = next(h for h in nc.HAND if h[0] == "both-gaps")[1:4]
    t = np.array([(1, x, y) for x, y in pairs], dtype=np.int32)
    tp = t.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.full((1, 4), -1, dtype=np.int64)
    op = out.ctypes.data_as(C.POINTER(C.c_int64))
    args = (sx.encode(), len(sx), sy.encode(), len(sy))
    assert L.cpecan_next_runs_of_pairs(tp, len(t), *args, 0, E, op, 1) == 2  # the count may exceed cap; nothing beyond it is written
    assert out.tolist() == [[0, 0, 3, E]]
    assert L.cpecan_next_runs_of_pairs(tp, len(t), *args, 0, E, None, 0) == 2
    assert L.cpecan_next_runs_of_pairs(tp, len(t), *args, -1, E, None, 0) == -1  # CPECAN_EINVAL
    assert L.cpecan_next_runs_of_pairs(tp, len(t), *args, 0, -1, None, 0) == -1
    assert L.cpecan_next_runs_of_pairs(None, 3, *args, 0, E, None, 0) == -1
    assert L.cpecan_next_runs_of_pairs(tp, len(t), *args, 0, E, None, 5) == -1  # room promised, none given
    with pytest.raises(api.CpecanError):
        realign.next_runs_of_pairs([(1, 0, 0), (1, 1, 0)], "AC", "AC")  # no chain: y does not increase
    with pytest.raises(api.CpecanError):
        realign.next_runs_of_pairs([(1, 0, 2)], "AC", "AC")  # outside Y
    huge = realign.next_runs_of_pairs([(1, i, i) for i in range(10)], "ACGTACGTAC", "ACGTACGTAC", trim=2 ** 40)
    assert len(huge) == 0


def test_batch_stage_argument_checks():
    with api.Batch(api.stateMachine5_construct()) as b:
        with pytest.raises(api.CpecanError, match="ORDERED"):
            realign.batch_set_next_runs(b, 0, 4)  # the stage reads the ordered alignment
        b.set_post(api.POST_REWEIGHT | api.POST_ORDERED, 0.5, 0.85)
        with pytest.raises(api.CpecanError):
            realign.batch_set_next_runs(b, -1, 4)
        with pytest.raises(api.CpecanError):
            realign.batch_set_next_runs(b, 0, -7)
        realign.batch_set_next_runs(b, 2, 4)
        realign.batch_set_next_runs(b, 0, realign.NEXT_RUNS_OFF)
        with pytest.raises(api.CpecanError):
            realign.batch_next_runs(b, 0)  # nothing downloaded
    L = realign._lib()
    assert L.cpecan_batch_set_next_runs(None, 0, 4) == -1
    assert L.cpecan_batch_next_runs(None, 0, None, None) == -5  # CPECAN_ESTATE, as every getter without a download


def _realigner(**kw):
    r = Realigner(options=realign_options(**kw))
    r.add_sequence("X", "ACGTACGTACGTACGTACGT")
    r.add_sequence("Y", "ACGTACGTACTTACGTACGT")
    return r


def test_realigner_argument_checks():
    c = Cigar("X", 0, 20, True, "Y", 0, 20, True, 1.0, [(0, 20)])
    for kw in (dict(rescoreOriginalAlignment=1), dict(splitIndelsLongerThanThis=5)):
        with _realigner(**kw) as r:
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):  # CPECAN_EINVAL before a device is looked for
                r.reanchor([c])
    with _realigner() as r:
        assert r.reanchor([]) == []
        with pytest.raises(api.CpecanError):
            bad = api.stateMachine5_construct()
            bad.type = 9
            r.set_model(bad)
        r.set_model(api.stateMachine3_construct())
        r.set_model(api.stateMachine5_construct())
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            r.reanchor([c], runs_in=[[(0, 0, 25, 4)]])  # a run that leaves the sequences
        if api.device_count() <= 0:
            with pytest.raises(api.CpecanError, match=r"\(-2\)"):  # CPECAN_ENODEVICE: no realignment without a GPU
                r.reanchor([c])
            with pytest.raises(api.CpecanError, match=r"\(-2\)"):
                r.expectations_on_runs([c], [[(0, 0, 10, 4)]], api.hmm_constructEmpty(0.0, api.fiveState))
    L = realign._lib()
    assert L.cpecan_realigner_reanchor(None, None, 0, None, None) == -1
    assert L.cpecan_realigner_set_model(None, None) == -1
    assert L.cpecan_expect_set_create_runs(None, None, None, 0, None, None) == -1


def test_trainer_argument_checks(tmp_path):
    o = em.em_options()
    assert o.updateTheBand == 0  # the default
    with em.Trainer(em.em_options(updateTheBand=1, randomStart=1, trials=2)) as t:
        with pytest.raises(api.CpecanError, match="updateTheBand"):
            t.set_concurrent_trials(2)
        t.set_concurrent_trials(1)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):  # CPECAN_ESTATE: nothing was trained
            t.alignments()
    with em.Trainer(em.em_options()) as t:
        t.set_concurrent_trials(2)  # without the option as before
        tm = t.timing()
        assert (tm.realignMs, tm.replanMs, tm.handoffMs) == (0.0, 0.0, 0.0)
    assert em._lib().cpecan_em_trainer_alignments(None, None, None, None) == -1


def test_headers_declare_what_the_bindings_export():
    L = em._lib()
    for header, exports in (("cpecan_realign.h", realign.EXPORTS), ("cpecan_em.h", em.EXPORTS)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b(cpecan_[a-z_0-9]+)\s*\(", text))
        assert declared == set(exports), header
        for name in sorted(declared):
            assert hasattr(L, name), name
    hip = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    assert "next_runs" not in hip  # the stage is declared with the realign front end


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_command_line_accepts_the_option_and_refuses_concurrent_trials(tmp_path):
    assert os.path.exists(EXE), "build the command line with make -C cpecan_amd/csrc"
    line = "cpecan_em: --updateTheBand: the sampled alignments are realigned after every iteration"
    res = _run("--sequences", str(tmp_path / "a.fa"), "--alignments", "x", "--updateTheBand")
    assert res.returncode != 0 and line in res.stderr.split("\n") and "cannot open" in res.stderr  # accepted: the files are missing
    res = _run("--sequences", str(tmp_path / "a.fa"), "--alignments", "x", "--updateTheBand", "--concurrentTrials", "2")
    assert res.returncode != 0 and "concurrent trials" in res.stderr and "cannot open" not in res.stderr
    res = _run("--sequences", "a.fa", "--alignments", "x", "--outputXMLModelFile", "m.xml")
    assert res.returncode != 0 and "outputXMLModelFile is not supported" in res.stderr
    assert "--updateTheBand" in _run("--help").stderr


# ---- the preconditions of the GPU cases, on the oracle ----
@pytest.mark.parametrize("name", [c.name for c in nc.all_cases()])
def test_gpu_cases_are_what_they_are_built_for(name):
    """The kernels agree with the oracle to one score unit, so a pair at a threshold could flip an alignment: no posterior
    within 1e-4 of the threshold, no reweighted weight within 1e-4 of matchGamma.  And every case has the shape it is named
    after."""
    c, lists = nc.case(name), nc.oracle_lists(name)
    assert len(lists) == len(c.cigars)
    for chain, (d_thr, d_gamma) in lists:
        assert d_thr >= nc.MARGIN and d_gamma >= nc.MARGIN, (name, d_thr, d_gamma)
    sizes = [len(chain) for chain, _ in lists]
    if name.startswith("identical-"):
        assert sizes == [int(name.split("-")[1])]
    elif name == "straddle":
        trim = c.opts["constraintDiagonalTrim"]
        first = nm.blocks(lists[0][0])[0]
        end = first[0] + first[2] - 1  # the block's last column
        assert trim == 3 and end - trim < 63 < 64 <= end  # its trimmed columns lie on both sides of the chunk edge
        assert nm.blocks(lists[0][0])[1][0] > 64
    elif name == "empty":
        assert sizes == [0]
    elif name == "many-300":
        assert len(sizes) == 300 and sizes[137] == 0 and sum(s > 0 for s in sizes) == 299
    elif name == "minus":
        assert c.cigars[0][7] is False and c.cigars[0][5] > c.cigars[0][6] and sizes[0] > 150
    elif name == "long-1200":
        sx, sy, _ = nc.problems(c)[0]
        assert len(sx) == 1200 and len(sx) + len(sy) > 2 * 1000  # more diagonals than minDiagsBetweenTraceBack: several segments
        assert sizes[0] > 1100 and len(nm.blocks(lists[0][0])) >= 3


def test_em_world_meets_the_precondition_in_every_iteration():
    margins, anchors, running = nc.oracle_em_update_band()
    seqs, cigars = nc.em_world()
    assert len(cigars) == 8 and sum(c[9][-1][0] == nc.DX and len(c[9]) == 2 for c in cigars) == 3  # three misplaced deletions
    assert all(150 <= abs(c[2] - c[1]) <= 300 for c in cigars)
    assert len(margins) == 8 * (nc.EM_ITERATIONS - 1)
    for d_thr, d_gamma in margins:
        assert d_thr >= nc.MARGIN and d_gamma >= nc.MARGIN, (d_thr, d_gamma)
    assert len(running) == nc.EM_ITERATIONS and all(np.isfinite(running))
    # the option does something here: the last anchors are not those of the sampled cigars
    first = [nc.cigar_anchors(*nc.sub_sequences(seqs, c), c[9], 0, nc.EM_E) for c in cigars]
    assert any(tuple(a) != b for a, b in zip(first, anchors))
