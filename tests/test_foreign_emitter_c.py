"""Builds tests/c/test_foreign_emitter.c against include/cpecan_dropin.h + libcpecan_hip.so and runs it on cases (a)-(f) and (h)
of tests/dense_cases.py: a C caller's OWN per-diagonal emitter through getPosteriorProbsWithBanding and
getPosteriorProbsWithBandingSplittingAlignmentsByLargeGaps, held against the three token emitters and against the live-row
contract of cpecan_dense_schedule (the program's header says how).  The expectation sums the foreign emitter accumulates are
then held against the oracle's here.  A second, stand-alone program puts the host side of the dense layer and the replay
under AddressSanitizer and UndefinedBehaviorSanitizer on fabricated rows: no library, no HIP, no GPU."""
import os
import subprocess

import numpy as np
import pytest

import dense_cases as dc
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cpecan_amd")
CSRC = os.path.join(LIBDIR, "csrc")

# fp64 exp over log-space values that agree with the oracle's to parity.LOG_TOL, summed in fp64 on both sides
EXPECT_REL = 1e-9


def _all_cases():
    return dc.cases() + (dc.split_case(),)


def _write_cases(path):
    with open(path, "w") as f:
        f.write("%d\n" % len(_all_cases()))
        for c in _all_cases():
            lib_model = dc.model_pair(c.model)[0]
            f.write("%s %d " % (c.name, lib_model.type))
            if c.model == "threeStateAsymInf":
                ph = dc.inf_hmm()[0]
                f.write("1 " + " ".join(float(ph.transitions[i]).hex() for i in range(9)) + " " +
                        " ".join(float(ph.emissions[i]).hex() for i in range(48)) + "\n")
            else:
                f.write("0\n")
            p = dc.lib_params(c)
            f.write("%s %d %d %d %d %d %d %d\n" % (float(p.threshold).hex(), p.minDiagsBetweenTraceBack, p.traceBackDiagonals,
                                                   p.diagonalExpansion, p.splitMatrixBiggerThanThis, p.dynamicAnchorExpansion,
                                                   int(c.ragged_left), int(c.ragged_right)))
            f.write("%d %s %d %s\n" % (len(c.sx), c.sx.decode() or "-", len(c.sy), c.sy.decode() or "-"))
            a = dc.anchors_of(c)
            f.write("%d %s\n" % (len(a), " ".join("%d %d %d" % t for t in a)))


@pytest.mark.gpu
def test_foreign_emitters_through_both_entry_points(tmp_path):
    exe, cases, out = str(tmp_path / "test_foreign_emitter"), str(tmp_path / "cases.txt"), str(tmp_path / "expectations.txt")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_foreign_emitter.c"), "-o", exe,
                           "-L", LIBDIR, "-lcpecan_hip", "-lm", "-Wl,-rpath," + LIBDIR])
    _write_cases(cases)
    r = subprocess.run([exe, cases, out], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert "0 failure(s)" in r.stdout, r.stdout[-6000:]
    # the sums of the foreign expectation emitter against the oracle's
    by_name = {c.name: c for c in _all_cases()}
    worst, seen = 0.0, set()
    for line in open(out):
        tok = line.split()
        c, split, S = by_name[tok[0]], int(tok[1]), int(tok[2])
        got = np.array([float(v) for v in tok[3:]])
        assert len(got) == S * S + S * 16 + 1
        om = dc.model_pair(c.model)[1]
        p = dc.oracle_params(c)
        if not split:  # getPosteriorProbsWithBanding: one region whatever its size
            p.splitMatrixBiggerThanThis = 2 ** 62
        acc = ob.hmm(om.type, 0.0)
        ob.expectations(om, acc, c.sx, c.sy, dc.anchors_of(c), p, c.ragged_left, c.ragged_right)
        want = np.array([acc.T[i] for i in range(S * S)] + [acc.E[i] for i in range(S * 16)] + [acc.likelihood])
        assert np.array_equal(got == 0, want == 0), (c.name, split)
        nz = want != 0
        if nz.any():
            rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= EXPECT_REL), (c.name, split, float(rel.max()))
        seen.add((c.name, split))
    print("largest relative difference of an expectation entry, foreign against oracle: %.3g" % worst)
    assert seen == {(c.name, s) for c in _all_cases() for s in (0, 1)}


def test_dense_host_side_and_replay_under_the_sanitizers(tmp_path):
    """cpecan_dense.c and the replay of cpecan_dropin.c with fabricated rows in place of the device layer."""
    exe = str(tmp_path / "test_dense_replay")
    srcs = [os.path.join(ROOT, "tests", "c", "test_dense_replay.c")] + [os.path.join(CSRC, f) for f in (
        "cpecan_dense.c", "cpecan_dropin.c", "cpecan_host.c", "cpecan_sets.c", "cpecan_realign.c", "cpecan_anchor.c", "cpecan_em.c")]
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-fopenmp",
                           "-ffunction-sections", "-Wl,--gc-sections", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + srcs +
                          ["-o", exe, "-lm", "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CPECAN_")}
    r = subprocess.run([exe], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-6000:]
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-6000:]
