"""Builds tests/c/test_sets_dropin.c against include/cpecan_dropin.h + libcpecan_hip.so and runs it: SeqFrag and
makeAllPairwiseAlignments (inc/multipleAligner.h) as a C caller would use them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cpecan_amd")


def _build(tmp_path):
    exe = str(tmp_path / "test_sets_dropin")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_sets_dropin.c"), "-o", exe,
                           "-L", LIBDIR, "-lcpecan_hip", "-lm", "-Wl,-rpath," + LIBDIR])
    return exe


def _run(exe, mode, cwd):
    r = subprocess.run([exe, mode], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout, r.stdout


def test_sets_dropin_host_side(tmp_path):
    """seqFrag_construct, stIntTuple_construct5, a list without a pair, the similarity score: no GPU needed."""
    _run(_build(tmp_path), "cpu", str(tmp_path))


@pytest.mark.gpu
def test_sets_dropin_all_pairs_on_gpu(tmp_path):
    _run(_build(tmp_path), "gpu", str(tmp_path))
