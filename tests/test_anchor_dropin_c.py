"""Builds tests/c/test_anchor_dropin.c against include/cpecan_dropin.h + libcpecan_hip.so and runs it: the reference's
getAlignedPairs and getBlastPairsForPairwiseAlignmentParameters on sequences beyond anchorMatrixBiggerThanThis."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cpecan_amd")


def _build(tmp_path):
    exe = str(tmp_path / "test_anchor_dropin")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_anchor_dropin.c"), "-o", exe,
                           "-L", LIBDIR, "-lcpecan_hip", "-lm", "-Wl,-rpath," + LIBDIR])
    return exe


def test_anchor_dropin_builds(tmp_path):
    """The header declares what the C check uses and the library exports it: compiles and links without a GPU."""
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_anchor_dropin_on_gpu(tmp_path):
    r = subprocess.run([_build(tmp_path)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout, r.stdout
