"""Builds tests/c/test_band_edge.c together with cpecan_amd/csrc/cpecan_host.c under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it: cpecan_band_edge_of_pairs over its edge shapes and a few hundred random problems,
stand-alone -- no library, no HIP, no GPU.  Leak detection stays on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpecan_amd", "csrc")


def test_band_edge_of_pairs_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_band_edge")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                           "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "c", "test_band_edge.c"),
                           os.path.join(CSRC, "cpecan_host.c"), "-o", exe, "-lm", "-lpthread"])
    r = subprocess.run([exe], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout
