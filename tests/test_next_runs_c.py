"""Builds tests/c/test_next_runs.c together with cpecan_amd/csrc/cpecan_host.c under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it: cpecan_next_runs_of_pairs over its edge shapes and two thousand random chains,
stand-alone -- no library, no HIP, no GPU.  Leak detection stays on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpecan_amd", "csrc")


def test_next_runs_of_pairs_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_next_runs")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                           "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "c", "test_next_runs.c"),
                           os.path.join(CSRC, "cpecan_host.c"), "-o", exe, "-lm", "-lpthread"])
    r = subprocess.run([exe], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout
