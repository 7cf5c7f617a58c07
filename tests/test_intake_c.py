"""Builds tests/c/test_intake.c together with cpecan_amd/csrc/cpecan_host.c under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it: the add calls in every form against a sequential restatement, and the overflow scan of
a download on hand-made arrays, stand-alone -- no library, no HIP, no GPU.  Leak detection stays on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpecan_amd", "csrc")


def test_intake_and_overflow_scan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_intake")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                           "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "c", "test_intake.c"),
                           os.path.join(CSRC, "cpecan_host.c"), "-o", exe, "-lm", "-lpthread"])
    env = {k: v for k, v in os.environ.items() if k not in ("CPECAN_KEEP_RUNS", "CPECAN_THREADS")}
    r = subprocess.run([exe], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout
