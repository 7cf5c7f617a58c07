"""Builds tests/c/test_viterbi.c together with cpecan_amd/csrc/cpecan_viterbi.c and cpecan_host.c under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it: the host-only calls of include/cpecan_viterbi.h from C -- argument checks, info against
a restatement of the regions, run without a device, replay and pairs -- stand-alone: no library, no HIP, no GPU.  Leak
detection stays on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpecan_amd", "csrc")


def test_viterbi_host_code_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_viterbi")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                           "-ffp-contract=off", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_viterbi.c"), os.path.join(CSRC, "cpecan_viterbi.c"),
                           os.path.join(CSRC, "cpecan_host.c"), "-o", exe, "-lm", "-lpthread"])
    r = subprocess.run([exe], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout
