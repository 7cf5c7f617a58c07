"""Builds tests/c/test_local_gapped_plan.c together with cpecan_amd/csrc/cpecan_local.c and cpecan_anchor.c under
AddressSanitizer and UndefinedBehaviorSanitizer and runs it: the host code of cpecan_find_local_chains_many_gapped over
synthetic passes that extend their chains, stand-alone -- no library, no HIP, no GPU.  Leak detection stays on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpecan_amd", "csrc")


def test_gapped_local_stages_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_local_gapped_plan")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "c", "test_local_gapped_plan.c"),
                           os.path.join(CSRC, "cpecan_local.c"), os.path.join(CSRC, "cpecan_anchor.c"), "-o", exe])
    r = subprocess.run([exe], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "0 failure(s)" in r.stdout and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout
