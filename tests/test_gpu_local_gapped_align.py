"""cpecan_align --local --extendChains on the GPU: the command line gives, line for line, the texts of
cpecan_amd.local.align_local(gapped=True), which are Realigner.realign on the cigars of the model's chains
(tests/local_model_gapped.py).  Without the new options --local prints the bytes it printed before they existed
(tests/golden/local_gapped_align_*.txt, recorded from a build of the commit before them)."""
import os
import subprocess

import pytest

import anchor_model as am
import local_gapped_cases as gc
import local_model_gapped as lmg
from cpecan_amd import api, local, realign

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
PAIRS = {"inversion": (gc.inversion_pair(), "both"), "shared_middle": (gc.shared_middle_pair(), "plus")}


def write_fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s a header word\n" % name)
        for i in range(0, len(seq), 70):
            f.write(seq[i:i + 70] + "\n")


def _files(tmp_path, name):
    (sx, sy), _ = PAIRS[name]
    t, q = str(tmp_path / "target.fa"), str(tmp_path / "query.fa")
    write_fasta(t, "target_" + name, sx)
    write_fasta(q, "query_" + name, sy)
    return t, q


def _run(args):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("name,yDrop", [("inversion", 0), ("shared_middle", 0), ("inversion", 600)])
def test_command_line_equals_align_local_equals_the_realigner_on_the_model(tmp_path, name, yDrop):
    """The command line has the default anchor parameters (one long HSP per segment), so the extension works at the chains'
    ends and across the indels next to them."""
    (sx, sy), strand = PAIRS[name]
    t, q = _files(tmp_path, name)
    args = ["--local", "--extendChains"] + (["--chainYDrop", str(yDrop)] if yDrop else [])
    lines = _run(args + ["--strand", strand, "--maxChains", "4", t, q]).splitlines()
    targets, queries = {"target_" + name: sx}, {"query_" + name: sy}
    options = local.local_options(maxChains=4)
    ro = realign.realign_options(gapGamma=0.5)
    ao = api.anchor_options(gappedExtension=1, yDrop=yDrop)
    got = local.align_local(targets, queries, realign_options=ro, trim=0, options=options, strand=strand, gapped=True,
                            anchor_options=ao if yDrop else None)
    assert lines == [c.format() for c in got] and len(lines) >= 1
    # the realigner on the model's chains
    chains, _ = lmg.local_chains(sx, sy, strand, 4, 0, 0, 20, am.default_params(), gapped=1, yDrop=yDrop)
    assert any(len(c["runs"]) > c["nHsps"] for c in chains)                 # the extension did something here
    cigars = [local.cigar_of_chain("target_" + name, "query_" + name, len(sy), c) for c in chains]
    with realign.Realigner(None, ro) as r:
        r.add_sequence("target_" + name, sx)
        r.add_sequence("query_" + name, sy)
        assert [c.format() for c in r.realign(cigars)] == lines
    for line in lines:
        realign.Cigar.parse(line)                                           # cpecan_cigar_parse: the operations add up
    plain = _run(["--local", "--strand", strand, "--maxChains", "4", t, q]).splitlines()
    assert len(plain) == len(lines)                                         # the peel is the same; the chains are longer


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_without_the_new_options_local_prints_what_it_printed(tmp_path, name):
    _, strand = PAIRS[name]
    t, q = _files(tmp_path, name)
    want = open(os.path.join(ROOT, "tests", "golden", "local_gapped_align_%s.txt" % name)).read()
    assert want.count("\n") >= 1
    assert _run(["--local", "--strand", strand, "--maxChains", "4", t, q]) == want
