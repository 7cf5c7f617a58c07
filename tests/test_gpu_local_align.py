"""cpecan_align --local on the GPU: the command line gives, line for line, the texts of cpecan_amd.local.align_local, which
are Realigner.realign on cigar_of_chain of find_local_chains; every line is a cigar cpecan_cigar_parse accepts.  Without
--local the binary prints the bytes it printed before the option existed (tests/golden/local_align_*.txt, recorded from a
build of the commit before it)."""
import os
import subprocess

import pytest

import local_cases as lc
from cpecan_amd import local, realign

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
PAIRS = {"inversion": (lc.INVERSION_X, lc.INVERSION_Y), "transposition": (lc.TRANSPOSITION_X, lc.TRANSPOSITION_Y)}


def write_fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s a header word\n" % name)
        for i in range(0, len(seq), 70):
            f.write(seq[i:i + 70] + "\n")


def _files(tmp_path, name):
    sx, sy = PAIRS[name]
    t, q = str(tmp_path / "target.fa"), str(tmp_path / "query.fa")
    write_fasta(t, "target_" + name, sx)
    write_fasta(q, "query_" + name, sy)
    return t, q


def _run(args):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("name,strand", [("inversion", "both"), ("inversion", "minus"), ("transposition", "both")])
def test_command_line_equals_align_local_equals_the_realigner(tmp_path, name, strand):
    """The command line has the default anchor parameters.  With those every segment of the inversion case is one long HSP
    that runs a few chance matches into its neighbours, so BOTH keeps the plus chain alone (the
    kill rule); the inverted segment is what --strand minus finds.  The transposition gives two plus chains."""
    sx, sy = PAIRS[name]
    t, q = _files(tmp_path, name)
    lines = _run(["--local", "--strand", strand, "--maxChains", "4", t, q]).splitlines()
    targets, queries = {"target_" + name: sx}, {"query_" + name: sy}
    options = local.local_options(maxChains=4)
    ro = realign.realign_options(gapGamma=0.5)
    got = local.align_local(targets, queries, realign_options=ro, trim=0, options=options, strand=strand)
    assert lines == [c.format() for c in got] and len(lines) >= (2 if name == "transposition" else 1)
    # the same, step by step
    chains, _ = local.find_local_chains([(sx, sy)], trim=0, options=options, strand=strand)
    cigars = [local.cigar_of_chain("target_" + name, "query_" + name, len(sy), c) for c in chains[0]]
    with realign.Realigner(None, ro) as r:
        r.add_sequence("target_" + name, sx)
        r.add_sequence("query_" + name, sy)
        assert [c.format() for c in r.realign(cigars)] == lines
    for line, first in zip(lines, cigars):
        c = realign.Cigar.parse(line)                                      # cpecan_cigar_parse: the operations add up
        assert (c.contig1, c.contig2, c.strand1, c.strand2) == (first.contig1, first.contig2, True, first.strand2)
        assert first.start1 <= c.start1 < c.end1 <= first.end1
        assert c.strand2 == (strand != "minus")
        assert sum(n for op, n in c.ops if op == 0) > (c.end1 - c.start1) // 2      # mostly matches: the segment is aligned


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_without_local_the_output_is_what_it_was(tmp_path, name):
    t, q = _files(tmp_path, name)
    for strand in ("plus", "both"):
        want = open(os.path.join(ROOT, "tests", "golden", "local_align_%s_%s.txt" % (name, strand))).read()
        assert _run(["--strand", strand, t, q]) == want
