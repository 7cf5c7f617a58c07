"""The adaptive band of the realign flow (cpecan_realigner_set_adaptive_band) and of the two command lines on the eight
cigars of tests/band_edge_cases.py: five with a 10-base deletion the input cigar pushes to its end, three with the
deletion where it belongs.  E = 4, maxRounds = 3, minEdgeScore S = 1 000 000; tests/test_band_edge_cpu.py holds the
margin that makes the rounds predictable from the oracle's lists."""
import os
import re
import subprocess

import pytest

import band_edge_cases as bc
from cpecan_amd import api, realign

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cigars():
    return [realign.Cigar(nx, 0, len(x), True, ny, 0, len(y), True, 0.0, ops) for nx, x, ny, y, ops, _ in bc.adaptive_inputs()]


def _realigner(**options):
    r = realign.Realigner(options=realign.realign_options(**options))
    for nx, x, ny, y, _, _ in bc.adaptive_inputs():
        r.add_sequence(nx, x)
        r.add_sequence(ny, y)
    return r


def _texts(cigars):
    return [c.format() for c in cigars]


@pytest.fixture(scope="module")
def plain():
    """Every cigar through a realigner without the option at 4, 8, 16 and 32: texts[E][i].  Computed once, read only."""
    out = {}
    for k in range(bc.ADAPTIVE_ROUNDS + 1):
        E = bc.ADAPTIVE_E << k
        with _realigner(diagonalExpansion=E) as r:
            out[E] = tuple(_texts(r.realign(_cigars())))
            assert r.adaptive_rounds() == [0] * 8
    return out


def test_rounds_and_cigars_of_the_adaptive_band(plain):
    want = bc.adaptive_predictions()
    assert sorted(set(want)) == [0, 2]
    with _realigner() as r:
        r.set_adaptive_band(bc.ADAPTIVE_ROUNDS, bc.S)
        got = _texts(r.realign(_cigars()))
        assert r.adaptive_rounds() == want
        assert got == [plain[bc.ADAPTIVE_E << k][i] for i, k in enumerate(want)]
        assert got != list(plain[bc.ADAPTIVE_E])  # the wider band did change the flagged cigars
        # the same cigars as two shards on one device: every shard adapts on its own, the result is per cigar
        r.set_devices([0, 0])
        assert _texts(r.realign(_cigars())) == got and r.adaptive_rounds() == want
        # one round only: the flagged cigars end on round 1, at expansion 8
        r.set_devices([0])
        r.set_adaptive_band(1, bc.S)
        assert _texts(r.realign(_cigars())) == [plain[bc.ADAPTIVE_E << min(k, 1)][i] for i, k in enumerate(want)]
        assert r.adaptive_rounds() == [min(k, 1) for k in want]
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            api._check(realign._lib().cpecan_realigner_adaptive_rounds(r._h, None, 3), "cpecan_realigner_adaptive_rounds")


def test_max_rounds_zero_is_todays_call(plain):
    with _realigner() as r:
        r.set_adaptive_band(2, bc.S)
        r.set_adaptive_band(0)
        assert _texts(r.realign(_cigars())) == list(plain[bc.ADAPTIVE_E]) and r.adaptive_rounds() == [0] * 8
    with _realigner() as r:
        r.set_adaptive_band(0, 0)
        assert _texts(r.realign(_cigars())) == list(plain[bc.ADAPTIVE_E])


def test_split_pieces_are_those_of_the_last_run():
    """splitIndelsLongerThanThis cuts the repaired cigars at their 10-base deletion: the pieces are the plain realigner's at
    the expansion the cigar ended on."""
    want = bc.adaptive_predictions()
    with _realigner(splitIndelsLongerThanThis=5) as r:
        r.set_adaptive_band(bc.ADAPTIVE_ROUNDS, bc.S)
        got = _texts(r.realign(_cigars()))
        assert r.adaptive_rounds() == want
    expect = []
    for E in sorted({bc.ADAPTIVE_E << k for k in want}):
        with _realigner(splitIndelsLongerThanThis=5, diagonalExpansion=E) as r:
            for i, c in enumerate(_cigars()):
                if bc.ADAPTIVE_E << want[i] == E:
                    expect.append((i, _texts(r.realign([c]))))
    assert got == [t for _, pieces in sorted(expect) for t in pieces] and len(got) > 8


def _fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n%s\n" % (name, seq))


def test_cpecan_realign_binary(plain, tmp_path):
    fa = str(tmp_path / "seqs.fa")
    _fasta(fa, [(n, s) for nx, x, ny, y, _, _ in bc.adaptive_inputs() for n, s in ((nx, x), (ny, y))])
    text = "".join(c.format() + "\n" for c in _cigars())
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_realign")
    done = subprocess.run([exe, "--adaptiveBand", str(bc.ADAPTIVE_ROUNDS), "--minEdgeScore", str(bc.S), fa], input=text,
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    want = bc.adaptive_predictions()
    assert done.stdout.splitlines() == [plain[bc.ADAPTIVE_E << k][i] for i, k in enumerate(want)]
    done = subprocess.run([exe, fa], input=text, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.splitlines() == list(plain[bc.ADAPTIVE_E]), done.stderr


def test_cpecan_align_binary(tmp_path):
    """One --adaptiveBand run at expansion 2 against plain runs at the expansion every pair ended on."""
    target, queries = bc.align_inputs()
    tfa, qfa = str(tmp_path / "t.fa"), str(tmp_path / "q.fa")
    _fasta(tfa, [("t", target)])
    _fasta(qfa, [("q%d" % i, q) for i, q in enumerate(queries)])
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")

    def run(*opts):
        done = subprocess.run([exe] + list(opts) + [tfa, qfa], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stderr
        return done.stdout.splitlines(), done.stderr

    got, err = run("-r", str(bc.ALIGN_E), "--adaptiveBand", "2", "--minEdgeScore", str(bc.S))
    ended = [(int(k), int(e)) for k, e in re.findall(r"^cpecan_align: t q\d: round (\d), expansion (\d+)$", err, re.M)]
    assert ended == [(1, 2 * bc.ALIGN_E), (0, bc.ALIGN_E)], err  # the prediction of tests/test_band_edge_cpu.py
    assert len(got) == 2
    by_expansion = {e: run("-r", str(e))[0] for e in {e for _, e in ended}}
    assert got == [by_expansion[e][i] for i, (_, e) in enumerate(ended)]
    # (the detour ran ON the band's last cell at expansion 2, so that run already found it: the flag says the band was
    # tight, not that the cigar is wrong, and the cigar of the wider run may well be the same)
