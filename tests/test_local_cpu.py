"""Local chains without a GPU: every refusal of cpecan_find_local_chains_many comes before the device is looked for, the
header against cpecan_amd.local.EXPORTS, cpecan_cigar_from_local_chain against hand-worked chains and against
cpecan_cigar_from_aligned_pairs, the refusals of cpecan_align --local, and the host stages with the model as the pass."""
import os
import re
import subprocess

import numpy as np
import pytest

import local_cases as lc
import local_model as lm
import local_stages as ls
from cpecan_amd import api, local, realign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = [("ACGT" * 50, "ACGT" * 50)]
no_gpu = pytest.mark.skipif(api.device_count() > 0, reason="asserts what a machine without a device answers")


def _refused(code, **kw):
    with pytest.raises(api.CpecanError) as e:
        local.find_local_chains(kw.pop("problems", PAIR), **kw)
    assert "(%d)" % code in str(e.value), str(e.value)
    return str(e.value)


def _raw_options(**words):
    o = local.local_options()
    for k, v in words.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


@pytest.mark.parametrize("bad", [
    dict(options=_raw_options(maxChains=0)), dict(options=_raw_options(maxChains=17)), dict(options=_raw_options(maxChains=-1)),
    dict(options=_raw_options(minChainScore=-5)), dict(options=_raw_options(minChainScore=799)),
    dict(options=_raw_options(reserved=0)), dict(options=_raw_options(reserved=5)),
    dict(anchor_options="gapped"), dict(anchor_options="reserved"), dict(anchor_options="threshold"),
    dict(strand=3), dict(trim=-1), dict(params="seedTransitions"), dict(device=-1, options=_raw_options(maxChains=0)),
])
def test_every_refusal_is_einval_whatever_the_device(bad):
    """CPECAN_EINVAL (-1), never CPECAN_ENODEVICE (-2): the checks come first, here on a machine that may have no device."""
    kw = dict(bad)
    if kw.get("anchor_options") == "gapped":
        kw["anchor_options"] = api.anchor_options(gappedExtension=1)
    elif kw.get("anchor_options") == "reserved":
        kw["anchor_options"] = api.anchor_options()
        kw["anchor_options"].reserved[6] = 1
    elif kw.get("anchor_options") == "threshold":
        kw["anchor_options"] = api.anchor_options(transitionHspThreshold=10)
    if kw.get("params") == "seedTransitions":
        kw["params"] = api.anchor_params_default(seedTransitions=2)
    _refused(-1, **kw)


def test_minimum_score_at_the_threshold_is_accepted_and_no_device_is_enodevice():
    for kw in (dict(), dict(options=local.local_options(maxChains=16, minChainScore=800)), dict(problems=[])):
        if api.device_count() > 0:
            local.find_local_chains(kw.pop("problems", PAIR), **kw)
        else:
            _refused(-2, **kw)
    _refused(-2, device=10 ** 6)


def test_header_declares_the_exports():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpecan_local.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpecan_\w+)\s*\(", header))
    assert declared == set(local.EXPORTS)
    L = api.lib()
    for name in local.EXPORTS:
        assert getattr(L, name)
    o = local.local_options()
    assert (o.maxChains, o.minChainScore, list(o.reserved)) == (1, 0, [0] * 6)


def _chain(strand, runs, score=1234):
    return dict(strand=strand, score=score, nHsps=len(runs), x0=0, x1=0, y0=0, y1=0, runs=[(x, y, n, 20) for x, y, n in runs])


def test_cigar_of_hand_worked_chains():
    one = local.cigar_of_chain("t", "q", 100, _chain("plus", [(10, 20, 30)]))
    assert one.format() == "cigar: q 20 50 + t 10 40 + 1234.000000 M 30"
    one = local.cigar_of_chain("t", "q", 100, _chain("minus", [(10, 20, 30)]))
    assert one.format() == "cigar: q 80 50 - t 10 40 + 1234.000000 M 30"
    assert (one.start2, one.end2, one.strand2, one.strand1) == (80, 50, False, True)
    three = local.cigar_of_chain("t", "q", 100, _chain("minus", [(10, 20, 5), (17, 25, 3), (20, 30, 4), (30, 40, 1)]))
    assert three.format() == "cigar: q 80 59 - t 10 31 + 1234.000000 M 5 D 2 M 3 I 2 M 4 D 6 I 6 M 1"
    realign.Cigar.parse(three.format())                                    # the operations add up to the coordinates
    for bad in (_chain("plus", []), _chain("plus", [(10, 20, 5), (12, 30, 5)]), _chain("minus", [(0, 90, 20)])):
        with pytest.raises(api.CpecanError) as e:
            local.cigar_of_chain("t", "q", 100, bad)
        assert "(-1)" in str(e.value)


def _merged(ops):
    out = []
    for t, n in ops:
        if out and out[-1][0] == t:
            out[-1] = (t, out[-1][1] + n)
        else:
            out.append((t, n))
    return out


def test_cigar_indel_order_is_that_of_aligned_pairs():
    """On the model's chains: the chain's columns inside its cropped rectangle through cpecan_cigar_from_aligned_pairs give
    the same operations (two runs that touch diagonally are one M there)."""
    seen = set()
    for name in ("inversion", "transposition", "pool_sizes"):
        case = lc.by_name(name)
        for (chains, _), (sx, sy) in zip(lc.model(case), case["problems"]):
            for c in chains:
                got = local.cigar_of_chain("t", "q", len(sy), c)
                r = c["runs"]
                x0, y0 = int(r[0][0]), int(r[0][1])
                x1, y1 = int(r[-1][0] + r[-1][2]), int(r[-1][1] + r[-1][2])
                xy = [(int(x) - x0 + k, int(y) - y0 + k) for x, y, n, _ in r for k in range(int(n))]
                want = realign.Cigar.from_aligned_pairs("t", "q", c["score"], x1 - x0, y1 - y0, xy)
                assert _merged(got.ops) == want.ops, name
                assert (got.start1, got.end1) == (x0, x1) and got.score == c["score"]
                assert (got.start2, got.end2) == ((y0, y1) if c["strand"] == "plus" else (len(sy) - y0, len(sy) - y1))
                seen |= {t for t, _ in got.ops}
    assert seen == {0, 1, 2}                                                # M, D and I all occur


def test_command_line_refusals(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGT\n")
    for args, word in ((["--local", "--gapped"], "--local"), (["--local", "--adaptiveBand", "2", "--minEdgeScore", "5"], "--local"),
                       (["--maxChains", "3"], "need --local"), (["--minChainScore", "900"], "need --local"),
                       (["--local", "--maxChains", "17"], "cpecan_align"), (["--local", "--maxChains", "0"], "cpecan_align")):
        r = subprocess.run([exe] + args + [str(fa), str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and word in r.stderr, (args, r.stderr)


@no_gpu
def test_command_line_local_needs_a_device(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    fa = tmp_path / "a.fa"
    fa.write_text(">a\n" + "ACGT" * 20 + "\n")
    r = subprocess.run([exe, "--local", "--maxChains", "4", str(fa), str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.parametrize("strand", ["both", "plus", "minus"])
def test_host_stages_with_the_model_as_the_pass(strand):
    problems = [(lc.INVERSION_X, lc.INVERSION_Y), ("", "ACGT"), (lc.TRANSPOSITION_X, lc.TRANSPOSITION_Y), ("ACGTACG", lc.A),
                (lc.TIE_S, lc.TIE_S + lc.rc(lc.TIE_S)), lc.UNRELATED, (lc.A, "")]
    for trim, K, S in ((0, 4, 0), (14, 2, 60000)):
        got, stats = ls.run_call(problems, strand=strand, trim=trim, expansion=12, K=K, S=S)
        for (sx, sy), chains, st in zip(problems, got, stats):
            want, wst = lm.local_chains(sx, sy, strand, K, S, trim, 12)
            assert len(chains) == len(want)
            assert all(lm.same(g, w) for g, w in zip(chains, want))
            assert {k: st[k] for k in wst} == wst and st["kernelMs"] == 1.5
