"""Local chains with gapped extension (cpecan_find_local_chains_many_gapped) without a GPU:
every refusal of the new entry point comes before the device is looked for, the header against cpecan_amd.local.EXPORTS, the
refusals of cpecan_align --extendChains / --chainYDrop, and the host stages of cpecan_local.c with the model
(tests/local_model_gapped.py) in the place of the pass."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import anchor_model as am
import anchor_stages as ast
import local_gapped_cases as gc
import local_model as lm
import local_model_gapped as lmg
import local_stages as ls
from cpecan_amd import api, local

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = [("ACGT" * 50, "ACGT" * 50)]
GAPPED, DIAGS_SHIFT = 4, 8                                   # CPK_ANCHOR_GAPPED, CPK_ANCHOR_DIAGS_SHIFT of cpecan_internal.h


def _refused(code, **kw):
    with pytest.raises(api.CpecanError) as e:
        local.find_local_chains(kw.pop("problems", PAIR), gapped=True, **kw)
    assert "(%d)" % code in str(e.value), str(e.value)
    assert "cpecan_find_local_chains_many_gapped" in str(e.value)
    return str(e.value)


def _options(**words):
    o = local.local_options()
    for k, v in words.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


def _anchor_options(reserved=None, **kw):
    o = api.anchor_options(**kw)
    if reserved is not None:
        o.reserved[reserved] = 1
    return o


@pytest.mark.parametrize("bad", [
    dict(options=_options(maxChains=0)), dict(options=_options(maxChains=17)), dict(options=_options(minChainScore=-5)),
    dict(options=_options(minChainScore=799)), dict(options=_options(reserved=0)), dict(options=_options(reserved=5)),
    dict(anchor=dict(gappedExtension=2)), dict(anchor=dict(gappedExtension=-1)), dict(anchor=dict(gappedExtension=1, yDrop=-1)),
    dict(anchor=dict(gappedExtension=1, gappedMaxDiagonals=63)), dict(anchor=dict(gappedExtension=1, gappedMaxDiagonals=4097)),
    dict(anchor=dict(gappedExtension=0, yDrop=600)), dict(anchor=dict(gappedExtension=0, gappedMaxDiagonals=64)),
    dict(anchor=dict(gappedExtension=1, reserved=3)), dict(anchor=dict(gappedExtension=1, transitionHspThreshold=10)),
    dict(strand=3), dict(trim=-1), dict(params="seedTransitions"), dict(device=-1, options=_options(maxChains=0)),
])
def test_every_refusal_is_einval_whatever_the_device(bad):
    """CPECAN_EINVAL (-1), never CPECAN_ENODEVICE (-2): the checks come first, here on a machine that may have no device."""
    kw = dict(bad)
    if "anchor" in kw:
        kw["anchor_options"] = _anchor_options(**kw.pop("anchor"))
    if kw.get("params") == "seedTransitions":
        kw["params"] = api.anchor_params_default(seedTransitions=2)
    _refused(-1, **kw)


def test_what_is_admitted_reaches_the_device_check():
    """gappedExtension = 1 with its two values, and the keyword alone: accepted, so a machine without a device says ENODEVICE;
    the entry point of before still refuses the option."""
    for kw in (dict(), dict(anchor_options=api.anchor_options(gappedExtension=1, yDrop=600, gappedMaxDiagonals=64)),
               dict(anchor_options=api.anchor_options(gappedExtension=1, gappedMaxDiagonals=4096)),
               dict(anchor_options=api.anchor_options()), dict(problems=[])):
        if api.device_count() > 0:
            local.find_local_chains(kw.pop("problems", PAIR), gapped=True, **kw)
        else:
            _refused(-2, **kw)
    _refused(-2, device=10 ** 6)
    with pytest.raises(api.CpecanError) as e:
        local.find_local_chains(PAIR, anchor_options=api.anchor_options(gappedExtension=1))
    assert "(-1)" in str(e.value)


def test_header_declares_the_exports():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpecan_local.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpecan_\w+)\s*\(", header))
    assert declared == set(local.EXPORTS) and "cpecan_find_local_chains_many_gapped" in declared
    many, gapped = (re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1).split() for name in
                    ("cpecan_find_local_chains_many", "cpecan_find_local_chains_many_gapped"))
    assert many == gapped                                                   # the argument list of the entry point of before
    L = api.lib()
    for name in local.EXPORTS:
        assert getattr(L, name)
    # the structures keep their layout
    assert (C.sizeof(local.LocalOptions), C.sizeof(local.LocalChain), C.sizeof(local.LocalStats)) == (32, 64, 48)


def test_command_line_refusals(tmp_path):
    exe = os.path.join(ROOT, "cpecan_amd", "cpecan_align")
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGT\n")
    for args, word in ((["--extendChains"], "need --local"), (["--chainYDrop", "600"], "need --local"),
                       (["--extendChains", "--chainYDrop", "600"], "need --local"),
                       (["--local", "--chainYDrop", "600"], "--chainYDrop needs --extendChains"),
                       (["--local", "--extendChains", "--chainYDrop", "0"], "cpecan_align"),
                       (["--local", "--extendChains", "--gapped"], "--local does not go with --gapped"),
                       (["--local", "--gapped"], "--local does not go with --gapped")):
        r = subprocess.run([exe] + args + [str(fa), str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and word in r.stderr, (args, r.stderr)
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and "--extendChains" in r.stderr and "--chainYDrop" in r.stderr


def _model_pass(sym, lst, lprobs, nLocal, pass_, lpass, params, nForward):
    """cpk_local_pass played by the model, as local_stages.model_pass does it, for a list whose problems carry step 7b: the
    three options are read back from the problems, where the host put them."""
    ast.check_plan(pass_, lst.probs, lst.n, len(sym), nForward)
    K = lpass.maxChains
    chains = (ls.PassChain * max(1, nLocal * K))()
    found = []
    for k in range(nLocal):
        q = lprobs[k]
        p = lst.probs[q.first]
        x = bytes(sym[p.xOff:p.xOff + p.lX])
        fwd = p.yFwd if p.flags & ast.RC_Y else p.yOff
        y = bytes(sym[fwd:fwd + p.lY])
        strand = "both" if q.twins == 2 else "minus" if p.flags & ast.RC_Y else "plus"
        for t in range(q.twins):                            # every twin carries the same three values
            pt = lst.probs[q.first + t]
            assert (pt.flags & GAPPED, pt.flags >> DIAGS_SHIFT, pt.pad) == (p.flags & GAPPED, p.flags >> DIAGS_SHIFT, p.pad)
        gapped = int(bool(p.flags & GAPPED))
        got, st = lmg.local_chains(x, y, strand, K, lpass.minChainScore, pass_.trim, 0, params, gapped=gapped,
                                   yDrop=p.pad if gapped else 0, gappedMaxDiagonals=(p.flags >> DIAGS_SHIFT) if gapped else 0)
        triples = []
        for j, c in enumerate(got):
            rec = chains[k * K + j]
            rec.strand, rec.score, rec.nHsps = api.STRAND_NAMES.index(c["strand"]), c["score"], c["nHsps"]
            rec.x0, rec.x1, rec.y0, rec.y1 = c["x0"], c["x1"], c["y0"], c["y1"]
            rec.runOff, rec.nRuns = len(triples) // 3, len(c["runs"])
            triples += [int(v) for r in c["runs"].tolist() for v in r[:3]]
        q.nChains, q.nRuns, q.rounds = len(got), len(triples) // 3, st["rounds"]
        for t in range(q.twins):
            pt = lst.probs[q.first + t]
            o = "Minus" if pt.flags & ast.RC_Y else "Plus"
            pt.hits, pt.hsps, pt.capped = st["hits" + o], st["hsps" + o], (st["capped"] >> (o == "Minus")) & 1
        found.append(triples)
    flat = []
    for k in reversed(range(nLocal)):                       # a run list of its own: only hspOff says where a problem's runs lie
        flat += [-7, -7, -7]
        lst.probs[lprobs[k].first].hspOff = len(flat) // 3
        flat += found[k]
    return chains, (C.c_int32 * max(1, len(flat)))(*flat)


def _run_call(problems, strand, trim, expansion, K, anchor_options, want_flags):
    """cpecan_find_local_chains_many_gapped of cpecan_local.c with _model_pass for the device."""
    L = ls.stages()
    L.cpk_local_check_gapped.argtypes = L.cpk_local_check.argtypes
    L.cpk_local_mark_gapped.argtypes = [C.POINTER(ast.List), C.POINTER(api.AnchorOptions)]
    L.cpk_local_mark_gapped.restype = None
    arr, n, keep = api._anchor_problems(problems)
    chains, nChains = (C.POINTER(local.LocalChain) * max(1, n))(), (C.c_int64 * max(1, n))()
    runs, nRuns = (ls.i64p * max(1, n))(), (C.c_int64 * max(1, n))()
    stats = (local.LocalStats * max(1, n))()
    call = ls.Call(b"run_call", arr, n, expansion, 0, api._strand_mode(strand), chains, nChains, runs, nRuns, stats)
    pass_, lpass, params = ast.Pass(), ls.LocalPass(), am.default_params()
    opts = local.local_options(maxChains=K)
    ao = C.byref(anchor_options) if anchor_options is not None else None
    assert L.cpk_local_check(C.byref(call), trim, None, ao, C.byref(opts), C.byref(pass_), C.byref(lpass)) == (-1 if want_flags else 0)
    assert L.cpk_local_check_gapped(C.byref(call), trim, None, ao, C.byref(opts), C.byref(pass_), C.byref(lpass)) == 0, L.cpecan_last_error()
    top, raw, lprobs = ast.List(), C.POINTER(C.c_uint8)(), C.POINTER(ls.LocalProblem)()
    nBytes, nExtra, nLocal = C.c_int64(), C.c_int64(), C.c_int64()
    try:
        assert L.cpk_local_layout(C.byref(call), C.byref(top), C.byref(raw), C.byref(nBytes), C.byref(nExtra), C.byref(lprobs),
                                  C.byref(nLocal)) == 0
        L.cpk_local_mark_gapped(C.byref(top), ao)
        for k in range(top.n):
            p = top.probs[k]
            assert (p.flags & GAPPED, p.flags >> DIAGS_SHIFT, p.pad) == want_flags if want_flags else (p.flags >> 2, p.pad) == (0, 0)
        nForward = nBytes.value
        nSym = ((nForward + 1) & ~1) + nExtra.value if nExtra.value else nForward
        sym = bytearray(C.string_at(raw, nForward)) + bytearray(nSym - nForward)
        recs, triples = _model_pass(sym, top, lprobs, nLocal.value, pass_, lpass, params, nForward)
        assert L.cpk_local_assemble(C.byref(call), C.byref(top), lprobs, nLocal.value, recs, triples, K, 2.5) == 0
        out = []
        for i in range(n):
            mine = []
            for j in range(nChains[i]):
                c = chains[i][j]
                r = np.array([runs[i][4 * u + v] for u in range(c.runOff, c.runOff + c.nRuns) for v in range(4)], dtype=np.int64)
                mine.append(dict(strand=api.STRAND_NAMES[c.strand], score=c.score, nHsps=c.nHsps, x0=c.x0, x1=c.x1, y0=c.y0,
                                 y1=c.y1, runs=r.reshape(-1, 4)))
            out.append(mine)
        return out, [stats[i].as_dict() for i in range(n)]
    finally:
        for i in range(n):
            L.cpecan_free(C.cast(chains[i], C.c_void_p))
            L.cpecan_free(C.cast(runs[i], C.c_void_p))
        L.cpecan_free(C.cast(raw, C.c_void_p))
        L.cpecan_free(C.cast(lprobs, C.c_void_p))
        L.cpk_anchor_list_free(C.byref(top))


@pytest.mark.parametrize("strand", ["both", "plus", "minus"])
def test_host_stages_with_the_model_as_the_pass(strand):
    """The option reaches the pass in the problems' flags and yDrop, and what the pass hands back -- chains with more runs
    than HSPs, in a list only hspOff points to -- becomes the caller's arrays."""
    problems = [gc.inversion_pair(), ("", "ACGT"), gc.shared_middle_pair(), ("ACGTACG", "ACGT" * 30), gc.end_gap_pairs()[1]]
    for trim, K, ao, flags, (y, d) in ((0, 4, api.anchor_options(gappedExtension=1), (GAPPED, 4096, 9400), (0, 0)),
                                       (14, 2, api.anchor_options(gappedExtension=1, yDrop=600, gappedMaxDiagonals=64),
                                        (GAPPED, 64, 600), (600, 64)),
                                       (0, 3, None, None, (0, 0)), (0, 3, api.anchor_options(), None, (0, 0))):
        got, stats = _run_call(problems, strand, trim, 12, K, ao, flags)
        more = 0
        for (sx, sy), chains, st in zip(problems, got, stats):
            want, wst = lmg.local_chains(sx, sy, strand, K, 0, trim, 12, gapped=int(flags is not None), yDrop=y, gappedMaxDiagonals=d)
            assert len(chains) == len(want)
            assert all(lm.same(g, w) for g, w in zip(chains, want))
            assert {k: st[k] for k in wst} == wst and st["kernelMs"] == 2.5
            more += sum(len(c["runs"]) > c["nHsps"] for c in chains)
        assert flags is None or trim or more > 0
