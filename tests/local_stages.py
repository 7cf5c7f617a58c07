"""The host stages of the local chains (cpecan_internal.h: cpk_local_check, _layout, _assemble) reached through ctypes, with
the model in the device's place: run_call is cpecan_find_local_chains_many of cpecan_local.c with model_pass where
cpk_local_pass stands.  Nothing here needs a GPU.  The structures mirror cpecan_internal.h field for field."""
import ctypes as C

import anchor_model as am
import anchor_stages as ast
import local_model as lm
import strand_model as sm
from cpecan_amd import api, local

i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


class LocalProblem(C.Structure):
    """CpkLocalProblem."""
    _fields_ = [("first", C.c_int64), ("twins", C.c_int32), ("nChains", C.c_int32), ("nRuns", C.c_int32), ("rounds", C.c_int32)]


class PassChain(C.Structure):
    """CpkLocalChain."""
    _fields_ = [(k, C.c_int32) for k in ("strand", "score", "nHsps", "runOff", "nRuns", "x0", "x1", "y0", "y1", "pad")]


class LocalPass(C.Structure):
    """CpkLocalPass."""
    _fields_ = [("maxChains", C.c_int32), ("minChainScore", C.c_int32)]


class Call(C.Structure):
    """CpkLocalCall."""
    _fields_ = [("who", C.c_char_p), ("problems", C.POINTER(api.AnchorProblem)), ("n", C.c_int64), ("expansion", C.c_int64),
                ("device", C.c_int32), ("strandMode", C.c_int32), ("chains", C.POINTER(C.POINTER(local.LocalChain))),
                ("nChains", i64p), ("runs", C.POINTER(i64p)), ("nRuns", i64p), ("stats", C.POINTER(local.LocalStats))]


def stages():
    L = ast.stages()
    local._lib()
    if getattr(L, "_local_stages_bound", False):
        return L
    call, lst = C.POINTER(Call), C.POINTER(ast.List)
    L.cpk_local_check.argtypes = [call, C.c_int64, C.POINTER(api.AnchorParams), C.POINTER(api.AnchorOptions),
                                  C.POINTER(local.LocalOptions), C.POINTER(ast.Pass), C.POINTER(LocalPass)]
    L.cpk_local_layout.argtypes = [call, lst, C.POINTER(C.POINTER(C.c_uint8)), i64p, i64p, C.POINTER(C.POINTER(LocalProblem)), i64p]
    L.cpk_local_assemble.argtypes = [call, lst, C.POINTER(LocalProblem), C.c_int64, C.POINTER(PassChain), i32p, C.c_int32, C.c_double]
    L._local_stages_bound = True
    return L


def model_pass(sym, lst, lprobs, nLocal, pass_, lpass, params, nForward):
    """cpk_local_pass played by the model: fills hits / hsps / capped of the list's problems, the counts of lprobs, and
    returns (chain records, run triples).  The run blocks lie in reverse list order behind a poisoned triple, as
    anchor_stages.model_pass lays them: the host may rely on hspOff alone."""
    ast.check_plan(pass_, lst.probs, lst.n, len(sym), nForward)
    K = lpass.maxChains
    chains = (PassChain * max(1, nLocal * K))()
    found = []
    for k in range(nLocal):
        q = lprobs[k]
        p = lst.probs[q.first]
        assert q.twins in (1, 2) and (q.twins == 1 or lst.probs[q.first + 1].flags & ast.SHARE_X)
        x = bytes(sym[p.xOff:p.xOff + p.lX])
        fwd = p.yFwd if p.flags & ast.RC_Y else p.yOff
        y = bytes(sym[fwd:fwd + p.lY])
        strand = "both" if q.twins == 2 else "minus" if p.flags & ast.RC_Y else "plus"
        got, st = lm.local_chains(x, y, strand, K, lpass.minChainScore, pass_.trim, 0, params)
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
    for k in reversed(range(nLocal)):
        flat += [-7, -7, -7]
        lst.probs[lprobs[k].first].hspOff = len(flat) // 3
        flat += found[k]
    return chains, (C.c_int32 * max(1, len(flat)))(*flat)


def run_call(problems, strand="both", trim=0, expansion=20, K=4, S=0):
    """cpecan_find_local_chains_many with the default parameters and model_pass for the device: ([chains per problem] as
    cpecan_amd.local.find_local_chains returns them, [statistics dict])."""
    import numpy as np
    L = stages()
    arr, n, keep = api._anchor_problems(problems)
    chains, nChains = (C.POINTER(local.LocalChain) * max(1, n))(), (C.c_int64 * max(1, n))()
    runs, nRuns = (i64p * max(1, n))(), (C.c_int64 * max(1, n))()
    stats = (local.LocalStats * max(1, n))()
    call = Call(b"run_call", arr, n, expansion, 0, api._strand_mode(strand), chains, nChains, runs, nRuns, stats)
    pass_, lpass, params = ast.Pass(), LocalPass(), am.default_params()
    opts = local.local_options(maxChains=K, minChainScore=S)
    assert L.cpk_local_check(C.byref(call), trim, None, None, C.byref(opts), C.byref(pass_), C.byref(lpass)) == 0, L.cpecan_last_error()
    assert (lpass.maxChains, lpass.minChainScore) == (K, S or params["hspThreshold"])
    top, raw, lprobs = ast.List(), C.POINTER(C.c_uint8)(), C.POINTER(LocalProblem)()
    nBytes, nExtra, nLocal = C.c_int64(), C.c_int64(), C.c_int64()
    try:
        assert L.cpk_local_layout(C.byref(call), C.byref(top), C.byref(raw), C.byref(nBytes), C.byref(nExtra), C.byref(lprobs),
                                  C.byref(nLocal)) == 0
        assert nLocal.value == sum(1 for pr in problems if len(pr[0]) and len(pr[1]))
        if top.n:
            nForward = nBytes.value
            nSym = ((nForward + 1) & ~1) + nExtra.value if nExtra.value else nForward
            sym = bytearray(C.string_at(raw, nForward)) + bytearray(nSym - nForward)
            recs, triples = model_pass(sym, top, lprobs, nLocal.value, pass_, lpass, params, nForward)
            assert L.cpk_local_assemble(C.byref(call), C.byref(top), lprobs, nLocal.value, recs, triples, K, 1.5) == 0
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
