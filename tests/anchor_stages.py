"""The anchor finder's host stages (cpecan_internal.h: cpk_anchor_check, _layout, _pick, _gaps, _splice, _pass_plan) reached
through ctypes, with the model in the device's place: run_call is find_runs of cpecan_anchor.c with model_pass where
cpk_anchor_pass stands.  Nothing here needs a GPU.  The structures mirror cpecan_internal.h field for field; the sizes are
asserted in tests/test_anchor_stages_cpu.py."""
import ctypes as C

import anchor_model as am
import strand_model as sm
from cpecan_amd import api

RC_Y, SHARE_X = 1, 2
OK, EINVAL = 0, -1
i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


class PassProblem(C.Structure):
    """CpkAnchorProblem."""
    _fields_ = [("xOff", C.c_int64), ("yOff", C.c_int64), ("lX", C.c_int32), ("lY", C.c_int32), ("softMask", C.c_int32),
                ("capX", C.c_int32), ("capY", C.c_int32), ("hspCap", C.c_int32), ("keyXOff", C.c_int64),
                ("keyYOff", C.c_int64), ("hspOff", C.c_int64), ("hits", C.c_int32), ("hsps", C.c_int32),
                ("chained", C.c_int32), ("nRuns", C.c_int32), ("capped", C.c_int32), ("flags", C.c_int32),
                ("columns", C.c_int64), ("yFwd", C.c_int64), ("score", C.c_int32), ("pad", C.c_int32)]


class PassParams(C.Structure):
    """CpkAnchorParams."""
    _fields_ = [("scores", C.c_int32 * 25), ("maxSeedOccurrences", C.c_int32), ("xDrop", C.c_int32),
                ("hspThreshold", C.c_int32), ("maxHsps", C.c_int32)]


class Pass(C.Structure):
    """CpkAnchorPass."""
    _fields_ = [("prm", PassParams), ("seed", C.c_char * 32), ("seedTransitions", C.c_int32),
                ("variantThreshold", C.c_int32), ("trim", C.c_int32)]


class PlanSeed(C.Structure):
    _fields_ = [("span", C.c_int32), ("weight", C.c_int32), ("pos", C.c_uint8 * 16)]


class Plan(C.Structure):
    """CpkAnchorPlan."""
    _fields_ = [("seed", PlanSeed), ("transitions", C.c_int32), ("maxCap", C.c_int32), ("maxRc", C.c_int32),
                ("maxHits", C.c_int32), ("hitsPerWindow", C.c_int64), ("nKeys", C.c_int64), ("nSlots", C.c_int64),
                ("nCounters", C.c_int64)]


class Call(C.Structure):
    """CpkAnchorCall."""
    _fields_ = [("who", C.c_char_p), ("problems", C.POINTER(api.AnchorProblem)), ("n", C.c_int64), ("expansion", C.c_int64),
                ("anchorMatrixBiggerThanThis", C.c_int64), ("repeatMaskMatrixBiggerThanThis", C.c_int64),
                ("device", C.c_int32), ("strandMode", C.c_int32), ("once", C.c_int32), ("softMaskTop", C.c_int32),
                ("runs", C.POINTER(i64p)), ("nRuns", i64p), ("stats", C.POINTER(api.AnchorStats)),
                ("strands", C.POINTER(api.StrandResult))]


class List(C.Structure):
    """CpkAnchorList."""
    _fields_ = [("probs", C.POINTER(PassProblem)), ("owner", i64p), ("before", i64p), ("n", C.c_int64), ("cap", C.c_int64)]


def stages():
    """The library with the stage functions' prototypes set."""
    L = api.lib()
    if getattr(L, "_anchor_stages_bound", False):
        return L
    call, lst = C.POINTER(Call), C.POINTER(List)
    L.cpk_anchor_check.argtypes = [call, C.c_int64, C.POINTER(api.AnchorParams), C.POINTER(api.AnchorOptions), C.POINTER(Pass)]
    L.cpk_anchor_layout.argtypes = [call, lst, C.POINTER(C.POINTER(C.c_uint8)), i64p, i64p]
    L.cpk_anchor_pick.argtypes = [call, lst]
    L.cpk_anchor_pick.restype = None
    L.cpk_anchor_gaps.argtypes = [call, lst, i32p, lst]
    L.cpk_anchor_splice.argtypes = [call, lst, i32p, lst, i32p, C.c_double]
    L.cpk_anchor_list_free.argtypes = [lst]
    L.cpk_anchor_list_free.restype = None
    L.cpk_anchor_pass_plan.argtypes = [C.POINTER(Pass), C.POINTER(PassProblem), C.c_int64, C.c_int64, C.c_int64, C.POINTER(Plan)]
    L.cpk_anchor_pass_size.argtypes = [C.POINTER(PassProblem), C.c_int64, C.POINTER(Plan)]
    L.cpk_anchor_pass_size.restype = None
    L._anchor_stages_bound = True
    return L


def default_pass(**fields):
    """The CpkAnchorPass of a call with the default parameters, trim 14, with fields replaced (prm's by their own names)."""
    q = Pass()
    d = api.anchor_params_default()
    q.prm.scores[:] = d.scores[:]
    q.prm.maxSeedOccurrences, q.prm.xDrop, q.prm.hspThreshold, q.prm.maxHsps = d.maxSeedOccurrences, d.xDrop, d.hspThreshold, d.maxHsps
    q.seed, q.seedTransitions, q.variantThreshold, q.trim = d.seed, 0, d.hspThreshold, 14
    for k, v in fields.items():
        setattr(q.prm if hasattr(q.prm, k) else q, k, v)
    return q


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def check_plan(pass_, probs, n, nSym, nForward):
    """cpk_anchor_pass_plan on a list the host stages made: CPECAN_OK, and the key slots are what the kernels rely on.
    Then cpk_anchor_pass_size on a copy with hit counts of its own: the HSP slots."""
    L = stages()
    plan = Plan()
    assert L.cpk_anchor_pass_plan(C.byref(pass_), probs, n, nSym, nForward, C.byref(plan)) == OK, L.cpecan_last_error()
    span = plan.seed.span
    assert span == len(pass_.seed) and plan.seed.weight == pass_.seed.count(b"1")
    ranges, maxRc = [], 0
    for i in range(n):
        p = probs[i]
        assert _pow2(p.capX) and p.capX >= p.lX - span + 1 and _pow2(p.capY) and p.capY >= p.lY - span + 1
        assert (p.hits, p.hsps, p.chained, p.nRuns, p.capped, p.score, p.columns) == (0,) * 7
        if p.flags & SHARE_X:                                  # a twin reads its partner's X keys and owns only its Y's
            assert p.keyXOff == probs[i - 1].keyXOff and not probs[i - 1].flags & SHARE_X
        else:
            ranges.append((p.keyXOff, p.keyXOff + p.capX))
        ranges.append((p.keyYOff, p.keyYOff + p.capY))
        if p.flags & RC_Y:
            assert p.yOff % 2 == 0 and p.yOff >= (nForward + 1) & ~1 and p.yOff + p.lY <= nSym
            maxRc = max(maxRc, p.lY)
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), "key ranges overlap"
    assert not ranges or (ranges[0][0] >= 0 and ranges[-1][1] <= plan.nKeys)
    assert plan.maxRc == maxRc and plan.maxCap == max([1] + [max(probs[i].capX, probs[i].capY) for i in range(n)])
    copy = (PassProblem * max(1, n))(*[probs[i] for i in range(n)])
    for i in range(n):
        copy[i].hits = (37 * i) % 11
    L.cpk_anchor_pass_size(copy, n, C.byref(plan))
    at = 0
    for i in range(n):
        assert _pow2(copy[i].hspCap) and copy[i].hspCap >= max(1, copy[i].hits) and copy[i].hspOff == at
        at += copy[i].hspCap
    assert plan.nSlots == at and plan.maxHits == max([1] + [copy[i].hits for i in range(n)]) and plan.nCounters == n
    return plan


_once, _score = {}, {}


def model_pass(sym, lst, pass_, params, nForward, score):
    """cpk_anchor_pass played by the model on the n problems of lst over the symbol buffer sym (a bytearray: the forward
    bytes, then the area of the reverse complements, which this writes as the device does).  Fills the counts, nRuns,
    hspOff and, with `score`, the chain score; returns the triples.  The run blocks lie in reverse list order with a
    poisoned triple between them: the host may rely on hspOff and nRuns alone."""
    n = lst.n
    check_plan(pass_, lst.probs, n, len(sym), nForward)
    found = []
    for i in range(n):
        p = lst.probs[i]
        x = bytes(sym[p.xOff:p.xOff + p.lX])
        if p.flags & RC_Y:
            sym[p.yOff:p.yOff + p.lY] = sm.rc(bytes(sym[p.yFwd:p.yFwd + p.lY]))
        y = bytes(sym[p.yOff:p.yOff + p.lY])
        key = (x, y, p.softMask, pass_.trim)
        if key not in _once:
            _once[key] = am.anchors_once(x, y, pass_.trim, bool(p.softMask), params)
        runs, counts = _once[key]
        p.hits, p.hsps, p.chained, p.capped, p.nRuns = counts["hits"], counts["hsps"], counts["chained"], counts["capped"], len(runs)
        p.columns = sum(r[2] for r in runs)
        if score:
            if (x, y) not in _score:
                _score[(x, y)] = sm.strand_score(x, y, params)
            p.score = _score[(x, y)]
        found.append(runs)
    triples = []
    for i in reversed(range(n)):
        triples += [-7, -7, -7]
        lst.probs[i].hspOff = len(triples) // 3
        lst.probs[i].hspCap = max(1, len(found[i]))
        triples += [v for r in found[i] for v in r]
    return (C.c_int32 * max(1, len(triples)))(*triples)


def run_call(problems, strand="both", trim=14, expansion=20, anchorMatrixBiggerThanThis=500 * 500,
             repeatMaskMatrixBiggerThanThis=500 * 500, once=False, softMaskTop=1):
    """find_runs of cpecan_anchor.c with the default parameters and model_pass for the device: ([int64 (x, y, length,
    expansion) rows per problem], [statistics dict], [strand dict], facts), facts being what the stages did on the way:
    "scored" -- the caller's problems in the top-level pass, "searched" -- those that went on to the gaps, "gaps" -- the
    owner of every gap problem."""
    L = stages()
    arr, n, keep = api._anchor_problems(problems)
    runs, counts = (i64p * max(1, n))(), (C.c_int64 * max(1, n))()
    stats, strands = (api.AnchorStats * max(1, n))(), (api.StrandResult * max(1, n))()
    call = Call(b"run_call", arr, n, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, 0,
                api._strand_mode(strand), int(once), softMaskTop, runs, counts, stats, strands)
    pass_, params = Pass(), am.default_params()
    assert L.cpk_anchor_check(C.byref(call), trim, None, None, C.byref(pass_)) == OK, L.cpecan_last_error()
    assert (pass_.seed.decode(), pass_.prm.hspThreshold, pass_.variantThreshold, pass_.trim, pass_.seedTransitions) == \
        (params["seed"], params["hspThreshold"], params["hspThreshold"], trim, 0)
    top, sub, raw = List(), List(), C.POINTER(C.c_uint8)()
    nBytes, nExtra = C.c_int64(), C.c_int64()
    facts = dict(scored=[], searched=[], gaps=[])
    try:
        assert L.cpk_anchor_layout(C.byref(call), C.byref(top), C.byref(raw), C.byref(nBytes), C.byref(nExtra)) == OK
        if top.n:
            nForward = nBytes.value
            nSym = ((nForward + 1) & ~1) + nExtra.value if nExtra.value else nForward       # cpk_anchor_open's
            sym = bytearray(C.string_at(raw, nForward)) + bytearray(nSym - nForward)
            facts["scored"] = sorted(set(top.owner[k] for k in range(top.n)))
            topRuns = model_pass(sym, top, pass_, params, nForward, score=not once)
            L.cpk_anchor_pick(C.byref(call), C.byref(top))
            facts["searched"] = [top.owner[k] for k in range(top.n)]
            assert L.cpk_anchor_gaps(C.byref(call), C.byref(top), topRuns, C.byref(sub)) == OK
            facts["gaps"] = [top.owner[sub.owner[g]] for g in range(sub.n)]
            subRuns = model_pass(sym, sub, pass_, params, nForward, score=False)
            assert L.cpk_anchor_splice(C.byref(call), C.byref(top), topRuns, C.byref(sub), subRuns, 0.0) == OK
        out = [[tuple(runs[i][4 * k:4 * k + 4]) for k in range(counts[i])] for i in range(n)]
        return out, [stats[i].as_dict() for i in range(n)], [strands[i].as_dict() for i in range(n)], facts
    finally:
        for i in range(n):
            L.cpecan_free(C.cast(runs[i], C.c_void_p))
        L.cpecan_free(C.cast(raw, C.c_void_p))
        L.cpk_anchor_list_free(C.byref(top))
        L.cpk_anchor_list_free(C.byref(sub))
