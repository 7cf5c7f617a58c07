"""ctypes mirror of include/cpecan_local.h: the K best mutually disjoint chains of a pair over one or both orientations
(DESIGN.md section 7, step 7), the cigars that stand for them, and the realignment of those cigars -- the reference's
`lastz | cPecanRealign` pipeline in one process.

    chains, stats = find_local_chains([(sX, sY), ...], strand="both", options=local_options(maxChains=4))
    cigars = align_local({"t": sX}, {"q": sY}, strand="both", options=local_options(maxChains=4))
"""
import ctypes as C

import numpy as np

from . import api
from . import realign

# Every symbol include/cpecan_local.h declares (checked by tests/test_local_cpu.py).
EXPORTS = ["cpecan_local_options_default", "cpecan_find_local_chains_many", "cpecan_find_local_chains_many_gapped",
           "cpecan_cigar_from_local_chain"]

MAX_CHAINS = 16


class LocalOptions(C.Structure):
    """cpecan_local_options."""
    _fields_ = [("maxChains", C.c_int32), ("minChainScore", C.c_int32), ("reserved", C.c_int32 * 6)]


class LocalChain(C.Structure):
    """cpecan_local_chain."""
    _fields_ = [("strand", C.c_int32), ("score", C.c_int32), ("nHsps", C.c_int64), ("x0", C.c_int64), ("x1", C.c_int64),
                ("y0", C.c_int64), ("y1", C.c_int64), ("runOff", C.c_int64), ("nRuns", C.c_int64)]


class LocalStats(C.Structure):
    """cpecan_local_stats."""
    _fields_ = [("hitsPlus", C.c_int64), ("hitsMinus", C.c_int64), ("hspsPlus", C.c_int64), ("hspsMinus", C.c_int64),
                ("capped", C.c_int32), ("rounds", C.c_int32), ("kernelMs", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_bound = False


def _lib():
    global _bound
    L = api.lib()
    realign._lib()
    if not _bound:
        i64p = C.POINTER(C.c_int64)
        L.cpecan_local_options_default.argtypes = [C.POINTER(LocalOptions)]
        L.cpecan_find_local_chains_many.argtypes = [
            C.POINTER(api.AnchorProblem), C.c_int64, C.c_int64, C.c_int64, C.POINTER(api.AnchorParams),
            C.POINTER(api.AnchorOptions), C.POINTER(LocalOptions), C.c_int, C.c_int, C.POINTER(C.POINTER(LocalChain)), i64p,
            C.POINTER(i64p), i64p, C.POINTER(LocalStats)]
        L.cpecan_find_local_chains_many_gapped.argtypes = L.cpecan_find_local_chains_many.argtypes
        L.cpecan_cigar_from_local_chain.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(LocalChain), i64p,
                                                    C.POINTER(realign._Cigar)]
        _bound = True
    return L


def local_options(**overrides):
    """cpecan_local_options_default (maxChains 1, minChainScore 0 = hspThreshold); keyword overrides name its fields."""
    o = LocalOptions()
    api._check(_lib().cpecan_local_options_default(C.byref(o)), "cpecan_local_options_default")
    for k, v in overrides.items():
        if k == "reserved" or not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, int(v))
    return o


def find_local_chains(problems, trim=api.CONSTRAINT_DIAGONAL_TRIM, expansion=20, params=None, anchor_options=None, options=None,
                      device=0, strand="both", gapped=False):
    """cpecan_find_local_chains_many on (sX, sY, ...) tuples: ([chains per problem], [statistics dict per problem]).  A chain
    is a dict: strand "plus" / "minus", score, nHsps, the rectangle x0, x1, y0, y1 and runs, int64[n, 4] of (x, y, length,
    expansion); rectangle and runs of a minus chain are in the coordinates of (sX, reverse_complement(sY)).
    gapped: cpecan_find_local_chains_many_gapped instead, which extends every chain into its gaps and outwards (DESIGN.md
    section 7, step 7b) as anchor_options' gappedExtension, yDrop and gappedMaxDiagonals say; without anchor_options that is
    gappedExtension = 1 at the defaults."""
    L = _lib()
    entry, name = L.cpecan_find_local_chains_many, "cpecan_find_local_chains_many"
    if gapped:
        entry, name = L.cpecan_find_local_chains_many_gapped, "cpecan_find_local_chains_many_gapped"
        if anchor_options is None:
            anchor_options = api.anchor_options(gappedExtension=1)
    arr, n, keep = api._anchor_problems(problems)
    i64p = C.POINTER(C.c_int64)
    chains, nChains = (C.POINTER(LocalChain) * max(1, n))(), (C.c_int64 * max(1, n))()
    runs, nRuns = (i64p * max(1, n))(), (C.c_int64 * max(1, n))()
    stats = (LocalStats * max(1, n))()
    try:
        api._check(entry(
            arr, n, trim, expansion, C.byref(params) if params is not None else None,
            C.byref(anchor_options) if anchor_options is not None else None, C.byref(options) if options is not None else None,
            device, api._strand_mode(strand), chains, nChains, runs, nRuns, stats), name)
        out = []
        for i in range(n):
            all_runs = np.zeros((0, 4), dtype=np.int64)
            if nRuns[i]:
                all_runs = np.ctypeslib.as_array(runs[i], shape=(nRuns[i] * 4,)).copy().reshape(nRuns[i], 4)
            mine = []
            for j in range(nChains[i]):
                c = chains[i][j]
                mine.append(dict(strand=api.STRAND_NAMES[c.strand], score=c.score, nHsps=c.nHsps, x0=c.x0, x1=c.x1, y0=c.y0,
                                 y1=c.y1, runs=all_runs[c.runOff:c.runOff + c.nRuns].copy()))
            out.append(mine)
        return out, [stats[i].as_dict() for i in range(n)]
    finally:
        for i in range(n):
            L.cpecan_free(C.cast(chains[i], C.c_void_p))
            L.cpecan_free(C.cast(runs[i], C.c_void_p))


def cigar_of_chain(contig1, contig2, lY, chain):
    """cpecan_cigar_from_local_chain on a chain of find_local_chains: a realign.Cigar from the start of the chain's first run
    to the end of its last; a minus chain reads "<start2> <end2> -" with start2 > end2 for contig2."""
    r = np.ascontiguousarray(np.asarray(chain["runs"], dtype=np.int64).reshape(-1, 4))
    rec = LocalChain(api._strand_mode(chain["strand"]), int(chain["score"]), int(chain.get("nHsps", len(r))), int(chain["x0"]),
                     int(chain["x1"]), int(chain["y0"]), int(chain["y1"]), 0, len(r))
    buf = r if len(r) else np.zeros((1, 4), dtype=np.int64)
    c = realign._Cigar()
    api._check(_lib().cpecan_cigar_from_local_chain(contig1.encode(), contig2.encode(), int(lY), C.byref(rec),
                                                    buf.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(c)),
               "cpecan_cigar_from_local_chain")
    try:
        return realign.Cigar._from_c(c)
    finally:
        _lib().cpecan_cigar_clear(C.byref(c))


def local_cigars(targets, queries, trim=0, expansion=20, params=None, anchor_options=None, options=None, device=0,
                 strand="both", gapped=False):
    """The cigars of every chain of every (target, query) pair from ONE find_local_chains call: queries outer, targets inner,
    the chains of a pair in round order; a chain without runs has no cigar.  targets, queries: {name: sequence}.  gapped: as
    in find_local_chains."""
    pairs = [(t, q) for q in queries for t in targets]
    chains, _ = find_local_chains([(targets[t], queries[q]) for t, q in pairs], trim, expansion, params, anchor_options, options,
                                  device, strand, gapped)
    return [cigar_of_chain(t, q, len(queries[q]), c) for (t, q), mine in zip(pairs, chains) for c in mine if len(c["runs"])]


def align_local(targets, queries, sM=None, realign_options=None, trim=0, expansion=20, params=None, anchor_options=None,
                options=None, device=0, strand="both", gapped=False):
    """chains -> cigars -> Realigner.realign: one anchor call and one realign call; the realigned realign.Cigar list in the
    order of local_cigars.  realign_options: a realign.RealignOptions (default: cPecanRealign's).  gapped: as in
    find_local_chains."""
    cigars = local_cigars(targets, queries, trim, expansion, params, anchor_options, options, device, strand, gapped)
    with realign.Realigner(sM, realign_options, device) as r:
        for name, seq in list(targets.items()) + list(queries.items()):
            r.add_sequence(name, seq)
        return r.realign(cigars) if cigars else []
