"""Local chains as DESIGN.md section 7 step 7 (include/cpecan_local.h) defines them, in plain Python on top of
tests/anchor_model.py and its relatives: the model the GPU result is compared with, integer for integer.  Written from the
definition -- pools, intervals, rounds -- with loops over sets; nothing about lanes, binary searches or launches.

    pool(sX, sY, params, seedTransitions, transitionHspThreshold)   -> (HSPs sorted by place, after the cap; counts dict)
    local_chains(sX, sY, strand, maxChains, minChainScore, trim, expansion, params, seedTransitions, transitionHspThreshold)
        -> (chains [dict], statistics dict)
"""
import numpy as np

import anchor_model as am
import anchor_model_threshold as amth
import strand_model as sm


def pool(sX, sY, params, seedTransitions=0, transitionHspThreshold=0):
    """Steps 1-3 on the whole pair, soft mask on, as the top-level pass runs them (anchor_model_threshold._hsps): the HSPs
    (x, y, len, score) sorted by (x, y, len) after duplicates and the maxHsps cap, and the counts."""
    if len(sX) == 0 or len(sY) == 0:
        return [], dict(hits=0, hsps=0, capped=0)
    hsps, hits, found = amth._hsps(sX, sY, True, params, seedTransitions, transitionHspThreshold)
    return hsps, dict(hits=hits, hsps=found, capped=int(found > params["maxHsps"]))


def intervals(h, minus, lY):
    """The X interval and the forward-Y interval an HSP occupies."""
    x, y, length = h[0], h[1], h[2]
    return (x, x + length), ((lY - y - length, lY - y) if minus else (y, y + length))


def _meet(a, b):
    return a[0] < b[1] and b[0] < a[1]


def local_chains(sX, sY, strand="both", maxChains=1, minChainScore=0, trim=14, expansion=20, params=None,
                 seedTransitions=0, transitionHspThreshold=0):
    """Points 1-4 of the definition.  A chain: strand, score, nHsps, x0, x1, y0, y1, runs int64[n, 4], and `hsps`, the
    chained HSPs themselves, which only the model has.  Statistics: hits / hsps per orientation, capped (bit 0 plus, bit 1
    minus), rounds."""
    params = params or am.default_params()
    S = minChainScore or params["hspThreshold"]
    lY = len(sY)
    modes = {"plus": ["plus"], "minus": ["minus"], "both": ["plus", "minus"]}[strand]
    st = dict(hitsPlus=0, hitsMinus=0, hspsPlus=0, hspsMinus=0, capped=0, rounds=0)
    pools, live = {}, {}
    for o in modes:
        hsps, c = pool(sX, sm.rc(sY) if o == "minus" else sY, params, seedTransitions, transitionHspThreshold)
        pools[o], live[o] = hsps, [True] * len(hsps)
        st["hits" + o.capitalize()], st["hsps" + o.capitalize()] = c["hits"], c["hsps"]
        st["capped"] |= c["capped"] << (o == "minus")
    chains = []
    for _ in range(maxChains):
        best = None
        for o in modes:                                     # plus first: a tie stays with it
            idx = [i for i, alive in enumerate(live[o]) if alive]
            if not idx:
                continue
            sub = [pools[o][i] for i in idx]                # pool order is kept, so are the tie rules
            picked = [idx[k] for k in am.chain(sub)]
            score = sum(pools[o][i][3] for i in picked)
            if best is None or score > best[0]:
                best = (score, o, picked)
        if best is None:
            break
        st["rounds"] += 1
        score, o, picked = best
        if score < S:
            break
        hs = [pools[o][i] for i in picked]
        runs = [(h[0] + trim, h[1] + trim, h[2] - 2 * trim, expansion) for h in hs if h[2] - 2 * trim > 0]
        chains.append(dict(strand=o, score=int(score), nHsps=len(hs), x0=hs[0][0], x1=hs[-1][0] + hs[-1][2], y0=hs[0][1],
                           y1=hs[-1][1] + hs[-1][2], runs=np.array(runs, dtype=np.int64).reshape(-1, 4), hsps=hs))
        taken = [intervals(h, o == "minus", lY) for h in hs]
        for q in modes:
            for i, h in enumerate(pools[q]):
                if live[q][i]:
                    ix, iy = intervals(h, q == "minus", lY)
                    if any(_meet(ix, tx) or _meet(iy, ty) for tx, ty in taken):
                        live[q][i] = False
    return chains, st


def same(got, want):
    """A chain of cpecan_amd.local.find_local_chains against one of the model: every integer."""
    keys = ("strand", "score", "nHsps", "x0", "x1", "y0", "y1")
    return all(got[k] == want[k] for k in keys) and np.array_equal(got["runs"], want["runs"])
