// cpk_local.inl -- local chains (include/cpecan_local.h: cpecan_find_local_chains_many).
// The K best mutually disjoint chains of a pair over one or both orientations, peeled round by round from the HSP pools
// that steps 1-3 of the anchor finder (cpk_anchor.inl) leave.  One workgroup of 256 per CALLER problem: it owns the pools
// of the problem's orientation twins, which lie next to each other in the pass list, because the winner of a round and the
// kill rule cross orientations.  Everything is integer work on sorted lists; no atomics beyond pool preparation's.
//
// Liveness is the score word of a pool's HSP: a killed HSP gets CPK_LOCAL_DEAD there, which no sum of column scores
// reaches.  best / pred are rewritten every round; after the walk back, best[0 .. m) of the winning orientation holds the
// chain's pool indices from its last HSP to its first, which the kill pass reads.

#define CPK_LOCAL_DEAD ((int)0x80000000)

// Chain HSP k (in chain order) of the round's winner, as the interval it occupies on X (side 0) or on forward Y (side 1).
// Interval k is the k-th smallest on that side: on X the intervals ascend along the chain; on forward Y they ascend along a
// plus chain and descend along a minus chain, whose k-th smallest is therefore its k-th from the end.
__device__ __forceinline__ int2 local_chain_interval(const int4 *hsp, const int32_t *walk, int m, int k, int side, bool minus, int lY) {
    const bool flip = side == 1 && minus;
    const int4 h = hsp[walk[flip ? k : m - 1 - k]];  // walk[] runs from the chain's last HSP to its first
    if (side == 0) return make_int2(h.x, h.x + h.z);
    return minus ? make_int2(lY - h.y - h.z, lY - h.y) : make_int2(h.y, h.y + h.z);
}

// Does [a, b) meet one of the chain's m disjoint intervals on `side`?  The first interval that ends behind a decides.
__device__ __forceinline__ bool local_meets(const int4 *hsp, const int32_t *walk, int m, int side, bool minus, int lY, int a, int b) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (local_chain_interval(hsp, walk, m, mid, side, minus, lY).y <= a) lo = mid + 1;
        else hi = mid;
    }
    return lo < m && local_chain_interval(hsp, walk, m, lo, side, minus, lY).x < b;
}

// probs: the pass list (twins included); lprobs: one record per caller problem; chainsAll: maxChains records per caller
// problem; the runs of a problem go to the run slots of its twins, 3 * hspOff of the first onwards, hspCap of both together:
// every chained HSP leaves its pool, so the pools bound them.
__global__ void __launch_bounds__(256) cpk_local_peel(CpkAnchorProblem *probs, CpkLocalProblem *lprobs, int4 *hspsAll,
                                                      const int32_t *nHsp, int32_t *bestAll, int32_t *predAll, int32_t *runsAll,
                                                      CpkLocalChain *chainsAll, int maxHsps, int trim, int maxChains,
                                                      int minChainScore) {
    __shared__ long long red[16];
    __shared__ int shLen, shMade;
    const int tid = threadIdx.x, nT = blockDim.x;
    const CpkLocalProblem lp = lprobs[blockIdx.x];
    const int twins = lp.twins;
    CpkLocalChain *chains = chainsAll + (int64_t)blockIdx.x * maxChains;
    // the twins' lists, each in variables of its own: indexed by constants after unrolling, so nothing spills to scratch
    int4 *hsp[2] = {nullptr, nullptr};
    int32_t *best[2] = {nullptr, nullptr}, *pred[2] = {nullptr, nullptr};
    int n[2] = {0, 0}, lY = 0;
    bool minusOf[2] = {false, false};
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (t >= twins) break;
        const int64_t q = lp.first + t;
        const CpkAnchorProblem pr = probs[q];
        hsp[t] = hspsAll + pr.hspOff;
        best[t] = bestAll + pr.hspOff;
        pred[t] = predAll + pr.hspOff;
        minusOf[t] = (pr.flags & CPK_ANCHOR_RC_Y) != 0;
        lY = pr.lY;
        int nUnique, capped;
        n[t] = anchor_pool_prepare(hsp[t], pr.hspCap, nHsp[q], maxHsps, pred[t], &nUnique, &capped);
        if (tid == 0) {
            probs[q].hsps = nUnique;
            probs[q].capped = capped;
        }
    }
    int32_t *runs = runsAll + 3 * probs[lp.first].hspOff;
    int nChains = 0, nRuns = 0, rounds = 0;
    for (int r = 0; r < maxChains; r++) {
        long long endKey[2] = {CPK_ANCHOR_NO_KEY, CPK_ANCHOR_NO_KEY};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t >= twins) break;
            const int4 *h = hsp[t];
            int32_t *b = best[t], *pd = pred[t];
            const int nt = n[t];
            // step 4 over the live HSPs: a dead one is neither a predecessor nor an end
            for (int i = 0; i < nt; i++) {
                const int4 me = h[i];
                if (me.w == CPK_LOCAL_DEAD) continue;  // the same in every thread
                long long key = CPK_ANCHOR_NO_KEY;
                for (int j = tid; j < i; j += nT) {
                    const int4 o = h[j];
                    if (o.w != CPK_LOCAL_DEAD && o.x + o.z <= me.x && o.y + o.z <= me.y) {
                        const long long k = (long long)b[j] * 4294967296LL + (unsigned)~j;  // largest best, then smallest j
                        key = k > key ? k : key;
                    }
                }
                key = anchor_block_max(key, red);
                if (tid == 0) {
                    b[i] = me.w + (key == CPK_ANCHOR_NO_KEY ? 0 : (int)(key >> 32));
                    pd[i] = key == CPK_ANCHOR_NO_KEY ? -1 : (int)~(unsigned)key;
                }
                __syncthreads();
            }
            long long k = CPK_ANCHOR_NO_KEY;
            for (int i = tid; i < nt; i += nT)
                if (h[i].w != CPK_LOCAL_DEAD) {
                    const long long v = (long long)b[i] * 4294967296LL + (unsigned)~i;
                    k = v > k ? v : k;
                }
            endKey[t] = anchor_block_max(k, red);
        }
        // the round's chain: the larger score, a tie to the orientation that comes first (plus, with both); wave-uniform
        const bool second = endKey[1] != CPK_ANCHOR_NO_KEY && (endKey[0] == CPK_ANCHOR_NO_KEY || (endKey[1] >> 32) > (endKey[0] >> 32));
        const long long winKey = second ? endKey[1] : endKey[0];
        if (winKey == CPK_ANCHOR_NO_KEY) break;  // nothing live
        rounds++;
        const int score = (int)(winKey >> 32);
        if (score < minChainScore) break;
        int4 *hspW = second ? hsp[1] : hsp[0];
        int32_t *walk = second ? best[1] : best[0];  // free after the recurrence: it holds the walk
        const int32_t *predW = second ? pred[1] : pred[0];
        const bool minusW = second ? minusOf[1] : minusOf[0];
        if (tid == 0) {
            // step 5 on the chain: walk back from the end, then the trimmed runs in increasing order
            int m = 0;
            for (int i = (int)~(unsigned)winKey; i >= 0; i = predW[i]) walk[m++] = i;
            const int4 first = hspW[walk[m - 1]], last = hspW[walk[0]];
            CpkLocalChain c;
            c.strand = minusW ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
            c.score = score;
            c.nHsps = m;
            c.runOff = nRuns;
            c.x0 = first.x;
            c.y0 = first.y;
            c.x1 = last.x + last.z;
            c.y1 = last.y + last.z;
            int made = 0;
            for (int k = m - 1; k >= 0; k--) {
                const int4 h = hspW[walk[k]];
                const int len = h.z - 2 * trim;
                if (len > 0) {
                    int32_t *q = runs + 3 * (nRuns + made);
                    q[0] = h.x + trim;
                    q[1] = h.y + trim;
                    q[2] = len;
                    made++;
                }
            }
            c.nRuns = made;
            chains[nChains] = c;
            shLen = m;
            shMade = made;
        }
        __syncthreads();
        const int m = shLen;
        nChains++;
        nRuns += shMade;
        // the kill pass: two binary searches per live HSP in the chain just written; it kills the chain's own HSPs too
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t >= twins) break;
            int4 *h = hsp[t];
            for (int i = tid; i < n[t]; i += nT) {
                const int4 me = h[i];
                if (me.w == CPK_LOCAL_DEAD) continue;
                const int ya = minusOf[t] ? lY - me.y - me.z : me.y;
                if (local_meets(hspW, walk, m, 0, minusW, lY, me.x, me.x + me.z) ||
                    local_meets(hspW, walk, m, 1, minusW, lY, ya, ya + me.z))
                    h[i].w = CPK_LOCAL_DEAD;
            }
        }
        __syncthreads();  // shLen and shMade may be written again
    }
    if (tid == 0) {
        lprobs[blockIdx.x].nChains = nChains;
        lprobs[blockIdx.x].nRuns = nRuns;
        lprobs[blockIdx.x].rounds = rounds;
    }
}

// ---- step 7b: gapped extension of the chains (include/cpecan_local.h: cpecan_find_local_chains_many_gapped) ----
// A pass that extends chains runs the peel with trim 0, so the problem's run slots hold every chain's HSP triples in chain
// order, chain r's at runOff .. runOff + nHsps - 1.  The host lays out the gaps: gapBase[k * maxChains + r] is the first gap
// of chain r of caller problem k (nHsps + 1 of them; the gaps of a problem follow each other, chain by chain), and gap q has
// the block slots gapRow[2 * q] onwards, of which those from gapRow[2 * q + 1] on are its left extension's -- the layout of
// cpk_anchor_gapped, a triple per scratch row of the UNFENCED gap, which the fences only shrink.  The rows of a round lie
// together, so a launch of round r takes the rows [lo, hi) of it and `trace` holds hi - lo rows.

// One occupied element against the four fences of the gap from (aX, aY) to (bX, bY), in the orientation of the gap's chain.
struct LocalFences {
    int xR, yR, xL, yL;  // smallest occupied start in [a, b); largest occupied end in (a, b]
};
__device__ __forceinline__ void local_fence(LocalFences &f, int aX, int aY, int bX, int bY, int xs, int xe, int ys, int ye) {
    if (xs >= aX && xs < bX) f.xR = min(f.xR, xs);
    if (ys >= aY && ys < bY) f.yR = min(f.yR, ys);
    if (xe > aX && xe <= bX) f.xL = max(f.xL, xe);
    if (ye > aY && ye <= bY) f.yL = max(f.yL, ye);
}

// the chain (0 .. nChains - 1) that HSP t of the problem's list belongs to; nChains <= 16
__device__ __forceinline__ int local_chain_of(const CpkLocalChain *chains, int nChains, int t) {
    int j = 0;
    while (j + 1 < nChains && t >= chains[j + 1].runOff) j++;
    return j;
}

// One wave per (caller problem, gap of chain r).  The lanes scan the problem's occupied elements -- the HSPs of every other
// chain, and the blocks the chains before r kept -- for the four fences, a wave minimum / maximum makes them uniform, and the
// walks of step 5b run on the fenced sides.  Blocks and counts are this wave's alone; what it reads of other chains was
// written by the peel or by the launches of earlier rounds on the same stream.
__global__ void __launch_bounds__(64) cpk_local_gapped(const CpkAnchorProblem *probs, const CpkLocalProblem *lprobs,
                                                       const CpkLocalChain *chainsAll, const uint8_t *sym, CpkAnchorParams prm,
                                                       const int32_t *hspAll, const int64_t *gapBase, const int64_t *gapRow,
                                                       int maxChains, int r, int64_t lo, int64_t hi, uint8_t *trace,
                                                       int32_t *blocks, int2 *counts) {
    __shared__ int sc[25];
    if (threadIdx.x < 25) sc[threadIdx.x] = prm.scores[threadIdx.x];
    __syncthreads();
    const int k = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    const CpkLocalProblem lp = lprobs[k];
    if (r >= lp.nChains) return;
    const CpkLocalChain *chains = chainsAll + (int64_t)k * maxChains;
    const CpkLocalChain me = chains[r];
    const int c = me.nHsps;
    if (g > c) return;
    const bool minus = me.strand == CPECAN_STRAND_MINUS;
    CpkAnchorProblem pr = probs[lp.first];
    if (lp.twins == 2 && minus != ((pr.flags & CPK_ANCHOR_RC_Y) != 0)) pr = probs[lp.first + 1];
    const int32_t *hsp = hspAll + 3 * probs[lp.first].hspOff, *chain = hsp + 3 * me.runOff;
    const int lY = pr.lY;
    const int aX = g ? chain[3 * (g - 1)] + chain[3 * (g - 1) + 2] : 0, aY = g ? chain[3 * (g - 1) + 1] + chain[3 * (g - 1) + 2] : 0;
    const int bX = g < c ? chain[3 * g] : pr.lX, bY = g < c ? chain[3 * g + 1] : lY;
    const int m = bX - aX, n = bY - aY;
    const bool right = g >= 1, left = g < c;
    const int maxDiags = CPK_ANCHOR_DIAGS(pr.flags);
    const int rows = min(m + n, maxDiags), rowsR = right ? rows : 0, rowsL = left ? rows : 0;
    const int64_t q = gapBase[(int64_t)k * maxChains + r] + g;
    const int64_t row0 = gapRow[2 * q], mid = gapRow[2 * q + 1];
    // A launch takes the gaps that lie inside its slice.  `mid - row0 != rowsR` is never expected to hold: the host laid the
    // rows out from the same chain records; it only keeps a wave inside its slots if the two ever disagreed, and the gap then
    // stays unextended, which the comparison with the model shows.
    if (rows <= 0 || mid - row0 != rowsR || row0 < lo || row0 + rowsR + rowsL > hi) return;

    LocalFences f = {bX, bY, aX, aY};
    const CpkLocalChain lastChain = chains[lp.nChains - 1];
    const int nHspAll = lastChain.runOff + lastChain.nHsps;
    for (int t = lane; t < nHspAll; t += 64) {  // the chained HSPs of every other chain
        const int j = local_chain_of(chains, lp.nChains, t);
        if (j == r) continue;
        const int x = hsp[3 * t], y = hsp[3 * t + 1], len = hsp[3 * t + 2];
        const bool same = (chains[j].strand == CPECAN_STRAND_MINUS) == minus;
        const int ys = same ? y : lY - y - len;
        local_fence(f, aX, aY, bX, bY, x, x + len, ys, ys + len);
    }
    const int64_t gap0 = gapBase[(int64_t)k * maxChains], gapsBefore = gapBase[(int64_t)k * maxChains + r] - gap0;
    for (int64_t t = lane; t < gapsBefore; t += 64) {  // the blocks kept by the chains before r, gap by gap
        int j = 0;
        while (j + 1 < r && gap0 + t >= gapBase[(int64_t)k * maxChains + j + 1]) j++;
        const bool same = (chains[j].strand == CPECAN_STRAND_MINUS) == minus;
        const int2 cnt = counts[gap0 + t];
        const int32_t *b = blocks + 3 * gapRow[2 * (gap0 + t) + 1];
        for (int u = -cnt.x; u < cnt.y; u++) {
            const int x = b[3 * u], y = b[3 * u + 1], len = b[3 * u + 2];
            const int ys = same ? y : lY - y - len;
            local_fence(f, aX, aY, bX, bY, x, x + len, ys, ys + len);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        f.xR = min(f.xR, __shfl_xor(f.xR, o));
        f.yR = min(f.yR, __shfl_xor(f.yR, o));
        f.xL = max(f.xL, __shfl_xor(f.xL, o));
        f.yL = max(f.yL, __shfl_xor(f.yL, o));
    }
    const int mR = f.xR - aX, nR = f.yR - aY, mL = bX - f.xL, nL = bY - f.yL;  // each within 0 .. m or 0 .. n

    uint8_t *traceR = trace + (size_t)(row0 - lo) * 64, *traceL = traceR + (size_t)rowsR * 64;
    int32_t *blocksR = blocks + 3 * row0, *blocksL = blocks + 3 * mid;
    AnchorReach R = {0, 0, 0}, L = {0, 0, 0};
    if (right) R = anchor_gapped_walk(sym, sc, pr.xOff + aX, pr.yOff + aY, 1, mR, nR, pr.yDrop, min(mR + nR, maxDiags), traceR);
    if (left) L = anchor_gapped_walk(sym, sc, pr.xOff + bX - 1, pr.yOff + bY - 1, -1, mL, nL, pr.yDrop, min(mL + nL, maxDiags), traceL);
    if (R.i + L.i > m || R.j + L.j > n) {  // 5b's test on the whole gap: the smaller best goes, the left one on a tie
        if (R.best < L.best) R.best = 0;
        else L.best = 0;
    }
    __threadfence();  // the bytes other lanes stored are read below
    const int kR = R.best > 0 ? anchor_gapped_blocks(traceR, R, false, aX, aY, blocksR, rows) : 0;
    const int kL = L.best > 0 ? anchor_gapped_blocks(traceL, L, true, bX, bY, blocksL, rows) : 0;
    if (lane == 0) counts[q] = make_int2(kR, kL);
}

// Assembly, merging and step 5 of one chain, as cpk_anchor_assemble does them for a problem: per gap the right blocks, the
// left blocks, then the next HSP.  out == nullptr counts only.  rect: the start of the first merged block and the end of the
// last, untrimmed.
__device__ __forceinline__ int local_chain_runs(const int32_t *chain, int c, int64_t gapFirst, const int64_t *gapRow,
                                                const int32_t *blocks, const int2 *counts, int trim, int32_t *out, int4 *rect) {
    int nRuns = 0, x = 0, y = 0, len = 0;
    bool first = true;
    auto flush = [&]() {
        if (len > 0 && first) rect->x = x, rect->y = y, first = false;
        if (len > 0) rect->z = x + len, rect->w = y + len;
        if (len - 2 * trim > 0) {
            if (out) {
                out[3 * nRuns] = x + trim;
                out[3 * nRuns + 1] = y + trim;
                out[3 * nRuns + 2] = len - 2 * trim;
            }
            nRuns++;
        }
    };
    auto put = [&](int bx, int by, int blen) {
        if (len > 0 && x + len == bx && y + len == by) {
            len += blen;
        } else {
            flush();
            x = bx, y = by, len = blen;
        }
    };
    for (int g = 0; g <= c; g++) {
        const int2 cnt = counts[gapFirst + g];
        const int32_t *b = blocks + 3 * gapRow[2 * (gapFirst + g) + 1];
        for (int t = -cnt.x; t < cnt.y; t++) put(b[3 * t], b[3 * t + 1], b[3 * t + 2]);  // the right ones end where the left ones start
        if (g < c) put(chain[3 * g], chain[3 * g + 1], chain[3 * g + 2]);
    }
    flush();
    return nRuns;
}

// One wave per caller problem, lane j for chain j: count the chain's runs, a prefix sum over the lanes, write them.  The
// runs of problem k go to runBase[k] of runsOut, chain by chain; the chain records get their rectangle, runOff and nRuns, the
// problem its run count.
__global__ void __launch_bounds__(64) cpk_local_gapped_assemble(const CpkAnchorProblem *probs, CpkLocalProblem *lprobs,
                                                                CpkLocalChain *chainsAll, const int32_t *hspAll,
                                                                const int64_t *gapBase, const int64_t *gapRow, const int64_t *runBase,
                                                                const int32_t *blocks, const int2 *counts, int32_t *runsOut,
                                                                int maxChains, int trim) {
    const int k = blockIdx.x, j = threadIdx.x;
    const CpkLocalProblem lp = lprobs[k];
    const bool mine = j < lp.nChains;
    CpkLocalChain *rec = chainsAll + (int64_t)k * maxChains + (mine ? j : 0);
    const CpkLocalChain me = *rec;
    const int32_t *chain = hspAll + 3 * (probs[lp.first].hspOff + me.runOff);
    const int64_t gapFirst = gapBase[(int64_t)k * maxChains + (mine ? j : 0)];
    int4 rect = make_int4(0, 0, 0, 0);
    const int made = mine ? local_chain_runs(chain, me.nHsps, gapFirst, gapRow, blocks, counts, trim, nullptr, &rect) : 0;
    int before = 0, total = 0;
    for (int o = 0; o < CPK_LOCAL_MAX_CHAINS; o++) {
        const int v = __shfl(made, o);
        before += o < j ? v : 0;
        total += v;
    }
    if (mine) {
        local_chain_runs(chain, me.nHsps, gapFirst, gapRow, blocks, counts, trim, runsOut + 3 * (runBase[k] + before), &rect);
        rec->x0 = rect.x;
        rec->y0 = rect.y;
        rec->x1 = rect.z;
        rec->y1 = rect.w;
        rec->runOff = before;
        rec->nRuns = made;
    }
    if (j == 0) lprobs[k].nRuns = total;
}
