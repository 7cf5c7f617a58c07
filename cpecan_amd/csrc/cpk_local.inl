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
