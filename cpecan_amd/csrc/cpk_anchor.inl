// cpk_anchor.inl -- the anchor finder (include/cpecan_hip.h: cpecan_find_anchor_runs_many).
// Integer work over a batch of sequence pairs: spaced-seed words, a k-mer join on sorted (word, position) keys, ungapped
// x-drop extension with one hit per lane, and per-problem sort / duplicate removal / chaining with one workgroup per
// problem.  Every result is defined on sets and sorted orders: the atomics below only hand out slots of lists that are
// sorted before anything reads their order.  With cpecan_anchor_options.gappedExtension the chain is then extended into
// the gaps between its HSPs, one wave per gap, before it is trimmed (step 5b, at the end of this file).
//
// Symbols are held as in stage_symbols (cpk_device_common.inl): two to a byte, low nibble = even index; the code is
// 0..3 = a c g t, CPK_SYM_N = anything else, and bit 3 marks a lower-case (soft-masked) base.  X and Y strings of all
// problems share one buffer and are addressed by global symbol index, so a sub-problem of the recursion is an offset
// and a length, not a copy.  That holds for the minus strand too: cpk_anchor_revcomp writes the reverse complement of a
// problem's Y behind the forward symbols of the same buffer.

#define CPK_ANCHOR_LOWER 8
#define CPK_ANCHOR_MAX_WEIGHT 15 /* word < 2^30: a key (word << 32 | position) never equals the all-ones filler */
#define CPK_ANCHOR_KEY_NONE (~0ull)
#define CPK_ANCHOR_NO_KEY (-0x7fffffffffffffffLL - 1)
#define CPK_ANCHOR_HIT_EXACT (1 << 24) /* in the y of a listed hit (wy < 2^24): the two words are equal */

struct CpkAnchorSeed {
    int32_t span, weight;
    uint8_t pos[16]; /* offsets of the seed's 1 positions inside the window */
};

__device__ __forceinline__ int anchor_sym(const uint8_t *sym, int64_t g) { return (sym[g >> 1] >> ((int)(g & 1) * 4)) & 15; }

// raw bytes -> packed symbols; one output byte per thread (the partner of a last odd symbol is N)
__global__ void __launch_bounds__(256) cpk_anchor_pack(const uint8_t *raw, int64_t n, uint8_t *sym) {
    const int64_t nOut = (n + 1) >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nOut; i += (int64_t)gridDim.x * blockDim.x) {
        int nib[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int64_t g = 2 * i + h;
            const int c = g < n ? raw[g] : 'N';
            const int u = c & ~32;
            const int code = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : CPK_SYM_N;
            nib[h] = code | ((code != CPK_SYM_N && (c & 32)) ? CPK_ANCHOR_LOWER : 0);
        }
        sym[i] = (uint8_t)(nib[0] | (nib[1] << 4));
    }
}

// Step 0: the reverse complement of the Y range of every problem that asks for it (CPK_ANCHOR_RC_Y): symbol i of the
// range at yOff is the complement of symbol lY - 1 - i of the forward range at yFwd.  One output byte per thread; yOff is
// even, so a byte belongs to one range, and the partner of a last odd symbol is N.  The source nibbles straddle bytes when
// yFwd + lY is odd.  Complementing a code 0..3 is 3 - code; N and the lower-case bit pass through.
__global__ void __launch_bounds__(256) cpk_anchor_revcomp(const CpkAnchorProblem *probs, uint8_t *sym) {
    const CpkAnchorProblem pr = probs[blockIdx.x];
    if (!(pr.flags & CPK_ANCHOR_RC_Y)) return;
    const int nOut = (pr.lY + 1) >> 1;
    uint8_t *out = sym + (pr.yOff >> 1);
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < nOut; i += gridDim.y * blockDim.x) {
        int nib[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int d = 2 * i + h;
            int s = CPK_SYM_N;
            if (d < pr.lY) {
                s = anchor_sym(sym, pr.yFwd + (pr.lY - 1 - d));
                if ((s & 7) < 4) s = (3 - (s & 3)) | (s & CPK_ANCHOR_LOWER);
            }
            nib[h] = s;
        }
        out[i] = (uint8_t)(nib[0] | (nib[1] << 4));
    }
}

// Step 1a: one key per window slot of X (blockIdx.z == 0) or Y (1): word << 32 | position, or the filler for a window
// that is skipped (N or, with softMask, a lower-case base at a 1 position) and for the slots that pad to a power of two.
// A problem that shares the X keys of its twin (CPK_ANCHOR_SHARE_X) has no side 0 of its own.
__global__ void __launch_bounds__(256) cpk_anchor_words(const CpkAnchorProblem *probs, const uint8_t *sym, CpkAnchorSeed seed,
                                                        unsigned long long *keys) {
    const CpkAnchorProblem pr = probs[blockIdx.x];
    const int side = blockIdx.z;
    if (side == 0 && (pr.flags & CPK_ANCHOR_SHARE_X)) return;
    const int cap = side ? pr.capY : pr.capX, l = side ? pr.lY : pr.lX;
    const int64_t off = side ? pr.yOff : pr.xOff;
    unsigned long long *out = keys + (side ? pr.keyYOff : pr.keyXOff);
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < cap; i += gridDim.y * blockDim.x) {
        unsigned long long key = CPK_ANCHOR_KEY_NONE;
        if (i + seed.span <= l) {
            unsigned word = 0;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < seed.weight) {
                    const int s = anchor_sym(sym, off + i + seed.pos[k]);
                    if ((s & 7) > 3 || (pr.softMask && (s & CPK_ANCHOR_LOWER))) ok = false;
                    word = (word << 2) | (unsigned)(s & 3);
                }
            }
            if (ok) key = ((unsigned long long)word << 32) | (unsigned)i;
        }
        out[i] = key;
    }
}

// Bitonic sort of n (a power of two) elements in global memory by one workgroup.
template <typename T, typename Less>
__device__ void anchor_bitonic(T *a, int n, Less less) {
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), m = i | j;
                const T x = a[i], y = a[m];
                const bool sw = (i & k) == 0 ? less(y, x) : less(x, y);
                if (sw) {
                    a[i] = y;
                    a[m] = x;
                }
            }
            __syncthreads();
        }
}

struct AnchorKeyLess {
    __device__ bool operator()(unsigned long long a, unsigned long long b) const { return a < b; }
};

// Step 1b: the keys of one side of one problem in (word, position) order, fillers last.
__global__ void __launch_bounds__(1024) cpk_anchor_sort_keys(const CpkAnchorProblem *probs, unsigned long long *keys) {
    const CpkAnchorProblem pr = probs[blockIdx.x];
    const int side = blockIdx.y;
    if (side == 0 && (pr.flags & CPK_ANCHOR_SHARE_X)) return;  // uniform over the workgroup: no barrier is left behind
    anchor_bitonic(keys + (side ? pr.keyYOff : pr.keyXOff), side ? pr.capY : pr.capX, AnchorKeyLess());
}

// first index in the sorted keys a[0..n) whose word is >= w
__device__ __forceinline__ int anchor_lower_bound(const unsigned long long *a, int n, unsigned long long w) {
    int lo = 0, hi = n;
    const unsigned long long key = w << 32;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int anchor_score(const int *sc, int a, int b) { return sc[(a & 7) * 5 + (b & 7)]; }

// Steps 1c and 2.  One lane per Y window: the X windows with its word (none unless the word occurs at most
// maxSeedOccurrences times on both sides) are its hits.  EXTEND == false counts them; EXTEND == true extends each to an
// HSP and appends those that reach hspThreshold to the problem's list (slot order is arbitrary: cpk_anchor_chain sorts).
template <bool EXTEND>
__global__ void __launch_bounds__(256) cpk_anchor_hits(CpkAnchorProblem *probs, const uint8_t *sym, const unsigned long long *keys,
                                                       CpkAnchorParams prm, int span, int4 *hsps, int32_t *nHsp) {
    __shared__ int sc[25];
    if (threadIdx.x < 25) sc[threadIdx.x] = prm.scores[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x;
    const CpkAnchorProblem pr = probs[p];
    const unsigned long long *kx = keys + pr.keyXOff, *ky = keys + pr.keyYOff;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < pr.capY; i += gridDim.y * blockDim.x) {
        const unsigned long long key = ky[i];
        if (key == CPK_ANCHOR_KEY_NONE) continue;
        const unsigned long long w = key >> 32;
        const int y0 = anchor_lower_bound(ky, pr.capY, w), y1 = anchor_lower_bound(ky, pr.capY, w + 1);
        if (y1 - y0 > prm.maxSeedOccurrences) continue;
        const int x0 = anchor_lower_bound(kx, pr.capX, w), x1 = anchor_lower_bound(kx, pr.capX, w + 1);
        if (x1 == x0 || x1 - x0 > prm.maxSeedOccurrences) continue;
        if (!EXTEND) {
            atomicAdd(&probs[p].hits, x1 - x0);
            continue;
        }
        const int wy = (int)(unsigned)key;
        for (int h = x0; h < x1; h++) {
            const int wx = (int)(unsigned)kx[h];
            int score = 0;
            for (int k = 0; k < span; k++) score += anchor_score(sc, anchor_sym(sym, pr.xOff + wx + k), anchor_sym(sym, pr.yOff + wy + k));
            int lenR = 0, lenL = 0;
            {
                const int room = min(pr.lX - (wx + span), pr.lY - (wy + span));
                const int64_t gx = pr.xOff + wx + span, gy = pr.yOff + wy + span;
                int sum = 0, best = 0;
                for (int k = 0; k < room; k++) {
                    sum += anchor_score(sc, anchor_sym(sym, gx + k), anchor_sym(sym, gy + k));
                    if (sum > best) {
                        best = sum;
                        lenR = k + 1;
                    }
                    if (sum < best - prm.xDrop) break;
                }
                score += best;
            }
            {
                const int room = min(wx, wy);
                const int64_t gx = pr.xOff + wx - 1, gy = pr.yOff + wy - 1;
                int sum = 0, best = 0;
                for (int k = 0; k < room; k++) {
                    sum += anchor_score(sc, anchor_sym(sym, gx - k), anchor_sym(sym, gy - k));
                    if (sum > best) {
                        best = sum;
                        lenL = k + 1;
                    }
                    if (sum < best - prm.xDrop) break;
                }
                score += best;
            }
            if (score >= prm.hspThreshold) {
                const int slot = atomicAdd(&nHsp[p], 1);
                if (slot < pr.hspCap) hsps[pr.hspOff + slot] = make_int4(wx - lenL, wy - lenL, span + lenL + lenR, score);
            }
        }
    }
}

// Step 1c with seedTransitions == 1.  One lane per Y window: 1 + weight lookups among X's sorted keys, its own word and the
// word with one compared base replaced by its transition partner (XOR 2 on the base's two bits: a <-> g, c <-> t).  Only
// words that pass the occurrence filter on their own side seed.  An X and a Y window match by at most one variant, so the
// hits of a lane are distinct.  WRITE == false counts them; WRITE == true appends them as (wx, wy) to the problem's hit
// list, which has the problem's hspCap slots at hspOff (slot order is arbitrary: the HSPs they extend to are sorted).
// The hits of the lane's own word (v == 0) are the exact ones: their wy carries CPK_ANCHOR_HIT_EXACT.
// The lookups are a loop of the same length in every lane; the extension is a kernel of its own with one HIT per lane,
// because a lane here holds up to (1 + weight) * maxSeedOccurrences hits and most lanes hold none.
template <bool WRITE>
__global__ void __launch_bounds__(256) cpk_anchor_join(CpkAnchorProblem *probs, const unsigned long long *keys, int maxOcc, int weight,
                                                       int2 *hitList, int32_t *nHit) {
    const int p = blockIdx.x;
    const CpkAnchorProblem pr = probs[p];
    const unsigned long long *kx = keys + pr.keyXOff, *ky = keys + pr.keyYOff;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < pr.capY; i += gridDim.y * blockDim.x) {
        const unsigned long long key = ky[i];
        if (key == CPK_ANCHOR_KEY_NONE) continue;
        const unsigned long long w = key >> 32;
        const int y0 = anchor_lower_bound(ky, pr.capY, w), y1 = anchor_lower_bound(ky, pr.capY, w + 1);
        if (y1 - y0 > maxOcc) continue;
        const int wy = (int)(unsigned)key;
        int count = 0;
        for (int v = 0; v <= weight; v++) {
            const unsigned long long wv = v == 0 ? w : w ^ (2ull << (2 * (v - 1)));
            const int x0 = anchor_lower_bound(kx, pr.capX, wv), x1 = anchor_lower_bound(kx, pr.capX, wv + 1);
            if (x1 == x0 || x1 - x0 > maxOcc) continue;
            if (WRITE) {
                const int slot = atomicAdd(&nHit[p], x1 - x0);
                const int wyClass = v == 0 ? wy | CPK_ANCHOR_HIT_EXACT : wy;
                for (int h = x0; h < x1; h++)
                    if (slot + (h - x0) < pr.hspCap) hitList[pr.hspOff + slot + (h - x0)] = make_int2((int)(unsigned)kx[h], wyClass);
            }
            count += x1 - x0;
        }
        if (!WRITE && count > 0) atomicAdd(&probs[p].hits, count);
    }
}

// Step 2 with seedTransitions == 1.  One lane per hit of the problem's list: the x-drop walk and slot hand-out of
// cpk_anchor_hits<true>, column for column, and the threshold of the hit's class: hspThreshold for an exact hit,
// variantThreshold (>= hspThreshold; equal to it unless cpecan_anchor_options says otherwise) for a variant hit.  An HSP
// that hits of both classes extend to is appended by the exact ones whatever the others do, and cpk_anchor_chain drops
// its duplicates: the kept set does not depend on the order of the lanes.
__global__ void __launch_bounds__(256) cpk_anchor_extend(const CpkAnchorProblem *probs, const uint8_t *sym, const int2 *hitList,
                                                         CpkAnchorParams prm, int variantThreshold, int span, int4 *hsps,
                                                         int32_t *nHsp) {
    __shared__ int sc[25];
    if (threadIdx.x < 25) sc[threadIdx.x] = prm.scores[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x;
    const CpkAnchorProblem pr = probs[p];
    const int nHits = min(pr.hits, pr.hspCap);
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < nHits; i += gridDim.y * blockDim.x) {
        const int2 hit = hitList[pr.hspOff + i];
        const int wx = hit.x, wy = hit.y & (CPK_ANCHOR_HIT_EXACT - 1);
        const int threshold = (hit.y & CPK_ANCHOR_HIT_EXACT) ? prm.hspThreshold : variantThreshold;
        int score = 0;
        for (int k = 0; k < span; k++) score += anchor_score(sc, anchor_sym(sym, pr.xOff + wx + k), anchor_sym(sym, pr.yOff + wy + k));
        int lenR = 0, lenL = 0;
        {
            const int room = min(pr.lX - (wx + span), pr.lY - (wy + span));
            const int64_t gx = pr.xOff + wx + span, gy = pr.yOff + wy + span;
            int sum = 0, best = 0;
            for (int k = 0; k < room; k++) {
                sum += anchor_score(sc, anchor_sym(sym, gx + k), anchor_sym(sym, gy + k));
                if (sum > best) {
                    best = sum;
                    lenR = k + 1;
                }
                if (sum < best - prm.xDrop) break;
            }
            score += best;
        }
        {
            const int room = min(wx, wy);
            const int64_t gx = pr.xOff + wx - 1, gy = pr.yOff + wy - 1;
            int sum = 0, best = 0;
            for (int k = 0; k < room; k++) {
                sum += anchor_score(sc, anchor_sym(sym, gx - k), anchor_sym(sym, gy - k));
                if (sum > best) {
                    best = sum;
                    lenL = k + 1;
                }
                if (sum < best - prm.xDrop) break;
            }
            score += best;
        }
        if (score >= threshold) {
            const int slot = atomicAdd(&nHsp[p], 1);
            if (slot < pr.hspCap) hsps[pr.hspOff + slot] = make_int4(wx - lenL, wy - lenL, span + lenL + lenR, score);
        }
    }
}

#define CPK_ANCHOR_HSP_NONE make_int4(0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000)
struct AnchorHspByPlace {  // (x, y, length); fillers last
    __device__ bool operator()(const int4 &a, const int4 &b) const {
        if (a.x != b.x) return a.x < b.x;
        if (a.y != b.y) return a.y < b.y;
        return a.z < b.z;
    }
};
struct AnchorHspByScore {  // (score descending, x, y, length); fillers last
    __device__ bool operator()(const int4 &a, const int4 &b) const {
        if (a.w != b.w) return a.w > b.w;
        return AnchorHspByPlace()(a, b);
    }
};

// the largest key of the workgroup (every thread gets it); red: 16 slots of LDS
__device__ __forceinline__ long long anchor_block_max(long long v, long long *red) {
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    __syncthreads();  // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = red[w] > r ? red[w] : r;
    return r;
}

// Steps 2 (duplicates) to 5, one workgroup per problem.  hsps: the problem's hspCap slots, of which the first nHsp[p] were
// filled by cpk_anchor_hits; best / pred: hspCap ints each; runs: hspCap triples (x, y, length), relative to the problem.
//
// UNTRIMMED (cpk_anchor_chain_untrimmed, step 5b): the pass extends chains, and a problem with CPK_ANCHOR_GAPPED leaves
// its chain in `runs` as it is, in chain order, with nRuns == 0; gapRow gets, at hspOff + p + g for gap g = 0 .. chained,
// the scratch rows of the gaps in front of g (anchor_gap_rows), and `columns` their total, which the host sizes by.
__device__ __forceinline__ int anchor_gap_rows(int m, int n, bool right, bool left, int maxDiags) {
    const int rows = min(m + n, maxDiags);
    return (right ? rows : 0) + (left ? rows : 0);
}

// What comes before step 4 on one problem's list, by the whole workgroup: the slots behind the nIn filled ones padded, the
// list sorted by place, exact duplicates dropped (step 2), the cap of step 3, sorted by place again.  hsp: the problem's
// cap slots; pred: cap ints of scratch.  Returns the size of the pool; *nUnique: the HSPs before the cap; *capped: step 3
// cut.  Every thread gets the same values, and the list is ready for all of them (cpk_anchor_chain and cpk_local_peel
// share this).
__device__ __forceinline__ int anchor_pool_prepare(int4 *hsp, int cap, int nIn, int maxHsps, int32_t *pred, int *nUnique, int *capped) {
    __shared__ int shCount;
    const int tid = threadIdx.x, nT = blockDim.x;
    int n = min(nIn, cap);
    for (int i = n + tid; i < cap; i += nT) hsp[i] = CPK_ANCHOR_HSP_NONE;
    if (tid == 0) shCount = 0;
    anchor_bitonic(hsp, cap, AnchorHspByPlace());
    // exact duplicates of (x, y, length) follow each other; the score is a function of the three
    for (int i = tid; i < n; i += nT) {
        bool dup = false;
        if (i > 0) {
            const int4 a = hsp[i - 1], b = hsp[i];
            dup = a.x == b.x && a.y == b.y && a.z == b.z;
        }
        pred[i] = dup;
        if (!dup) atomicAdd(&shCount, 1);
    }
    __syncthreads();
    for (int i = tid; i < n; i += nT)
        if (pred[i]) hsp[i] = CPK_ANCHOR_HSP_NONE;
    __syncthreads();
    *nUnique = shCount;
    if (*nUnique != n) anchor_bitonic(hsp, cap, AnchorHspByPlace());
    n = *nUnique;
    *capped = 0;
    if (n > maxHsps) {  // step 3
        *capped = 1;
        anchor_bitonic(hsp, cap, AnchorHspByScore());
        for (int i = maxHsps + tid; i < n; i += nT) hsp[i] = CPK_ANCHOR_HSP_NONE;
        n = maxHsps;
        anchor_bitonic(hsp, cap, AnchorHspByPlace());
    }
    __syncthreads();
    return n;
}

template <bool UNTRIMMED>
__device__ __forceinline__ void anchor_chain_body(CpkAnchorProblem *probs, int4 *hspsAll, const int32_t *nHsp, int32_t *bestAll,
                                                  int32_t *predAll, int32_t *runsAll, int maxHsps, int trim, int32_t *gapRow) {
    __shared__ long long red[16];
    const int p = blockIdx.x, tid = threadIdx.x, nT = blockDim.x;
    const CpkAnchorProblem pr = probs[p];
    int4 *hsp = hspsAll + pr.hspOff;
    int32_t *best = bestAll + pr.hspOff, *pred = predAll + pr.hspOff, *runs = runsAll + 3 * pr.hspOff;
    int nUnique, capped;
    const int n = anchor_pool_prepare(hsp, pr.hspCap, nHsp[p], maxHsps, pred, &nUnique, &capped);
    // step 4: predecessors of i have a smaller x, so they come before i
    for (int i = 0; i < n; i++) {
        const int4 me = hsp[i];
        long long key = CPK_ANCHOR_NO_KEY;
        for (int j = tid; j < i; j += nT) {
            const int4 o = hsp[j];
            if (o.x + o.z <= me.x && o.y + o.z <= me.y) {
                const long long k = (long long)best[j] * 4294967296LL + (unsigned)~j;  // largest best, then smallest j
                key = k > key ? k : key;
            }
        }
        key = anchor_block_max(key, red);
        if (tid == 0) {
            best[i] = me.w + (key == CPK_ANCHOR_NO_KEY ? 0 : (int)(key >> 32));
            pred[i] = key == CPK_ANCHOR_NO_KEY ? -1 : (int)~(unsigned)key;
        }
        __syncthreads();
    }
    long long endKey = CPK_ANCHOR_NO_KEY;
    for (int i = tid; i < n; i += nT) {
        const long long k = (long long)best[i] * 4294967296LL + (unsigned)~i;
        endKey = k > endKey ? k : endKey;
    }
    endKey = anchor_block_max(endKey, red);
    if (tid == 0) {
        // step 5: walk back from the end, then write the trimmed runs in increasing order (best[] is free: it holds the walk)
        int m = 0;
        for (int i = n > 0 ? (int)~(unsigned)endKey : -1; i >= 0; i = pred[i]) best[m++] = i;
        int nRuns = 0, toTrim = m;
        long long columns = 0;
        if (UNTRIMMED && (pr.flags & CPK_ANCHOR_GAPPED)) {
            int32_t *rowAt = gapRow + pr.hspOff + p;
            const int maxDiags = CPK_ANCHOR_DIAGS(pr.flags);
            int pX = 0, pY = 0;
            for (int g = 0; g <= m; g++) {
                rowAt[g] = (int32_t)columns;
                int4 h = make_int4(pr.lX, pr.lY, 0, 0);
                if (g < m) {
                    h = hsp[best[m - 1 - g]];
                    runs[3 * g] = h.x;
                    runs[3 * g + 1] = h.y;
                    runs[3 * g + 2] = h.z;
                }
                columns += anchor_gap_rows(h.x - pX, h.y - pY, g >= 1, g < m, maxDiags);
                pX = h.x + h.z;
                pY = h.y + h.z;
            }
            toTrim = 0;  // step 5 comes after the extension (cpk_anchor_assemble)
        }
        for (int k = toTrim - 1; k >= 0; k--) {
            const int4 h = hsp[best[k]];
            const int len = h.z - 2 * trim;
            if (len > 0) {
                runs[3 * nRuns] = h.x + trim;
                runs[3 * nRuns + 1] = h.y + trim;
                runs[3 * nRuns + 2] = len;
                nRuns++;
                columns += len;
            }
        }
        probs[p].hsps = nUnique;
        probs[p].chained = m;
        probs[p].nRuns = nRuns;
        probs[p].columns = columns;
        probs[p].capped = capped;
        probs[p].score = n > 0 ? (int32_t)(endKey >> 32) : 0;  // the chain score: the strand score of a top-level pass
    }
}

__global__ void __launch_bounds__(256) cpk_anchor_chain(CpkAnchorProblem *probs, int4 *hspsAll, const int32_t *nHsp, int32_t *bestAll,
                                                        int32_t *predAll, int32_t *runsAll, int maxHsps, int trim) {
    anchor_chain_body<false>(probs, hspsAll, nHsp, bestAll, predAll, runsAll, maxHsps, trim, nullptr);
}

__global__ void __launch_bounds__(256) cpk_anchor_chain_untrimmed(CpkAnchorProblem *probs, int4 *hspsAll, const int32_t *nHsp,
                                                                  int32_t *bestAll, int32_t *predAll, int32_t *runsAll, int maxHsps,
                                                                  int trim, int32_t *gapRow) {
    anchor_chain_body<true>(probs, hspsAll, nHsp, bestAll, predAll, runsAll, maxHsps, trim, gapRow);
}

// ---- step 5b: gapped extension of the chain (include/cpecan_hip.h: cpecan_anchor_options.gappedExtension) ----
// One wave per (problem, gap) runs the gap's right and left extension, applies the overlap rule and writes the gap's blocks;
// no wave waits for another.  Lane l owns the matrix diagonal i - j = l - 32 (lane 0 owns none), and the states of the two
// anti-diagonals before d are in registers: the I predecessor (i - 1, j) is lane l - 1 of d - 1, the D predecessor
// (i, j - 1) lane l + 1 of d - 1, the M predecessor (i - 1, j - 1) the same lane of d - 2.  A wave shift (DPP wave_shr /
// wave_shl, which cross the 16-lane rows) fetches the neighbours; a lane without a source keeps NO_PATH.
// NO_PATH stands for minus infinity: a state is a real sum (above -2^20: 4096 anti-diagonals of at most 130 each) or
// exactly NO_PATH, because nothing is derived from a NO_PATH source.
#define CPK_ANCHOR_NO_PATH (-(1 << 29))
#define CPK_ANCHOR_IS_PATH(v) ((v) > CPK_ANCHOR_NO_PATH / 2)

__device__ __forceinline__ int anchor_lane_below(int v) {  // lane l: lane l - 1's v
    return __builtin_amdgcn_update_dpp(CPK_ANCHOR_NO_PATH, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ int anchor_lane_above(int v) {  // lane l: lane l + 1's v
    return __builtin_amdgcn_update_dpp(CPK_ANCHOR_NO_PATH, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

struct AnchorReach {
    int best, i, j;  // the best M cell; best == 0: the extension is empty
};

// The walk of one extension.  Symbol i of the gap's X is at xAt + dir * i (dir == -1: the reversed strings of a left
// extension), likewise Y.  trace: dMax rows of 64 bytes, row d - 1 for anti-diagonal d; a lane's byte holds the source of
// its M (bits 0-1: 0 M, 1 I, 2 D), of its I (bit 2: 0 M, 1 I) and of its D (bit 3: 0 M, 1 D).
__device__ AnchorReach anchor_gapped_walk(const uint8_t *sym, const int *sc, int64_t xAt, int64_t yAt, int dir, int m, int n,
                                          int yDrop, int dMax, uint8_t *trace) {
    const int lane = threadIdx.x, k = lane - 32;
    const int openExtend = CPECAN_ANCHOR_GAP_OPEN + CPECAN_ANCHOR_GAP_EXTEND;
    int m1 = lane == 32 ? 0 : CPK_ANCHOR_NO_PATH, i1 = CPK_ANCHOR_NO_PATH, d1 = CPK_ANCHOR_NO_PATH;  // anti-diagonal d - 1
    int x1 = m1, s1 = 0;                  // the largest of its three states and which (M, then I, then D)
    int x2 = CPK_ANCHOR_NO_PATH, s2 = 0;  // the same of d - 2
    AnchorReach r = {0, 0, 0};
    int topBefore = 0;
    for (int d = 1; d <= dMax; d++) {
        const int i = (d + k) >> 1, j = (d - k) >> 1;
        const bool cell = lane >= 1 && ((d + k) & 1) == 0 && i >= 0 && i <= m && j >= 0 && j <= n;
        const int belowM = anchor_lane_below(m1), belowI = anchor_lane_below(i1);
        const int aboveM = anchor_lane_above(m1), aboveD = anchor_lane_above(d1);
        int mNew = CPK_ANCHOR_NO_PATH, iNew = CPK_ANCHOR_NO_PATH, dNew = CPK_ANCHOR_NO_PATH;
        unsigned bits = 0;
        if (cell) {
            if (i >= 1 && j >= 1 && CPK_ANCHOR_IS_PATH(x2)) {
                mNew = x2 + anchor_score(sc, anchor_sym(sym, xAt + (int64_t)dir * (i - 1)), anchor_sym(sym, yAt + (int64_t)dir * (j - 1)));
                bits = (unsigned)s2;
            }
            if (i >= 1 && (CPK_ANCHOR_IS_PATH(belowM) || CPK_ANCHOR_IS_PATH(belowI))) {
                const int open = belowM - openExtend, extend = belowI - CPECAN_ANCHOR_GAP_EXTEND;  // a tie goes to M
                iNew = max(open, extend);
                bits |= extend > open ? 4u : 0u;
            }
            if (j >= 1 && (CPK_ANCHOR_IS_PATH(aboveM) || CPK_ANCHOR_IS_PATH(aboveD))) {
                const int open = aboveM - openExtend, extend = aboveD - CPECAN_ANCHOR_GAP_EXTEND;
                dNew = max(open, extend);
                bits |= extend > open ? 8u : 0u;
            }
        }
        trace[(size_t)(d - 1) * 64 + lane] = (uint8_t)bits;
        int xNew = mNew, sNew = 0;
        if (iNew > xNew) xNew = iNew, sNew = 1;
        if (dNew > xNew) xNew = dNew, sNew = 2;
        // wave-uniform: the largest M of d, on the smallest i - j among equals, and top(d)
        long long key = (long long)mNew * 64 + (63 - lane);
        int top = xNew;
        for (int o = 32; o > 0; o >>= 1) {
            const long long u = __shfl_xor(key, o);
            key = u > key ? u : key;
            top = max(top, __shfl_xor(top, o));
        }
        const int dBest = (int)(key >> 6);
        if (dBest > r.best) {  // strictly: the smallest d keeps it
            const int kBest = 63 - (int)(key & 63) - 32;
            r.best = dBest;
            r.i = (d + kBest) >> 1;
            r.j = (d - kBest) >> 1;
        }
        // both anti-diagonals a cell reads are under the bound: nothing that follows can reach it
        if (top < r.best - yDrop && topBefore < r.best - yDrop) break;
        topBefore = top;
        x2 = x1, s2 = s1;
        x1 = xNew, s1 = sNew;
        m1 = mNew, i1 = iNew, d1 = dNew;
    }
    return r;
}

// The way back from the best cell in state M to (0, 0); every M step is the aligned column (i - 1, j - 1), and the maximal
// runs of them on one matrix diagonal are the blocks.  The walk meets them from the last to the first.  A right extension
// (left == false) has its corner (cX, cY) below: block (i, j, len) is (cX + i, cY + j, len), written from slot cap - 1
// downwards so that they end up ascending in the last slots.  A left extension walked the reversed strings from the corner
// above: the block is (cX - i - len, cY - j - len, len), ascending as met, written from slot 0 upwards.  Every lane walks;
// lane 0 writes.  Returns the number of blocks (at most cap: a block takes two anti-diagonals and a gap between two one).
__device__ int anchor_gapped_blocks(const uint8_t *trace, AnchorReach r, bool left, int cX, int cY, int32_t *out, int cap) {
    int i = r.i, j = r.j, state = 0, nBlocks = 0, len = 0;
    while (i >= 0 && j >= 0 && i + j > 0) {  // (0, 0) is reached in state M: I and D have no path there
        const unsigned bits = trace[(size_t)(i + j - 1) * 64 + (i - j + 32)];
        if (state == 0) {
            i--, j--, len++;  // the block so far: (i, j, len)
            state = (int)(bits & 3);
            if (state != 0 || (i == 0 && j == 0)) {
                if (threadIdx.x == 0 && nBlocks < cap) {
                    int32_t *q = out + 3 * (left ? nBlocks : cap - 1 - nBlocks);
                    q[0] = left ? cX - i - len : cX + i;
                    q[1] = left ? cY - j - len : cY + j;
                    q[2] = len;
                }
                nBlocks++;
                len = 0;
            }
        } else if (state == 1) {
            i--;
            state = (bits & 4) ? 1 : 0;
        } else {
            j--;
            state = (bits & 8) ? 2 : 0;
        }
    }
    return min(nBlocks, cap);
}

// gapRow, rowBase: where the rows of a gap start (cpk_anchor_chain_untrimmed, cpk_anchor_gapped_size).  A launch does the
// gaps whose rows start in [lo, hi), a range the host cuts at gap boundaries so that `trace` holds hi - lo rows.  blocks: a
// triple per row of the whole pass, gap by gap as the rows lie: the right extension's, then the left one's.  counts: per gap
// the blocks kept of either (zeroed before the first launch: a gap without rows is never visited).
__global__ void __launch_bounds__(64) cpk_anchor_gapped(const CpkAnchorProblem *probs, const uint8_t *sym, CpkAnchorParams prm,
                                                        const int32_t *chainAll, const int32_t *gapRow, const int64_t *rowBase,
                                                        int64_t lo, int64_t hi, uint8_t *trace, int32_t *blocks, int2 *counts) {
    __shared__ int sc[25];
    if (threadIdx.x < 25) sc[threadIdx.x] = prm.scores[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x, g = blockIdx.y;
    const CpkAnchorProblem pr = probs[p];
    const int c = pr.chained;
    if (!(pr.flags & CPK_ANCHOR_GAPPED) || g > c) return;
    const int32_t *chain = chainAll + 3 * pr.hspOff;
    const int aX = g ? chain[3 * (g - 1)] + chain[3 * (g - 1) + 2] : 0, aY = g ? chain[3 * (g - 1) + 1] + chain[3 * (g - 1) + 2] : 0;
    const int bX = g < c ? chain[3 * g] : pr.lX, bY = g < c ? chain[3 * g + 1] : pr.lY;
    const int m = bX - aX, n = bY - aY;
    const bool right = g >= 1, left = g < c;
    const int rows = min(m + n, CPK_ANCHOR_DIAGS(pr.flags)), rowsR = right ? rows : 0;
    const int64_t row0 = rowBase[p] + gapRow[pr.hspOff + p + g];
    if (rows == 0 || row0 < lo || row0 >= hi) return;
    uint8_t *traceR = trace + (size_t)(row0 - lo) * 64, *traceL = traceR + (size_t)rowsR * 64;
    int32_t *blocksR = blocks + 3 * row0, *blocksL = blocksR + 3 * rowsR;
    AnchorReach R = {0, 0, 0}, L = {0, 0, 0};
    if (right) R = anchor_gapped_walk(sym, sc, pr.xOff + aX, pr.yOff + aY, 1, m, n, pr.yDrop, rows, traceR);
    if (left) L = anchor_gapped_walk(sym, sc, pr.xOff + bX - 1, pr.yOff + bY - 1, -1, m, n, pr.yDrop, rows, traceL);
    if (R.i + L.i > m || R.j + L.j > n) {  // they overlap: the smaller best goes, the left one on a tie
        if (R.best < L.best) R.best = 0;
        else L.best = 0;
    }
    __threadfence();  // the bytes other lanes stored are read below
    const int nR = R.best > 0 ? anchor_gapped_blocks(traceR, R, false, aX, aY, blocksR, rows) : 0;
    const int nL = L.best > 0 ? anchor_gapped_blocks(traceL, L, true, bX, bY, blocksL, rows) : 0;
    if (threadIdx.x == 0) counts[pr.hspOff + p + g] = make_int2(nR, nL);
}

// Assembly and step 5, thread 0 of a workgroup per problem as in cpk_anchor_chain: per gap the right blocks, the left
// blocks, then the next HSP; neighbours that continue each other merged; every merged block trimmed.  The problem's runs go
// to runBase[p] of runsOut, where hspOff points afterwards; a problem whose chain was not extended has its runs copied.
__global__ void __launch_bounds__(64) cpk_anchor_assemble(CpkAnchorProblem *probs, const int32_t *chainAll, const int32_t *gapRow,
                                                          const int64_t *rowBase, const int64_t *runBase, const int32_t *blocks,
                                                          const int2 *counts, int32_t *runsOut, int trim) {
    if (threadIdx.x != 0) return;
    const int p = blockIdx.x;
    const CpkAnchorProblem pr = probs[p];
    const int32_t *chain = chainAll + 3 * pr.hspOff;
    int32_t *out = runsOut + 3 * runBase[p];
    probs[p].hspOff = runBase[p];
    if (!(pr.flags & CPK_ANCHOR_GAPPED)) {
        for (int k = 0; k < 3 * pr.nRuns; k++) out[k] = chain[k];
        return;
    }
    const int c = pr.chained, maxDiags = CPK_ANCHOR_DIAGS(pr.flags);
    int nRuns = 0, x = 0, y = 0, len = 0, pX = 0, pY = 0;
    long long columns = 0;
    auto flush = [&]() {
        if (len - 2 * trim > 0) {
            out[3 * nRuns] = x + trim;
            out[3 * nRuns + 1] = y + trim;
            out[3 * nRuns + 2] = len - 2 * trim;
            nRuns++;
            columns += len - 2 * trim;
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
        const int hX = g < c ? chain[3 * g] : pr.lX, hY = g < c ? chain[3 * g + 1] : pr.lY, hLen = g < c ? chain[3 * g + 2] : 0;
        const int rowsR = g >= 1 ? min(hX - pX + hY - pY, maxDiags) : 0;
        const int2 cnt = counts[pr.hspOff + p + g];
        const int32_t *q = blocks + 3 * (rowBase[p] + gapRow[pr.hspOff + p + g] + rowsR);
        for (int t = -cnt.x; t < cnt.y; t++) put(q[3 * t], q[3 * t + 1], q[3 * t + 2]);  // the right ones end where the left ones start
        if (g < c) put(hX, hY, hLen);
        pX = hX + hLen;
        pY = hY + hLen;
    }
    flush();
    probs[p].nRuns = nRuns;
    probs[p].columns = columns;
}
