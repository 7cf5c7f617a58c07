// cpk_viterbi.inl -- Viterbi decoding of a region: the most probable banded state path and its log-probability
// (include/cpecan_viterbi.h).  Part of the single HIP translation unit cpecan_kernels.hip; not compiled
// on its own.  Not a variant of the kernel table, and the launch plan does not know it.
//
//   cpecan_viterbi_sweep<LDS>  one wave per region: V of diagonals 0 .. N, lanes across the cells of a diagonal, three rolling
//                              rows of S doubles per cell -- in LDS (rows of the launch's widest diagonal), or in global memory
//                              read back behind a barrier (ld_self) for regions whose diagonals are too wide -- and one
//                              pointer byte per band cell to global memory, diagonal by diagonal
//   cpecan_viterbi_traceback   one wave per region: the pointer bytes the path can reach on the next CPK_VIT_BLOCK_DIAGS
//                              diagonals are staged in LDS by the whole wave (a triangle: j diagonals down the path has moved
//                              at most j steps sideways), one lane walks them there and writes the run-length ops, last run
//                              first, with plain stores
//
// Candidates are compared with > so that the first transition of the model's ordered list wins a tie; every candidate is
// V[src][from] + (e + tP), in this association.  No logAdd, no exp / log: the bytes do not depend on the build of logadd.
//
// The pointer byte.  Five states: bits 0-2 the match state's source, bit 3 / 4 / 5 / 6 whether shortX / shortY / longX /
// longY came from itself (1) or from the match state (0).  Three states: bits 0-1 / 2-3 / 4-5 the source of match / gapX /
// gapY.  A state whose candidates were all -inf has no meaningful field; the traceback never reaches it: it starts from a
// finite value and every pointer it follows was set by a finite candidate.

struct VitArgs {
    const CpkVitRegion *regions;
    const CpkVitDiag *diags;
    const uint8_t *symbols;
    const int32_t *order;
    uint8_t *ptr;
    double *roll;
    CpkVitOut *out;
    int32_t *ops;
    int32_t ldsStride;  // doubles per state row of an LDS rolling row
};

constexpr int kVitEm = 40;  // matchEm[25], gapXEm[5] at 25, gapYEm[5] at 30, padded

// cand > best keeps the pointer; never fmax
#define VIT_TAKE(best, from, cand, code) \
    do {                                 \
        const double c_ = (cand);        \
        if (c_ > best) {                 \
            best = c_;                   \
            from = (code);               \
        }                                \
    } while (0)

// The rolling rows of one region: row r, state s, cell k.  LDS: [r][s][stride]; global: [r][k][s] read with ld_self.
template <bool LDS, int S>
struct VitRows {
    double *base;
    int stride;
    __device__ __forceinline__ double get(int r, int k, int s) const {
        if constexpr (LDS) return base[(r * S + s) * stride + k];
        else return ld_self(base + ((int64_t)r * stride + k) * S + s);
    }
    __device__ __forceinline__ void put(int r, int k, int s, double v) const {
        if constexpr (LDS) base[(r * S + s) * stride + k] = v;
        else base[((int64_t)r * stride + k) * S + s] = v;
    }
};

template <bool LDS, int S>
__device__ __forceinline__ void vit_load(double (&v)[S], const VitRows<LDS, S> &rows, int r, int k) {
#pragma unroll
    for (int s = 0; s < S; s++) v[s] = NEG_INF;
    if (k >= 0) {
#pragma unroll
        for (int s = 0; s < S; s++) v[s] = rows.get(r, k, s);
    }
}

__device__ __forceinline__ int vit_cell_index(const CpkVitDiag &g, bool valid, int xmy) {
    const int k = (xmy - g.xmyL) >> 1;
    return valid && xmy >= g.xmyL && k < g.width ? k : -1;
}

template <bool LDS, int S>
__device__ __forceinline__ void vit_sweep_region(const CpkModel &m, const VitArgs &a, const double *em, double *ldsRows) {
    const int ri = a.order[blockIdx.x];
    const CpkVitRegion rg = a.regions[ri];
    const int N = rg.lX + rg.lY, lane = threadIdx.x;
    const CpkVitDiag *diags = a.diags + rg.diagOff;
    const uint8_t *sx = a.symbols + rg.symX, *sy = a.symbols + rg.symY;
    uint8_t *ptr = a.ptr + rg.ptrBase;
    VitRows<LDS, S> rows;
    rows.base = LDS ? ldsRows : a.roll + rg.rollBase;
    rows.stride = LDS ? a.ldsStride : rg.maxWidth;
    if (lane == 0) {  // diagonal 0: the one cell (0, 0)
#pragma unroll
        for (int s = 0; s < S; s++) rows.put(0, 0, s, rg.raggedLeft ? m.raggedStart[s] : m.start[s]);
        ptr[0] = 0;
    }
    __syncthreads();
    CpkVitDiag g2 = diags[0], g1 = diags[0];  // diagonals d - 2 and d - 1
    int r2 = 0, r1 = 0, r0 = 1;               // their rows and the row of d
    for (int d = 1; d <= N; d++) {
        const CpkVitDiag g = diags[d];
        for (int k = lane; k < g.width; k += CPK_WAVE) {
            const int xmy = g.xmyL + 2 * k, x = (d + xmy) >> 1, y = (d - xmy) >> 1;
            const int cX = sx[x], cY = sy[y];
            const double eM = em[cX * 5 + cY], eX = em[25 + cX], eY = em[30 + cY];
            double lo[S], mi[S], up[S], best[S];
            vit_load<LDS, S>(lo, rows, r1, vit_cell_index(g1, true, xmy - 1));    // (x - 1, y)
            vit_load<LDS, S>(mi, rows, r2, vit_cell_index(g2, d >= 2, xmy));      // (x - 1, y - 1)
            vit_load<LDS, S>(up, rows, r1, vit_cell_index(g1, true, xmy + 1));    // (x, y - 1)
#pragma unroll
            for (int s = 0; s < S; s++) best[s] = NEG_INF;
            int pM = 0, pSX = 0, pSY = 0;
            unsigned code;
            if constexpr (S == 5) {  // the list of impl/stateMachine.c:450-480, in its order
                int pLX = 0, pLY = 0;
                VIT_TAKE(best[1], pSX, lo[0] + (eX + m.shortOpenX), 0);
                VIT_TAKE(best[1], pSX, lo[1] + (eX + m.shortExtendX), 1);
                VIT_TAKE(best[3], pLX, lo[0] + (eX + m.longOpenX), 0);
                VIT_TAKE(best[3], pLX, lo[3] + (eX + m.longExtendX), 1);
                VIT_TAKE(best[0], pM, mi[0] + (eM + m.matchContinue), 0);
                VIT_TAKE(best[0], pM, mi[1] + (eM + m.matchFromShortX), 1);
                VIT_TAKE(best[0], pM, mi[2] + (eM + m.matchFromShortY), 2);
                VIT_TAKE(best[0], pM, mi[3] + (eM + m.matchFromLongX), 3);
                VIT_TAKE(best[0], pM, mi[4] + (eM + m.matchFromLongY), 4);
                VIT_TAKE(best[2], pSY, up[0] + (eY + m.shortOpenY), 0);
                VIT_TAKE(best[2], pSY, up[2] + (eY + m.shortExtendY), 1);
                VIT_TAKE(best[4], pLY, up[0] + (eY + m.longOpenY), 0);
                VIT_TAKE(best[4], pLY, up[4] + (eY + m.longExtendY), 1);
                code = (unsigned)pM | (unsigned)pSX << 3 | (unsigned)pSY << 4 | (unsigned)pLX << 5 | (unsigned)pLY << 6;
            } else {  // :689-714
                VIT_TAKE(best[1], pSX, lo[0] + (eX + m.shortOpenX), 0);
                VIT_TAKE(best[1], pSX, lo[1] + (eX + m.shortExtendX), 1);
                VIT_TAKE(best[1], pSX, lo[2] + (eX + m.shortSwitchToX), 2);
                VIT_TAKE(best[0], pM, mi[0] + (eM + m.matchContinue), 0);
                VIT_TAKE(best[0], pM, mi[1] + (eM + m.matchFromShortX), 1);
                VIT_TAKE(best[0], pM, mi[2] + (eM + m.matchFromShortY), 2);
                VIT_TAKE(best[2], pSY, up[0] + (eY + m.shortOpenY), 0);
                VIT_TAKE(best[2], pSY, up[2] + (eY + m.shortExtendY), 2);
                VIT_TAKE(best[2], pSY, up[1] + (eY + m.shortSwitchToY), 1);
                code = (unsigned)pM | (unsigned)pSX << 2 | (unsigned)pSY << 4;
            }
#pragma unroll
            for (int s = 0; s < S; s++) rows.put(r0, k, s, best[s]);
            ptr[g.cellOff + k] = (uint8_t)code;
        }
        __syncthreads();  // the row is visible to the whole (single-wave) workgroup before the next diagonal reads it
        g2 = g1;
        g1 = g;
        r2 = r1;
        r1 = r0;
        r0 = r0 == 2 ? 0 : r0 + 1;
    }
    if (lane == 0) {  // the last diagonal is the one cell (lX, lY), in row r1
        double logP = NEG_INF;
        int endState = -1;
        for (int s = 0; s < S; s++) {
            const double c = rows.get(r1, 0, s) + (rg.raggedRight ? m.raggedEnd[s] : m.end[s]);
            if (c > logP) {
                logP = c;
                endState = s;
            }
        }
        CpkVitOut o;
        o.logP = logP;
        o.startState = -1;
        o.endState = endState;
        o.nOps = 0;
        o.pad = 0;
        a.out[ri] = o;
    }
}

template <bool LDS>
__global__ void __launch_bounds__(CPK_WAVE) cpecan_viterbi_sweep(const CpkModel m, const VitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double vitLds[];  // em, then the LDS rows
    double *em = vitLds;
    for (int i = threadIdx.x; i < kVitEm; i += CPK_WAVE) em[i] = i < 25 ? m.matchEm[i] : i < 30 ? m.gapXEm[i - 25] : i < 35 ? m.gapYEm[i - 30] : 0.0;
    __syncthreads();
    if (m.nStates == 5) vit_sweep_region<LDS, 5>(m, a, em, vitLds + kVitEm);
    else vit_sweep_region<LDS, 3>(m, a, em, vitLds + kVitEm);
}

// The state a pointer byte names as the source of state s, and the step s made.
template <int S>
__device__ __forceinline__ int vit_source(unsigned code, int s) {
    if constexpr (S == 5) {
        if (s == 0) return (int)(code & 7u);
        return (code >> (s == 1 ? 3 : s == 2 ? 4 : s == 3 ? 5 : 6)) & 1u ? s : 0;
    } else {
        return (int)((code >> (2 * s)) & 3u);
    }
}

template <int S>
__device__ __forceinline__ void vit_traceback_region(const VitArgs &a, uint8_t (*stage)[CPK_VIT_BLOCK_DIAGS], volatile int *walk) {
    const int ri = blockIdx.x;
    const CpkVitRegion rg = a.regions[ri];
    const CpkVitOut o = a.out[ri];
    if (o.endState < 0) return;  // no path: the sweep's record stands
    const int lane = threadIdx.x;
    const CpkVitDiag *diags = a.diags + rg.diagOff;
    const uint8_t *ptr = a.ptr + rg.ptrBase;
    int32_t *ops = a.ops + 2 * rg.opBase;
    // walk[0..2]: the diagonal, x - y and state the next block starts from; walk[3..5]: the open run's state and length, ops written
    if (lane == 0) {
        walk[0] = rg.lX + rg.lY;
        walk[1] = rg.lX - rg.lY;
        walk[2] = o.endState;
        walk[3] = -1;
        walk[4] = 0;
        walk[5] = 0;
    }
    __syncthreads();
    while (walk[0] > 0) {
        const int dTop = walk[0], xmy0 = walk[1];
        // diagonal dTop - j can be reached at x - y in xmy0 - j .. xmy0 + j only: byte i of its row is x - y = xmy0 - j + 2 i
        for (int j = 0; j < CPK_VIT_BLOCK_DIAGS && j < dTop; j++) {
            if (lane > j) continue;
            const CpkVitDiag g = diags[dTop - j];
            const int xmy = xmy0 - j + 2 * lane, k = (xmy - g.xmyL) >> 1;
            stage[j][lane] = xmy >= g.xmyL && k < g.width ? ptr[g.cellOff + k] : (uint8_t)0;
        }
        __syncthreads();
        if (lane == 0) {
            int d = dTop, xmy = xmy0, s = walk[2], runState = walk[3], runLen = walk[4], nOps = walk[5];
            while (d > 0 && dTop - d < CPK_VIT_BLOCK_DIAGS) {
                const int j = dTop - d;
                const unsigned code = stage[j][(xmy - (xmy0 - j)) >> 1];
                if (s == runState) runLen++;
                else {
                    if (runLen > 0) {
                        ops[2 * nOps] = runState;
                        ops[2 * nOps + 1] = runLen;
                        nOps++;
                    }
                    runState = s;
                    runLen = 1;
                }
                const int from = vit_source<S>(code, s);
                if (s == 0) d -= 2;              // (x - 1, y - 1)
                else if (s == 1 || s == 3) {     // (x - 1, y)
                    d -= 1;
                    xmy -= 1;
                } else {                         // (x, y - 1)
                    d -= 1;
                    xmy += 1;
                }
                s = from;
            }
            walk[0] = d;
            walk[1] = xmy;
            walk[2] = s;
            walk[3] = runState;
            walk[4] = runLen;
            walk[5] = nOps;
        }
        __syncthreads();
    }
    if (lane == 0) {
        int nOps = walk[5];
        if (walk[4] > 0) {
            ops[2 * nOps] = walk[3];
            ops[2 * nOps + 1] = walk[4];
            nOps++;
        }
        a.out[ri].startState = walk[2];
        a.out[ri].nOps = nOps;
    }
}

__global__ void __launch_bounds__(CPK_WAVE) cpecan_viterbi_traceback(const int nStates, const VitArgs a) {
    __shared__ uint8_t stage[CPK_VIT_BLOCK_DIAGS][CPK_VIT_BLOCK_DIAGS];
    __shared__ int walk[6];
    if (nStates == 5) vit_traceback_region<5>(a, stage, walk);
    else vit_traceback_region<3>(a, stage, walk);
}

// ---- Counts of the decoded paths: Viterbi training's E-step (include/cpecan_viterbi.h) ----
//
//   cpecan_viterbi_count         one wave per region, after the traceback, over the ops it left on the device (run-length
//                                encoded, last run first).  A pass lays out 64 runs, one per lane: three wave scans give every
//                                run its end cell -- (lX, lY) minus the steps of the runs stored before it -- and its first
//                                step among the pass's steps; the source state of a run's first step is the state of the run
//                                stored after it, startState for the last stored run.  Transitions are arithmetic on the runs:
//                                1 to trans[prev][s] (a ballot and a population count per pair of states), L - 1 to
//                                trans[s][s] (a wave sum per state).  The steps of the pass are then spread over the lanes, 64
//                                at a time whichever run they belong to (a binary search in the scanned lengths, in LDS), each
//                                lane reads its cell's two symbols, and every emission bin present is counted with a ballot
//                                and a population count.  Lane l keeps bins l and l + 64 in two registers: no atomics, no
//                                LDS read-modify-write; the region's S * S + S * 16 bins leave as one slab of plain stores.
//   cpecan_viterbi_count_reduce  one workgroup per bin: thread t sums the slabs of regions t, t + 256, ... in ascending order,
//                                the 256 partial sums are folded pairwise in a fixed order, and thread 0 adds the total to
//                                the run's int64 bin.  Integers: any order gives these bytes; this one is fixed.

__device__ __forceinline__ int vit_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int off = 1; off < CPK_WAVE; off <<= 1) {
        const int t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

__device__ __forceinline__ int vit_wave_sum(int v) {
#pragma unroll
    for (int off = CPK_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int S>
__device__ __forceinline__ void vit_count_region(const VitArgs &a, uint32_t *slabs, int *sIncl, int *sState, int *sEndX, int *sEndY) {
    constexpr int kBins = S * S + S * 16;
    static_assert(kBins <= 2 * CPK_WAVE, "a lane keeps two bins");
    const int ri = blockIdx.x, lane = threadIdx.x;
    const CpkVitRegion rg = a.regions[ri];
    const CpkVitOut o = a.out[ri];
    const int nOps = o.endState < 0 ? 0 : o.nOps;  // no path: no counts
    const uint8_t *sx = a.symbols + rg.symX, *sy = a.symbols + rg.symY;
    const int32_t *ops = a.ops + 2 * rg.opBase;
    uint32_t acc0 = 0, acc1 = 0;  // bins lane and lane + 64
    auto add = [&](int bin, int n) {
        if (lane == (bin & (CPK_WAVE - 1))) {
            if (bin < CPK_WAVE) acc0 += (uint32_t)n;
            else acc1 += (uint32_t)n;
        }
    };
    int endX = rg.lX, endY = rg.lY;  // the end cell of the pass's first run
    for (int base = 0; base < nOps; base += CPK_WAVE) {
        const int k = base + lane;
        const bool valid = k < nOps;
        const int st = valid ? ops[2 * k] : 0, len = valid ? ops[2 * k + 1] : 0;
        const int prev = !valid ? 0 : k + 1 < nOps ? ops[2 * (k + 1)] : o.startState;
        const int dx = st == 0 || st == 1 || st == 3 ? len : 0, dy = st == 0 || st == 2 || st == 4 ? len : 0;
        const int incl = vit_scan_inclusive(len, lane), inclX = vit_scan_inclusive(dx, lane), inclY = vit_scan_inclusive(dy, lane);
#pragma unroll
        for (int p = 0; p < S; p++)
#pragma unroll
            for (int s = 0; s < S; s++) add(p * S + s, __popcll(__ballot(valid && prev == p && st == s)));
#pragma unroll
        for (int s = 0; s < S; s++) add(s * S + s, vit_wave_sum(valid && st == s ? len - 1 : 0));
        __syncthreads();  // the pass before has read its runs
        sIncl[lane] = incl;
        sState[lane] = st;
        sEndX[lane] = endX - (inclX - dx);
        sEndY[lane] = endY - (inclY - dy);
        __syncthreads();
        const int T = sIncl[CPK_WAVE - 1];
        for (int t0 = 0; t0 < T; t0 += CPK_WAVE) {
            const bool active = t0 + lane < T;
            const int t = active ? t0 + lane : 0;
            int i = 0;  // the runs that end at or before step t: the index of the run that holds it
#pragma unroll
            for (int half = CPK_WAVE / 2; half > 0; half >>= 1)
                if (sIncl[i + half - 1] <= t) i += half;
            const int s = sState[i], back = sIncl[i] - 1 - t;  // steps between this one and the run's end cell
            int x = sEndX[i] - (s == 0 || s == 1 || s == 3 ? back : 0), y = sEndY[i] - (s == 0 || s == 2 || s == 4 ? back : 0);
            x = x < 0 ? 0 : x > rg.lX ? rg.lX : x;  // ops that are the traceback's never leave the region
            y = y < 0 ? 0 : y > rg.lY ? rg.lY : y;
            const int cX = sx[x], cY = sy[y];  // padded: row and column 0 see N
            const bool emits = active && cX < 4 && cY < 4;
            const int code = emits ? s * 16 + cX * 4 + cY : -1;
#pragma unroll
            for (int q = 0; q < S; q++) {
                if (!__ballot(emits && s == q)) continue;
#pragma unroll
                for (int b = 0; b < 16; b++) add(S * S + q * 16 + b, __popcll(__ballot(code == q * 16 + b)));
            }
        }
        endX -= __shfl(inclX, CPK_WAVE - 1);
        endY -= __shfl(inclY, CPK_WAVE - 1);
    }
    uint32_t *slab = slabs + (int64_t)ri * kBins;
    if (lane < kBins) slab[lane] = acc0;
    if (lane + CPK_WAVE < kBins) slab[lane + CPK_WAVE] = acc1;
}

__global__ void __launch_bounds__(CPK_WAVE) cpecan_viterbi_count(const int nStates, const VitArgs a, uint32_t *slabs) {
    __shared__ int sIncl[CPK_WAVE], sState[CPK_WAVE], sEndX[CPK_WAVE], sEndY[CPK_WAVE];
    if (nStates == 5) vit_count_region<5>(a, slabs, sIncl, sState, sEndX, sEndY);
    else vit_count_region<3>(a, slabs, sIncl, sState, sEndX, sEndY);
}

constexpr int kVitReduceThreads = 256;

__global__ void __launch_bounds__(kVitReduceThreads) cpecan_viterbi_count_reduce(const uint32_t *slabs, const int nRegions, const int nBins,
                                                                                 int64_t *bins) {
    __shared__ int64_t part[kVitReduceThreads];
    const int bin = blockIdx.x, t = threadIdx.x;
    int64_t sum = 0;
    for (int r = t; r < nRegions; r += kVitReduceThreads) sum += slabs[(int64_t)r * nBins + bin];
    part[t] = sum;
    __syncthreads();
    for (int half = kVitReduceThreads / 2; half > 0; half >>= 1) {
        if (t < half) part[t] += part[t + half];
        __syncthreads();
    }
    if (t == 0) bins[bin] += part[0];  // the launches of a run follow one another on the stream
}
