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
