// cpk_dense.inl -- dense forward / backward rows of a region: every state of F and B for every band cell and the total
// the reference passes to its emitter on every diagonal (include/cpecan_dense.h).  Part of the single HIP translation unit
// cpecan_kernels.hip; not compiled on its own.
//
// The fourth result form beside lists, counts and the forward probability, for callers that bring their own per-diagonal
// emitter (inc/pairwiseAligner.h:245-248): the drop-in layer replays such a callback over these rows on the host.  Not a
// variant of the kernel table, and the launch plan does not know it: two plain kernels, nothing resident.
//
//   cpecan_dense_forward   one wave per problem: F of diagonals 0..N, folded as SURVEY 8a rows a6 / a7
//   cpecan_dense_backward  one wave per traceback (tbPrev, dTop, tbFrom): B of diagonals dTop..tbPrev + 1 as the gather of
//                          row a8, and the totals of row a9 on the 1st, 11th, 21st ... emitted diagonal
//
// A neighbour that does not exist (outside the band, beyond the seed diagonal) reads as -inf in every state: logAdd(v, -inf)
// is v to the bit in both builds of logadd, so this IS the reference's "block skipped".  Rows stay in global memory: the
// wave reads back what it wrote a diagonal ago (ld_self) behind a workgroup barrier, as the sweeps' global rolling rows
// do.  Host-bound by nature; no throughput target.

struct DenseArgs {
    const CpkDenseProblem *problems;
    const CpkDenseDiag *diags;
    const CpkDenseSeg *segs;
    const uint8_t *symbols;
    double *F, *B, *side, *totals;
};

constexpr int kDenseEm = 40;  // matchEm[25], gapXEm[5] at 25, gapYEm[5] at 30, padded

__device__ __forceinline__ void dense_stage_model(double *lds, double *em, const CpkModel &m) {
    fill_cubics(lds);
    for (int i = threadIdx.x; i < kDenseEm; i += CPK_WAVE) em[i] = i < 25 ? m.matchEm[i] : i < 30 ? m.gapXEm[i - 25] : i < 35 ? m.gapYEm[i - 30] : 0.0;
    __syncthreads();
}

// Cell x - y = xmy of a diagonal: its index, or -1 where the diagonal (valid = it exists for the caller) does not hold it.
__device__ __forceinline__ int dense_cell_index(const CpkDenseDiag &g, bool valid, int xmy) {
    const int k = (xmy - g.xmyL) >> 1;
    return valid && xmy >= g.xmyL && k < g.width ? k : -1;
}

// The S values of cell k of a row this launch may have written; -inf for k < 0.
template <int S>
__device__ __forceinline__ void dense_load(double (&v)[S], const double *row, int k) {
#pragma unroll
    for (int s = 0; s < S; s++) v[s] = NEG_INF;
    if (k >= 0) {
#pragma unroll
        for (int s = 0; s < S; s++) v[s] = ld_self(row + (int64_t)k * S + s);
    }
}

// The middle block of cellCalculate (impl/stateMachine.c:462-467, :701-704) into `acc`: matches out of every state.
template <int S>
__device__ __forceinline__ double dense_middle(const Cubic *lg, const CpkModel &m, double acc, const double (&mi)[S], double eM) {
    acc = logadd(lg, acc, mi[0] + (eM + m.matchContinue));
    acc = logadd(lg, acc, mi[1] + (eM + m.matchFromShortX));
    acc = logadd(lg, acc, mi[2] + (eM + m.matchFromShortY));
    if constexpr (S == 5) {
        acc = logadd(lg, acc, mi[3] + (eM + m.matchFromLongX));
        acc = logadd(lg, acc, mi[4] + (eM + m.matchFromLongY));
    }
    return acc;
}

// cell_dotProduct, impl/pairwiseAligner.c:402-408
template <int S>
__device__ __forceinline__ double dense_dot(const Cubic *lg, const double (&a)[S], const double (&b)[S]) {
    double t = a[0] + b[0];
#pragma unroll
    for (int s = 1; s < S; s++) t = logadd(lg, t, a[s] + b[s]);
    return t;
}

template <int S>
__device__ __forceinline__ void dense_forward_problem(const CpkModel &m, const DenseArgs &a, const Cubic *lg, const double *em) {
    const CpkDenseProblem pb = a.problems[blockIdx.x];
    const int N = pb.lX + pb.lY, lane = threadIdx.x;
    if (N == 0) return;  // no rows
    const CpkDenseDiag *diags = a.diags + pb.diagOff;
    const uint8_t *sx = a.symbols + pb.symX, *sy = a.symbols + pb.symY;
    double *F = a.F + pb.cellBase * S;
    // diagonal 0: the start prior; B of diagonal 0 and totalUsed[0] are never computed and read NaN
    {
        const CpkDenseDiag g = diags[0];
        double *B = a.B + pb.cellBase * S;
        for (int k = lane; k < g.width; k += CPK_WAVE)
#pragma unroll
            for (int s = 0; s < S; s++) {
                F[(g.cellOff + k) * S + s] = pb.raggedLeft ? m.raggedStart[s] : m.start[s];
                B[(g.cellOff + k) * S + s] = __builtin_nan("");
            }
        if (lane == 0) a.totals[pb.diagOff] = __builtin_nan("");
    }
    __syncthreads();
    CpkDenseDiag g2 = diags[0], g1 = diags[0];  // diagonals d - 2 and d - 1
    for (int d = 1; d <= N; d++) {
        const CpkDenseDiag g = diags[d];
        const double *row1 = F + g1.cellOff * S, *row2 = F + g2.cellOff * S;
        for (int k = lane; k < g.width; k += CPK_WAVE) {
            const int xmy = g.xmyL + 2 * k, x = (d + xmy) >> 1, y = (d - xmy) >> 1;
            const int cX = sx[x], cY = sy[y];
            const double eM = em[cX * 5 + cY], eX = em[25 + cX], eY = em[30 + cY];
            double lo[S], mi[S], up[S], cur[S];
            dense_load<S>(lo, row1, dense_cell_index(g1, true, xmy - 1));
            dense_load<S>(mi, row2, dense_cell_index(g2, d >= 2, xmy));
            dense_load<S>(up, row1, dense_cell_index(g1, true, xmy + 1));
#pragma unroll
            for (int s = 0; s < S; s++) cur[s] = NEG_INF;
            if constexpr (S == 5) {  // impl/stateMachine.c:450-480
                cur[1] = logadd(lg, cur[1], lo[0] + (eX + m.shortOpenX));
                cur[1] = logadd(lg, cur[1], lo[1] + (eX + m.shortExtendX));
                cur[3] = logadd(lg, cur[3], lo[0] + (eX + m.longOpenX));
                cur[3] = logadd(lg, cur[3], lo[3] + (eX + m.longExtendX));
                cur[0] = dense_middle<S>(lg, m, cur[0], mi, eM);
                cur[2] = logadd(lg, cur[2], up[0] + (eY + m.shortOpenY));
                cur[2] = logadd(lg, cur[2], up[2] + (eY + m.shortExtendY));
                cur[4] = logadd(lg, cur[4], up[0] + (eY + m.longOpenY));
                cur[4] = logadd(lg, cur[4], up[4] + (eY + m.longExtendY));
            } else {  // :689-714
                cur[1] = logadd(lg, cur[1], lo[0] + (eX + m.shortOpenX));
                cur[1] = logadd(lg, cur[1], lo[1] + (eX + m.shortExtendX));
                cur[1] = logadd(lg, cur[1], lo[2] + (eX + m.shortSwitchToX));
                cur[0] = dense_middle<S>(lg, m, cur[0], mi, eM);
                cur[2] = logadd(lg, cur[2], up[0] + (eY + m.shortOpenY));
                cur[2] = logadd(lg, cur[2], up[2] + (eY + m.shortExtendY));
                cur[2] = logadd(lg, cur[2], up[1] + (eY + m.shortSwitchToY));
            }
            double *out = F + (g.cellOff + k) * S;
#pragma unroll
            for (int s = 0; s < S; s++) out[s] = cur[s];
        }
        __syncthreads();  // the row is visible to the whole (single-wave) workgroup before the next diagonal reads it
        g2 = g1;
        g1 = g;
    }
}

__global__ void __launch_bounds__(CPK_WAVE) cpecan_dense_forward(const CpkModel m, const DenseArgs a) {
    __shared__ __attribute__((aligned(16))) double lds[kLdsCubics];
    __shared__ double em[kDenseEm];
    dense_stage_model(lds, em, m);
    const Cubic *lg = reinterpret_cast<const Cubic *>(lds);
    if (m.nStates == 5) dense_forward_problem<5>(m, a, lg, em);
    else dense_forward_problem<3>(m, a, lg, em);
}

// diagonalCalculationTotalProbability (impl/pairwiseAligner.c:636-653) on diagonal d: cells ascending, states ascending, one
// sequential fold; then the matches that straddle d.  The per-cell dot products are formed 64 at a time, one per lane; the
// fold over them is every lane's own, in cell order, so the result is wave-uniform and no tree.
template <int S>
__device__ __forceinline__ double dense_fold_cells(const Cubic *lg, double *cbuf, double total, double c, int n) {
    __syncthreads();  // the last pass's readers are done with cbuf
    cbuf[threadIdx.x] = c;
    __syncthreads();
    for (int j = 0; j < n; j++) total = logadd(lg, total, cbuf[j]);
    return total;
}

template <int S>
__device__ __forceinline__ double dense_total(const CpkModel &m, const Cubic *lg, const double *em, double *cbuf, const uint8_t *sx,
                                              const uint8_t *sy, int d, const CpkDenseDiag &g, const double *fRow, const double *bRow,
                                              bool straddles, const CpkDenseDiag &gUp, const double *bUp, const CpkDenseDiag &gDown,
                                              const double *fDown) {
    const int lane = threadIdx.x;
    double total = NEG_INF;
    for (int k0 = 0; k0 < g.width; k0 += CPK_WAVE) {
        const int k = k0 + lane;
        double c = NEG_INF;
        if (k < g.width) {
            double f[S], b[S];
#pragma unroll
            for (int s = 0; s < S; s++) f[s] = fRow[(int64_t)k * S + s];
            dense_load<S>(b, bRow, k);
            c = dense_dot<S>(lg, f, b);
        }
        total = dense_fold_cells<S>(lg, cbuf, total, c, g.width - k0 < CPK_WAVE ? g.width - k0 : CPK_WAVE);
    }
    if (!straddles) return total;
    double straddle = NEG_INF;  // from F[d - 1] into the cells of d + 1, dotted with B[d + 1]
    for (int k0 = 0; k0 < gUp.width; k0 += CPK_WAVE) {
        const int k = k0 + lane;
        double c = NEG_INF;
        if (k < gUp.width) {
            const int xmy = gUp.xmyL + 2 * k, x = (d + 1 + xmy) >> 1, y = (d + 1 - xmy) >> 1;
            const double eM = em[sx[x] * 5 + sy[y]];
            double mi[S], tmp[S], b[S];
            const int kd = dense_cell_index(gDown, true, xmy);
#pragma unroll
            for (int s = 0; s < S; s++) mi[s] = tmp[s] = NEG_INF;
            if (kd >= 0) {
#pragma unroll
                for (int s = 0; s < S; s++) mi[s] = fDown[(int64_t)kd * S + s];
            }
            tmp[0] = dense_middle<S>(lg, m, tmp[0], mi, eM);
            dense_load<S>(b, bUp, k);
            c = dense_dot<S>(lg, tmp, b);
        }
        straddle = dense_fold_cells<S>(lg, cbuf, straddle, c, gUp.width - k0 < CPK_WAVE ? gUp.width - k0 : CPK_WAVE);
    }
    return logadd(lg, total, straddle);
}

template <int S>
__device__ __forceinline__ void dense_backward_segment(const CpkModel &m, const DenseArgs &a, const Cubic *lg, const double *em, double *cbuf) {
    const CpkDenseSeg sg = a.segs[blockIdx.x];
    const CpkDenseProblem pb = a.problems[sg.problem];
    const int N = pb.lX + pb.lY, lane = threadIdx.x;
    const CpkDenseDiag *diags = a.diags + pb.diagOff;
    const uint8_t *sx = a.symbols + pb.symX, *sy = a.symbols + pb.symY;
    const double *F = a.F + pb.cellBase * S;
    double *B = a.B + pb.cellBase * S;
    // rows tbFrom + 1 .. dTop are another traceback's to emit: this one's values of them go to the side array
    const int64_t sideShift = sg.tbFrom < sg.dTop ? sg.sideBase - diags[sg.tbFrom + 1].cellOff : 0;
    double *side = a.side + sideShift * S;
    const bool raggedEnd = sg.dTop == N && pb.raggedRight;
    CpkDenseDiag g1 = diags[sg.dTop], g2 = g1;  // diagonals d + 1 and d + 2
    double *row1 = nullptr, *row2 = nullptr;
    double total = NEG_INF;
    for (int d = sg.dTop; d > sg.tbPrev; d--) {
        const CpkDenseDiag g = diags[d];
        double *row = (d <= sg.tbFrom ? B : side) + g.cellOff * S;
        const bool has1 = d + 1 <= sg.dTop, has2 = d + 2 <= sg.dTop;
        for (int k = lane; k < g.width; k += CPK_WAVE) {
            double cur[S];
            if (d == sg.dTop) {  // the seed: the end prior on every cell (:798-799)
#pragma unroll
                for (int s = 0; s < S; s++) cur[s] = raggedEnd ? m.raggedEnd[s] : m.end[s];
            } else {
                const int xmy = g.xmyL + 2 * k, x = (d + xmy) >> 1, y = (d - xmy) >> 1;
                const int cX1 = sx[x + 1], cY1 = sy[y + 1];  // x <= lX, y <= lY: inside the padded strings
                const double eM = em[cX1 * 5 + cY1], eX = em[25 + cX1], eY = em[30 + cY1];
                double mi[S], up[S], lo[S];
                dense_load<S>(mi, row2, dense_cell_index(g2, has2, xmy));      // (x + 1, y + 1): this cell is its middle
                dense_load<S>(up, row1, dense_cell_index(g1, has1, xmy - 1));  // (x, y + 1): this cell is its upper
                dense_load<S>(lo, row1, dense_cell_index(g1, has1, xmy + 1));  // (x + 1, y): this cell is its lower
#pragma unroll
                for (int s = 0; s < S; s++) cur[s] = NEG_INF;
                cur[0] = logadd(lg, cur[0], mi[0] + (eM + m.matchContinue));
                cur[1] = logadd(lg, cur[1], mi[0] + (eM + m.matchFromShortX));
                cur[2] = logadd(lg, cur[2], mi[0] + (eM + m.matchFromShortY));
                if constexpr (S == 5) {
                    cur[3] = logadd(lg, cur[3], mi[0] + (eM + m.matchFromLongX));
                    cur[4] = logadd(lg, cur[4], mi[0] + (eM + m.matchFromLongY));
                    cur[0] = logadd(lg, cur[0], up[2] + (eY + m.shortOpenY));
                    cur[2] = logadd(lg, cur[2], up[2] + (eY + m.shortExtendY));
                    cur[0] = logadd(lg, cur[0], up[4] + (eY + m.longOpenY));
                    cur[4] = logadd(lg, cur[4], up[4] + (eY + m.longExtendY));
                    cur[0] = logadd(lg, cur[0], lo[1] + (eX + m.shortOpenX));
                    cur[1] = logadd(lg, cur[1], lo[1] + (eX + m.shortExtendX));
                    cur[0] = logadd(lg, cur[0], lo[3] + (eX + m.longOpenX));
                    cur[3] = logadd(lg, cur[3], lo[3] + (eX + m.longExtendX));
                } else {
                    cur[0] = logadd(lg, cur[0], up[2] + (eY + m.shortOpenY));
                    cur[2] = logadd(lg, cur[2], up[2] + (eY + m.shortExtendY));
                    cur[1] = logadd(lg, cur[1], up[2] + (eY + m.shortSwitchToY));
                    cur[0] = logadd(lg, cur[0], lo[1] + (eX + m.shortOpenX));
                    cur[1] = logadd(lg, cur[1], lo[1] + (eX + m.shortExtendX));
                    cur[2] = logadd(lg, cur[2], lo[1] + (eX + m.shortSwitchToX));
                }
            }
            double *out = row + (int64_t)k * S;
#pragma unroll
            for (int s = 0; s < S; s++) out[s] = cur[s];
        }
        __syncthreads();
        if (d <= sg.tbFrom) {
            if ((sg.tbFrom - d) % CPK_REFRESH_PERIOD == 0)  // the 1st, 11th, 21st ... emitted diagonal (:830)
                total = dense_total<S>(m, lg, em, cbuf, sx, sy, d, g, F + g.cellOff * S, row, has1, g1, row1, diags[d - 1],
                                       F + diags[d - 1].cellOff * S);
            if (lane == 0) a.totals[pb.diagOff + d] = total;
        }
        g2 = g1;
        g1 = g;
        row2 = row1;
        row1 = row;
    }
}

__global__ void __launch_bounds__(CPK_WAVE) cpecan_dense_backward(const CpkModel m, const DenseArgs a) {
    __shared__ __attribute__((aligned(16))) double lds[kLdsCubics];
    __shared__ double em[kDenseEm];
    __shared__ double cbuf[CPK_WAVE];
    dense_stage_model(lds, em, m);
    const Cubic *lg = reinterpret_cast<const Cubic *>(lds);
    if (m.nStates == 5) dense_backward_segment<5>(m, a, lg, em, cbuf);
    else dense_backward_segment<3>(m, a, lg, em, cbuf);
}
