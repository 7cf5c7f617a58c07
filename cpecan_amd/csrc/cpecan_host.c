/*
 * cpecan_host.c -- host side (plain C99) of libcpecan_hip.so.
 *
 * Everything that is integer bookkeeping in the reference stays on the host, in C, as the north star asks:
 * the band (impl/pairwiseAligner.c:94-234), the split into regions (:1206-1326), the traceback schedule
 * (:791-810), packing of problems into flat arrays for the GPU and re-assembly of the returned triples into
 * the reference's list order (:1411-1418).  All floating-point DP work happens in cpecan_kernels.hip; there is
 * no CPU implementation of it in this library.
 */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <omp.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"
#include "cpecan_realign.h" /* cpecan_batch_set_next_runs / cpecan_batch_next_runs / cpecan_next_runs_of_pairs */
#include "cpecan_sets.h" /* cpecan_batch_set_quintuples / cpecan_batch_quintuples */
#include "cpecan_band.inl"

/* ------------------------------------------------------------------------------------------------
 * models: impl/stateMachine.c
 * ---------------------------------------------------------------------------------------------- */
enum { kMatch = 0, kShortX = 1, kShortY = 2, kLongX = 3, kLongY = 4 }; /* stateMachine.c:261-263 */

static int is_five(int32_t type) { return type == CPECAN_FIVE_STATE || type == CPECAN_FIVE_STATE_ASYM; }
static int is_three(int32_t type) { return type == CPECAN_THREE_STATE || type == CPECAN_THREE_STATE_ASYM; }

int cpecan_model_default(cpecan_model *m, int32_t type) {
    if (!m || !(is_five(type) || is_three(type))) return CPECAN_EINVAL;
    memset(m, 0, sizeof *m);
    m->type = type;
    /* emissions: stateMachine.c:269-292 */
    const double eMatch = -2.1149196655034745, eTransversion = -4.5691014376830479, eTransition = -3.9833860032220842;
    for (int x = 0; x < 4; x++) {
        for (int y = 0; y < 4; y++) {
            m->emissionMatch[x * 4 + y] = x == y ? eMatch : (((x ^ y) == 2) ? eTransition : eTransversion);
        }
        m->emissionGapX[x] = m->emissionGapY[x] = -1.6094379124341003;
    }
    m->matchContinue = -0.030064059121770816;
    m->matchFromShortGapX = m->matchFromShortGapY = -1.272871422049609;
    m->gapShortExtendX = m->gapShortExtendY = -0.3388262689231553;
    m->gapShortSwitchToX = m->gapShortSwitchToY = -4.910694825551255;
    if (is_five(type)) { /* stateMachine.c:484-501 */
        m->matchFromLongGapX = m->matchFromLongGapY = -5.673280173170473;
        m->gapShortOpenX = m->gapShortOpenY = -4.34381910900448;
        m->gapLongOpenX = m->gapLongOpenY = -6.30810595366929;
        m->gapLongExtendX = m->gapLongExtendY = -0.003442492794189331;
        m->gapLongSwitchToX = m->gapLongSwitchToY = -6.30810595366929;
    } else { /* stateMachine.c:718-726 */
        m->gapShortOpenX = m->gapShortOpenY = -4.21256642;
    }
    return CPECAN_OK;
}

int cpecan_hmm_init(cpecan_hmm *h, int32_t type, double pseudo) { /* stateMachine.c:23-48 */
    if (!h || !(is_five(type) || is_three(type))) return CPECAN_EINVAL;
    h->type = type;
    h->stateNumber = is_five(type) ? 5 : 3;
    for (int i = 0; i < 25; i++) h->transitions[i] = pseudo;
    for (int i = 0; i < 80; i++) h->emissions[i] = pseudo;
    h->likelihood = 0.0;
    return CPECAN_OK;
}

int cpecan_hmm_normalise(cpecan_hmm *h) { /* stateMachine.c:88-112 */
    if (!h) return CPECAN_EINVAL;
    const int S = h->stateNumber;
    for (int from = 0; from < S; from++) {
        double sum = 0.0;
        for (int to = 0; to < S; to++) sum += h->transitions[from * S + to];
        for (int to = 0; to < S; to++) h->transitions[from * S + to] /= sum;
    }
    for (int s = 0; s < S; s++) {
        double sum = 0.0;
        for (int i = 0; i < 16; i++) sum += h->emissions[s * 16 + i];
        for (int i = 0; i < 16; i++) h->emissions[s * 16 + i] /= sum;
    }
    return CPECAN_OK;
}

int cpecan_hmm_write(const cpecan_hmm *h, const char *path) { /* stateMachine.c:133-143 */
    if (!h || !path) return CPECAN_EINVAL;
    FILE *f = fopen(path, "w");
    if (!f) return CPECAN_EINVAL;
    const int S = h->stateNumber;
    fprintf(f, "%i\t", h->type);
    for (int i = 0; i < S * S; i++) fprintf(f, "%f\t", h->transitions[i]);
    fprintf(f, "%f\n", h->likelihood);
    for (int i = 0; i < S * 16; i++) fprintf(f, "%f\t", h->emissions[i]);
    fprintf(f, "\n");
    fclose(f);
    return CPECAN_OK;
}

int cpecan_hmm_load(cpecan_hmm *h, const char *path) { /* stateMachine.c:145-202 */
    if (!h || !path) return CPECAN_EINVAL;
    FILE *f = fopen(path, "r");
    if (!f) return CPECAN_EINVAL;
    int type = -1, rc = CPECAN_EINVAL;
    if (fscanf(f, "%i", &type) == 1 && cpecan_hmm_init(h, type, 0.0) == CPECAN_OK) {
        const int S = h->stateNumber;
        int ok = 1;
        for (int i = 0; i < S * S && ok; i++) ok = fscanf(f, "%lf", &h->transitions[i]) == 1;
        ok = ok && fscanf(f, "%lf", &h->likelihood) == 1;
        for (int i = 0; i < S * 16 && ok; i++) ok = fscanf(f, "%lf", &h->emissions[i]) == 1;
        if (ok) rc = CPECAN_OK;
    }
    fclose(f);
    return rc;
}

static double tr(const cpecan_hmm *h, int from, int to) { return h->transitions[from * h->stateNumber + to]; }
static double emi(const cpecan_hmm *h, int s, int x, int y) { return h->emissions[s * 16 + x * 4 + y]; }

/* emissions_loadGapProbs, stateMachine.c:327-349: collapse gap-state emission matrices onto one sequence */
static void gap_emissions(const cpecan_hmm *h, double *out, const int *xs, int nx, const int *ys, int ny) {
    double acc[4] = {0, 0, 0, 0}, sum = 0.0;
    for (int i = 0; i < nx; i++)
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++) acc[x] += emi(h, xs[i], x, y);
    for (int i = 0; i < ny; i++)
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++) acc[y] += emi(h, ys[i], x, y);
    for (int i = 0; i < 4; i++) sum += acc[i];
    for (int i = 0; i < 4; i++) out[i] = log(acc[i] / sum);
}

static void exchange(double *a, double *b) {
    double t = *a;
    *a = *b;
    *b = t;
}

/* keep "long" the state with the larger extend probability, stateMachine.c:544-550 */
static void order_short_long(double *extS, double *extL, double *fromS, double *fromL, double *openS, double *openL,
                             double *swS, double *swL) {
    if (*extS > *extL) {
        exchange(extS, extL);
        exchange(fromS, fromL);
        exchange(openS, openL);
        exchange(swS, swL);
    }
}

int cpecan_model_from_hmm(cpecan_model *m, const cpecan_hmm *h) { /* stateMachine.c:529-620, 747-819 */
    if (!m || !h) return CPECAN_EINVAL;
    if (cpecan_model_default(m, h->type) != CPECAN_OK) return CPECAN_EINVAL;
    const int sym = (h->type == CPECAN_FIVE_STATE || h->type == CPECAN_THREE_STATE);
    const int xs5[2] = {kShortX, kLongX}, ys5[2] = {kShortY, kLongY}, xs3[1] = {kShortX}, ys3[1] = {kShortY};
    m->matchContinue = log(tr(h, kMatch, kMatch));
    /* match emissions: stateMachine.c:298-317 */
    for (int x = 0; x < 4; x++) {
        for (int y = 0; y < 4; y++) {
            m->emissionMatch[x * 4 + y] =
                (!sym || x == y) ? log(emi(h, kMatch, x, y)) : log((emi(h, kMatch, x < y ? x : y, x < y ? y : x) +
                                                                    emi(h, kMatch, x < y ? y : x, x < y ? x : y)) / 2.0);
        }
    }
    if (h->type == CPECAN_FIVE_STATE) {
        m->matchFromShortGapX = log((tr(h, kShortX, kMatch) + tr(h, kShortY, kMatch)) / 2);
        m->matchFromLongGapX = log((tr(h, kLongX, kMatch) + tr(h, kLongY, kMatch)) / 2);
        m->gapShortOpenX = log((tr(h, kMatch, kShortX) + tr(h, kMatch, kShortY)) / 2);
        m->gapShortExtendX = log((tr(h, kShortX, kShortX) + tr(h, kShortY, kShortY)) / 2);
        m->gapShortSwitchToX = log((tr(h, kShortX, kShortY) + tr(h, kShortY, kShortX)) / 2);
        m->gapLongOpenX = log((tr(h, kMatch, kLongX) + tr(h, kMatch, kLongY)) / 2);
        m->gapLongExtendX = log((tr(h, kLongX, kLongX) + tr(h, kLongY, kLongY)) / 2);
        m->gapLongSwitchToX = log((tr(h, kLongX, kLongY) + tr(h, kLongY, kLongX)) / 2);
        order_short_long(&m->gapShortExtendX, &m->gapLongExtendX, &m->matchFromShortGapX, &m->matchFromLongGapX,
                         &m->gapShortOpenX, &m->gapLongOpenX, &m->gapShortSwitchToX, &m->gapLongSwitchToX);
        m->matchFromShortGapY = m->matchFromShortGapX;
        m->matchFromLongGapY = m->matchFromLongGapX;
        m->gapShortOpenY = m->gapShortOpenX;
        m->gapShortExtendY = m->gapShortExtendX;
        m->gapShortSwitchToY = m->gapShortSwitchToX;
        m->gapLongOpenY = m->gapLongOpenX;
        m->gapLongExtendY = m->gapLongExtendX;
        m->gapLongSwitchToY = m->gapLongSwitchToX;
        gap_emissions(h, m->emissionGapX, xs5, 2, ys5, 2);
        gap_emissions(h, m->emissionGapY, xs5, 2, ys5, 2);
    } else if (h->type == CPECAN_FIVE_STATE_ASYM) {
        m->matchFromShortGapX = log(tr(h, kShortX, kMatch));
        m->matchFromLongGapX = log(tr(h, kLongX, kMatch));
        m->gapShortOpenX = log(tr(h, kMatch, kShortX));
        m->gapShortExtendX = log(tr(h, kShortX, kShortX));
        m->gapShortSwitchToX = log(tr(h, kShortY, kShortX));
        m->gapLongOpenX = log(tr(h, kMatch, kLongX));
        m->gapLongExtendX = log(tr(h, kLongX, kLongX));
        m->gapLongSwitchToX = log(tr(h, kLongY, kLongX));
        order_short_long(&m->gapShortExtendX, &m->gapLongExtendX, &m->matchFromShortGapX, &m->matchFromLongGapX,
                         &m->gapShortOpenX, &m->gapLongOpenX, &m->gapShortSwitchToX, &m->gapLongSwitchToX);
        m->matchFromShortGapY = log(tr(h, kShortY, kMatch));
        m->matchFromLongGapY = log(tr(h, kLongY, kMatch));
        m->gapShortOpenY = log(tr(h, kMatch, kShortY));
        m->gapShortExtendY = log(tr(h, kShortY, kShortY));
        m->gapShortSwitchToY = log(tr(h, kShortX, kShortY));
        m->gapLongOpenY = log(tr(h, kMatch, kLongY));
        m->gapLongExtendY = log(tr(h, kLongY, kLongY));
        m->gapLongSwitchToY = log(tr(h, kLongX, kLongY));
        order_short_long(&m->gapShortExtendY, &m->gapLongExtendY, &m->matchFromShortGapY, &m->matchFromLongGapY,
                         &m->gapShortOpenY, &m->gapLongOpenY, &m->gapShortSwitchToY, &m->gapLongSwitchToY);
        gap_emissions(h, m->emissionGapX, xs5, 2, NULL, 0);
        gap_emissions(h, m->emissionGapY, NULL, 0, ys5, 2);
    } else if (h->type == CPECAN_THREE_STATE) {
        m->matchFromShortGapX = m->matchFromShortGapY = log((tr(h, kShortX, kMatch) + tr(h, kShortY, kMatch)) / 2.0);
        m->gapShortOpenX = m->gapShortOpenY = log((tr(h, kMatch, kShortX) + tr(h, kMatch, kShortY)) / 2.0);
        m->gapShortExtendX = m->gapShortExtendY = log((tr(h, kShortX, kShortX) + tr(h, kShortY, kShortY)) / 2.0);
        m->gapShortSwitchToX = m->gapShortSwitchToY = log((tr(h, kShortY, kShortX) + tr(h, kShortX, kShortY)) / 2.0);
        gap_emissions(h, m->emissionGapX, xs3, 1, ys3, 1);
        gap_emissions(h, m->emissionGapY, xs3, 1, ys3, 1);
    } else {
        m->matchFromShortGapX = log(tr(h, kShortX, kMatch));
        m->matchFromShortGapY = log(tr(h, kShortY, kMatch));
        m->gapShortOpenX = log(tr(h, kMatch, kShortX));
        m->gapShortOpenY = log(tr(h, kMatch, kShortY));
        m->gapShortExtendX = log(tr(h, kShortX, kShortX));
        m->gapShortExtendY = log(tr(h, kShortY, kShortY));
        m->gapShortSwitchToX = log(tr(h, kShortY, kShortX));
        m->gapShortSwitchToY = log(tr(h, kShortX, kShortY));
        gap_emissions(h, m->emissionGapX, xs3, 1, NULL, 0);
        gap_emissions(h, m->emissionGapY, NULL, 0, ys3, 1);
    }
    return CPECAN_OK;
}

int cpecan_params_default(cpecan_params *p) { /* pairwiseAligner.c:1334-1348 */
    if (!p) return CPECAN_EINVAL;
    memset(p, 0, sizeof *p);
    p->threshold = 0.01;
    p->minDiagsBetweenTraceBack = 1000;
    p->traceBackDiagonals = 40;
    p->diagonalExpansion = 20;
    p->splitMatrixBiggerThanThis = (int64_t)3000 * 3000;
    p->dynamicAnchorExpansion = 0;
    return CPECAN_OK;
}

/* Kernel-side view of the model: priors (stateMachine.c:401-448, 648-687) and N-padded emissions (:351-366). */
static void kernel_model(const cpecan_model *m, double threshold, CpkModel *k) {
    const double ninf = -INFINITY;
    memset(k, 0, sizeof *k);
    k->type = m->type;
    k->nStates = is_five(m->type) ? 5 : 3;
    k->threshold = threshold;
    for (int s = 0; s < CPK_MAX_STATES; s++) k->start[s] = k->raggedStart[s] = k->end[s] = k->raggedEnd[s] = ninf;
    k->start[kMatch] = 0.0;
    k->end[kMatch] = m->matchContinue;
    k->end[kShortX] = m->matchFromShortGapX;
    k->end[kShortY] = m->matchFromShortGapY;
    if (k->nStates == 5) {
        k->raggedStart[kLongX] = k->raggedStart[kLongY] = 0.0;
        k->end[kLongX] = m->matchFromLongGapX;
        k->end[kLongY] = m->matchFromLongGapY;
        k->raggedEnd[kMatch] = m->gapLongOpenX;
        k->raggedEnd[kShortX] = m->gapLongOpenX;
        k->raggedEnd[kShortY] = m->gapLongOpenY;
        k->raggedEnd[kLongX] = m->gapLongExtendX;
        k->raggedEnd[kLongY] = m->gapLongExtendY;
    } else {
        k->raggedStart[kShortX] = k->raggedStart[kShortY] = 0.0;
        k->raggedEnd[kMatch] = (m->gapShortOpenX + m->gapShortOpenY) / 2.0;
        k->raggedEnd[kShortX] = m->gapShortExtendX;
        k->raggedEnd[kShortY] = m->gapShortExtendY;
    }
    k->matchContinue = m->matchContinue;
    k->matchFromShortX = m->matchFromShortGapX;
    k->matchFromShortY = m->matchFromShortGapY;
    k->matchFromLongX = m->matchFromLongGapX;
    k->matchFromLongY = m->matchFromLongGapY;
    k->shortOpenX = m->gapShortOpenX;
    k->shortOpenY = m->gapShortOpenY;
    k->shortExtendX = m->gapShortExtendX;
    k->shortExtendY = m->gapShortExtendY;
    k->shortSwitchToX = m->gapShortSwitchToX;
    k->shortSwitchToY = m->gapShortSwitchToY;
    k->longOpenX = m->gapLongOpenX;
    k->longOpenY = m->gapLongOpenY;
    k->longExtendX = m->gapLongExtendX;
    k->longExtendY = m->gapLongExtendY;
    for (int x = 0; x < 5; x++) {
        k->gapXEm[x] = x == CPK_SYM_N ? -1.386294361 : m->emissionGapX[x];
        k->gapYEm[x] = x == CPK_SYM_N ? -1.386294361 : m->emissionGapY[x];
        for (int y = 0; y < 5; y++)
            k->matchEm[x * 5 + y] = (x == CPK_SYM_N || y == CPK_SYM_N) ? -2.772588722 : m->emissionMatch[x * 4 + y];
    }
}
void cpk_kernel_model(const cpecan_model *m, double threshold, CpkModel *k) { kernel_model(m, threshold, k); } /* cpecan_dense.c */

/* ------------------------------------------------------------------------------------------------
 * band and split geometry (integers only)
 * ---------------------------------------------------------------------------------------------- */
/* CPECAN_TRACE_HOST=1: wall time of the host stages of upload and download on stderr (diagnostic) */
static double now_ms(void) { return 1e3 * omp_get_wtime(); }
static int trace_host(void) {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("CPECAN_TRACE_HOST");
        v = e && atoi(e) != 0;
    }
    return v;
}
static int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
static int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

/* band_construct / band_constructDynamic (pairwiseAligner.c:128-234) through the shared iterator (cpecan_band.inl). */
int cpecan_band(const int64_t *anchors, int64_t nAnchors, int64_t lX, int64_t lY, int64_t expansion, int dynamic,
                int64_t *out) {
    const int64_t n = lX + lY + 1;
    if (n <= 0 || !out || nAnchors < 0) return CPECAN_EINVAL;
    if (nAnchors > 0 && !anchors) return CPECAN_EINVAL;
    int32_t *a32 = malloc(sizeof(int32_t) * 3 * (size_t)(nAnchors ? nAnchors : 1)); /* the iterator reads 32-bit values */
    if (!a32) return CPECAN_ENOMEM;
    int rc = CPECAN_OK;
    for (int64_t i = 0; i < 3 * nAnchors; i++) {
        if (anchors[i] < INT32_MIN || anchors[i] > INT32_MAX) rc = CPECAN_EINVAL;
        a32[i] = (int32_t)anchors[i];
    }
    CpkBandIter it;
    if (rc == CPECAN_OK && cpk_band_init(&it, a32, 3, nAnchors, lX, lY, expansion, dynamic)) rc = CPECAN_EINVAL;
    for (int64_t d = 0; rc == CPECAN_OK && d < n; d++) {
        int64_t lo, hi;
        if (cpk_band_next(&it, d, &lo, &hi)) {
            rc = CPECAN_EINVAL;
            break;
        }
        out[3 * d] = d;
        out[3 * d + 1] = lo;
        out[3 * d + 2] = hi;
    }
    free(a32);
    return rc;
}

/* One anchor entry of an add call, whichever form the call came in: (x, y, length, expansion); a triple is a run of one.
 * The cursor walks a problem's entries in order. */
typedef struct {
    int64_t x, y, len, expansion;
} AnchorEntry;
typedef struct {
    const int64_t *at, *end;
    int runs; /* quadruples (x, y, length, expansion); 0: triples (x, y, expansion) */
} AnchorCursor;
static inline int next_entry(AnchorCursor *c, AnchorEntry *e) {
    const int64_t *a = c->at;
    if (a == c->end) return 0;
    *e = c->runs ? (AnchorEntry){a[0], a[1], a[2], a[3]} : (AnchorEntry){a[0], a[1], 1, a[2]};
    c->at = a + (c->runs ? 4 : 3);
    return 1;
}
/* Anchors go to a problem's split rectangles in order (pairwiseAligner.c:1296-1308): the entries whose first diagonal x + y
 * lies below diagEnd = x2 + y2 of the rectangle belong to it -- a rectangle ends inside a gap, never inside a run.  The next
 * entry into *e if it belongs to the rectangle.  (The cursor is a local of the loop that uses it: this runs once per anchor of
 * the batch, beside stores through pointers that could alias anything longer-lived.) */
static inline int next_in_rect(AnchorCursor *c, int64_t diagEnd, AnchorEntry *e) {
    return c->at != c->end && c->at[0] + c->at[1] < diagEnd && next_entry(c, e);
}

/* getSplitPoints, pairwiseAligner.c:1206-1257.  A gap between consecutive anchors whose matrix exceeds
 * maxMatrixSize closes the current rectangle half-way into the gap (at most sqrt(max) deep) and opens the
 * next one the same distance before the following anchor. */
typedef struct {
    int64_t x1, y1; /* start of the rectangle being grown */
    int64_t *out;
    int64_t count;
    int64_t limit, depth;
} SplitState;

static int cut_if_large(SplitState *s, int64_t fromX, int64_t fromY, int64_t toX, int64_t toY, int suppress) {
    const int64_t gx = toX - fromX, gy = toY - fromY;
    if (gx * gy <= s->limit) return 0;
    const int64_t hx = imin(gx / 2, s->depth), hy = imin(gy / 2, s->depth);
    if (!suppress) {
        int64_t *r = s->out + 4 * s->count++;
        r[0] = s->x1;
        r[1] = s->y1;
        r[2] = fromX + hx;
        r[3] = fromY + hy;
    }
    s->x1 = toX - hx;
    s->y1 = toY - hy;
    return 1;
}

/* Between two anchors of a run the gap is empty (0 x 0 cells), so only the gaps in front of an entry and behind the last one
 * can be cut: runs give the same rectangles as their anchors one by one. */
static int64_t split_points_entries(AnchorCursor cur, int64_t lX, int64_t lY, int64_t maxMatrixSize, int raggedLeft, int raggedRight,
                                    int64_t *out) {
    SplitState s = {0, 0, out, 0, maxMatrixSize, (int64_t)sqrt((double)maxMatrixSize)};
    const int none = cur.at == cur.end;
    int64_t fromX = 0, fromY = 0;
    AnchorEntry e;
    for (int first = 1; next_entry(&cur, &e); first = 0) {
        if (e.x < fromX || e.y < fromY || e.len < 1 || e.x + e.len > lX || e.y + e.len > lY) return CPECAN_EINVAL; /* :1240-1243 */
        cut_if_large(&s, fromX, fromY, e.x, e.y, raggedLeft && first);
        fromX = e.x + e.len;
        fromY = e.y + e.len;
    }
    const int cutAtEnd = cut_if_large(&s, fromX, fromY, lX, lY, raggedLeft && none);
    if (!cutAtEnd || !raggedRight) {
        int64_t *r = out + 4 * s.count++;
        r[0] = s.x1;
        r[1] = s.y1;
        r[2] = lX;
        r[3] = lY;
    }
    return s.count;
}

int64_t cpecan_split_points(const int64_t *anchors, int64_t nAnchors, int64_t lX, int64_t lY, int64_t maxMatrixSize,
                            int raggedLeft, int raggedRight, int64_t *out) {
    if (lX < 0 || lY < 0 || nAnchors < 0 || !out) return CPECAN_EINVAL;
    return split_points_entries((AnchorCursor){anchors, anchors + 3 * nAnchors, 0}, lX, lY, maxMatrixSize, raggedLeft, raggedRight, out);
}

/* ------------------------------------------------------------------------------------------------
 * the batch object
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t problem;   /* owning problem */
    int64_t x1, y1;    /* offset of the region inside the problem (coordinate correction, :1411-1418) */
    int64_t lX, lY;
    int64_t seqXOff, seqYOff; /* into the symbol blob */
    int64_t anchorOff, nAnchors;
    int64_t runOff, nRuns; /* its runs in cpecan_batch.runs (a batch that keeps its anchors as runs) */
    int raggedLeft, raggedRight;
    /* filled by upload */
    int64_t cells;
    int64_t devIndex; /* position in the cost-sorted device array */
} HostRegion;

typedef struct {
    int64_t firstRegion, nRegions;
    int32_t *triples[4]; /* lists 0..2 into cpecan_batch.results, list 3 (MEA alignment) into postMea/postShift; not owned */
    int64_t nTriples[4];
    int64_t lX, lY;          /* of the whole problem */
    int64_t charX, charY;    /* raw upper-case sequences in cpecan_batch.chars */
    int32_t minus;           /* Y was added reverse-complemented (cpecan_batch_add_many_runs_stranded) */
    double scores[CPK_POST_SCORES]; /* byPosterior, byPosteriorIgnoringGaps, MEA alignment score, byIdentity, ...IgnoringGaps */
} HostProblem;

struct cpecan_batch {
    cpecan_model model;
    cpecan_params params;
    int emit, device, debug;
    int frozen, ran, downloaded;
    HostProblem *problems;
    int64_t nProblems, capProblems;
    HostRegion *regions;
    int64_t nRegions, capRegions;
    uint8_t *symbols;
    int64_t nSymbols, capSymbols;
    int32_t *anchors; /* cpk_anchor_t: anchorStride values per anchor, coordinates relative to the region */
    int anchorStride; /* 2: (x, y); 3: (x, y, expansion) for per-anchor expansions */
    int64_t nAnchorVals, capAnchorVals;
    /* Round 4: a batch of fixed expansion whose first problems arrive as runs (cpecan_batch_add_many_runs) KEEPS them as runs
     * -- (x, y, length, index of the run's first anchor among the batch's anchors) -- and never holds one anchor per column
     * on the host: planning walks the runs (cpk_band_init_runs) and the device expands them in front of its table builder.
     * BASELINE config 4: 6e7 anchors, 0.5 GB written by every add and read again by every band walk.  runForm: -1 not
     * decided yet, 0 anchors, 1 runs.  nAnchorVals still counts the expanded anchors. */
    int32_t *runs;
    int64_t nRunVals, capRunVals;
    int runForm;
    /* frozen state */
    CpkRegion *devRegions; /* cost-sorted */
    int64_t *devToHost;    /* devRegions[i] describes regions[devToHost[i]] */
    CpkSegment *segs;
    int64_t nSegs;
    int64_t nDiags;
    CpkGeometry geo;
    int64_t outTriples; /* per list */
    int nLists;
    int64_t dbgCells, dbgDiags;
    CpkDevice *dev;
    double *forward; /* [slot][nRegions] in device order, FORWARD emitter; [slot][106] sums, EXPECT emitter */
    int modelSlots;  /* cpecan_batch_reserve_models: models reserved per run; 0: a plain batch */
    int activeModels, downloadedModels; /* models of the next run / of the downloaded one */
    int32_t *results; /* every emitted triple of the batch, list-ordered: [list][problem][triple] */
    uint8_t *chars;   /* raw upper-case sequences (leftShiftAlignment compares letters, not symbols) */
    int64_t nChars, capChars;
    int postFlags;    /* CPECAN_POST_* applied by download */
    double postGapGamma;
    float postMatchGamma; /* ORDERED: matchGamma of cPecanRealign.c:355 */
    int32_t *postMea, *postShift;
    int bandEdge;            /* cpecan_batch_set_band_edge: downloads also compute the statistic */
    cpecan_band_edge *edges; /* [nProblems] of the downloaded run, or NULL: it was not asked for */
    /* cpecan_batch_set_quintuples (include/cpecan_sets.h): the two names of every problem, or NULL: the stage is off */
    int32_t *quintNames;
    int32_t *quints;                 /* the downloaded run's records (host pool), its nProblems + 1 offsets and nProblems sums */
    int64_t *quintOffsets, *quintSums;
    double quintStageMs;
    /* cpecan_batch_set_next_runs (include/cpecan_realign.h): the ordered alignment leaves the device as anchor runs */
    int nextRuns;
    int64_t nextTrim, nextExpansion;
    int64_t *nextRunVals;    /* the downloaded run's quadruples (x, y, length, expansion), problem i at 4 * nextRunOffsets[i] */
    int64_t *nextRunOffsets; /* [nProblems + 1], or NULL: the downloaded run was not asked for them */
    double nextStageMs;
    cpecan_stats stats;
    /* cpecan_batch_download_begin / _end */
    pthread_t dlThread;
    int dlActive, dlResult;
    char dlError[256]; /* the helper's error text: cpk_last_error is per thread */
};

/* The batch's arrays live in blocks of the host pool (cpk_host_alloc: pinned and recycled when there is a GPU). */
static int grow(void **p, int64_t *cap, int64_t need, size_t elem) {
    if (need <= *cap) return 0;
    int64_t c = *cap ? *cap : 16;
    while (c < need) c *= 2;
    void *q = cpk_host_grow(*p, (size_t)*cap * elem, (size_t)c * elem);
    if (!q) return -1;
    *p = q;
    *cap = c;
    return 0;
}
static void *host_zalloc(size_t count, size_t elem) {
    void *q = cpk_host_alloc((count ? count : 1) * elem);
    if (q) memset(q, 0, (count ? count : 1) * elem);
    return q;
}

int64_t cpecan_anchors_from_alignment(const int64_t *ops, int64_t nOps, int64_t start1, int64_t start2, int64_t trim,
                                      int64_t expansion, const char *sX, int64_t lX, const char *sY, int64_t lY,
                                      int64_t *anchors) {
    if (nOps < 0 || (nOps > 0 && !ops) || !anchors || trim < 0) return CPECAN_EINVAL;
    const int filter = sX && sY;
    int64_t x = start1, y = start2, n = 0;
    for (int64_t i = 0; i < nOps; i++) {
        const int64_t type = ops[2 * i], len = ops[2 * i + 1];
        if (len < 0 || type < CPECAN_OP_MATCH || type > CPECAN_OP_INDEL_Y) return CPECAN_EINVAL;
        if (type == CPECAN_OP_MATCH) {
            for (int64_t l = trim; l < len - trim; l++) { /* :987-989 */
                const int64_t ax = x + l, ay = y + l;
                if (filter) {
                    if (ax < 0 || ay < 0 || ax >= lX || ay >= lY) return CPECAN_EINVAL;
                    int cx = (unsigned char)sX[ax], cy = (unsigned char)sY[ay]; /* toupper, "C" locale */
                    cx -= (cx >= 'a' && cx <= 'z') ? 'a' - 'A' : 0;
                    cy -= (cy >= 'a' && cy <= 'z') ? 'a' - 'A' : 0;
                    if (cx != cy || cx == 'N') continue; /* cPecanRealign.c:277-281 */
                }
                anchors[3 * n] = ax;
                anchors[3 * n + 1] = ay;
                anchors[3 * n + 2] = expansion;
                n++;
            }
        }
        if (type != CPECAN_OP_INDEL_Y) x += len; /* :991-996 */
        if (type != CPECAN_OP_INDEL_X) y += len;
    }
    return n;
}

/* The same anchors as runs (cpecan_batch_add_many_runs): the kept columns of a match operation that follow each other
 * on a matrix diagonal -- a mismatched column or the end of the operation ends a run -- as (x, y, length, expansion). */
int64_t cpecan_anchor_runs_from_alignment(const int64_t *ops, int64_t nOps, int64_t start1, int64_t start2, int64_t trim,
                                          int64_t expansion, const char *sX, int64_t lX, const char *sY, int64_t lY,
                                          int64_t *runs, int64_t cap) {
    if (nOps < 0 || (nOps > 0 && !ops) || trim < 0 || cap < 0 || (cap > 0 && !runs)) return CPECAN_EINVAL;
    const int filter = sX && sY;
    int64_t x = start1, y = start2, n = 0, rx = 0, ry = 0, len = 0; /* the open run: (rx, ry) .. len columns, len == 0: none */
    for (int64_t i = 0; i < nOps; i++) {
        const int64_t type = ops[2 * i], opLen = ops[2 * i + 1];
        if (opLen < 0 || type < CPECAN_OP_MATCH || type > CPECAN_OP_INDEL_Y) return CPECAN_EINVAL;
        if (type == CPECAN_OP_MATCH) {
            for (int64_t l = trim; l < opLen - trim; l++) {
                const int64_t ax = x + l, ay = y + l;
                if (filter) {
                    if (ax < 0 || ay < 0 || ax >= lX || ay >= lY) return CPECAN_EINVAL;
                    int cx = (unsigned char)sX[ax], cy = (unsigned char)sY[ay];
                    cx -= (cx >= 'a' && cx <= 'z') ? 'a' - 'A' : 0;
                    cy -= (cy >= 'a' && cy <= 'z') ? 'a' - 'A' : 0;
                    if (cx != cy || cx == 'N') continue;
                }
                if (len > 0 && ax == rx + len && ay == ry + len) {
                    len++;
                    continue;
                }
                if (len > 0) {
                    if (n < cap) {
                        runs[4 * n] = rx;
                        runs[4 * n + 1] = ry;
                        runs[4 * n + 2] = len;
                        runs[4 * n + 3] = expansion;
                    }
                    n++;
                }
                rx = ax;
                ry = ay;
                len = 1;
            }
        }
        if (type != CPECAN_OP_INDEL_Y) x += opLen;
        if (type != CPECAN_OP_INDEL_X) y += opLen;
    }
    if (len > 0) {
        if (n < cap) {
            runs[4 * n] = rx;
            runs[4 * n + 1] = ry;
            runs[4 * n + 2] = len;
            runs[4 * n + 3] = expansion;
        }
        n++;
    }
    return n;
}

/* filterToRemoveOverlap (impl/pairwiseAligner.c:1095-1135): one backward and one forward pass over the sorted pairs */
int64_t cpecan_filter_to_remove_overlap(const int64_t *pairs, int64_t n, int64_t *out) {
    if (n < 0 || (n > 0 && (!pairs || !out))) return CPECAN_EINVAL;
    uint8_t *below = malloc((size_t)(n ? n : 1)); /* strictly below every later pair in both coordinates */
    if (!below) return CPECAN_ENOMEM;
    int64_t mX = INT64_MAX, mY = INT64_MAX;
    for (int64_t i = n - 1; i >= 0; i--) {
        const int64_t x = pairs[3 * i], y = pairs[3 * i + 1];
        below[i] = x < mX && y < mY;
        mX = x < mX ? x : mX;
        mY = y < mY ? y : mY;
        if (i > 0 && (pairs[3 * i - 3] > x || (pairs[3 * i - 3] == x && pairs[3 * i - 2] > y))) { /* asserted sorted, :1124-1127 */
            free(below);
            cpk_set_error("filterToRemoveOverlap: the pairs are not sorted by x, then y");
            return CPECAN_EINVAL;
        }
    }
    int64_t count = 0;
    mX = INT64_MIN;
    mY = INT64_MIN;
    for (int64_t i = 0; i < n; i++) {
        const int64_t x = pairs[3 * i], y = pairs[3 * i + 1];
        if (below[i] && x > mX && y > mY) {
            out[3 * count] = x;
            out[3 * count + 1] = y;
            out[3 * count + 2] = pairs[3 * i + 2];
            count++;
        }
        mX = x > mX ? x : mX;
        mY = y > mY ? y : mY;
    }
    free(below);
    return count;
}

int cpecan_device_count(void) { return cpk_device_count(); }
int cpecan_current_device(void) { return cpk_current_device(); }
int64_t cpecan_cache_trim(int device) { return cpk_cache_trim(device); }

int cpecan_ref_cells(const cpecan_model *model, int mode, const cpecan_cell_op *ops, int64_t n, double *cells,
                     int64_t nDoubles, double total) {
    /* the kernel's operation count is an int */
    if (!model || !ops || !cells || n < 0 || n > INT32_MAX || nDoubles < 0 || mode < CPECAN_CELLS_FORWARD || mode > CPECAN_CELLS_POSTERIOR ||
        model->type < CPECAN_FIVE_STATE || model->type > CPECAN_THREE_STATE_ASYM) {
        cpk_set_error("cpecan_ref_cells: invalid arguments");
        return CPECAN_EINVAL;
    }
    const int S = is_five(model->type) ? 5 : 3;
    for (int64_t i = 0; i < n; i++) { /* every offset names a whole cell inside the buffer: the kernel trusts them */
        const int32_t o[4] = {ops[i].cur, ops[i].lower, ops[i].middle, ops[i].upper};
        for (int f = 0; f < 4; f++) {
            const int need = mode == CPECAN_CELLS_POSTERIOR ? (f == 2 ? 0 : 1) : S;
            const int may_be_null = mode != CPECAN_CELLS_POSTERIOR && f > 0;
            if (need == 0 || (may_be_null && o[f] < 0)) continue;
            if (o[f] < 0 || (int64_t)o[f] + need > nDoubles) {
                cpk_set_error("cpecan_ref_cells: operation %lld names a cell outside the buffer", (long long)i);
                return CPECAN_EINVAL;
            }
        }
        if (mode != CPECAN_CELLS_POSTERIOR && (ops[i].cX < 0 || ops[i].cX > 4 || ops[i].cY < 0 || ops[i].cY > 4)) {
            cpk_set_error("cpecan_ref_cells: operation %lld has a symbol outside 0..4", (long long)i);
            return CPECAN_EINVAL;
        }
    }
    CpkModel km;
    kernel_model(model, 0.0, &km);
    return cpk_ref_cells(cpk_current_device(), &km, mode, (const CpkCellOp *)ops, n, cells, nDoubles, total);
}
const char *cpecan_last_error(void) { return cpk_last_error(); }

int cpecan_batch_create(cpecan_batch **out, const cpecan_model *model, const cpecan_params *params, int emit,
                        int device) {
    if (!out || !model || !params) return CPECAN_EINVAL;
    if (!(is_five(model->type) || is_three(model->type))) return CPECAN_EINVAL;
    if (emit != CPECAN_EMIT_MATCH && emit != CPECAN_EMIT_INDEL && emit != CPECAN_EMIT_FORWARD && emit != CPECAN_EMIT_EXPECT) {
        cpk_set_error("unknown emitter %d", emit);
        return CPECAN_EINVAL;
    }
    /* preconditions of getPosteriorProbsWithBanding, pairwiseAligner.c:761-765 */
    if (params->traceBackDiagonals < 1 || params->diagonalExpansion < 0 || params->diagonalExpansion % 2 != 0 ||
        params->minDiagsBetweenTraceBack < 2 || params->traceBackDiagonals + 1 >= params->minDiagsBetweenTraceBack ||
        !(params->threshold >= 0.0 && params->threshold <= 1.0)) {
        cpk_set_error("invalid banding parameters");
        return CPECAN_EINVAL;
    }
    /* The GPU is bound at upload time: adding problems and planning (bands, schedules) are host-only integer work. */
    cpecan_batch *b = calloc(1, sizeof *b);
    if (!b) return CPECAN_ENOMEM;
    b->model = *model;
    b->params = *params;
    b->emit = emit;
    b->device = device;
    b->dev = NULL;
    b->nLists = emit == CPECAN_EMIT_INDEL ? 3 : 1;
    b->anchorStride = params->dynamicAnchorExpansion ? 3 : 2;
    b->runForm = -1;
    b->postMatchGamma = 0.85f; /* cPecanRealign.c:355 */
    b->activeModels = b->downloadedModels = 1;
    *out = b;
    return CPECAN_OK;
}

static void free_results(cpecan_batch *b) {
    for (int64_t i = 0; i < b->nProblems; i++)
        for (int l = 0; l < 4; l++) {
            b->problems[i].triples[l] = NULL;
            b->problems[i].nTriples[l] = 0;
        }
    cpk_host_free(b->results);
    cpk_host_free(b->postMea);
    cpk_host_free(b->postShift);
    free(b->edges);
    cpk_host_free(b->quints);
    free(b->quintOffsets);
    free(b->quintSums);
    b->results = b->postMea = b->postShift = NULL;
    b->edges = NULL;
    b->quints = NULL;
    b->quintOffsets = b->quintSums = NULL;
    free(b->nextRunVals);
    free(b->nextRunOffsets);
    b->nextRunVals = b->nextRunOffsets = NULL;
}

void cpecan_batch_destroy(cpecan_batch *b) {
    if (!b) return;
    if (b->dlActive) (void)cpecan_batch_download_end(b);
    free_results(b);
    cpk_device_destroy(b->dev);
    cpk_host_free(b->problems);
    cpk_host_free(b->regions);
    cpk_host_free(b->symbols);
    cpk_host_free(b->anchors);
    cpk_host_free(b->runs);
    cpk_host_free(b->devRegions);
    cpk_host_free(b->devToHost);
    cpk_host_free(b->segs);
    free(b->forward);
    cpk_host_free(b->chars);
    free(b->quintNames);
    free(b);
}

/* A download running on the helper thread (cpecan_batch_download_begin) rewrites the batch's result arrays, segment
 * table and device order: until cpecan_batch_download_end every other entry point refuses the batch. */
static _Thread_local const cpecan_batch *tl_helperOf = NULL; /* set by the helper thread itself: the batch it downloads */
static int dl_busy(const cpecan_batch *b) {
    /* dlActive is written before pthread_create and after pthread_join only, both of which order it against the helper;
     * the helper recognises itself by its own thread-local mark, not by comparing ids with a field pthread_create is
     * still writing */
    if (!b || !b->dlActive || tl_helperOf == b) return 0;
    cpk_set_error("the batch is being downloaded on its helper thread: call cpecan_batch_download_end first");
    return 1;
}

int cpecan_batch_set_debug(cpecan_batch *b, int on) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || b->frozen) return CPECAN_ESTATE;
    b->debug = on != 0;
    return CPECAN_OK;
}

/* symbol_convertCharToSymbol (pairwiseAligner.c:317-334), toupper and the complement of an upper-case letter (A/C/G/T
 * swapped, everything else as it is) as byte tables: they run over every base added */
static uint8_t g_symbolOf[256], g_upperOf[256], g_complementOf[256];
/* Filled ONCE, when the library is loaded.  (Round 1 refilled them in every cpecan_batch_create, resetting every entry to
 * N first: a batch created on one host thread while another thread converted bases saw A/C/G/T as N for an instant --
 * the intermittent mismatch of the two-host-thread test, found in round 2.) */
__attribute__((constructor)) static void init_byte_tables(void) {
    for (int c = 0; c < 256; c++) {
        g_symbolOf[c] = CPK_SYM_N;
        g_upperOf[c] = (uint8_t)((c >= 'a' && c <= 'z') ? c - 'a' + 'A' : c);
        g_complementOf[c] = (uint8_t)c;
    }
    g_complementOf['A'] = 'T';
    g_complementOf['C'] = 'G';
    g_complementOf['G'] = 'C';
    g_complementOf['T'] = 'A';
    g_symbolOf['A'] = g_symbolOf['a'] = 0;
    g_symbolOf['C'] = g_symbolOf['c'] = 1;
    g_symbolOf['G'] = g_symbolOf['g'] = 2;
    g_symbolOf['T'] = g_symbolOf['t'] = 3;
}
uint8_t cpk_symbol_of(unsigned char c) { return g_symbolOf[c]; } /* cpecan_dense.c */

/* Writes N + symbols + N at dst[at..] (so that index x addresses base x-1 and x = 0 / x = l+1 read as N); returns the
 * offset behind them. */
static int64_t put_symbols(uint8_t *dst, int64_t at, const char *s, int64_t l) {
    dst[at] = CPK_SYM_N;
    for (int64_t i = 0; i < l; i++) dst[at + 1 + i] = g_symbolOf[(unsigned char)s[i]];
    dst[at + l + 1] = CPK_SYM_N;
    return at + l + 2;
}

/* The reversed twin of put_symbols: the l symbols that END at s[end - 1], complemented, last first -- bases a .. a + l - 1
 * of the reverse complement of a sequence of length lY when end = lY - a. */
static int64_t put_symbols_rc(uint8_t *dst, int64_t at, const char *s, int64_t end, int64_t l) {
    dst[at] = CPK_SYM_N;
    for (int64_t i = 0; i < l; i++) {
        const uint8_t c = g_symbolOf[(unsigned char)s[end - 1 - i]];
        dst[at + 1 + i] = c < 4 ? (uint8_t)(3 - c) : c;
    }
    dst[at + l + 1] = CPK_SYM_N;
    return at + l + 2;
}

/* One problem of an add call: its anchors as triples (x, y, expansion), one per anchor, or -- `runs` -- as quadruples
 * (x, y, length, expansion), one per run of diagonal neighbours (cpecan_batch_add_many_runs). */
typedef struct {
    const char *sX;
    int64_t lX;
    const char *sY;
    int64_t lY;
    const int64_t *anchors;
    int64_t nAnchors; /* entries: anchors or runs */
    int32_t raggedLeft, raggedRight;
    int runs;
    int minus; /* anchors and results are in the coordinates of (X, rc(sY)) */
} ProblemView;
static inline AnchorCursor cursor_of(const ProblemView *it) {
    return (AnchorCursor){it->anchors, it->anchors + (it->runs ? 4 : 3) * it->nAnchors, it->runs};
}

/* The split rectangles of one problem (getSplitPoints semantics, pairwiseAligner.c:1230-1271) into *rects, grown as
 * needed.  Returns their number or < 0. */
static int64_t problem_rects(const cpecan_batch *b, const ProblemView *it, int64_t **rects, int64_t *cap) {
    if (4 * (it->nAnchors + 2) > *cap) { /* the caller's scratch: plain heap memory, freed with free() */
        const int64_t c = 8 * (it->nAnchors + 2);
        int64_t *q = realloc(*rects, sizeof(int64_t) * (size_t)c);
        if (!q) return CPECAN_ENOMEM;
        *rects = q;
        *cap = c;
    }
    if (b->emit == CPECAN_EMIT_FORWARD) { /* computeForwardProbability never splits (pairwiseAligner.c:936-949) */
        (*rects)[0] = 0;
        (*rects)[1] = 0;
        (*rects)[2] = it->lX;
        (*rects)[3] = it->lY;
        return 1;
    }
    return split_points_entries(cursor_of(it), it->lX, it->lY, b->params.splitMatrixBiggerThanThis, it->raggedLeft, it->raggedRight, *rects);
}

static int problem_valid(const ProblemView *it) {
    if (it->lX < 0 || it->lY < 0 || it->nAnchors < 0 || (it->lX > 0 && !it->sX) || (it->lY > 0 && !it->sY) ||
        (it->nAnchors > 0 && !it->anchors))
        return 0;
    if (it->lX + it->lY >= (int64_t)1 << 30) return 0;
    /* entries strictly increase in both coordinates from the last anchor of one to the first of the next
     * (pairwiseAligner.c:159-164) and lie inside the matrix; expansions are kept as 32-bit values */
    AnchorCursor cur = cursor_of(it);
    AnchorEntry e;
    for (int64_t px = -1, py = -1; next_entry(&cur, &e); px = e.x + e.len - 1, py = e.y + e.len - 1)
        if (e.len < 1 || e.x <= px || e.y <= py || e.x + e.len > it->lX || e.y + e.len > it->lY || e.expansion < INT32_MIN ||
            e.expansion > INT32_MAX)
            return 0;
    return 1;
}

/* problem i of an add call in either form (the two public structs differ in what their anchor arrays hold) */
static ProblemView view_of(const void *items, int runs, const int32_t *yMinus, int64_t i) {
    ProblemView v;
    if (runs) {
        const cpecan_problem_runs *p = (const cpecan_problem_runs *)items + i;
        v = (ProblemView){p->sX, p->lX, p->sY, p->lY, p->runs, p->nRuns, p->raggedLeft, p->raggedRight, 1, yMinus && yMinus[i]};
    } else {
        const cpecan_problem *p = (const cpecan_problem *)items + i;
        v = (ProblemView){p->sX, p->lX, p->sY, p->lY, p->anchors, p->nAnchors, p->raggedLeft, p->raggedRight, 0, 0};
    }
    return v;
}

/* The scratch of an add call, one record per problem: what the problem adds to the batch's arrays (stage one) and where its
 * slices start (stage two); one more than the call has problems. */
typedef struct {
    int64_t nRects, symbolBytes, nAnchorsKept, nRunsKept;
    int64_t regionAt, symbolAt, anchorValAt, runValAt, charAt;
} AddSlot;

/* Stage one: validates every problem and counts what it needs (the problems are independent: OpenMP when there are enough
 * of them).  The error names the first bad problem of the call. */
static int add_count(const cpecan_batch *b, const void *items, int runs, const int32_t *yMinus, int64_t n, AddSlot *slots) {
    int64_t firstBad = n;
    int bad = CPECAN_OK;
#pragma omp parallel num_threads(cpk_host_threads()) if (n >= 64)
    {
        int64_t *rects = NULL, cap = 0;
#pragma omp for schedule(dynamic, 32)
        for (int64_t i = 0; i < n; i++) {
            const ProblemView view = view_of(items, runs, yMinus, i), *it = &view;
            AddSlot *s = &slots[i];
            memset(s, 0, sizeof *s);
            const int64_t nRects = problem_valid(it) ? problem_rects(b, it, &rects, &cap) : CPECAN_EINVAL;
            if (nRects < 0) {
#pragma omp critical(cpk_add)
                if (i < firstBad) {
                    firstBad = i;
                    bad = nRects == CPECAN_ENOMEM ? CPECAN_ENOMEM : CPECAN_EINVAL;
                }
                continue;
            }
            AnchorCursor cur = cursor_of(it);
            AnchorEntry e;
            int64_t sym = 0, kept = 0, entries = 0;
            for (int64_t k = 0; k < nRects; k++) {
                const int64_t *rect = rects + 4 * k, diagEnd = rect[2] + rect[3];
                sym += (rect[2] - rect[0]) + (rect[3] - rect[1]) + 4; /* N + bases + N, twice */
                for (; next_in_rect(&cur, diagEnd, &e); entries++) kept += e.len;
            }
            s->nRects = nRects;
            s->symbolBytes = sym;
            s->nAnchorsKept = kept;
            /* a batch that keeps runs: the problem's runs as they are, or -- anchors given one by one -- a run of one each */
            s->nRunsKept = entries;
        }
        free(rects);
    }
    if (bad == CPECAN_EINVAL) cpk_set_error("problem %lld of the call: bad lengths or anchors", (long long)firstBad);
    return bad;
}

/* Stage two: the counts become offsets -- slots[n] receives where the call ends --, and the batch's arrays grow to hold the
 * call.  Nothing of the batch but the capacities changes here. */
static int add_reserve(cpecan_batch *b, const void *items, int runs, const int32_t *yMinus, int64_t n, AddSlot *slots) {
    const int keepRuns = b->runForm == 1;
    AddSlot at = {0, 0, 0, 0, b->nRegions, b->nSymbols, b->nAnchorVals, b->nRunVals, b->nChars}; /* the running offsets */
    for (int64_t i = 0; i <= n; i++) {
        AddSlot *s = &slots[i];
        s->regionAt = at.regionAt;
        s->symbolAt = at.symbolAt;
        s->anchorValAt = at.anchorValAt;
        s->runValAt = at.runValAt;
        s->charAt = at.charAt;
        if (i == n) break;
        const ProblemView view = view_of(items, runs, yMinus, i);
        at.regionAt += s->nRects;
        at.symbolAt += s->symbolBytes;
        at.anchorValAt += b->anchorStride * s->nAnchorsKept;
        if (keepRuns) at.runValAt += 4 * s->nRunsKept;
        at.charAt += view.lX + view.lY;
    }
    if (grow((void **)&b->problems, &b->capProblems, b->nProblems + n, sizeof(HostProblem)) ||
        grow((void **)&b->regions, &b->capRegions, at.regionAt, sizeof(HostRegion)) ||
        (keepRuns ? grow((void **)&b->runs, &b->capRunVals, at.runValAt, sizeof(int32_t))
                  : grow((void **)&b->anchors, &b->capAnchorVals, at.anchorValAt, sizeof(int32_t))) ||
        grow((void **)&b->symbols, &b->capSymbols, at.symbolAt, 1) || grow((void **)&b->chars, &b->capChars, at.charAt + 1, 1) ||
        (keepRuns && at.anchorValAt / 2 >= ((int64_t)1 << 31))) /* (a run's first anchor is a 32-bit index) */
        return CPECAN_ENOMEM;
    return CPECAN_OK;
}

/* Stage three, one problem: its record, its letters, and per rectangle a region with its symbols and its anchors.  The
 * rectangles are those stage one counted. */
static void add_write_problem(cpecan_batch *b, const ProblemView *it, const int64_t *rects, const AddSlot *s, int64_t problem) {
    const int keepRuns = b->runForm == 1, stride = b->anchorStride;
    HostProblem *pr = &b->problems[problem];
    memset(pr, 0, sizeof *pr);
    pr->firstRegion = s->regionAt;
    pr->nRegions = s->nRects;
    pr->lX = it->lX;
    pr->lY = it->lY;
    pr->charX = s->charAt;
    pr->charY = pr->charX + it->lX;
    pr->minus = it->minus;
    uint8_t *ch = b->chars + s->charAt;
    for (int64_t k = 0; k < it->lX; k++) ch[k] = g_upperOf[(unsigned char)it->sX[k]];
    if (it->minus)
        for (int64_t k = 0; k < it->lY; k++) ch[it->lX + k] = g_complementOf[g_upperOf[(unsigned char)it->sY[it->lY - 1 - k]]];
    else
        for (int64_t k = 0; k < it->lY; k++) ch[it->lX + k] = g_upperOf[(unsigned char)it->sY[k]];
    int64_t symAt = s->symbolAt, anchorAt = s->anchorValAt, runValAt = s->runValAt;
    AnchorCursor cur = cursor_of(it);
    AnchorEntry e;
    for (int64_t k = 0; k < s->nRects; k++) {
        const int64_t *rect = rects + 4 * k, x1 = rect[0], y1 = rect[1], diagEnd = rect[2] + rect[3];
        HostRegion *r = &b->regions[s->regionAt + k];
        memset(r, 0, sizeof *r);
        r->problem = problem;
        r->x1 = x1;
        r->y1 = y1;
        r->lX = rect[2] - x1;
        r->lY = rect[3] - y1;
        r->raggedLeft = (it->raggedLeft || k > 0) ? 1 : 0;
        r->raggedRight = (it->raggedRight || k < s->nRects - 1) ? 1 : 0;
        r->seqXOff = symAt;
        symAt = put_symbols(b->symbols, symAt, it->sX + x1, r->lX);
        r->seqYOff = symAt;
        symAt = it->minus ? put_symbols_rc(b->symbols, symAt, it->sY, it->lY - y1, r->lY) : put_symbols(b->symbols, symAt, it->sY + y1, r->lY);
        r->anchorOff = anchorAt / stride;
        if (keepRuns) { /* the runs stay runs: 16 bytes each, whatever their length */
            r->runOff = runValAt / 4;
            while (next_in_rect(&cur, diagEnd, &e)) {
                int32_t *q = b->runs + runValAt;
                q[0] = (int32_t)(e.x - x1);
                q[1] = (int32_t)(e.y - y1);
                q[2] = (int32_t)e.len;
                q[3] = (int32_t)(anchorAt / 2); /* its first anchor among the batch's (expanded on the device) */
                runValAt += 4;
                anchorAt += 2 * e.len;
                r->nAnchors += e.len;
                r->nRuns++;
            }
            continue;
        }
        /* an entry becomes its anchors: the batch's own 8 (12) bytes each, never the API's 24 */
        while (next_in_rect(&cur, diagEnd, &e)) {
            const int32_t rx = (int32_t)(e.x - x1), ry = (int32_t)(e.y - y1), ex = (int32_t)e.expansion;
            int32_t *a = b->anchors + anchorAt;
            if (e.len == 1) { /* a triple: no loop to set up for the one anchor (6e7 of them in a config-4 batch) */
                a[0] = rx;
                a[1] = ry;
                if (stride == 3) a[2] = ex;
            } else
                for (int64_t q = 0; q < e.len; q++, a += stride) {
                    a[0] = rx + (int32_t)q;
                    a[1] = ry + (int32_t)q;
                    if (stride == 3) a[2] = ex;
                }
            anchorAt += stride * e.len;
            r->nAnchors += e.len;
        }
    }
}

/* Stage three: every problem writes its own slices.  The rectangles are recomputed, not kept from stage one. */
static int add_write(cpecan_batch *b, const void *items, int runs, const int32_t *yMinus, int64_t n, const AddSlot *slots) {
    int oom = 0;
#pragma omp parallel num_threads(cpk_host_threads()) if (n >= 64)
    {
        int64_t *rects = NULL, cap = 0;
#pragma omp for schedule(dynamic, 32)
        for (int64_t i = 0; i < n; i++) {
            const ProblemView view = view_of(items, runs, yMinus, i);
            if (problem_rects(b, &view, &rects, &cap) != slots[i].nRects) { /* only an allocation failure can change the answer */
#pragma omp atomic write
                oom = 1;
                continue;
            }
            add_write_problem(b, &view, rects, &slots[i], b->nProblems + i);
        }
        free(rects);
    }
    return oom ? CPECAN_ENOMEM : CPECAN_OK;
}

/* An add call in three stages -- count, reserve, write -- and then the commit: the used lengths move only when every stage
 * went through, so a failed call leaves the batch as it was. */
static int64_t add_many(cpecan_batch *b, const void *items, int runs, const int32_t *yMinus, int64_t n) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || b->frozen) return CPECAN_ESTATE;
    if (n < 0 || (n > 0 && !items)) return CPECAN_EINVAL;
    if (n == 0) return b->nProblems;
    if (b->runForm < 0) { /* decided by the batch's first problems.  CPECAN_KEEP_RUNS=0: one anchor per column on the host, as rounds 1-3 */
        const char *env = getenv("CPECAN_KEEP_RUNS");
        b->runForm = (runs && b->anchorStride == 2 && !(env && atoi(env) == 0)) ? 1 : 0;
    }
    AddSlot *slots = malloc(sizeof(AddSlot) * (size_t)(n + 1)); /* the one exit below frees it */
    int64_t rc = slots ? add_count(b, items, runs, yMinus, n, slots) : CPECAN_ENOMEM;
    if (rc == CPECAN_OK) rc = add_reserve(b, items, runs, yMinus, n, slots);
    if (rc == CPECAN_OK) rc = add_write(b, items, runs, yMinus, n, slots);
    if (rc == CPECAN_OK) {
        const AddSlot *end = &slots[n];
        rc = b->nProblems; /* the index of the call's first problem */
        b->nProblems += n;
        b->nRegions = end->regionAt;
        b->nSymbols = end->symbolAt;
        b->nAnchorVals = end->anchorValAt;
        b->nRunVals = end->runValAt;
        b->nChars = end->charAt;
    }
    free(slots);
    return rc;
}

int64_t cpecan_batch_add_many(cpecan_batch *b, const cpecan_problem *items, int64_t n) { return add_many(b, items, 0, NULL, n); }
int64_t cpecan_batch_add_many_runs(cpecan_batch *b, const cpecan_problem_runs *items, int64_t n) { return add_many(b, items, 1, NULL, n); }
int64_t cpecan_batch_add_many_runs_stranded(cpecan_batch *b, const cpecan_problem_runs *items, const int32_t *yMinus, int64_t n) {
    return add_many(b, items, 1, yMinus, n);
}

int cpecan_batch_problem_strand(const cpecan_batch *b, int64_t problem) {
    if (!b || problem < 0 || problem >= b->nProblems) return CPECAN_EINVAL;
    return b->problems[problem].minus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
}

int64_t cpecan_anchor_runs(const int64_t *anchors, int64_t nAnchors, int64_t *out, int64_t cap) {
    if (nAnchors < 0 || cap < 0 || (nAnchors > 0 && !anchors) || (cap > 0 && !out)) return CPECAN_EINVAL;
    int64_t n = 0;
    for (int64_t i = 0; i < nAnchors;) {
        int64_t len = 1;
        while (i + len < nAnchors && anchors[3 * (i + len)] == anchors[3 * i] + len && anchors[3 * (i + len) + 1] == anchors[3 * i + 1] + len &&
               anchors[3 * (i + len) + 2] == anchors[3 * i + 2])
            len++;
        if (n < cap) {
            out[4 * n] = anchors[3 * i];
            out[4 * n + 1] = anchors[3 * i + 1];
            out[4 * n + 2] = len;
            out[4 * n + 3] = anchors[3 * i + 2];
        }
        n++;
        i += len;
    }
    return n;
}

int64_t cpecan_batch_add(cpecan_batch *b, const char *sX, int64_t lX, const char *sY, int64_t lY,
                         const int64_t *anchors, int64_t nAnchors, int raggedLeft, int raggedRight) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    const cpecan_problem it = {sX, lX, sY, lY, anchors, nAnchors, raggedLeft ? 1 : 0, raggedRight ? 1 : 0};
    return cpecan_batch_add_many(b, &it, 1);
}

typedef struct {
    int64_t cells;
    int64_t index;
    int cls; /* 0, 1, 2: narrow, at most 8 / 16 / 32 cells per diagonal (packed kernel); 3 ..: the wide classes */
} CostKey;

/* what planning keeps of a region's band walk */
typedef struct {
    int64_t maxW, liveMax, fbMax, nSeg, refreshMax;
    int smooth; /* both edges of the band move by exactly one x-y step per diagonal (fixed expansions do): the region may run
                 * under the absolute-position sweeps (cpk_table_gather.inl, "positions") */
    int64_t winBytes; /* LDS bytes of the largest symbol window of a traceback segment (both strings, two symbols per byte):
                       * what the absolute-position sweeps stage per segment instead of the whole strings (cpk_sweep.inl) */
} RegionPlan;

static int by_cost_desc(const void *a, const void *b) {
    const CostKey *p = a, *q = b;
    if (p->cls != q->cls) return p->cls < q->cls ? -1 : 1;
    if (p->cells != q->cells) return p->cells > q->cells ? -1 : 1;
    return p->index < q->index ? -1 : (p->index > q->index);
}

static int64_t default_out_cap(const cpecan_batch *b, const HostRegion *r) {
    int64_t cap = 6 * (r->lX + r->lY) + 64;
    if (b->params.threshold <= 0.0 || cap > r->cells) cap = r->cells;
    return cap < 1 ? 1 : cap;
}

/* Threads for the host's parallel loops: OpenMP's default is every hardware thread of the machine, which on a shared
 * multi-GPU host is far more than this process's share; 16 unless CPECAN_THREADS or a smaller OMP_NUM_THREADS says otherwise. */
int cpk_host_threads(void) {
    const char *env = getenv("CPECAN_THREADS");
    int n = env ? atoi(env) : 0;
    if (n < 1) {
        n = omp_get_max_threads();
        if (n > 16) n = 16;
    }
    return n < 1 ? 1 : n;
}

/* What one upload's planning holds until the batch takes it over (host_plan_commit) or it is dropped (host_plan_free). */
typedef struct {
    int64_t *diagStart, *segStart; /* per region: its first diagonal of the device's table and its first segment slot */
    CostKey *keys;                 /* per region; in device order once sorted */
    RegionPlan *plan;
    CpkSegment *segs;
    int64_t nSegs; /* slots: every region gets room for an upper bound on its segment count */
    int64_t totalDiags, totalCells;
    CpkRegion *devRegions;
    int64_t *devToHost;
    int64_t outTriples, dbgCells, dbgDiags; /* at least 1 each */
    int dynamic;    /* per-anchor expansions are in force */
    int fastWalk;   /* CPECAN_FAST_WALK=0: plan_region walks every diagonal */
    int packedKnob; /* CPECAN_PACKED: -1 unset; 0 = one wave per region for every region (diagnostic); 2 = pack however few */
} HostPlan;

static void host_plan_free(HostPlan *hp) {
    free(hp->diagStart);
    free(hp->segStart);
    free(hp->keys);
    free(hp->plan);
    cpk_host_free(hp->segs);
    cpk_host_free(hp->devRegions);
    cpk_host_free(hp->devToHost);
    memset(hp, 0, sizeof *hp);
}

/* The one point at which the batch becomes the owner of the plan's device-order arrays. */
static void host_plan_commit(cpecan_batch *b, HostPlan *hp, const CpkGeometry *geo) {
    b->geo = *geo;
    b->devRegions = hp->devRegions;
    b->devToHost = hp->devToHost;
    b->segs = hp->segs;
    b->nSegs = hp->nSegs;
    b->nDiags = hp->totalDiags;
    b->outTriples = hp->outTriples;
    b->dbgCells = hp->dbgCells;
    b->dbgDiags = hp->dbgDiags;
    hp->devRegions = NULL;
    hp->devToHost = NULL;
    hp->segs = NULL;
}

/* The knobs, read once per upload, and the per-region diagonal and segment slots. */
static int host_plan_init(const cpecan_batch *b, HostPlan *hp) {
    const cpecan_params *p = &b->params;
    const char *fwEnv = getenv("CPECAN_FAST_WALK"), *pkEnv = getenv("CPECAN_PACKED");
    memset(hp, 0, sizeof *hp);
    hp->dynamic = b->emit == CPECAN_EMIT_FORWARD ? 0 : p->dynamicAnchorExpansion; /* :894: forward uses the static band */
    hp->fastWalk = !(fwEnv && atoi(fwEnv) == 0);
    hp->packedKnob = pkEnv ? atoi(pkEnv) : -1;
    hp->diagStart = malloc(sizeof(int64_t) * (size_t)b->nRegions);
    hp->segStart = malloc(sizeof(int64_t) * (size_t)b->nRegions);
    hp->keys = malloc(sizeof(CostKey) * (size_t)b->nRegions);
    hp->plan = calloc((size_t)b->nRegions, sizeof(RegionPlan));
    if (!hp->diagStart || !hp->segStart || !hp->keys || !hp->plan) return CPECAN_ENOMEM;
    for (int64_t i = 0; i < b->nRegions; i++) {
        const int64_t N = b->regions[i].lX + b->regions[i].lY;
        hp->diagStart[i] = hp->totalDiags;
        hp->totalDiags += N + 1;
        hp->segStart[i] = hp->nSegs;
        /* consecutive traceback points are at least minDiagsBetweenTraceBack - (traceBackDiagonals + 1) >= 1 apart */
        hp->nSegs += N / (p->minDiagsBetweenTraceBack - p->traceBackDiagonals - 1) + 2;
    }
    hp->segs = host_zalloc((size_t)hp->nSegs, sizeof(CpkSegment));
    return hp->segs ? CPECAN_OK : CPECAN_ENOMEM;
}

/* One region's band walk and traceback schedule (pairwiseAligner.c:791-810): fills plan[i], the region's segments and its
 * cell count.  hist: 4 K cell offsets, widths and first coordinates of the last K = traceBackDiagonals + 3 diagonals --
 * the schedule looks that far back.  Returns nonzero for anchors that do not define a valid band. */
static int plan_region(cpecan_batch *b, HostPlan *hp, int64_t i, int64_t *hist) {
    const cpecan_params *p = &b->params;
    const int64_t K = p->traceBackDiagonals + 3;
    int64_t *histOff = hist, *histW = hist + K, *histXlo = hist + 2 * K, *histYlo = hist + 3 * K;
    HostRegion *r = &b->regions[i];
    RegionPlan *pl = &hp->plan[i];
    const int64_t N = r->lX + r->lY;
    const int dynamic = hp->dynamic;
    CpkBandIter it;
    memset(&it, 0, sizeof it);
    int bad = b->runForm == 1 ? cpk_band_init_runs(&it, b->runs + 4 * r->runOff, r->nRuns, r->nAnchors, r->lX, r->lY, p->diagonalExpansion)
                              : cpk_band_init(&it, b->anchors + (int64_t)b->anchorStride * r->anchorOff, b->anchorStride, r->nAnchors,
                                              r->lX, r->lY, p->diagonalExpansion, dynamic);
    CpkSegment *sg = hp->segs + hp->segStart[i];
    int64_t cells = 0, tracedBackTo = 0;
    int64_t offTracedBackTo = 0; /* cells before diagonal tracedBackTo */
    int64_t offAfter = 0;        /* cells before diagonal tracedBackTo + 1 */
    int64_t slot = 0; /* d % K without the division: this loop runs once per diagonal of the batch */
    int64_t maxW = 0;
    int64_t prevLo = 0, prevHi = 0;
    int64_t winXlo = 0, winYlo = 0; /* smallest x and y of diagonal tracedBackTo + 1 (symbol windows, RegionPlan::winBytes) */
    int smooth = !dynamic;
    const int64_t minBetween = p->minDiagsBetweenTraceBack, narrow = p->diagonalExpansion * 2 + 1;
    /* Runs of diagonal neighbours among the anchors (realign-style input: one anchor per matching column) are walked
     * in closed form.  Between two anchors (X, Y) and (X + 1, Y + 1) of a run, away from the matrix edges, the band
     * holds exactly two diagonals: x-y in [X-Y-E-1, X-Y+E+1] (E + 2 cells) and [X-Y-E, X-Y+E] (E + 1 cells) -- both
     * "narrow" for E >= 2 (<= 2E + 1) and both edges one x-y step apart from their neighbours'.  So a stretch of s such
     * intervals adds s (2E + 3) cells and nothing else, unless a traceback point may fall into it or behind it within the
     * K diagonals whose offsets the schedule looks back at: those diagonals are walked one by one.
     * (BASELINE config 4: 1.25e8 diagonals at ~14 cycles each were 31 ms of every batch on 16 threads.)  CPECAN_FAST_WALK=0
     * walks every diagonal (tests compare the two).  The iterator finds the stretch and steps over it (cpk_band_run_ahead,
     * cpk_band_skip_run); how far a skip may go and what it adds to the plan is decided here. */
    const int64_t E = p->diagonalExpansion;
    const int fastOk = hp->fastWalk && !dynamic && E >= 2 && b->anchorStride == 2;  /* (runs are kept for stride 2 only) */
    for (int64_t d = 0; d <= N && !bad; d++, slot = slot + 1 == K ? 0 : slot + 1) {
        if (fastOk && cpk_band_in_run(&it, d)) {
            /* every skipped diagonal stays K + 1 below the next traceback point, and below the region's last two */
            const int64_t sMax = imin((tracedBackTo + minBetween - (K + 1) - d) / 2, (N - 2 - d) / 2);
            const int64_t sRun = cpk_band_run_ahead(&it, sMax);
            if (sRun >= 2) {
                const int64_t add = sRun * (2 * E + 3);
                if (cells + add >= (int64_t)1 << 31) {
                    bad = 1;
                    break;
                }
                const int64_t xmy0 = cpk_band_run_xmy(&it);
                if (d > 0) { /* the step into the stretch: from the diagonal before to its first one */
                    const int64_t dl = (xmy0 - E - 1) - prevLo, dh = (xmy0 + E + 1) - prevHi;
                    smooth &= (dl == 1 || dl == -1) && (dh == 1 || dh == -1);
                }
                cells += add;
                maxW = E + 2 > maxW ? E + 2 : maxW;
                prevLo = xmy0 - E; /* the stretch's last diagonal: the second one of an interval */
                prevHi = xmy0 + E;
                if (cpk_band_skip_run(&it, sRun)) {
                    bad = 1;
                    break;
                }
                d += 2 * sRun - 1; /* the loop's own step makes it 2 sRun */
                slot = (slot + 2 * sRun - 1) % K;
                continue;
            }
        }
        int64_t lo, hi;
        if (cpk_band_next(&it, d, &lo, &hi)) {
            bad = 1;
            break;
        }
        const int64_t w = (hi - lo) / 2 + 1;
        if (cells + w >= (int64_t)1 << 31) {
            bad = 1;
            break;
        }
        if (d > 0) {
            const int64_t dl = lo - prevLo, dh = hi - prevHi;
            smooth &= (dl == 1 || dl == -1) && (dh == 1 || dh == -1);
        }
        prevLo = lo;
        prevHi = hi;
        histOff[slot] = cells;
        histW[slot] = w;
        histXlo[slot] = (d + lo) >> 1;      /* x of the diagonal's first cell */
        histYlo[slot] = d - ((d + hi) >> 1); /* y of its last cell: the smallest */
        if (d == 1) {
            offAfter = cells; /* tracedBackTo == 0 for the first segment */
            winXlo = histXlo[slot];
            winYlo = histYlo[slot];
        }
        maxW = w > maxW ? w : maxW;
        cells += w;
        if (d == 0) continue;
        const int atEnd = d == N;
        const int tracebackPoint = d >= tracedBackTo + minBetween && w <= narrow;
        if (!atEnd && !tracebackPoint) continue;
        memset(sg, 0, sizeof *sg);
        sg->tbPrev = (int32_t)tracedBackTo;
        sg->dTop = (int32_t)d;
        sg->tbFrom = (int32_t)(d - (atEnd ? 0 : p->traceBackDiagonals + 1));
        sg->atEnd = atEnd;
        sg->nRefresh = (int32_t)((sg->tbFrom - (sg->tbPrev + 1)) / CPK_REFRESH_PERIOD + 1);
        pl->refreshMax = sg->nRefresh > pl->refreshMax ? sg->nRefresh : pl->refreshMax;
        /* forward diagonals tbPrev..dTop are live during this traceback */
        pl->liveMax = imax(pl->liveMax, cells - offTracedBackTo);
        const int64_t tf = sg->tbFrom;
        const int64_t tfSlot = tf % K; /* once per segment */
        const int64_t fbCells = histOff[tfSlot] + histW[tfSlot] - offAfter;
        pl->fbMax = imax(pl->fbMax, fbCells);
        sg->emitCells = (int32_t)fbCells;
        {
            /* the symbols the segment's diagonals tbPrev + 1 .. d touch, the kernel's arithmetic (cpk_sweep.inl,
             * "Symbol windows"): from the even index at or below the smallest x (y) to one past the largest */
            const int64_t x0 = winXlo & ~(int64_t)1, y0 = winYlo & ~(int64_t)1;
            const int64_t x1 = imin(((d + hi) >> 1) + 1, r->lX + 1), y1 = imin(d - ((d + lo) >> 1) + 1, r->lY + 1);
            pl->winBytes = imax(pl->winBytes, (x1 - x0 + 2) / 2 + (y1 - y0 + 2) / 2);
        }
        pl->nSeg++;
        sg++;

        /* the next segment starts from tbFrom: remember the cell offsets of tbFrom and tbFrom + 1 */
        tracedBackTo = tf;
        offTracedBackTo = histOff[tfSlot];
        offAfter = histOff[tfSlot] + histW[tfSlot];
        if (tf < d) { /* diagonal tf + 1 has been walked already: within the last K */
            const int64_t s1 = (tf + 1) % K;
            winXlo = histXlo[s1];
            winYlo = histYlo[s1];
        }
    }
    pl->maxW = maxW;
    pl->smooth = smooth;
    if (bad) return 1;
    r->cells = cells;
    hp->keys[i].cells = N > 0 ? cells : 0;
    return 0;
}

/* Planning walks every region's band ONCE as a stream of diagonals (cpecan_band.inl) and keeps per-region sums only:
 * cell count, widest diagonal, the traceback schedule (pairwiseAligner.c:791-810) and the scratch sizes it implies.
 * The per-diagonal table the kernels read (16 bytes per diagonal, 640 MB at 10 000 pairs x 2 kb) is built on the
 * device from the anchors by the same iterator (cpk_device_upload).  Regions are independent: OpenMP.  Of the regions
 * whose band is bad the lowest index is reported, whichever thread met it first. */
static int plan_regions(cpecan_batch *b, HostPlan *hp) {
    const size_t K = (size_t)b->params.traceBackDiagonals + 3;
    int rc = CPECAN_OK;
    int64_t badRegion = -1;
#pragma omp parallel num_threads(cpk_host_threads())
    {
        int64_t *hist = malloc(sizeof(int64_t) * K * 4);
        if (!hist) {
#pragma omp critical(cpk_plan)
            rc = CPECAN_ENOMEM;
        }
#pragma omp for schedule(dynamic, 16)
        for (int64_t i = 0; i < b->nRegions; i++) {
            hp->keys[i].cells = 0;
            hp->keys[i].index = i;
            if (!hist || !plan_region(b, hp, i, hist)) continue;
#pragma omp critical(cpk_plan)
            {
                rc = CPECAN_EINVAL;
                if (badRegion < 0 || i < badRegion) badRegion = i;
            }
        }
        free(hist);
    }
    if (badRegion >= 0)
        cpk_set_error("region %lld of problem %lld: anchors do not define a valid band (or the band exceeds 2^31 cells)",
                      (long long)badRegion, (long long)b->regions[badRegion].problem);
    return rc;
}

/* Narrow regions (no diagonal wider than 32 cells: realign-style bands) are packed several to a wave by their own
 * kernel; they come first in the device order.  Within each class: longest first (the work queues are LPT). */
static void classify_regions(const cpecan_batch *b, HostPlan *hp) {
    const int S = is_five(b->model.type) ? 5 : 3;
    CostKey *keys = hp->keys;
    /* (bands with per-anchor expansions run the packed kernel's DYN variant: their edges may move backwards) */
    const int enabled = (b->emit == CPECAN_EMIT_MATCH || b->emit == CPECAN_EMIT_INDEL || b->emit == CPECAN_EMIT_EXPECT) && !b->debug &&
                        hp->packedKnob != 0;
    /* a launch is not worth fewer regions (CPECAN_PACKED=2: always, for tests).  The indel emitter's packed form pays a
     * pass of its own over every emitted cell: measured on realign-style batches it ties with one wave per region at
     * 10 000 alignments (32.1 against 30.5 ms) and wins 2.4x at 50 000 (61 against 148 ms) -- from ~12 000 regions of
     * a class, i.e. once a wave has half a dozen rounds to go (profiles/r04_packed_indel_emitter.txt) */
    const int64_t minCount = hp->packedKnob >= 2 ? 1 : (b->emit == CPECAN_EMIT_INDEL ? 12000 : 64);
    int64_t perClass[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < b->nRegions; i++) {
        const int64_t w = hp->plan[i].maxW;
        const int empty = b->regions[i].lX + b->regions[i].lY == 0;
        keys[i].cls = (!enabled || empty || w > 32) ? 3 : (w <= 8 ? 0 : (w <= 16 ? 1 : 2));
        perClass[keys[i].cls]++;
    }
    for (int k = 0; k < 3; k++) /* a class too small for its own launch joins the next wider one */
        if (perClass[k] > 0 && perClass[k] < minCount) {
            for (int64_t i = 0; i < b->nRegions; i++)
                if (keys[i].cls == k) keys[i].cls = k + 1;
            perClass[k + 1] += perClass[k];
            perClass[k] = 0;
        }
    /* the wide regions by the LDS their rolling buffers and symbol strings need (classes 3..9; the last one keeps
     * both in global memory): a launch per class, each with its own occupancy and per-wave scratch */
    for (int64_t i = 0; i < b->nRegions; i++) {
        if (keys[i].cls != 3) continue;
        const int64_t w = hp->plan[i].maxW;
        const size_t lds = sizeof(double) * (size_t)(544 + 768 + (2 * S + 1) * (w + 1)) +
                           (size_t)((b->regions[i].lX + 3) / 2 + (b->regions[i].lY + 3) / 2) + 16;
        static const int64_t edge[CPK_WIDE_CLASSES - 2] = {64, 128, 192, 256, 384, 512};
        /* up to 64 cells: a class of its own for the expectation emitter only -- its in-sweep kernel has a build unrolled
         * for one 64-lane group per diagonal (BASELINE config 5: 99 % of the regions); the other emitters' kernels loop
         * over groups and gain nothing from another launch */
        int k = b->emit == CPECAN_EMIT_EXPECT ? 0 : 1;
        while (k < CPK_WIDE_CLASSES - 2 && w > edge[k]) k++; /* CPK_WIDE_CLASSES - 2: wider, but its LDS still fits */
        keys[i].cls = 3 + (lds > 64 * 1024 ? CPK_WIDE_CLASSES - 1 : k);
    }
}

/* sort value: class in the top 4 of 36 bits, then 2^31 - 1 - cells (cells < 2^31): ascending = by_cost_desc */
static inline int cost_key_digit(const CostKey *k, int pass) {
    return (int)(((((uint64_t)k->cls) << 32 | (uint64_t)(0x7fffffffll - k->cells)) >> (12 * pass)) & 0xfff);
}

/* (class, cells descending, index): the keys stand in index order, so a STABLE sort by (class, -cells) is the order
 * by_cost_desc defines -- three counting passes of 12 bits instead of qsort's n log n comparator calls (4.3 ms of every
 * config-4 batch on one thread). */
static void sort_cost_keys(CostKey *keys, int64_t n) {
    CostKey *tmp = malloc(sizeof(CostKey) * (size_t)(n ? n : 1));
    if (!tmp) {
        qsort(keys, (size_t)n, sizeof(CostKey), by_cost_desc);
        return;
    }
    CostKey *src = keys, *dst = tmp;
    for (int pass = 0; pass < 3; pass++) {
        int64_t count[4097];
        memset(count, 0, sizeof count);
        for (int64_t i = 0; i < n; i++) count[cost_key_digit(&src[i], pass) + 1]++;
        for (int q = 0; q < 4096; q++) count[q + 1] += count[q];
        for (int64_t i = 0; i < n; i++) dst[count[cost_key_digit(&src[i], pass)]++] = src[i];
        CostKey *t = src;
        src = dst;
        dst = t;
    }
    if (src != keys) memcpy(keys, src, sizeof(CostKey) * (size_t)n); /* three passes: the result is in tmp */
    free(tmp);
}

/* Class counts add up, class maxima are maxima: one thread's geometry into the batch's. */
static void geometry_merge(CpkGeometry *dst, const CpkGeometry *src) {
    for (int k = 0; k < 3; k++) {
        dst->nPacked[k] += src->nPacked[k];
        dst->pMaxRefresh[k] = (int32_t)imax(dst->pMaxRefresh[k], src->pMaxRefresh[k]);
        dst->pRingCells[k] = imax(dst->pRingCells[k], src->pRingCells[k]);
        dst->pFbCells[k] = imax(dst->pFbCells[k], src->pFbCells[k]);
    }
    for (int k = 0; k < CPK_WIDE_CLASSES; k++) {
        dst->nWide[k] += src->nWide[k];
        dst->wMaxWidth[k] = (int32_t)imax(dst->wMaxWidth[k], src->wMaxWidth[k]);
        dst->wMaxRefresh[k] = (int32_t)imax(dst->wMaxRefresh[k], src->wMaxRefresh[k]);
        dst->wRingCells[k] = imax(dst->wRingCells[k], src->wRingCells[k]);
        dst->wFbCells[k] = imax(dst->wFbCells[k], src->wFbCells[k]);
        dst->wSeqLdsBytes[k] = (int32_t)imax(dst->wSeqLdsBytes[k], src->wSeqLdsBytes[k]);
        dst->wWinLdsBytes[k] = (int32_t)imax(dst->wWinLdsBytes[k], src->wWinLdsBytes[k]);
    }
}

/* A class that has regions gets scratch of at least one cell and one refresh point. */
static void geometry_clamp(CpkGeometry *geo) {
    for (int k = 0; k < 3; k++)
        if (geo->nPacked[k]) {
            if (geo->pMaxRefresh[k] < 1) geo->pMaxRefresh[k] = 1;
            if (geo->pRingCells[k] < 1) geo->pRingCells[k] = 1;
            if (geo->pFbCells[k] < 1) geo->pFbCells[k] = 1;
        }
    for (int k = 0; k < CPK_WIDE_CLASSES; k++)
        if (geo->nWide[k]) {
            if (geo->emit == CPECAN_EMIT_FORWARD) { /* no traceback: nothing is kept of the forward matrix */
                geo->wRingCells[k] = 1;
                geo->wFbCells[k] = 1;
            }
            if (geo->wMaxRefresh[k] < 1) geo->wMaxRefresh[k] = 1;
            if (geo->wRingCells[k] < 1) geo->wRingCells[k] = 1;
            if (geo->wFbCells[k] < 1) geo->wFbCells[k] = 1;
        }
}

/* Device region di = host region keys[di].index: what its entry holds of its own, and its segments' output slices.
 * Returns 0, or the size of an output slice that does not fit 32 bits. */
static int64_t layout_region(cpecan_batch *b, HostPlan *hp, int64_t di) {
    const int64_t hiRegion = hp->keys[di].index;
    HostRegion *r = &b->regions[hiRegion];
    const RegionPlan *pl = &hp->plan[hiRegion];
    CpkRegion *g = &hp->devRegions[di];
    r->devIndex = di;
    hp->devToHost[di] = hiRegion;
    g->seqXOff = r->seqXOff;
    g->seqYOff = r->seqYOff;
    g->diagOff = hp->diagStart[hiRegion];
    g->segOff = hp->segStart[hiRegion];
    g->anchorOff = r->anchorOff;
    g->nAnchors = (int32_t)r->nAnchors;
    g->nSeg = (int32_t)pl->nSeg;
    g->lX = (int32_t)r->lX;
    g->lY = (int32_t)r->lY;
    g->raggedLeft = r->raggedLeft;
    g->raggedRight = r->raggedRight;
    g->maxWidth = (int32_t)pl->maxW;
    g->absOk = pl->smooth;
    /* ring: diagonals are laid down one after another and never straddle the end of the ring */
    g->ringCap = (int32_t)imin(pl->liveMax + pl->maxW, ((int64_t)1 << 31) - 1);
    g->cells = r->cells;
    g->outCap = (int32_t)default_out_cap(b, r);
    /* every traceback segment gets a part of the region's output slice of its own (used when the segments run as
     * separate queue items, see CpkItem): in proportion to its emitted diagonals, the parts add up to outCap */
    CpkSegment *sg = hp->segs + hp->segStart[hiRegion];
    const int64_t N = r->lX + r->lY;
    int64_t at = 0;
    for (int64_t si = 0; si < pl->nSeg; si++) {
        int64_t cap = N > 0 ? (int64_t)g->outCap * (sg[si].tbFrom - sg[si].tbPrev) / N + 16 : 1;
        /* every cell may be emitted: the cells of the segment's own emitted diagonals (round 3 gave every segment
         * the whole region's cells, nSeg times what the slice can ever hold) */
        if (b->params.threshold <= 0.0) cap = sg[si].emitCells;
        sg[si].outOff = (int32_t)at;
        sg[si].outCap = (int32_t)cap;
        at += cap;
    }
    if (at > ((int64_t)1 << 31) - 1) return at;
    if (at > g->outCap) g->outCap = (int32_t)at;
    return 0;
}

/* One region into a thread's class counts and maxima: its own class only, this runs once per region of the batch
 * (geometry_merge, over every class, joins the threads). */
static void geometry_add_region(CpkGeometry *lg, int cls, const HostRegion *r, const RegionPlan *pl) {
    if (cls < 3) { /* narrow: scratch of the packed kernel's sub-slots */
        const int k = cls;
        lg->nPacked[k]++;
        lg->pMaxRefresh[k] = (int32_t)imax(lg->pMaxRefresh[k], pl->refreshMax);
        lg->pRingCells[k] = imax(lg->pRingCells[k], pl->liveMax + pl->maxW);
        lg->pFbCells[k] = imax(lg->pFbCells[k], pl->fbMax);
    } else {
        const int k = cls - 3;
        lg->nWide[k]++;
        lg->wMaxWidth[k] = (int32_t)imax(lg->wMaxWidth[k], (int32_t)pl->maxW);
        lg->wMaxRefresh[k] = (int32_t)imax(lg->wMaxRefresh[k], pl->refreshMax);
        lg->wRingCells[k] = imax(lg->wRingCells[k], pl->liveMax + pl->maxW);
        lg->wFbCells[k] = imax(lg->wFbCells[k], pl->fbMax);
        lg->wSeqLdsBytes[k] = (int32_t)imax(lg->wSeqLdsBytes[k], imin((r->lX + 3) / 2 + (r->lY + 3) / 2, (int64_t)1 << 30));
        lg->wWinLdsBytes[k] = (int32_t)imax(lg->wWinLdsBytes[k], imin(pl->winBytes, (int64_t)1 << 30));
    }
}

/* The regions in device order: CpkRegion entries, every segment's output slice, the running offsets and the class
 * geometry.  Two passes: what a region's entry holds of its own (the regions are visited in sorted order, i.e. at random
 * in memory: on one thread this loop was 6-9 ms of every config-4 batch), then the running offsets and the class maxima. */
static int layout_device_order(cpecan_batch *b, HostPlan *hp, CpkGeometry *geo) {
    hp->devRegions = host_zalloc((size_t)b->nRegions, sizeof(CpkRegion));
    hp->devToHost = cpk_host_alloc(sizeof(int64_t) * (size_t)b->nRegions);
    if (!hp->devRegions || !hp->devToHost) return CPECAN_ENOMEM;
    memset(geo, 0, sizeof *geo);
    geo->nRegions = (int32_t)b->nRegions;
    geo->nStates = is_five(b->model.type) ? 5 : 3;
    geo->emit = b->emit;
    geo->debug = b->debug;
    int64_t tooLarge = -1;
#pragma omp parallel num_threads(cpk_host_threads()) if (b->nRegions >= 4096)
    {
        CpkGeometry lg; /* this thread's class counts and maxima */
        memset(&lg, 0, sizeof lg);
#pragma omp for schedule(static)
        for (int64_t di = 0; di < b->nRegions; di++) {
            const int64_t at = layout_region(b, hp, di);
            if (at) {
#pragma omp critical(cpk_order)
                if (at > tooLarge) tooLarge = at;
                continue;
            }
            geometry_add_region(&lg, hp->keys[di].cls, &b->regions[hp->keys[di].index], &hp->plan[hp->keys[di].index]);
        }
#pragma omp critical(cpk_order)
        geometry_merge(geo, &lg);
    }
    if (tooLarge >= 0) {
        /* segment offsets and the region's slice are 32-bit: threshold <= 0 on a region of more than 2^31 cells x
         * segments cannot be laid out (the reference would return a list of that many tuples) */
        cpk_set_error("a region's output slice exceeds 2^31 triples (%lld): raise the threshold or split the region", (long long)tooLarge);
        return CPECAN_EINVAL;
    }
    int64_t outAt = 0, dbgCells = 0, dbgDiags = 0;
    for (int64_t di = 0; di < b->nRegions; di++) { /* the running offsets, in device order */
        CpkRegion *g = &hp->devRegions[di];
        g->dbgCellOff = dbgCells;
        g->dbgDiagOff = dbgDiags;
        if (b->debug) {
            dbgCells += g->cells;
            dbgDiags += (int64_t)g->lX + g->lY + 1;
        }
        hp->totalCells += g->cells;
        g->outOff = outAt;
        outAt += g->outCap;
    }
    geometry_clamp(geo);
    /* the scalar geometry (maxWidth, rollStride, ringCells, ..., useGlobalRoll) is filled per launch from the class
     * arrays by the device side (cpk_class_geometry) */
    hp->outTriples = outAt < 1 ? 1 : outAt;
    hp->dbgCells = dbgCells < 1 ? 1 : dbgCells;
    hp->dbgDiags = dbgDiags < 1 ? 1 : dbgDiags;
    return CPECAN_OK;
}

/* The planned batch as the device layer is told about it (CpkBatchPlan, cpecan_internal.h): the one place that spells the
 * batch's fields out.  The arrays stay where they are -- the batch's and, until host_plan_commit, the plan's. */
static CpkBatchPlan batch_plan_record(const cpecan_batch *b, const HostPlan *hp, const CpkGeometry *geo) {
    const int runs = b->runForm == 1;
    return (CpkBatchPlan){.geo = *geo, .regions = hp->devRegions, .segs = hp->segs, .nSegs = hp->nSegs, .nDiags = hp->totalDiags,
                          .anchors = runs ? NULL : b->anchors, .anchorStride = b->anchorStride, .nAnchors = b->nAnchorVals / b->anchorStride,
                          .runs = runs ? b->runs : NULL, .nRuns = runs ? b->nRunVals / 4 : 0, .expansion = b->params.diagonalExpansion,
                          .dynamic = hp->dynamic, .symbols = b->symbols, .nSymbolBytes = b->nSymbols, .outTriplesPerList = hp->outTriples,
                          .nLists = b->nLists, .dbgCells = hp->dbgCells, .dbgDiags = hp->dbgDiags, .modelSlots = b->modelSlots};
}

/* Everything an upload decides before a device is involved; integers only.  On failure the caller frees hp all the same. */
static int batch_plan(cpecan_batch *b, HostPlan *hp, CpkBatchPlan *plan, CpkModel *km) {
    CpkGeometry geo;
    const double t0 = now_ms();
    int rc = host_plan_init(b, hp);
    if (rc == CPECAN_OK) rc = plan_regions(b, hp);
    if (rc != CPECAN_OK) return rc;
    const double t1 = now_ms();
    classify_regions(b, hp);
    const double t2 = now_ms();
    sort_cost_keys(hp->keys, b->nRegions);
    const double t3 = now_ms();
    rc = layout_device_order(b, hp, &geo);
    if (rc != CPECAN_OK) return rc;
    *plan = batch_plan_record(b, hp, &geo);
    kernel_model(&b->model, b->params.threshold, km);
    const double t4 = now_ms();
    if (trace_host())
        fprintf(stderr, "cpecan upload: %lld regions, %lld segment slots: band walk %.1f ms, classes %.1f, sort %.1f, device order %.1f\n",
                (long long)b->nRegions, (long long)hp->nSegs, t1 - t0, t2 - t1, t3 - t2, t4 - t3);
    return CPECAN_OK;
}

static uint64_t fnv1a64(const void *data, size_t n, uint64_t h) {
    const unsigned char *p = data;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

/* For tests, no device needed: plans an unfrozen batch as cpecan_batch_upload would and hashes (FNV-1a, 64 bits) the
 * whole plan -- the CpkRegion array in device order, devToHost, every segment slot, and the geometry with outTriples,
 * nDiags, dbgCells and dbgDiags.  The plan is dropped; of the batch only what every plan rewrites (a region's cell
 * count and device index) is touched. */
int cpk_batch_plan_digest(cpecan_batch *b, uint64_t out[4]) {
    if (!b || !out || b->frozen || dl_busy(b)) return CPECAN_ESTATE;
    const uint64_t seed = 0xcbf29ce484222325ull;
    out[0] = out[1] = out[2] = out[3] = seed;
    if (b->nRegions == 0) return CPECAN_OK;
    HostPlan hp;
    CpkBatchPlan plan;
    CpkModel km;
    const int rc = batch_plan(b, &hp, &plan, &km);
    if (rc == CPECAN_OK) {
        const int64_t totals[4] = {hp.outTriples, hp.totalDiags, hp.dbgCells, hp.dbgDiags};
        out[0] = fnv1a64(hp.devRegions, sizeof(CpkRegion) * (size_t)b->nRegions, seed);
        out[1] = fnv1a64(hp.devToHost, sizeof(int64_t) * (size_t)b->nRegions, seed);
        out[2] = fnv1a64(hp.segs, sizeof(CpkSegment) * (size_t)hp.nSegs, seed);
        out[3] = fnv1a64(totals, sizeof totals, fnv1a64(&plan.geo, sizeof plan.geo, seed));
    }
    host_plan_free(&hp);
    return rc;
}

/* For tests: what the add calls packed into the batch (cpecan_internal.h), field by field where a record holds pointers or
 * padding; reads only. */
int cpk_batch_intake_digest(const cpecan_batch *b, uint64_t out[5]) {
    if (!b || !out || dl_busy(b)) return CPECAN_ESTATE;
    const uint64_t seed = 0xcbf29ce484222325ull;
    const int64_t form[2] = {b->runForm, b->anchorStride};
    const int keepRuns = b->runForm == 1;
    out[0] = out[1] = seed;
    out[3] = fnv1a64(form, sizeof form, seed);
    for (int64_t i = 0; i < b->nProblems; i++) {
        const HostProblem *pr = &b->problems[i];
        const int64_t f[7] = {pr->firstRegion, pr->nRegions, pr->lX, pr->lY, pr->charX, pr->charY, pr->minus};
        out[0] = fnv1a64(f, sizeof f, out[0]);
    }
    for (int64_t i = 0; i < b->nRegions; i++) {
        const HostRegion *r = &b->regions[i];
        const int64_t f[11] = {r->problem, r->x1, r->y1, r->lX, r->lY, r->seqXOff, r->seqYOff, r->anchorOff, r->nAnchors, r->raggedLeft, r->raggedRight};
        const int64_t runs[2] = {r->runOff, r->nRuns};
        out[1] = fnv1a64(f, sizeof f, out[1]);
        if (keepRuns) out[3] = fnv1a64(runs, sizeof runs, out[3]);
    }
    out[2] = fnv1a64(b->symbols, (size_t)b->nSymbols, seed);
    out[3] = fnv1a64(keepRuns ? b->runs : b->anchors, sizeof(int32_t) * (size_t)(keepRuns ? b->nRunVals : b->nAnchorVals), out[3]);
    out[4] = fnv1a64(b->chars, (size_t)b->nChars, seed);
    return CPECAN_OK;
}

/* For tests, no device needed: the launches cpecan_batch_upload would plan on a device of numCUs compute units.
 * (The launch plan lives in the device layer; a program that links this file against a stand-in for that layer need not
 * have it: a weak reference, CPECAN_ESTATE without it.) */
extern __typeof__(cpk_plan_describe) cpk_plan_describe __attribute__((weak));
int cpk_batch_launch_plan(cpecan_batch *b, int numCUs, int64_t memBytes, int64_t *out, int maxClasses) {
    if (!b || !out || b->frozen || dl_busy(b) || !cpk_plan_describe) return CPECAN_ESTATE;
    if (b->nRegions == 0) return 0;
    HostPlan hp;
    CpkBatchPlan plan;
    CpkModel km;
    int rc = batch_plan(b, &hp, &plan, &km);
    if (rc == CPECAN_OK) rc = cpk_plan_describe(&plan, numCUs, memBytes, out, maxClasses);
    host_plan_free(&hp);
    return rc;
}
/* ... and the chains of that plan with its traceback queues (cpecan_internal.h). */
extern __typeof__(cpk_plan_chains) cpk_plan_chains __attribute__((weak));
int cpk_batch_chain_plan(cpecan_batch *b, int numCUs, int64_t memBytes, int64_t *chainsOut, int maxClasses, int64_t *itemsOut,
                         int64_t maxItems, int64_t *nItems) {
    if (!b || !chainsOut || b->frozen || dl_busy(b) || !cpk_plan_chains) return CPECAN_ESTATE;
    if (nItems) *nItems = 0;
    if (b->nRegions == 0) return 0;
    HostPlan hp;
    CpkBatchPlan plan;
    CpkModel km;
    int rc = batch_plan(b, &hp, &plan, &km);
    if (rc == CPECAN_OK) rc = cpk_plan_chains(&plan, numCUs, memBytes, chainsOut, maxClasses, itemsOut, maxItems, nItems);
    host_plan_free(&hp);
    return rc;
}

/* For tests: the launches the uploaded batch really has, as its device planned them (cpk_plan_describe's numbers).
 * (A weak reference, as cpk_plan_describe above: a stand-in for the device layer need not have it.) */
extern __typeof__(cpk_device_launch_forms) cpk_device_launch_forms __attribute__((weak));
int cpk_batch_launch_forms(cpecan_batch *b, int64_t *out, int maxClasses) {
    if (!b || !out || !b->frozen || dl_busy(b) || !cpk_device_launch_forms) return CPECAN_ESTATE;
    if (b->nRegions == 0 || !b->dev) return 0;
    return cpk_device_launch_forms(b->dev, out, maxClasses);
}

int cpecan_batch_upload(cpecan_batch *b) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || b->frozen) return CPECAN_ESTATE;
    if (b->nRegions == 0) {
        if (cpk_device_count() < 1) {
            cpk_set_error("no usable HIP device: the HIP path has no CPU fallback");
            return CPECAN_ENODEVICE;
        }
        b->frozen = 1;
        return CPECAN_OK;
    }
    HostPlan hp;
    CpkBatchPlan plan;
    CpkModel km;
    int rc = batch_plan(b, &hp, &plan, &km);
    if (rc == CPECAN_OK) {
        b->stats.problems = b->nProblems;
        b->stats.regions = b->nRegions;
        b->stats.cells = hp.totalCells;
        b->stats.diagonals = hp.totalDiags;
        if (!b->dev) rc = cpk_device_create(&b->dev, b->device); /* fails with CPECAN_ENODEVICE when there is no GPU */
    }
    if (rc == CPECAN_OK) rc = cpk_device_upload(b->dev, &plan, &km, &b->stats.h2dMs);
    if (rc == CPECAN_OK) {
        b->stats.deviceBytes = cpk_device_bytes(b->dev);
        b->stats.wavesPerLaunch = cpk_device_waves(b->dev);
        b->stats.launchForm = cpk_device_form(b->dev);
        host_plan_commit(b, &hp, &plan.geo);
        b->frozen = 1;
    }
    host_plan_free(&hp);
    return rc;
}

int cpecan_batch_run(cpecan_batch *b, void *stream) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->frozen) return CPECAN_ESTATE;
    b->downloaded = 0;
    if (b->nRegions == 0) {
        b->ran = 1;
        return CPECAN_OK;
    }
    int rc = cpk_device_run(b->dev, stream);
    if (rc == CPECAN_OK) {
        b->ran = 1;
        b->stats.launches = 1;
    }
    return rc;
}

int cpecan_batch_reserve_models(cpecan_batch *b, int nSlots) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b) return CPECAN_EINVAL;
    if (b->frozen) {
        cpk_set_error("reserve_models after upload");
        return CPECAN_ESTATE;
    }
    if (b->emit != CPECAN_EMIT_EXPECT && b->emit != CPECAN_EMIT_FORWARD) {
        cpk_set_error("reserve_models: only CPECAN_EMIT_EXPECT and CPECAN_EMIT_FORWARD batches take model slots (emitter %d returns lists)", b->emit);
        return CPECAN_EINVAL;
    }
    if (nSlots < 1 || nSlots > CPECAN_MAX_MODEL_SLOTS) {
        cpk_set_error("reserve_models: %d slots, 1 to %d are possible", nSlots, CPECAN_MAX_MODEL_SLOTS);
        return CPECAN_EINVAL;
    }
    b->modelSlots = nSlots;
    return CPECAN_OK;
}

int cpecan_batch_set_models(cpecan_batch *b, const cpecan_model *models, int n) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !models) return CPECAN_EINVAL;
    if (n < 1 || n > CPECAN_MAX_MODEL_SLOTS) { /* before models[] is read */
        cpk_set_error("set_models: %d models, 1 to %d are possible", n, CPECAN_MAX_MODEL_SLOTS);
        return CPECAN_EINVAL;
    }
    for (int k = 0; k < n; k++) {
        const cpecan_model *m = &models[k];
        if (!(is_five(m->type) || is_three(m->type)) || is_five(m->type) != is_five(b->model.type)) {
            cpk_set_error("set_models: a model of %d states for a batch planned for %d", is_five(m->type) ? 5 : 3,
                          is_five(b->model.type) ? 5 : 3);
            return CPECAN_EINVAL;
        }
    }
    if (!b->frozen) {
        cpk_set_error("set_models before upload");
        return CPECAN_ESTATE;
    }
    if (n > (b->modelSlots > 0 ? b->modelSlots : 1)) {
        cpk_set_error("set_models: %d models for a batch that reserved %d", n, b->modelSlots);
        return CPECAN_EINVAL;
    }
    if (b->nRegions > 0) {
        CpkModel km[CPECAN_MAX_MODEL_SLOTS];
        for (int k = 0; k < n; k++) kernel_model(&models[k], b->params.threshold, &km[k]);
        const int rc = cpk_device_set_models(b->dev, km, n);
        if (rc != CPECAN_OK) return rc;
        b->stats.wavesPerLaunch = cpk_device_waves(b->dev); /* a reserved batch: the waves of a run grow with its models */
    }
    b->model = models[0];
    b->activeModels = n;
    b->ran = 0; /* a run not downloaded yet belongs to the old models: the next download needs a new run */
    return CPECAN_OK;
}

int cpecan_batch_set_model(cpecan_batch *b, const cpecan_model *m) {
    if (!b || !m) return dl_busy(b) ? CPECAN_ESTATE : CPECAN_EINVAL;
    return cpecan_batch_set_models(b, m, 1);
}

/* The copy plan of cpk_device_gather for the whole batch: per list, problems in order, regions in order, traceback
 * segments in DEScending order (each traceback's pairs are prepended, pairwiseAligner.c:1415-1417), every triple shifted
 * by its region's offset (:1411-1418).  Sets the per-problem result pointers into b->results. */
static int plan_results(cpecan_batch *b, const int32_t *counts, const int32_t *segStarts, const int32_t *segCounts,
                        CpkChunk **chunksOut, int64_t *nChunksOut, int64_t *totalOut, int32_t **chunkRegionOut,
                        int32_t **chunkProblemOut, int64_t *nChunks0Out) {
    int64_t total = 0;
    for (int l = 0; l < b->nLists; l++)
        for (int64_t di = 0; di < b->nRegions; di++) total += counts[(size_t)l * b->nRegions + di];
    CpkChunk *chunks = cpk_host_alloc(sizeof(CpkChunk) * (size_t)(b->nLists * (b->nSegs ? b->nSegs : 1)));
    b->results = cpk_host_alloc(sizeof(int32_t) * 3 * (size_t)(total ? total : 1));
    /* the band-edge statistic (cpk_device_band_edge): device region and problem of every list-0 chunk, beside the list */
    int32_t *chunkRegion = NULL, *chunkProblem = NULL;
    if (b->bandEdge) {
        chunkRegion = malloc(sizeof(int32_t) * (size_t)(b->nSegs ? b->nSegs : 1));
        chunkProblem = malloc(sizeof(int32_t) * (size_t)(b->nSegs ? b->nSegs : 1));
    }
    if (!chunks || !b->results || (b->bandEdge && (!chunkRegion || !chunkProblem))) {
        cpk_host_free(chunks);
        free(chunkRegion);
        free(chunkProblem);
        return CPECAN_ENOMEM;
    }
    int64_t nChunks = 0, at = 0;
    *nChunks0Out = 0;
    for (int l = 0; l < b->nLists; l++) {
        const int32_t *cnt = counts + (size_t)l * b->nRegions;
        const int32_t *ss = segStarts + (size_t)l * b->nSegs;
        const int32_t *sc = segCounts + (size_t)l * b->nSegs;
        for (int64_t pi = 0; pi < b->nProblems; pi++) {
            HostProblem *pr = &b->problems[pi];
            pr->triples[l] = b->results + 3 * at;
            const int64_t first = at;
            for (int64_t i = 0; i < pr->nRegions; i++) {
                const HostRegion *r = &b->regions[pr->firstRegion + i];
                const CpkRegion *g = &b->devRegions[r->devIndex];
                const int32_t n = cnt[r->devIndex];
                for (int sgi = g->nSeg - 1; sgi >= 0; sgi--) {
                    const int32_t from = ss[g->segOff + sgi];
                    /* a split region's segments were written apart, each with its own count */
                    const int32_t to = g->split ? from + sc[g->segOff + sgi] : (sgi + 1 < g->nSeg ? ss[g->segOff + sgi + 1] : n);
                    if (to <= from) continue;
                    if (l == 0 && chunkRegion) {
                        chunkRegion[nChunks] = (int32_t)r->devIndex;
                        chunkProblem[nChunks] = (int32_t)pi;
                    }
                    CpkChunk *c = &chunks[nChunks++];
                    c->src = (int64_t)l * b->outTriples + g->outOff + from;
                    c->dst = at;
                    c->len = to - from;
                    c->dx = (int32_t)r->x1;
                    c->dy = (int32_t)r->y1;
                    c->pad = 0;
                    at += to - from;
                }
            }
            pr->nTriples[l] = at - first;
        }
        if (l == 0) *nChunks0Out = nChunks;
    }
    *chunkRegionOut = chunkRegion;
    *chunkProblemOut = chunkProblem;
    *chunksOut = chunks;
    *nChunksOut = nChunks;
    *totalOut = at;
    return CPECAN_OK;
}

/* Fills one consumer descriptor per problem and the scratch totals of the job. */
static void post_layout(CpkPostJob *job, CpkPostProblem *pp, int64_t i, const int64_t off[3], const int64_t n[3],
                        int64_t lX, int64_t lY, int64_t charX, int64_t charY) {
    memset(pp, 0, sizeof *pp);
    for (int l = 0; l < 3; l++) {
        pp->off[l] = off[l];
        pp->n[l] = (int32_t)n[l];
    }
    pp->lX = (int32_t)lX;
    pp->lY = (int32_t)lY;
    pp->seqOff = job->seqSlots;
    pp->chainOff = job->chainSlots;
    pp->charX = charX;
    pp->charY = charY;
    pp->meaOut = job->meaCap;
    pp->shiftOut = job->shiftCap;
    job->seqSlots += lX + 2 * lY; /* ORDERED: column heads + the staircase's two arrays; the other consumers use lX + lY */
    job->chainSlots += n[0] + 1;
    job->meaCap += n[0];
    job->shiftCap += n[0] + imin(lX, lY) + 1;
    pp->nextOff = job->nextSlots;
    job->nextSlots += 2 * lX;
    (void)i;
}

static int run_post(cpecan_batch *b) {
    CpkPostJob job;
    memset(&job, 0, sizeof job);
    job.flags = b->postFlags;
    job.gapGamma = b->postGapGamma;
    job.matchGamma = (double)b->postMatchGamma; /* float widened, as the reference passes it (multipleAligner.c:945) */
    job.nProblems = b->nProblems;
    CpkPostProblem *pp = malloc(sizeof(CpkPostProblem) * (size_t)(b->nProblems ? b->nProblems : 1));
    double *scores = malloc(sizeof(double) * CPK_POST_SCORES * (size_t)(b->nProblems ? b->nProblems : 1));
    int32_t *counts = malloc(sizeof(int32_t) * 2 * (size_t)(b->nProblems ? b->nProblems : 1));
    int rc = (pp && scores && counts) ? CPECAN_OK : CPECAN_ENOMEM;
    for (int64_t i = 0; rc == CPECAN_OK && i < b->nProblems; i++) {
        const HostProblem *pr = &b->problems[i];
        int64_t off[3] = {0, 0, 0}, n[3] = {0, 0, 0};
        for (int l = 0; l < b->nLists; l++) {
            off[l] = (pr->triples[l] - b->results) / 3;
            n[l] = pr->nTriples[l];
        }
        post_layout(&job, &pp[i], i, off, n, pr->lX, pr->lY, pr->charX, pr->charY);
    }
    if (rc == CPECAN_OK) {
        job.problems = pp;
        job.scores = scores;
        job.counts = counts;
        /* identity scores and the left shift compare letters; neither exists without a consumer (cpecan_batch_identity_scores) */
        job.chars = job.flags ? b->chars : NULL;
        job.nChars = job.flags ? b->nChars : 0;
        if ((job.flags & (CPECAN_POST_MEA | CPECAN_POST_ORDERED)) && !b->nextRuns) { /* (with the next-runs stage list 3 stays on the device) */
            b->postMea = cpk_host_alloc(sizeof(int32_t) * 3 * (size_t)(job.meaCap ? job.meaCap : 1));
            job.mea = b->postMea;
            if (!b->postMea) rc = CPECAN_ENOMEM;
        }
        if (rc == CPECAN_OK && (job.flags & CPECAN_POST_LEFT_SHIFT)) {
            b->postShift = cpk_host_alloc(sizeof(int32_t) * 3 * (size_t)(job.shiftCap ? job.shiftCap : 1));
            job.shift = b->postShift;
            if (!b->postShift) rc = CPECAN_ENOMEM;
        }
    }
    if (rc == CPECAN_OK && b->quintNames) { /* the quintuple stage: list 0 of every problem as records, and their score sums */
        b->quints = cpk_host_alloc(sizeof(int32_t) * 5 * (size_t)(job.meaCap ? job.meaCap : 1));
        b->quintOffsets = malloc(sizeof(int64_t) * (size_t)(b->nProblems + 1));
        b->quintSums = calloc((size_t)(b->nProblems ? b->nProblems : 1), sizeof(int64_t));
        b->quintStageMs = 0.0;
        if (!b->quints || !b->quintOffsets || !b->quintSums) rc = CPECAN_ENOMEM;
        job.names = b->quintNames;
        job.quints = b->quints;
        job.sums = b->quintSums;
        job.stageMs = &b->quintStageMs;
    }
    int32_t *runCounts = NULL, *runVals = NULL;
    if (rc == CPECAN_OK && b->nextRuns) { /* the next-runs stage: list 3 of every problem as the anchor runs of the next E-step */
        runCounts = malloc(sizeof(int32_t) * (size_t)(b->nProblems ? b->nProblems : 1));
        b->nextRunOffsets = calloc((size_t)(b->nProblems + 1), sizeof(int64_t));
        b->nextStageMs = 0.0;
        if (!runCounts || !b->nextRunOffsets) rc = CPECAN_ENOMEM;
        job.nextRuns = 1;
        job.nextTrim = (int32_t)(b->nextTrim < ((int64_t)1 << 30) ? b->nextTrim : ((int64_t)1 << 30)); /* longer than any sequence */
        job.nextExpansion = (int32_t)b->nextExpansion;
        job.runCounts = runCounts;
        job.runOffsets = b->nextRunOffsets;
        job.runsOut = &runVals;
        job.nextMs = &b->nextStageMs;
    }
    if (rc == CPECAN_OK) rc = cpk_device_post(b->dev, &job);
    if (rc == CPECAN_OK && b->nextRuns) { /* widened to what cpecan_batch_add_many_runs takes */
        const int64_t total = 4 * b->nextRunOffsets[b->nProblems];
        b->nextRunVals = malloc(sizeof(int64_t) * (size_t)(total ? total : 1));
        if (!b->nextRunVals) rc = CPECAN_ENOMEM;
        for (int64_t k = 0; rc == CPECAN_OK && k < total; k++) b->nextRunVals[k] = runVals[k];
    }
    cpk_host_free(runVals);
    free(runCounts);
    if (rc == CPECAN_OK && b->quintNames) {
        for (int64_t i = 0; i < b->nProblems; i++) b->quintOffsets[i] = pp[i].meaOut;
        b->quintOffsets[b->nProblems] = job.meaCap;
    }
    for (int64_t i = 0; rc == CPECAN_OK && i < b->nProblems; i++) {
        HostProblem *pr = &b->problems[i];
        for (int k = 0; k < CPK_POST_SCORES; k++) pr->scores[k] = scores[CPK_POST_SCORES * i + k];
        if (job.flags & CPECAN_POST_LEFT_SHIFT) {
            pr->triples[3] = b->postShift + 3 * pp[i].shiftOut;
            pr->nTriples[3] = counts[2 * i + 1];
        } else if (b->nextRuns) {
            pr->nTriples[3] = counts[2 * i];
        } else if (job.flags & (CPECAN_POST_MEA | CPECAN_POST_ORDERED)) {
            pr->triples[3] = b->postMea + 3 * pp[i].meaOut;
            pr->nTriples[3] = counts[2 * i];
        }
    }
    free(pp);
    free(scores);
    free(counts);
    return rc;
}

int cpecan_batch_set_post(cpecan_batch *b, int flags, double gapGamma) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b) return CPECAN_EINVAL;
    if (flags & ~(CPECAN_POST_REWEIGHT | CPECAN_POST_MEA | CPECAN_POST_LEFT_SHIFT | CPECAN_POST_ORDERED)) return CPECAN_EINVAL;
    if ((flags & CPECAN_POST_LEFT_SHIFT) && !(flags & CPECAN_POST_MEA)) return CPECAN_EINVAL;
    if ((flags & CPECAN_POST_ORDERED) && (flags & (CPECAN_POST_MEA | CPECAN_POST_LEFT_SHIFT))) return CPECAN_EINVAL;
    if ((flags & CPECAN_POST_MEA) && (flags & CPECAN_POST_REWEIGHT)) return CPECAN_EINVAL; /* alternatives in the reference */
    if ((flags & CPECAN_POST_MEA) && b->emit != CPECAN_EMIT_INDEL) {
        cpk_set_error("the MEA alignment needs the gap lists: create the batch with CPECAN_EMIT_INDEL");
        return CPECAN_EINVAL;
    }
    if (flags && (b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT)) return CPECAN_EINVAL;
    b->postFlags = flags;
    b->postGapGamma = gapGamma;
    if (!(flags & CPECAN_POST_ORDERED)) b->nextRuns = 0; /* the next-runs stage goes with the list it reads */
    return CPECAN_OK;
}

int cpecan_batch_set_quintuples(cpecan_batch *b, const int32_t *names, int64_t nProblems) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b) return CPECAN_EINVAL;
    if (!names) {
        free(b->quintNames);
        b->quintNames = NULL;
        return CPECAN_OK;
    }
    if (b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT) {
        cpk_set_error("quintuples are made of the pair lists: EXPECT and FORWARD batches have none");
        return CPECAN_EINVAL;
    }
    if (nProblems != b->nProblems) {
        cpk_set_error("cpecan_batch_set_quintuples: names for %lld problems, the batch holds %lld", (long long)nProblems,
                      (long long)b->nProblems);
        return CPECAN_EINVAL;
    }
    int32_t *copy = malloc(sizeof(int32_t) * 2 * (size_t)(nProblems ? nProblems : 1));
    if (!copy) return CPECAN_ENOMEM;
    if (nProblems) memcpy(copy, names, sizeof(int32_t) * 2 * (size_t)nProblems);
    free(b->quintNames);
    b->quintNames = copy;
    return CPECAN_OK;
}

int cpecan_batch_quintuples(const cpecan_batch *b, const int32_t **quints, const int64_t **offsets, const int64_t **sums) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (!b->quints) {
        cpk_set_error("quintuples were not asked for: cpecan_batch_set_quintuples before the download");
        return CPECAN_ESTATE;
    }
    if (quints) *quints = b->quints;
    if (offsets) *offsets = b->quintOffsets;
    if (sums) *sums = b->quintSums;
    return CPECAN_OK;
}

int cpk_batch_take_quintuples(cpecan_batch *b, int32_t **quints, int64_t **offsets, int64_t **sums, double *stageMs) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded || !b->quints) return CPECAN_ESTATE;
    *quints = b->quints;
    *offsets = b->quintOffsets;
    *sums = b->quintSums;
    if (stageMs) *stageMs = b->quintStageMs;
    b->quints = NULL;
    b->quintOffsets = b->quintSums = NULL;
    b->downloaded = 0; /* the run's results have left the batch */
    return CPECAN_OK;
}

/* ---- the next-runs stage (include/cpecan_realign.h) ---- */
int cpecan_batch_set_next_runs(cpecan_batch *b, int64_t trim, int64_t expansion) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b) return CPECAN_EINVAL;
    if (b->frozen) {
        cpk_set_error("cpecan_batch_set_next_runs: before upload");
        return CPECAN_EINVAL;
    }
    if (expansion == CPECAN_NEXT_RUNS_OFF) {
        b->nextRuns = 0;
        return CPECAN_OK;
    }
    if (!(b->postFlags & CPECAN_POST_ORDERED)) {
        cpk_set_error("the next runs are made of the ordered alignment: select CPECAN_POST_ORDERED first");
        return CPECAN_EINVAL;
    }
    if (trim < 0 || expansion < 0 || expansion > INT32_MAX) {
        cpk_set_error("cpecan_batch_set_next_runs: trim %lld, expansion %lld", (long long)trim, (long long)expansion);
        return CPECAN_EINVAL;
    }
    b->nextRuns = 1;
    b->nextTrim = trim;
    b->nextExpansion = expansion;
    return CPECAN_OK;
}

int cpecan_batch_next_runs(const cpecan_batch *b, int64_t problem, const int64_t **runs, int64_t *nRuns) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (!b->nextRunOffsets) {
        cpk_set_error("the next runs were not asked for: cpecan_batch_set_next_runs before the upload");
        return CPECAN_ESTATE;
    }
    if (problem < 0 || problem >= b->nProblems || !runs || !nRuns) return CPECAN_EINVAL;
    *runs = b->nextRunVals + 4 * b->nextRunOffsets[problem];
    *nRuns = b->nextRunOffsets[problem + 1] - b->nextRunOffsets[problem];
    return CPECAN_OK;
}

double cpk_batch_next_runs_ms(const cpecan_batch *b) { return b ? b->nextStageMs : 0.0; }

static int cmp_pair_xy(const void *a, const void *b) {
    const int64_t *p = a, *q = b;
    if (p[0] != q[0]) return p[0] < q[0] ? -1 : 1;
    return p[1] < q[1] ? -1 : (p[1] > q[1] ? 1 : 0);
}

/* The definition of the stage on the host: the pairs sorted, cut into blocks, trimmed, filtered, joined into runs. */
int64_t cpecan_next_runs_of_pairs(const int32_t *triples, int64_t n, const char *sX, int64_t lX, const char *sY, int64_t lY,
                                  int64_t trim, int64_t expansion, int64_t *runs, int64_t cap) {
    if (n < 0 || (n > 0 && !triples) || lX < 0 || lY < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || trim < 0 || expansion < 0 ||
        cap < 0 || (cap > 0 && !runs))
        return CPECAN_EINVAL;
    int64_t *xy = malloc(sizeof(int64_t) * 2 * (size_t)(n ? n : 1));
    if (!xy) return CPECAN_ENOMEM;
    for (int64_t i = 0; i < n; i++) {
        xy[2 * i] = triples[3 * i + 1];
        xy[2 * i + 1] = triples[3 * i + 2];
        if (xy[2 * i] < 0 || xy[2 * i] >= lX || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= lY) {
            free(xy);
            cpk_set_error("cpecan_next_runs_of_pairs: pair %lld lies outside the sequences", (long long)i);
            return CPECAN_EINVAL;
        }
    }
    qsort(xy, (size_t)n, 2 * sizeof(int64_t), cmp_pair_xy);
    for (int64_t i = 1; i < n; i++)
        if (xy[2 * i] <= xy[2 * i - 2] || xy[2 * i + 1] <= xy[2 * i - 1]) {
            free(xy);
            cpk_set_error("cpecan_next_runs_of_pairs: the pairs are no chain");
            return CPECAN_EINVAL;
        }
    int64_t count = 0;
    for (int64_t i = 0; i < n;) {
        int64_t len = 1; /* the block: pairs i .. i + len - 1 */
        while (i + len < n && xy[2 * (i + len)] == xy[2 * i] + len && xy[2 * (i + len) + 1] == xy[2 * i + 1] + len) len++;
        int64_t open = 0; /* columns of the run that is open */
        for (int64_t l = trim; l < len - trim; l++) {
            const int64_t x = xy[2 * i] + l, y = xy[2 * i + 1] + l;
            const uint8_t a = g_upperOf[(unsigned char)sX[x]], c = g_upperOf[(unsigned char)sY[y]];
            if (a != c || a == 'N') {
                open = 0;
                continue;
            }
            if (open == 0) {
                if (count < cap) {
                    runs[4 * count] = x;
                    runs[4 * count + 1] = y;
                    runs[4 * count + 2] = 0;
                    runs[4 * count + 3] = expansion;
                }
                count++;
            }
            open++;
            if (count <= cap) runs[4 * (count - 1) + 2] = open;
        }
        i += len;
    }
    free(xy);
    return count;
}

int cpecan_batch_set_band_edge(cpecan_batch *b, int on) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b) return CPECAN_EINVAL;
    if (b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT) {
        cpk_set_error("the band edge statistic is a function of the pair lists: EXPECT and FORWARD batches have none");
        return CPECAN_EINVAL;
    }
    b->bandEdge = on != 0;
    return CPECAN_OK;
}

int cpecan_batch_band_edge(const cpecan_batch *b, int64_t problem, cpecan_band_edge *out) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (!b->edges) {
        cpk_set_error("the band edge statistic was not asked for: cpecan_batch_set_band_edge before the download");
        return CPECAN_ESTATE;
    }
    if (problem < 0 || problem >= b->nProblems || !out) return CPECAN_EINVAL;
    *out = b->edges[problem];
    return CPECAN_OK;
}

/* The definition of cpecan_band_edge on the host: regions as cpecan_batch_add cuts them, each region's band, every pair
 * against its own anti-diagonal. */
int cpecan_band_edge_of_pairs(const int64_t *anchors, int64_t nAnchors, int64_t lX, int64_t lY, const cpecan_params *p,
                              int raggedLeft, int raggedRight, const int32_t *triples, int64_t n, cpecan_band_edge *out) {
    if (!p || !out || lX < 0 || lY < 0 || nAnchors < 0 || n < 0 || (nAnchors > 0 && !anchors) || (n > 0 && !triples))
        return CPECAN_EINVAL;
    memset(out, 0, sizeof *out);
    int64_t *rects = malloc(sizeof(int64_t) * 4 * (size_t)(nAnchors + 2));
    if (!rects) return CPECAN_ENOMEM;
    const int64_t nRects = cpecan_split_points(anchors, nAnchors, lX, lY, p->splitMatrixBiggerThanThis, raggedLeft, raggedRight, rects);
    int rc = nRects < 0 ? (int)nRects : CPECAN_OK;
    int64_t *own = NULL, *band = NULL, *regionOf = NULL, *first = NULL, *order = NULL;
    if (rc == CPECAN_OK) {
        own = malloc(sizeof(int64_t) * 3 * (size_t)(nAnchors ? nAnchors : 1));
        regionOf = malloc(sizeof(int64_t) * (size_t)(n ? n : 1));
        order = malloc(sizeof(int64_t) * (size_t)(n ? n : 1));
        first = calloc((size_t)nRects + 2, sizeof(int64_t));
        if (!own || !regionOf || !order || !first) rc = CPECAN_ENOMEM;
    }
    /* the rectangles are disjoint and ascend in x and in y: a pair's region is the last one that starts at or left of it */
    for (int64_t i = 0; rc == CPECAN_OK && i < n; i++) {
        const int64_t x = triples[3 * i + 1], y = triples[3 * i + 2];
        int64_t lo = 0, hi = nRects - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (rects[4 * mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        if (nRects == 0 || x < rects[4 * lo] || x >= rects[4 * lo + 2] || y < rects[4 * lo + 1] || y >= rects[4 * lo + 3]) {
            cpk_set_error("cpecan_band_edge_of_pairs: pair %lld (%lld, %lld) lies in no region of the problem", (long long)i,
                          (long long)x, (long long)y);
            rc = CPECAN_EINVAL;
            break;
        }
        regionOf[i] = lo;
        first[lo + 2]++;
    }
    if (rc == CPECAN_OK) { /* the pairs by region: first[k + 1] .. of region k after the scatter */
        for (int64_t k = 0; k < nRects; k++) first[k + 2] += first[k + 1];
        for (int64_t i = 0; i < n; i++) order[first[regionOf[i] + 1]++] = i;
    }
    int64_t next = 0;
    for (int64_t k = 0; rc == CPECAN_OK && k < nRects; k++) {
        const int64_t x1 = rects[4 * k], y1 = rects[4 * k + 1], x2 = rects[4 * k + 2], y2 = rects[4 * k + 3];
        const int64_t rX = x2 - x1, rY = y2 - y1;
        int64_t nOwn = 0; /* anchors go to regions in order (pairwiseAligner.c:1296-1308) */
        for (; next < nAnchors && anchors[3 * next] + anchors[3 * next + 1] < x2 + y2; next++, nOwn++) {
            own[3 * nOwn] = anchors[3 * next] - x1;
            own[3 * nOwn + 1] = anchors[3 * next + 1] - y1;
            own[3 * nOwn + 2] = anchors[3 * next + 2];
        }
        if (first[k] == first[k + 1]) continue; /* no pair in this region */
        int64_t *grown = realloc(band, sizeof(int64_t) * 3 * (size_t)(rX + rY + 1));
        if (!grown) {
            rc = CPECAN_ENOMEM;
            break;
        }
        band = grown;
        rc = cpecan_band(own, nOwn, rX, rY, p->diagonalExpansion, p->dynamicAnchorExpansion != 0, band);
        for (int64_t q = first[k]; rc == CPECAN_OK && q < first[k + 1]; q++) {
            const int64_t i = order[q];
            const int64_t xs = (int64_t)triples[3 * i + 1] - x1, ys = (int64_t)triples[3 * i + 2] - y1;
            const int64_t d = xs + ys + 2, xmy = xs - ys; /* cell (xs + 1, ys + 1) */
            const int left = xmy == band[3 * d + 1] && ys + 2 <= rY;  /* (x - 1, y + 1) is in the matrix; x - 1 >= 0 always */
            const int right = xmy == band[3 * d + 2] && xs + 2 <= rX; /* (x + 1, y - 1) */
            if (left || right) {
                out->edgePairs++;
                out->edgeScoreSum += triples[3 * i];
                if (triples[3 * i] > out->edgeScoreMax) out->edgeScoreMax = triples[3 * i];
            }
        }
    }
    if (rc != CPECAN_OK) memset(out, 0, sizeof *out);
    free(rects);
    free(own);
    free(band);
    free(regionOf);
    free(first);
    free(order);
    return rc;
}

int cpecan_batch_set_match_gamma(cpecan_batch *b, float matchGamma) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !(matchGamma >= 0.0f)) return CPECAN_EINVAL;
    b->postMatchGamma = matchGamma;
    return CPECAN_OK;
}

int cpecan_batch_identity_scores(const cpecan_batch *b, int64_t problem, double *byIdentity, double *byIdentityIgnoringGaps) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (problem < 0 || problem >= b->nProblems || b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT)
        return CPECAN_EINVAL;
    if (!b->postFlags) {
        cpk_set_error("identity scores are computed by the consumer stage: select one with cpecan_batch_set_post");
        return CPECAN_ESTATE;
    }
    if (byIdentity) *byIdentity = b->problems[problem].scores[3];
    if (byIdentityIgnoringGaps) *byIdentityIgnoringGaps = b->problems[problem].scores[4];
    return CPECAN_OK;
}

int cpecan_batch_scores(const cpecan_batch *b, int64_t problem, double *byPosterior, double *byPosteriorIgnoringGaps,
                        double *meaScore) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (problem < 0 || problem >= b->nProblems || b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT)
        return CPECAN_EINVAL;
    if (byPosterior) *byPosterior = b->problems[problem].scores[0];
    if (byPosteriorIgnoringGaps) *byPosteriorIgnoringGaps = b->problems[problem].scores[1];
    if (meaScore) *meaScore = b->problems[problem].scores[2];
    return CPECAN_OK;
}

int cpk_overflow_scan(CpkRegion *regions, int64_t nRegions, CpkSegment *segs, int64_t nSegs, int nLists, int32_t *counts,
                      const int32_t *segCounts, int64_t *outTriples) {
    int overflow = 0;
    int64_t outAt = 0;
    for (int64_t di = 0; di < nRegions; di++) {
        CpkRegion *g = &regions[di];
        if (g->split) {
            /* the segments were written apart: a region's count is the sum, and each segment has its own capacity */
            int64_t at = 0;
            for (int l = 0; l < nLists; l++) counts[(size_t)l * nRegions + di] = 0;
            for (int32_t si = 0; si < g->nSeg; si++) {
                CpkSegment *sg = &segs[g->segOff + si];
                int32_t need = 0;
                for (int l = 0; l < nLists; l++) {
                    const int32_t c = segCounts[(size_t)l * nSegs + g->segOff + si];
                    need = c > need ? c : need;
                    counts[(size_t)l * nRegions + di] += c < sg->outCap ? c : sg->outCap;
                }
                if (need > sg->outCap) {
                    overflow = 1;
                    sg->outCap = need;
                }
                sg->outOff = (int32_t)at;
                at += sg->outCap;
            }
            if (at > g->outCap) g->outCap = (int32_t)at;
        } else {
            int32_t need = 0;
            for (int l = 0; l < nLists; l++) {
                const int32_t c = counts[(size_t)l * nRegions + di];
                need = c > need ? c : need;
            }
            if (need > g->outCap) {
                overflow = 1;
                g->outCap = need;
            }
        }
        g->outOff = outAt;
        outAt += g->outCap;
    }
    *outTriples = outAt;
    return overflow;
}

int cpecan_batch_download(cpecan_batch *b) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->ran) return CPECAN_ESTATE;
    free_results(b);
    b->stats.pairs = 0;
    if (b->nRegions == 0) {
        if (b->bandEdge) b->edges = calloc((size_t)(b->nProblems ? b->nProblems : 1), sizeof(cpecan_band_edge));
        if (b->bandEdge && !b->edges) return CPECAN_ENOMEM;
        if (b->quintNames) { /* no region, no pair: empty records, offsets and sums of 0 */
            b->quints = cpk_host_alloc(sizeof(int32_t) * 5);
            b->quintOffsets = calloc((size_t)(b->nProblems + 1), sizeof(int64_t));
            b->quintSums = calloc((size_t)(b->nProblems ? b->nProblems : 1), sizeof(int64_t));
            b->quintStageMs = 0.0;
            if (!b->quints || !b->quintOffsets || !b->quintSums) return CPECAN_ENOMEM;
        }
        if (b->nextRuns) { /* no region, no pair, no run */
            b->nextRunVals = malloc(sizeof(int64_t));
            b->nextRunOffsets = calloc((size_t)(b->nProblems + 1), sizeof(int64_t));
            if (!b->nextRunVals || !b->nextRunOffsets) return CPECAN_ENOMEM;
        }
        b->downloaded = 1;
        return CPECAN_OK;
    }
    int rc = CPECAN_OK;
    int32_t *counts = NULL, *segStarts = NULL, *segCounts = NULL;
    const double tD0 = now_ms();
    double tD1 = tD0;
    for (int attempt = 0; attempt < 3; attempt++) {
        cpk_host_free(counts);
        cpk_host_free(segStarts);
        cpk_host_free(segCounts);
        counts = cpk_host_alloc(sizeof(int32_t) * (size_t)b->nLists * b->nRegions);
        segStarts = cpk_host_alloc(sizeof(int32_t) * (size_t)b->nLists * (b->nSegs ? b->nSegs : 1));
        segCounts = cpk_host_alloc(sizeof(int32_t) * (size_t)b->nLists * (b->nSegs ? b->nSegs : 1));
        if (!counts || !segStarts || !segCounts) {
            rc = CPECAN_ENOMEM;
            break;
        }
        if ((b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT) && !b->forward) {
            b->forward = malloc(sizeof(double) * (size_t)(b->modelSlots > 0 ? b->modelSlots : 1) * (size_t)(b->nRegions > 106 ? b->nRegions : 106));
            if (!b->forward) {
                rc = CPECAN_ENOMEM;
                break;
            }
        }
        rc = cpk_device_download(b->dev, counts, segStarts, segCounts, b->forward, &b->stats.kernelMs, &b->stats.d2hMs);
        if (rc != CPECAN_OK) break;
        b->stats.h2dMs = cpk_device_h2d_ms(b->dev);
        tD1 = now_ms();
        if (b->emit == CPECAN_EMIT_FORWARD || b->emit == CPECAN_EMIT_EXPECT) break; /* these emitters produce no lists */
        /* did any region overflow its output slice?  If so enlarge exactly and run once more. */
        int64_t outAt = 0;
        const int overflow = cpk_overflow_scan(b->devRegions, b->nRegions, b->segs, b->nSegs, b->nLists, counts, segCounts, &outAt);
        if (!overflow) break;
        b->outTriples = outAt;
        rc = cpk_device_update_regions(b->dev, b->devRegions, b->segs, b->outTriples);
        if (rc != CPECAN_OK) break;
        rc = cpk_device_rerun(b->dev); /* same stream as the run that overflowed */
        if (rc != CPECAN_OK) break;
        b->stats.launches++;
        if (attempt == 2) {
            cpk_set_error("output overflow persisted after re-running");
            rc = CPECAN_ESTATE;
        }
    }
    if (rc == CPECAN_OK && b->emit != CPECAN_EMIT_FORWARD && b->emit != CPECAN_EMIT_EXPECT) {
        /* the lists are put in order on the device; only the emitted triples cross PCIe */
        CpkChunk *chunks = NULL;
        int64_t nChunks = 0, total = 0;
        const double tD2 = now_ms();
        int32_t *chunkRegion = NULL, *chunkProblem = NULL;
        int64_t nChunks0 = 0;
        rc = plan_results(b, counts, segStarts, segCounts, &chunks, &nChunks, &total, &chunkRegion, &chunkProblem, &nChunks0);
        const double tD3 = now_ms();
        if (rc == CPECAN_OK) rc = cpk_device_gather(b->dev, chunks, nChunks, total);
        cpk_host_free(chunks);
        if (rc == CPECAN_OK && b->bandEdge) { /* on the sweep's own scores: in front of the consumers (REWEIGHT rewrites them) */
            b->edges = malloc(sizeof(cpecan_band_edge) * (size_t)(b->nProblems ? b->nProblems : 1));
            rc = b->edges ? cpk_device_band_edge(b->dev, nChunks0, chunkRegion, chunkProblem, b->nProblems, b->edges) : CPECAN_ENOMEM;
        }
        free(chunkRegion);
        free(chunkProblem);
        const double tD4 = now_ms();
        if (rc == CPECAN_OK) rc = run_post(b); /* consumers of the lists, on the device, before they leave it */
        const double tD5 = now_ms();
        /* with the quintuple stage the records have left the device in run_post: the triples stay where they are */
        if (rc == CPECAN_OK && !b->quintNames && !b->nextRuns) rc = cpk_device_fetch(b->dev, b->results, total, &b->stats.d2hMs);
        b->stats.pairs = total;
        if (trace_host())
            fprintf(stderr, "cpecan download: wait + counts %.1f ms, overflow scan %.1f, list plan %.1f (%lld chunks), gather %.1f, consumers %.1f, fetch %.1f (%lld triples)\n",
                    tD1 - tD0, tD2 - tD1, tD3 - tD2, (long long)nChunks, tD4 - tD3, tD5 - tD4, now_ms() - tD5, (long long)total);
    }
    if (rc == CPECAN_OK) {
        b->downloaded = 1;
        b->downloadedModels = b->activeModels;
    }
    cpk_host_free(counts);
    cpk_host_free(segStarts);
    cpk_host_free(segCounts);
    return rc;
}

static void *download_helper(void *arg) {
    cpecan_batch *b = arg;
    tl_helperOf = b;
    b->dlResult = cpecan_batch_download(b);
    if (b->dlResult != CPECAN_OK) {
        strncpy(b->dlError, cpk_last_error(), sizeof b->dlError - 1);
        b->dlError[sizeof b->dlError - 1] = 0;
    }
    return NULL;
}

int cpecan_batch_download_begin(cpecan_batch *b) {
    if (!b || !b->ran || b->dlActive) return CPECAN_ESTATE;
    b->dlResult = CPECAN_OK;
    b->dlError[0] = 0;
    b->dlActive = 1;
    if (pthread_create(&b->dlThread, NULL, download_helper, b) != 0) {
        b->dlActive = 0;
        cpk_set_error("cannot start the download helper thread");
        return CPECAN_ENOMEM;
    }
    return CPECAN_OK;
}

int cpecan_batch_download_end(cpecan_batch *b) {
    if (!b || !b->dlActive) return CPECAN_ESTATE;
    pthread_join(b->dlThread, NULL);
    b->dlActive = 0;
    if (b->dlResult != CPECAN_OK) cpk_set_error("%s", b->dlError);
    return b->dlResult;
}

int cpecan_batch_result(const cpecan_batch *b, int64_t problem, int which, const int32_t **triples, int64_t *n) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded) return CPECAN_ESTATE;
    if (problem < 0 || problem >= b->nProblems || which < 0) return CPECAN_EINVAL;
    if (which >= b->nLists && !(which == 3 && (b->postFlags & (CPECAN_POST_MEA | CPECAN_POST_ORDERED)))) return CPECAN_EINVAL;
    if (which < 3 && b->quints) {
        cpk_set_error("the batch downloads quintuples (cpecan_batch_set_quintuples): its triples stayed on the device");
        return CPECAN_ESTATE;
    }
    if (b->nextRunOffsets) {
        cpk_set_error("the batch downloads anchor runs (cpecan_batch_set_next_runs): its triples stayed on the device");
        return CPECAN_ESTATE;
    }
    *triples = b->problems[problem].triples[which];
    *n = b->problems[problem].nTriples[which];
    return CPECAN_OK;
}

int cpecan_batch_forward_prob_slot(const cpecan_batch *b, int slot, int64_t problem, double *logProb) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded || b->emit != CPECAN_EMIT_FORWARD) return CPECAN_ESTATE;
    if (problem < 0 || problem >= b->nProblems || !logProb) return CPECAN_EINVAL;
    if (slot < 0 || slot >= b->downloadedModels) {
        cpk_set_error("slot %d of a run with %d models", slot, b->downloadedModels);
        return CPECAN_EINVAL;
    }
    *logProb = b->forward[(size_t)slot * b->nRegions + b->regions[b->problems[problem].firstRegion].devIndex];
    return CPECAN_OK;
}
int cpecan_batch_forward_prob(const cpecan_batch *b, int64_t problem, double *logProb) {
    return cpecan_batch_forward_prob_slot(b, 0, problem, logProb);
}

int cpecan_batch_expectations_slot(const cpecan_batch *b, int slot, cpecan_hmm *acc) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded || b->emit != CPECAN_EMIT_EXPECT) return CPECAN_ESTATE;
    const int S = is_five(b->model.type) ? 5 : 3;
    if (!acc || acc->stateNumber != S) return CPECAN_EINVAL;
    if (slot < 0 || slot >= b->downloadedModels) {
        cpk_set_error("slot %d of a run with %d models", slot, b->downloadedModels);
        return CPECAN_EINVAL;
    }
    if (b->nRegions == 0) return CPECAN_OK;
    /* b->forward holds the sums per slot: [0,25) transitions [from*S+to], [25,105) emissions, [105] likelihood */
    const double *sum = b->forward + (size_t)slot * 106;
    for (int i = 0; i < S * S; i++) acc->transitions[i] += sum[i];
    for (int i = 0; i < S * 16; i++) acc->emissions[i] += sum[25 + i];
    acc->likelihood += sum[105];
    return CPECAN_OK;
}
int cpecan_batch_expectations(const cpecan_batch *b, cpecan_hmm *acc) { return cpecan_batch_expectations_slot(b, 0, acc); }

int cpecan_batch_stats(const cpecan_batch *b, cpecan_stats *s) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !s) return CPECAN_EINVAL;
    *s = b->stats;
    return CPECAN_OK;
}

int cpecan_batch_debug_fetch(const cpecan_batch *b, int64_t problem, double *fbMatch, int64_t cells, double *totalUsed,
                             int64_t diagonals) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->downloaded || !b->debug) return CPECAN_ESTATE;
    if (problem < 0 || problem >= b->nProblems || b->problems[problem].nRegions != 1) return CPECAN_EINVAL;
    const HostRegion *r = &b->regions[b->problems[problem].firstRegion];
    const CpkRegion *g = &b->devRegions[r->devIndex];
    if (cells != r->cells || diagonals != r->lX + r->lY + 1) return CPECAN_EINVAL;
    double *fbAll = malloc(sizeof(double) * (size_t)b->dbgCells), *totAll = malloc(sizeof(double) * (size_t)b->dbgDiags);
    if (!fbAll || !totAll) {
        free(fbAll);
        free(totAll);
        return CPECAN_ENOMEM;
    }
    int rc = cpk_device_debug_fetch(b->dev, fbAll, b->dbgCells, totAll, b->dbgDiags);
    if (rc == CPECAN_OK) {
        memcpy(fbMatch, fbAll + g->dbgCellOff, sizeof(double) * (size_t)cells);
        memcpy(totalUsed, totAll + g->dbgDiagOff, sizeof(double) * (size_t)diagonals);
    }
    free(fbAll);
    free(totAll);
    return rc;
}

/* The band table of one region as the device built it for the plan that runs (tests/test_gpu_table.py): the region's
 * facts come from the host's copies of the plan, the entries and position words from the device.  Needs no debug mode. */
int cpecan_batch_table_fetch(const cpecan_batch *b, int64_t problem, int64_t regionInProblem, cpecan_table_info *info,
                             int32_t *diags, int32_t *dpos, int64_t nDiags, int32_t *segs, int64_t nSegs) {
    if (dl_busy(b)) return CPECAN_ESTATE;
    if (!b || !b->frozen) return CPECAN_ESTATE;
    if (!info || problem < 0 || problem >= b->nProblems || regionInProblem < 0 ||
        regionInProblem >= b->problems[problem].nRegions)
        return CPECAN_EINVAL;
    if (!b->dev || !b->devRegions) return CPECAN_ESTATE;
    const HostRegion *r = &b->regions[b->problems[problem].firstRegion + regionInProblem];
    const CpkRegion *g = &b->devRegions[r->devIndex];
    const int dynamic = b->emit == CPECAN_EMIT_FORWARD ? 0 : b->params.dynamicAnchorExpansion; /* host_plan_init */
    int hasPos = 0;
    int64_t ringDoubles = 0;
    int rc = cpk_device_table_fetch(b->dev, g, dynamic, NULL, NULL, &hasPos, &ringDoubles);
    if (rc != CPECAN_OK) return rc;
    memset(info, 0, sizeof *info);
    info->x1 = r->x1;
    info->y1 = r->y1;
    info->cells = g->cells;
    info->ringDoubles = ringDoubles;
    info->lX = g->lX;
    info->lY = g->lY;
    info->maxWidth = g->maxWidth;
    info->ringCap = g->ringCap;
    info->split = g->split;
    info->absOk = g->absOk;
    info->nSeg = g->nSeg;
    info->hasPos = hasPos;
    info->nStates = is_five(b->model.type) ? 5 : 3;
    info->nRegions = (int32_t)b->problems[problem].nRegions;
    if (!diags) return CPECAN_OK;
    if (nDiags != (int64_t)g->lX + g->lY + 1 || (segs && nSegs != g->nSeg)) return CPECAN_EINVAL;
    for (int64_t s = 0; segs && s < g->nSeg; s++) {
        const CpkSegment *sg = &b->segs[g->segOff + s];
        segs[3 * s] = sg->tbPrev;
        segs[3 * s + 1] = sg->dTop;
        segs[3 * s + 2] = sg->tbFrom;
    }
    return cpk_device_table_fetch(b->dev, g, dynamic, (CpkDiag *)diags, dpos, &hasPos, &ringDoubles);
}

/* ------------------------------------------------------------------------------------------------
 * single-problem convenience
 * ---------------------------------------------------------------------------------------------- */
/* ---- the list consumers on host-held lists: one problem through cpk_post_lists ---- */
typedef struct {
    int32_t *buf;    /* concatenated lists */
    int64_t total;
    CpkPostProblem pp;
    CpkPostJob job;
    uint8_t *chars;
    double scores[CPK_POST_SCORES];
    int32_t counts[2];
} PostSingle;

static void post_single_free(PostSingle *ps) {
    free(ps->buf);
    free(ps->chars);
    free(ps->job.mea);
    free(ps->job.shift);
}

static int post_single_run(PostSingle *ps, int flags, double gapGamma, double matchGamma, const int32_t *lists[3],
                           const int64_t n[3], int64_t lX, int64_t lY, const char *sX, const char *sY) {
    memset(ps, 0, sizeof *ps);
    ps->job.matchGamma = matchGamma;
    if (lX < 0 || lY < 0 || lX + lY >= (int64_t)1 << 30) return CPECAN_EINVAL;
    int64_t off[3], at = 0;
    for (int l = 0; l < 3; l++) {
        if (n[l] < 0 || n[l] >= (int64_t)1 << 30 || (n[l] > 0 && !lists[l])) return CPECAN_EINVAL;
        off[l] = at;
        at += n[l];
    }
    ps->total = at;
    ps->buf = malloc(sizeof(int32_t) * 3 * (size_t)(at ? at : 1));
    if (!ps->buf) return CPECAN_ENOMEM;
    for (int l = 0; l < 3; l++) {
        for (int64_t i = 0; (flags || sX) && i < n[l]; i++) { /* coordinates index the mass arrays and the sequences: check them */
            const int32_t x = lists[l][3 * i + 1], y = lists[l][3 * i + 2];
            const int okX = x >= 0 && x < lX, okY = y >= 0 && y < lY;
            if ((l == 0 && !(okX && okY)) || (l == 1 && !okX) || (l == 2 && !okY)) return CPECAN_EINVAL;
        }
        if (n[l]) memcpy(ps->buf + 3 * off[l], lists[l], sizeof(int32_t) * 3 * (size_t)n[l]);
    }
    ps->job.flags = flags;
    ps->job.gapGamma = gapGamma;
    ps->job.nProblems = 1;
    post_layout(&ps->job, &ps->pp, 0, off, n, lX, lY, 0, lX);
    ps->job.problems = &ps->pp;
    ps->job.scores = ps->scores;
    ps->job.counts = ps->counts;
    if (flags & (CPECAN_POST_MEA | CPECAN_POST_ORDERED)) {
        ps->job.mea = malloc(sizeof(int32_t) * 3 * (size_t)(ps->job.meaCap ? ps->job.meaCap : 1));
        if (!ps->job.mea) return CPECAN_ENOMEM;
    }
    if ((flags & CPECAN_POST_LEFT_SHIFT) && (!sX || !sY)) return CPECAN_EINVAL;
    if (sX && sY) {
        ps->chars = malloc((size_t)(lX + lY + 1));
        if (!ps->chars) return CPECAN_ENOMEM;
        for (int64_t i = 0; i < lX; i++) ps->chars[i] = (uint8_t)toupper((unsigned char)sX[i]);
        for (int64_t i = 0; i < lY; i++) ps->chars[lX + i] = (uint8_t)toupper((unsigned char)sY[i]);
        ps->job.chars = ps->chars;
        ps->job.nChars = lX + lY;
    }
    if (flags & CPECAN_POST_LEFT_SHIFT) {
        ps->job.shift = malloc(sizeof(int32_t) * 3 * (size_t)(ps->job.shiftCap ? ps->job.shiftCap : 1));
        if (!ps->job.shift) return CPECAN_ENOMEM;
    }
    return cpk_post_lists(cpk_current_device(), ps->buf, ps->total, &ps->job); /* the caller's current device */
}

static int take_list(const int32_t *src, int64_t n, int32_t **out, int64_t *nOut) {
    int32_t *t = malloc(sizeof(int32_t) * 3 * (size_t)(n ? n : 1));
    if (!t) return CPECAN_ENOMEM;
    if (n) memcpy(t, src, sizeof(int32_t) * 3 * (size_t)n);
    *out = t;
    *nOut = n;
    return CPECAN_OK;
}

/* The reweighting kernel keeps PROB_1 minus the listed mass of a base in an int32 (cpecan_post_reweight), the reference in
 * an int64 (impl/pairwiseAligner.c:1519-1534).  The two agree while that difference fits: the listed mass of every row
 * and every column must lie in [PROB_1 - INT32_MAX, PROB_1 - INT32_MIN] = [-2137483647, 2157483648], about 215 pairs of
 * probability one on one base.  A posterior list stays below 1 x PROB_1 (+ rounding); a list beyond the bound is refused
 * here, before a device is looked for ("The list consumers"). */
static int reweight_mass_fits(const int32_t *triples, int64_t n, int64_t lX, int64_t lY) {
    if (n < 0 || lX < 0 || lY < 0 || lX + lY >= (int64_t)1 << 30 || (n > 0 && !triples)) return CPECAN_EINVAL;
    int64_t *mass = calloc((size_t)(lX + lY ? lX + lY : 1), sizeof(int64_t));
    if (!mass) return CPECAN_ENOMEM;
    int rc = CPECAN_OK;
    for (int64_t i = 0; i < n && rc == CPECAN_OK; i++) {
        const int64_t x = triples[3 * i + 1], y = triples[3 * i + 2];
        if (x < 0 || x >= lX || y < 0 || y >= lY) {
            rc = CPECAN_EINVAL;
        } else {
            mass[x] += triples[3 * i];
            mass[lX + y] += triples[3 * i];
        }
    }
    for (int64_t i = 0; i < lX + lY && rc == CPECAN_OK; i++)
        if (mass[i] < (int64_t)CPECAN_PROB_1 - INT32_MAX || mass[i] > (int64_t)CPECAN_PROB_1 - INT32_MIN) {
            cpk_set_error("reweightAlignedPairs2: base %lld of %s lists a mass of %lld, outside [%lld, %lld]",
                          (long long)(i < lX ? i : i - lX), i < lX ? "X" : "Y", (long long)mass[i],
                          (long long)CPECAN_PROB_1 - INT32_MAX, (long long)CPECAN_PROB_1 - INT32_MIN);
            rc = CPECAN_EINVAL;
        }
    free(mass);
    return rc;
}

int cpecan_reweight_aligned_pairs(int32_t *triples, int64_t n, int64_t lX, int64_t lY, double gapGamma) {
    const int32_t *lists[3] = {triples, NULL, NULL};
    const int64_t ns[3] = {n, 0, 0};
    PostSingle ps;
    int rc = gapGamma > 0.0 ? reweight_mass_fits(triples, n, lX, lY) : CPECAN_OK; /* (:1551: no mass is formed otherwise) */
    if (rc != CPECAN_OK) return rc;
    rc = post_single_run(&ps, CPECAN_POST_REWEIGHT, gapGamma, 0.0, lists, ns, lX, lY, NULL, NULL);
    if (rc == CPECAN_OK && n) memcpy(triples, ps.buf, sizeof(int32_t) * 3 * (size_t)n);
    post_single_free(&ps);
    return rc;
}

int cpecan_posterior_scores(const int32_t *triples, int64_t n, int64_t lX, int64_t lY, double *byPosterior,
                            double *byPosteriorIgnoringGaps) {
    const int32_t *lists[3] = {triples, NULL, NULL};
    const int64_t ns[3] = {n, 0, 0};
    PostSingle ps;
    int rc = post_single_run(&ps, 0, 0.0, 0.0, lists, ns, lX, lY, NULL, NULL);
    if (rc == CPECAN_OK) {
        if (byPosterior) *byPosterior = ps.scores[0];
        if (byPosteriorIgnoringGaps) *byPosteriorIgnoringGaps = ps.scores[1];
    }
    post_single_free(&ps);
    return rc;
}

int cpecan_identity_scores(const int32_t *triples, int64_t n, const char *sX, const char *sY, double *byIdentity,
                           double *byIdentityIgnoringGaps) {
    if (!sX || !sY) return CPECAN_EINVAL;
    const int32_t *lists[3] = {triples, NULL, NULL};
    const int64_t ns[3] = {n, 0, 0};
    PostSingle ps;
    int rc = post_single_run(&ps, 0, 0.0, 0.0, lists, ns, (int64_t)strlen(sX), (int64_t)strlen(sY), sX, sY);
    if (rc == CPECAN_OK) {
        if (byIdentity) *byIdentity = ps.scores[3];
        if (byIdentityIgnoringGaps) *byIdentityIgnoringGaps = ps.scores[4];
    }
    post_single_free(&ps);
    return rc;
}

static int cmp_cell(const void *a, const void *b) {
    const int64_t u = *(const int64_t *)a, v = *(const int64_t *)b;
    return u < v ? -1 : (u > v ? 1 : 0);
}

/* A list that names one cell (x, y) twice is refused.  The reference keeps the weights of an X column in a set sorted by
 * Y position (impl/multipleAligner.c:121-131), so which copy's weight the chain sees is the set's insertion rule, and
 * filterMultipleAlignedPairs (:569-601) then keeps EVERY listed pair of a chosen cell, the copies under matchGamma
 * included; the oracle keeps the copy with the lower index and the kernels the one with the higher.  No emitter lists a
 * cell twice.  Checked here, before a device is looked for ("The list consumers"). */
static int cells_are_distinct(const int32_t *pairs, int64_t n) {
    if (n < 2) return CPECAN_OK;
    int64_t *cells = malloc(sizeof(int64_t) * (size_t)n);
    if (!cells) return CPECAN_ENOMEM;
    for (int64_t i = 0; i < n; i++) cells[i] = (int64_t)pairs[3 * i + 1] * ((int64_t)1 << 32) + (uint32_t)pairs[3 * i + 2];
    qsort(cells, (size_t)n, sizeof(int64_t), cmp_cell);
    int rc = CPECAN_OK;
    for (int64_t i = 1; i < n && rc == CPECAN_OK; i++)
        if (cells[i] == cells[i - 1]) {
            cpk_set_error("filterPairwiseAlignmentToMakePairsOrdered: cell (%lld, %lld) is listed more than once",
                          (long long)(cells[i] >> 32), (long long)(int32_t)(uint32_t)cells[i]);
            rc = CPECAN_EINVAL;
        }
    free(cells);
    return rc;
}

int cpecan_filter_pairs_ordered(const int32_t *pairs, int64_t n, int64_t lX, int64_t lY, float matchGamma, int32_t **out,
                                int64_t *nOut) {
    if (!out || !nOut || !(matchGamma >= 0.0f)) return CPECAN_EINVAL;
    if (n < 0 || n >= (int64_t)1 << 30 || (n > 0 && !pairs)) return CPECAN_EINVAL;
    {
        const int distinct = cells_are_distinct(pairs, n);
        if (distinct != CPECAN_OK) return distinct;
    }
    const int32_t *lists[3] = {pairs, NULL, NULL};
    const int64_t ns[3] = {n, 0, 0};
    PostSingle ps;
    int rc = post_single_run(&ps, CPECAN_POST_ORDERED, 0.0, (double)matchGamma, lists, ns, lX, lY, NULL, NULL);
    if (rc == CPECAN_OK) rc = take_list(ps.job.mea, ps.counts[0], out, nOut);
    post_single_free(&ps);
    return rc;
}

int cpecan_mea_alignment(const int32_t *pairs, int64_t n, const int32_t *gapX, int64_t nGapX, const int32_t *gapY,
                         int64_t nGapY, int64_t lX, int64_t lY, float gapGamma, int32_t **out, int64_t *nOut,
                         double *alignmentScore) {
    if (!out || !nOut) return CPECAN_EINVAL;
    const int32_t *lists[3] = {pairs, gapX, gapY};
    const int64_t ns[3] = {n, nGapX, nGapY};
    PostSingle ps;
    int rc = post_single_run(&ps, CPECAN_POST_MEA, (double)gapGamma, 0.0, lists, ns, lX, lY, NULL, NULL);
    if (rc == CPECAN_OK) rc = take_list(ps.job.mea, ps.counts[0], out, nOut);
    if (rc == CPECAN_OK && alignmentScore) *alignmentScore = ps.scores[2];
    post_single_free(&ps);
    return rc;
}

int cpecan_left_shift_alignment(const int32_t *pairs, int64_t n, const char *sX, const char *sY, int32_t **out,
                                int64_t *nOut) {
    if (!out || !nOut || !sX || !sY) return CPECAN_EINVAL;
    /* LEFT_SHIFT without MEA: the consumer stage shifts list 0 itself (it must be a chain, as in the reference) */
    const int32_t *lists[3] = {pairs, NULL, NULL};
    const int64_t ns[3] = {n, 0, 0};
    PostSingle ps;
    int rc = post_single_run(&ps, CPECAN_POST_LEFT_SHIFT, 0.0, 0.0, lists, ns, (int64_t)strlen(sX), (int64_t)strlen(sY), sX, sY);
    if (rc == CPECAN_OK) rc = take_list(ps.job.shift, ps.counts[1], out, nOut);
    post_single_free(&ps);
    return rc;
}

int cpecan_get_shifted_mea_alignment(const cpecan_model *m, const char *sX, const char *sY, const int64_t *anchors,
                                     int64_t nAnchors, const cpecan_params *p, float gapGamma, int raggedLeft,
                                     int raggedRight, int32_t **out, int64_t *nOut, double *alignmentScore) {
    if (!m || !sX || !sY || !p || !out || !nOut) return CPECAN_EINVAL;
    cpecan_batch *b = NULL;
    int rc = cpecan_batch_create(&b, m, p, CPECAN_EMIT_INDEL, cpk_current_device());
    if (rc != CPECAN_OK) return rc;
    rc = cpecan_batch_set_post(b, CPECAN_POST_MEA | CPECAN_POST_LEFT_SHIFT, (double)gapGamma);
    if (rc == CPECAN_OK) {
        const int64_t idx = cpecan_batch_add(b, sX, (int64_t)strlen(sX), sY, (int64_t)strlen(sY), anchors, nAnchors,
                                             raggedLeft, raggedRight);
        rc = idx < 0 ? (int)idx : CPECAN_OK;
    }
    if (rc == CPECAN_OK) rc = cpecan_batch_upload(b);
    if (rc == CPECAN_OK) rc = cpecan_batch_run(b, NULL);
    if (rc == CPECAN_OK) rc = cpecan_batch_download(b);
    if (rc == CPECAN_OK) rc = take_list(b->problems[0].triples[3], b->problems[0].nTriples[3], out, nOut);
    if (rc == CPECAN_OK && alignmentScore) *alignmentScore = b->problems[0].scores[2];
    cpecan_batch_destroy(b);
    return rc;
}

void cpecan_free(void *p) { free(p); }

/* one problem through a batch of one: create, add, upload, run, download */
static int run_single(cpecan_batch **out, const cpecan_model *m, const char *sX, const char *sY, const int64_t *anchors,
                      int64_t nAnchors, const cpecan_params *p, int raggedLeft, int raggedRight, int emit) {
    if (!m || !sX || !sY || !p) return CPECAN_EINVAL;
    cpecan_batch *b = NULL;
    int rc = cpecan_batch_create(&b, m, p, emit, cpk_current_device()); /* single-problem calls: the caller's current device */
    if (rc != CPECAN_OK) return rc;
    int64_t idx = cpecan_batch_add(b, sX, (int64_t)strlen(sX), sY, (int64_t)strlen(sY), anchors, nAnchors, raggedLeft,
                                   raggedRight);
    rc = idx < 0 ? (int)idx : CPECAN_OK;
    if (rc == CPECAN_OK) rc = cpecan_batch_upload(b);
    if (rc == CPECAN_OK) rc = cpecan_batch_run(b, NULL);
    if (rc == CPECAN_OK) rc = cpecan_batch_download(b);
    if (rc != CPECAN_OK) {
        cpecan_batch_destroy(b);
        return rc;
    }
    *out = b;
    return CPECAN_OK;
}

static int copy_list(const cpecan_batch *b, int which, int32_t **triples, int64_t *n) {
    const int32_t *src;
    int64_t cnt;
    int rc = cpecan_batch_result(b, 0, which, &src, &cnt);
    if (rc != CPECAN_OK) return rc;
    *triples = malloc(sizeof(int32_t) * 3 * (size_t)(cnt ? cnt : 1));
    if (!*triples) return CPECAN_ENOMEM;
    memcpy(*triples, src, sizeof(int32_t) * 3 * (size_t)cnt);
    *n = cnt;
    return CPECAN_OK;
}

int cpecan_get_aligned_pairs_using_anchors(const cpecan_model *m, const char *sX, const char *sY,
                                           const int64_t *anchors, int64_t nAnchors, const cpecan_params *p,
                                           int raggedLeft, int raggedRight, int32_t **triples, int64_t *n) {
    if (!triples || !n) return CPECAN_EINVAL;
    cpecan_batch *b = NULL;
    int rc = run_single(&b, m, sX, sY, anchors, nAnchors, p, raggedLeft, raggedRight, CPECAN_EMIT_MATCH);
    if (rc != CPECAN_OK) return rc;
    rc = copy_list(b, 0, triples, n);
    cpecan_batch_destroy(b);
    return rc;
}

int cpecan_get_aligned_pairs_with_indels_using_anchors(const cpecan_model *m, const char *sX, const char *sY,
                                                       const int64_t *anchors, int64_t nAnchors, const cpecan_params *p,
                                                       int raggedLeft, int raggedRight, int32_t **match, int64_t *nMatch,
                                                       int32_t **gapX, int64_t *nGapX, int32_t **gapY, int64_t *nGapY) {
    if (!match || !nMatch || !gapX || !nGapX || !gapY || !nGapY) return CPECAN_EINVAL;
    cpecan_batch *b = NULL;
    int rc = run_single(&b, m, sX, sY, anchors, nAnchors, p, raggedLeft, raggedRight, CPECAN_EMIT_INDEL);
    if (rc != CPECAN_OK) return rc;
    *match = *gapX = *gapY = NULL;
    rc = copy_list(b, 0, match, nMatch);
    if (rc == CPECAN_OK) rc = copy_list(b, 1, gapX, nGapX);
    if (rc == CPECAN_OK) rc = copy_list(b, 2, gapY, nGapY);
    if (rc != CPECAN_OK) {
        free(*match);
        free(*gapX);
        free(*gapY);
    }
    cpecan_batch_destroy(b);
    return rc;
}

int cpecan_compute_forward_probability(const cpecan_model *m, const char *sX, const char *sY, const int64_t *anchors,
                                       int64_t nAnchors, const cpecan_params *p, int raggedLeft, int raggedRight,
                                       double *logProb) {
    if (!logProb) return CPECAN_EINVAL;
    cpecan_batch *b = NULL;
    int rc = run_single(&b, m, sX, sY, anchors, nAnchors, p, raggedLeft, raggedRight, CPECAN_EMIT_FORWARD);
    if (rc != CPECAN_OK) return rc;
    rc = cpecan_batch_forward_prob(b, 0, logProb);
    cpecan_batch_destroy(b);
    return rc;
}
