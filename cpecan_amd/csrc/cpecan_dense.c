/*
 * cpecan_dense.c -- dense forward / backward rows (include/cpecan_dense.h): the host side.
 *
 * Host code only: the problems, their bands and traceback schedules (integers), the cap, and the borrowed views of the four
 * result arrays.  The values are the GPU's (cpk_dense.inl): nothing here adds two log-probabilities.
 */
#define _POSIX_C_SOURCE 200809L
#include "cpecan_dense.h"

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_band.inl"
#include "cpecan_internal.h"

typedef struct {
    int64_t lX, lY, nDiags, nCells, nSegs, sideCells;
    int32_t raggedLeft, raggedRight;
    uint8_t *symbols;         /* N + X + N, N + Y + N */
    cpecan_dense_diag *diags; /* [nDiags] */
    int64_t *cellOff;         /* [nDiags + 1] */
    cpecan_dense_seg *segs;
    int64_t *bnextOff;        /* [nSegs + 1] */
    /* after a run: where the problem's slices start in the object's arrays */
    int64_t cellBase, diagBase, bnextBase;
} DenseProblem;

struct cpecan_dense {
    cpecan_model model;
    cpecan_params params;
    int device, ran;
    DenseProblem *problems;
    int64_t n, cap;
    double *F, *B, *bnext, *totals; /* of all problems */
    double kernelMs;
};

static int params_valid(const cpecan_params *p) { /* pairwiseAligner.c:761-765 */
    return p->traceBackDiagonals >= 1 && p->diagonalExpansion >= 0 && p->diagonalExpansion % 2 == 0 &&
           p->minDiagsBetweenTraceBack >= 2 && p->traceBackDiagonals + 1 < p->minDiagsBetweenTraceBack;
}

/* Lengths and anchors as cpecan_batch_add takes them (cpecan_host.c, problem_valid). */
static int problem_args_valid(const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors, int64_t nAnchors) {
    if (lX < 0 || lY < 0 || nAnchors < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || (nAnchors > 0 && !anchors)) return 0;
    if (lX + lY >= (int64_t)1 << 30) return 0;
    for (int64_t i = 0, px = -1, py = -1; i < nAnchors; px = anchors[3 * i], py = anchors[3 * i + 1], i++)
        if (anchors[3 * i] <= px || anchors[3 * i + 1] <= py || anchors[3 * i] >= lX || anchors[3 * i + 1] >= lY ||
            anchors[3 * i + 2] < INT32_MIN || anchors[3 * i + 2] > INT32_MAX)
            return 0;
    return 1;
}

/* The band of a problem, diagonal by diagonal, and its tracebacks by the rule of pairwiseAligner.c:791-810.  diags, cellOff
 * and segs may be NULL (segs: at most segCap are written).  Returns CPECAN_OK, CPECAN_EINVAL for anchors that give no valid
 * band, CPECAN_ENOMEM. */
static int plan_problem(int64_t lX, int64_t lY, const int64_t *anchors, int64_t nAnchors, const cpecan_params *p,
                        cpecan_dense_diag *diags, int64_t *cellOff, cpecan_dense_seg *segs, int64_t segCap, int64_t *nSegs,
                        int64_t *nCells) {
    const int64_t N = lX + lY;
    cpk_anchor_t *a32 = malloc(sizeof *a32 * 3 * (size_t)(nAnchors ? nAnchors : 1));
    if (!a32) return CPECAN_ENOMEM;
    for (int64_t i = 0; i < 3 * nAnchors; i++) a32[i] = (cpk_anchor_t)anchors[i];
    CpkBandIter it;
    int rc = cpk_band_init(&it, a32, 3, nAnchors, lX, lY, p->diagonalExpansion, p->dynamicAnchorExpansion != 0) ? CPECAN_EINVAL : CPECAN_OK;
    int64_t cells = 0, tracedBackTo = 0, ns = 0;
    for (int64_t d = 0; rc == CPECAN_OK && d <= N; d++) {
        int64_t lo, hi;
        if (cpk_band_next(&it, d, &lo, &hi)) {
            rc = CPECAN_EINVAL;
            break;
        }
        const int64_t width = (hi - lo) / 2 + 1;
        if (diags) diags[d] = (cpecan_dense_diag){(int32_t)lo, (int32_t)width};
        if (cellOff) cellOff[d] = cells;
        cells += width;
        const int atEnd = d == N;
        if (d == 0 || !(atEnd || (d >= tracedBackTo + p->minDiagsBetweenTraceBack && width <= p->diagonalExpansion * 2 + 1))) continue;
        const int64_t tracedBackFrom = d - (atEnd ? 0 : p->traceBackDiagonals + 1);
        if (segs && ns < segCap) segs[ns] = (cpecan_dense_seg){(int32_t)tracedBackTo, (int32_t)d, (int32_t)tracedBackFrom};
        ns++;
        tracedBackTo = tracedBackFrom;
    }
    if (cellOff && rc == CPECAN_OK) cellOff[N + 1] = cells;
    free(a32);
    if (nSegs) *nSegs = ns;
    if (nCells) *nCells = cells;
    return rc;
}

int cpecan_dense_schedule(int64_t lX, int64_t lY, const int64_t *anchors, int64_t nAnchors, const cpecan_params *params,
                          cpecan_dense_seg *segsOut, int64_t segCap, int64_t *nSegs, cpecan_dense_call *callsOut,
                          int64_t callCap, int64_t *nCalls) {
    cpecan_params def;
    if (!params) {
        cpecan_params_default(&def);
        params = &def;
    }
    if (!params_valid(params) || segCap < 0 || callCap < 0 || (segCap > 0 && !segsOut) || (callCap > 0 && !callsOut) ||
        !problem_args_valid("", lX, "", lY, anchors, nAnchors)) {
        cpk_set_error("cpecan_dense_schedule: invalid arguments");
        return CPECAN_EINVAL;
    }
    if (nSegs) *nSegs = 0;
    if (nCalls) *nCalls = 0;
    const int64_t N = lX + lY;
    if (N == 0) return CPECAN_OK; /* :767-770 */
    int64_t ns = 0;
    int rc = plan_problem(lX, lY, anchors, nAnchors, params, NULL, NULL, NULL, 0, &ns, NULL);
    if (rc != CPECAN_OK) return rc;
    cpecan_dense_seg *segs = malloc(sizeof *segs * (size_t)ns);
    if (!segs) return CPECAN_ENOMEM;
    rc = plan_problem(lX, lY, anchors, nAnchors, params, NULL, NULL, segs, ns, NULL, NULL);
    int64_t nc = 0;
    for (int64_t k = 0; rc == CPECAN_OK && k < ns; k++) {
        const cpecan_dense_seg g = segs[k];
        if (k < segCap) segsOut[k] = g;
        for (int64_t d = g.tbFrom; d > g.tbPrev; d--, nc++) {
            if (nc >= callCap) continue;
            cpecan_dense_call *c = &callsOut[nc];
            c->xay = d;
            c->seg = k;
            c->fLo = g.tbPrev;
            c->fHi = d;
            c->f2Lo = g.dTop == N ? 0 : g.tbFrom;
            c->f2Hi = g.dTop == N ? -1 : g.dTop;
            c->bLo = d - 1 > g.tbPrev ? d - 1 : g.tbPrev + 1;
            c->bHi = d + 1 < g.dTop ? d + 1 : g.dTop;
        }
    }
    free(segs);
    if (nSegs) *nSegs = ns;
    if (nCalls) *nCalls = nc;
    return rc;
}

int cpecan_dense_create(cpecan_dense **out, const cpecan_model *model, const cpecan_params *params, int device) {
    if (!out || !model || device < 0 || model->type < CPECAN_FIVE_STATE || model->type > CPECAN_THREE_STATE_ASYM) return CPECAN_EINVAL;
    cpecan_params p;
    if (params) p = *params;
    else cpecan_params_default(&p);
    if (!params_valid(&p)) {
        cpk_set_error("invalid banding parameters");
        return CPECAN_EINVAL;
    }
    cpecan_dense *d = calloc(1, sizeof *d);
    if (!d) return CPECAN_ENOMEM;
    d->model = *model;
    d->params = p;
    d->device = device;
    *out = d;
    return CPECAN_OK;
}

static void drop_results(cpecan_dense *d) {
    free(d->F);
    free(d->B);
    free(d->bnext);
    free(d->totals);
    d->F = d->B = d->bnext = d->totals = NULL;
    d->ran = 0;
}

static void free_problem(DenseProblem *q) {
    free(q->symbols);
    free(q->diags);
    free(q->cellOff);
    free(q->segs);
    free(q->bnextOff);
}

void cpecan_dense_destroy(cpecan_dense *d) {
    if (!d) return;
    drop_results(d);
    for (int64_t i = 0; i < d->n; i++) free_problem(&d->problems[i]);
    free(d->problems);
    free(d);
}

int64_t cpecan_dense_add(cpecan_dense *d, const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors,
                         int64_t nAnchors, int raggedLeft, int raggedRight) {
    if (!d) return CPECAN_EINVAL;
    if (!problem_args_valid(sX, lX, sY, lY, anchors, nAnchors)) {
        cpk_set_error("cpecan_dense_add: bad lengths or anchors");
        return CPECAN_EINVAL;
    }
    if (d->n == d->cap) {
        const int64_t cap = d->cap ? 2 * d->cap : 8;
        DenseProblem *g = realloc(d->problems, sizeof *g * (size_t)cap);
        if (!g) return CPECAN_ENOMEM;
        d->problems = g;
        d->cap = cap;
    }
    DenseProblem q;
    memset(&q, 0, sizeof q);
    q.lX = lX;
    q.lY = lY;
    q.raggedLeft = raggedLeft != 0;
    q.raggedRight = raggedRight != 0;
    const int64_t N = lX + lY;
    int rc = CPECAN_OK;
    if (N > 0) { /* N == 0: a legal problem without rows (:767-770) */
        q.nDiags = N + 1;
        rc = plan_problem(lX, lY, anchors, nAnchors, &d->params, NULL, NULL, NULL, 0, &q.nSegs, NULL);
        if (rc == CPECAN_OK) {
            q.symbols = malloc((size_t)N + 4);
            q.diags = malloc(sizeof *q.diags * (size_t)q.nDiags);
            q.cellOff = malloc(sizeof *q.cellOff * (size_t)(q.nDiags + 1));
            q.segs = malloc(sizeof *q.segs * (size_t)q.nSegs);
            q.bnextOff = malloc(sizeof *q.bnextOff * (size_t)(q.nSegs + 1));
            if (!q.symbols || !q.diags || !q.cellOff || !q.segs || !q.bnextOff) rc = CPECAN_ENOMEM;
        }
        if (rc == CPECAN_OK) rc = plan_problem(lX, lY, anchors, nAnchors, &d->params, q.diags, q.cellOff, q.segs, q.nSegs, NULL, &q.nCells);
        if (rc == CPECAN_OK) {
            uint8_t *s = q.symbols;
            *s++ = CPK_SYM_N;
            for (int64_t i = 0; i < lX; i++) *s++ = cpk_symbol_of((unsigned char)sX[i]);
            *s++ = CPK_SYM_N;
            *s++ = CPK_SYM_N;
            for (int64_t i = 0; i < lY; i++) *s++ = cpk_symbol_of((unsigned char)sY[i]);
            *s++ = CPK_SYM_N;
            int64_t off = 0;
            for (int64_t k = 0; k < q.nSegs; k++) { /* Bnext: the row of tbFrom + 1; on the device, rows tbFrom + 1 .. dTop */
                const cpecan_dense_seg g = q.segs[k];
                q.bnextOff[k] = off;
                if (g.tbFrom < g.dTop) {
                    off += q.diags[g.tbFrom + 1].width;
                    q.sideCells += q.cellOff[g.dTop + 1] - q.cellOff[g.tbFrom + 1];
                }
            }
            q.bnextOff[q.nSegs] = off;
        }
    }
    if (rc != CPECAN_OK) {
        free_problem(&q);
        if (rc == CPECAN_EINVAL) cpk_set_error("cpecan_dense_add: the anchors give no valid band");
        return rc;
    }
    drop_results(d);
    d->problems[d->n] = q;
    return d->n++;
}

static int64_t max_bytes(void) {
    const char *e = getenv("CPECAN_DENSE_MAX_BYTES");
    if (e && *e) {
        char *end = NULL;
        const long long v = strtoll(e, &end, 10);
        if (end != e && v >= 0) return (int64_t)v;
    }
    return CPECAN_DENSE_MAX_BYTES;
}

int cpecan_dense_run(cpecan_dense *d) {
    if (!d) return CPECAN_EINVAL;
    drop_results(d);
    CpkModel km;
    cpk_kernel_model(&d->model, d->params.threshold, &km);
    const int S = km.nStates;
    CpkDenseJob job;
    memset(&job, 0, sizeof job);
    job.nProblems = d->n;
    int64_t bnextCells = 0;
    for (int64_t i = 0; i < d->n; i++) {
        DenseProblem *q = &d->problems[i];
        q->cellBase = job.totalCells;
        q->diagBase = job.nDiags;
        q->bnextBase = bnextCells;
        job.totalCells += q->nCells;
        job.nDiags += q->nDiags;
        job.nSegs += q->nSegs;
        job.sideCells += q->sideCells;
        job.nSymbolBytes += q->nDiags ? q->lX + q->lY + 4 : 0;
        bnextCells += q->nSegs ? q->bnextOff[q->nSegs] : 0;
    }
    const int64_t need = cpk_dense_device_bytes(&job, S), cap = max_bytes();
    if (need > cap) { /* before a device is looked for (cpk_dense_run does that): the answer does not depend on one */
        cpk_set_error("cpecan_dense_run: the dense rows need %lld bytes on the device, CPECAN_DENSE_MAX_BYTES allows %lld",
                      (long long)need, (long long)cap);
        return CPECAN_ENOMEM;
    }
    const size_t one = 1;
    CpkDenseProblem *hp = calloc((size_t)job.nProblems + one, sizeof *hp);
    CpkDenseDiag *hd = calloc((size_t)job.nDiags + one, sizeof *hd);
    CpkDenseSeg *hs = calloc((size_t)job.nSegs + one, sizeof *hs);
    uint8_t *sym = calloc((size_t)job.nSymbolBytes + one, 1);
    double *side = malloc(sizeof(double) * ((size_t)job.sideCells * S + one));
    d->F = malloc(sizeof(double) * ((size_t)job.totalCells * S + one));
    d->B = malloc(sizeof(double) * ((size_t)job.totalCells * S + one));
    d->bnext = malloc(sizeof(double) * ((size_t)bnextCells * S + one));
    d->totals = malloc(sizeof(double) * ((size_t)job.nDiags + one));
    int rc = (hp && hd && hs && sym && side && d->F && d->B && d->bnext && d->totals) ? CPECAN_OK : CPECAN_ENOMEM;
    if (rc == CPECAN_OK) {
        int64_t symAt = 0, segAt = 0, sideAt = 0;
        for (int64_t i = 0; i < d->n; i++) {
            const DenseProblem *q = &d->problems[i];
            CpkDenseProblem *o = &hp[i];
            o->lX = (int32_t)q->lX;
            o->lY = (int32_t)q->lY;
            o->raggedLeft = q->raggedLeft;
            o->raggedRight = q->raggedRight;
            o->diagOff = q->diagBase;
            o->cellBase = q->cellBase;
            if (!q->nDiags) continue;
            o->symX = symAt;
            o->symY = symAt + q->lX + 2;
            memcpy(sym + symAt, q->symbols, (size_t)(q->lX + q->lY + 4));
            symAt += q->lX + q->lY + 4;
            for (int64_t k = 0; k < q->nDiags; k++) hd[q->diagBase + k] = (CpkDenseDiag){q->diags[k].xmyL, q->diags[k].width, q->cellOff[k]};
            for (int64_t k = 0; k < q->nSegs; k++, segAt++) {
                const cpecan_dense_seg g = q->segs[k];
                hs[segAt] = (CpkDenseSeg){g.tbPrev, g.dTop, g.tbFrom, (int32_t)i, sideAt};
                if (g.tbFrom < g.dTop) sideAt += q->cellOff[g.dTop + 1] - q->cellOff[g.tbFrom + 1];
            }
        }
        job.problems = hp;
        job.diags = hd;
        job.segs = hs;
        job.symbols = sym;
        job.F = d->F;
        job.B = d->B;
        job.side = side;
        job.totals = d->totals;
        rc = cpk_dense_run(d->device, &km, &job, &d->kernelMs);
    }
    if (rc == CPECAN_OK) { /* Bnext: the first of every traceback's side rows */
        int64_t segAt = 0;
        for (int64_t i = 0; i < d->n; i++) {
            const DenseProblem *q = &d->problems[i];
            for (int64_t k = 0; k < q->nSegs; k++, segAt++)
                memcpy(d->bnext + (q->bnextBase + q->bnextOff[k]) * S, side + hs[segAt].sideBase * S,
                       sizeof(double) * (size_t)((q->bnextOff[k + 1] - q->bnextOff[k]) * S));
        }
        d->ran = 1;
    }
    free(hp);
    free(hd);
    free(hs);
    free(sym);
    free(side);
    if (rc != CPECAN_OK) drop_results(d);
    return rc;
}

int cpecan_dense_info(const cpecan_dense *d, int64_t problem, cpecan_dense_info_t *info) {
    if (!d || !info || problem < 0 || problem >= d->n) return CPECAN_EINVAL;
    const DenseProblem *q = &d->problems[problem];
    info->nDiagonals = q->nDiags;
    info->nCells = q->nCells;
    info->nSegments = q->nSegs;
    info->nStates = (d->model.type == CPECAN_FIVE_STATE || d->model.type == CPECAN_FIVE_STATE_ASYM) ? 5 : 3;
    return CPECAN_OK;
}

int cpecan_dense_rows(const cpecan_dense *d, int64_t problem, cpecan_dense_rows_t *rows) {
    if (!d || !rows || problem < 0 || problem >= d->n) return CPECAN_EINVAL;
    if (!d->ran) {
        cpk_set_error("cpecan_dense_rows before cpecan_dense_run");
        return CPECAN_ESTATE;
    }
    const DenseProblem *q = &d->problems[problem];
    const int S = (d->model.type == CPECAN_FIVE_STATE || d->model.type == CPECAN_FIVE_STATE_ASYM) ? 5 : 3;
    rows->diags = q->diags;
    rows->cellOff = q->cellOff;
    rows->F = d->F + q->cellBase * S;
    rows->B = d->B + q->cellBase * S;
    rows->Bnext = d->bnext + q->bnextBase * S;
    rows->bnextOff = q->bnextOff;
    rows->totalUsed = d->totals + q->diagBase;
    rows->segs = q->segs;
    return CPECAN_OK;
}

double cpecan_dense_kernel_ms(const cpecan_dense *d) { return d ? d->kernelMs : 0.0; }
