/*
 * cpecan_viterbi.c -- Viterbi decoding (include/cpecan_viterbi.h): the host side.
 *
 * Host code only: the problems, their regions and bands (integers), the cut of a run into launches under the budget, the
 * borrowed views of the results, and the two pure host functions (replay, pairs).  The values of a run are the GPU's
 * (cpk_viterbi.inl); cpecan_viterbi_replay repeats the additions of one path on the host.  cpecan_viterbi_run_counts is the
 * resident form: the same plan, its inputs uploaded once and kept, the paths counted on the device;
 * cpecan_viterbi_counts_of_ops is that count over one path on the host.
 */
#define _POSIX_C_SOURCE 200809L
#include "cpecan_viterbi.h"

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_band.inl"
#include "cpecan_internal.h"

typedef struct {
    int64_t x1, y1, x2, y2;
    int64_t nCells, bytes;
    int32_t raggedLeft, raggedRight, maxWidth;
    CpkVitDiag *diags; /* [x2 - x1 + y2 - y1 + 1] */
} VitRegion;

typedef struct {
    int64_t lX, lY, firstRegion, nRegions, nCells, bytes;
    uint8_t *symX, *symY; /* the symbols of the whole sequences */
    /* after a run */
    double logP;
    int64_t opStart, nOps; /* its pairs in the object's ops */
} VitProblem;

struct cpecan_viterbi {
    cpecan_model model;
    cpecan_params params;
    int device, ran, form, nStates;
    int64_t budget;
    VitProblem *problems;
    int64_t n, cap;
    VitRegion *regions;
    int64_t nRegions, capRegions;
    cpecan_viterbi_region *out; /* [nRegions] of the last run */
    int32_t *ops;
    int64_t nOps, capOps;
    int64_t nLaunches, nLds, nGlobal;
    double sweepMs, tracebackMs;
    /* the resident form: the launches of the plan it was uploaded under, regions resFirst[k] .. resFirst[k + 1] - 1 each */
    CpkVitResident *resident;
    int64_t nResLaunches, *resFirst, resLds, resMaxRegions;
    /* after cpecan_viterbi_run_counts */
    int keepProblemCounts, countsRan;
    cpecan_viterbi_counts *problemCounts; /* [n], only when kept */
    double countMs, reduceMs;
};

static int is_five(int type) { return type == CPECAN_FIVE_STATE || type == CPECAN_FIVE_STATE_ASYM; }

static int params_valid(const cpecan_params *p) { /* pairwiseAligner.c:761-765 */
    return p->traceBackDiagonals >= 1 && p->diagonalExpansion >= 0 && p->diagonalExpansion % 2 == 0 &&
           p->minDiagsBetweenTraceBack >= 2 && p->traceBackDiagonals + 1 < p->minDiagsBetweenTraceBack;
}

/* Lengths and anchors as cpecan_dense_add takes them. */
static int problem_args_valid(const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors, int64_t nAnchors) {
    if (lX < 0 || lY < 0 || nAnchors < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || (nAnchors > 0 && !anchors)) return 0;
    if (lX + lY >= (int64_t)1 << 30) return 0;
    for (int64_t i = 0, px = -1, py = -1; i < nAnchors; px = anchors[3 * i], py = anchors[3 * i + 1], i++)
        if (anchors[3 * i] <= px || anchors[3 * i + 1] <= py || anchors[3 * i] >= lX || anchors[3 * i + 1] >= lY ||
            anchors[3 * i + 2] < INT32_MIN || anchors[3 * i + 2] > INT32_MAX)
            return 0;
    return 1;
}

/* What a region takes on the device: one pointer byte per band cell, its band records, its padded symbols, three rolling rows
 * of its widest diagonal (kept for either form: the figure does not depend on the form), room for lX + lY ops, its records. */
static int64_t region_bytes(const VitRegion *r, int S) {
    const int64_t N = r->x2 - r->x1 + r->y2 - r->y1;
    return r->nCells + (int64_t)sizeof(CpkVitDiag) * (N + 1) + (N + 4) + (int64_t)sizeof(double) * 3 * S * r->maxWidth +
           (int64_t)sizeof(int32_t) * 2 * N + (int64_t)(sizeof(CpkVitRegion) + sizeof(CpkVitOut) + sizeof(int32_t));
}

/* The band of a region, diagonal by diagonal.  CPECAN_EINVAL for anchors that give no valid band. */
static int plan_region(VitRegion *r, const cpk_anchor_t *a32, int64_t nAnchors, const cpecan_params *p) {
    const int64_t lX = r->x2 - r->x1, lY = r->y2 - r->y1, N = lX + lY;
    r->diags = malloc(sizeof *r->diags * (size_t)(N + 1));
    if (!r->diags) return CPECAN_ENOMEM;
    CpkBandIter it;
    if (cpk_band_init(&it, a32, 3, nAnchors, lX, lY, p->diagonalExpansion, p->dynamicAnchorExpansion != 0)) return CPECAN_EINVAL;
    int64_t cells = 0, widest = 1;
    for (int64_t d = 0; d <= N; d++) {
        int64_t lo, hi;
        if (cpk_band_next(&it, d, &lo, &hi)) return CPECAN_EINVAL;
        const int64_t width = (hi - lo) / 2 + 1;
        r->diags[d] = (CpkVitDiag){(int32_t)lo, (int32_t)width, cells};
        cells += width;
        if (width > widest) widest = width;
    }
    r->nCells = cells;
    r->maxWidth = (int32_t)widest;
    return CPECAN_OK;
}

int cpecan_viterbi_create(cpecan_viterbi **out, const cpecan_model *model, const cpecan_params *params, int device) {
    if (!out || !model || device < 0 || model->type < CPECAN_FIVE_STATE || model->type > CPECAN_THREE_STATE_ASYM) return CPECAN_EINVAL;
    cpecan_params p;
    if (params) p = *params;
    else cpecan_params_default(&p);
    if (!params_valid(&p)) {
        cpk_set_error("invalid banding parameters");
        return CPECAN_EINVAL;
    }
    cpecan_viterbi *v = calloc(1, sizeof *v);
    if (!v) return CPECAN_ENOMEM;
    v->model = *model;
    v->params = p;
    v->device = device;
    v->nStates = is_five(model->type) ? 5 : 3;
    v->budget = CPECAN_VITERBI_MAX_BYTES;
    v->form = CPECAN_VITERBI_FORM_AUTO;
    *out = v;
    return CPECAN_OK;
}

static void drop_results(cpecan_viterbi *v) {
    free(v->out);
    free(v->ops);
    v->out = NULL;
    v->ops = NULL;
    v->nOps = v->capOps = 0;
    v->ran = 0;
    v->nLaunches = v->nLds = v->nGlobal = 0;
    v->sweepMs = v->tracebackMs = 0.0;
    free(v->problemCounts);
    v->problemCounts = NULL;
    v->countsRan = 0;
    v->countMs = v->reduceMs = 0.0;
}

/* The resident form lives in the device layer; a program that links this file against a stand-in for that layer need not have
 * it: weak references, as cpecan_host.c takes the launch plan.  Such a program has no device, and nothing below calls them
 * before one is found. */
extern __typeof__(cpk_viterbi_resident_create) cpk_viterbi_resident_create __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_upload) cpk_viterbi_resident_upload __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_reserve) cpk_viterbi_resident_reserve __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_begin) cpk_viterbi_resident_begin __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_run) cpk_viterbi_resident_run __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_bins) cpk_viterbi_resident_bins __attribute__((weak));
extern __typeof__(cpk_viterbi_resident_destroy) cpk_viterbi_resident_destroy __attribute__((weak));

/* The resident inputs belong to one set of problems cut into launches under one budget and one form. */
static void drop_resident(cpecan_viterbi *v) {
    if (v->resident) cpk_viterbi_resident_destroy(v->resident);
    free(v->resFirst);
    v->resident = NULL;
    v->resFirst = NULL;
    v->nResLaunches = v->resLds = v->resMaxRegions = 0;
}

void cpecan_viterbi_destroy(cpecan_viterbi *v) {
    if (!v) return;
    drop_results(v);
    drop_resident(v);
    for (int64_t i = 0; i < v->n; i++) {
        free(v->problems[i].symX);
        free(v->problems[i].symY);
    }
    for (int64_t i = 0; i < v->nRegions; i++) free(v->regions[i].diags);
    free(v->problems);
    free(v->regions);
    free(v);
}

int64_t cpecan_viterbi_add(cpecan_viterbi *v, const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors,
                           int64_t nAnchors, int raggedLeft, int raggedRight) {
    if (!v) return CPECAN_EINVAL;
    if (!problem_args_valid(sX, lX, sY, lY, anchors, nAnchors)) {
        cpk_set_error("cpecan_viterbi_add: bad lengths or anchors");
        return CPECAN_EINVAL;
    }
    raggedLeft = raggedLeft != 0;
    raggedRight = raggedRight != 0;
    int64_t *rects = malloc(sizeof(int64_t) * 4 * (size_t)(nAnchors + 2));
    cpk_anchor_t *own = malloc(sizeof(cpk_anchor_t) * 3 * (size_t)(nAnchors ? nAnchors : 1));
    VitProblem q;
    memset(&q, 0, sizeof q);
    q.symX = malloc((size_t)lX + 1);
    q.symY = malloc((size_t)lY + 1);
    VitRegion *made = NULL;
    int64_t nRects = 0;
    int rc = (rects && own && q.symX && q.symY) ? CPECAN_OK : CPECAN_ENOMEM;
    if (rc == CPECAN_OK) {
        nRects = cpecan_split_points(anchors, nAnchors, lX, lY, v->params.splitMatrixBiggerThanThis, raggedLeft, raggedRight, rects);
        if (nRects <= 0) rc = CPECAN_EINVAL;
    }
    if (rc == CPECAN_OK && !(made = calloc((size_t)nRects, sizeof *made))) rc = CPECAN_ENOMEM;
    int64_t next = 0;
    for (int64_t k = 0; rc == CPECAN_OK && k < nRects; k++) {
        VitRegion *r = &made[k];
        r->x1 = rects[4 * k];
        r->y1 = rects[4 * k + 1];
        r->x2 = rects[4 * k + 2];
        r->y2 = rects[4 * k + 3];
        r->raggedLeft = raggedLeft || k > 0;
        r->raggedRight = raggedRight || k < nRects - 1;
        int64_t nOwn = 0; /* anchors go to regions in order (pairwiseAligner.c:1296-1308) */
        for (; next < nAnchors && anchors[3 * next] + anchors[3 * next + 1] < r->x2 + r->y2; next++, nOwn++) {
            if (anchors[3 * next] < r->x1 || anchors[3 * next] >= r->x2 || anchors[3 * next + 1] < r->y1 || anchors[3 * next + 1] >= r->y2)
                rc = CPECAN_EINVAL; /* :1304-1305 */
            own[3 * nOwn] = (cpk_anchor_t)(anchors[3 * next] - r->x1);
            own[3 * nOwn + 1] = (cpk_anchor_t)(anchors[3 * next + 1] - r->y1);
            own[3 * nOwn + 2] = (cpk_anchor_t)anchors[3 * next + 2];
        }
        if (rc == CPECAN_OK) rc = plan_region(r, own, nOwn, &v->params);
        r->bytes = rc == CPECAN_OK ? region_bytes(r, v->nStates) : 0;
        q.nCells += r->nCells;
        q.bytes += r->bytes;
    }
    if (rc == CPECAN_OK && next != nAnchors) rc = CPECAN_EINVAL; /* :1324 */
    if (rc == CPECAN_OK && v->n == v->cap) {
        const int64_t cap = v->cap ? 2 * v->cap : 8;
        VitProblem *g = realloc(v->problems, sizeof *g * (size_t)cap);
        if (g) {
            v->problems = g;
            v->cap = cap;
        } else rc = CPECAN_ENOMEM;
    }
    if (rc == CPECAN_OK && v->nRegions + nRects > v->capRegions) {
        int64_t cap = v->capRegions ? v->capRegions : 8;
        while (cap < v->nRegions + nRects) cap *= 2;
        VitRegion *g = realloc(v->regions, sizeof *g * (size_t)cap);
        if (g) {
            v->regions = g;
            v->capRegions = cap;
        } else rc = CPECAN_ENOMEM;
    }
    free(rects);
    free(own);
    if (rc != CPECAN_OK) {
        for (int64_t k = 0; made && k < nRects; k++) free(made[k].diags);
        free(made);
        free(q.symX);
        free(q.symY);
        if (rc == CPECAN_EINVAL) cpk_set_error("cpecan_viterbi_add: the anchors give no valid regions or band");
        return rc;
    }
    for (int64_t i = 0; i < lX; i++) q.symX[i] = cpk_symbol_of((unsigned char)sX[i]);
    for (int64_t i = 0; i < lY; i++) q.symY[i] = cpk_symbol_of((unsigned char)sY[i]);
    q.lX = lX;
    q.lY = lY;
    q.firstRegion = v->nRegions;
    q.nRegions = nRects;
    memcpy(v->regions + v->nRegions, made, sizeof *made * (size_t)nRects);
    free(made);
    drop_results(v);
    drop_resident(v);
    v->nRegions += nRects;
    v->problems[v->n] = q;
    return v->n++;
}

int cpecan_viterbi_set_budget(cpecan_viterbi *v, int64_t bytes) {
    if (!v || bytes <= 0) {
        cpk_set_error("cpecan_viterbi_set_budget: a budget of %lld bytes", (long long)bytes);
        return CPECAN_EINVAL;
    }
    if (bytes != v->budget) drop_resident(v); /* another cut into launches */
    v->budget = bytes;
    return CPECAN_OK;
}

int cpecan_viterbi_set_form(cpecan_viterbi *v, int form) {
    if (!v || form < CPECAN_VITERBI_FORM_AUTO || form > CPECAN_VITERBI_FORM_GLOBAL) {
        cpk_set_error("cpecan_viterbi_set_form: form %d, 0 (automatic), 1 (LDS rows) and 2 (global rows) exist", form);
        return CPECAN_EINVAL;
    }
    if (form != v->form) drop_resident(v); /* another order within the launches */
    v->form = form;
    return CPECAN_OK;
}

/* The inputs of one launch, packed for the device. */
typedef struct {
    CpkVitRegion *regions;
    CpkVitDiag *diags;
    uint8_t *symbols;
    int32_t *order;
} VitPack;

static void pack_free(VitPack *k) {
    free(k->regions);
    free(k->diags);
    free(k->symbols);
    free(k->order);
    memset(k, 0, sizeof *k);
}

/* Regions first .. last - 1 as one launch: the job's sizes, and its region records, band records, padded symbols and order. */
static int pack_launch(const cpecan_viterbi *v, int64_t first, int64_t last, const int64_t *problemOf, CpkVitJob *job, VitPack *k) {
    const int S = v->nStates;
    const size_t one = 1;
    memset(job, 0, sizeof *job);
    memset(k, 0, sizeof *k);
    job->nRegions = last - first;
    for (int64_t i = first; i < last; i++) {
        const VitRegion *r = &v->regions[i];
        const int64_t N = r->x2 - r->x1 + r->y2 - r->y1;
        job->nDiags += N + 1;
        job->nSymbolBytes += N + 4;
        job->nPtrBytes += r->nCells;
        job->nRollDoubles += (int64_t)3 * S * r->maxWidth;
        job->nOpPairs += N;
    }
    CpkVitRegion *hr = k->regions = calloc((size_t)job->nRegions + one, sizeof *hr);
    CpkVitDiag *hd = k->diags = calloc((size_t)job->nDiags + one, sizeof *hd);
    uint8_t *sym = k->symbols = calloc((size_t)job->nSymbolBytes + one, 1);
    int32_t *order = k->order = calloc((size_t)job->nRegions + one, sizeof *order);
    if (!hr || !hd || !sym || !order) {
        pack_free(k);
        return CPECAN_ENOMEM;
    }
    int64_t diagAt = 0, symAt = 0, ptrAt = 0, rollAt = 0, opAt = 0;
    for (int64_t i = first; i < last; i++) {
        const VitRegion *r = &v->regions[i];
        const VitProblem *q = &v->problems[problemOf[i]];
        const int64_t lX = r->x2 - r->x1, lY = r->y2 - r->y1, N = lX + lY;
        CpkVitRegion *o = &hr[i - first];
        o->symX = symAt;
        o->symY = symAt + lX + 2;
        o->diagOff = diagAt;
        o->ptrBase = ptrAt;
        o->rollBase = rollAt;
        o->opBase = opAt;
        o->lX = (int32_t)lX;
        o->lY = (int32_t)lY;
        o->raggedLeft = r->raggedLeft;
        o->raggedRight = r->raggedRight;
        o->maxWidth = r->maxWidth;
        uint8_t *s = sym + symAt;
        *s++ = CPK_SYM_N;
        memcpy(s, q->symX + r->x1, (size_t)lX);
        s += lX;
        *s++ = CPK_SYM_N;
        *s++ = CPK_SYM_N;
        memcpy(s, q->symY + r->y1, (size_t)lY);
        s += lY;
        *s++ = CPK_SYM_N;
        memcpy(hd + diagAt, r->diags, sizeof *hd * (size_t)(N + 1));
        diagAt += N + 1;
        symAt += N + 4;
        ptrAt += r->nCells;
        rollAt += (int64_t)3 * S * r->maxWidth;
        opAt += N;
    }
    /* the LDS-form regions first, then the global-form ones, each in region order */
    int64_t at = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int64_t i = first; i < last; i++) {
            const int32_t w = v->regions[i].maxWidth;
            const int lds = v->form == CPECAN_VITERBI_FORM_LDS || (v->form == CPECAN_VITERBI_FORM_AUTO && w <= CPK_VIT_LDS_MAX_WIDTH);
            if (lds != (pass == 0)) continue;
            order[at++] = (int32_t)(i - first);
            if (lds && w > job->ldsMaxWidth) job->ldsMaxWidth = w;
        }
        if (pass == 0) job->nLds = at;
    }
    job->regions = hr;
    job->diags = hd;
    job->symbols = sym;
    job->order = order;
    return CPECAN_OK;
}

/* Regions first .. last - 1 in one launch; their results are appended to v->out and v->ops. */
static int run_launch(cpecan_viterbi *v, const CpkModel *km, int64_t first, int64_t last, const int64_t *problemOf) {
    const size_t one = 1;
    CpkVitJob job;
    VitPack pack;
    int rc = pack_launch(v, first, last, problemOf, &job, &pack);
    const CpkVitRegion *hr = pack.regions;
    CpkVitOut *out = rc == CPECAN_OK ? calloc((size_t)job.nRegions + one, sizeof *out) : NULL;
    int32_t *ops = rc == CPECAN_OK ? calloc(2 * (size_t)job.nOpPairs + one, sizeof *ops) : NULL;
    if (rc == CPECAN_OK && !(out && ops)) rc = CPECAN_ENOMEM;
    if (rc == CPECAN_OK) {
        job.out = out;
        job.ops = ops;
        double sweepMs = 0.0, tracebackMs = 0.0;
        rc = cpk_viterbi_launch(v->device, km, &job, &sweepMs, &tracebackMs);
        v->sweepMs += sweepMs;
        v->tracebackMs += tracebackMs;
    }
    for (int64_t i = first; rc == CPECAN_OK && i < last; i++) {
        const VitRegion *r = &v->regions[i];
        const CpkVitOut *g = &out[i - first];
        VitProblem *q = &v->problems[problemOf[i]];
        const int64_t N = r->x2 - r->x1 + r->y2 - r->y1;
        if (g->nOps < 0 || g->nOps > N) {
            cpk_set_error("cpecan_viterbi_run: region %lld came back with %d ops", (long long)i, g->nOps);
            rc = CPECAN_EHIP;
            break;
        }
        if (v->nOps + g->nOps > v->capOps) {
            int64_t cap = v->capOps ? v->capOps : 1024;
            while (cap < v->nOps + g->nOps) cap *= 2;
            int32_t *grown = realloc(v->ops, sizeof(int32_t) * 2 * (size_t)cap);
            if (!grown) {
                rc = CPECAN_ENOMEM;
                break;
            }
            v->ops = grown;
            v->capOps = cap;
        }
        if (i == q->firstRegion) {
            q->opStart = v->nOps;
            q->nOps = 0;
            q->logP = 0.0;
        }
        cpecan_viterbi_region *o = &v->out[i];
        o->x1 = r->x1;
        o->y1 = r->y1;
        o->x2 = r->x2;
        o->y2 = r->y2;
        o->logP = g->logP;
        o->startState = g->startState; /* -1 with endState -1: no path */
        o->endState = g->endState;
        o->opOff = q->nOps;
        o->nOps = g->nOps;
        q->logP = i == q->firstRegion ? g->logP : q->logP + g->logP; /* the plain sum, region order */
        const int32_t *src = ops + 2 * hr[i - first].opBase; /* last run first */
        for (int64_t k = 0; k < g->nOps; k++) {
            v->ops[2 * (v->nOps + k)] = src[2 * (g->nOps - 1 - k)];
            v->ops[2 * (v->nOps + k) + 1] = src[2 * (g->nOps - 1 - k) + 1];
        }
        v->nOps += g->nOps;
        q->nOps += g->nOps;
    }
    if (rc == CPECAN_OK) {
        v->nLaunches++;
        v->nLds += job.nLds;
        v->nGlobal += job.nRegions - job.nLds;
    }
    pack_free(&pack);
    free(out);
    free(ops);
    return rc;
}

/* Before a device is looked for: the answers do not depend on one. */
static int check_regions(const cpecan_viterbi *v, const char *who) {
    for (int64_t i = 0; i < v->nRegions; i++) {
        const VitRegion *r = &v->regions[i];
        if (v->form == CPECAN_VITERBI_FORM_LDS && r->maxWidth > CPK_VIT_LDS_MAX_WIDTH) {
            cpk_set_error("%s: the LDS form holds diagonals of %d cells, region %lld has one of %d", who, CPK_VIT_LDS_MAX_WIDTH, (long long)i,
                          r->maxWidth);
            return CPECAN_EINVAL;
        }
        if (r->bytes > v->budget) {
            cpk_set_error("%s: region %lld alone needs %lld bytes on the device, the budget allows %lld", who, (long long)i,
                          (long long)r->bytes, (long long)v->budget);
            return CPECAN_ENOMEM;
        }
    }
    return CPECAN_OK;
}

static int check_device(const cpecan_viterbi *v) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || v->device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, v->device);
        return CPECAN_ENODEVICE;
    }
    return CPECAN_OK;
}

/* The problem of every region, or NULL. */
static int64_t *problem_of(const cpecan_viterbi *v) {
    const size_t one = 1;
    int64_t *problemOf = malloc(sizeof(int64_t) * ((size_t)v->nRegions + one));
    if (problemOf)
        for (int64_t i = 0; i < v->n; i++)
            for (int64_t k = 0; k < v->problems[i].nRegions; k++) problemOf[v->problems[i].firstRegion + k] = i;
    return problemOf;
}

/* Consecutive launches of whole regions: where the launch that starts at region first ends. */
static int64_t launch_end(const cpecan_viterbi *v, int64_t first) {
    int64_t last = first, bytes = 0;
    while (last < v->nRegions && bytes + v->regions[last].bytes <= v->budget) bytes += v->regions[last++].bytes;
    return last;
}

int cpecan_viterbi_run(cpecan_viterbi *v) {
    if (!v) return CPECAN_EINVAL;
    drop_results(v);
    int rc = check_regions(v, "cpecan_viterbi_run");
    if (rc == CPECAN_OK) rc = check_device(v);
    if (rc != CPECAN_OK) return rc;
    CpkModel km;
    cpk_kernel_model(&v->model, v->params.threshold, &km);
    const size_t one = 1;
    int64_t *problemOf = problem_of(v);
    v->out = calloc((size_t)v->nRegions + one, sizeof *v->out);
    rc = (problemOf && v->out) ? CPECAN_OK : CPECAN_ENOMEM;
    for (int64_t first = 0; rc == CPECAN_OK && first < v->nRegions;) {
        const int64_t last = launch_end(v, first);
        rc = run_launch(v, &km, first, last, problemOf);
        first = last;
    }
    free(problemOf);
    if (rc == CPECAN_OK) v->ran = 1;
    else drop_results(v);
    return rc;
}

/* ---- Viterbi training's E-step: the counts of the decoded paths ---- */

int cpecan_viterbi_set_model(cpecan_viterbi *v, const cpecan_model *model) {
    if (!v || !model || model->type < CPECAN_FIVE_STATE || model->type > CPECAN_THREE_STATE_ASYM) return CPECAN_EINVAL;
    if ((is_five(model->type) ? 5 : 3) != v->nStates) {
        cpk_set_error("cpecan_viterbi_set_model: a model of %d states for an object of %d", is_five(model->type) ? 5 : 3, v->nStates);
        return CPECAN_EINVAL;
    }
    v->model = *model;
    drop_results(v); /* the resident inputs do not depend on the model */
    return CPECAN_OK;
}

int cpecan_viterbi_set_keep_problem_counts(cpecan_viterbi *v, int on) {
    if (!v) return CPECAN_EINVAL;
    v->keepProblemCounts = on != 0;
    drop_results(v);
    return CPECAN_OK;
}

/* What launch first .. last - 1 keeps on the device for good, and what it needs of each scratch array. */
static void launch_bytes(const cpecan_viterbi *v, int64_t first, int64_t last, int64_t *inputs, int64_t scratch[5]) {
    const int S = v->nStates;
    const int64_t n = last - first;
    int64_t diags = 0, cells = 0, roll = 0;
    for (int64_t i = first; i < last; i++) {
        const VitRegion *r = &v->regions[i];
        diags += r->x2 - r->x1 + r->y2 - r->y1 + 1;
        cells += r->nCells;
        roll += (int64_t)3 * S * r->maxWidth;
    }
    *inputs = (int64_t)(sizeof(CpkVitRegion) + sizeof(int32_t)) * n + (int64_t)sizeof(CpkVitDiag) * diags + (diags + 3 * n);
    scratch[0] = cells;
    scratch[1] = (int64_t)sizeof(double) * roll;
    scratch[2] = (int64_t)sizeof(CpkVitOut) * n;
    scratch[3] = (int64_t)sizeof(int32_t) * 2 * (diags - n);
    scratch[4] = (int64_t)sizeof(uint32_t) * (S * S + S * 16) * n;
}

int cpecan_viterbi_resident_bytes(const cpecan_viterbi *v, int64_t *inputBytes, int64_t *scratchBytes) {
    if (!v) return CPECAN_EINVAL;
    const int rc = check_regions(v, "cpecan_viterbi_resident_bytes");
    if (rc != CPECAN_OK) return rc;
    int64_t inputs = 0, most[5] = {0, 0, 0, 0, 0};
    for (int64_t first = 0; first < v->nRegions;) {
        const int64_t last = launch_end(v, first);
        int64_t in, sc[5];
        launch_bytes(v, first, last, &in, sc);
        inputs += in;
        for (int i = 0; i < 5; i++)
            if (sc[i] > most[i]) most[i] = sc[i];
        first = last;
    }
    if (inputBytes) *inputBytes = inputs;
    if (scratchBytes) *scratchBytes = most[0] + most[1] + most[2] + most[3] + most[4];
    return CPECAN_OK;
}

/* Plans the launches as cpecan_viterbi_run does and uploads the inputs of each, once. */
static int make_resident(cpecan_viterbi *v) {
    int64_t inputs = 0, scratch = 0, nLaunches = 0;
    int rc = cpecan_viterbi_resident_bytes(v, &inputs, &scratch);
    if (rc != CPECAN_OK) return rc;
    for (int64_t first = 0; first < v->nRegions; first = launch_end(v, first)) nLaunches++;
    const size_t one = 1;
    int64_t *problemOf = problem_of(v);
    v->resFirst = malloc(sizeof(int64_t) * ((size_t)nLaunches + one));
    rc = (problemOf && v->resFirst) ? CPECAN_OK : CPECAN_ENOMEM;
    if (rc == CPECAN_OK) rc = cpk_viterbi_resident_create(&v->resident, v->device, v->nStates, nLaunches, inputs, scratch);
    int64_t first = 0;
    for (int64_t k = 0; rc == CPECAN_OK && k < nLaunches; k++) {
        const int64_t last = launch_end(v, first);
        CpkVitJob job;
        VitPack pack;
        rc = pack_launch(v, first, last, problemOf, &job, &pack);
        if (rc == CPECAN_OK) rc = cpk_viterbi_resident_upload(v->resident, k, &job);
        pack_free(&pack);
        if (rc != CPECAN_OK) break;
        v->resFirst[k] = first;
        v->resFirst[k + 1] = last;
        v->resLds += job.nLds;
        if (last - first > v->resMaxRegions) v->resMaxRegions = last - first;
        first = last;
    }
    if (rc == CPECAN_OK) rc = cpk_viterbi_resident_reserve(v->resident);
    free(problemOf);
    if (rc == CPECAN_OK) v->nResLaunches = nLaunches;
    else drop_resident(v);
    return rc;
}

static void counts_clear(cpecan_viterbi_counts *c, int nStates) {
    memset(c, 0, sizeof *c);
    c->nStates = nStates;
}

/* bins: S * S transitions, then S * 16 emissions. */
static void counts_add_bins(cpecan_viterbi_counts *c, int S, const int64_t *bins) {
    for (int b = 0; b < S * S; b++) {
        c->transitions[b] += bins[b];
        c->nSteps += bins[b];
    }
    for (int b = 0; b < S * 16; b++) c->emissions[b] += bins[S * S + b];
}

/* One region's slab, widened. */
static void counts_add_slab(cpecan_viterbi_counts *c, int S, const uint32_t *slab) {
    int64_t bins[CPK_VIT_MAX_BINS];
    for (int b = 0; b < S * S + S * 16; b++) bins[b] = (int64_t)slab[b];
    counts_add_bins(c, S, bins);
}

int cpecan_viterbi_run_counts(cpecan_viterbi *v, cpecan_viterbi_counts *total) {
    if (!v || !total) return CPECAN_EINVAL;
    drop_results(v);
    int rc = check_regions(v, "cpecan_viterbi_run_counts");
    if (rc == CPECAN_OK) rc = check_device(v);
    if (rc == CPECAN_OK && !cpk_viterbi_resident_create) rc = CPECAN_ESTATE; /* a device without the device layer */
    if (rc == CPECAN_OK && !v->resident) rc = make_resident(v);
    if (rc != CPECAN_OK) return rc;
    const int S = v->nStates, nBins = S * S + S * 16;
    const size_t one = 1;
    CpkModel km;
    cpk_kernel_model(&v->model, v->params.threshold, &km);
    CpkVitOut *out = malloc(sizeof *out * ((size_t)v->resMaxRegions + one));
    uint32_t *slabs = v->keepProblemCounts ? malloc(sizeof *slabs * (size_t)nBins * ((size_t)v->resMaxRegions + one)) : NULL;
    if (v->keepProblemCounts) v->problemCounts = calloc((size_t)v->n + one, sizeof *v->problemCounts);
    if (!out || (v->keepProblemCounts && !(slabs && v->problemCounts))) rc = CPECAN_ENOMEM;
    cpecan_viterbi_counts sum;
    counts_clear(&sum, S);
    for (int64_t i = 0; rc == CPECAN_OK && v->problemCounts && i < v->n; i++) counts_clear(&v->problemCounts[i], S);
    if (rc == CPECAN_OK) rc = cpk_viterbi_resident_begin(v->resident);
    int64_t problem = 0;
    for (int64_t k = 0; rc == CPECAN_OK && k < v->nResLaunches; k++) {
        const int64_t first = v->resFirst[k], last = v->resFirst[k + 1];
        double ms[4];
        rc = cpk_viterbi_resident_run(v->resident, k, &km, out, slabs, ms);
        if (rc != CPECAN_OK) break;
        v->sweepMs += ms[0];
        v->tracebackMs += ms[1];
        v->countMs += ms[2];
        v->reduceMs += ms[3];
        for (int64_t i = first; i < last; i++) { /* global region order: the sums do not depend on the cut into launches */
            const VitRegion *r = &v->regions[i];
            const CpkVitOut *g = &out[i - first];
            if (g->nOps < 0 || g->nOps > r->x2 - r->x1 + r->y2 - r->y1) {
                cpk_set_error("cpecan_viterbi_run_counts: region %lld came back with %d ops", (long long)i, g->nOps);
                rc = CPECAN_EHIP;
                break;
            }
            while (i >= v->problems[problem].firstRegion + v->problems[problem].nRegions) problem++;
            cpecan_viterbi_counts *pc = v->problemCounts ? &v->problemCounts[problem] : NULL;
            if (g->endState < 0) { /* no path: no counts, nothing to the likelihood */
                sum.nNoPath++;
                if (pc) pc->nNoPath++;
                continue;
            }
            sum.logP = sum.logP + g->logP;
            if (pc) {
                pc->logP = pc->logP + g->logP;
                counts_add_slab(pc, S, slabs + (size_t)nBins * (size_t)(i - first));
            }
        }
    }
    if (rc == CPECAN_OK) {
        int64_t bins[CPK_VIT_MAX_BINS];
        rc = cpk_viterbi_resident_bins(v->resident, bins);
        if (rc == CPECAN_OK) counts_add_bins(&sum, S, bins);
    }
    free(out);
    free(slabs);
    if (rc != CPECAN_OK) {
        drop_results(v);
        return rc;
    }
    v->countsRan = 1;
    v->nLaunches = v->nResLaunches;
    v->nLds = v->resLds;
    v->nGlobal = v->nRegions - v->resLds;
    *total = sum;
    return CPECAN_OK;
}

int cpecan_viterbi_problem_counts(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_counts *out) {
    if (!v || !out || problem < 0 || problem >= v->n) return CPECAN_EINVAL;
    if (!v->keepProblemCounts || !v->countsRan || !v->problemCounts) {
        cpk_set_error("cpecan_viterbi_problem_counts: %s", !v->keepProblemCounts ? "cpecan_viterbi_set_keep_problem_counts is off"
                                                                                 : "before cpecan_viterbi_run_counts");
        return CPECAN_ESTATE;
    }
    *out = v->problemCounts[problem];
    return CPECAN_OK;
}

int cpecan_viterbi_count_ms(const cpecan_viterbi *v, double *countMs, double *reduceMs) {
    if (!v) return CPECAN_EINVAL;
    if (countMs) *countMs = v->countMs;
    if (reduceMs) *reduceMs = v->reduceMs;
    return CPECAN_OK;
}

int cpecan_viterbi_counts_of_ops(int nStates, const char *sX, int64_t lX, const char *sY, int64_t lY, int startState, const int32_t *ops,
                                 int64_t nOps, cpecan_viterbi_counts *out) {
    if (!out || (nStates != 3 && nStates != 5) || lX < 0 || lY < 0 || nOps < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || (nOps > 0 && !ops) ||
        startState < 0 || startState >= nStates) {
        cpk_set_error("cpecan_viterbi_counts_of_ops: invalid arguments");
        return CPECAN_EINVAL;
    }
    const int S = nStates;
    cpecan_viterbi_counts c;
    counts_clear(&c, S);
    int64_t x = 0, y = 0;
    int s = startState;
    for (int64_t i = 0; i < nOps; i++) {
        const int to = ops[2 * i];
        if (ops[2 * i + 1] < 1 || to < 0 || to >= S) {
            cpk_set_error("cpecan_viterbi_counts_of_ops: op %lld is (%d, %d)", (long long)i, to, ops[2 * i + 1]);
            return CPECAN_EINVAL;
        }
        for (int32_t k = 0; k < ops[2 * i + 1]; k++) {
            x += to == 0 || to == 1 || to == 3;
            y += to == 0 || to == 2 || to == 4;
            if (x > lX || y > lY) {
                cpk_set_error("cpecan_viterbi_counts_of_ops: op %lld leaves the matrix", (long long)i);
                return CPECAN_EINVAL;
            }
            const int cX = x > 0 ? cpk_symbol_of((unsigned char)sX[x - 1]) : CPK_SYM_N;
            const int cY = y > 0 ? cpk_symbol_of((unsigned char)sY[y - 1]) : CPK_SYM_N;
            c.transitions[s * S + to]++;
            if (cX < 4 && cY < 4) c.emissions[to * 16 + cX * 4 + cY]++; /* updateExpectations, pairwiseAligner.c:418-432 */
            c.nSteps++;
            s = to;
        }
    }
    if (x != lX || y != lY) {
        cpk_set_error("cpecan_viterbi_counts_of_ops: the ops end at (%lld, %lld), not at (%lld, %lld)", (long long)x, (long long)y,
                      (long long)lX, (long long)lY);
        return CPECAN_EINVAL;
    }
    *out = c;
    return CPECAN_OK;
}

int cpecan_viterbi_counts_add_to_hmm(const cpecan_viterbi_counts *counts, cpecan_hmm *acc) {
    if (!counts || !acc) return CPECAN_EINVAL;
    if (counts->nStates != acc->stateNumber || (acc->stateNumber != 3 && acc->stateNumber != 5)) {
        cpk_set_error("cpecan_viterbi_counts_add_to_hmm: counts of %lld states for an hmm of %d", (long long)counts->nStates, acc->stateNumber);
        return CPECAN_EINVAL;
    }
    const int S = acc->stateNumber;
    for (int i = 0; i < S * S; i++) acc->transitions[i] += (double)counts->transitions[i];
    for (int i = 0; i < S * 16; i++) acc->emissions[i] += (double)counts->emissions[i];
    acc->likelihood += counts->logP;
    return CPECAN_OK;
}

int cpecan_viterbi_launch_forms(const cpecan_viterbi *v, int64_t *nLaunches, int64_t *nLds, int64_t *nGlobal) {
    if (!v) return CPECAN_EINVAL;
    if (nLaunches) *nLaunches = v->nLaunches;
    if (nLds) *nLds = v->nLds;
    if (nGlobal) *nGlobal = v->nGlobal;
    return CPECAN_OK;
}

int cpecan_viterbi_info(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_info_t *info) {
    if (!v || !info || problem < 0 || problem >= v->n) return CPECAN_EINVAL;
    const VitProblem *q = &v->problems[problem];
    info->nRegions = q->nRegions;
    info->nCells = q->nCells;
    info->nStates = v->nStates;
    info->deviceBytes = q->bytes;
    return CPECAN_OK;
}

int cpecan_viterbi_result(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_result_t *res) {
    if (!v || !res || problem < 0 || problem >= v->n) return CPECAN_EINVAL;
    if (!v->ran) {
        cpk_set_error("cpecan_viterbi_result before cpecan_viterbi_run");
        return CPECAN_ESTATE;
    }
    const VitProblem *q = &v->problems[problem];
    res->logP = q->logP;
    res->nRegions = q->nRegions;
    res->nOps = q->nOps;
    res->regions = v->out + q->firstRegion;
    res->ops = v->ops ? v->ops + 2 * q->opStart : NULL;
    return CPECAN_OK;
}

int cpecan_viterbi_kernel_ms(const cpecan_viterbi *v, double *sweepMs, double *tracebackMs) {
    if (!v) return CPECAN_EINVAL;
    if (sweepMs) *sweepMs = v->sweepMs;
    if (tracebackMs) *tracebackMs = v->tracebackMs;
    return CPECAN_OK;
}

/* The model's transition from -> to: 1 and *tP, or 0 where its ordered list has none. */
static int transition(const CpkModel *m, int from, int to, double *tP) {
    const int S = m->nStates;
    if (from < 0 || from >= S || to < 0 || to >= S) return 0;
    if (to == 0) {
        const double t[5] = {m->matchContinue, m->matchFromShortX, m->matchFromShortY, m->matchFromLongX, m->matchFromLongY};
        *tP = t[from];
        return 1;
    }
    if (from == 0) {
        const double t[5] = {0.0, m->shortOpenX, m->shortOpenY, m->longOpenX, m->longOpenY};
        *tP = t[to];
        return 1;
    }
    if (from == to) {
        const double t[5] = {0.0, m->shortExtendX, m->shortExtendY, m->longExtendX, m->longExtendY};
        *tP = t[to];
        return 1;
    }
    if (S == 3) { /* the switches, impl/stateMachine.c:689-714 */
        *tP = to == 1 ? m->shortSwitchToX : m->shortSwitchToY;
        return 1;
    }
    return 0;
}

int cpecan_viterbi_replay(const cpecan_model *model, const char *sX, int64_t lX, const char *sY, int64_t lY, int raggedLeft,
                          int raggedRight, int startState, int endState, const int32_t *ops, int64_t nOps, double *logP) {
    if (!model || !logP || lX < 0 || lY < 0 || nOps < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || (nOps > 0 && !ops) ||
        model->type < CPECAN_FIVE_STATE || model->type > CPECAN_THREE_STATE_ASYM) {
        cpk_set_error("cpecan_viterbi_replay: invalid arguments");
        return CPECAN_EINVAL;
    }
    CpkModel m;
    cpk_kernel_model(model, 0.0, &m);
    const int S = m.nStates;
    if (startState < 0 || startState >= S || endState < 0 || endState >= S) {
        cpk_set_error("cpecan_viterbi_replay: states %d .. %d of a model with %d", startState, endState, S);
        return CPECAN_EINVAL;
    }
    double val = raggedLeft ? m.raggedStart[startState] : m.start[startState];
    int64_t x = 0, y = 0;
    int s = startState;
    for (int64_t i = 0; i < nOps; i++) {
        const int to = ops[2 * i];
        double tP = 0.0;
        if (ops[2 * i + 1] < 1 || to < 0 || to >= S) {
            cpk_set_error("cpecan_viterbi_replay: op %lld is (%d, %d)", (long long)i, to, ops[2 * i + 1]);
            return CPECAN_EINVAL;
        }
        for (int32_t k = 0; k < ops[2 * i + 1]; k++) {
            if (!transition(&m, s, to, &tP)) {
                cpk_set_error("cpecan_viterbi_replay: op %lld uses the transition %d -> %d, which the model lacks", (long long)i, s, to);
                return CPECAN_EINVAL;
            }
            x += to == 0 || to == 1 || to == 3;
            y += to == 0 || to == 2 || to == 4;
            if (x > lX || y > lY) {
                cpk_set_error("cpecan_viterbi_replay: op %lld leaves the matrix", (long long)i);
                return CPECAN_EINVAL;
            }
            const int cX = x > 0 ? cpk_symbol_of((unsigned char)sX[x - 1]) : CPK_SYM_N;
            const int cY = y > 0 ? cpk_symbol_of((unsigned char)sY[y - 1]) : CPK_SYM_N;
            const double e = to == 0 ? m.matchEm[cX * 5 + cY] : (to == 1 || to == 3) ? m.gapXEm[cX] : m.gapYEm[cY];
            val = val + (e + tP);
            s = to;
        }
    }
    if (x != lX || y != lY || s != endState) {
        cpk_set_error("cpecan_viterbi_replay: the ops end at (%lld, %lld) in state %d, not at (%lld, %lld) in state %d", (long long)x,
                      (long long)y, s, (long long)lX, (long long)lY, endState);
        return CPECAN_EINVAL;
    }
    *logP = val + (raggedRight ? m.raggedEnd[endState] : m.end[endState]);
    return CPECAN_OK;
}

int64_t cpecan_viterbi_pairs(const cpecan_viterbi_result_t *res, int64_t *xy, int64_t cap) {
    if (!res || cap < 0 || (cap > 0 && !xy) || res->nRegions < 0 || (res->nRegions > 0 && !res->regions)) return CPECAN_EINVAL;
    int64_t n = 0;
    for (int64_t i = 0; i < res->nRegions; i++) {
        const cpecan_viterbi_region *r = &res->regions[i];
        int64_t x = r->x1, y = r->y1;
        for (int64_t k = 0; k < r->nOps; k++) {
            const int32_t s = res->ops[2 * (r->opOff + k)], len = res->ops[2 * (r->opOff + k) + 1];
            if (s == 0)
                for (int32_t j = 0; j < len; j++, n++)
                    if (n < cap) {
                        xy[2 * n] = x + j;
                        xy[2 * n + 1] = y + j;
                    }
            x += (s == 0 || s == 1 || s == 3) ? len : 0;
            y += (s == 0 || s == 2 || s == 4) ? len : 0;
        }
    }
    return n;
}
