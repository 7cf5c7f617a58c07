/* A C caller that brings its OWN per-diagonal emitter to getPosteriorProbsWithBanding and to
 * getPosteriorProbsWithBandingSplittingAlignmentsByLargeGaps (include/cpecan_dropin.h).  The library serves such an emitter
 * from dense rows computed on the GPU (include/cpecan_dense.h); the three emitters the reference ships are recognised by
 * address and run on kernels of their own.  Here each of the three is restated as a foreign callback that uses only what it is
 * handed -- dpMatrix_getDiagonal, dpDiagonal_getCell, sM->cellCalculate, totalProbability -- and held against its token:
 *   (i)   match posteriors against diagonalCalculationPosteriorMatchProbs: same order; the same pairs but for pairs within
 *         1e-5 * threshold of the threshold (at most 1 % of the list); scores within max(1, 1e-5 * score);
 *   (ii)  match and gap-state posteriors against diagonalCalculationPosteriorProbs, the same rule on all three lists;
 *   (iii) expectations from F[d - 1], F[d - 2], B[d], likelihood += total per call, against diagonalCalculationExpectations:
 *         every entry to 1e-5 relative (the token path forms its events in fp32).  The sums are written to the output file;
 *         tests/test_foreign_emitter_c.py holds them against the oracle at 1e-9.
 * Every call also asserts the live-row contract of cpecan_dense_schedule: the sequence of xay values, which rows each matrix
 * holds (forward[d - 2] == NULL at the bottom of every traceback after the first; backward[d + 1] != NULL unless d == N), and
 * dpMatrix_getActiveDiagonalNumber.  (That both matrices end with zero active rows is the library's own check: it aborts.)
 * usage: test_foreign_emitter <cases file> <output file>       -- the cases file is written by the pytest wrapper */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_dense.h"
#include "cpecan_dropin.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 40) fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

enum { MATCH = 0, INDEL = 1, EXPECT = 2 };

typedef struct {
    char name[64];
    StateMachine *sM;
    PairwiseAlignmentParameters *p;
    int raggedLeft, raggedRight;
    int64_t lX, lY, nAnchors;
    char *sx, *sy;
    int64_t *anchors;
} Case;

/* one region of an entry-point call and the calls the library owes it */
typedef struct {
    int64_t x1, y1, lX, lY, nCalls, nSegs;
    cpecan_dense_call *calls;
} Region;

typedef struct {
    int kind;
    Region *regions;
    int64_t nRegions, region, at; /* the call expected next: `at` of `region` */
    int64_t corrections;          /* coordinateCorrectionFn calls so far */
    stList *lists[3];
    Hmm *hmm;
    int64_t bottoms;              /* calls at the bottom of a traceback behind the first: forward[d - 2] must be NULL there */
} Foreign;

/* ---- the live-row contract ---- */
static int in_range(int64_t r, int64_t lo, int64_t hi) { return r >= lo && r <= hi; }
static void check_contract(Foreign *f, int64_t xay, DpMatrix *forward, DpMatrix *backward, const SymbolString sX, const SymbolString sY) {
    while (f->region < f->nRegions && f->at == f->regions[f->region].nCalls) { /* regions without diagonals make no call */
        f->region++;
        f->at = 0;
    }
    CHECK(f->region < f->nRegions);
    if (f->region >= f->nRegions) return;
    const Region *rg = &f->regions[f->region];
    const cpecan_dense_call *c = &rg->calls[f->at++];
    const int64_t N = rg->lX + rg->lY;
    CHECK(xay == c->xay);
    CHECK(sX.length == rg->lX && sY.length == rg->lY);
    CHECK(f->corrections == f->region || f->kind == EXPECT); /* the correction of a region comes after its last call */
    int64_t nF = 0, nB = 0;
    for (int64_t r = 0; r <= N; r++) {
        const int wantF = in_range(r, c->fLo, c->fHi) || in_range(r, c->f2Lo, c->f2Hi), wantB = in_range(r, c->bLo, c->bHi);
        CHECK((dpMatrix_getDiagonal(forward, r) != NULL) == wantF);
        CHECK((dpMatrix_getDiagonal(backward, r) != NULL) == wantB);
        nF += wantF;
        nB += wantB;
    }
    CHECK(dpMatrix_getActiveDiagonalNumber(forward) == nF && dpMatrix_getActiveDiagonalNumber(backward) == nB);
    CHECK(dpMatrix_getDiagonal(forward, xay) != NULL && dpMatrix_getDiagonal(forward, xay - 1) != NULL); /* :824-825 */
    CHECK(dpMatrix_getDiagonal(backward, xay) != NULL);
    CHECK(xay == N || dpMatrix_getDiagonal(backward, xay + 1) != NULL);
    CHECK(dpMatrix_getDiagonal(backward, xay - 2) == NULL); /* the half-accumulated row is not served */
    if (xay == c->fLo + 1 && c->fLo >= 1) {                 /* the bottom of a traceback behind the first: F[d - 2] is freed */
        CHECK(dpMatrix_getDiagonal(forward, xay - 2) == NULL);
        f->bottoms++;
    }
}

/* the cells of a row, found as a foreign caller can find them: dpDiagonal_getCell is NULL outside the band */
#define FOR_CELLS(row, xay, lX, lY, xmy)                                                                              \
    for (int64_t xmy = ((xay) - 2 * (lY) > -(xay) ? (xay) - 2 * (lY) : -(xay)); xmy <= (xay) && xmy <= 2 * (lX) - (xay); xmy += 2) \
        if (dpDiagonal_getCell(row, xmy) != NULL)

static void keep(stList *out, double pp, double threshold, int64_t x, int64_t y) { /* the rule of addPosteriorProb */
    if (pp >= threshold) stList_append(out, stIntTuple_construct3((int64_t)floor((pp > 1.0 ? 1.0 : pp) * PAIR_ALIGNMENT_PROB_1), x - 1, y - 1));
}

typedef struct {
    double total;
    Hmm *hmm;
    Symbol cX, cY;
} Event;
static void count_event(double *from, double *to, int64_t f, int64_t t, double eP, double tP, void *extra) {
    Event *e = extra;
    const double pr = exp(from[f] + to[t] + (eP + tP) - e->total);
    hmm_addToTransitionExpectation(e->hmm, f, t, pr);
    if (e->cX < n && e->cY < n) hmm_addToEmissionsExpectation(e->hmm, t, e->cX, e->cY, pr);
}

static void foreign_emitter(StateMachine *sM, int64_t xay, DpMatrix *forward, DpMatrix *backward, const SymbolString sX,
                            const SymbolString sY, double total, PairwiseAlignmentParameters *p, void *extraArgs) {
    Foreign *f = ((void **)extraArgs)[1];
    check_contract(f, xay, forward, backward, sX, sY);
    DpDiagonal *fRow = dpMatrix_getDiagonal(forward, xay), *bRow = dpMatrix_getDiagonal(backward, xay);
    if (!fRow || !bRow) return;
    if (f->kind == EXPECT) {
        DpDiagonal *m1 = dpMatrix_getDiagonal(forward, xay - 1), *m2 = dpMatrix_getDiagonal(forward, xay - 2);
        f->hmm->likelihood += total;
        FOR_CELLS(bRow, xay, sX.length, sY.length, xmy) {
            const int64_t x = diagonal_getXCoordinate(xay, xmy), y = diagonal_getYCoordinate(xay, xmy);
            Event e = {total, f->hmm, x > 0 ? sX.sequence[x - 1] : n, y > 0 ? sY.sequence[y - 1] : n};
            sM->cellCalculate(sM, dpDiagonal_getCell(bRow, xmy), m1 ? dpDiagonal_getCell(m1, xmy - 1) : NULL,
                              m2 ? dpDiagonal_getCell(m2, xmy) : NULL, m1 ? dpDiagonal_getCell(m1, xmy + 1) : NULL, e.cX, e.cY,
                              count_event, &e);
        }
        return;
    }
    FOR_CELLS(fRow, xay, sX.length, sY.length, xmy) {
        const int64_t x = diagonal_getXCoordinate(xay, xmy), y = diagonal_getYCoordinate(xay, xmy);
        const double *fc = dpDiagonal_getCell(fRow, xmy), *bc = dpDiagonal_getCell(bRow, xmy);
        CHECK(bc != NULL);
        if (!bc) continue;
        if (x > 0 && y > 0) keep(f->lists[0], exp(fc[sM->matchState] + bc[sM->matchState] - total), p->threshold, x, y);
        if (f->kind == INDEL && x > 0) keep(f->lists[1], exp(fc[sM->gapXState] + bc[sM->gapXState] - total), p->threshold, x, y);
        if (f->kind == INDEL && y > 0) keep(f->lists[2], exp(fc[sM->gapYState] + bc[sM->gapYState] - total), p->threshold, x, y);
    }
}

static void correction(int64_t x1, int64_t y1, void *extraArgs) {
    Foreign *f = ((void **)extraArgs)[1];
    CHECK(f->corrections < f->nRegions);
    if (f->corrections < f->nRegions) CHECK(f->regions[f->corrections].x1 == x1 && f->regions[f->corrections].y1 == y1);
    f->corrections++;
}

/* ---- the comparison of two lists ---- */
static int at_threshold(int64_t score, double threshold) {
    return fabs((double)score - threshold * PAIR_ALIGNMENT_PROB_1) <= 1e-5 * threshold * PAIR_ALIGNMENT_PROB_1 + 1.0;
}
static void compare_lists(const char *what, stList *got, stList *want, double threshold) {
    int64_t i = 0, j = 0, excused = 0;
    const int64_t nG = stList_length(got), nW = stList_length(want);
    while (i < nG || j < nW) {
        stIntTuple *u = i < nG ? stList_get(got, i) : NULL, *v = j < nW ? stList_get(want, j) : NULL;
        if (u && v && stIntTuple_get(u, 1) == stIntTuple_get(v, 1) && stIntTuple_get(u, 2) == stIntTuple_get(v, 2)) {
            const double a = (double)stIntTuple_get(u, 0), b = (double)stIntTuple_get(v, 0), tol = 1e-5 * b > 1.0 ? 1e-5 * b : 1.0;
            if (fabs(a - b) > tol) {
                fprintf(stderr, "%s: pair (%lld, %lld): foreign %.0f, token %.0f\n", what, (long long)stIntTuple_get(u, 1),
                        (long long)stIntTuple_get(u, 2), a, b);
                failures++;
            }
            i++;
            j++;
        } else if (u && at_threshold(stIntTuple_get(u, 0), threshold)) { /* on one side only, at the threshold */
            excused++;
            i++;
        } else if (v && at_threshold(stIntTuple_get(v, 0), threshold)) {
            excused++;
            j++;
        } else {
            fprintf(stderr, "%s: the lists part at foreign %lld of %lld, token %lld of %lld\n", what, (long long)i, (long long)nG,
                    (long long)j, (long long)nW);
            failures++;
            return;
        }
    }
    if (excused * 100 > nW) {
        fprintf(stderr, "%s: %lld of %lld pairs excused at the threshold\n", what, (long long)excused, (long long)nW);
        failures++;
    }
}

static double worstExpect = 0.0;
static void compare_entry(const char *what, const char *entry, double got, double want) {
    const double scale = fabs(got) > fabs(want) ? fabs(got) : fabs(want);
    if (scale == 0.0) return;
    const double rel = fabs(got - want) / scale;
    if (rel > worstExpect) worstExpect = rel;
    if (!(rel <= 1e-5)) {
        fprintf(stderr, "%s: %s: foreign %.17g, token %.17g (%.3g relative)\n", what, entry, got, want, rel);
        failures++;
    }
}

/* ---- the regions of an entry-point call and their schedules ---- */
static void params_of(const PairwiseAlignmentParameters *p, cpecan_params *q) {
    memset(q, 0, sizeof *q);
    q->threshold = p->threshold;
    q->minDiagsBetweenTraceBack = p->minDiagsBetweenTraceBack;
    q->traceBackDiagonals = p->traceBackDiagonals;
    q->diagonalExpansion = p->diagonalExpansion;
    q->splitMatrixBiggerThanThis = p->splitMatrixBiggerThanThis;
    q->dynamicAnchorExpansion = p->dynamicAnchorExpansion;
}
static stList *anchor_list(const Case *cs) {
    stList *l = stList_construct3(0, (void (*)(void *))stIntTuple_destruct);
    for (int64_t i = 0; i < cs->nAnchors; i++)
        stList_append(l, stIntTuple_construct3(cs->anchors[3 * i], cs->anchors[3 * i + 1], cs->anchors[3 * i + 2]));
    return l;
}
static Region *regions_of(const Case *cs, int split, int64_t *nRegions) {
    stList *anchors = anchor_list(cs);
    stList *rects = NULL;
    int64_t nR = 1;
    if (split) {
        rects = getSplitPoints(anchors, cs->lX, cs->lY, cs->p->splitMatrixBiggerThanThis, cs->raggedLeft, cs->raggedRight);
        nR = stList_length(rects);
    }
    Region *out = calloc((size_t)nR + 1, sizeof *out);
    int64_t *sub = malloc(sizeof(int64_t) * 3 * (size_t)(cs->nAnchors + 1));
    cpecan_params q;
    params_of(cs->p, &q);
    int64_t j = 0;
    for (int64_t i = 0; i < nR; i++) {
        Region *rg = &out[i];
        int64_t x2 = cs->lX, y2 = cs->lY;
        if (split) {
            stIntTuple *r4 = stList_get(rects, i);
            rg->x1 = stIntTuple_get(r4, 0);
            rg->y1 = stIntTuple_get(r4, 1);
            x2 = stIntTuple_get(r4, 2);
            y2 = stIntTuple_get(r4, 3);
        }
        rg->lX = x2 - rg->x1;
        rg->lY = y2 - rg->y1;
        int64_t m = 0;
        for (; j < cs->nAnchors && (!split || cs->anchors[3 * j] + cs->anchors[3 * j + 1] < x2 + y2); j++, m++) {
            sub[3 * m] = cs->anchors[3 * j] - rg->x1;
            sub[3 * m + 1] = cs->anchors[3 * j + 1] - rg->y1;
            sub[3 * m + 2] = cs->anchors[3 * j + 2];
        }
        CHECK(cpecan_dense_schedule(rg->lX, rg->lY, sub, m, &q, NULL, 0, &rg->nSegs, NULL, 0, &rg->nCalls) == CPECAN_OK);
        CHECK(rg->nCalls == rg->lX + rg->lY);
        rg->calls = calloc((size_t)rg->nCalls + 1, sizeof *rg->calls);
        CHECK(cpecan_dense_schedule(rg->lX, rg->lY, sub, m, &q, NULL, 0, NULL, rg->calls, rg->nCalls, NULL) == CPECAN_OK);
    }
    free(sub);
    if (rects) stList_destruct(rects);
    stList_destruct(anchors);
    *nRegions = nR;
    return out;
}

typedef void (*Emitter)(StateMachine *, int64_t, DpMatrix *, DpMatrix *, const SymbolString, const SymbolString, double,
                        PairwiseAlignmentParameters *, void *);
static void call_entry(const Case *cs, int split, Emitter fn, void *extraArgs, void (*fix)()) {
    stList *anchors = anchor_list(cs);
    if (split) {
        getPosteriorProbsWithBandingSplittingAlignmentsByLargeGaps(cs->sM, anchors, cs->sx, cs->sy, cs->lX, cs->lY, cs->p, cs->raggedLeft,
                                                                   cs->raggedRight, fn, fix, extraArgs);
    } else {
        SymbolString sX = symbolString_construct(cs->sx, cs->lX), sY = symbolString_construct(cs->sy, cs->lY);
        getPosteriorProbsWithBanding(cs->sM, anchors, sX, sY, cs->p, cs->raggedLeft, cs->raggedRight, fn, extraArgs);
        free(sX.sequence);
        free(sY.sequence);
    }
    stList_destruct(anchors);
}

static stList *new_list(void) { return stList_construct3(0, (void (*)(void *))stIntTuple_destruct); }

static void run_case(const Case *cs, int split, FILE *out) {
    int64_t nRegions = 0, expectedBottoms = 0, totalCalls = 0;
    Region *regions = regions_of(cs, split, &nRegions);
    for (int64_t i = 0; i < nRegions; i++) {
        expectedBottoms += regions[i].nSegs > 0 ? regions[i].nSegs - 1 : 0;
        totalCalls += regions[i].nCalls;
    }
    char what[160];
    for (int kind = MATCH; kind <= EXPECT; kind++) {
        Foreign f;
        memset(&f, 0, sizeof f);
        f.kind = kind;
        f.regions = regions;
        f.nRegions = nRegions;
        snprintf(what, sizeof what, "%s %s %s", cs->name, split ? "splitting" : "banding", kind == MATCH ? "match" : kind == INDEL ? "indel" : "expect");
        if (kind == EXPECT) {
            Hmm *token = hmm_constructEmpty(0.0, cs->sM->type);
            f.hmm = hmm_constructEmpty(0.0, cs->sM->type);
            void *extra[2] = {NULL, &f};
            call_entry(cs, split, diagonalCalculationExpectations, token, NULL);
            call_entry(cs, split, foreign_emitter, extra, NULL);
            const int64_t S = f.hmm->stateNumber;
            char entry[32];
            for (int64_t i = 0; i < S * S; i++) {
                snprintf(entry, sizeof entry, "T[%lld]", (long long)i);
                compare_entry(what, entry, f.hmm->transitions[i], token->transitions[i]);
            }
            for (int64_t i = 0; i < S * 16; i++) {
                snprintf(entry, sizeof entry, "E[%lld]", (long long)i);
                compare_entry(what, entry, f.hmm->emissions[i], token->emissions[i]);
            }
            compare_entry(what, "likelihood", f.hmm->likelihood, token->likelihood);
            fprintf(out, "%s %d %lld", cs->name, split, (long long)S);
            for (int64_t i = 0; i < S * S; i++) fprintf(out, " %.17g", f.hmm->transitions[i]);
            for (int64_t i = 0; i < S * 16; i++) fprintf(out, " %.17g", f.hmm->emissions[i]);
            fprintf(out, " %.17g\n", f.hmm->likelihood);
            hmm_destruct(token);
            hmm_destruct(f.hmm);
        } else {
            stList *token[3] = {new_list(), new_list(), new_list()};
            for (int l = 0; l < 3; l++) f.lists[l] = new_list();
            Foreign tf; /* the token's calls reach only the correction */
            memset(&tf, 0, sizeof tf);
            tf.regions = regions;
            tf.nRegions = nRegions;
            void *tokenExtra[5] = {token[0], &tf, token[1], NULL, token[2]}, *extra[5] = {f.lists[0], &f, f.lists[1], NULL, f.lists[2]};
            call_entry(cs, split, kind == MATCH ? diagonalCalculationPosteriorMatchProbs : diagonalCalculationPosteriorProbs, tokenExtra,
                       (void (*)())correction);
            call_entry(cs, split, foreign_emitter, extra, (void (*)())correction);
            if (split) CHECK(tf.corrections == nRegions && f.corrections == nRegions);
            for (int l = 0; l < (kind == MATCH ? 1 : 3); l++) {
                char which[200];
                snprintf(which, sizeof which, "%s list %d", what, l);
                compare_lists(which, f.lists[l], token[l], cs->p->threshold);
            }
            printf("%s: %lld / %lld / %lld entries\n", what, (long long)stList_length(f.lists[0]), (long long)stList_length(f.lists[1]),
                   (long long)stList_length(f.lists[2]));
            for (int l = 0; l < 3; l++) {
                stList_destruct(token[l]);
                stList_destruct(f.lists[l]);
            }
        }
        while (f.region < f.nRegions && f.at == regions[f.region].nCalls) { /* every call owed was made */
            f.region++;
            f.at = 0;
        }
        CHECK(f.region == f.nRegions);
        CHECK(f.bottoms == expectedBottoms);
    }
    printf("%s %s: %lld region(s), %lld calls, %lld traceback bottoms\n", cs->name, split ? "splitting" : "banding", (long long)nRegions,
           (long long)totalCalls, (long long)expectedBottoms);
    for (int64_t i = 0; i < nRegions; i++) free(regions[i].calls);
    free(regions);
}

/* ---- the cases file ----
 * nCases, then per case: name type hasHmm [S*S transitions, S*16 emissions] threshold minDiagsBetweenTraceBack traceBackDiagonals
 * diagonalExpansion splitMatrixBiggerThanThis dynamicAnchorExpansion raggedLeft raggedRight lX sX lY sY nAnchors (x y e)*; a
 * sequence of length 0 is written as "-"; doubles as hexadecimal floats */
static double read_double(FILE *in) {
    char tok[64];
    if (fscanf(in, "%63s", tok) != 1) {
        fprintf(stderr, "cases file: a number is missing\n");
        exit(2);
    }
    return strtod(tok, NULL);
}
static long long read_int(FILE *in) {
    long long v;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "cases file: an integer is missing\n");
        exit(2);
    }
    return v;
}
static char *read_seq(FILE *in, int64_t *length) {
    *length = read_int(in);
    char *s = malloc((size_t)*length + 2);
    if (fscanf(in, " %[^ \n]", s) != 1) exit(2); /* "-" for an empty sequence */
    if (*length == 0) s[0] = 0;
    return s;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <cases file> <output file>\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    const long long nCases = read_int(in);
    for (long long k = 0; k < nCases; k++) {
        Case cs;
        memset(&cs, 0, sizeof cs);
        if (fscanf(in, "%63s", cs.name) != 1) return 2;
        const StateMachineType type = (StateMachineType)read_int(in);
        if (read_int(in)) {
            Hmm *h = hmm_constructEmpty(0.0, type);
            for (int64_t i = 0; i < h->stateNumber * h->stateNumber; i++) h->transitions[i] = read_double(in);
            for (int64_t i = 0; i < h->stateNumber * 16; i++) h->emissions[i] = read_double(in);
            cs.sM = hmm_getStateMachine(h);
            hmm_destruct(h);
        } else {
            cs.sM = (type == fiveState || type == fiveStateAsymmetric) ? stateMachine5_construct(type) : stateMachine3_construct(type);
        }
        cs.p = pairwiseAlignmentBandingParameters_construct();
        cs.p->threshold = read_double(in);
        cs.p->minDiagsBetweenTraceBack = read_int(in);
        cs.p->traceBackDiagonals = read_int(in);
        cs.p->diagonalExpansion = read_int(in);
        cs.p->splitMatrixBiggerThanThis = read_int(in);
        cs.p->dynamicAnchorExpansion = read_int(in) != 0;
        cs.raggedLeft = (int)read_int(in);
        cs.raggedRight = (int)read_int(in);
        cs.sx = read_seq(in, &cs.lX);
        cs.sy = read_seq(in, &cs.lY);
        cs.nAnchors = read_int(in);
        cs.anchors = malloc(sizeof(int64_t) * 3 * (size_t)(cs.nAnchors + 1));
        for (int64_t i = 0; i < 3 * cs.nAnchors; i++) cs.anchors[i] = read_int(in);
        run_case(&cs, 0, out);
        run_case(&cs, 1, out);
        free(cs.anchors);
        free(cs.sx);
        free(cs.sy);
        pairwiseAlignmentBandingParameters_destruct(cs.p);
        stateMachine_destruct(cs.sM);
    }
    fclose(in);
    fclose(out);
    printf("largest relative difference of an expectation entry, foreign against token: %.3g\n", worstExpect);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
