/* The host side of the dense rows (cpecan_amd/csrc/cpecan_dense.c) and the replay of foreign emitters over them
 * (cpecan_amd/csrc/cpecan_dropin.c), stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer: built by
 * tests/test_foreign_emitter_c.py from the sources, with tests/c/device_standins.h in place of the device layer and a stand-in
 * cpk_dense_run below that FABRICATES the rows -- every double tells which array and which index it was written to, so a
 * callback that reads every cell of every live row checks every offset of the host code: between problems, between
 * diagonals, and of the Bnext rows in the tracebacks' side array.  No library, no HIP, no GPU.  Prints "N failure(s)". */
#define _POSIX_C_SOURCE 200809L
#include <math.h>

#include "device_standins.h"

#include "cpecan_dense.h"
#include "cpecan_dropin.h"

/* ---- the fabricated device ---- */
#define MARK_F 0.25
#define MARK_B 0.5
#define MARK_SIDE 0.75
#define MARK_TOTAL 0.125
static double fabricated(int64_t index, double mark) { return -(double)index - mark; }

static struct {
    CpkDenseProblem *problems;
    CpkDenseDiag *diags;
    CpkDenseSeg *segs;
    int64_t nProblems, nDiags, nSegs;
    int S;
} last; /* the job of the last run, kept for the callback */

int64_t cpk_dense_device_bytes(const CpkDenseJob *j, int S) { return 8 * ((2 * j->totalCells + j->sideCells) * S + j->nDiags); }
int cpk_dense_run(int device, const CpkModel *model, const CpkDenseJob *j, double *kernelMs) {
    (void)device;
    free(last.problems);
    free(last.diags);
    free(last.segs);
    last.S = model->nStates;
    last.nProblems = j->nProblems;
    last.nDiags = j->nDiags;
    last.nSegs = j->nSegs;
    last.problems = malloc(sizeof *last.problems * (size_t)(j->nProblems + 1));
    last.diags = malloc(sizeof *last.diags * (size_t)(j->nDiags + 1));
    last.segs = malloc(sizeof *last.segs * (size_t)(j->nSegs + 1));
    memcpy(last.problems, j->problems, sizeof *last.problems * (size_t)j->nProblems);
    memcpy(last.diags, j->diags, sizeof *last.diags * (size_t)j->nDiags);
    memcpy(last.segs, j->segs, sizeof *last.segs * (size_t)j->nSegs);
    for (int64_t i = 0; i < j->totalCells * last.S; i++) {
        j->F[i] = fabricated(i, MARK_F);
        j->B[i] = fabricated(i, MARK_B);
    }
    for (int64_t i = 0; i < j->sideCells * last.S; i++) j->side[i] = fabricated(i, MARK_SIDE);
    for (int64_t i = 0; i < j->nDiags; i++) j->totals[i] = fabricated(i, MARK_TOTAL);
    if (kernelMs) *kernelMs = 0.0;
    return CPECAN_OK;
}
/* ---- the callback ---- */
typedef struct {
    int64_t problem, calls, callsOfProblem, cellsRead;
} Walk;

static void read_row(DpMatrix *m, int64_t r, int64_t base, double mark, Walk *w) {
    DpDiagonal *row = dpMatrix_getDiagonal(m, r);
    CHECK(row != NULL);
    if (!row) return;
    const CpkDenseProblem *pb = &last.problems[w->problem];
    const CpkDenseDiag g = last.diags[pb->diagOff + r];
    CHECK(dpDiagonal_getCell(row, g.xmyL - 2) == NULL && dpDiagonal_getCell(row, g.xmyL + 2 * (int64_t)g.width) == NULL);
    for (int64_t k = 0; k < g.width; k++) {
        const double *cell = dpDiagonal_getCell(row, g.xmyL + 2 * k);
        CHECK(cell != NULL);
        if (!cell) return;
        for (int s = 0; s < last.S; s++) CHECK(cell[s] == fabricated((base + k) * last.S + s, mark));
        w->cellsRead++;
    }
}

static void walker(StateMachine *sM, int64_t xay, DpMatrix *forward, DpMatrix *backward, const SymbolString sX, const SymbolString sY,
                   double total, PairwiseAlignmentParameters *p, void *extraArgs) {
    (void)p;
    Walk *w = extraArgs;
    while (w->problem < last.nProblems && w->callsOfProblem == last.problems[w->problem].lX + last.problems[w->problem].lY) {
        w->problem++;
        w->callsOfProblem = 0;
    }
    CHECK(w->problem < last.nProblems);
    if (w->problem >= last.nProblems) return;
    const CpkDenseProblem *pb = &last.problems[w->problem];
    const int64_t N = pb->lX + pb->lY;
    CHECK(sX.length == pb->lX && sY.length == pb->lY && sM->stateNumber == last.S);
    const CpkDenseSeg *sg = NULL; /* the traceback that emits xay */
    for (int64_t k = 0; k < last.nSegs; k++)
        if (last.segs[k].problem == w->problem && xay > last.segs[k].tbPrev && xay <= last.segs[k].tbFrom) sg = &last.segs[k];
    CHECK(sg != NULL);
    if (!sg) return;
    CHECK(total == fabricated(pb->diagOff + xay, MARK_TOTAL));
    int64_t nF = 0, nB = 0;
    for (int64_t r = sg->tbPrev; r <= sg->dTop; r++) { /* forward: tbPrev .. xay and, unless dTop == N, tbFrom .. dTop */
        if (!(r <= xay || (sg->dTop != N && r >= sg->tbFrom))) continue;
        read_row(forward, r, pb->cellBase + last.diags[pb->diagOff + r].cellOff, MARK_F, w);
        nF++;
    }
    for (int64_t r = xay - 1; r <= xay + 1; r++) { /* backward: xay - 1 .. xay + 1 inside tbPrev + 1 .. dTop */
        if (r <= sg->tbPrev || r > sg->dTop) continue;
        if (r <= sg->tbFrom) read_row(backward, r, pb->cellBase + last.diags[pb->diagOff + r].cellOff, MARK_B, w);
        else read_row(backward, r, sg->sideBase, MARK_SIDE, w); /* Bnext: the first of the traceback's side rows */
        nB++;
    }
    CHECK(dpMatrix_getActiveDiagonalNumber(forward) == nF && dpMatrix_getActiveDiagonalNumber(backward) == nB);
    if (xay == sg->tbPrev + 1 && sg->tbPrev >= 1) CHECK(dpMatrix_getDiagonal(forward, xay - 2) == NULL);
    CHECK(dpMatrix_getDiagonal(backward, xay - 2) == NULL);
    w->calls++;
    w->callsOfProblem++;
}

static int64_t corrections = 0;
static void correction(int64_t x1, int64_t y1, void *extraArgs) {
    (void)x1, (void)y1, (void)extraArgs;
    corrections++;
}

static char *random_sequence(unsigned *state, int64_t length) {
    char *s = malloc((size_t)length + 1);
    for (int64_t i = 0; i < length; i++) {
        *state = *state * 1103515245u + 12345u;
        s[i] = "ACGTNacgt"[(*state >> 16) % 9];
    }
    s[length] = 0;
    return s;
}

int main(void) {
    unsigned rng = 7;
    /* 1. the object itself: several problems, offsets between them, results dropped by a later add, the cap, errors */
    cpecan_dense *d = NULL;
    cpecan_model model;
    memset(&model, 0, sizeof model);
    model.type = CPECAN_THREE_STATE;
    cpecan_params prm;
    cpecan_params_default(&prm);
    prm.minDiagsBetweenTraceBack = 12;
    prm.traceBackDiagonals = 3;
    prm.diagonalExpansion = 4;
    CHECK(cpecan_dense_create(&d, &model, &prm, 0) == CPECAN_OK);
    char *sx = random_sequence(&rng, 60), *sy = random_sequence(&rng, 57);
    const int64_t anchors[9] = {10, 9, 0, 30, 28, 0, 50, 47, 0};
    CHECK(cpecan_dense_add(d, sx, 60, sy, 57, anchors, 3, 0, 1) == 0);
    CHECK(cpecan_dense_add(d, "", 0, "", 0, NULL, 0, 0, 0) == 1);
    CHECK(cpecan_dense_add(d, sx, 7, "", 0, NULL, 0, 1, 0) == 2);
    const int64_t bad[6] = {5, 5, 0, 4, 6, 0};
    CHECK(cpecan_dense_add(d, sx, 60, sy, 57, bad, 2, 0, 0) == CPECAN_EINVAL);
    cpecan_dense_rows_t rows;
    CHECK(cpecan_dense_rows(d, 0, &rows) == CPECAN_ESTATE);
    CHECK(cpecan_dense_run(d) == CPECAN_OK); /* the fabricating stand-in above */
    CHECK(last.nProblems == 3 && last.problems[1].cellBase == last.problems[2].cellBase && last.problems[2].cellBase > 0);
    CHECK(cpecan_dense_rows(d, 0, &rows) == CPECAN_OK && rows.F[0] == fabricated(0, MARK_F) && rows.B[4] == fabricated(4, MARK_B));
    CHECK(rows.totalUsed[117] == fabricated(117, MARK_TOTAL) && rows.cellOff[0] == 0 && rows.cellOff[1] == 1);
    for (int64_t k = 0; k + 1 < last.nSegs; k++) /* Bnext: the first side row of every traceback but a problem's last */
        if (last.segs[k].problem == 0 && last.segs[k].tbFrom < last.segs[k].dTop)
            CHECK(rows.Bnext[rows.bnextOff[k] * 3] == fabricated(last.segs[k].sideBase * 3, MARK_SIDE) &&
                  rows.bnextOff[k + 1] - rows.bnextOff[k] == rows.diags[rows.segs[k].tbFrom + 1].width);
    CHECK(cpecan_dense_rows(d, 2, &rows) == CPECAN_OK && rows.F[0] == fabricated(last.problems[2].cellBase * 3, MARK_F));
    CHECK(rows.totalUsed[1] == fabricated(118 + 1, MARK_TOTAL) && rows.bnextOff[1] == 0);
    CHECK(cpecan_dense_rows(d, 1, &rows) == CPECAN_OK); /* no rows; nothing to read */
    setenv("CPECAN_DENSE_MAX_BYTES", "100", 1);
    CHECK(cpecan_dense_run(d) == CPECAN_ENOMEM && strstr(cpk_last_error(), "bytes") != NULL);
    unsetenv("CPECAN_DENSE_MAX_BYTES");
    CHECK(cpecan_dense_rows(d, 0, &rows) == CPECAN_ESTATE); /* a refused run leaves no results */
    CHECK(cpecan_dense_run(d) == CPECAN_OK);
    CHECK(cpecan_dense_add(d, sy, 5, sx, 9, NULL, 0, 0, 0) == 3); /* an add drops the results */
    CHECK(cpecan_dense_rows(d, 0, &rows) == CPECAN_ESTATE);
    cpecan_dense_info_t info;
    CHECK(cpecan_dense_info(d, 0, &info) == CPECAN_OK && info.nDiagonals == 118 && info.nStates == 3 && info.nSegments >= 3);
    CHECK(cpecan_dense_info(d, 1, &info) == CPECAN_OK && info.nDiagonals == 0 && info.nCells == 0 && info.nSegments == 0);
    CHECK(cpecan_dense_info(d, 2, &info) == CPECAN_OK && info.nDiagonals == 8 && info.nCells == 8 && info.nSegments == 1);
    CHECK(cpecan_dense_info(d, 4, &info) == CPECAN_EINVAL);
    cpecan_dense_destroy(d);
    cpecan_dense_destroy(NULL);

    /* 2. the schedule */
    cpecan_dense_seg segs[64];
    int64_t nSegs = 0, nCalls = 0;
    CHECK(cpecan_dense_schedule(60, 57, anchors, 3, &prm, segs, 64, &nSegs, NULL, 0, &nCalls) == CPECAN_OK && nCalls == 117 && nSegs >= 3);
    cpecan_dense_call *calls = malloc(sizeof *calls * (size_t)nCalls);
    CHECK(cpecan_dense_schedule(60, 57, anchors, 3, &prm, segs, 2, NULL, calls, nCalls, NULL) == CPECAN_OK); /* fewer segments than there are */
    CHECK(calls[0].xay == segs[0].tbFrom && calls[nCalls - 1].xay == segs[nSegs > 64 ? 63 : nSegs - 1].tbPrev + 1 - 0);
    free(calls);
    CHECK(cpecan_dense_schedule(0, 0, NULL, 0, NULL, NULL, 0, &nSegs, NULL, 0, &nCalls) == CPECAN_OK && nSegs == 0 && nCalls == 0);

    /* 3. the replay through both entry points */
    StateMachine *sM = stateMachine3_construct(threeState);
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    p->minDiagsBetweenTraceBack = 12;
    p->traceBackDiagonals = 3;
    p->diagonalExpansion = 4;
    stList *anchorList = stList_construct3(0, (void (*)(void *))stIntTuple_destruct);
    for (int i = 0; i < 3; i++) stList_append(anchorList, stIntTuple_construct3(anchors[3 * i], anchors[3 * i + 1], anchors[3 * i + 2]));
    SymbolString sX = symbolString_construct(sx, 60), sY = symbolString_construct(sy, 57);
    Walk w;
    memset(&w, 0, sizeof w);
    getPosteriorProbsWithBanding(sM, anchorList, sX, sY, p, 0, 1, walker, &w);
    CHECK(w.calls == 117 && w.cellsRead > 117 * 3);
    /* ... an empty problem makes no call */
    SymbolString none = symbolString_construct("", 0);
    memset(&w, 0, sizeof w);
    stList *noAnchors = stList_construct3(0, (void (*)(void *))stIntTuple_destruct);
    getPosteriorProbsWithBanding(sM, noAnchors, none, none, p, 0, 0, walker, &w);
    CHECK(w.calls == 0);
    stList_destruct(noAnchors);
    free(none.sequence);
    /* ... the splitting entry point: rectangles of one object, one run */
    p->splitMatrixBiggerThanThis = 12 * 12;
    stList *rects = getSplitPoints(anchorList, 60, 57, p->splitMatrixBiggerThanThis, 0, 1);
    const int64_t nRects = stList_length(rects);
    CHECK(nRects >= 3);
    int64_t owed = 0;
    for (int64_t i = 0; i < nRects; i++) {
        stIntTuple *r4 = stList_get(rects, i);
        owed += stIntTuple_get(r4, 2) - stIntTuple_get(r4, 0) + stIntTuple_get(r4, 3) - stIntTuple_get(r4, 1);
    }
    stList_destruct(rects);
    memset(&w, 0, sizeof w);
    getPosteriorProbsWithBandingSplittingAlignmentsByLargeGaps(sM, anchorList, sx, sy, 60, 57, p, 0, 1, walker, (void (*)())correction, &w);
    CHECK(last.nProblems == nRects && corrections == nRects && w.calls == owed);
    free(sX.sequence);
    free(sY.sequence);
    stList_destruct(anchorList);
    pairwiseAlignmentBandingParameters_destruct(p);
    stateMachine_destruct(sM);
    free(sx);
    free(sy);
    free(last.problems);
    free(last.diags);
    free(last.segs);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
