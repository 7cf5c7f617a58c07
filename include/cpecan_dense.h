/*
 * cpecan_dense.h -- dense forward / backward rows of a region: every state of F and B for every band cell, and the total the
 * reference hands its emitter on every diagonal, computed on the GPU under the reference's traceback schedule.
 *
 * Reference: getPosteriorProbsWithBanding (impl/pairwiseAligner.c:756-877) calls a per-diagonal emitter
 * (inc/pairwiseAligner.h:245-248) with its forward and backward DpMatrix.  The three emitters the reference ships run on
 * kernels of their own (CPECAN_EMIT_MATCH / INDEL / EXPECT); this is the result form for every OTHER emitter: the rows it
 * would have been shown.  include/cpecan_dropin.h replays a foreign callback over them.  One problem = one region: the
 * dense path never splits (splitMatrixBiggerThanThis is ignored; the drop-in layer hands over one problem per rectangle).
 *
 * Layout.  N = lX + lY, diagonals 0 .. N, S states.  Cells are ordered by diagonal, then x - y ascending; cell k of
 * diagonal d is cell cellOff[d] + k and has x - y = diags[d].xmyL + 2 k.
 *   F          [nCells][S]  forward values, the start prior (or the ragged start prior) on diagonal 0
 *   B          [nCells][S]  backward values; diagonal d holds the values of the ONE traceback that emits d.  Diagonal 0: NaN
 *   segs       the tracebacks (tbPrev, dTop, tbFrom) in ascending order (:791-810): seeded with the end prior at dTop (the
 *              ragged end prior only when dTop == N && raggedRight), emitting tbFrom down to tbPrev + 1
 *   Bnext      for every traceback but the last one more row: ITS backward values on diagonal tbFrom + 1, which the next
 *              traceback emits with other values.  The emitter of tbFrom and the total's straddle term need it.  The row of
 *              traceback k starts at cell bnextOff[k] of Bnext; bnextOff has nSegments + 1 entries, the last row is empty
 *   totalUsed  [nDiagonals] the total the reference passes when it emits d: refreshed on the 1st, 11th, 21st ... emitted
 *              diagonal of each traceback, counting down from tbFrom (:830-838), folded as
 *              diagonalCalculationTotalProbability does (:636-653): cells ascending, states ascending, then the straddle
 *              term.  totalUsed[0]: NaN
 * With the library built with -DCPK_LOGADD_EXACT=1 every value is the reference's to the bit.
 */
#ifndef CPECAN_DENSE_H_
#define CPECAN_DENSE_H_

#include "cpecan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cpecan_dense cpecan_dense;

typedef struct cpecan_dense_info_t {
    int64_t nDiagonals; /* lX + lY + 1, or 0 for lX + lY == 0: a legal problem without rows */
    int64_t nCells;
    int64_t nSegments;
    int64_t nStates;
} cpecan_dense_info_t;

typedef struct cpecan_dense_diag {
    int32_t xmyL, width;
} cpecan_dense_diag;

typedef struct cpecan_dense_seg {
    int32_t tbPrev, dTop, tbFrom;
} cpecan_dense_seg;

/* Borrowed host pointers, valid until the object's next run or its destruction. */
typedef struct cpecan_dense_rows_t {
    const cpecan_dense_diag *diags; /* [nDiagonals] */
    const int64_t *cellOff;         /* [nDiagonals + 1] */
    const double *F, *B;            /* [nCells * nStates] */
    const double *Bnext;            /* [bnextOff[nSegments] * nStates] */
    const int64_t *bnextOff;        /* [nSegments + 1], in cells */
    const double *totalUsed;        /* [nDiagonals] */
    const cpecan_dense_seg *segs;   /* [nSegments] */
} cpecan_dense_rows_t;

/* params NULL = the defaults.  CPECAN_EINVAL for a model type or banding parameters the reference asserts on
 * (pairwiseAligner.c:761-765).  No device is touched before cpecan_dense_run. */
int cpecan_dense_create(cpecan_dense **out, const cpecan_model *model, const cpecan_params *params, int device);
void cpecan_dense_destroy(cpecan_dense *d);

/* Copies the problem; anchors are (x, y, expansion) triples checked as cpecan_batch_add checks them (strictly increasing in
 * both coordinates, inside the matrix, a valid band).  params->dynamicAnchorExpansion is honoured.  Returns the problem's
 * index, or < 0.  Results of an earlier run are dropped. */
int64_t cpecan_dense_add(cpecan_dense *d, const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors,
                         int64_t nAnchors, int raggedLeft, int raggedRight);

/* All added problems in one launch sequence: the forward kernel over the problems, the backward kernel over their
 * tracebacks.  CPECAN_ENODEVICE without the device.  Refused with CPECAN_ENOMEM, and a message that names the bytes
 * needed, when the rows on the device would exceed CPECAN_DENSE_MAX_BYTES (the environment variable of that name overrides
 * the default).  A 2 kb five-state pair at expansion 100 needs about 39 MB. */
#define CPECAN_DENSE_MAX_BYTES ((int64_t)1 << 30)
int cpecan_dense_run(cpecan_dense *d);

/* Known from cpecan_dense_add on. */
int cpecan_dense_info(const cpecan_dense *d, int64_t problem, cpecan_dense_info_t *info);
/* After cpecan_dense_run (CPECAN_ESTATE before it). */
int cpecan_dense_rows(const cpecan_dense *d, int64_t problem, cpecan_dense_rows_t *rows);
/* HIP-event time of the last run's two kernels, milliseconds. */
double cpecan_dense_kernel_ms(const cpecan_dense *d);

/* One call of the reference's emitter and the rows its two matrices hold at that moment (inclusive ranges of diagonals; an
 * empty range is lo = 0, hi = -1).
 *   forward   rows fLo .. fHi = tbPrev .. xay and, unless dTop == N, rows f2Lo .. f2Hi = tbFrom .. dTop: the reference's live
 *             set (:843-855).  In particular row xay - 2 is ABSENT at xay == tbPrev + 1 for tbPrev >= 1: the reference has freed it
 *   backward  rows bLo .. bHi = xay - 1 .. xay + 1 clipped to tbPrev + 1 .. dTop, all with final values; row xay + 1 at
 *             xay == tbFrom is Bnext.  Row xay - 2, which the reference holds half-accumulated at that moment, is not served. */
typedef struct cpecan_dense_call {
    int64_t xay, seg;
    int64_t fLo, fHi, f2Lo, f2Hi;
    int64_t bLo, bHi;
} cpecan_dense_call;

/* Pure host code, no device: the tracebacks of a problem and the order in which the reference calls its emitter --
 * tracebacks ascending, inside a traceback from tbFrom down to tbPrev + 1.  Writes at most segCap segments and callCap
 * calls (either array may be NULL with a capacity of 0); *nSegs and *nCalls (may be NULL) receive how many there are: lX + lY
 * calls.  params NULL = the defaults. */
int cpecan_dense_schedule(int64_t lX, int64_t lY, const int64_t *anchors, int64_t nAnchors, const cpecan_params *params,
                          cpecan_dense_seg *segsOut, int64_t segCap, int64_t *nSegs, cpecan_dense_call *callsOut,
                          int64_t callCap, int64_t *nCalls);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_DENSE_H_ */
