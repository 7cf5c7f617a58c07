/*
 * cpecan_viterbi.h -- Viterbi decoding: the most probable banded state path of two sequences under a pair-HMM and its
 * log-probability, computed on the GPU.  Not in the reference; DESIGN.md section 12 is the definition.
 *
 * One problem = two sequences, anchors as (x, y, expansion) triples, the ragged flags.  Unlike the dense rows the problem IS
 * split: its regions are the rectangles of cpecan_split_points with params->splitMatrixBiggerThanThis, region i of n run
 * with raggedLeft || i > 0 and raggedRight || i < n - 1 over the anchors that fall into it (shifted), its band that of
 * cpecan_band with the parameters' expansion (dynamicAnchorExpansion honoured).
 *
 * Per region, S states, N = lX + lY, cell (x, y) sees cX = sX[x - 1], cY = sY[y - 1]:
 *   V[(0, 0)][s] = startvec[s]                               (the ragged start prior when the region is ragged left)
 *   per band cell of diagonals 1 .. N, over the model's ordered transition list (impl/stateMachine.c:450-480, :689-714):
 *       cand = V[src][from] + (e + tP);  cand > best[to] (strict)  ->  best[to] = cand, ptr[to] = from
 *   logP = max over s ascending, strict, of V[(lX, lY)][s] + endvec[s]; the winner is endState
 *   logP == -inf: no path (nOps = 0, startState = endState = -1).  Otherwise ptr is followed back to (0, 0); the state
 *   reached there is startState and emits nothing; the states of the steps, first to last, run-length encoded with maximal
 *   runs as (state, length) int32 pairs, are the ops.  A match state steps (x + 1, y + 1), a gap-X state (x + 1, y), a
 *   gap-Y state (x, y + 1).
 * The problem's logP is the plain double sum of its regions' logP in region order.  Only IEEE double additions and
 * comparisons: both builds of the library give the same bits.
 */
#ifndef CPECAN_VITERBI_H_
#define CPECAN_VITERBI_H_

#include "cpecan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cpecan_viterbi cpecan_viterbi;

typedef struct cpecan_viterbi_info_t {
    int64_t nRegions;
    int64_t nCells;      /* band cells of all regions, diagonal 0 of each included */
    int64_t nStates;
    int64_t deviceBytes; /* what the problem's regions take on the device: pointers, band records, symbols, rows, ops */
} cpecan_viterbi_info_t;

typedef struct cpecan_viterbi_region {
    int64_t x1, y1, x2, y2; /* the rectangle, problem coordinates */
    double logP;
    int32_t startState, endState; /* -1, -1: no path */
    int64_t opOff, nOps;          /* in (state, length) pairs, into the problem's ops */
} cpecan_viterbi_region;

/* Borrowed host pointers, valid until the object's next add, run or its destruction. */
typedef struct cpecan_viterbi_result_t {
    double logP;
    int64_t nRegions, nOps;
    const cpecan_viterbi_region *regions; /* [nRegions] */
    const int32_t *ops;                   /* [2 * nOps] */
} cpecan_viterbi_result_t;

/* Kernel forms: where the sweep keeps its three rolling rows of V. */
#define CPECAN_VITERBI_FORM_AUTO 0   /* per region: LDS where the widest diagonal fits, global memory where it does not */
#define CPECAN_VITERBI_FORM_LDS 1
#define CPECAN_VITERBI_FORM_GLOBAL 2
/* The widest diagonal, in cells, whose rows the LDS form holds. */
#define CPECAN_VITERBI_LDS_MAX_WIDTH 256

/* params NULL = the defaults.  CPECAN_EINVAL for a model type or banding parameters the reference asserts on.  No device is
 * touched before cpecan_viterbi_run. */
int cpecan_viterbi_create(cpecan_viterbi **out, const cpecan_model *model, const cpecan_params *params, int device);
void cpecan_viterbi_destroy(cpecan_viterbi *v);

/* Copies the problem; validates as cpecan_dense_add does, before any device is looked for.  Returns the problem's index, or
 * < 0.  Results of an earlier run are dropped. */
int64_t cpecan_viterbi_add(cpecan_viterbi *v, const char *sX, int64_t lX, const char *sY, int64_t lY, const int64_t *anchors,
                           int64_t nAnchors, int raggedLeft, int raggedRight);

/* The device bytes one launch may take: a budget, not a measured figure.  A run that needs more is cut into consecutive
 * launches of whole regions; only a single region above the budget makes cpecan_viterbi_run return CPECAN_ENOMEM, with the
 * bytes named in the message.  The result does not depend on the budget.  CPECAN_EINVAL for bytes <= 0. */
#define CPECAN_VITERBI_MAX_BYTES ((int64_t)4 << 30)
int cpecan_viterbi_set_budget(cpecan_viterbi *v, int64_t bytes);

/* CPECAN_VITERBI_FORM_*; CPECAN_EINVAL for any other value.  Every form gives the same bytes.  A run with
 * CPECAN_VITERBI_FORM_LDS forced over a region wider than CPECAN_VITERBI_LDS_MAX_WIDTH is CPECAN_EINVAL. */
int cpecan_viterbi_set_form(cpecan_viterbi *v, int form);

/* All added problems in as few launches as the budget allows.  CPECAN_ENODEVICE without the device. */
int cpecan_viterbi_run(cpecan_viterbi *v);

/* Of the last run: how many launches it was cut into and how many regions ran in the LDS and in the global form. */
int cpecan_viterbi_launch_forms(const cpecan_viterbi *v, int64_t *nLaunches, int64_t *nLds, int64_t *nGlobal);

/* Known from cpecan_viterbi_add on. */
int cpecan_viterbi_info(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_info_t *info);
/* After cpecan_viterbi_run (CPECAN_ESTATE before it). */
int cpecan_viterbi_result(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_result_t *res);
/* HIP-event times of the last run's sweep and traceback kernels, summed over its launches, milliseconds. */
int cpecan_viterbi_kernel_ms(const cpecan_viterbi *v, double *sweepMs, double *tracebackMs);

/* Pure host code, no device: walks the ops over ONE region (sX, sY: the region's own stretch of the sequences) and accumulates
 * v = startvec[startState], then v = v + (e + tP) per step, then v + endvec[endState] -- the additions the recurrence made
 * along that path, so *logP equals the region's logP to the bit.  CPECAN_EINVAL for ops that do not end at (lX, lY) or that
 * use a transition the model lacks. */
int cpecan_viterbi_replay(const cpecan_model *model, const char *sX, int64_t lX, const char *sY, int64_t lY, int raggedLeft,
                          int raggedRight, int startState, int endState, const int32_t *ops, int64_t nOps, double *logP);

/* The (x, y) of every match-state step of all regions, ascending, in problem coordinates, 0-based: what
 * cpecan_cigar_from_aligned_pairs_stranded takes.  Writes at most cap pairs (xy may be NULL with cap 0); returns how many
 * there are, or < 0. */
int64_t cpecan_viterbi_pairs(const cpecan_viterbi_result_t *res, int64_t *xy, int64_t cap);

/*
 * ---- Viterbi training's E-step: the counts of the decoded paths ----
 *
 * A region with a path (endState >= 0) has the start state q_0 and the steps t = 1 .. T; step t is in state q_t and ends at the
 * cell (x_t, y_t) of the region, which sees cX = symbol(sX[x_t - 1]) if x_t > 0, else N, and cY likewise
 * (impl/pairwiseAligner.c:597-607).  Its counts are updateExpectations (:418-432) with p = 1 for the transition taken:
 *     transitions[q_{t-1} * S + q_t] += 1              every step
 *     emissions[q_t * 16 + cX * 4 + cY] += 1           only where cX < 4 and cY < 4 -- the cell's symbols, not the state's: a
 *                                                      step on row or column 0, or on an N, counts its transition alone
 *     nSteps += T
 * The start and end priors count nothing.  A region without a path counts nothing, adds nothing to logP and one to nNoPath.
 * A problem's counts are the sums over its regions, the object's over its problems; logP is 0.0 plus the logP of the
 * contributing regions, one after the other in region order, whatever the cut into launches.
 */
typedef struct cpecan_viterbi_counts {
    int64_t transitions[25]; /* [from * nStates + to] */
    int64_t emissions[80];   /* [state * 16 + cX * 4 + cY] */
    int64_t nSteps, nNoPath;
    int64_t nStates;
    double logP;
} cpecan_viterbi_counts;

/* Another model of the same state count (CPECAN_EINVAL otherwise) for the next run.  Results of an earlier run are dropped;
 * what cpecan_viterbi_run_counts keeps on the device stays. */
int cpecan_viterbi_set_model(cpecan_viterbi *v, const cpecan_model *model);

/* Decodes every region and counts along the paths, on the device.  The first call plans the launches under the budget as
 * cpecan_viterbi_run does and uploads every launch's region records, band records, symbols and order; they stay there, beside
 * one scratch of the largest launch's size, until the next cpecan_viterbi_add, cpecan_viterbi_destroy, or a
 * cpecan_viterbi_set_budget / cpecan_viterbi_set_form that changes the value.  Later calls move the model down and the
 * per-region records and the bins up; the ops never leave the device, so cpecan_viterbi_result stays CPECAN_ESTATE
 * (cpecan_viterbi_launch_forms and cpecan_viterbi_kernel_ms answer for this run).  CPECAN_ENODEVICE without the device, after
 * the refusals cpecan_viterbi_run makes without one; CPECAN_ENOMEM, with the bytes named, where the resident inputs and the
 * scratch do not fit the device -- nothing is planned again.  The counts do not depend on the budget or the form. */
int cpecan_viterbi_run_counts(cpecan_viterbi *v, cpecan_viterbi_counts *total);

/* What cpecan_viterbi_run_counts keeps on the device under the present budget and form: the inputs of all launches, and the one
 * scratch beside them.  Host arithmetic; the refusals of cpecan_viterbi_run that need no device. */
int cpecan_viterbi_resident_bytes(const cpecan_viterbi *v, int64_t *inputBytes, int64_t *scratchBytes);

/* on != 0: cpecan_viterbi_run_counts also brings every region's bins home and sums them per problem.  Off by default. */
int cpecan_viterbi_set_keep_problem_counts(cpecan_viterbi *v, int on);
/* Of the last cpecan_viterbi_run_counts; CPECAN_ESTATE with the switch off or before that run. */
int cpecan_viterbi_problem_counts(const cpecan_viterbi *v, int64_t problem, cpecan_viterbi_counts *out);

/* HIP-event times of the last cpecan_viterbi_run_counts' count and reduce kernels, summed over its launches, milliseconds. */
int cpecan_viterbi_count_ms(const cpecan_viterbi *v, double *countMs, double *reduceMs);

/* Pure host code, no device: the definition above over ONE region's ops (first step first, as cpecan_viterbi_result gives
 * them); out->logP = 0.  CPECAN_EINVAL for ops that do not end at (lX, lY). */
int cpecan_viterbi_counts_of_ops(int nStates, const char *sX, int64_t lX, const char *sY, int64_t lY, int startState, const int32_t *ops,
                                 int64_t nOps, cpecan_viterbi_counts *out);

/* acc->transitions[i] += (double)transitions[i], acc->emissions[i] += (double)emissions[i], acc->likelihood += logP: exact below
 * 2^53.  CPECAN_EINVAL when the state numbers differ. */
int cpecan_viterbi_counts_add_to_hmm(const cpecan_viterbi_counts *counts, cpecan_hmm *acc);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_VITERBI_H_ */
