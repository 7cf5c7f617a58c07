/*
 * cpecan_sets.h -- sets of sequence fragments: every chosen pair of every set aligned in ONE anchor batch and ONE DP batch.
 *
 * Reference: impl/multipleAligner.c.  Its GPU work is addMultipleAlignedPairs (:653-666) -- getAlignedPairs with the ragged
 * flags taken from the fragments' end ids, reweightAlignedPairs2, getAlignmentScore (:604-619) -- called once per pair from
 * makeAllPairwiseAlignments (:668-681) and from the rounds of makeAlignment (:903-933).  This layer takes the fragments of
 * many sets (the ends of a Cactus bar phase), chooses the pairs as the reference does and returns per pair what the
 * reference appends to its lists: (score, seq1, pos1, seq2, pos2) records in the order convertAlignedPairsToMultipleAlignedPairs
 * (:621-634) leaves them, and the similarity score.  Everything behind the pairwise stage -- columns, poset merges, distance
 * matrix, the filter of the final pairs -- stays with the caller.
 *
 * Sequence names in the records are the fragments' GLOBAL indices, 0, 1, ... in the order they were added.
 */
#ifndef CPECAN_SETS_H_
#define CPECAN_SETS_H_

#include "cpecan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cpecan_sets cpecan_sets;
typedef struct cpecan_sets_result cpecan_sets_result;

/* The fields of PairwiseAlignmentParameters this layer reads beyond cpecan_params (inc/pairwiseAligner.h:28-41). */
typedef struct cpecan_sets_options {
    float gapGamma; /* widened to double where it reaches reweightAlignedPairs2, as the reference does (:662) */
    int32_t reserved;
    int64_t constraintDiagonalTrim;
    int64_t anchorMatrixBiggerThanThis;
    int64_t repeatMaskMatrixBiggerThanThis;
} cpecan_sets_options;
/* 0.5f, 14, 500 * 500, 500 * 500 (pairwiseAligner.c:1340-1345) */
int cpecan_sets_options_default(cpecan_sets_options *o);

/* params and options NULL = the defaults.  No device is touched before cpecan_sets_align. */
int cpecan_sets_create(cpecan_sets **out, const cpecan_model *model, const cpecan_params *params,
                       const cpecan_sets_options *options, int device);
void cpecan_sets_destroy(cpecan_sets *s);

/* Copies `length` bytes of seq (length 0 is legal) as a fragment of set `set` -- any caller id; the fragments of one set need
 * not be added together.  Returns the fragment's global index, or < 0. */
int64_t cpecan_sets_add_fragment(cpecan_sets *s, int64_t set, const char *seq, int64_t length, int64_t leftEndId,
                                 int64_t rightEndId);

/* The pairs the reference would align, as global indices, two values per pair: writes at most cap pairs and returns the
 * number there are (which may exceed cap), or < 0.  Sets come in ascending order of the global index of their first
 * fragment.  No device is touched.
 * ALL        makeAllPairwiseAlignments (:668-681): per set seq1 ascending, then seq2 > seq1 ascending.
 * REFERENCE  getReferencePairwiseAlignments (:722-770): per set the fragments sorted by (rightEndId, length, index); in every
 *            run [i, j) of equal rightEndId the element at (i + j) / 2 is the run's reference and pairs with every other
 *            member; the runs' references, in run order, are one more run treated the same way.  Every pair is (min, max)
 *            and a set's pairs are sorted by (seq1, seq2), as makeAlignment iterates its sorted set (:903).  A set of n
 *            fragments has n - 1 pairs. */
enum { CPECAN_SETS_ALL = 0, CPECAN_SETS_REFERENCE = 1 };
int64_t cpecan_sets_pairs(const cpecan_sets *s, int mode, int64_t *pairs, int64_t cap);

/* Aligns pair k = (pairs[2k], pairs[2k + 1]) = (a, b) with X = a and Y = b AS GIVEN (the later rounds of makeAlignment call
 * with seq > otherSeq too, :932); raggedLeft = leftEndId(a) != leftEndId(b), raggedRight likewise (:661).
 * CPECAN_EINVAL for a == b, fragments of different sets, an index out of range -- all checked before a device is looked
 * for; CPECAN_ENODEVICE without the device.
 * All pairs go through one cpecan_find_anchor_runs_many call with the options (a pair with lX * lY <=
 * anchorMatrixBiggerThanThis gets no anchors, pairwiseAligner.c:1164), then through one CPECAN_EMIT_MATCH batch added as
 * runs, with CPECAN_POST_REWEIGHT and the quintuple stage below.  May be called again on the same object with other pairs;
 * every call returns a result of its own (cpecan_sets_result_free). */
int cpecan_sets_align(cpecan_sets *s, const int64_t *pairs, int64_t nPairs, cpecan_sets_result **out);

/* *n records (score, seq1, pos1, seq2, pos2) as int32: the pairs concatenated in the order given; within a pair the
 * reweighted list 0 REVERSED, since convertAlignedPairsToMultipleAlignedPairs pops from the end (:625-632). */
int cpecan_sets_result_pairs(const cpecan_sets_result *r, const int32_t **quints, int64_t *n);
/* nPairs + 1 offsets into the records. */
int cpecan_sets_result_offsets(const cpecan_sets_result *r, const int64_t **offsets, int64_t *nPairs);
/* getAlignmentScore (:604-619) of every pair, the first value of the reference's seqPairSimilarityScores tuples. */
int cpecan_sets_result_similarity(const cpecan_sets_result *r, const int64_t **similarity, int64_t *nPairs);
/* Where the call's time went (milliseconds).  anchorMs: the anchor batch, wall; packMs: adding the problems, planning and
 * upload, wall; dpKernelMs: HIP-event time of the DP launches; stageMs: HIP-event time of the quintuple stage; downloadMs:
 * cpecan_batch_download, wall -- the wait for the DP, list gather, consumers, the stage and the copies; totalMs: the call. */
typedef struct cpecan_sets_timing {
    double anchorMs, packMs, dpKernelMs, stageMs, downloadMs, totalMs;
} cpecan_sets_timing;
int cpecan_sets_result_timing(const cpecan_sets_result *r, cpecan_sets_timing *t);
void cpecan_sets_result_free(cpecan_sets_result *r);

/* getAlignmentScore's arithmetic (:613-618), pure: j = min(lX, lY), 1 if that is 0; d = (double)scoreSum / (double)(j *
 * PAIR_ALIGNMENT_PROB_1) clamped to [0, 1]; the result is d * PAIR_ALIGNMENT_PROB_1 truncated.  < 0: a negative length. */
int64_t cpecan_similarity_score(int64_t scoreSum, int64_t lX, int64_t lY);

/* ---- the device stage behind it, as a switch of any batch that has lists (MATCH, INDEL) ----
 * names: two int32 per problem of the batch as it stands (copied; nProblems must be the batch's count), NULL = off, the
 * default: a batch without it allocates and launches exactly what it did before the stage existed.  With it, every later
 * download runs one more kernel behind the consumers (so behind REWEIGHT): per problem list 0 reversed as (score, names[0],
 * x, names[1], y) records at the problem's offset into one array of the whole batch, and the exact int64 sum of the
 * scores.  Those two arrays and the offsets are what the download then copies: the triples of such a batch stay on the
 * device and cpecan_batch_result refuses with CPECAN_ESTATE. */
int cpecan_batch_set_quintuples(cpecan_batch *b, const int32_t *names, int64_t nProblems);
/* After download: the records, nProblems + 1 offsets and nProblems sums; the batch owns them until its next download. */
int cpecan_batch_quintuples(const cpecan_batch *b, const int32_t **quints, const int64_t **offsets, const int64_t **sums);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_SETS_H_ */
