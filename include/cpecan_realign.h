/*
 * cpecan_realign.h -- the batch front end of cPecanRealign on top of cpecan_hip.h: cigar and fasta
 * text in, realigned cigars (or expectation counts) out, every alignment of a call in ONE GPU batch.
 *
 * Reference: cPecanRealign.c:354-624 (main loop), :49-96 (convertAlignedPairsToPairwiseAlignment), :98-230 (hasLongIndel,
 * splitPairwiseAlignment), :232-277 (rebase, getSubSequence, addToSequencesHash), :314-348 (scoreAnchorPairs).
 * Text formats: cigarRead / cigarWrite / fastaReadToFunction / stString_reverseComplementString live in sonLib
 * (benedictpaten/sonLib, a sibling checkout the reference's include.mk points at; not vendored in the reference, no pinned
 * version).  Their published formats are restated here:
 *   cigar line  "cigar: <contig2> <start2> <end2> <strand2> <contig1> <start1> <end1> <strand1> <score>( <op> <length>)*"
 *               op M = match, D = bases of contig1 (X) only, I = bases of contig2 (Y) only; strand '+' or '-'; on '-' the
 *               start is larger than the end; score printed with %f
 *   fasta       '>' header lines, sequence lines concatenated with white space removed; the key of a sequence is the first
 *               white-space delimited token of its header (cPecanRealign.c:245-275)
 */
#ifndef CPECAN_REALIGN_H_
#define CPECAN_REALIGN_H_

#include "cpecan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* struct PairwiseAlignment of sonLib, flattened.  contig1 is sequence X of the aligner, contig2 is Y. */
typedef struct cpecan_cigar {
    char *contig1, *contig2; /* malloc'd */
    int64_t start1, end1, start2, end2;
    int32_t strand1, strand2; /* 1 = '+' */
    double score;
    int64_t nOps;
    int64_t *ops; /* nOps pairs (CPECAN_OP_*, length), malloc'd */
} cpecan_cigar;

/* cigarRead on one line of text.  Returns CPECAN_EINVAL for a line that is not a cigar or whose operations do not add up
 * to its coordinates (checkPairwiseAlignment). */
int cpecan_cigar_parse(const char *line, cpecan_cigar *out);
/* cigarWrite(fileHandle, pA, 0) without the newline.  Returns the length of the text; writes at most cap bytes incl. NUL. */
int64_t cpecan_cigar_format(const cpecan_cigar *c, char *buf, int64_t cap);
void cpecan_cigar_clear(cpecan_cigar *c);
/* Frees an array returned by cpecan_realigner_realign or cpecan_cigar_split. */
void cpecan_cigars_free(cpecan_cigar *cigars, int64_t n);
/* convertAlignedPairsToPairwiseAlignment (cPecanRealign.c:49-96): xy holds n pairs (x, y) in increasing order; the result
 * spans [0, length1) x [0, length2) on the forward strands, unaligned ends included as leading / trailing indels. */
int cpecan_cigar_from_aligned_pairs(const char *contig1, const char *contig2, double score, int64_t length1, int64_t length2,
                                    const int64_t *xy, int64_t n, cpecan_cigar *out);
/* The same for a query on either strand: strand2 1 is the function above; strand2 0 takes the pairs (x, y') in the
 * coordinates of (X, rc(Y)) and gives start2 = length2, end2 = 0, strand2 = 0 with the operations in the order of the
 * pairs -- what the realigner reads back as rc(Y) (getSubSequence, cPecanRealign.c:252-258). */
int cpecan_cigar_from_aligned_pairs_stranded(const char *contig1, const char *contig2, double score, int64_t length1,
                                             int64_t length2, int strand2, const int64_t *xy, int64_t n, cpecan_cigar *out);
/* splitPairwiseAlignment (cPecanRealign.c:117-230): cuts c at every run of indels longer than maxIndelLength; the runs
 * that are cut and any indels at either end are dropped.  *out: malloc'd array of *nOut cigars (cpecan_cigars_free). */
int cpecan_cigar_split(const cpecan_cigar *c, int64_t maxIndelLength, cpecan_cigar **out, int64_t *nOut);

/* ---- the hand-off from one realignment to the anchors of the next (cPecanEm.py:205-215, --updateTheBand) ----
 * A batch stage behind CPECAN_POST_ORDERED (cpecan_hip.h), defined for one problem as a pure integer function of result
 * list 3, the ordered alignment: take its pairs (x, y) sorted ascending -- a chain, both coordinates increase strictly.  A
 * BLOCK is a maximal run of consecutive pairs in which both coordinates step by one: the match operations
 * convertAlignedPairsToPairwiseAlignment makes of the chain (cPecanRealign.c:50-92).  Drop `trim` columns at both ends of
 * every block (convertPairwiseForwardStrandAlignmentToAnchorPairs), keep a column iff its two letters are equal, case-
 * insensitive, and not N (matchFn, cPecanRealign.c:277-281); kept columns that follow each other inside a block form a run
 * (x, y, length, expansion).  These are the runs cpecan_anchor_runs_from_alignment gives for the operations of the cigar
 * cpecan_cigar_from_aligned_pairs builds from the same pairs, integer for integer, ready for cpecan_batch_add_many_runs.
 *
 * cpecan_batch_set_next_runs, before upload: downloads of the batch also run the stage, one wave per problem.  Only the runs
 * and their counts are copied out: the triples of such a batch stay on the device, cpecan_batch_result refuses it, the
 * scores remain.  CPECAN_EINVAL without CPECAN_POST_ORDERED, for a negative trim or expansion, or after upload; a later
 * cpecan_batch_set_post without CPECAN_POST_ORDERED switches the stage off with the list it reads.  expansion
 * CPECAN_NEXT_RUNS_OFF switches the stage off again: the batch then allocates and launches what it did before.
 * cpecan_batch_next_runs, after download: the nRuns quadruples of problem i (the batch's memory). */
#define CPECAN_NEXT_RUNS_OFF (-1)
int cpecan_batch_set_next_runs(cpecan_batch *b, int64_t trim, int64_t expansion);
int cpecan_batch_next_runs(const cpecan_batch *b, int64_t problem, const int64_t **runs, int64_t *nRuns);
/* The same definition on the host, no device needed: n triples (score, x, y) of a chain in any order.  runs receives at most
 * cap quadruples; returns the number of runs (which may exceed cap), or < 0: CPECAN_EINVAL for a pair outside the
 * sequences or pairs that are no chain. */
int64_t cpecan_next_runs_of_pairs(const int32_t *triples, int64_t n, const char *sX, int64_t lX, const char *sY, int64_t lY,
                                  int64_t trim, int64_t expansion, int64_t *runs, int64_t cap);

/* The options of cPecanRealign's command line with its defaults (cPecanRealign.c:354-370). */
typedef struct cpecan_realign_options {
    cpecan_params params;           /* diagonalExpansion 4 (-r), splitMatrixBiggerThanThis 10 (-o takes the square root) */
    int64_t constraintDiagonalTrim; /* -t, 0 */
    float gapGamma;                 /* -l, 0.5 */
    float matchGamma;               /* -L, 0.85 */
    int32_t rescoreOriginalAlignment;           /* -x */
    int32_t rescoreByIdentity;                  /* -i */
    int32_t rescoreByPosteriorProb;             /* -j */
    int32_t rescoreByIdentityIgnoringGaps;      /* -k */
    int32_t rescoreByPosteriorProbIgnoringGaps; /* -m */
    int64_t splitIndelsLongerThanThis;          /* -s, -1 = do not split */
} cpecan_realign_options;
void cpecan_realign_options_default(cpecan_realign_options *o);

typedef struct cpecan_realigner cpecan_realigner;
int cpecan_realigner_create(cpecan_realigner **out, const cpecan_model *model, const cpecan_realign_options *o, int device);
void cpecan_realigner_destroy(cpecan_realigner *r);
/* addToSequencesHash (cPecanRealign.c:245-275): a repeated key keeps the longer sequence. */
int cpecan_realigner_add_sequence(cpecan_realigner *r, const char *header, const char *seq, int64_t length);
/* fastaReadToFunction(file, addToSequencesHash).  Returns the number of records read, or < 0. */
int64_t cpecan_realigner_read_fasta(cpecan_realigner *r, const char *path);
/* Tab separated "x y probability" files as --outputPosteriorProbs (the final pairs) and --outputAllPosteriorProbs (every
 * pair of the banded alignment).  The reference reopens the file with "w" for every cigar, so what is left is the last
 * cigar's pairs; that is what is written here.  NULL = none. */
int cpecan_realigner_set_posterior_files(cpecan_realigner *r, const char *finalPairsPath, const char *allPairsPath);

/* Several GPUs from ONE process.  The reference fans a realignment out as one cPecanRealign process per shard
 * of the cigar file and sums the shards' expectation files (cPecanEm.py:168-188); with a device list the cigars of every
 * realign / expectations call are cut into nDevices contiguous shards of about equal band cells
 * (cpecan_realign_shard_bounds), shard k runs as its own batch on devices[k] from a host thread of its own, and the
 * results are joined in input order -- expectation counts summed on the host in shard order.  A device may be listed more
 * than once (two shards on one GPU); nDevices 0 or 1: one batch on the device given to cpecan_realigner_create. */
int cpecan_realigner_set_devices(cpecan_realigner *r, const int *devices, int nDevices);
/* bounds[0..nShards]: shard k is cigars [bounds[k], bounds[k+1]); a cigar costs (|end1 - start1| + |end2 - start2| + 1) *
 * (diagonalExpansion + 1), shard k ends at the first cigar where the running cost reaches k / nShards of the total. */
int cpecan_realign_shard_bounds(const cpecan_cigar *in, int64_t n, int64_t diagonalExpansion, int nShards, int64_t *bounds);

/* The realign loop (cPecanRealign.c:509-600) over n cigars as one batch.  *out: malloc'd array of *nOut cigars in input
 * order (more than n when splitIndelsLongerThanThis cuts some), to be released with cpecan_cigars_free. */
int cpecan_realigner_realign(cpecan_realigner *r, const cpecan_cigar *in, int64_t n, cpecan_cigar **out, int64_t *nOut);
/* The adaptive band.  The band of a realignment is diagonalExpansion / 2 diagonals either side of
 * whatever the input cigar says, so a misplaced indel in the input cannot be repaired, and the output looks like any other
 * cigar.  With maxRounds 1 .. 4 every realign call asks its batch for the band-edge statistic (cpecan_band_edge,
 * cpecan_hip.h); a cigar is FLAGGED iff its edgeScoreSum >= minEdgeScore.  Round 0 is the call as it is without this
 * option; round k = 1 .. maxRounds runs the cigars flagged in round k - 1 as a batch of their own with
 * params.diagonalExpansion * 2^k for the run expansions and the parameter, everything else -- exact-match filter, trim,
 * consumers -- as before.  A cigar's output (cigar, score, split pieces) is that of its last run: byte for byte what a
 * realigner without this option returns for it at that expansion.  The posterior files are those of the last cigar's last
 * run.  maxRounds 0 is off and the default: the calls and launches of a realigner that never heard of it.  minEdgeScore
 * >= 1 is required when on; it has no default (DESIGN.md section 9 says what the quality record suggests).
 * CPECAN_EINVAL: maxRounds outside 0 .. 4, minEdgeScore < 1 when on, or a realigner with rescoreOriginalAlignment, which
 * returns its input.  Expectations calls are unaffected.  With several devices every shard adapts on its own; the result is
 * per cigar, so it is the same. */
int cpecan_realigner_set_adaptive_band(cpecan_realigner *r, int maxRounds, int64_t minEdgeScore);
/* The round each of the n input cigars of the last realign call ended on (all 0 without the option).  CPECAN_ESTATE before
 * the first realign call, CPECAN_EINVAL when n is not that call's count. */
int cpecan_realigner_adaptive_rounds(const cpecan_realigner *r, int32_t *rounds, int64_t n);
/* --outputExpectations (cPecanRealign.c:530-534): adds the expectation counts of the n alignments to *acc, which the
 * caller made with cpecan_hmm_init(acc, type, 0.000000000001) (:497) and writes with cpecan_hmm_write (:612). */
int cpecan_realigner_expectations(cpecan_realigner *r, const cpecan_cigar *in, int64_t n, cpecan_hmm *acc);

/* The E-step of expectation maximisation on a RESIDENT set of alignments (include/cpecan_em.h).  _create prepares the n
 * cigars as cpecan_realigner_expectations does (exact-match anchors, diagonalExpansion, splitMatrixBiggerThanThis,
 * constraintDiagonalTrim of the realigner's options), cuts them into the realigner's device shards
 * (cpecan_realign_shard_bounds) and plans and uploads one EXPECT batch per shard, once.  A set that does not fit in a
 * device's memory fails with CPECAN_ENOMEM and a message that names the limit; nothing is re-planned.  _run then adds the
 * expectation counts of all n alignments under model m to *acc -- the result of cpecan_realigner_expectations with a
 * realigner of model m -- by swapping the model of the resident batches (cpecan_batch_set_model) and running only the
 * kernels.  m must have the state count of the realigner's model. */
typedef struct cpecan_expect_set cpecan_expect_set;
int cpecan_expect_set_create(cpecan_expect_set **out, cpecan_realigner *r, const cpecan_cigar *in, int64_t n);
int cpecan_expect_set_run(cpecan_expect_set *s, const cpecan_model *m, cpecan_hmm *acc);
/* Model slots (cpecan_batch_reserve_models, cpecan_hip.h).  A set takes its options from the realigner it is created
 * from, so the reservation is made there, before cpecan_expect_set_create: the batches of every set created afterwards
 * reserve nSlots models (1 .. CPECAN_MAX_MODEL_SLOTS; 0: plain batches again).  cpecan_expect_set_run_models is then n E-steps in one launch per
 * shard, 1 <= n <= nSlots (a set that reserved nothing takes n = 1): every shard queues its launch before the first
 * download waits, and accs[j] receives the counts of models[j], added in shard order as cpecan_expect_set_run adds them. */
int cpecan_expect_set_reserve_models(cpecan_realigner *r, int nSlots);
int cpecan_expect_set_run_models(cpecan_expect_set *s, const cpecan_model *models, int n, cpecan_hmm *accs);
int cpecan_expect_set_shards(const cpecan_expect_set *s);
/* Statistics of shard k's batch (launch form, waves, cells, kernel time of the last run); zeros for an empty shard. */
int cpecan_expect_set_stats(const cpecan_expect_set *s, int shard, cpecan_stats *st);
void cpecan_expect_set_destroy(cpecan_expect_set *s);

/* ---- realigning the band: the three steps of an --updateTheBand iteration (cPecanEm.py:205-215) ----
 * cpecan_realigner_set_model: the model of every later call (cpecan_realigner_create's copy is replaced).
 * cpecan_realigner_reanchor: the batch of cpecan_realigner_realign with the next-runs stage on
 * (cpecan_batch_set_next_runs with the realigner's constraintDiagonalTrim and diagonalExpansion).  *nRuns: malloc'd, n counts;
 * *runs: malloc'd, the quadruples of cigar 0, then cigar 1, ... (both cpecan_free) -- per input cigar the exact-match anchor
 * runs of the cigar cpecan_realigner_realign would return for it, in the coordinates of the cigar's sub-sequences, that is
 * what cpecan_anchor_runs_from_alignment gives for that cigar's operations from (0, 0).  Refuses rescoreOriginalAlignment
 * and splitIndelsLongerThanThis != -1 with CPECAN_EINVAL before a device is looked for; the adaptive band does not apply.
 * With cpecan_realigner_set_devices the shards are joined in input order.
 * cpecan_realigner_reanchor_runs: the same with the anchors of cigar i taken from its nRunsIn[i] quadruples of runsIn (the
 * layout _reanchor returns) instead of from the cigar's operations: feeding a call's result to the next one is realigning
 * the realigned cigars, as cPecanEm.py:212-215 does when it moves the realigned file over the alignments file.
 * cpecan_expect_set_create_runs: cpecan_expect_set_create with the anchors of cigar i taken from its nRuns[i] quadruples of
 * `runs` (laid out as _reanchor returns them) instead of from the cigar's operations, which are not read. */
int cpecan_realigner_set_model(cpecan_realigner *r, const cpecan_model *model);
int cpecan_realigner_reanchor(cpecan_realigner *r, const cpecan_cigar *in, int64_t n, int64_t **runs, int64_t **nRuns);
int cpecan_realigner_reanchor_runs(cpecan_realigner *r, const cpecan_cigar *in, int64_t n, const int64_t *runsIn,
                                   const int64_t *nRunsIn, int64_t **runs, int64_t **nRuns);
int cpecan_expect_set_create_runs(cpecan_expect_set **out, cpecan_realigner *r, const cpecan_cigar *in, int64_t n,
                                  const int64_t *runs, const int64_t *nRuns);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_REALIGN_H_ */
