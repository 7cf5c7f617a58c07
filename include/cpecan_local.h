/*
 * cpecan_local.h -- local chains: the K best mutually disjoint colinear chains of a pair, over one or both orientations
 * (DESIGN.md section 7, steps 7 and 7b), and the cigars that hand them to the realigner of cpecan_realign.h.
 *
 * The reference never finds these itself: lastz hands cPecanRealign local alignments on both strands, many per pair, and
 * cPecanRealign realigns each (cPecanRealign.c:509-600).  cpecan_find_anchor_runs_many (cpecan_hip.h) keeps ONE chain per
 * pair in ONE orientation, for a global alignment.  The entry point below keeps up to maxChains, so that an inverted or
 * transposed segment is a chain of its own instead of a gap; each chain becomes a cigar, and cpecan_realigner_realign
 * bands on it.
 *
 * Definition, for one problem (X, Y) -- a pure integer function like steps 1-6:
 *   pools      per orientation searched (PLUS: (X, Y); MINUS: (X, rc(Y)); BOTH: both) steps 1-3 of the finder on the whole
 *              pair whatever its size, softMask on: the HSPs (x, y, len, score) sorted by (x, y, len), duplicates dropped,
 *              capped at maxHsps.  Every HSP starts live.
 *   intervals  an HSP occupies [x, x + len) of X; a plus HSP [y, y + len) of forward Y; a minus HSP at y' of rc(Y) occupies
 *              [lY - y' - len, lY - y') of forward Y.
 *   round      r = 1 .. maxChains: step 4 over the live HSPs of each orientation, tie rules unchanged; the chain with the
 *              larger score is the round's, a tie goes to plus.  No live HSP, or a score under minChainScore: stop.
 *              Otherwise record the chain, then kill every live HSP of either orientation whose X interval meets the X
 *              interval of a chained HSP or whose forward-Y interval meets the forward-Y interval of one.
 * So chain scores never increase, and all chained HSPs of a problem are pairwise disjoint on X and on forward Y.
 * Step 6 (the recursion into gaps) is not run.  cpecan_anchor_options.gappedExtension is refused by
 * cpecan_find_local_chains_many and served by cpecan_find_local_chains_many_gapped (step 7b, below).
 */
#ifndef CPECAN_LOCAL_H_
#define CPECAN_LOCAL_H_

#include "cpecan_realign.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cpecan_local_options {
    int32_t maxChains;     /* K: 1 .. 16 */
    int32_t minChainScore; /* S: 0 stands for cpecan_anchor_params.hspThreshold; otherwise at least that */
    int32_t reserved[6];   /* must be 0 */
} cpecan_local_options;
/* maxChains 1, minChainScore 0 */
int cpecan_local_options_default(cpecan_local_options *o);

/* One chain.  The rectangle [x0, x1) x [y0, y1) goes from the start of its first HSP to the end of its last (of its first and
 * last merged block where chains are extended); it and the runs
 * are in the coordinates of the chain's orientation: (X, Y) for plus, (X, rc(Y)) for minus.  The runs are step 5 on the
 * chain's HSPs with the call's trim: quadruples runOff .. runOff + nRuns - 1 of the problem's run array.  A chain whose runs
 * all trim away is still reported, with nRuns 0. */
typedef struct cpecan_local_chain {
    int32_t strand; /* CPECAN_STRAND_PLUS or CPECAN_STRAND_MINUS */
    int32_t score;  /* sum of the chained HSPs' scores */
    int64_t nHsps;
    int64_t x0, x1, y0, y1;
    int64_t runOff, nRuns;
} cpecan_local_chain;

/* Per problem: hits and HSPs (after duplicates, before the cap) of each orientation searched, 0 for one that was not;
 * capped: step 3 cut a pool (bit 0: plus, bit 1: minus); rounds: the rounds that found a chain, which is nChains, or one
 * more when a chain under minChainScore ended them; kernelMs: HIP-event time of the call's kernels, the same in every record. */
typedef struct cpecan_local_stats {
    int64_t hitsPlus, hitsMinus, hspsPlus, hspsMinus;
    int32_t capped, rounds;
    double kernelMs;
} cpecan_local_stats;

/* The local chains of n problems in one batch on `device`.  chains[i]: a malloc'd array of nChains[i] records in round order;
 * runs[i]: a malloc'd array of nRuns[i] quadruples (x, y, length, expansion); both are released with cpecan_free.  stats: n
 * records, or NULL.  params, anchorOptions, localOptions: NULL = the defaults.  strandMode: CPECAN_STRAND_*.
 * CPECAN_EINVAL, before a device is looked for: what cpecan_find_anchor_runs_many_with_options refuses; maxChains outside
 * 1 .. 16; minChainScore negative, or positive and under hspThreshold; anchorOptions->gappedExtension = 1 (the entry point
 * below takes it); a nonzero reserved word.  CPECAN_ENODEVICE after those. */
int cpecan_find_local_chains_many(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                  const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                                  const cpecan_local_options *localOptions, int device, int strandMode,
                                  cpecan_local_chain **chains, int64_t *nChains, int64_t **runs, int64_t *nRuns,
                                  cpecan_local_stats *stats);

/* The same, and with anchorOptions->gappedExtension = 1 every chain is extended into the gaps between its HSPs and outwards
 * from its ends.  After the last round the chains are extended in round order.  When chain r
 * is extended the occupied set is every chained HSP of every other chain of the problem, later rounds included, and every
 * extension block that chains 1 .. r - 1 kept, each with its X interval and its forward-Y interval (above), mapped into the
 * orientation of chain r.  The gaps are those of step 5b (cpecan_hip.h) on the chain's HSPs in its own orientation, the end
 * gaps reaching to (0, 0) and (lX, lY).  A right extension runs from the gap's lower corner up to the smallest occupied
 * start inside the gap on either axis, a left extension from the upper corner down to the largest occupied end; the walk
 * is step 5b's -- band, gap costs, tie rules, yDrop, gappedMaxDiagonals on the fenced sides -- and so is the test on two
 * extensions of one gap, on the whole gap.  Blocks are assembled, merged and trimmed as in 5b.
 * So all untrimmed blocks of a problem are pairwise disjoint on X and on forward Y, a chain's blocks ascend on both axes of
 * its orientation, and every chained HSP lies inside a block of its chain.  strand, score and nHsps of a record and the
 * statistics are those of cpecan_find_local_chains_many; the rectangle goes from the start of the chain's first merged block
 * to the end of its last, and nRuns may exceed nHsps.  One chain on the plus strand has the runs of
 * cpecan_find_anchor_runs_once(softMask = 1) with the same options.  With gappedExtension = 0 the call is
 * cpecan_find_local_chains_many.  yDrop, gappedMaxDiagonals: meaning, defaults and CPECAN_EINVAL cases as in
 * cpecan_find_anchor_runs_many_with_options; every other refusal as above, before a device is looked for. */
int cpecan_find_local_chains_many_gapped(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                         const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                                         const cpecan_local_options *localOptions, int device, int strandMode,
                                         cpecan_local_chain **chains, int64_t *nChains, int64_t **runs, int64_t *nRuns,
                                         cpecan_local_stats *stats);

/* The cigar of a chain; touches no device.  runs: the problem's run array, of which the chain's runOff and nRuns name a part
 * (a caller may pass a copy of the chain that names fewer).  The cigar spans from the start of the first of those runs to
 * the end of the last: start1 < end1, strand1 = 1; plus: start2 < end2, strand2 = 1; minus, with the runs at y0' .. y1' of
 * rc(Y): start2 = lY - y0', end2 = lY - y1', strand2 = 0 -- the convention of cpecan_cigar_from_aligned_pairs_stranded, so
 * the realigner reads the range back as rc(Y).  One M per run; between two runs a step (dx, dy) is D dx, then I dy, the
 * order of cpecan_cigar_from_aligned_pairs.  score: the chain score.  CPECAN_EINVAL: no runs, runs that are no chain, or
 * a minus chain that does not fit lY. */
int cpecan_cigar_from_local_chain(const char *contig1, const char *contig2, int64_t lY, const cpecan_local_chain *chain,
                                  const int64_t *runs, cpecan_cigar *out);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_LOCAL_H_ */
