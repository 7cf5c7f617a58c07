/*
 * pairwiseAlignment.h -- STAND-IN (test infrastructure; see sonLib.h beside it).  Only the fields that the reference's
 * impl/pairwiseAligner.c touches (convertPairwiseForwardStrandAlignmentToAnchorPairs and the cigar loop of
 * getBlastPairs) are declared.  cigarRead and destructPairwiseAlignment are stubs that name themselves and abort.
 */
#ifndef REF_STANDIN_PAIRWISEALIGNMENT_H_
#define REF_STANDIN_PAIRWISEALIGNMENT_H_

#include <stdint.h>
#include <stdio.h>

enum { PAIRWISE_MATCH = 0, PAIRWISE_INDEL_X = 1, PAIRWISE_INDEL_Y = 2 };

struct List {
    int64_t length;
    void **list;
};

struct AlignmentOperation {
    int64_t opType;
    int64_t length;
};

struct PairwiseAlignment {
    char *contig1;
    int64_t start1, end1, strand1;
    char *contig2;
    int64_t start2, end2, strand2;
    struct List *operationList;
};

struct PairwiseAlignment *cigarRead(FILE *file);
void destructPairwiseAlignment(struct PairwiseAlignment *pA);

#endif
