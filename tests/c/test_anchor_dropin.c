/*
 * The reference-named entry points that find their own anchors (include/cpecan_dropin.h), as a C caller uses them:
 * getAlignedPairs on two 2 kb strings returns instead of aborting, and getBlastPairsForPairwiseAlignmentParameters
 * returns a strictly increasing list of (x, y, diagonalExpansion).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_dropin.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                    \
        }                                                                  \
    } while (0)

/* two related 2 kb strings: Y is X with a substitution every 17th base and a base dropped every 301st */
static void make_pair(char *sX, char *sY, int n) {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    int m = 0;
    for (int i = 0; i < n; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        sX[i] = "ACGT"[(s >> 33) & 3];
        if (i % 301 == 300) continue;
        sY[m++] = i % 17 == 16 ? "ACGT"[((s >> 33) + 1) & 3] : sX[i];
    }
    sX[n] = 0;
    sY[m] = 0;
}

int main(void) {
    enum { N = 2000 };
    char *sX = malloc(N + 1), *sY = malloc(N + 1);
    make_pair(sX, sY, N);
    const int64_t lX = (int64_t)strlen(sX), lY = (int64_t)strlen(sY);
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    StateMachine *sM = stateMachine5_construct(fiveState);
    CHECK(lX * lY > p->anchorMatrixBiggerThanThis);

    stList *anchors = getBlastPairsForPairwiseAlignmentParameters(sX, sY, lX, lY, p);
    CHECK(stList_length(anchors) > 500);
    int64_t pX = -1, pY = -1;
    for (int64_t i = 0; i < stList_length(anchors); i++) {
        stIntTuple *t = stList_get(anchors, i);
        CHECK(stIntTuple_length(t) == 3);
        CHECK(stIntTuple_get(t, 0) > pX && stIntTuple_get(t, 1) > pY);
        CHECK(stIntTuple_get(t, 0) < lX && stIntTuple_get(t, 1) < lY);
        CHECK(stIntTuple_get(t, 2) == p->diagonalExpansion);
        pX = stIntTuple_get(t, 0);
        pY = stIntTuple_get(t, 1);
    }
    stList *filtered = filterToRemoveOverlap(anchors);
    CHECK(stList_length(filtered) == stList_length(anchors));
    stList *top = getBlastPairs(sX, sY, lX, lY, p->constraintDiagonalTrim, p->diagonalExpansion, 1);
    CHECK(stList_length(top) > 0 && stList_length(top) <= stList_length(anchors));

    stList *pairs = getAlignedPairs(sM, sX, sY, p, 1, 1);
    stList *same = getAlignedPairsUsingAnchors(sM, sX, sY, anchors, p, 1, 1);
    CHECK(stList_length(pairs) > 1500);
    CHECK(stList_length(pairs) == stList_length(same));
    for (int64_t i = 0; i < stList_length(pairs) && i < stList_length(same); i++)
        for (int f = 0; f < 3; f++) CHECK(stIntTuple_get(stList_get(pairs, i), f) == stIntTuple_get(stList_get(same, i), f));

    /* up to the size limit: no anchors, as before */
    sX[100] = 0;
    sY[100] = 0;
    stList *none = getBlastPairsForPairwiseAlignmentParameters(sX, sY, 100, 100, p);
    CHECK(stList_length(none) == 0);

    stList_destruct(none);
    stList_destruct(pairs);
    stList_destruct(same);
    stList_destruct(top);
    stList_destruct(filtered);
    stList_destruct(anchors);
    stateMachine_destruct(sM);
    pairwiseAlignmentBandingParameters_destruct(p);
    free(sX);
    free(sY);
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
