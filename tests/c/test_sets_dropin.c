/* C-level test of the multiple aligner's pairwise stage in the reference-named layer (include/cpecan_dropin.h):
 * SeqFrag, seqFrag_construct / _destruct and makeAllPairwiseAlignments (impl/multipleAligner.c:668-681), as a C caller of
 * inc/multipleAligner.h uses them.
 * usage: test_sets_dropin cpu | gpu */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_dropin.h"
#include "cpecan_sets.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static void test_host_side(void) {
    char text[] = "ACGTN";
    SeqFrag *f = seqFrag_construct(text, 3, -4);
    text[0] = 'T'; /* the fragment holds a copy */
    CHECK(strcmp(f->seq, "ACGTN") == 0 && f->length == 5 && f->leftEndId == 3 && f->rightEndId == -4);
    stIntTuple *t = stIntTuple_construct5(9, 8, 7, 6, 5);
    CHECK(stIntTuple_length(t) == 5 && stIntTuple_get(t, 0) == 9 && stIntTuple_get(t, 3) == 6 && stIntTuple_get(t, 4) == 5);
    stIntTuple_destruct(t);
    /* fewer than two fragments: no pair, and nothing is asked of a GPU */
    StateMachine *sM = stateMachine5_construct(fiveState);
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    stList *frags = stList_construct3(0, (void (*)(void *))seqFrag_destruct);
    for (int n = 0; n < 2; n++) {
        stList *scores = NULL;
        stList *pairs = makeAllPairwiseAlignments(sM, frags, p, &scores);
        CHECK(pairs && scores && stList_length(pairs) == 0 && stList_length(scores) == 0);
        stList_destruct(pairs);
        stList_destruct(scores);
        if (n == 0) stList_append(frags, f);
    }
    stList_destruct(frags);
    CHECK(cpecan_similarity_score(25000000, 4, 6) == 6250000 && cpecan_similarity_score(-1, 4, 6) == 0);
    CHECK(cpecan_similarity_score(50000000, 4, 6) == 10000000 && cpecan_similarity_score(5000000, 0, 6) == 5000000);
    pairwiseAlignmentBandingParameters_destruct(p);
    stateMachine_destruct(sM);
}

static void test_all_pairs_gpu(void) {
    const char *seqs[3] = {"AGCG", "AGTTCG", "AGTCG"};
    const int64_t left[3] = {0, 0, 1}, right[3] = {5, 6, 5};
    StateMachine *sM = stateMachine5_construct(fiveState);
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    stList *frags = stList_construct3(0, (void (*)(void *))seqFrag_destruct);
    for (int i = 0; i < 3; i++) stList_append(frags, seqFrag_construct(seqs[i], left[i], right[i]));
    stList *scores = NULL;
    stList *pairs = makeAllPairwiseAlignments(sM, frags, p, &scores);
    /* the order of makeAllPairwiseAlignments: (0, 1), (0, 2), (1, 2) */
    const int64_t want[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    CHECK(stList_length(scores) == 3);
    int64_t at = 0;
    for (int k = 0; k < 3 && stList_length(scores) == 3; k++) {
        const int64_t a = want[k][0], b = want[k][1];
        stIntTuple *s = stList_get(scores, k);
        CHECK(stIntTuple_length(s) == 3 && stIntTuple_get(s, 1) == a && stIntTuple_get(s, 2) == b);
        /* the reference's three calls for the same pair (:660-662) */
        stList *l = getAlignedPairs(sM, seqs[a], seqs[b], p, left[a] != left[b], right[a] != right[b]);
        l = reweightAlignedPairs2(l, (int64_t)strlen(seqs[a]), (int64_t)strlen(seqs[b]), p->gapGamma);
        const int64_t n = stList_length(l);
        CHECK(n > 0 && at + n <= stList_length(pairs));
        int64_t sum = 0;
        for (int64_t i = 0; i < n && at + i < stList_length(pairs); i++) {
            stIntTuple *q = stList_get(pairs, at + i), *t = stList_get(l, n - 1 - i); /* popped from the end (:625-632) */
            CHECK(stIntTuple_length(q) == 5 && stIntTuple_get(q, 1) == a && stIntTuple_get(q, 3) == b);
            CHECK(stIntTuple_get(q, 2) == stIntTuple_get(t, 1) && stIntTuple_get(q, 4) == stIntTuple_get(t, 2));
            CHECK(stIntTuple_get(q, 2) >= 0 && stIntTuple_get(q, 2) < (int64_t)strlen(seqs[a]));
            CHECK(stIntTuple_get(q, 4) >= 0 && stIntTuple_get(q, 4) < (int64_t)strlen(seqs[b]));
            sum += stIntTuple_get(q, 0);
        }
        at += n;
        const int64_t lA = (int64_t)strlen(seqs[a]), lB = (int64_t)strlen(seqs[b]);
        CHECK(stIntTuple_get(s, 0) == cpecan_similarity_score(sum, lA, lB)); /* getAlignmentScore (:604-619) of the pair's tuples */
        CHECK(stIntTuple_get(s, 0) > 0 && stIntTuple_get(s, 0) <= PAIR_ALIGNMENT_PROB_1);
        stList_destruct(l);
    }
    CHECK(at == stList_length(pairs)); /* the list is the three lists, nothing else */
    stList_destruct(pairs); /* both lists carry stIntTuple_destruct */
    stList_destruct(scores);
    stList_destruct(frags);
    pairwiseAlignmentBandingParameters_destruct(p);
    stateMachine_destruct(sM);
}

int main(int argc, char **argv) {
    const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
    test_host_side();
    if (gpu) test_all_pairs_gpu();
    printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
    return failures != 0;
}
