/*
 * cpecan_next_runs_of_pairs (cpecan_amd/csrc/cpecan_host.c) without the library, HIP or a GPU, built with
 * -fsanitize=address,undefined by tests/test_next_runs_c.py: device_standins.h stands in for the device layer cpecan_host.c
 * calls, none of which the function under test reaches.  main runs the function over an empty list, a list shorter than the
 * trim, a trim larger than any int32 and a cap smaller than the count, and over two thousand random chains against the
 * operations of the chain's cigar walked by cpecan_anchor_runs_from_alignment.  Sequences, triples and runs live in blocks
 * of exactly their size, so a read or write past them is caught.  Everything is freed: the leak check stays on.
 */
#include "device_standins.h"

#include "cpecan_realign.h"

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static int64_t rnd(int64_t n) { /* 0 .. n - 1 */
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((rngState >> 33) % (uint64_t)n);
}

static void random_chain(void) {
    const char *letters = "ACGTacgtNn";
    const int64_t nBlocks = rnd(6);
    int64_t cap = 0, n = 0, x = 0, y = 0, nOps = 0;
    int64_t lens[8], gx[8], gy[8];
    for (int64_t b = 0; b < nBlocks; b++) {
        gx[b] = rnd(4);
        gy[b] = rnd(3);
        if (b > 0 && gx[b] == 0 && gy[b] == 0) gx[b] = 1; /* a new block does not continue the one before */
        lens[b] = 1 + rnd(90);
        cap += lens[b];
    }
    int32_t *t = malloc(sizeof(int32_t) * 3 * (size_t)(cap ? cap : 1));
    int64_t *ops = malloc(sizeof(int64_t) * 2 * (size_t)(3 * nBlocks + 1));
    for (int64_t b = 0; b < nBlocks; b++) {
        if (gx[b]) {
            ops[2 * nOps] = CPECAN_OP_INDEL_X;
            ops[2 * nOps++ + 1] = gx[b];
        }
        if (gy[b]) {
            ops[2 * nOps] = CPECAN_OP_INDEL_Y;
            ops[2 * nOps++ + 1] = gy[b];
        }
        x += gx[b];
        y += gy[b];
        ops[2 * nOps] = CPECAN_OP_MATCH;
        ops[2 * nOps++ + 1] = lens[b];
        for (int64_t k = 0; k < lens[b]; k++, n++) {
            t[3 * n] = (int32_t)rnd(10000000);
            t[3 * n + 1] = (int32_t)(x + k);
            t[3 * n + 2] = (int32_t)(y + k);
        }
        x += lens[b];
        y += lens[b];
    }
    const int64_t lX = x + rnd(3), lY = y + rnd(3);
    char *sX = malloc((size_t)(lX ? lX : 1)), *sY = malloc((size_t)(lY ? lY : 1));
    for (int64_t i = 0; i < lX; i++) sX[i] = letters[rnd(10)];
    for (int64_t i = 0; i < lY; i++) sY[i] = letters[rnd(10)];
    for (int64_t i = 0; i < n; i++)
        if (rnd(10) < 8) sY[t[3 * i + 2]] = sX[t[3 * i + 1]];
    for (int64_t i = n - 1; i > 0; i--) { /* any order: the device's list is not sorted either */
        const int64_t j = rnd(i + 1);
        for (int f = 0; f < 3; f++) {
            const int32_t tmp = t[3 * i + f];
            t[3 * i + f] = t[3 * j + f];
            t[3 * j + f] = tmp;
        }
    }
    const int64_t trim = rnd(5), expansion = 2 * rnd(6);
    const int64_t want = cpecan_anchor_runs_from_alignment(ops, nOps, 0, 0, trim, expansion, sX, lX, sY, lY, NULL, 0);
    const int64_t got = cpecan_next_runs_of_pairs(t, n, sX, lX, sY, lY, trim, expansion, NULL, 0);
    CHECK(want >= 0 && got == want);
    if (want >= 0 && got == want) {
        int64_t *a = malloc(sizeof(int64_t) * 4 * (size_t)(want ? want : 1)), *b = malloc(sizeof(int64_t) * 4 * (size_t)(want ? want : 1));
        CHECK(cpecan_anchor_runs_from_alignment(ops, nOps, 0, 0, trim, expansion, sX, lX, sY, lY, a, want) == want);
        CHECK(cpecan_next_runs_of_pairs(t, n, sX, lX, sY, lY, trim, expansion, b, want) == want);
        CHECK(memcmp(a, b, sizeof(int64_t) * 4 * (size_t)want) == 0);
        if (want > 1) { /* a cap below the count: nothing behind it is written (the block holds exactly `half` runs) */
            const int64_t half = want / 2;
            int64_t *c = malloc(sizeof(int64_t) * 4 * (size_t)half);
            CHECK(cpecan_next_runs_of_pairs(t, n, sX, lX, sY, lY, trim, expansion, c, half) == want);
            CHECK(memcmp(a, c, sizeof(int64_t) * 4 * (size_t)half) == 0);
            free(c);
        }
        free(a);
        free(b);
    }
    free(t);
    free(ops);
    free(sX);
    free(sY);
}

int main(void) {
    int64_t runs[8];
    CHECK(cpecan_next_runs_of_pairs(NULL, 0, "ACGT", 4, "ACGT", 4, 0, 4, runs, 2) == 0);
    CHECK(cpecan_next_runs_of_pairs(NULL, 0, NULL, 0, NULL, 0, 0, 4, NULL, 0) == 0);
    const int32_t t[9] = {5, 0, 0, 5, 1, 1, 5, 2, 2};
    CHECK(cpecan_next_runs_of_pairs(t, 3, "ACG", 3, "ACG", 3, 2, 4, runs, 2) == 0); /* shorter than 2 * trim + 1 */
    CHECK(cpecan_next_runs_of_pairs(t, 3, "ACG", 3, "ACG", 3, (int64_t)1 << 40, 4, runs, 2) == 0);
    CHECK(cpecan_next_runs_of_pairs(t, 3, "ACG", 3, "ACG", 3, 1, 4, runs, 2) == 1 && runs[0] == 1 && runs[1] == 1 && runs[2] == 1 && runs[3] == 4);
    CHECK(cpecan_next_runs_of_pairs(t, 3, "ACG", 3, "AC", 2, 0, 4, runs, 2) == CPECAN_EINVAL); /* a pair outside Y */
    const int32_t crossed[6] = {5, 0, 1, 5, 1, 0};
    CHECK(cpecan_next_runs_of_pairs(crossed, 2, "AC", 2, "AC", 2, 0, 4, runs, 2) == CPECAN_EINVAL); /* no chain */
    for (int i = 0; i < 2000; i++) random_chain();
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
