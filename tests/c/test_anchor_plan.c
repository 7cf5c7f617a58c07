/*
 * The host side of the anchor finder (cpecan_amd/csrc/cpecan_anchor.c) without the library, HIP or a GPU, built with
 * -fsanitize=address,undefined by tests/test_anchor_plan_c.py: this file stands in for the few cpk_* functions that
 * cpecan_anchor.c calls.  Its cpk_anchor_pass hands back seeded synthetic runs, strictly increasing inside each problem,
 * at hspOff values that are not in list order.  main calls the public entry points on a few hundred problems in all three
 * strand modes with limits so small that the gap list outgrows its first 64 slots several times, and checks that every
 * returned list is strictly increasing and inside its problem and that the statistics add up.  Everything is freed: the
 * leak check of the sanitizer stays on.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static int64_t rnd(int64_t n) { /* 0 .. n - 1 */
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((rngState >> 33) % (uint64_t)n);
}

/* ---- the stand-ins ---- */
struct CpkAnchorCtx {
    int64_t nSym, nForward;
};
static char lastError[512];
static int64_t passes = 0, passProblems[2], contexts = 0;
static double passMs = 0.0;

void cpk_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(lastError, sizeof lastError, fmt, ap);
    va_end(ap);
}
int cpk_device_count(void) { return 1; }
int cpk_current_device(void) { return 0; }

int cpk_anchor_open(CpkAnchorCtx **out, int device, const uint8_t *bytes, int64_t nBytes, int64_t nExtra) {
    CHECK(device == 0 && bytes && nBytes > 0 && nExtra >= 0 && nExtra % 2 == 0);
    int64_t sum = 0;
    for (int64_t i = 0; i < nBytes; i++) sum += bytes[i]; /* every byte of the layout's buffer is readable and set */
    CHECK(sum > 0);
    *out = malloc(sizeof **out);
    (*out)->nForward = nBytes;
    (*out)->nSym = nExtra > 0 ? ((nBytes + 1) & ~(int64_t)1) + nExtra : nBytes;
    contexts++;
    return CPECAN_OK;
}

void cpk_anchor_close(CpkAnchorCtx *c) {
    if (c) contexts--;
    free(c);
}

/* Fixed counts (3 hits, 2 HSPs) so that the sums of the splice can be told from outside; a random chain score. */
int cpk_anchor_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int32_t **runs, double *ms) {
    *runs = NULL;
    passProblems[passes++ & 1] = n;
    if (n <= 0) return CPECAN_OK;
    CHECK(pass->trim == 2 && pass->seedTransitions == 0 && pass->variantThreshold == pass->prm.hspThreshold && strlen(pass->seed) == 19);
    int64_t cap = 0, at = 0;
    for (int64_t i = 0; i < n; i++) cap += 1 + (probs[i].lX < probs[i].lY ? probs[i].lX : probs[i].lY);
    int32_t *r = malloc(sizeof *r * 3 * (size_t)cap);
    for (int64_t i = n - 1; i >= 0; i--) { /* the last problem's block first */
        CpkAnchorProblem *p = &probs[i];
        const int twin = (p->flags & CPK_ANCHOR_SHARE_X) != 0;
        CHECK(p->lX > 0 && p->lY > 0 && p->xOff >= 0 && p->yOff >= 0 && p->xOff + p->lX <= c->nSym && p->yOff + p->lY <= c->nSym);
        CHECK(!twin || (i > 0 && probs[i - 1].xOff == p->xOff && probs[i - 1].lX == p->lX && !(probs[i - 1].flags & CPK_ANCHOR_SHARE_X)));
        CHECK(!(p->flags & CPK_ANCHOR_RC_Y) || (p->yOff % 2 == 0 && p->yOff >= ((c->nForward + 1) & ~(int64_t)1) && p->yFwd >= 0 &&
                                                p->yFwd + p->lY <= c->nForward));
        for (int k = 0; k < 3; k++) r[3 * at + k] = -12345; /* between the blocks: nobody's */
        p->hspOff = ++at;
        p->nRuns = 0;
        for (int64_t x = rnd(12), y = rnd(12);;) {
            const int64_t len = 1 + rnd(9);
            if (x + len > p->lX || y + len > p->lY) break;
            r[3 * at] = (int32_t)x;
            r[3 * at + 1] = (int32_t)y;
            r[3 * at + 2] = (int32_t)len;
            at++;
            p->nRuns++;
            x += len + rnd(30);
            y += len + rnd(30);
        }
        p->hits = 3;
        p->hsps = 2;
        p->chained = p->nRuns;
        p->capped = 0;
        p->score = (int32_t)rnd(4); /* ties are frequent */
    }
    CHECK(at <= cap);
    *runs = r;
    *ms += 0.5;
    passMs += 0.5;
    return CPECAN_OK;
}

/* ---- the checks ---- */
enum { N = 300, LIMIT = 60, TRIM = 2, EXPANSION = 5 };

static void check_problem(const cpecan_anchor_problem *q, const int64_t *runs, int64_t n, const cpecan_anchor_stats *st,
                          const cpecan_strand_result *sr, int mode) {
    const int searched = q->lX > 0 && q->lY > 0 && q->lX * q->lY > LIMIT;
    int64_t pX = 0, pY = 0, columns = 0, largest = 0;
    for (int64_t j = 0; j <= n; j++) {
        const int64_t x = j < n ? runs[4 * j] : q->lX, y = j < n ? runs[4 * j + 1] : q->lY, len = j < n ? runs[4 * j + 2] : 0;
        CHECK(x >= pX && y >= pY && x + len <= q->lX && y + len <= q->lY); /* increasing, inside the problem */
        if (j < n) CHECK(len > 0 && runs[4 * j + 3] == EXPANSION && (j == 0 || (x > runs[4 * j - 4] && y > runs[4 * j - 3])));
        if ((x - pX) * (y - pY) > largest) largest = (x - pX) * (y - pY);
        columns += len;
        pX = x + len;
        pY = y + len;
    }
    CHECK(st->runs == n && st->anchorColumns == columns && st->largestGap == largest && st->largestGapTop >= largest);
    CHECK(st->kernelMs == passMs && st->capped == 0);
    if (searched) {
        CHECK(st->hits == 3 * (1 + st->subProblems) && st->hsps == 2 * (1 + st->subProblems) && st->chained == n);
        CHECK((st->subProblems > 0) == (st->largestGapTop > LIMIT));
    } else {
        CHECK(n == 0 && st->hits == 0 && st->hsps == 0 && st->chained == 0 && st->subProblems == 0 && largest == q->lX * q->lY);
    }
    if (mode == CPECAN_STRAND_BOTH) {
        CHECK(sr->strand == (sr->scoreMinus > sr->scorePlus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS));
        CHECK(q->lX > 0 && q->lY > 0 ? sr->scorePlus >= 0 && sr->scoreMinus >= 0 : sr->scorePlus == 0 && sr->scoreMinus == 0);
    } else {
        const int32_t mine = mode == CPECAN_STRAND_MINUS ? sr->scoreMinus : sr->scorePlus;
        CHECK(sr->strand == mode && (mode == CPECAN_STRAND_MINUS ? sr->scorePlus : sr->scoreMinus) == -1);
        CHECK(searched ? mine >= 0 : mine == -1);
    }
}

static void free_runs(int64_t **runs, int64_t n) {
    for (int64_t i = 0; i < n; i++) free(runs[i]);
}

int main(void) {
    cpecan_anchor_problem *q = calloc(N, sizeof *q);
    int64_t *runs[N], nRuns[N];
    cpecan_anchor_stats *stats = malloc(sizeof *stats * N);
    cpecan_strand_result *strands = malloc(sizeof *strands * N);
    for (int i = 0; i < N; i++) { /* every 50th empty on one side, every 7th at or under the limit, the others up to 600 long */
        q[i].lX = i % 50 == 49 ? 0 : i % 7 == 3 ? 1 + rnd(7) : 100 + rnd(500);
        q[i].lY = i % 50 == 24 ? 0 : i % 7 == 3 ? 1 + rnd(7) : 101 + rnd(500);
        char *sX = malloc((size_t)q[i].lX + 1), *sY = malloc((size_t)q[i].lY + 1);
        for (int64_t k = 0; k < q[i].lX; k++) sX[k] = "ACGTacgtN"[rnd(9)];
        for (int64_t k = 0; k < q[i].lY; k++) sY[k] = "ACGTacgtN"[rnd(9)];
        q[i].sX = sX;
        q[i].sY = sY;
    }
    for (int mode = CPECAN_STRAND_PLUS; mode <= CPECAN_STRAND_BOTH; mode++) {
        passes = 0, passMs = 0.0;
        int rc = cpecan_find_anchor_runs_many_stranded(q, N, TRIM, EXPANSION, LIMIT, 10 * LIMIT, NULL, 0, mode, runs, nRuns, stats, strands);
        CHECK(rc == CPECAN_OK && passes == 2 && contexts == 0);
        CHECK(passProblems[1] > 16 * 64); /* the gap list doubled from 64 slots at least five times */
        int64_t subs = 0;
        for (int i = 0; i < N; i++) {
            check_problem(&q[i], runs[i], nRuns[i], &stats[i], &strands[i], mode);
            subs += stats[i].subProblems;
        }
        CHECK(subs == passProblems[1]);
        free_runs(runs, N);
    }
    /* the other entry points: no statistics, no strands, one problem, steps 1-5 alone */
    passes = 0, passMs = 0.0;
    CHECK(cpecan_find_anchor_runs_many(q, N, TRIM, EXPANSION, LIMIT, LIMIT, NULL, 0, runs, nRuns, NULL) == CPECAN_OK && passes == 2);
    free_runs(runs, N);
    passMs = 0.0;
    CHECK(cpecan_find_anchor_runs(q[0].sX, q[0].lX, q[0].sY, q[0].lY, TRIM, EXPANSION, LIMIT, LIMIT, NULL, runs, nRuns, stats) == CPECAN_OK);
    check_problem(&q[0], runs[0], nRuns[0], &stats[0], &(cpecan_strand_result){CPECAN_STRAND_PLUS, 0, -1, 0}, CPECAN_STRAND_PLUS);
    free_runs(runs, 1);
    passes = 0;
    CHECK(cpecan_find_anchor_runs_once(q[3].sX, q[3].lX, q[3].sY, q[3].lY, TRIM, EXPANSION, 0, NULL, runs, nRuns) == CPECAN_OK);
    CHECK(passes == 2 && passProblems[0] == 1 && passProblems[1] == 0 && nRuns[0] >= 0); /* under the limit, searched all the same */
    free_runs(runs, 1);
    CHECK(cpecan_find_anchor_runs_many(q, 0, TRIM, EXPANSION, LIMIT, LIMIT, NULL, 0, NULL, NULL, NULL) == CPECAN_OK);
    /* refusals leave the outputs defined */
    runs[0] = (int64_t *)q;
    nRuns[0] = 7;
    CHECK(cpecan_find_anchor_runs_many(q, N, TRIM, EXPANSION, LIMIT, LIMIT, NULL, 5, runs, nRuns, stats) == CPECAN_ENODEVICE);
    CHECK(runs[0] == NULL && nRuns[0] == 0 && strstr(lastError, "no usable HIP device"));
    CHECK(cpecan_find_anchor_runs_many(q, N, -1, EXPANSION, LIMIT, LIMIT, NULL, 5, runs, nRuns, stats) == CPECAN_EINVAL);
    CHECK(cpecan_find_anchor_runs_many_stranded(q, N, TRIM, EXPANSION, LIMIT, LIMIT, NULL, 0, 3, runs, nRuns, stats, strands) == CPECAN_EINVAL);
    CHECK(contexts == 0);

    for (int i = 0; i < N; i++) {
        free((char *)q[i].sX);
        free((char *)q[i].sY);
    }
    free(q);
    free(stats);
    free(strands);
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
