/*
 * The host side of the local chains (cpecan_amd/csrc/cpecan_local.c, on the layout stage of cpecan_anchor.c) without the
 * library, HIP or a GPU, built with -fsanitize=address,undefined by tests/test_local_c.py: this file stands in for the few
 * cpk_* functions the two files call.  Its cpk_local_pass hands back seeded synthetic chains -- up to maxChains per caller
 * problem, each a strictly increasing list of runs, some with none -- in arrays of exactly the size it says, the run blocks
 * of the problems in reverse list order.  main calls the public entry point on a few hundred problems in all three strand
 * modes and checks every record against what the pass made, turns every chain with runs into a cigar whose operations must
 * add up to its coordinates, and tries the refusals.  Everything is freed: the leak check of the sanitizer stays on.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"
#include "cpecan_local.h"

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
static int64_t contexts = 0, passes = 0, devices = 1;

void cpk_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(lastError, sizeof lastError, fmt, ap);
    va_end(ap);
}
int cpk_device_count(void) { return (int)devices; }
int cpk_current_device(void) { return 0; }
void cpecan_cigar_clear(cpecan_cigar *c) {
    free(c->contig1);
    free(c->contig2);
    free(c->ops);
    memset(c, 0, sizeof *c);
}

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

int cpk_anchor_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int32_t **runs, double *ms) {
    (void)c, (void)pass, (void)probs, (void)n, (void)ms;
    *runs = NULL;
    CHECK(!"the local entry point runs no anchor pass");
    return CPECAN_EINVAL;
}

/* what the last pass made, for main to compare with: per caller problem of the list */
typedef struct {
    int32_t nChains, nRuns, rounds, twins;
    CpkLocalChain chains[CPK_LOCAL_MAX_CHAINS];
    int32_t runs[3 * 4 * CPK_LOCAL_MAX_CHAINS];
} Made;
static Made *made = NULL;
static int64_t nMade = 0;
static int32_t wantTrim = 0, wantChains = 1, wantScore = 800;

int cpk_local_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, const CpkLocalPass *lp, CpkAnchorProblem *probs, int64_t n,
                   CpkLocalProblem *lprobs, int64_t nLocal, CpkLocalChain **chains, int32_t **runs, double *ms) {
    passes++;
    *chains = NULL;
    *runs = NULL;
    CHECK(n > 0 && nLocal > 0 && pass->trim == wantTrim && lp->maxChains == wantChains && lp->minChainScore == wantScore);
    free(made);
    made = calloc((size_t)nLocal, sizeof *made);
    nMade = nLocal;
    int64_t total = 0;
    for (int64_t k = 0; k < nLocal; k++) {
        CpkLocalProblem *q = &lprobs[k];
        const CpkAnchorProblem *p = &probs[q->first];
        Made *m = &made[k];
        CHECK(q->twins >= 1 && q->twins <= 2 && q->first >= 0 && q->first + q->twins <= n);
        CHECK(p->lX > 0 && p->lY > 0 && p->softMask == 1 && p->xOff + p->lX <= c->nForward && p->yOff + p->lY <= c->nSym);
        CHECK(q->twins == 1 || ((probs[q->first + 1].flags & CPK_ANCHOR_SHARE_X) && (probs[q->first + 1].flags & CPK_ANCHOR_RC_Y) &&
                                !(p->flags & CPK_ANCHOR_RC_Y)));
        m->twins = q->twins;
        m->nChains = (int32_t)rnd(lp->maxChains + 1);
        m->rounds = m->nChains + (int32_t)rnd(2);
        for (int32_t j = 0; j < m->nChains; j++) {
            CpkLocalChain *ch = &m->chains[j];
            const int minus = q->twins == 2 ? (int)rnd(2) : (p->flags & CPK_ANCHOR_RC_Y) != 0;
            ch->strand = minus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
            ch->score = 100000 - 1000 * j;
            ch->runOff = m->nRuns;
            int64_t x = rnd(5), y = rnd(5);
            ch->x0 = (int32_t)x;
            ch->y0 = (int32_t)y;
            for (int u = (int)rnd(5); u > 0; u--) {
                const int64_t len = 1 + rnd(6);
                if (x + len > p->lX || y + len > p->lY) break;
                int32_t *r = m->runs + 3 * (m->nRuns++);
                r[0] = (int32_t)x, r[1] = (int32_t)y, r[2] = (int32_t)len;
                ch->nRuns++;
                x += len + rnd(4);
                y += len + rnd(4);
            }
            ch->nHsps = ch->nRuns + 1;
            ch->x1 = (int32_t)x;
            ch->y1 = (int32_t)y;
        }
        total += 1 + m->nRuns;
    }
    /* arrays of exactly their size; the run blocks in reverse list order, a triple that is nobody's in front of each */
    CpkLocalChain *outChains = malloc(sizeof *outChains * (size_t)(nLocal * lp->maxChains));
    int32_t *outRuns = malloc(sizeof *outRuns * 3 * (size_t)total);
    int64_t at = 0;
    for (int64_t k = nLocal - 1; k >= 0; k--) {
        const Made *m = &made[k];
        for (int v = 0; v < 3; v++) outRuns[3 * at + v] = -12345;
        probs[lprobs[k].first].hspOff = ++at;
        memcpy(outRuns + 3 * at, m->runs, sizeof(int32_t) * 3 * (size_t)m->nRuns);
        at += m->nRuns;
        for (int32_t j = 0; j < lp->maxChains; j++) {
            if (j < m->nChains) outChains[k * lp->maxChains + j] = m->chains[j];
            else memset(&outChains[k * lp->maxChains + j], 0x55, sizeof *outChains);
        }
        lprobs[k].nChains = m->nChains;
        lprobs[k].nRuns = m->nRuns;
        lprobs[k].rounds = m->rounds;
        for (int t = 0; t < m->twins; t++) {
            probs[lprobs[k].first + t].hits = 30 + t;
            probs[lprobs[k].first + t].hsps = 20 + t;
            probs[lprobs[k].first + t].capped = t;
        }
    }
    CHECK(at == total);
    *chains = outChains;
    *runs = outRuns;
    *ms += 0.25;
    return CPECAN_OK;
}

/* ---- the call ---- */
#define N 230
static char *seqs[2 * N];

static void one_call(int strandMode, int32_t K, int32_t S, int64_t trim) {
    cpecan_anchor_problem problems[N];
    cpecan_local_chain *chains[N];
    int64_t *runs[N], nChains[N], nRuns[N];
    cpecan_local_stats stats[N];
    memset(chains, 0x11, sizeof chains); /* the call must zero its outputs */
    memset(runs, 0x11, sizeof runs);
    int64_t live = 0;
    for (int i = 0; i < N; i++) {
        const int64_t lX = i % 17 == 3 ? 0 : 8 + rnd(40), lY = i % 23 == 5 ? 0 : 8 + rnd(40);
        seqs[2 * i] = malloc((size_t)(lX ? lX : 1));     /* exactly lX bytes: no terminator to lean on */
        seqs[2 * i + 1] = malloc((size_t)(lY ? lY : 1));
        for (int64_t k = 0; k < lX; k++) seqs[2 * i][k] = "ACGT"[rnd(4)];
        for (int64_t k = 0; k < lY; k++) seqs[2 * i + 1][k] = "ACGT"[rnd(4)];
        problems[i] = (cpecan_anchor_problem){lX ? seqs[2 * i] : NULL, lX, lY ? seqs[2 * i + 1] : NULL, lY};
        live += lX > 0 && lY > 0;
    }
    cpecan_local_options o;
    cpecan_local_options_default(&o);
    o.maxChains = K;
    o.minChainScore = S;
    wantTrim = (int32_t)trim, wantChains = K, wantScore = S ? S : 800;
    const int64_t before = passes;
    const int rc = cpecan_find_local_chains_many(problems, N, trim, 12, NULL, NULL, &o, 0, strandMode, chains, nChains, runs, nRuns, stats);
    CHECK(rc == CPECAN_OK && passes == before + 1 && contexts == 0 && nMade == live);
    int64_t k = 0;
    for (int i = 0; rc == CPECAN_OK && i < N; i++) {
        if (problems[i].lX == 0 || problems[i].lY == 0) {
            CHECK(chains[i] == NULL && runs[i] == NULL && nChains[i] == 0 && nRuns[i] == 0 && stats[i].rounds == 0 && stats[i].hitsPlus == 0);
            CHECK(stats[i].kernelMs == 0.25);
            continue;
        }
        const Made *m = &made[k++];
        CHECK(nChains[i] == m->nChains && nRuns[i] == m->nRuns && stats[i].rounds == m->rounds && stats[i].kernelMs == 0.25);
        if (strandMode == CPECAN_STRAND_BOTH) CHECK(stats[i].hitsPlus == 30 && stats[i].hitsMinus == 31 && stats[i].hspsPlus == 20 && stats[i].hspsMinus == 21 && stats[i].capped == 2);
        if (strandMode == CPECAN_STRAND_PLUS) CHECK(stats[i].hitsPlus == 30 && stats[i].hitsMinus == 0 && stats[i].hspsMinus == 0 && stats[i].capped == 0);
        if (strandMode == CPECAN_STRAND_MINUS) CHECK(stats[i].hitsPlus == 0 && stats[i].hitsMinus == 30 && stats[i].hspsMinus == 20);
        for (int64_t u = 0; u < nRuns[i]; u++)
            CHECK(runs[i][4 * u] == m->runs[3 * u] && runs[i][4 * u + 1] == m->runs[3 * u + 1] && runs[i][4 * u + 2] == m->runs[3 * u + 2] && runs[i][4 * u + 3] == 12);
        for (int64_t j = 0; j < nChains[i]; j++) {
            const cpecan_local_chain *c = &chains[i][j];
            const CpkLocalChain *w = &m->chains[j];
            CHECK(c->strand == w->strand && c->score == w->score && c->nHsps == w->nHsps && c->runOff == w->runOff && c->nRuns == w->nRuns);
            CHECK(c->x0 == w->x0 && c->x1 == w->x1 && c->y0 == w->y0 && c->y1 == w->y1 && c->runOff + c->nRuns <= nRuns[i]);
            cpecan_cigar g;
            const int rg = cpecan_cigar_from_local_chain("target", "query", problems[i].lY, c, runs[i], &g);
            if (c->nRuns == 0) {
                CHECK(rg == CPECAN_EINVAL);
                continue;
            }
            CHECK(rg == CPECAN_OK);
            if (rg != CPECAN_OK) continue;
            int64_t span1 = 0, span2 = 0, matches = 0;
            for (int64_t t = 0; t < g.nOps; t++) {
                CHECK(g.ops[2 * t + 1] > 0);
                if (g.ops[2 * t] != CPECAN_OP_INDEL_Y) span1 += g.ops[2 * t + 1];
                if (g.ops[2 * t] != CPECAN_OP_INDEL_X) span2 += g.ops[2 * t + 1];
                matches += g.ops[2 * t] == CPECAN_OP_MATCH;
            }
            CHECK(matches == c->nRuns && g.strand1 == 1 && g.end1 - g.start1 == span1 && g.score == (double)c->score);
            CHECK(g.strand2 == (c->strand == CPECAN_STRAND_PLUS) && (g.strand2 ? g.end2 - g.start2 : g.start2 - g.end2) == span2);
            CHECK(g.start2 >= 0 && g.end2 >= 0 && g.start2 <= problems[i].lY && g.end2 <= problems[i].lY);
            CHECK(strcmp(g.contig1, "target") == 0 && strcmp(g.contig2, "query") == 0);
            cpecan_cigar_clear(&g);
        }
    }
    CHECK(k == nMade);
    for (int i = 0; i < N; i++) {
        free(chains[i]);
        free(runs[i]);
        free(seqs[2 * i]);
        free(seqs[2 * i + 1]);
    }
}

static void refusals(void) {
    const cpecan_anchor_problem q = {"ACGTACGTACGT", 12, "ACGTACGTACGT", 12};
    cpecan_local_chain *chains = (cpecan_local_chain *)&failures;
    int64_t *runs = (int64_t *)&failures, nChains = 7, nRuns = 7;
    cpecan_local_options o;
    cpecan_anchor_options a;
    const int64_t before = passes;
    devices = 0; /* every refusal comes before the device is looked for */
#define REFUSED(setup, code)                                                                                                        \
    do {                                                                                                                            \
        cpecan_local_options_default(&o);                                                                                           \
        cpecan_anchor_options_default(&a);                                                                                          \
        setup;                                                                                                                      \
        CHECK(cpecan_find_local_chains_many(&q, 1, 0, 20, NULL, &a, &o, 0, CPECAN_STRAND_BOTH, &chains, &nChains, &runs, &nRuns, NULL) == (code)); \
        CHECK(chains == NULL && runs == NULL && nChains == 0 && nRuns == 0);                                                        \
    } while (0)
    REFUSED(o.maxChains = 0, CPECAN_EINVAL);
    REFUSED(o.maxChains = 17, CPECAN_EINVAL);
    REFUSED(o.minChainScore = 799, CPECAN_EINVAL);
    REFUSED(o.minChainScore = -1, CPECAN_EINVAL);
    REFUSED(o.reserved[5] = 1, CPECAN_EINVAL);
    REFUSED(a.gappedExtension = 1, CPECAN_EINVAL);
    REFUSED(a.reserved[0] = 1, CPECAN_EINVAL);
    REFUSED(o.maxChains = 16, CPECAN_ENODEVICE);
    REFUSED(o.minChainScore = 800, CPECAN_ENODEVICE);
    devices = 1;
    CHECK(passes == before);
    CHECK(cpecan_find_local_chains_many(&q, 1, 0, 20, NULL, NULL, NULL, 0, 7, &chains, &nChains, &runs, &nRuns, NULL) == CPECAN_EINVAL);
    CHECK(cpecan_find_local_chains_many(&q, 1, 0, 20, NULL, NULL, NULL, 0, 0, NULL, &nChains, &runs, &nRuns, NULL) == CPECAN_EINVAL);
    CHECK(cpecan_find_local_chains_many(NULL, 0, 0, 20, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL) == CPECAN_OK);
}

int main(void) {
    refusals();
    for (int mode = CPECAN_STRAND_PLUS; mode <= CPECAN_STRAND_BOTH; mode++) {
        one_call(mode, 1, 0, 0);
        one_call(mode, 4, 900, 14);
        one_call(mode, 16, 0, 3);
    }
    free(made);
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
