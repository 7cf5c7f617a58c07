/*
 * The host side of local chains with gapped extension (cpecan_find_local_chains_many_gapped of cpecan_amd/csrc/cpecan_local.c;
 * DESIGN.md section 7, step 7b) without the library, HIP or a GPU, built with -fsanitize=address,undefined by
 * tests/test_local_gapped_c.py.  This file stands in for the cpk_* functions that cpecan_local.c and cpecan_anchor.c call.
 * Its cpk_local_pass checks what the option must have put into every problem of the list -- CPK_ANCHOR_GAPPED, the
 * anti-diagonals above the flag bits, yDrop, the same in both twins -- and hands back what a pass that extends chains hands
 * back: chains with more runs than HSPs, in a run list of its own that only hspOff points to, in arrays of exactly their
 * size.  main calls the entry point in all three strand modes with the option on at its defaults, on with values of its own
 * and off, checks every record, turns every chain into a cigar, and tries the refusals with no device present.
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

static uint64_t rngState = 0x2545F4914F6CDD1Dull;
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
    CHECK(device == 0 && bytes && nBytes > 0 && nExtra >= 0);
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

/* what the last pass made, per caller problem of the list; a chain of h HSPs has up to 3 * h + 2 runs */
#define MAX_HSPS 3
#define MAX_RUNS (3 * MAX_HSPS + 2)
typedef struct {
    int32_t nChains, nRuns, rounds;
    CpkLocalChain chains[CPK_LOCAL_MAX_CHAINS];
    int32_t runs[3 * MAX_RUNS * CPK_LOCAL_MAX_CHAINS];
} Made;
static Made *made = NULL;
static int64_t nMade = 0, moreRunsThanHsps = 0;
static int32_t wantChains = 1, wantFlags = 0, wantYDrop = 0; /* wantFlags: what every problem carries above RC_Y / SHARE_X */

int cpk_local_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, const CpkLocalPass *lp, CpkAnchorProblem *probs, int64_t n,
                   CpkLocalProblem *lprobs, int64_t nLocal, CpkLocalChain **chains, int32_t **runs, double *ms) {
    passes++;
    *chains = NULL;
    *runs = NULL;
    CHECK(n > 0 && nLocal > 0 && lp->maxChains == wantChains && pass->trim == 5);
    for (int64_t i = 0; i < n; i++) { /* the option travels with every problem, twins included, and nothing else does */
        CHECK((probs[i].flags & ~(CPK_ANCHOR_RC_Y | CPK_ANCHOR_SHARE_X)) == wantFlags && probs[i].yDrop == wantYDrop);
        CHECK(probs[i].yOff + probs[i].lY <= c->nSym);
    }
    free(made);
    made = calloc((size_t)nLocal, sizeof *made);
    nMade = nLocal;
    int64_t total = 0;
    for (int64_t k = 0; k < nLocal; k++) {
        CpkLocalProblem *q = &lprobs[k];
        const CpkAnchorProblem *p = &probs[q->first];
        Made *m = &made[k];
        m->nChains = (int32_t)rnd(lp->maxChains + 1);
        m->rounds = m->nChains + (int32_t)rnd(2);
        for (int32_t j = 0; j < m->nChains; j++) {
            CpkLocalChain *ch = &m->chains[j];
            const int minus = q->twins == 2 ? (int)rnd(2) : (p->flags & CPK_ANCHOR_RC_Y) != 0;
            ch->strand = minus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
            ch->score = 90000 - 1000 * j;
            ch->nHsps = 1 + (int32_t)rnd(MAX_HSPS);
            ch->runOff = m->nRuns;
            int64_t x = rnd(3), y = rnd(3);
            ch->x0 = (int32_t)x;
            ch->y0 = (int32_t)y;
            const int want = wantFlags ? (int)rnd(3 * ch->nHsps + 3) : (int)rnd(ch->nHsps + 1); /* extended: up to 3 h + 2 */
            for (int u = 0; u < want; u++) {
                const int64_t len = 1 + rnd(3);
                if (x + len > p->lX || y + len > p->lY) break;
                int32_t *r = m->runs + 3 * (m->nRuns++);
                r[0] = (int32_t)x, r[1] = (int32_t)y, r[2] = (int32_t)len;
                ch->nRuns++;
                x += len + rnd(2);
                y += len + rnd(2);
            }
            moreRunsThanHsps += ch->nRuns > ch->nHsps;
            ch->x1 = (int32_t)x;
            ch->y1 = (int32_t)y;
        }
        total += 2 + m->nRuns;
    }
    /* a run list of its own, exactly its size: the problems in reverse order, two triples that are nobody's before each */
    CpkLocalChain *outChains = malloc(sizeof *outChains * (size_t)(nLocal * lp->maxChains));
    int32_t *outRuns = malloc(sizeof *outRuns * 3 * (size_t)total);
    int64_t at = 0;
    for (int64_t k = nLocal - 1; k >= 0; k--) {
        const Made *m = &made[k];
        for (int v = 0; v < 6; v++) outRuns[3 * at + v] = -4321;
        at += 2;
        probs[lprobs[k].first].hspOff = at;
        if (lprobs[k].twins == 2) probs[lprobs[k].first + 1].hspOff = -1000000; /* the first twin's alone counts */
        memcpy(outRuns + 3 * at, m->runs, sizeof(int32_t) * 3 * (size_t)m->nRuns);
        at += m->nRuns;
        for (int32_t j = 0; j < lp->maxChains; j++) {
            if (j < m->nChains) outChains[k * lp->maxChains + j] = m->chains[j];
            else memset(&outChains[k * lp->maxChains + j], 0x66, sizeof *outChains);
        }
        lprobs[k].nChains = m->nChains;
        lprobs[k].nRuns = m->nRuns;
        lprobs[k].rounds = m->rounds;
    }
    CHECK(at == total);
    *chains = outChains;
    *runs = outRuns;
    *ms += 0.5;
    return CPECAN_OK;
}

/* ---- the call ---- */
#define N 150
static void one_call(int strandMode, int32_t K, const cpecan_anchor_options *a, int32_t flags, int32_t yDrop) {
    static char *seqs[2 * N];
    cpecan_anchor_problem problems[N];
    cpecan_local_chain *chains[N];
    int64_t *runs[N], nChains[N], nRuns[N];
    cpecan_local_stats stats[N];
    memset(chains, 0x11, sizeof chains);
    memset(runs, 0x11, sizeof runs);
    int64_t live = 0;
    for (int i = 0; i < N; i++) {
        const int64_t lX = i % 13 == 2 ? 0 : 8 + rnd(30), lY = i % 19 == 4 ? 0 : 8 + rnd(30);
        seqs[2 * i] = malloc((size_t)(lX ? lX : 1));
        seqs[2 * i + 1] = malloc((size_t)(lY ? lY : 1));
        for (int64_t k = 0; k < lX; k++) seqs[2 * i][k] = "ACGT"[rnd(4)];
        for (int64_t k = 0; k < lY; k++) seqs[2 * i + 1][k] = "ACGT"[rnd(4)];
        problems[i] = (cpecan_anchor_problem){lX ? seqs[2 * i] : NULL, lX, lY ? seqs[2 * i + 1] : NULL, lY};
        live += lX > 0 && lY > 0;
    }
    cpecan_local_options o;
    cpecan_local_options_default(&o);
    o.maxChains = K;
    wantChains = K, wantFlags = flags, wantYDrop = yDrop;
    const int64_t before = passes;
    const int rc = cpecan_find_local_chains_many_gapped(problems, N, 5, 12, NULL, a, &o, 0, strandMode, chains, nChains, runs, nRuns, stats);
    CHECK(rc == CPECAN_OK && passes == before + 1 && contexts == 0 && nMade == live);
    int64_t k = 0;
    for (int i = 0; rc == CPECAN_OK && i < N; i++) {
        if (problems[i].lX == 0 || problems[i].lY == 0) {
            CHECK(chains[i] == NULL && runs[i] == NULL && nChains[i] == 0 && nRuns[i] == 0 && stats[i].kernelMs == 0.5);
            continue;
        }
        const Made *m = &made[k++];
        CHECK(nChains[i] == m->nChains && nRuns[i] == m->nRuns && stats[i].rounds == m->rounds && stats[i].kernelMs == 0.5);
        for (int64_t u = 0; u < nRuns[i]; u++)
            CHECK(runs[i][4 * u] == m->runs[3 * u] && runs[i][4 * u + 1] == m->runs[3 * u + 1] && runs[i][4 * u + 2] == m->runs[3 * u + 2] && runs[i][4 * u + 3] == 12);
        for (int64_t j = 0; j < nChains[i]; j++) {
            const cpecan_local_chain *c = &chains[i][j];
            const CpkLocalChain *w = &m->chains[j];
            CHECK(c->strand == w->strand && c->score == w->score && c->nHsps == w->nHsps && c->runOff == w->runOff && c->nRuns == w->nRuns);
            CHECK(c->x0 == w->x0 && c->x1 == w->x1 && c->y0 == w->y0 && c->y1 == w->y1 && c->runOff + c->nRuns <= nRuns[i]);
            cpecan_cigar g;
            const int rg = cpecan_cigar_from_local_chain("target", "query", problems[i].lY, c, runs[i], &g);
            CHECK(rg == (c->nRuns ? CPECAN_OK : CPECAN_EINVAL));
            if (rg != CPECAN_OK) continue;
            int64_t span1 = 0, span2 = 0, matches = 0;
            for (int64_t t = 0; t < g.nOps; t++) {
                if (g.ops[2 * t] != CPECAN_OP_INDEL_Y) span1 += g.ops[2 * t + 1];
                if (g.ops[2 * t] != CPECAN_OP_INDEL_X) span2 += g.ops[2 * t + 1];
                matches += g.ops[2 * t] == CPECAN_OP_MATCH;
            }
            CHECK(matches == c->nRuns && g.end1 - g.start1 == span1 && (g.strand2 ? g.end2 - g.start2 : g.start2 - g.end2) == span2);
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
#define REFUSED(entry, setup, code)                                                                                  \
    do {                                                                                                             \
        cpecan_local_options_default(&o);                                                                            \
        cpecan_anchor_options_default(&a);                                                                           \
        setup;                                                                                                       \
        CHECK(entry(&q, 1, 0, 20, NULL, &a, &o, 0, CPECAN_STRAND_BOTH, &chains, &nChains, &runs, &nRuns, NULL) == (code)); \
        CHECK(chains == NULL && runs == NULL && nChains == 0 && nRuns == 0);                                         \
    } while (0)
    REFUSED(cpecan_find_local_chains_many_gapped, o.maxChains = 0, CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, o.minChainScore = 799, CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, o.reserved[2] = 1, CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, a.gappedExtension = 2, CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, (a.gappedExtension = 1, a.yDrop = -1), CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, (a.gappedExtension = 1, a.gappedMaxDiagonals = 63), CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, (a.gappedExtension = 1, a.gappedMaxDiagonals = 4097), CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, a.yDrop = 500, CPECAN_EINVAL); /* wants gappedExtension */
    REFUSED(cpecan_find_local_chains_many_gapped, a.gappedMaxDiagonals = 64, CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, (a.gappedExtension = 1, a.reserved[0] = 1), CPECAN_EINVAL);
    REFUSED(cpecan_find_local_chains_many_gapped, a.gappedExtension = 1, CPECAN_ENODEVICE);
    REFUSED(cpecan_find_local_chains_many_gapped, (a.gappedExtension = 1, a.yDrop = 1, a.gappedMaxDiagonals = 4096), CPECAN_ENODEVICE);
    REFUSED(cpecan_find_local_chains_many_gapped, a.gappedExtension = 0, CPECAN_ENODEVICE);
    REFUSED(cpecan_find_local_chains_many, a.gappedExtension = 1, CPECAN_EINVAL); /* the entry point of before still refuses */
    devices = 1;
    CHECK(passes == before);
    CHECK(cpecan_find_local_chains_many_gapped(&q, 1, 0, 20, NULL, NULL, NULL, 0, 7, &chains, &nChains, &runs, &nRuns, NULL) == CPECAN_EINVAL);
    CHECK(cpecan_find_local_chains_many_gapped(NULL, 0, 0, 20, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL) == CPECAN_OK);
}

int main(void) {
    refusals();
    cpecan_anchor_options on, own, off;
    cpecan_anchor_options_default(&on);
    cpecan_anchor_options_default(&own);
    cpecan_anchor_options_default(&off);
    on.gappedExtension = own.gappedExtension = 1;
    own.yDrop = 600;
    own.gappedMaxDiagonals = 64;
    for (int mode = CPECAN_STRAND_PLUS; mode <= CPECAN_STRAND_BOTH; mode++) {
        one_call(mode, 1, &on, CPK_ANCHOR_GAPPED | (CPK_ANCHOR_GAPPED_MAX_DIAGS << CPK_ANCHOR_DIAGS_SHIFT), CPK_ANCHOR_GAPPED_Y_DROP);
        one_call(mode, 4, &own, CPK_ANCHOR_GAPPED | (64 << CPK_ANCHOR_DIAGS_SHIFT), 600);
        one_call(mode, 16, &off, 0, 0);
        one_call(mode, 3, NULL, 0, 0);
    }
    CHECK(moreRunsThanHsps > 50);
    free(made);
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
