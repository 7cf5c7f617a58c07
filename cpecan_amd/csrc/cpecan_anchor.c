/*
 * cpecan_anchor.c -- host side of the anchor finder (include/cpecan_hip.h: cpecan_find_anchor_runs_many_stranded).
 * The kernels (cpk_anchor.inl) do steps 1-5 on a list of problems; this file lays the sequences of a call out in one
 * buffer, runs the top-level pass, makes the second pass's problems out of the gaps between the top-level anchors
 * (getBlastPairsForPairwiseAlignmentParameters, impl/pairwiseAligner.c:1175-1191) and splices the runs together.
 * A call is a sequence of stages -- check, layout, strand pick, gaps, splice -- around the two passes; no stage touches a
 * device (cpecan_internal.h declares them, tests/test_anchor_stages_cpu.py runs them with the model in the passes' place).
 * Strand: a problem that may lie on the minus strand gets a twin in the top-level pass whose
 * Y is the reverse complement, written on the device behind the forward symbols; the chain scores of the two decide, and
 * only the chosen orientation goes on to the gaps and the splice.
 * Gapped extension (step 5b, cpecan_anchor_options.gappedExtension) is a flag and two values on every problem of both
 * passes; the stages work on whatever runs a pass returns, so they do not know about it.
 */
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"

int cpecan_anchor_params_default(cpecan_anchor_params *p) {
    if (!p) return CPECAN_EINVAL;
    /* HOXD70 (lastz's default matrix), rows and columns a c g t */
    static const int32_t hoxd70[16] = {91, -114, -31, -123, -114, 100, -125, -31, -31, -125, 100, -114, -123, -31, -114, 91};
    memset(p, 0, sizeof *p);
    strcpy(p->seed, "1110100110010101111");
    p->maxSeedOccurrences = 1;
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 5; b++) p->scores[a * 5 + b] = (a < 4 && b < 4) ? hoxd70[a * 4 + b] : -100;
    p->xDrop = 910;
    p->hspThreshold = 800;
    p->maxHsps = 4096;
    p->seedTransitions = 0; /* lastz's own default is 1 (--transition); DESIGN.md section 7 */
    return CPECAN_OK;
}

int cpecan_anchor_options_default(cpecan_anchor_options *o) {
    if (!o) return CPECAN_EINVAL;
    memset(o, 0, sizeof *o);
    return CPECAN_OK;
}

int cpecan_reverse_complement(const char *s, int64_t l, char *out) {
    if (l < 0 || (l > 0 && (!s || !out))) return CPECAN_EINVAL;
    static const char from[] = "ACGTacgt", to[] = "TGCAtgca";
    for (int64_t i = 0, j = l - 1; i <= j; i++, j--) { /* from both ends inwards: out may be s */
        unsigned char a = (unsigned char)s[i], b = (unsigned char)s[j];
        const char *fa = a ? strchr(from, a) : NULL, *fb = b ? strchr(from, b) : NULL;
        if (fa) a = (unsigned char)to[fa - from];
        if (fb) b = (unsigned char)to[fb - from];
        out[i] = (char)b;
        out[j] = (char)a;
    }
    return CPECAN_OK;
}

static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

void cpk_anchor_list_free(CpkAnchorList *l) {
    free(l->probs);
    free(l->owner);
    free(l->before);
}

/* One more problem at the end of the list, zeroed; NULL when there is no memory (the list stays as it was). */
static CpkAnchorProblem *list_push(CpkAnchorList *l, int64_t owner, int64_t before) {
    if (l->n == l->cap) {
        const size_t cap = l->cap ? 2 * (size_t)l->cap : 64;
        void *p;
        if (!(p = realloc(l->probs, sizeof *l->probs * cap))) return NULL;
        l->probs = p;
        if (!(p = realloc(l->owner, sizeof *l->owner * cap))) return NULL;
        l->owner = p;
        if (!(p = realloc(l->before, sizeof *l->before * cap))) return NULL;
        l->before = p;
        l->cap = (int64_t)cap;
    }
    l->owner[l->n] = owner;
    l->before[l->n] = before;
    return memset(&l->probs[l->n++], 0, sizeof *l->probs);
}

/* The rectangle in front of every run and behind the last (_gaps of tests/anchor_model.py): gap j is (pX, pY) .. (x, y),
 * and for j < n run j, of len columns, starts at (x, y).  The runs are triples of a pass (r3) or quadruples of a result
 * (r4); a walk starts with j = -1 and the rest of the last line 0. */
typedef struct {
    const int32_t *r3;
    const int64_t *r4;
    int64_t n, lX, lY;
    int64_t j, pX, pY, x, y, len;
} GapWalk;

static inline int gap_next(GapWalk *w) { /* inline: the walk's state stays in registers */
    if (w->j == w->n) return 0;
    const int64_t j = ++w->j;
    w->pX = w->x + w->len;
    w->pY = w->y + w->len;
    w->x = j == w->n ? w->lX : w->r3 ? w->r3[3 * j] : w->r4[4 * j];
    w->y = j == w->n ? w->lY : w->r3 ? w->r3[3 * j + 1] : w->r4[4 * j + 1];
    w->len = j == w->n ? 0 : w->r3 ? w->r3[3 * j + 2] : w->r4[4 * j + 2];
    return 1;
}

static int64_t gap_matrix(const GapWalk *w) { return (w->x - w->pX) * (w->y - w->pY); }

int cpk_anchor_check(const CpkAnchorCall *c, int64_t trim, const cpecan_anchor_params *params,
                     const cpecan_anchor_options *options, CpkAnchorPass *pass) {
    const int64_t n = c->n;
    if (n < 0 || (n > 0 && (!c->problems || !c->runs || !c->nRuns)) || trim < 0 || trim > (1 << 24) ||
        c->strandMode < CPECAN_STRAND_PLUS || c->strandMode > CPECAN_STRAND_BOTH) {
        cpk_set_error("%s: bad arguments", c->who);
        return CPECAN_EINVAL;
    }
    cpecan_anchor_params def;
    if (!params) {
        cpecan_anchor_params_default(&def);
        params = &def;
    }
    if (memchr(params->seed, 0, sizeof params->seed) == NULL) {
        cpk_set_error("%s: the seed is not terminated", c->who);
        return CPECAN_EINVAL;
    }
    if (params->seedTransitions != 0 && params->seedTransitions != 1) {
        cpk_set_error("%s: seedTransitions is 0 or 1", c->who);
        return CPECAN_EINVAL;
    }
    /* variantThreshold: step 2's for an HSP that only variant hits extend to; hspThreshold says: no class is told from the other */
    *pass = (CpkAnchorPass){.seedTransitions = params->seedTransitions, .variantThreshold = params->hspThreshold, .trim = (int32_t)trim};
    pass->prm = (CpkAnchorParams){.maxSeedOccurrences = params->maxSeedOccurrences, .xDrop = params->xDrop,
                                  .hspThreshold = params->hspThreshold, .maxHsps = params->maxHsps};
    memcpy(pass->prm.scores, params->scores, sizeof pass->prm.scores);
    memcpy(pass->seed, params->seed, sizeof pass->seed);
    if (options) {
        for (int k = 0; k < 4; k++)
            if (options->reserved[k] != 0) {
                cpk_set_error("%s: a reserved word of the options is not 0", c->who);
                return CPECAN_EINVAL;
            }
        if (options->transitionHspThreshold < 0 ||
            (options->transitionHspThreshold != 0 && options->transitionHspThreshold < params->hspThreshold)) {
            cpk_set_error("%s: transitionHspThreshold is 0 or at least hspThreshold", c->who);
            return CPECAN_EINVAL;
        }
        if (options->transitionHspThreshold != 0) pass->variantThreshold = options->transitionHspThreshold;
        /* step 5b; what it asks for reaches the passes with the problems (mark_gapped) */
        if (options->gappedExtension != 0 && options->gappedExtension != 1) {
            cpk_set_error("%s: gappedExtension is 0 or 1", c->who);
            return CPECAN_EINVAL;
        }
        if (options->yDrop < 0 || (options->gappedMaxDiagonals != 0 && (options->gappedMaxDiagonals < CPK_ANCHOR_GAPPED_MIN_DIAGS ||
                                                                        options->gappedMaxDiagonals > CPK_ANCHOR_GAPPED_MAX_DIAGS))) {
            cpk_set_error("%s: yDrop is 0 or positive, gappedMaxDiagonals 0 or %d .. %d", c->who, CPK_ANCHOR_GAPPED_MIN_DIAGS,
                          CPK_ANCHOR_GAPPED_MAX_DIAGS);
            return CPECAN_EINVAL;
        }
        if (!options->gappedExtension && (options->yDrop != 0 || options->gappedMaxDiagonals != 0)) {
            cpk_set_error("%s: yDrop and gappedMaxDiagonals want gappedExtension", c->who);
            return CPECAN_EINVAL;
        }
    }
    for (int64_t i = 0; i < n; i++) {
        c->runs[i] = NULL;
        c->nRuns[i] = 0;
    }
    for (int64_t i = 0; i < n; i++) {
        const cpecan_anchor_problem *q = &c->problems[i];
        if (q->lX < 0 || q->lY < 0 || (q->lX > 0 && !q->sX) || (q->lY > 0 && !q->sY) || q->lX > (1 << 24) || q->lY > (1 << 24)) {
            cpk_set_error("%s: problem %lld has no sequence or one longer than 2^24", c->who, (long long)i);
            return CPECAN_EINVAL;
        }
    }
    if (c->stats) memset(c->stats, 0, sizeof *c->stats * (size_t)n);
    for (int64_t i = 0; c->strands && i < n; i++) { /* what holds without a pass: forced, or plus; nothing scored */
        c->strands[i].strand = c->strandMode == CPECAN_STRAND_MINUS ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
        c->strands[i].scorePlus = c->strands[i].scoreMinus = -1;
    }
    return CPECAN_OK;
}

/* The top-level problems, their sequences end to end in one buffer: those beyond the size limit and, with BOTH, the
 * others too, for their strand score.  A problem scored on both strands is a pair of twins, plus then minus; the
 * reverse complements get even offsets in an area that starts at the first even index behind the sequences. */
int cpk_anchor_layout(const CpkAnchorCall *c, CpkAnchorList *top, uint8_t **bytes, int64_t *nBytes, int64_t *nExtra) {
    const int both = c->strandMode == CPECAN_STRAND_BOTH, twins = both ? 2 : 1;
    *bytes = NULL;
    *nBytes = *nExtra = 0;
    for (int64_t i = 0; i < c->n; i++) {
        const cpecan_anchor_problem *q = &c->problems[i];
        if (c->stats) c->stats[i].largestGapTop = c->stats[i].largestGap = q->lX * q->lY;
        if (q->lX == 0 || q->lY == 0) { /* :1012; no HSP on either strand */
            if (c->strands && both) c->strands[i].scorePlus = c->strands[i].scoreMinus = 0;
            continue;
        }
        if (!c->once && !both && q->lX * q->lY <= c->anchorMatrixBiggerThanThis) continue;
        for (int t = 0; t < twins; t++) {
            CpkAnchorProblem *p = list_push(top, i, 0);
            if (!p) return CPECAN_ENOMEM;
            p->xOff = *nBytes;
            p->yOff = *nBytes + q->lX;
            p->lX = (int32_t)q->lX;
            p->lY = (int32_t)q->lY;
            p->softMask = c->once ? c->softMaskTop != 0 : 1; /* :1168 */
            if (both ? t : c->strandMode == CPECAN_STRAND_MINUS) {
                p->flags = CPK_ANCHOR_RC_Y | (t ? CPK_ANCHOR_SHARE_X : 0);
                p->yFwd = p->yOff;
                p->yOff = *nExtra; /* inside the area, whose place is known once nBytes is */
                *nExtra += (q->lY + 1) & ~(int64_t)1;
            }
        }
        *nBytes += q->lX + q->lY;
    }
    if (top->n == 0) return CPECAN_OK;
    if (!(*bytes = malloc((size_t)*nBytes))) return CPECAN_ENOMEM;
    for (int64_t k = 0; k < top->n; k++) {
        CpkAnchorProblem *p = &top->probs[k];
        if (p->flags & CPK_ANCHOR_RC_Y) p->yOff += (*nBytes + 1) & ~(int64_t)1;
        if (p->flags & CPK_ANCHOR_SHARE_X) continue;
        const cpecan_anchor_problem *q = &c->problems[top->owner[k]];
        memcpy(*bytes + p->xOff, q->sX, (size_t)q->lX);
        memcpy(*bytes + p->xOff + q->lX, q->sY, (size_t)q->lY);
    }
    return CPECAN_OK;
}

/* The strand of every problem; what does not go on is dropped from the list: the twin that lost and, with BOTH, the
 * problems at or under the size limit, which were there to be scored. */
void cpk_anchor_pick(const CpkAnchorCall *c, CpkAnchorList *top) {
    const int both = c->strandMode == CPECAN_STRAND_BOTH, twins = both ? 2 : 1;
    int64_t kept = 0;
    for (int64_t k = 0; k < top->n; k += twins) {
        const int64_t i = top->owner[k];
        const CpkAnchorProblem *p = &top->probs[k];
        int64_t pick = k;
        if (both) {
            const int minus = p[1].score > p[0].score; /* a tie, 0 = 0 included, is plus */
            pick = k + minus;
            if (c->strands) {
                c->strands[i].strand = minus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
                c->strands[i].scorePlus = p[0].score;
                c->strands[i].scoreMinus = p[1].score;
            }
        } else if (c->strands) {
            *(c->strandMode == CPECAN_STRAND_MINUS ? &c->strands[i].scoreMinus : &c->strands[i].scorePlus) = p->score;
        }
        if (!c->once && c->problems[i].lX * c->problems[i].lY <= c->anchorMatrixBiggerThanThis) continue;
        top->probs[kept] = top->probs[pick];
        top->owner[kept++] = i;
    }
    top->n = kept;
}

/* the gaps between consecutive top-level anchors that are still too large: the second pass (:1175-1191) */
int cpk_anchor_gaps(const CpkAnchorCall *c, const CpkAnchorList *top, const int32_t *topRuns, CpkAnchorList *sub) {
    for (int64_t k = 0; k < top->n && !c->once; k++) {
        const CpkAnchorProblem *t = &top->probs[k];
        GapWalk w = {.r3 = topRuns + 3 * t->hspOff, .n = t->nRuns, .lX = t->lX, .lY = t->lY, .j = -1};
        int64_t largest = 0;
        while (gap_next(&w)) {
            const int64_t matrix = gap_matrix(&w);
            largest = max64(largest, matrix);
            if (matrix <= c->anchorMatrixBiggerThanThis) continue;
            CpkAnchorProblem *s = list_push(sub, k, w.j);
            if (!s) return CPECAN_ENOMEM;
            s->xOff = t->xOff + w.pX;
            s->yOff = t->yOff + w.pY;
            s->lX = (int32_t)(w.x - w.pX);
            s->lY = (int32_t)(w.y - w.pY);
            s->softMask = matrix > c->repeatMaskMatrixBiggerThanThis;
        }
        if (c->stats) c->stats[top->owner[k]].largestGapTop = largest;
    }
    return CPECAN_OK;
}

static int64_t put_run(int64_t *out, int64_t m, int64_t x, int64_t y, int64_t len, int64_t expansion) {
    const int64_t q[4] = {x, y, len, expansion};
    memcpy(out + 4 * m, q, sizeof q);
    return m + 1;
}

/* splice: the gaps of a problem are in increasing order, each in front of the top-level run it recorded */
int cpk_anchor_splice(const CpkAnchorCall *c, const CpkAnchorList *top, const int32_t *topRuns, const CpkAnchorList *sub,
                      const int32_t *subRuns, double kernelMs) {
    int64_t g = 0;
    for (int64_t k = 0; k < top->n; k++) {
        const int64_t i = top->owner[k];
        const CpkAnchorProblem *t = &top->probs[k];
        int64_t total = t->nRuns, m = 0;
        for (int64_t h = g; h < sub->n && sub->owner[h] == k; h++) total += sub->probs[h].nRuns;
        int64_t *out = malloc(sizeof *out * 4 * (size_t)(total ? total : 1));
        if (!out) return CPECAN_ENOMEM;
        c->runs[i] = out;
        cpecan_anchor_stats st = {.hits = t->hits, .hsps = t->hsps, .chained = t->chained, .capped = t->capped};
        GapWalk w = {.r3 = topRuns + 3 * t->hspOff, .n = t->nRuns, .lX = t->lX, .lY = t->lY, .j = -1};
        while (gap_next(&w)) {
            if (g < sub->n && sub->owner[g] == k && sub->before[g] == w.j) {
                const CpkAnchorProblem *s = &sub->probs[g++];
                const int32_t *r = subRuns + 3 * s->hspOff;
                for (int64_t u = 0; u < s->nRuns; u++) m = put_run(out, m, w.pX + r[3 * u], w.pY + r[3 * u + 1], r[3 * u + 2], c->expansion);
                st.hits += s->hits;
                st.hsps += s->hsps;
                st.chained += s->chained;
                st.capped |= s->capped;
                st.subProblems++;
            }
            if (w.j < t->nRuns) m = put_run(out, m, w.x, w.y, w.len, c->expansion);
        }
        c->nRuns[i] = st.runs = m;
        w = (GapWalk){.r4 = out, .n = m, .lX = t->lX, .lY = t->lY, .j = -1};
        while (gap_next(&w)) {
            st.largestGap = max64(st.largestGap, gap_matrix(&w));
            st.anchorColumns += w.len;
        }
        if (c->stats) {
            st.largestGapTop = c->stats[i].largestGapTop;
            c->stats[i] = st;
        }
    }
    for (int64_t i = 0; c->stats && i < c->n; i++) c->stats[i].kernelMs = kernelMs;
    return CPECAN_OK;
}

/* Step 5b on every problem of a list, with the options' values or what their zeros stand for; the options passed the check. */
static void mark_gapped(CpkAnchorList *l, const cpecan_anchor_options *o) {
    if (!o || !o->gappedExtension) return;
    const int32_t diags = o->gappedMaxDiagonals ? o->gappedMaxDiagonals : CPK_ANCHOR_GAPPED_MAX_DIAGS;
    for (int64_t k = 0; k < l->n; k++) {
        l->probs[k].flags |= CPK_ANCHOR_GAPPED | (diags << CPK_ANCHOR_DIAGS_SHIFT);
        l->probs[k].yDrop = o->yDrop ? o->yDrop : CPK_ANCHOR_GAPPED_Y_DROP;
    }
}

/* The finder behind every entry point: check, device, layout, open, pass, pick, gaps, pass, splice, close. */
static int find_runs(const CpkAnchorCall *c, int64_t trim, const cpecan_anchor_params *params, const cpecan_anchor_options *options) {
    CpkAnchorPass pass;
    CpkAnchorList top = {0}, sub = {0};
    CpkAnchorCtx *ctx = NULL;
    uint8_t *bytes = NULL;
    int32_t *topRuns = NULL, *subRuns = NULL;
    int64_t nBytes = 0, nExtra = 0;
    double ms = 0.0;
    int rc = cpk_anchor_check(c, trim, params, options, &pass);
    if (rc != CPECAN_OK) return rc;
    const int nDev = cpk_device_count();
    if (nDev <= 0 || c->device < 0 || c->device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, c->device);
        return CPECAN_ENODEVICE;
    }
    if ((rc = cpk_anchor_layout(c, &top, &bytes, &nBytes, &nExtra)) != CPECAN_OK || top.n == 0) goto done;
    if ((rc = cpk_anchor_open(&ctx, c->device, bytes, nBytes, nExtra)) != CPECAN_OK) goto done;
    mark_gapped(&top, options);
    if ((rc = cpk_anchor_pass(ctx, &pass, top.probs, top.n, &topRuns, &ms)) != CPECAN_OK) goto done;
    cpk_anchor_pick(c, &top);
    if ((rc = cpk_anchor_gaps(c, &top, topRuns, &sub)) != CPECAN_OK) goto done;
    mark_gapped(&sub, options);
    if ((rc = cpk_anchor_pass(ctx, &pass, sub.probs, sub.n, &subRuns, &ms)) != CPECAN_OK) goto done;
    rc = cpk_anchor_splice(c, &top, topRuns, &sub, subRuns, ms);
done:
    if (rc == CPECAN_ENOMEM) cpk_set_error("%s: out of memory", c->who);
    for (int64_t i = 0; rc != CPECAN_OK && i < c->n; i++) {
        free(c->runs[i]);
        c->runs[i] = NULL;
        c->nRuns[i] = 0;
    }
    cpk_anchor_close(ctx);
    cpk_anchor_list_free(&top);
    cpk_anchor_list_free(&sub);
    free(bytes);
    free(topRuns);
    free(subRuns);
    return rc;
}

int cpecan_find_anchor_runs_many_with_options(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                              int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                                              const cpecan_anchor_params *params, int device, int strandMode, int64_t **runs,
                                              int64_t *nRuns, cpecan_anchor_stats *stats, cpecan_strand_result *strands,
                                              const cpecan_anchor_options *options) {
    const CpkAnchorCall c = {"cpecan_find_anchor_runs_many_with_options", problems, n, expansion, anchorMatrixBiggerThanThis,
                             repeatMaskMatrixBiggerThanThis, device, strandMode, 0, 1, runs, nRuns, stats, strands};
    return find_runs(&c, trim, params, options);
}

int cpecan_find_anchor_runs_many_stranded(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                          int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                                          const cpecan_anchor_params *params, int device, int strandMode, int64_t **runs,
                                          int64_t *nRuns, cpecan_anchor_stats *stats, cpecan_strand_result *strands) {
    return cpecan_find_anchor_runs_many_with_options(problems, n, trim, expansion, anchorMatrixBiggerThanThis,
                                                     repeatMaskMatrixBiggerThanThis, params, device, strandMode, runs, nRuns, stats,
                                                     strands, NULL);
}

int cpecan_find_anchor_runs_many(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                 int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                                 const cpecan_anchor_params *params, int device, int64_t **runs, int64_t *nRuns,
                                 cpecan_anchor_stats *stats) {
    return cpecan_find_anchor_runs_many_with_options(problems, n, trim, expansion, anchorMatrixBiggerThanThis,
                                                     repeatMaskMatrixBiggerThanThis, params, device, CPECAN_STRAND_PLUS, runs, nRuns,
                                                     stats, NULL, NULL);
}

int cpecan_find_anchor_runs(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim, int64_t expansion,
                            int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                            const cpecan_anchor_params *params, int64_t **runs, int64_t *nRuns, cpecan_anchor_stats *stats) {
    if (!runs || !nRuns) return CPECAN_EINVAL;
    const cpecan_anchor_problem q = {sX, lX, sY, lY};
    return cpecan_find_anchor_runs_many(&q, 1, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params,
                                        cpk_current_device(), runs, nRuns, stats);
}

/* Steps 1-5 alone are a mode of the call record the arguments of the entry point above cannot ask for, so this one has a twin. */
int cpecan_find_anchor_runs_once_with_options(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim,
                                              int64_t expansion, int softMask, const cpecan_anchor_params *params,
                                              int64_t **runs, int64_t *nRuns, const cpecan_anchor_options *options) {
    if (!runs || !nRuns) {
        cpk_set_error("cpecan_find_anchor_runs_once: bad arguments");
        return CPECAN_EINVAL;
    }
    const cpecan_anchor_problem q = {sX, lX, sY, lY};
    const CpkAnchorCall c = {"cpecan_find_anchor_runs_once", &q, 1, expansion, 0, 0, cpk_current_device(), CPECAN_STRAND_PLUS,
                             1, softMask, runs, nRuns, NULL, NULL};
    return find_runs(&c, trim, params, options);
}

int cpecan_find_anchor_runs_once(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim, int64_t expansion,
                                 int softMask, const cpecan_anchor_params *params, int64_t **runs, int64_t *nRuns) {
    return cpecan_find_anchor_runs_once_with_options(sX, lX, sY, lY, trim, expansion, softMask, params, runs, nRuns, NULL);
}
