/*
 * cpecan_anchor.c -- host side of the anchor finder (include/cpecan_hip.h: cpecan_find_anchor_runs_many_stranded).
 * The kernels (cpk_anchor.inl) do steps 1-5 on a list of problems; this file lays the sequences of a call out in one
 * buffer, runs the top-level pass, makes the second pass's problems out of the gaps between the top-level anchors
 * (getBlastPairsForPairwiseAlignmentParameters, impl/pairwiseAligner.c:1175-1191) and splices the runs together.
 * Strand: a problem that may lie on the minus strand gets a twin in the top-level pass whose
 * Y is the reverse complement, written on the device behind the forward symbols; the chain scores of the two decide, and
 * only the chosen orientation goes on to the gaps and the splice.
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

typedef struct {
    int64_t problem; /* index of the top-level problem this gap belongs to */
    int64_t pX, pY;  /* offset of the gap inside it */
} Gap;

static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

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

/* The finder behind every entry point.  once: steps 1-5 alone on every problem whatever its size, soft masking as
 * softMaskTop says, no recursion (cpecan_find_anchor_runs_once); otherwise the top level masks (:1168).  who: the entry
 * point, for the error texts. */
static int find_runs(const char *who, const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                     int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis, const cpecan_anchor_params *params,
                     int device, int strandMode, int once, int softMaskTop, int64_t **runs, int64_t *nRuns, cpecan_anchor_stats *stats,
                     cpecan_strand_result *strands, const cpecan_anchor_options *options) {
    if (n < 0 || (n > 0 && (!problems || !runs || !nRuns)) || trim < 0 || trim > (1 << 24) || strandMode < CPECAN_STRAND_PLUS ||
        strandMode > CPECAN_STRAND_BOTH) {
        cpk_set_error("%s: bad arguments", who);
        return CPECAN_EINVAL;
    }
    cpecan_anchor_params def;
    if (!params) {
        cpecan_anchor_params_default(&def);
        params = &def;
    }
    if (memchr(params->seed, 0, sizeof params->seed) == NULL) {
        cpk_set_error("%s: the seed is not terminated", who);
        return CPECAN_EINVAL;
    }
    if (params->seedTransitions != 0 && params->seedTransitions != 1) {
        cpk_set_error("%s: seedTransitions is 0 or 1", who);
        return CPECAN_EINVAL;
    }
    /* step 2's threshold for an HSP that only variant hits extend to; hspThreshold says: no class is told from the other */
    int32_t variantThreshold = params->hspThreshold;
    if (options) {
        for (int k = 0; k < 7; k++)
            if (options->reserved[k] != 0) {
                cpk_set_error("%s: a reserved word of the options is not 0", who);
                return CPECAN_EINVAL;
            }
        if (options->transitionHspThreshold < 0 ||
            (options->transitionHspThreshold != 0 && options->transitionHspThreshold < params->hspThreshold)) {
            cpk_set_error("%s: transitionHspThreshold is 0 or at least hspThreshold", who);
            return CPECAN_EINVAL;
        }
        if (options->transitionHspThreshold != 0) variantThreshold = options->transitionHspThreshold;
    }
    for (int64_t i = 0; i < n; i++) {
        runs[i] = NULL;
        nRuns[i] = 0;
    }
    for (int64_t i = 0; i < n; i++)
        if (problems[i].lX < 0 || problems[i].lY < 0 || (problems[i].lX > 0 && !problems[i].sX) ||
            (problems[i].lY > 0 && !problems[i].sY) || problems[i].lX > (1 << 24) || problems[i].lY > (1 << 24)) {
            cpk_set_error("%s: problem %lld has no sequence or one longer than 2^24", who, (long long)i);
            return CPECAN_EINVAL;
        }
    if (stats) memset(stats, 0, sizeof *stats * (size_t)n);
    for (int64_t i = 0; strands && i < n; i++) { /* what holds without a pass: forced, or plus; nothing scored */
        strands[i].strand = strandMode == CPECAN_STRAND_MINUS ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
        strands[i].scorePlus = strands[i].scoreMinus = -1;
    }
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    CpkAnchorParams prm;
    memcpy(prm.scores, params->scores, sizeof prm.scores);
    prm.maxSeedOccurrences = params->maxSeedOccurrences;
    prm.xDrop = params->xDrop;
    prm.hspThreshold = params->hspThreshold;
    prm.maxHsps = params->maxHsps;

    /* The top-level problems, their sequences end to end in one buffer: those beyond the size limit and, with BOTH, the
     * others too, for their strand score.  A problem scored on both strands is a pair of twins, plus then minus; the
     * reverse complements get even offsets in an area behind the sequences. */
    const int both = strandMode == CPECAN_STRAND_BOTH, twins = both ? 2 : 1;
    int rc = CPECAN_ENOMEM;
    int64_t nTop = 0, nBytes = 0, nExtra = 0, nGaps = 0, capGaps = 0, g = 0;
    double ms = 0.0;
    CpkAnchorCtx *ctx = NULL;
    CpkAnchorProblem *top = malloc(sizeof *top * (size_t)(n ? twins * n : 1)), *sub = NULL;
    int64_t *owner = malloc(sizeof *owner * (size_t)(n ? twins * n : 1));
    uint8_t *bytes = NULL;
    int32_t *topRuns = NULL, *subRuns = NULL;
    Gap *gaps = NULL;
    if (!top || !owner) goto done;
    for (int64_t i = 0; i < n; i++) {
        const cpecan_anchor_problem *q = &problems[i];
        if (stats) stats[i].largestGapTop = stats[i].largestGap = q->lX * q->lY;
        if (q->lX == 0 || q->lY == 0) { /* :1012; no HSP on either strand */
            if (strands && both) strands[i].scorePlus = strands[i].scoreMinus = 0;
            continue;
        }
        if (!once && !both && q->lX * q->lY <= anchorMatrixBiggerThanThis) continue;
        for (int t = 0; t < twins; t++) {
            const int minus = both ? t : strandMode == CPECAN_STRAND_MINUS;
            CpkAnchorProblem *p = &top[nTop];
            memset(p, 0, sizeof *p);
            p->xOff = nBytes;
            p->yOff = nBytes + q->lX;
            p->lX = (int32_t)q->lX;
            p->lY = (int32_t)q->lY;
            p->softMask = once ? softMaskTop != 0 : 1; /* :1168 */
            if (minus) {
                p->flags = CPK_ANCHOR_RC_Y | (t ? CPK_ANCHOR_SHARE_X : 0);
                p->yFwd = p->yOff;
                p->yOff = -1 - nExtra; /* its place in the area, known once nBytes is */
                nExtra += (q->lY + 1) & ~(int64_t)1;
            }
            owner[nTop++] = i;
        }
        nBytes += q->lX + q->lY;
    }
    if (nTop == 0) {
        rc = CPECAN_OK;
        goto done;
    }
    for (int64_t k = 0; k < nTop; k++)
        if (top[k].flags & CPK_ANCHOR_RC_Y) top[k].yOff = ((nBytes + 1) & ~(int64_t)1) + (-1 - top[k].yOff);
    bytes = malloc((size_t)nBytes);
    if (!bytes) goto done;
    for (int64_t k = 0; k < nTop; k++) {
        if (top[k].flags & CPK_ANCHOR_SHARE_X) continue;
        const cpecan_anchor_problem *q = &problems[owner[k]];
        memcpy(bytes + top[k].xOff, q->sX, (size_t)q->lX);
        memcpy(bytes + top[k].xOff + q->lX, q->sY, (size_t)q->lY);
    }
    if ((rc = cpk_anchor_open(&ctx, device, bytes, nBytes, nExtra)) != CPECAN_OK) goto done;
    if ((rc = cpk_anchor_pass(ctx, &prm, params->seed, params->seedTransitions, variantThreshold, top, nTop, (int32_t)trim, &topRuns, &ms)) != CPECAN_OK) goto done;

    /* The strand of every problem; what does not go on is dropped from the list: the twin that lost and, with BOTH, the
     * problems at or under the size limit, which were there to be scored. */
    {
        int64_t kept = 0;
        for (int64_t k = 0; k < nTop; k += twins) {
            const int64_t i = owner[k];
            int64_t pick = k;
            if (both) {
                const int minus = top[k + 1].score > top[k].score; /* a tie, 0 = 0 included, is plus */
                pick = k + minus;
                if (strands) {
                    strands[i].strand = minus ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS;
                    strands[i].scorePlus = top[k].score;
                    strands[i].scoreMinus = top[k + 1].score;
                }
            } else if (strands) {
                *(strandMode == CPECAN_STRAND_MINUS ? &strands[i].scoreMinus : &strands[i].scorePlus) = top[k].score;
            }
            if (!once && problems[i].lX * problems[i].lY <= anchorMatrixBiggerThanThis) continue;
            top[kept] = top[pick];
            owner[kept++] = i;
        }
        nTop = kept;
    }

    /* the gaps between consecutive top-level anchors that are still too large: the second pass (:1175-1191) */
    rc = CPECAN_ENOMEM;
    for (int64_t k = 0; k < nTop && !once; k++) {
        const int32_t *r = topRuns + 3 * top[k].hspOff;
        int64_t pX = 0, pY = 0, largest = 0;
        for (int64_t j = 0; j <= top[k].nRuns; j++) {
            const int64_t x = j < top[k].nRuns ? r[3 * j] : top[k].lX, y = j < top[k].nRuns ? r[3 * j + 1] : top[k].lY;
            const int64_t matrix = (x - pX) * (y - pY);
            largest = max64(largest, matrix);
            if (matrix > anchorMatrixBiggerThanThis) {
                if (nGaps == capGaps) {
                    capGaps = capGaps ? 2 * capGaps : 64;
                    Gap *gNew = realloc(gaps, sizeof *gNew * (size_t)capGaps);
                    if (gNew) gaps = gNew;
                    CpkAnchorProblem *sNew = realloc(sub, sizeof *sNew * (size_t)capGaps);
                    if (sNew) sub = sNew;
                    if (!gNew || !sNew) goto done;
                }
                CpkAnchorProblem *s = &sub[nGaps];
                memset(s, 0, sizeof *s);
                s->xOff = top[k].xOff + pX;
                s->yOff = top[k].yOff + pY;
                s->lX = (int32_t)(x - pX);
                s->lY = (int32_t)(y - pY);
                s->softMask = matrix > repeatMaskMatrixBiggerThanThis;
                gaps[nGaps].problem = k;
                gaps[nGaps].pX = pX;
                gaps[nGaps].pY = pY;
                nGaps++;
            }
            if (j < top[k].nRuns) {
                pX = x + r[3 * j + 2];
                pY = y + r[3 * j + 2];
            }
        }
        if (stats) stats[owner[k]].largestGapTop = largest;
    }
    if ((rc = cpk_anchor_pass(ctx, &prm, params->seed, params->seedTransitions, variantThreshold, sub, nGaps, (int32_t)trim, &subRuns, &ms)) != CPECAN_OK) goto done;

    /* splice: the gaps of a problem are in increasing order, each in front of the top-level run it ends at */
    rc = CPECAN_ENOMEM;
    for (int64_t k = 0; k < nTop; k++) {
        const int64_t i = owner[k];
        int64_t total = top[k].nRuns;
        for (int64_t h = g; h < nGaps && gaps[h].problem == k; h++) total += sub[h].nRuns;
        int64_t *out = malloc(sizeof *out * 4 * (size_t)(total ? total : 1));
        if (!out) goto done;
        runs[i] = out;
        const int32_t *r = topRuns + 3 * top[k].hspOff;
        cpecan_anchor_stats st;
        memset(&st, 0, sizeof st);
        st.hits = top[k].hits;
        st.hsps = top[k].hsps;
        st.chained = top[k].chained;
        st.capped = top[k].capped;
        int64_t m = 0, pX = 0, pY = 0;
        for (int64_t j = 0; j <= top[k].nRuns; j++) {
            const int64_t x = j < top[k].nRuns ? r[3 * j] : top[k].lX, y = j < top[k].nRuns ? r[3 * j + 1] : top[k].lY;
            if (g < nGaps && gaps[g].problem == k && gaps[g].pX == pX && gaps[g].pY == pY &&
                (x - pX) * (y - pY) > anchorMatrixBiggerThanThis) {
                const int32_t *s = subRuns + 3 * sub[g].hspOff;
                for (int64_t u = 0; u < sub[g].nRuns; u++, m++) {
                    out[4 * m] = pX + s[3 * u];
                    out[4 * m + 1] = pY + s[3 * u + 1];
                    out[4 * m + 2] = s[3 * u + 2];
                    out[4 * m + 3] = expansion;
                }
                st.hits += sub[g].hits;
                st.hsps += sub[g].hsps;
                st.chained += sub[g].chained;
                st.capped |= sub[g].capped;
                st.subProblems++;
                g++;
            }
            if (j < top[k].nRuns) {
                out[4 * m] = x;
                out[4 * m + 1] = y;
                out[4 * m + 2] = r[3 * j + 2];
                out[4 * m + 3] = expansion;
                m++;
                pX = x + r[3 * j + 2];
                pY = y + r[3 * j + 2];
            }
        }
        nRuns[i] = m;
        pX = pY = 0;
        for (int64_t j = 0; j <= m; j++) {
            const int64_t x = j < m ? out[4 * j] : top[k].lX, y = j < m ? out[4 * j + 1] : top[k].lY;
            st.largestGap = max64(st.largestGap, (x - pX) * (y - pY));
            if (j < m) {
                st.anchorColumns += out[4 * j + 2];
                pX = x + out[4 * j + 2];
                pY = y + out[4 * j + 2];
            }
        }
        st.runs = m;
        if (stats) {
            st.largestGapTop = stats[i].largestGapTop;
            stats[i] = st;
        }
    }
    if (stats)
        for (int64_t i = 0; i < n; i++) stats[i].kernelMs = ms;
    rc = CPECAN_OK;
done:
    if (rc == CPECAN_ENOMEM) cpk_set_error("%s: out of memory", who);
    if (rc != CPECAN_OK)
        for (int64_t i = 0; i < n; i++) {
            free(runs[i]);
            runs[i] = NULL;
            nRuns[i] = 0;
        }
    cpk_anchor_close(ctx);
    free(top);
    free(sub);
    free(owner);
    free(bytes);
    free(topRuns);
    free(subRuns);
    free(gaps);
    return rc;
}

int cpecan_find_anchor_runs_many_with_options(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                              int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                                              const cpecan_anchor_params *params, int device, int strandMode, int64_t **runs,
                                              int64_t *nRuns, cpecan_anchor_stats *stats, cpecan_strand_result *strands,
                                              const cpecan_anchor_options *options) {
    return find_runs("cpecan_find_anchor_runs_many_with_options", problems, n, trim, expansion, anchorMatrixBiggerThanThis,
                     repeatMaskMatrixBiggerThanThis, params, device, strandMode, 0, 1, runs, nRuns, stats, strands, options);
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

/* Steps 1-5 alone are a mode of find_runs the arguments of the entry point above cannot ask for, so this one has a twin. */
int cpecan_find_anchor_runs_once_with_options(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim,
                                              int64_t expansion, int softMask, const cpecan_anchor_params *params,
                                              int64_t **runs, int64_t *nRuns, const cpecan_anchor_options *options) {
    if (!runs || !nRuns) {
        cpk_set_error("cpecan_find_anchor_runs_once: bad arguments");
        return CPECAN_EINVAL;
    }
    const cpecan_anchor_problem q = {sX, lX, sY, lY};
    return find_runs("cpecan_find_anchor_runs_once", &q, 1, trim, expansion, 0, 0, params, cpk_current_device(), CPECAN_STRAND_PLUS,
                     1, softMask, runs, nRuns, NULL, NULL, options);
}

int cpecan_find_anchor_runs_once(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim, int64_t expansion,
                                 int softMask, const cpecan_anchor_params *params, int64_t **runs, int64_t *nRuns) {
    return cpecan_find_anchor_runs_once_with_options(sX, lX, sY, lY, trim, expansion, softMask, params, runs, nRuns, NULL);
}
