/*
 * cpecan_anchor.c -- host side of the anchor finder (include/cpecan_hip.h: cpecan_find_anchor_runs_many).
 * The kernels (cpk_anchor.inl) do steps 1-5 on a list of problems; this file lays the sequences of a call out in one
 * buffer, runs the top-level pass, makes the second pass's problems out of the gaps between the top-level anchors
 * (getBlastPairsForPairwiseAlignmentParameters, impl/pairwiseAligner.c:1175-1191) and splices the runs together.
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
    return CPECAN_OK;
}

typedef struct {
    int64_t problem; /* index of the top-level problem this gap belongs to */
    int64_t pX, pY;  /* offset of the gap inside it */
} Gap;

static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

int cpecan_find_anchor_runs_many(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                 int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                                 const cpecan_anchor_params *params, int device, int64_t **runs, int64_t *nRuns,
                                 cpecan_anchor_stats *stats) {
    if (n < 0 || (n > 0 && (!problems || !runs || !nRuns)) || trim < 0 || trim > (1 << 24)) {
        cpk_set_error("cpecan_find_anchor_runs_many: bad arguments");
        return CPECAN_EINVAL;
    }
    cpecan_anchor_params def;
    if (!params) {
        cpecan_anchor_params_default(&def);
        params = &def;
    }
    if (memchr(params->seed, 0, sizeof params->seed) == NULL) {
        cpk_set_error("cpecan_find_anchor_runs_many: the seed is not terminated");
        return CPECAN_EINVAL;
    }
    for (int64_t i = 0; i < n; i++) {
        runs[i] = NULL;
        nRuns[i] = 0;
    }
    for (int64_t i = 0; i < n; i++)
        if (problems[i].lX < 0 || problems[i].lY < 0 || (problems[i].lX > 0 && !problems[i].sX) ||
            (problems[i].lY > 0 && !problems[i].sY) || problems[i].lX > (1 << 24) || problems[i].lY > (1 << 24)) {
            cpk_set_error("cpecan_find_anchor_runs_many: problem %lld has no sequence or one longer than 2^24", (long long)i);
            return CPECAN_EINVAL;
        }
    if (stats) memset(stats, 0, sizeof *stats * (size_t)n);
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

    /* the problems beyond the size limit, their sequences end to end in one buffer */
    int rc = CPECAN_ENOMEM;
    int64_t nTop = 0, nBytes = 0, nGaps = 0, capGaps = 0, g = 0;
    double ms = 0.0;
    CpkAnchorCtx *ctx = NULL;
    CpkAnchorProblem *top = malloc(sizeof *top * (size_t)(n ? n : 1)), *sub = NULL;
    int64_t *owner = malloc(sizeof *owner * (size_t)(n ? n : 1));
    uint8_t *bytes = NULL;
    int32_t *topRuns = NULL, *subRuns = NULL;
    Gap *gaps = NULL;
    if (!top || !owner) goto done;
    for (int64_t i = 0; i < n; i++) {
        const cpecan_anchor_problem *q = &problems[i];
        if (stats) stats[i].largestGapTop = stats[i].largestGap = q->lX * q->lY;
        if (q->lX * q->lY <= anchorMatrixBiggerThanThis || q->lX == 0 || q->lY == 0) continue;
        CpkAnchorProblem *t = &top[nTop];
        memset(t, 0, sizeof *t);
        t->xOff = nBytes;
        t->yOff = nBytes + q->lX;
        t->lX = (int32_t)q->lX;
        t->lY = (int32_t)q->lY;
        t->softMask = 1; /* :1168 */
        owner[nTop++] = i;
        nBytes += q->lX + q->lY;
    }
    if (nTop == 0) {
        rc = CPECAN_OK;
        goto done;
    }
    bytes = malloc((size_t)nBytes);
    if (!bytes) goto done;
    for (int64_t k = 0; k < nTop; k++) {
        const cpecan_anchor_problem *q = &problems[owner[k]];
        memcpy(bytes + top[k].xOff, q->sX, (size_t)q->lX);
        memcpy(bytes + top[k].yOff, q->sY, (size_t)q->lY);
    }
    if ((rc = cpk_anchor_open(&ctx, device, bytes, nBytes)) != CPECAN_OK) goto done;
    if ((rc = cpk_anchor_pass(ctx, &prm, params->seed, top, nTop, (int32_t)trim, &topRuns, &ms)) != CPECAN_OK) goto done;

    /* the gaps between consecutive top-level anchors that are still too large: the second pass (:1175-1191) */
    rc = CPECAN_ENOMEM;
    for (int64_t k = 0; k < nTop; k++) {
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
    if ((rc = cpk_anchor_pass(ctx, &prm, params->seed, sub, nGaps, (int32_t)trim, &subRuns, &ms)) != CPECAN_OK) goto done;

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
    if (rc == CPECAN_ENOMEM) cpk_set_error("cpecan_find_anchor_runs_many: out of memory");
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

int cpecan_find_anchor_runs(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim, int64_t expansion,
                            int64_t anchorMatrixBiggerThanThis, int64_t repeatMaskMatrixBiggerThanThis,
                            const cpecan_anchor_params *params, int64_t **runs, int64_t *nRuns, cpecan_anchor_stats *stats) {
    if (!runs || !nRuns) return CPECAN_EINVAL;
    const cpecan_anchor_problem q = {sX, lX, sY, lY};
    return cpecan_find_anchor_runs_many(&q, 1, trim, expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis, params,
                                        cpk_current_device(), runs, nRuns, stats);
}

int cpecan_find_anchor_runs_once(const char *sX, int64_t lX, const char *sY, int64_t lY, int64_t trim, int64_t expansion,
                                 int softMask, const cpecan_anchor_params *params, int64_t **runs, int64_t *nRuns) {
    if (!runs || !nRuns || lX < 0 || lY < 0 || (lX > 0 && !sX) || (lY > 0 && !sY) || lX > (1 << 24) || lY > (1 << 24) || trim < 0 ||
        trim > (1 << 24)) {
        cpk_set_error("cpecan_find_anchor_runs_once: bad arguments");
        return CPECAN_EINVAL;
    }
    *runs = NULL;
    *nRuns = 0;
    cpecan_anchor_params def;
    if (!params) {
        cpecan_anchor_params_default(&def);
        params = &def;
    }
    if (memchr(params->seed, 0, sizeof params->seed) == NULL) {
        cpk_set_error("cpecan_find_anchor_runs_once: the seed is not terminated");
        return CPECAN_EINVAL;
    }
    if (cpk_device_count() <= 0) {
        cpk_set_error("no usable HIP device: the HIP path has no CPU fallback");
        return CPECAN_ENODEVICE;
    }
    if (lX == 0 || lY == 0) return CPECAN_OK; /* :1012 */
    CpkAnchorParams prm;
    memcpy(prm.scores, params->scores, sizeof prm.scores);
    prm.maxSeedOccurrences = params->maxSeedOccurrences;
    prm.xDrop = params->xDrop;
    prm.hspThreshold = params->hspThreshold;
    prm.maxHsps = params->maxHsps;
    uint8_t *bytes = malloc((size_t)(lX + lY));
    if (!bytes) {
        cpk_set_error("cpecan_find_anchor_runs_once: out of memory");
        return CPECAN_ENOMEM;
    }
    memcpy(bytes, sX, (size_t)lX);
    memcpy(bytes + lX, sY, (size_t)lY);
    CpkAnchorProblem t;
    memset(&t, 0, sizeof t);
    t.yOff = lX;
    t.lX = (int32_t)lX;
    t.lY = (int32_t)lY;
    t.softMask = softMask != 0;
    CpkAnchorCtx *ctx = NULL;
    int32_t *found = NULL;
    double ms = 0.0;
    int rc = cpk_anchor_open(&ctx, cpk_current_device(), bytes, lX + lY);
    if (rc == CPECAN_OK) rc = cpk_anchor_pass(ctx, &prm, params->seed, &t, 1, (int32_t)trim, &found, &ms);
    if (rc == CPECAN_OK) {
        int64_t *out = malloc(sizeof *out * 4 * (size_t)(t.nRuns ? t.nRuns : 1));
        if (!out) {
            cpk_set_error("cpecan_find_anchor_runs_once: out of memory");
            rc = CPECAN_ENOMEM;
        } else {
            for (int64_t j = 0; j < t.nRuns; j++) {
                for (int f = 0; f < 3; f++) out[4 * j + f] = found[3 * (t.hspOff + j) + f];
                out[4 * j + 3] = expansion;
            }
            *runs = out;
            *nRuns = t.nRuns;
        }
    }
    cpk_anchor_close(ctx);
    free(found);
    free(bytes);
    return rc;
}
