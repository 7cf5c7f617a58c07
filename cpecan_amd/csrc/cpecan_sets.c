/*
 * cpecan_sets.c -- sets of sequence fragments over the anchor batch and the DP batch (include/cpecan_sets.h).
 *
 * Host code only: the fragments, the choice of pairs (impl/multipleAligner.c:668-681, :722-770), the checks and the order
 * of the two batches.  The alignments, the reweighting and the (score, seq1, pos1, seq2, pos2) records are the GPU's
 * (cpecan_batch_set_quintuples); what remains here per call is a loop over the pairs, never one over their records.
 */
#define _POSIX_C_SOURCE 200809L
#include "cpecan_sets.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cpecan_internal.h"

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

typedef struct {
    char *seq;
    int64_t length, set, leftEndId, rightEndId;
} Fragment;

struct cpecan_sets {
    cpecan_model model;
    cpecan_params params;
    cpecan_sets_options options;
    int device;
    Fragment *frags;
    int64_t n, cap;
};

struct cpecan_sets_result {
    int64_t nPairs;
    int32_t *quints;   /* host pool (cpk_host_free) */
    int64_t *offsets;  /* nPairs + 1 */
    int64_t *similarity;
    cpecan_sets_timing timing;
};

int cpecan_sets_options_default(cpecan_sets_options *o) {
    if (!o) return CPECAN_EINVAL;
    memset(o, 0, sizeof *o);
    o->gapGamma = 0.5f;                          /* pairwiseAligner.c:1345 */
    o->constraintDiagonalTrim = 14;              /* :1340 */
    o->anchorMatrixBiggerThanThis = 500 * 500;   /* :1341 */
    o->repeatMaskMatrixBiggerThanThis = 500 * 500; /* :1342 */
    return CPECAN_OK;
}

int64_t cpecan_similarity_score(int64_t scoreSum, int64_t lX, int64_t lY) {
    if (lX < 0 || lY < 0) return CPECAN_EINVAL;
    int64_t j = lX < lY ? lX : lY;
    j = j == 0 ? 1 : j;
    double d = (double)scoreSum / (double)(j * CPECAN_PROB_1);
    d = d > 1.0 ? 1.0 : d;
    d = d < 0.0 ? 0.0 : d;
    return (int64_t)(d * CPECAN_PROB_1);
}

int cpecan_sets_create(cpecan_sets **out, const cpecan_model *model, const cpecan_params *params,
                       const cpecan_sets_options *options, int device) {
    if (!out || !model || device < 0) return CPECAN_EINVAL;
    if (options && (options->constraintDiagonalTrim < 0 || options->anchorMatrixBiggerThanThis < 0 ||
                    options->repeatMaskMatrixBiggerThanThis < 0 || options->gapGamma != options->gapGamma))
        return CPECAN_EINVAL;
    cpecan_sets *s = calloc(1, sizeof *s);
    if (!s) return CPECAN_ENOMEM;
    s->model = *model;
    if (params) s->params = *params;
    else cpecan_params_default(&s->params);
    if (options) s->options = *options;
    else cpecan_sets_options_default(&s->options);
    s->device = device;
    *out = s;
    return CPECAN_OK;
}

void cpecan_sets_destroy(cpecan_sets *s) {
    if (!s) return;
    for (int64_t i = 0; i < s->n; i++) free(s->frags[i].seq);
    free(s->frags);
    free(s);
}

int64_t cpecan_sets_add_fragment(cpecan_sets *s, int64_t set, const char *seq, int64_t length, int64_t leftEndId,
                                 int64_t rightEndId) {
    if (!s || length < 0 || (length > 0 && !seq) || length > INT32_MAX) return CPECAN_EINVAL;
    if (s->n >= INT32_MAX) { /* the records name a fragment in 32 bits */
        cpk_set_error("cpecan_sets_add_fragment: more than 2^31 - 1 fragments");
        return CPECAN_EINVAL;
    }
    if (s->n == s->cap) {
        const int64_t cap = s->cap ? 2 * s->cap : 64;
        Fragment *g = realloc(s->frags, sizeof *g * (size_t)cap);
        if (!g) return CPECAN_ENOMEM;
        s->frags = g;
        s->cap = cap;
    }
    Fragment *f = &s->frags[s->n];
    f->seq = malloc((size_t)length + 1);
    if (!f->seq) return CPECAN_ENOMEM;
    if (length) memcpy(f->seq, seq, (size_t)length);
    f->seq[length] = 0;
    f->length = length;
    f->set = set;
    f->leftEndId = leftEndId;
    f->rightEndId = rightEndId;
    return s->n++;
}

/* ---- the choice of pairs ---- */
static int by_pair(const void *a, const void *b) {
    const int64_t *p = a, *q = b;
    if (p[0] != q[0]) return p[0] < q[0] ? -1 : 1;
    return p[1] < q[1] ? -1 : p[1] > q[1];
}
static int by_triple(const void *a, const void *b) { /* stIntTuple_cmpFn on (rightEndId, length, index), :748-750 */
    const int64_t *p = a, *q = b;
    if (p[0] != q[0]) return p[0] < q[0] ? -1 : 1;
    return by_pair(p + 1, q + 1);
}

typedef struct {
    int64_t *pairs, cap, n;
} PairSink;
static void emit(PairSink *k, int64_t a, int64_t b) {
    if (k->n < k->cap) {
        k->pairs[2 * k->n] = a;
        k->pairs[2 * k->n + 1] = b;
    }
    k->n++;
}

/* getReferencePairwiseAlignmentsP (:722-733) on tuples (rightEndId, length, index): the one at (i + j) / 2 of l[i .. j) pairs
 * with every other one, as (min, max); returns it */
static const int64_t *star(const int64_t *l, int64_t i, int64_t j, int64_t *out, int64_t *nOut) {
    const int64_t *ref = l + 3 * ((i + j) / 2);
    const int64_t k = ref[2];
    for (; i < j; i++) {
        const int64_t m = l[3 * i + 2];
        if (m != k) {
            out[2 * *nOut] = k < m ? k : m;
            out[2 * *nOut + 1] = k < m ? m : k;
            (*nOut)++;
        }
    }
    return ref;
}

int64_t cpecan_sets_pairs(const cpecan_sets *s, int mode, int64_t *pairs, int64_t cap) {
    if (!s || (mode != CPECAN_SETS_ALL && mode != CPECAN_SETS_REFERENCE) || cap < 0 || (cap > 0 && !pairs)) return CPECAN_EINVAL;
    const int64_t n = s->n;
    if (n == 0) return 0;
    int64_t *order = malloc(sizeof(int64_t) * 2 * (size_t)n);  /* (set, index), sorted: the members of a set, ascending */
    int64_t *groups = malloc(sizeof(int64_t) * 3 * (size_t)n); /* (first member, start in order, count), by first member */
    int64_t *l = malloc(sizeof(int64_t) * 6 * (size_t)n);      /* one set's tuples, sorted; then the runs' references */
    int64_t *chosen = malloc(sizeof(int64_t) * 2 * (size_t)n); /* one set's n - 1 reference pairs */
    if (!order || !groups || !l || !chosen) {
        free(order);
        free(groups);
        free(l);
        free(chosen);
        return CPECAN_ENOMEM;
    }
    for (int64_t i = 0; i < n; i++) {
        order[2 * i] = s->frags[i].set;
        order[2 * i + 1] = i;
    }
    qsort(order, (size_t)n, sizeof *order * 2, by_pair);
    int64_t nGroups = 0;
    for (int64_t i = 0; i < n; i++) {
        if (i == 0 || order[2 * i] != order[2 * i - 2]) {
            groups[3 * nGroups] = order[2 * i + 1];
            groups[3 * nGroups + 1] = i;
            groups[3 * nGroups + 2] = 0;
            nGroups++;
        }
        groups[3 * (nGroups - 1) + 2]++;
    }
    qsort(groups, (size_t)nGroups, sizeof *groups * 3, by_pair); /* (first members are distinct) */
    PairSink sink = {pairs, cap, 0};
    for (int64_t g = 0; g < nGroups; g++) {
        const int64_t *m = order + 2 * groups[3 * g + 1], cnt = groups[3 * g + 2]; /* member k is m[2 * k + 1] */
        if (mode == CPECAN_SETS_ALL) {
            for (int64_t a = 0; a < cnt; a++)
                for (int64_t b = a + 1; b < cnt; b++) emit(&sink, m[2 * a + 1], m[2 * b + 1]);
            continue;
        }
        int64_t *l2 = l + 3 * cnt, nRefs = 0, nChosen = 0;
        for (int64_t k = 0; k < cnt; k++) { /* :746-750 */
            const Fragment *f = &s->frags[m[2 * k + 1]];
            l[3 * k] = f->rightEndId;
            l[3 * k + 1] = f->length;
            l[3 * k + 2] = m[2 * k + 1];
        }
        qsort(l, (size_t)cnt, sizeof *l * 3, by_triple);
        for (int64_t i = 0, j = 1; j <= cnt; j++) /* :752-763 */
            if (j == cnt || l[3 * j] != l[3 * i]) {
                memcpy(l2 + 3 * nRefs++, star(l, i, j, chosen, &nChosen), sizeof *l * 3);
                i = j;
            }
        star(l2, 0, nRefs, chosen, &nChosen); /* :765 */
        qsort(chosen, (size_t)nChosen, sizeof *chosen * 2, by_pair);
        for (int64_t k = 0; k < nChosen; k++) emit(&sink, chosen[2 * k], chosen[2 * k + 1]);
    }
    free(order);
    free(groups);
    free(l);
    free(chosen);
    return sink.n;
}

/* ---- aligning ---- */
void cpecan_sets_result_free(cpecan_sets_result *r) {
    if (!r) return;
    cpk_host_free(r->quints);
    free(r->offsets);
    free(r->similarity);
    free(r);
}

int cpecan_sets_align(cpecan_sets *s, const int64_t *pairs, int64_t nPairs, cpecan_sets_result **out) {
    if (!s || !out || nPairs < 0 || (nPairs > 0 && !pairs)) return CPECAN_EINVAL;
    for (int64_t k = 0; k < nPairs; k++) {
        const int64_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || b < 0 || a >= s->n || b >= s->n) {
            cpk_set_error("cpecan_sets_align: pair %lld names fragment %lld, there are %lld", (long long)k,
                          (long long)(a < 0 || a >= s->n ? a : b), (long long)s->n);
            return CPECAN_EINVAL;
        }
        if (a == b) {
            cpk_set_error("cpecan_sets_align: pair %lld aligns fragment %lld with itself", (long long)k, (long long)a);
            return CPECAN_EINVAL;
        }
        if (s->frags[a].set != s->frags[b].set) {
            cpk_set_error("cpecan_sets_align: pair %lld: fragments %lld and %lld are of different sets", (long long)k, (long long)a,
                          (long long)b);
            return CPECAN_EINVAL;
        }
    }
    const int nDev = cpk_device_count();
    if (nDev <= 0 || s->device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, s->device);
        return CPECAN_ENODEVICE;
    }
    const double t0 = now_ms();
    const size_t m = (size_t)(nPairs ? nPairs : 1);
    cpecan_sets_result *r = calloc(1, sizeof *r);
    cpecan_anchor_problem *ap = calloc(m, sizeof *ap);
    cpecan_problem_runs *pr = calloc(m, sizeof *pr);
    int64_t **runs = calloc(m, sizeof *runs), *nRuns = calloc(m, sizeof *nRuns);
    int32_t *names = calloc(m, sizeof *names * 2);
    cpecan_batch *b = NULL;
    int rc = (r && ap && pr && runs && nRuns && names) ? CPECAN_OK : CPECAN_ENOMEM;
    for (int64_t k = 0; rc == CPECAN_OK && k < nPairs; k++) {
        const Fragment *x = &s->frags[pairs[2 * k]], *y = &s->frags[pairs[2 * k + 1]];
        ap[k].sX = x->seq;
        ap[k].lX = x->length;
        ap[k].sY = y->seq;
        ap[k].lY = y->length;
        names[2 * k] = (int32_t)pairs[2 * k];
        names[2 * k + 1] = (int32_t)pairs[2 * k + 1];
    }
    /* ONE anchor batch (getBlastPairsForPairwiseAlignmentParameters per pair, pairwiseAligner.c:1162-1196) */
    if (rc == CPECAN_OK && nPairs > 0)
        rc = cpecan_find_anchor_runs_many(ap, nPairs, s->options.constraintDiagonalTrim, s->params.diagonalExpansion,
                                          s->options.anchorMatrixBiggerThanThis, s->options.repeatMaskMatrixBiggerThanThis, NULL,
                                          s->device, runs, nRuns, NULL);
    const double t1 = now_ms();
    /* ONE DP batch: getAlignedPairsUsingAnchors, reweightAlignedPairs2, the records and the score sums */
    for (int64_t k = 0; rc == CPECAN_OK && k < nPairs; k++) {
        const Fragment *x = &s->frags[pairs[2 * k]], *y = &s->frags[pairs[2 * k + 1]];
        pr[k].sX = ap[k].sX;
        pr[k].lX = ap[k].lX;
        pr[k].sY = ap[k].sY;
        pr[k].lY = ap[k].lY;
        pr[k].runs = runs[k];
        pr[k].nRuns = nRuns[k];
        pr[k].raggedLeft = x->leftEndId != y->leftEndId; /* multipleAligner.c:661 */
        pr[k].raggedRight = x->rightEndId != y->rightEndId;
    }
    if (rc == CPECAN_OK) rc = cpecan_batch_create(&b, &s->model, &s->params, CPECAN_EMIT_MATCH, s->device);
    if (rc == CPECAN_OK) rc = cpecan_batch_set_post(b, CPECAN_POST_REWEIGHT, (double)s->options.gapGamma); /* :662 */
    if (rc == CPECAN_OK && nPairs > 0) {
        const int64_t first = cpecan_batch_add_many_runs(b, pr, nPairs);
        if (first < 0) rc = (int)first;
    }
    if (rc == CPECAN_OK) rc = cpecan_batch_set_quintuples(b, names, nPairs);
    if (rc == CPECAN_OK) rc = cpecan_batch_upload(b);
    const double t2 = now_ms();
    if (rc == CPECAN_OK) rc = cpecan_batch_run(b, NULL);
    if (rc == CPECAN_OK) rc = cpecan_batch_download(b);
    const double t3 = now_ms();
    int64_t *sums = NULL;
    if (rc == CPECAN_OK) {
        cpecan_stats st;
        cpecan_batch_stats(b, &st);
        r->timing.dpKernelMs = st.kernelMs;
        rc = cpk_batch_take_quintuples(b, &r->quints, &r->offsets, &sums, &r->timing.stageMs);
    }
    if (rc == CPECAN_OK) { /* getAlignmentScore (:604-619) from the integer sums */
        r->similarity = sums;
        for (int64_t k = 0; k < nPairs; k++) r->similarity[k] = cpecan_similarity_score(sums[k], pr[k].lX, pr[k].lY);
        r->nPairs = nPairs;
        r->timing.anchorMs = t1 - t0;
        r->timing.packMs = t2 - t1;
        r->timing.downloadMs = t3 - t2;
        r->timing.totalMs = now_ms() - t0;
    }
    if (b) cpecan_batch_destroy(b);
    for (int64_t k = 0; runs && k < nPairs; k++) cpecan_free(runs[k]);
    free(runs);
    free(nRuns);
    free(ap);
    free(pr);
    free(names);
    if (rc != CPECAN_OK) {
        cpecan_sets_result_free(r);
        return rc;
    }
    *out = r;
    return CPECAN_OK;
}

int cpecan_sets_result_pairs(const cpecan_sets_result *r, const int32_t **quints, int64_t *n) {
    if (!r || !quints || !n) return CPECAN_EINVAL;
    *quints = r->quints;
    *n = r->offsets[r->nPairs];
    return CPECAN_OK;
}

int cpecan_sets_result_offsets(const cpecan_sets_result *r, const int64_t **offsets, int64_t *nPairs) {
    if (!r || !offsets) return CPECAN_EINVAL;
    *offsets = r->offsets;
    if (nPairs) *nPairs = r->nPairs;
    return CPECAN_OK;
}

int cpecan_sets_result_similarity(const cpecan_sets_result *r, const int64_t **similarity, int64_t *nPairs) {
    if (!r || !similarity) return CPECAN_EINVAL;
    *similarity = r->similarity;
    if (nPairs) *nPairs = r->nPairs;
    return CPECAN_OK;
}

int cpecan_sets_result_timing(const cpecan_sets_result *r, cpecan_sets_timing *t) {
    if (!r || !t) return CPECAN_EINVAL;
    *t = r->timing;
    return CPECAN_OK;
}
