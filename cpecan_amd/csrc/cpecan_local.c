/*
 * cpecan_local.c -- host side of the local chains (include/cpecan_local.h: cpecan_find_local_chains_many and
 * cpecan_find_local_chains_many_gapped).  The kernels do steps 0-3 as for every anchor
 * pass, peel the chains and, where the problems ask for it, extend them (cpk_local.inl); this file checks the call, lays the
 * pairs out with the anchor finder's own layout stage (every pair whole, soft-masked, twins for BOTH), and turns the device
 * records into the caller's arrays.  A call is three stages -- check, layout, assemble -- around one device function,
 * cpk_local_pass; no stage touches a device (tests/test_local_cpu.py and tests/test_local_gapped_cpu.py run them with the
 * model in the pass's place, tests/c/test_local_plan.c and test_local_gapped_plan.c over synthetic passes).
 */
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"
#include "cpecan_local.h"

int cpecan_local_options_default(cpecan_local_options *o) {
    if (!o) return CPECAN_EINVAL;
    memset(o, 0, sizeof *o);
    o->maxChains = 1;
    return CPECAN_OK;
}

/* The call as the anchor finder's stages see it: steps 1-5 alone on every problem whatever its size (`once`), soft mask on. */
static CpkAnchorCall anchor_call(const CpkLocalCall *c) {
    const CpkAnchorCall a = {c->who, c->problems, c->n, c->expansion, 0, 0, c->device, c->strandMode, 1, 1, c->runs, c->nRuns, NULL, NULL};
    return a;
}

static int local_check(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                       const cpecan_local_options *localOptions, CpkAnchorPass *pass, CpkLocalPass *lp, int admitGapped) {
    if (c->n < 0 || (c->n > 0 && (!c->chains || !c->nChains || !c->runs || !c->nRuns))) {
        cpk_set_error("%s: bad arguments", c->who);
        return CPECAN_EINVAL;
    }
    for (int64_t i = 0; i < c->n; i++) {
        c->chains[i] = NULL;
        c->nChains[i] = 0;
    }
    if (c->stats) memset(c->stats, 0, sizeof *c->stats * (size_t)c->n);
    const CpkAnchorCall a = anchor_call(c);
    const int rc = cpk_anchor_check(&a, trim, params, anchorOptions, pass); /* zeroes runs and nRuns */
    if (rc != CPECAN_OK) return rc;
    if (!admitGapped && anchorOptions && anchorOptions->gappedExtension) {
        cpk_set_error("%s: gappedExtension wants cpecan_find_local_chains_many_gapped", c->who);
        return CPECAN_EINVAL;
    }
    cpecan_local_options def;
    if (!localOptions) {
        cpecan_local_options_default(&def);
        localOptions = &def;
    }
    for (int k = 0; k < 6; k++)
        if (localOptions->reserved[k] != 0) {
            cpk_set_error("%s: a reserved word of the local options is not 0", c->who);
            return CPECAN_EINVAL;
        }
    if (localOptions->maxChains < 1 || localOptions->maxChains > CPK_LOCAL_MAX_CHAINS) {
        cpk_set_error("%s: maxChains is 1 .. %d", c->who, CPK_LOCAL_MAX_CHAINS);
        return CPECAN_EINVAL;
    }
    if (localOptions->minChainScore < 0 || (localOptions->minChainScore != 0 && localOptions->minChainScore < pass->prm.hspThreshold)) {
        cpk_set_error("%s: minChainScore is 0 or at least hspThreshold", c->who);
        return CPECAN_EINVAL;
    }
    lp->maxChains = localOptions->maxChains;
    lp->minChainScore = localOptions->minChainScore ? localOptions->minChainScore : pass->prm.hspThreshold;
    return CPECAN_OK;
}

int cpk_local_check(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                    const cpecan_local_options *localOptions, CpkAnchorPass *pass, CpkLocalPass *lp) {
    return local_check(c, trim, params, anchorOptions, localOptions, pass, lp, 0);
}

/* The check of the entry point that extends chains: gappedExtension = 1 passes, with what cpk_anchor_check holds its yDrop
 * and gappedMaxDiagonals to. */
int cpk_local_check_gapped(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params,
                           const cpecan_anchor_options *anchorOptions, const cpecan_local_options *localOptions, CpkAnchorPass *pass,
                           CpkLocalPass *lp) {
    return local_check(c, trim, params, anchorOptions, localOptions, pass, lp, 1);
}

/* Step 7b on every problem of the list, as step 5b reaches an anchor pass: the flag, and the options' values or what their
 * zeros stand for, travel with the problems.  The options passed the check. */
void cpk_local_mark_gapped(CpkAnchorList *top, const cpecan_anchor_options *o) {
    if (!o || !o->gappedExtension) return;
    const int32_t diags = o->gappedMaxDiagonals ? o->gappedMaxDiagonals : CPK_ANCHOR_GAPPED_MAX_DIAGS;
    for (int64_t k = 0; k < top->n; k++) {
        top->probs[k].flags |= CPK_ANCHOR_GAPPED | (diags << CPK_ANCHOR_DIAGS_SHIFT);
        top->probs[k].yDrop = o->yDrop ? o->yDrop : CPK_ANCHOR_GAPPED_Y_DROP;
    }
}

int cpk_local_layout(const CpkLocalCall *c, CpkAnchorList *top, uint8_t **bytes, int64_t *nBytes, int64_t *nExtra,
                     CpkLocalProblem **lprobs, int64_t *nLocal) {
    const CpkAnchorCall a = anchor_call(c);
    const int twins = c->strandMode == CPECAN_STRAND_BOTH ? 2 : 1;
    *lprobs = NULL;
    *nLocal = 0;
    const int rc = cpk_anchor_layout(&a, top, bytes, nBytes, nExtra);
    if (rc != CPECAN_OK || top->n == 0) return rc;
    *nLocal = top->n / twins;
    if (!(*lprobs = calloc((size_t)*nLocal, sizeof **lprobs))) return CPECAN_ENOMEM;
    for (int64_t k = 0; k < *nLocal; k++) {
        (*lprobs)[k].first = k * twins;
        (*lprobs)[k].twins = twins;
    }
    return CPECAN_OK;
}

int cpk_local_assemble(const CpkLocalCall *c, const CpkAnchorList *top, const CpkLocalProblem *lprobs, int64_t nLocal,
                       const CpkLocalChain *chains, const int32_t *runs, int32_t maxChains, double kernelMs) {
    for (int64_t k = 0; k < nLocal; k++) {
        const CpkLocalProblem *q = &lprobs[k];
        const int64_t i = top->owner[q->first];
        const CpkLocalChain *from = chains + k * maxChains;
        const int32_t *r = runs + 3 * top->probs[q->first].hspOff;
        cpecan_local_chain *out = malloc(sizeof *out * (size_t)(q->nChains ? q->nChains : 1));
        int64_t *outRuns = malloc(sizeof *outRuns * 4 * (size_t)(q->nRuns ? q->nRuns : 1));
        c->chains[i] = out;
        c->runs[i] = outRuns;
        if (!out || !outRuns) return CPECAN_ENOMEM;
        for (int32_t j = 0; j < q->nChains; j++) {
            const CpkLocalChain *f = &from[j];
            out[j] = (cpecan_local_chain){f->strand, f->score, f->nHsps, f->x0, f->x1, f->y0, f->y1, f->runOff, f->nRuns};
        }
        for (int32_t u = 0; u < q->nRuns; u++) {
            const int64_t quad[4] = {r[3 * u], r[3 * u + 1], r[3 * u + 2], c->expansion};
            memcpy(outRuns + 4 * u, quad, sizeof quad);
        }
        c->nChains[i] = q->nChains;
        c->nRuns[i] = q->nRuns;
        if (!c->stats) continue;
        cpecan_local_stats *st = &c->stats[i];
        st->rounds = q->rounds;
        for (int t = 0; t < q->twins; t++) {
            const CpkAnchorProblem *p = &top->probs[q->first + t];
            const int minus = (p->flags & CPK_ANCHOR_RC_Y) != 0;
            *(minus ? &st->hitsMinus : &st->hitsPlus) = p->hits;
            *(minus ? &st->hspsMinus : &st->hspsPlus) = p->hsps;
            if (p->capped) st->capped |= 1 << minus;
        }
    }
    for (int64_t i = 0; c->stats && i < c->n; i++) c->stats[i].kernelMs = kernelMs;
    return CPECAN_OK;
}

/* Both entry points: check, device, layout, open, pass, assemble, close. */
static int find_chains(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                       const cpecan_local_options *localOptions, int admitGapped) {
    const int64_t n = c->n;
    const int device = c->device;
    cpecan_local_chain **chains = c->chains;
    int64_t **runs = c->runs, *nChains = c->nChains, *nRuns = c->nRuns;
    CpkAnchorPass pass;
    CpkLocalPass lp;
    CpkAnchorList top = {0};
    CpkAnchorCtx *ctx = NULL;
    CpkLocalProblem *lprobs = NULL;
    CpkLocalChain *found = NULL;
    uint8_t *bytes = NULL;
    int32_t *foundRuns = NULL;
    int64_t nBytes = 0, nExtra = 0, nLocal = 0;
    double ms = 0.0;
    int rc = local_check(c, trim, params, anchorOptions, localOptions, &pass, &lp, admitGapped);
    if (rc != CPECAN_OK) return rc;
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    if ((rc = cpk_local_layout(c, &top, &bytes, &nBytes, &nExtra, &lprobs, &nLocal)) != CPECAN_OK || top.n == 0) goto done;
    cpk_local_mark_gapped(&top, anchorOptions);
    if ((rc = cpk_anchor_open(&ctx, device, bytes, nBytes, nExtra)) != CPECAN_OK) goto done;
    if ((rc = cpk_local_pass(ctx, &pass, &lp, top.probs, top.n, lprobs, nLocal, &found, &foundRuns, &ms)) != CPECAN_OK) goto done;
    rc = cpk_local_assemble(c, &top, lprobs, nLocal, found, foundRuns, lp.maxChains, ms);
done:
    if (rc == CPECAN_ENOMEM) cpk_set_error("%s: out of memory", c->who);
    for (int64_t i = 0; rc != CPECAN_OK && i < n; i++) {
        free(chains[i]);
        free(runs[i]);
        chains[i] = NULL;
        runs[i] = NULL;
        nChains[i] = nRuns[i] = 0;
    }
    cpk_anchor_close(ctx);
    cpk_anchor_list_free(&top);
    free(lprobs);
    free(bytes);
    free(found);
    free(foundRuns);
    return rc;
}

int cpecan_find_local_chains_many(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                  const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                                  const cpecan_local_options *localOptions, int device, int strandMode,
                                  cpecan_local_chain **chains, int64_t *nChains, int64_t **runs, int64_t *nRuns,
                                  cpecan_local_stats *stats) {
    const CpkLocalCall call = {"cpecan_find_local_chains_many", problems, n, expansion, device, strandMode, chains, nChains, runs, nRuns, stats};
    return find_chains(&call, trim, params, anchorOptions, localOptions, 0);
}

int cpecan_find_local_chains_many_gapped(const cpecan_anchor_problem *problems, int64_t n, int64_t trim, int64_t expansion,
                                         const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                                         const cpecan_local_options *localOptions, int device, int strandMode,
                                         cpecan_local_chain **chains, int64_t *nChains, int64_t **runs, int64_t *nRuns,
                                         cpecan_local_stats *stats) {
    const CpkLocalCall call = {"cpecan_find_local_chains_many_gapped", problems, n, expansion, device, strandMode, chains, nChains, runs, nRuns, stats};
    return find_chains(&call, trim, params, anchorOptions, localOptions, 1);
}

static int push_op(cpecan_cigar *c, int64_t type, int64_t len) {
    if (len <= 0) return 0;
    c->ops[2 * c->nOps] = type;
    c->ops[2 * c->nOps + 1] = len;
    c->nOps++;
    return 1;
}

int cpecan_cigar_from_local_chain(const char *contig1, const char *contig2, int64_t lY, const cpecan_local_chain *chain,
                                  const int64_t *runs, cpecan_cigar *out) {
    if (!contig1 || !contig2 || !chain || !runs || !out || lY < 0 || chain->nRuns < 1 || chain->runOff < 0 ||
        (chain->strand != CPECAN_STRAND_PLUS && chain->strand != CPECAN_STRAND_MINUS)) {
        cpk_set_error("cpecan_cigar_from_local_chain: bad arguments, or a chain without runs");
        return CPECAN_EINVAL;
    }
    const int64_t *r = runs + 4 * chain->runOff, m = chain->nRuns;
    for (int64_t k = 0; k < m; k++) { /* a chain: every run behind the one before it on both sequences */
        const int64_t pX = k ? r[4 * (k - 1)] + r[4 * (k - 1) + 2] : 0, pY = k ? r[4 * (k - 1) + 1] + r[4 * (k - 1) + 2] : 0;
        if (r[4 * k + 2] < 1 || r[4 * k] < pX || r[4 * k + 1] < pY) {
            cpk_set_error("cpecan_cigar_from_local_chain: run %lld does not follow the one before it", (long long)k);
            return CPECAN_EINVAL;
        }
    }
    const int64_t x0 = r[0], y0 = r[1], x1 = r[4 * (m - 1)] + r[4 * (m - 1) + 2], y1 = r[4 * (m - 1) + 1] + r[4 * (m - 1) + 2];
    const int minus = chain->strand == CPECAN_STRAND_MINUS;
    if (minus && y1 > lY) {
        cpk_set_error("cpecan_cigar_from_local_chain: the chain ends behind lY");
        return CPECAN_EINVAL;
    }
    memset(out, 0, sizeof *out);
    out->contig1 = malloc(strlen(contig1) + 1);
    out->contig2 = malloc(strlen(contig2) + 1);
    out->ops = malloc(sizeof *out->ops * 2 * 3 * (size_t)m);
    if (!out->contig1 || !out->contig2 || !out->ops) {
        cpecan_cigar_clear(out);
        cpk_set_error("cpecan_cigar_from_local_chain: out of memory");
        return CPECAN_ENOMEM;
    }
    strcpy(out->contig1, contig1);
    strcpy(out->contig2, contig2);
    out->start1 = x0;
    out->end1 = x1;
    out->strand1 = 1;
    out->start2 = minus ? lY - y0 : y0;
    out->end2 = minus ? lY - y1 : y1;
    out->strand2 = !minus;
    out->score = (double)chain->score;
    for (int64_t k = 0; k < m; k++) {
        if (k) { /* the X bases first, then the Y bases: cigar_from_pairs of cpecan_realign.c */
            push_op(out, CPECAN_OP_INDEL_X, r[4 * k] - (r[4 * (k - 1)] + r[4 * (k - 1) + 2]));
            push_op(out, CPECAN_OP_INDEL_Y, r[4 * k + 1] - (r[4 * (k - 1) + 1] + r[4 * (k - 1) + 2]));
        }
        push_op(out, CPECAN_OP_MATCH, r[4 * k + 2]);
    }
    return CPECAN_OK;
}
