/*
 * cpecan_align -- command line of cPecanAlign (cPecanAlign.c:91-164): every query sequence against every target
 * sequence, five-state default model, getAlignedPairs with both ends ragged, reweightAlignedPairs2 with gapGamma, ordered
 * filter at 0.9, one cigar per pair on stdout.  Unlike the reference's loop, the anchors of all pairs are found in one
 * anchor batch (cpecan_find_anchor_runs_many_stranded) and all pairs are aligned in one DP batch.  Output order: queries in
 * file order, for each the targets in file order (the reference iterates hash tables, so it defines no order).
 * --strand both does what the reference leaves open at cPecanAlign.c:116-117: every pair is tried against the query and
 * its reverse complement, and a pair on the minus strand gets a cigar with "<length> 0 -" for the query.
 * --seedTransitions lets a seed hit of the anchor finder carry one transition (cpecan_anchor_params.seedTransitions = 1).
 * --transitionHspThreshold N asks N of an HSP that only such hits extend to (cpecan_anchor_options); it needs --seedTransitions.
 * --gapped extends the chained HSPs of the anchor finder across indels (cpecan_anchor_options.gappedExtension); --yDrop N
 * sets what ends such an extension and needs --gapped.
 * --diagonalExpansion N replaces the expansion of pairwiseAlignmentBandingParameters_construct (20) for the anchors and the band.
 * --adaptiveBand N --minEdgeScore S (each needs the other): the DP batch also computes the posterior mass on the band's edge
 * (cpecan_band_edge); a pair whose edgeScoreSum reaches S runs again, up to N = 1..4 times, in a batch of the flagged pairs
 * with the expansion of their runs and of the parameters doubled per round.  Anchors are not searched again.  A pair's cigar
 * is that of its last run, and stderr names the round and the expansion every pair ended on.
 * --local [--maxChains K] [--minChainScore S]: the reference's `lastz | cPecanRealign` pipeline in one process.  All pairs go
 * through one cpecan_find_local_chains_many call (include/cpecan_local.h) with trim 0, every chain becomes a cigar, and all
 * cigars go through one cpecan_realigner_realign with the realigner's default options, the gapGamma of this command line and
 * its --diagonalExpansion and --loadHmm.  Output: queries outer, targets inner, the chains of a pair in round order; a pair
 * may have no line or several.  Sequences are looked up by name, so target and query names must differ.
 * --local --extendChains [--chainYDrop N]: the chains are extended into their gaps and outwards before they become cigars
 * (cpecan_find_local_chains_many_gapped), as lastz's cigars are gapped; --chainYDrop sets what
 * ends such an extension (default 9400).  Both need --local, --chainYDrop needs --extendChains.
 * --viterbi: anchors are found as above (--strand, --seedTransitions, --gapped and --diagonalExpansion apply), then all pairs go
 * through one cpecan_viterbi object (include/cpecan_viterbi.h) instead of the DP batch, both ends ragged: a pair's cigar is
 * made of the match steps of its most probable state path (cpecan_viterbi_pairs), columns between two regions unaligned, and
 * its score is the path's log-probability.  Refused with --local and with --adaptiveBand.
 */
#define _POSIX_C_SOURCE 200809L
#include <ctype.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_local.h"
#include "cpecan_realign.h"
#include "cpecan_viterbi.h"

typedef struct {
    char *name, *seq;
    int64_t length;
} Record;

typedef struct {
    Record *r;
    int64_t n, cap;
} Records;

static void usage(void) {
    fprintf(stderr, "cpecan_align [options] target.fa query.fa > cigars\n"
                    "-y --loadHmm FILE  -g --device N  -s --strand plus|minus|both (default plus)\n"
                    "-t --seedTransitions (anchor seed hits may carry one transition)  -h --help\n"
                    "-T --transitionHspThreshold N (with --seedTransitions: an HSP that no exact seed hit extends to must score N;\n"
                    "   at least the HSP threshold, 800)\n"
                    "-G --gapped (gapped extension of the chained HSPs)  -Y --yDrop N (with --gapped; default 9400)\n"
                    "-r --diagonalExpansion N (even; default 20)\n"
                    "--adaptiveBand N --minEdgeScore S (each needs the other): pairs whose posterior mass on the band's edge sums to S\n"
                    "   or more (score units, 10000000 = probability 1) run again, up to N = 1..4 times, each with the expansion doubled\n"
                    "--local (local chains on the strands of --strand, each realigned; one cigar per chain)\n"
                    "   --maxChains K (1..16, default 1)  --minChainScore S (default: the HSP threshold, 800); both need --local;\n"
                    "   --local does not go with --gapped or --adaptiveBand\n"
                    "   --extendChains (with --local: gapped extension of every chain into its gaps and outwards, each chain kept clear\n"
                    "   of the others)  --chainYDrop N (with --extendChains; default 9400)\n"
                    "--viterbi (the most probable state path of every pair instead of its posterior pairs; the cigar's score is the\n"
                    "   path's log-probability; does not go with --local or --adaptiveBand)\n");
}

static int fail(const char *what) {
    const char *e = cpecan_last_error();
    fprintf(stderr, "cpecan_align: %s: %s\n", what, e ? e : "");
    return 1;
}

/* fastaRead + the first white-space delimited token of the header as the name (cPecanAlign.c:17-37) */
static int read_fasta(const char *path, Records *out) {
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    char *line = NULL;
    size_t lineCap = 0;
    int64_t seqCap = 0;
    int rc = 0;
    Record *cur = NULL;
    while (getline(&line, &lineCap, f) >= 0) {
        if (line[0] == '>') {
            if (out->n == out->cap) {
                out->cap = out->cap ? 2 * out->cap : 16;
                Record *g = realloc(out->r, sizeof *g * (size_t)out->cap);
                if (!g) { rc = -1; break; }
                out->r = g;
            }
            cur = &out->r[out->n++];
            const size_t len = strcspn(line + 1, " \t\r\n");
            cur->name = strndup(line + 1, len);
            cur->seq = NULL;
            cur->length = 0;
            seqCap = 0;
            if (!cur->name) { rc = -1; break; }
        } else if (cur) {
            for (const char *p = line; *p; p++) {
                if (isspace((unsigned char)*p)) continue;
                if (cur->length + 1 >= seqCap) {
                    seqCap = seqCap ? 2 * seqCap : 1024;
                    char *g = realloc(cur->seq, (size_t)seqCap);
                    if (!g) { rc = -1; break; }
                    cur->seq = g;
                }
                cur->seq[cur->length++] = *p;
            }
            if (rc) break;
        }
    }
    for (int64_t i = 0; rc == 0 && i < out->n; i++) {
        if (!out->r[i].seq && !(out->r[i].seq = malloc(1))) rc = -1;
        if (rc == 0) out->r[i].seq[out->r[i].length] = 0;
    }
    free(line);
    fclose(f);
    return rc;
}

static void free_records(Records *a) {
    for (int64_t i = 0; i < a->n; i++) {
        free(a->r[i].name);
        free(a->r[i].seq);
    }
    free(a->r);
}

static int by_x(const void *a, const void *b) {
    const int64_t *p = a, *q = b;
    return p[0] < q[0] ? -1 : p[0] > q[0];
}

/* One DP batch over the m pairs idx[0 .. m): getAlignedPairs with both ends ragged, reweightAlignedPairs2, the ordered
 * filter at 0.9 (cPecanAlign.c:125-139).  texts[i] receives pair i's cigar (the text it held is released); edgeSum, when
 * given, its edgeScoreSum. */
static int align_pairs(const cpecan_model *model, const cpecan_params *params, double gapGamma, int device,
                       const cpecan_problem_runs *pr, const int32_t *yMinus, const Records *targets, const Records *queries,
                       const int64_t *idx, int64_t m, char **texts, int64_t *edgeSum) {
    int status = 0;
    cpecan_batch *b = NULL;
    cpecan_problem_runs *sub = malloc(sizeof *sub * (size_t)m);
    int32_t *subMinus = malloc(sizeof *subMinus * (size_t)m);
    if (!sub || !subMinus) status = 1;
    for (int64_t j = 0; status == 0 && j < m; j++) {
        sub[j] = pr[idx[j]];
        subMinus[j] = yMinus[idx[j]];
    }
    if (status != 0) status = 1;
    else if (cpecan_batch_create(&b, model, params, CPECAN_EMIT_MATCH, device) != CPECAN_OK) status = fail("batch");
    else if (cpecan_batch_set_post(b, CPECAN_POST_REWEIGHT | CPECAN_POST_ORDERED, gapGamma) != CPECAN_OK ||
             cpecan_batch_set_match_gamma(b, 0.9f) != CPECAN_OK) /* :129-139 */
        status = fail("consumers");
    else if (edgeSum && cpecan_batch_set_band_edge(b, 1) != CPECAN_OK) status = fail("band edge");
    else if (cpecan_batch_add_many_runs_stranded(b, sub, subMinus, m) < 0) status = fail("add");
    else if (cpecan_batch_upload(b) != CPECAN_OK) status = fail("upload");
    else if (cpecan_batch_run(b, NULL) != CPECAN_OK) status = fail("run");
    else if (cpecan_batch_download(b) != CPECAN_OK) status = fail("download");
    for (int64_t j = 0; status == 0 && j < m; j++) {
        const int64_t i = idx[j];
        const int32_t *tr = NULL;
        int64_t cnt = 0;
        cpecan_band_edge e;
        if (cpecan_batch_result(b, j, 3, &tr, &cnt) != CPECAN_OK || (edgeSum && cpecan_batch_band_edge(b, j, &e) != CPECAN_OK)) {
            status = fail("result");
            break;
        }
        if (edgeSum) edgeSum[i] = e.edgeScoreSum;
        int64_t *xy = malloc(sizeof *xy * 2 * (size_t)(cnt ? cnt : 1));
        if (!xy) {
            status = 1;
            break;
        }
        for (int64_t k = 0; k < cnt; k++) { /* :144-145 */
            xy[2 * k] = tr[3 * k + 1];
            xy[2 * k + 1] = tr[3 * k + 2];
        }
        qsort(xy, (size_t)cnt, sizeof *xy * 2, by_x);
        cpecan_cigar c;
        memset(&c, 0, sizeof c);
        if (cpecan_cigar_from_aligned_pairs_stranded(targets->r[i % targets->n].name, queries->r[i / targets->n].name, 0.0, pr[i].lX,
                                                     pr[i].lY, !yMinus[i], xy, cnt, &c) != CPECAN_OK) {
            status = fail("cigar");
        } else {
            const int64_t need = cpecan_cigar_format(&c, NULL, 0) + 1;
            char *text = malloc((size_t)need);
            if (text) {
                cpecan_cigar_format(&c, text, need);
                free(texts[i]);
                texts[i] = text;
            } else {
                status = 1;
            }
            cpecan_cigar_clear(&c);
        }
        free(xy);
    }
    if (b) cpecan_batch_destroy(b);
    free(sub);
    free(subMinus);
    return status;
}

/* --viterbi: all n pairs through one cpecan_viterbi object, both ends ragged; texts[i] receives pair i's cigar. */
static int viterbi_pairs(const cpecan_model *model, const cpecan_params *params, int device, const cpecan_problem_runs *pr,
                         const int32_t *yMinus, const Records *targets, const Records *queries, int64_t n, char **texts) {
    int status = 0;
    cpecan_viterbi *v = NULL;
    if (cpecan_viterbi_create(&v, model, params, device) != CPECAN_OK) return fail("viterbi");
    for (int64_t i = 0; status == 0 && i < n; i++) {
        int64_t nAnchors = 0;
        for (int64_t q = 0; q < pr[i].nRuns; q++) nAnchors += pr[i].runs[4 * q + 2];
        int64_t *a = malloc(sizeof *a * 3 * (size_t)(nAnchors ? nAnchors : 1));
        char *rc = yMinus[i] ? malloc((size_t)(pr[i].lY ? pr[i].lY : 1)) : NULL;
        if (!a || (yMinus[i] && !rc)) status = 1;
        else if (rc && cpecan_reverse_complement(pr[i].sY, pr[i].lY, rc) != CPECAN_OK) status = fail("reverse complement");
        for (int64_t q = 0, k = 0; status == 0 && q < pr[i].nRuns; q++)
            for (int64_t j = 0; j < pr[i].runs[4 * q + 2]; j++, k++) {
                a[3 * k] = pr[i].runs[4 * q] + j;
                a[3 * k + 1] = pr[i].runs[4 * q + 1] + j;
                a[3 * k + 2] = pr[i].runs[4 * q + 3];
            }
        if (status == 0 && cpecan_viterbi_add(v, pr[i].sX, pr[i].lX, rc ? rc : pr[i].sY, pr[i].lY, a, nAnchors, 1, 1) != i) status = fail("add");
        free(a);
        free(rc);
    }
    if (status == 0 && cpecan_viterbi_run(v) != CPECAN_OK) status = fail("run");
    for (int64_t i = 0; status == 0 && i < n; i++) {
        cpecan_viterbi_result_t res;
        if (cpecan_viterbi_result(v, i, &res) != CPECAN_OK) {
            status = fail("result");
            break;
        }
        const int64_t cnt = cpecan_viterbi_pairs(&res, NULL, 0);
        int64_t *xy = malloc(sizeof *xy * 2 * (size_t)(cnt > 0 ? cnt : 1));
        cpecan_cigar c;
        memset(&c, 0, sizeof c);
        if (!xy || cnt < 0 || cpecan_viterbi_pairs(&res, xy, cnt) != cnt) status = 1;
        else if (cpecan_cigar_from_aligned_pairs_stranded(targets->r[i % targets->n].name, queries->r[i / targets->n].name, res.logP,
                                                          pr[i].lX, pr[i].lY, !yMinus[i], xy, cnt, &c) != CPECAN_OK) {
            status = fail("cigar");
        } else {
            const int64_t need = cpecan_cigar_format(&c, NULL, 0) + 1;
            char *text = malloc((size_t)need);
            if (text) {
                cpecan_cigar_format(&c, text, need);
                free(texts[i]);
                texts[i] = text;
            } else {
                status = 1;
            }
            cpecan_cigar_clear(&c);
        }
        free(xy);
    }
    cpecan_viterbi_destroy(v);
    return status;
}

/* --local: chains -> cigars -> one realign call; prints the realigned cigars. */
static int run_local(const cpecan_model *model, const cpecan_anchor_problem *ap, int64_t n, const Records *targets,
                     const Records *queries, int64_t expansion, int64_t runExpansion, double gapGamma,
                     const cpecan_anchor_params *anchorParams, const cpecan_anchor_options *anchorOptions,
                     const cpecan_local_options *localOptions, int device, int strandMode, int extendChains) {
    int status = 0;
    cpecan_local_chain **chains = calloc((size_t)(n ? n : 1), sizeof *chains);
    int64_t **runs = calloc((size_t)(n ? n : 1), sizeof *runs);
    int64_t *nChains = calloc((size_t)(n ? n : 1), sizeof *nChains), *nRuns = calloc((size_t)(n ? n : 1), sizeof *nRuns);
    cpecan_cigar *in = NULL, *out = NULL;
    cpecan_realigner *r = NULL;
    int64_t nIn = 0, nOut = 0, total = 0;
    if (!chains || !runs || !nChains || !nRuns) status = 1;
    else if (n > 0 && (extendChains ? cpecan_find_local_chains_many_gapped : cpecan_find_local_chains_many)(
                          ap, n, 0, runExpansion, anchorParams, anchorOptions, localOptions, device, strandMode, chains, nChains, runs,
                          nRuns, NULL) != CPECAN_OK)
        status = fail("local chains");
    for (int64_t i = 0; status == 0 && i < n; i++) total += nChains[i];
    if (status == 0 && !(in = calloc((size_t)(total ? total : 1), sizeof *in))) status = 1;
    for (int64_t i = 0; status == 0 && i < n; i++)
        for (int64_t j = 0; status == 0 && j < nChains[i]; j++) {
            if (chains[i][j].nRuns == 0) continue; /* trim is 0: does not happen */
            if (cpecan_cigar_from_local_chain(targets->r[i % targets->n].name, queries->r[i / targets->n].name, ap[i].lY,
                                              &chains[i][j], runs[i], &in[nIn]) != CPECAN_OK)
                status = fail("cigar");
            else nIn++;
        }
    if (status == 0 && nIn > 0) {
        cpecan_realign_options ro;
        cpecan_realign_options_default(&ro);
        ro.gapGamma = (float)gapGamma;
        if (expansion >= 0) ro.params.diagonalExpansion = expansion;
        if (cpecan_realigner_create(&r, model, &ro, device) != CPECAN_OK) status = fail("realigner");
        for (int64_t t = 0; status == 0 && t < targets->n; t++)
            if (cpecan_realigner_add_sequence(r, targets->r[t].name, targets->r[t].seq, targets->r[t].length) != CPECAN_OK) status = fail("sequence");
        for (int64_t q = 0; status == 0 && q < queries->n; q++)
            if (cpecan_realigner_add_sequence(r, queries->r[q].name, queries->r[q].seq, queries->r[q].length) != CPECAN_OK) status = fail("sequence");
        if (status == 0 && cpecan_realigner_realign(r, in, nIn, &out, &nOut) != CPECAN_OK) status = fail("realign");
    }
    for (int64_t k = 0; status == 0 && k < nOut; k++) {
        const int64_t need = cpecan_cigar_format(&out[k], NULL, 0) + 1;
        char *text = malloc((size_t)need);
        if (!text) {
            status = 1;
            break;
        }
        cpecan_cigar_format(&out[k], text, need);
        puts(text);
        free(text);
    }
    if (r) cpecan_realigner_destroy(r);
    cpecan_cigars_free(out, nOut);
    cpecan_cigars_free(in, nIn);
    for (int64_t i = 0; i < n; i++) {
        if (chains) cpecan_free(chains[i]);
        if (runs) cpecan_free(runs[i]);
    }
    free(chains);
    free(runs);
    free(nChains);
    free(nRuns);
    return status;
}

int main(int argc, char **argv) {
    const char *hmmFile = NULL;
    long long device = 0;
    int strandMode = CPECAN_STRAND_PLUS, seedTransitions = 0, haveThreshold = 0;
    long long transitionHspThreshold = 0, yDrop = 0;
    int gapped = 0, haveYDrop = 0;
    long long expansion = -1, adaptiveBand = 0, minEdgeScore = 0;
    int haveAdaptive = 0, haveMinEdge = 0;
    int localMode = 0, haveMaxChains = 0, haveMinChainScore = 0;
    long long maxChains = 1, minChainScore = 0, chainYDrop = 0;
    int extendChains = 0, haveChainYDrop = 0, viterbiMode = 0;
    static struct option longOpts[] = {{"help", no_argument, 0, 'h'},
                                       {"loadHmm", required_argument, 0, 'y'},
                                       {"device", required_argument, 0, 'g'},
                                       {"strand", required_argument, 0, 's'},
                                       {"seedTransitions", no_argument, 0, 't'},
                                       {"transitionHspThreshold", required_argument, 0, 'T'},
                                       {"gapped", no_argument, 0, 'G'},
                                       {"yDrop", required_argument, 0, 'Y'},
                                       {"diagonalExpansion", required_argument, 0, 'r'},
                                       {"adaptiveBand", required_argument, 0, 1000},
                                       {"minEdgeScore", required_argument, 0, 1001},
                                       {"local", no_argument, 0, 1002},
                                       {"maxChains", required_argument, 0, 1003},
                                       {"minChainScore", required_argument, 0, 1004},
                                       {"extendChains", no_argument, 0, 1005},
                                       {"chainYDrop", required_argument, 0, 1006},
                                       {"viterbi", no_argument, 0, 1007},
                                       {0, 0, 0, 0}};
    for (int key; (key = getopt_long(argc, argv, "hy:g:s:tT:GY:r:", longOpts, NULL)) != -1;) {
        switch (key) {
        case 'h': usage(); return 0;
        case 'y': hmmFile = optarg; break;
        case 'g': if (sscanf(optarg, "%lld", &device) != 1) { usage(); return 1; } break;
        case 's':
            if (strcmp(optarg, "plus") == 0) strandMode = CPECAN_STRAND_PLUS;
            else if (strcmp(optarg, "minus") == 0) strandMode = CPECAN_STRAND_MINUS;
            else if (strcmp(optarg, "both") == 0) strandMode = CPECAN_STRAND_BOTH;
            else { usage(); return 1; }
            break;
        case 't': seedTransitions = 1; break;
        case 'T':
            if (sscanf(optarg, "%lld", &transitionHspThreshold) != 1 || transitionHspThreshold < 0 || transitionHspThreshold > 0x7fffffffLL) {
                usage();
                return 1;
            }
            haveThreshold = 1;
            break;
        case 'G': gapped = 1; break;
        case 'Y':
            if (sscanf(optarg, "%lld", &yDrop) != 1 || yDrop < 1 || yDrop > 0x7fffffffLL) {
                usage();
                return 1;
            }
            haveYDrop = 1;
            break;
        case 'r': if (sscanf(optarg, "%lld", &expansion) != 1 || expansion < 0 || expansion % 2 != 0 || expansion > (1 << 20)) { usage(); return 1; } break;
        case 1000: if (sscanf(optarg, "%lld", &adaptiveBand) != 1 || adaptiveBand < 1 || adaptiveBand > 4) { usage(); return 1; } haveAdaptive = 1; break;
        case 1001: if (sscanf(optarg, "%lld", &minEdgeScore) != 1 || minEdgeScore < 1) { usage(); return 1; } haveMinEdge = 1; break;
        case 1002: localMode = 1; break;
        case 1003: if (sscanf(optarg, "%lld", &maxChains) != 1 || maxChains < 1 || maxChains > 16) { usage(); return 1; } haveMaxChains = 1; break;
        case 1004: if (sscanf(optarg, "%lld", &minChainScore) != 1 || minChainScore < 1 || minChainScore > 0x7fffffffLL) { usage(); return 1; } haveMinChainScore = 1; break;
        case 1005: extendChains = 1; break;
        case 1006: if (sscanf(optarg, "%lld", &chainYDrop) != 1 || chainYDrop < 1 || chainYDrop > 0x7fffffffLL) { usage(); return 1; } haveChainYDrop = 1; break;
        case 1007: viterbiMode = 1; break;
        default: usage(); return 1;
        }
    }
    if (haveThreshold && !seedTransitions) {
        fprintf(stderr, "cpecan_align: --transitionHspThreshold needs --seedTransitions\n");
        return 1;
    }
    if (haveYDrop && !gapped) {
        fprintf(stderr, "cpecan_align: --yDrop needs --gapped\n");
        return 1;
    }
    if (haveAdaptive != haveMinEdge) {
        fprintf(stderr, "cpecan_align: --adaptiveBand and --minEdgeScore need each other\n");
        return 1;
    }
    if ((haveMaxChains || haveMinChainScore) && !localMode) {
        fprintf(stderr, "cpecan_align: --maxChains and --minChainScore need --local\n");
        return 1;
    }
    if ((extendChains || haveChainYDrop) && !localMode) {
        fprintf(stderr, "cpecan_align: --extendChains and --chainYDrop need --local\n");
        return 1;
    }
    if (haveChainYDrop && !extendChains) {
        fprintf(stderr, "cpecan_align: --chainYDrop needs --extendChains\n");
        return 1;
    }
    if (localMode && (gapped || haveAdaptive)) {
        fprintf(stderr, "cpecan_align: --local does not go with --gapped or --adaptiveBand\n");
        return 1;
    }
    if (viterbiMode && (localMode || haveAdaptive)) {
        fprintf(stderr, "cpecan_align: --viterbi does not go with --local or --adaptiveBand\n");
        return 1;
    }
    if (argc - optind != 2) { /* cPecanAlign.c:93-96 */
        usage();
        return 1;
    }
    cpecan_model model;
    if (hmmFile) {
        cpecan_hmm hmm;
        if (cpecan_hmm_load(&hmm, hmmFile) != CPECAN_OK || cpecan_model_from_hmm(&model, &hmm) != CPECAN_OK) return fail("loadHmm");
    } else if (cpecan_model_default(&model, CPECAN_FIVE_STATE) != CPECAN_OK) { /* :100 */
        return fail("model");
    }
    cpecan_params params;
    cpecan_params_default(&params); /* :102 */
    if (expansion >= 0) params.diagonalExpansion = expansion;
    cpecan_anchor_params anchorParams;
    cpecan_anchor_params_default(&anchorParams);
    anchorParams.seedTransitions = seedTransitions;
    cpecan_anchor_options anchorOptions;
    cpecan_anchor_options_default(&anchorOptions);
    anchorOptions.transitionHspThreshold = (int32_t)transitionHspThreshold;
    anchorOptions.gappedExtension = gapped;
    anchorOptions.yDrop = (int32_t)yDrop;
    const int64_t trim = 14, anchorMatrix = 500 * 500, repeatMaskMatrix = 500 * 500; /* pairwiseAligner.c:1340-1342 */
    const double gapGamma = 0.5;                                                     /* :1345 */
    Records targets = {0}, queries = {0};
    if (read_fasta(argv[optind], &targets) != 0) {
        fprintf(stderr, "cpecan_align: cannot read %s\n", argv[optind]);
        return 1;
    }
    if (read_fasta(argv[optind + 1], &queries) != 0) {
        fprintf(stderr, "cpecan_align: cannot read %s\n", argv[optind + 1]);
        return 1;
    }
    const int64_t n = targets.n * queries.n;
    int status = 0;
    cpecan_anchor_problem *ap = calloc((size_t)(n ? n : 1), sizeof *ap);
    cpecan_problem_runs *pr = calloc((size_t)(n ? n : 1), sizeof *pr);
    int64_t **runs = calloc((size_t)(n ? n : 1), sizeof *runs), *nRuns = calloc((size_t)(n ? n : 1), sizeof *nRuns);
    cpecan_strand_result *strands = calloc((size_t)(n ? n : 1), sizeof *strands);
    int32_t *yMinus = calloc((size_t)(n ? n : 1), sizeof *yMinus);
    char **texts = calloc((size_t)(n ? n : 1), sizeof *texts);
    int64_t *idx = calloc((size_t)(n ? n : 1), sizeof *idx), *edgeSum = calloc((size_t)(n ? n : 1), sizeof *edgeSum);
    int32_t *rounds = calloc((size_t)(n ? n : 1), sizeof *rounds);
    if (!ap || !pr || !runs || !nRuns || !strands || !yMinus || !texts || !idx || !edgeSum || !rounds) status = 1;
    for (int64_t q = 0, i = 0; status == 0 && q < queries.n; q++) /* :110-114 */
        for (int64_t t = 0; t < targets.n; t++, i++) {
            ap[i].sX = targets.r[t].seq; /* :123: the target is X */
            ap[i].lX = targets.r[t].length;
            ap[i].sY = queries.r[q].seq;
            ap[i].lY = queries.r[q].length;
        }
    if (status == 0 && localMode) {
        cpecan_local_options localOptions;
        cpecan_local_options_default(&localOptions);
        localOptions.maxChains = (int32_t)maxChains;
        localOptions.minChainScore = (int32_t)minChainScore;
        if (extendChains) { /* --gapped is refused with --local: the two fields are free for the chains */
            anchorOptions.gappedExtension = 1;
            anchorOptions.yDrop = (int32_t)chainYDrop;
        }
        status = run_local(&model, ap, n, &targets, &queries, expansion, params.diagonalExpansion, gapGamma, &anchorParams,
                           haveThreshold || extendChains ? &anchorOptions : NULL, &localOptions, (int)device, strandMode, extendChains);
    }
    if (status == 0 && n > 0 && !localMode) {
        if (cpecan_find_anchor_runs_many_with_options(ap, n, trim, params.diagonalExpansion, anchorMatrix, repeatMaskMatrix,
                                                      &anchorParams, (int)device, strandMode, runs, nRuns, NULL, strands,
                                                      haveThreshold || gapped ? &anchorOptions : NULL) != CPECAN_OK)
            status = fail("anchors");
    }
    if (status == 0 && n > 0 && !localMode) {
        for (int64_t i = 0; i < n; i++) {
            pr[i].sX = ap[i].sX;
            pr[i].lX = ap[i].lX;
            pr[i].sY = ap[i].sY;
            pr[i].lY = ap[i].lY;
            pr[i].runs = runs[i];
            pr[i].nRuns = nRuns[i];
            pr[i].raggedLeft = pr[i].raggedRight = 1; /* :125 */
            yMinus[i] = strands[i].strand == CPECAN_STRAND_MINUS;
            idx[i] = i;
        }
        status = viterbiMode ? viterbi_pairs(&model, &params, (int)device, pr, yMinus, &targets, &queries, n, texts)
                             : align_pairs(&model, &params, gapGamma, (int)device, pr, yMinus, &targets, &queries, idx, n, texts,
                                           haveAdaptive ? edgeSum : NULL);
    }
    for (long long k = 1; status == 0 && k <= adaptiveBand; k++) { /* the pairs flagged in round k - 1, the expansion doubled */
        int64_t m = 0;
        for (int64_t i = 0; i < n; i++)
            if (rounds[i] == k - 1 && edgeSum[i] >= minEdgeScore) idx[m++] = i;
        if (m == 0) break;
        cpecan_params wider = params;
        wider.diagonalExpansion = params.diagonalExpansion << k;
        for (int64_t j = 0; j < m; j++) {
            for (int64_t q = 0; q < nRuns[idx[j]]; q++) runs[idx[j]][4 * q + 3] *= 2;
            rounds[idx[j]] = (int32_t)k;
        }
        status = align_pairs(&model, &wider, gapGamma, (int)device, pr, yMinus, &targets, &queries, idx, m, texts, edgeSum);
    }
    for (int64_t i = 0; status == 0 && !localMode && i < n; i++) {
        puts(texts[i]); /* :149 */
        if (haveAdaptive)
            fprintf(stderr, "cpecan_align: %s %s: round %d, expansion %lld\n", targets.r[i % targets.n].name,
                    queries.r[i / targets.n].name, (int)rounds[i], (long long)(params.diagonalExpansion << rounds[i]));
    }
    for (int64_t i = 0; texts && i < n; i++) free(texts[i]);
    free(texts);
    free(idx);
    free(edgeSum);
    free(rounds);
    for (int64_t i = 0; runs && i < n; i++) cpecan_free(runs[i]);
    free(runs);
    free(nRuns);
    free(ap);
    free(pr);
    free(strands);
    free(yMinus);
    free_records(&targets);
    free_records(&queries);
    return status;
}
