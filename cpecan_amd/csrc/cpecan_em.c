/*
 * cpecan_em.c -- expectation maximisation of the pair-HMM (include/cpecan_em.h).
 *
 * Host code only.  The E-step is cpecan_expect_set_run on alignments that stay resident on the device(s) for the whole
 * training; the M-step (sum, normalise, tie or restore the emissions, convert to the next model) is a few hundred flops.
 */
#define _POSIX_C_SOURCE 200809L
#include "cpecan_em.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cpecan_internal.h"
#include "cpecan_viterbi.h"

#define EM_PSEUDO 0.000000000001 /* hmm_constructEmpty's pseudo-count of one cPecanRealign --outputExpectations job */

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

void cpecan_em_options_default(cpecan_em_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->modelType = CPECAN_FIVE_STATE;
    o->iterations = 10;
    o->trials = 3;
    o->setJukesCantorStartingEmissions = -1.0;
    o->maxAlignmentLengthPerJob = 1000000;
    o->maxAlignmentLengthToSample = 50000000;
}

/* ------------------------------------------------------------------------------------------------
 * model operations
 * ---------------------------------------------------------------------------------------------- */
static int hmm_ok(const cpecan_hmm *h) { return h && (h->stateNumber == 5 || h->stateNumber == 3); }

int cpecan_hmm_equalise(cpecan_hmm *h) {
    if (!hmm_ok(h)) return CPECAN_EINVAL;
    const int S = h->stateNumber;
    for (int i = 0; i < S * S; i++) h->transitions[i] = 1.0 / S;
    for (int i = 0; i < S * 16; i++) h->emissions[i] = 1.0 / 16.0;
    return CPECAN_OK;
}

int cpecan_hmm_set_jukes_cantor(cpecan_hmm *h, double divergence) {
    if (!hmm_ok(h) || !(divergence >= 0.0)) return CPECAN_EINVAL;
    const double e = exp(-4.0 * divergence / 3.0);
    const double same = (0.25 + 0.75 * e) / 4.0, other = (0.25 - 0.25 * e) / 4.0;
    for (int s = 0; s < h->stateNumber; s++)
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++) h->emissions[s * 16 + x * 4 + y] = x == y ? same : other;
    return CPECAN_OK;
}

int cpecan_hmm_tie_emissions(cpecan_hmm *h) {
    if (!hmm_ok(h)) return CPECAN_EINVAL;
    for (int s = 0; s < h->stateNumber; s++) {
        double *a = h->emissions + s * 16;
        const double identity = a[0] + a[5] + a[10] + a[15];
        for (int i = 0; i < 16; i++) a[i] = (i % 4 == i / 4) ? identity / 4.0 : (1.0 - identity) / 12.0;
    }
    return CPECAN_OK;
}

double cpecan_em_random(uint64_t *state) {
    uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

int cpecan_hmm_randomise(cpecan_hmm *h, uint64_t *state) {
    if (!hmm_ok(h) || !state) return CPECAN_EINVAL;
    const int S = h->stateNumber;
    for (int i = 0; i < S * S; i++) h->transitions[i] = cpecan_em_random(state);
    for (int i = 0; i < S * 16; i++) h->emissions[i] = cpecan_em_random(state);
    return cpecan_hmm_normalise(h);
}

/* ------------------------------------------------------------------------------------------------
 * sampling
 * ---------------------------------------------------------------------------------------------- */
static double cigar_length(const cpecan_cigar *c) {
    return (double)(llabs((long long)(c->start1 - c->end1)) + llabs((long long)(c->start2 - c->end2))) / 2.0;
}

int cpecan_em_sample(const cpecan_cigar *in, int64_t n, int64_t maxPerJob, int64_t maxToSample, uint64_t seed,
                     int64_t *order, int64_t *nOut, int64_t *nJobs, double *length) {
    if ((!in && n > 0) || n < 0 || !order || !nOut || !nJobs || maxPerJob < 0 || maxToSample < 0) return CPECAN_EINVAL;
    /* jobs: [first[j], first[j + 1]) with their lengths */
    int64_t *first = malloc(sizeof(int64_t) * (size_t)(n + 1));
    double *len = malloc(sizeof(double) * (size_t)(n + 1));
    int64_t *perm = malloc(sizeof(int64_t) * (size_t)(n + 1));
    if (!first || !len || !perm) {
        free(first);
        free(len);
        free(perm);
        return CPECAN_ENOMEM;
    }
    int64_t jobs = 0;
    double run = 0.0;
    first[0] = 0;
    for (int64_t i = 0; i < n; i++) {
        run += cigar_length(&in[i]);
        if (run > (double)maxPerJob || i == n - 1) { /* the job closes after this cigar */
            len[jobs] = run;
            first[++jobs] = i + 1;
            run = 0.0;
        }
    }
    uint64_t state = seed;
    for (int64_t j = 0; j < jobs; j++) perm[j] = j;
    for (int64_t j = jobs - 1; j > 0; j--) { /* Fisher-Yates */
        const int64_t k = (int64_t)(cpecan_em_random(&state) * (double)(j + 1));
        const int64_t tmp = perm[j];
        perm[j] = perm[k];
        perm[k] = tmp;
    }
    int64_t at = 0, taken = 0;
    double total = 0.0;
    for (int64_t j = 0; j < jobs; j++) {
        const int64_t job = perm[j];
        for (int64_t i = first[job]; i < first[job + 1]; i++) order[at++] = i;
        total += len[job];
        taken++;
        if (total >= (double)maxToSample) break;
    }
    *nOut = at;
    *nJobs = taken;
    if (length) *length = total;
    free(first);
    free(len);
    free(perm);
    return CPECAN_OK;
}

/* ------------------------------------------------------------------------------------------------
 * blast / lastz scoring matrix
 * ---------------------------------------------------------------------------------------------- */
int cpecan_em_blast_matrix(const cpecan_hmm *h, double gcFraction, double matchScores[16], double *gapOpen,
                           double *gapExtend) {
    if (!hmm_ok(h) || !matchScores || !gapOpen || !gapExtend) return CPECAN_EINVAL;
    /* the first three states (match, short gap X, short gap Y) as a three-state model, normalised */
    cpecan_hmm t;
    cpecan_hmm_init(&t, CPECAN_THREE_STATE, 0.0);
    for (int from = 0; from < 3; from++)
        for (int to = 0; to < 3; to++) t.transitions[from * 3 + to] = h->transitions[from * h->stateNumber + to];
    memcpy(t.emissions, h->emissions, sizeof(double) * 48);
    cpecan_hmm_normalise(&t);
    const double *tr = t.transitions;
    double base[4];
    for (int x = 0; x < 4; x++) base[x] = (x == 1 || x == 2) ? gcFraction / 2.0 : (1.0 - gcFraction) / 2.0;
    const double matchContinue = tr[0];
    double prob[16], logSum = 0.0;
    for (int x = 0; x < 4; x++)
        for (int y = 0; y < 4; y++) {
            prob[x * 4 + y] = t.emissions[x * 4 + y] / (base[x] * base[y]);
            logSum += log(prob[x * 4 + y] * matchContinue);
        }
    /* 6.94: a hundredth of the sum of lastz's default scoring matrix */
    const double nProb = sqrt(exp((6.94 + logSum) / 16.0)), n2 = nProb * nProb;
    const double weight = 100.0;
    for (int i = 0; i < 16; i++) matchScores[i] = weight * log(prob[i] * matchContinue / n2);
    *gapOpen = weight * log((0.5 * (tr[1] / nProb + tr[2] / nProb)) * ((tr[3] + tr[6]) / (2.0 * n2)) * (n2 / matchContinue));
    *gapExtend = weight * log(0.5 * (tr[4] / nProb + tr[8] / nProb));
    return CPECAN_OK;
}

int cpecan_em_write_lastz_matrix(const char *path, const double matchScores[16], double gapOpen, double gapExtend) {
    if (!path || !matchScores) return CPECAN_EINVAL;
    FILE *f = fopen(path, "w");
    if (!f) {
        cpk_set_error("cannot write %s", path);
        return CPECAN_EINVAL;
    }
    const char *bases = "ACGT";
    fprintf(f, "gap_open_penalty = %lld\n", (long long)round(-gapOpen));
    fprintf(f, "gap_extend_penalty = %lld\n", (long long)round(-gapExtend));
    fprintf(f, "\t\tA\tC\tG\tT\n");
    for (int x = 0; x < 4; x++) {
        fprintf(f, "\t%c", bases[x]);
        for (int y = 0; y < 4; y++) fprintf(f, "\t%lld", (long long)round(matchScores[x * 4 + y]));
        fprintf(f, "\n");
    }
    return fclose(f) == 0 ? CPECAN_OK : CPECAN_EINVAL;
}

int64_t cpecan_em_fasta_gc(const char *path, int64_t *gc, int64_t *total) {
    if (!path || !gc || !total) return CPECAN_EINVAL;
    FILE *f = fopen(path, "r");
    if (!f) {
        cpk_set_error("cannot open %s", path);
        return CPECAN_EINVAL;
    }
    char *line = NULL;
    size_t cap = 0;
    int64_t records = 0;
    int inRecord = 0;
    for (ssize_t got; (got = getline(&line, &cap, f)) >= 0;) {
        if (line[0] == '>') {
            records++;
            inRecord = 1;
            continue;
        }
        if (!inRecord) continue;
        for (ssize_t i = 0; i < got; i++) {
            const char c = line[i];
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f') continue;
            (*total)++;
            if (c == 'G' || c == 'C') (*gc)++;
        }
    }
    free(line);
    fclose(f);
    return records;
}

int cpecan_em_write_model(const cpecan_hmm *h, const double *running, int nRunning, const char *path) {
    if (!hmm_ok(h) || !path || nRunning < 0 || (nRunning > 0 && !running)) return CPECAN_EINVAL;
    FILE *f = fopen(path, "w");
    if (!f) {
        cpk_set_error("cannot write %s", path);
        return CPECAN_EINVAL;
    }
    const int S = h->stateNumber;
    fprintf(f, "%d", h->type);
    for (int i = 0; i < S * S; i++) fprintf(f, " %.17g", h->transitions[i]);
    fprintf(f, " %.17g\n", h->likelihood);
    for (int i = 0; i < S * 16; i++) fprintf(f, "%s%.17g", i ? " " : "", h->emissions[i]);
    fprintf(f, "\n");
    for (int i = 0; i < nRunning; i++) fprintf(f, "%s%.17g", i ? "\t" : "", running[i]);
    if (nRunning > 0) fprintf(f, "\n");
    return fclose(f) == 0 ? CPECAN_OK : CPECAN_EINVAL;
}

/* ------------------------------------------------------------------------------------------------
 * the trainer
 * ---------------------------------------------------------------------------------------------- */
struct cpecan_em_trainer {
    cpecan_em_options opt;
    char *inputModel, *blastFile;
    int32_t type;
    cpecan_hmm input; /* inputModel, normalised */
    cpecan_realigner *r;
    char **fastas;
    int nFastas;
    cpecan_em_timing timing;
    int concurrentTrials; /* cpecan_em_trainer_set_concurrent_trials: trials per launch (1: one after another) */
    /* cpecan_em_trainer_alignments: the anchors of the last E-step of the last trial (malloc'd; NULL before a training) */
    int64_t *lastRuns, *lastNRuns;
    int64_t lastN;
    /* cpecan_em_trainer_set_viterbi_training: the E-step counts along the most probable paths */
    int viterbiTraining;
    double viterbiPseudoCount;
};

static char *dup_str(const char *s) {
    if (!s) return NULL;
    const size_t n = strlen(s) + 1;
    char *t = malloc(n);
    if (t) memcpy(t, s, n);
    return t;
}

int cpecan_em_trainer_create(cpecan_em_trainer **out, const cpecan_em_options *o, const cpecan_realign_options *ro,
                             int device) {
    if (!out || !o || !ro) return CPECAN_EINVAL;
    *out = NULL;
    if (o->iterations < 0 || o->trials < 1 || o->maxAlignmentLengthPerJob < 0 || o->maxAlignmentLengthToSample < 0) {
        cpk_set_error("bad EM option (iterations >= 0, trials >= 1, lengths >= 0)");
        return CPECAN_EINVAL;
    }
    cpecan_em_trainer *t = calloc(1, sizeof *t);
    if (!t) return CPECAN_ENOMEM;
    t->opt = *o;
    t->inputModel = dup_str(o->inputModel);
    t->blastFile = dup_str(o->blastScoringMatrixFile);
    t->opt.inputModel = t->inputModel;
    t->opt.blastScoringMatrixFile = t->blastFile;
    t->type = o->modelType;
    t->concurrentTrials = 1;
    int rc = CPECAN_OK;
    if (t->inputModel) {
        if (cpecan_hmm_load(&t->input, t->inputModel) != CPECAN_OK) {
            cpk_set_error("cannot load the input model %s", t->inputModel);
            rc = CPECAN_EINVAL;
        } else {
            cpecan_hmm_normalise(&t->input);
            t->type = t->input.type;
        }
    }
    cpecan_model start;
    if (rc == CPECAN_OK && cpecan_model_default(&start, t->type) != CPECAN_OK) {
        cpk_set_error("unknown model type %d", t->type);
        rc = CPECAN_EINVAL;
    }
    if (rc == CPECAN_OK) rc = cpecan_realigner_create(&t->r, &start, ro, device);
    if (rc != CPECAN_OK) {
        cpecan_em_trainer_destroy(t);
        return rc;
    }
    *out = t;
    return CPECAN_OK;
}

void cpecan_em_trainer_destroy(cpecan_em_trainer *t) {
    if (!t) return;
    cpecan_realigner_destroy(t->r);
    for (int i = 0; i < t->nFastas; i++) free(t->fastas[i]);
    free(t->fastas);
    free(t->inputModel);
    free(t->blastFile);
    free(t->lastRuns);
    free(t->lastNRuns);
    free(t);
}

int64_t cpecan_em_trainer_read_fasta(cpecan_em_trainer *t, const char *path) {
    if (!t || !path) return CPECAN_EINVAL;
    const int64_t n = cpecan_realigner_read_fasta(t->r, path);
    if (n < 0) return n;
    char **grown = realloc(t->fastas, sizeof(char *) * (size_t)(t->nFastas + 1));
    if (!grown) return CPECAN_ENOMEM;
    t->fastas = grown;
    if (!(t->fastas[t->nFastas] = dup_str(path))) return CPECAN_ENOMEM;
    t->nFastas++;
    return n;
}

int cpecan_em_trainer_add_sequence(cpecan_em_trainer *t, const char *header, const char *seq, int64_t length) {
    if (!t) return CPECAN_EINVAL;
    return cpecan_realigner_add_sequence(t->r, header, seq, length);
}

int cpecan_em_trainer_set_devices(cpecan_em_trainer *t, const int *devices, int nDevices) {
    if (!t) return CPECAN_EINVAL;
    return cpecan_realigner_set_devices(t->r, devices, nDevices);
}

int cpecan_em_trainer_set_concurrent_trials(cpecan_em_trainer *t, int n) {
    if (!t) return CPECAN_EINVAL;
    if (n < 1 || n > CPECAN_MAX_MODEL_SLOTS) {
        cpk_set_error("concurrent trials: %d, 1 to %d are possible", n, CPECAN_MAX_MODEL_SLOTS);
        return CPECAN_EINVAL;
    }
    if (n > 1 && t->opt.updateTheBand) {
        cpk_set_error("updateTheBand with %d concurrent trials: the trials' bands differ, one resident batch cannot serve them", n);
        return CPECAN_EINVAL;
    }
    t->concurrentTrials = n;
    return CPECAN_OK;
}

/* What Viterbi training does not go with; checked where it is switched on and again where a training starts, before any
 * device is looked for. */
static int viterbi_training_refusal(const cpecan_em_trainer *t) {
    if (!t->viterbiTraining) return CPECAN_OK;
    if (t->opt.updateTheBand) {
        cpk_set_error("Viterbi training does not go with updateTheBand: the realignment between iterations is not built for it");
        return CPECAN_EINVAL;
    }
    if (t->concurrentTrials > 1) {
        cpk_set_error("Viterbi training with %d concurrent trials: one resident Viterbi object serves one model at a time", t->concurrentTrials);
        return CPECAN_EINVAL;
    }
    if (cpk_realigner_device_count(t->r) > 1) {
        cpk_set_error("Viterbi training on %d devices: the resident Viterbi object lives on one", cpk_realigner_device_count(t->r));
        return CPECAN_EINVAL;
    }
    return CPECAN_OK;
}

int cpecan_em_trainer_set_viterbi_training(cpecan_em_trainer *t, int on, double pseudoCount) {
    if (!t) return CPECAN_EINVAL;
    if (!isfinite(pseudoCount) || pseudoCount < 0.0) {
        cpk_set_error("Viterbi training: a pseudo-count of %g, it must be finite and >= 0", pseudoCount);
        return CPECAN_EINVAL;
    }
    const int before = t->viterbiTraining;
    t->viterbiTraining = on != 0;
    const int rc = viterbi_training_refusal(t);
    if (rc != CPECAN_OK) {
        t->viterbiTraining = before;
        return rc;
    }
    t->viterbiPseudoCount = pseudoCount;
    return CPECAN_OK;
}

int cpecan_em_trainer_timing(const cpecan_em_trainer *t, cpecan_em_timing *out) {
    if (!t || !out) return CPECAN_EINVAL;
    *out = t->timing;
    return CPECAN_OK;
}

/* The start model of a trial (expectationMaximisation): the input model, or random / equal probabilities, then the
 * Jukes-Cantor emissions if asked for. */
static int start_model(cpecan_em_trainer *t, uint64_t *rng, cpecan_hmm *h) {
    int rc;
    if (t->inputModel) {
        *h = t->input;
        rc = CPECAN_OK;
    } else {
        rc = cpecan_hmm_init(h, t->type, 0.0);
        if (rc == CPECAN_OK) rc = t->opt.randomStart ? cpecan_hmm_randomise(h, rng) : cpecan_hmm_equalise(h);
    }
    h->likelihood = 0.0;
    if (rc == CPECAN_OK && t->opt.setJukesCantorStartingEmissions >= 0.0)
        rc = cpecan_hmm_set_jukes_cantor(h, t->opt.setJukesCantorStartingEmissions);
    return rc;
}

int cpecan_em_trainer_alignments(const cpecan_em_trainer *t, const int64_t **runs, const int64_t **nRuns, int64_t *n) {
    if (!t || !runs || !nRuns || !n) return CPECAN_EINVAL;
    if (!t->lastRuns || !t->lastNRuns) {
        cpk_set_error("no training with updateTheBand yet");
        return CPECAN_ESTATE;
    }
    *runs = t->lastRuns;
    *nRuns = t->lastNRuns;
    *n = t->lastN;
    return CPECAN_OK;
}

static void keep_alignments(cpecan_em_trainer *t, int64_t *runs, int64_t *nRuns, int64_t n) {
    free(t->lastRuns);
    free(t->lastNRuns);
    t->lastRuns = runs;
    t->lastNRuns = nRuns;
    t->lastN = n;
}

/* The M-step of one trial from its E-step's counts (calculateMaximisation). */
static void m_step(const cpecan_em_trainer *t, cpecan_hmm *acc, cpecan_hmm *h, double *running) {
    cpecan_hmm_normalise(acc);
    *running = acc->likelihood;
    if (!t->opt.trainEmissions)
        memcpy(acc->emissions, h->emissions, sizeof acc->emissions);
    else if (t->opt.tieEmissions)
        cpecan_hmm_tie_emissions(acc);
    *h = *acc;
}

/* One trial: `iterations` E- and M-steps from h, the model file rewritten after every one (calculateMaximisation).  With
 * updateTheBand the sample is realigned between two iterations under the model of the M-step and the next E-step runs on
 * an EXPECT set planned for the new anchors; without it nothing of that runs.  first: the set of the sampled cigars' own
 * anchors, which every trial starts from. */
static int run_trial(cpecan_em_trainer *t, cpecan_expect_set *first, const cpecan_cigar *sample, int64_t nSample,
                     int64_t nJobs, cpecan_hmm *h, double *running, const char *path, int *reanchoredOut) {
    int rc = cpecan_em_write_model(h, NULL, 0, path);
    cpecan_model m;
    if (rc == CPECAN_OK)
        rc = t->opt.useDefaultModelAsStart ? cpecan_model_default(&m, t->type) : cpecan_model_from_hmm(&m, h);
    cpecan_expect_set *own = NULL, *set = first;
    int reanchored = 0;
    int64_t *curRuns = NULL, *curNRuns = NULL; /* the anchors `set` runs on; NULL: the sampled cigars' own */
    for (int it = 0; rc == CPECAN_OK && it < t->opt.iterations; it++) {
        cpecan_hmm acc;
        /* one pseudo-count per job, as one cPecanRealign --outputExpectations run per job adds it */
        rc = cpecan_hmm_init(&acc, t->type, EM_PSEUDO * (double)(nJobs > 0 ? nJobs : 1));
        if (rc == CPECAN_OK) rc = cpecan_expect_set_run(set, &m, &acc);
        if (rc != CPECAN_OK) break;
        m_step(t, &acc, h, &running[it]);
        rc = cpecan_em_write_model(h, NULL, 0, path);
        if (rc == CPECAN_OK) rc = cpecan_model_from_hmm(&m, h);
        if (rc != CPECAN_OK || !t->opt.updateTheBand || it + 1 >= t->opt.iterations) continue;
        int64_t *runs = NULL, *nRuns = NULL;
        const double t0 = now_ms();
        rc = cpecan_realigner_set_model(t->r, &m);
        /* the realigned cigars replace the alignments (cPecanEm.py:212-215): from the second realignment on the band is
         * that of the realignment before, not the sample's */
        if (rc == CPECAN_OK) rc = cpecan_realigner_reanchor_runs(t->r, sample, nSample, curRuns, curNRuns, &runs, &nRuns);
        const double t1 = now_ms();
        if (rc == CPECAN_OK) {
            cpecan_expect_set_destroy(own); /* (its memory goes back to the pool the new set is taken from) */
            own = NULL;
            rc = cpecan_expect_set_create_runs(&own, t->r, sample, nSample, runs, nRuns);
            set = own;
        }
        t->timing.realignMs += t1 - t0;
        t->timing.handoffMs += cpk_realigner_reanchor_ms(t->r);
        t->timing.replanMs += now_ms() - t1;
        if (rc == CPECAN_OK) {
            free(curRuns);
            free(curNRuns);
            curRuns = runs;
            curNRuns = nRuns;
            reanchored = 1;
        } else {
            free(runs);
            free(nRuns);
        }
    }
    cpecan_expect_set_destroy(own);
    if (rc == CPECAN_OK && reanchored) {
        keep_alignments(t, curRuns, curNRuns, nSample);
    } else {
        free(curRuns);
        free(curNRuns);
    }
    *reanchoredOut = reanchored; /* 0: the last E-step ran on the sample's own anchors */
    if (rc == CPECAN_OK) rc = cpecan_em_write_model(h, running, t->opt.iterations, path);
    return rc;
}

/* One trial of Viterbi training (hard EM): run_trial, except that the E-step decodes the most probable path of every sampled
 * alignment under the current model and counts along it (cpecan_viterbi_run_counts over the resident object vit), on top of
 * the pseudo-count in every bin.  The running likelihood is the sum of the paths' log-probabilities. */
static int run_trial_viterbi(cpecan_em_trainer *t, cpecan_viterbi *vit, cpecan_hmm *h, double *running, const char *path) {
    int rc = cpecan_em_write_model(h, NULL, 0, path);
    cpecan_model m;
    if (rc == CPECAN_OK)
        rc = t->opt.useDefaultModelAsStart ? cpecan_model_default(&m, t->type) : cpecan_model_from_hmm(&m, h);
    for (int it = 0; rc == CPECAN_OK && it < t->opt.iterations; it++) {
        cpecan_hmm acc;
        cpecan_viterbi_counts counts;
        rc = cpecan_hmm_init(&acc, t->type, t->viterbiPseudoCount);
        if (rc == CPECAN_OK) rc = cpecan_viterbi_set_model(vit, &m);
        if (rc == CPECAN_OK) rc = cpecan_viterbi_run_counts(vit, &counts);
        if (rc == CPECAN_OK) rc = cpecan_viterbi_counts_add_to_hmm(&counts, &acc);
        if (rc != CPECAN_OK) break;
        m_step(t, &acc, h, &running[it]);
        rc = cpecan_em_write_model(h, NULL, 0, path);
        if (rc == CPECAN_OK) rc = cpecan_model_from_hmm(&m, h);
    }
    if (rc == CPECAN_OK) rc = cpecan_em_write_model(h, running, t->opt.iterations, path);
    return rc;
}

/* A round of n trials side by side: every iteration is ONE cpecan_expect_set_run_models over the round's models plus the
 * M-step of each -- what run_trial does for one trial, file for file. */
static int run_round(cpecan_em_trainer *t, cpecan_expect_set *set, int64_t nJobs, cpecan_hmm *hmms, int n, double *runs,
                     int iters, char **paths) {
    cpecan_model ms[CPECAN_MAX_MODEL_SLOTS];
    cpecan_hmm accs[CPECAN_MAX_MODEL_SLOTS];
    int rc = CPECAN_OK;
    for (int j = 0; rc == CPECAN_OK && j < n; j++) {
        rc = cpecan_em_write_model(&hmms[j], NULL, 0, paths[j]);
        if (rc == CPECAN_OK)
            rc = t->opt.useDefaultModelAsStart ? cpecan_model_default(&ms[j], t->type) : cpecan_model_from_hmm(&ms[j], &hmms[j]);
    }
    for (int it = 0; rc == CPECAN_OK && it < iters; it++) {
        for (int j = 0; rc == CPECAN_OK && j < n; j++)
            rc = cpecan_hmm_init(&accs[j], t->type, EM_PSEUDO * (double)(nJobs > 0 ? nJobs : 1));
        if (rc == CPECAN_OK) rc = cpecan_expect_set_run_models(set, ms, n, accs);
        for (int j = 0; rc == CPECAN_OK && j < n; j++) {
            m_step(t, &accs[j], &hmms[j], &runs[(size_t)j * (size_t)iters + it]);
            rc = cpecan_em_write_model(&hmms[j], NULL, 0, paths[j]);
            if (rc == CPECAN_OK) rc = cpecan_model_from_hmm(&ms[j], &hmms[j]);
        }
    }
    for (int j = 0; rc == CPECAN_OK && j < n; j++)
        rc = cpecan_em_write_model(&hmms[j], runs + (size_t)j * (size_t)iters, iters, paths[j]);
    return rc;
}

int cpecan_em_train(cpecan_em_trainer *t, const cpecan_cigar *in, int64_t n, const char *outputModel, cpecan_hmm *best,
                    double *running) {
    if (!t || (!in && n > 0) || n < 0 || !outputModel) return CPECAN_EINVAL;
    if (t->opt.updateTheBand && t->concurrentTrials > 1) {
        cpk_set_error("updateTheBand with %d concurrent trials: the trials' bands differ, one resident batch cannot serve them",
                      t->concurrentTrials);
        return CPECAN_EINVAL;
    }
    if (viterbi_training_refusal(t) != CPECAN_OK) return CPECAN_EINVAL;
    keep_alignments(t, NULL, NULL, 0);
    const double t0 = now_ms();
    memset(&t->timing, 0, sizeof t->timing);
    const int iters = t->opt.iterations;
    const int trials = (!t->inputModel && t->opt.randomStart) ? t->opt.trials : 1;
    const int conc = t->concurrentTrials < trials ? t->concurrentTrials : trials; /* trials per launch */
    int64_t *order = malloc(sizeof(int64_t) * (size_t)(n ? n : 1));
    cpecan_cigar *sample = malloc(sizeof(cpecan_cigar) * (size_t)(n ? n : 1));
    double *runs = calloc((size_t)trials * (size_t)(iters ? iters : 1), sizeof(double));
    cpecan_hmm *hmms = calloc((size_t)trials, sizeof(cpecan_hmm));
    char *path = malloc(strlen(outputModel) + 32);
    int rc = (order && sample && runs && hmms && path) ? CPECAN_OK : CPECAN_ENOMEM;
    int64_t nSample = 0, nJobs = 0;
    if (rc == CPECAN_OK)
        rc = cpecan_em_sample(in, n, t->opt.maxAlignmentLengthPerJob, t->opt.maxAlignmentLengthToSample, t->opt.seed,
                              order, &nSample, &nJobs, NULL);
    cpecan_expect_set *set = NULL;
    cpecan_viterbi *vit = NULL;
    for (int64_t i = 0; rc == CPECAN_OK && i < nSample; i++) sample[i] = in[order[i]]; /* shallow copies: nothing is freed through them */
    if (rc == CPECAN_OK && t->viterbiTraining) { /* planned here; its inputs go to the device with the first E-step and stay */
        cpecan_model any;
        rc = cpecan_model_default(&any, t->type);
        if (rc == CPECAN_OK) rc = cpk_realigner_viterbi_create(t->r, &any, sample, nSample, &vit);
    } else if (rc == CPECAN_OK) {
        rc = cpecan_expect_set_reserve_models(t->r, conc > 1 ? conc : 0);
        if (rc == CPECAN_OK) rc = cpecan_expect_set_create(&set, t->r, sample, nSample);
    }
    uint64_t rng = t->opt.seed ^ 0x5DEECE66Dull; /* the random starts: a stream of their own, from the same seed */
    const double t1 = now_ms();
    int bestTrial = 0, reanchored = 0;
    if (conc > 1) {
        /* every start model first, in trial order, from the same generator state (the trials' iterations draw nothing):
         * trial k starts where it starts in a sequential run.  Then rounds of up to `conc` trials. */
        char *paths[CPECAN_MAX_MODEL_SLOTS] = {0};
        for (int k = 0; rc == CPECAN_OK && k < trials; k++) rc = start_model(t, &rng, &hmms[k]);
        for (int j = 0; rc == CPECAN_OK && j < conc; j++)
            if (!(paths[j] = malloc(strlen(outputModel) + 32))) rc = CPECAN_ENOMEM;
        for (int k0 = 0; rc == CPECAN_OK && k0 < trials; k0 += conc) {
            const int nr = trials - k0 < conc ? trials - k0 : conc;
            for (int j = 0; j < nr; j++) sprintf(paths[j], t->opt.outputTrialHmms ? "%s_%d" : "%s.trial_%d", outputModel, k0 + j);
            rc = run_round(t, set, nJobs, hmms + k0, nr, runs + (size_t)k0 * (size_t)iters, iters, paths);
            for (int j = 0; j < nr; j++) {
                if (!t->opt.outputTrialHmms) remove(paths[j]);
                if (rc == CPECAN_OK && hmms[k0 + j].likelihood > hmms[bestTrial].likelihood) bestTrial = k0 + j;
            }
        }
        for (int j = 0; j < conc; j++) free(paths[j]);
    }
    for (int k = 0; conc <= 1 && rc == CPECAN_OK && k < trials; k++) {
        rc = start_model(t, &rng, &hmms[k]);
        if (rc != CPECAN_OK) break;
        if (trials == 1) strcpy(path, outputModel);
        else if (t->opt.outputTrialHmms) sprintf(path, "%s_%d", outputModel, k);
        else sprintf(path, "%s.trial_%d", outputModel, k);
        if (t->viterbiTraining) rc = run_trial_viterbi(t, vit, &hmms[k], runs + (size_t)k * (size_t)iters, path);
        else rc = run_trial(t, set, sample, nSample, nJobs, &hmms[k], runs + (size_t)k * (size_t)iters, path, &reanchored);
        if (trials > 1 && !t->opt.outputTrialHmms) remove(path);
        if (rc == CPECAN_OK && hmms[k].likelihood > hmms[bestTrial].likelihood) bestTrial = k;
    }
    if (rc == CPECAN_OK && t->opt.updateTheBand && !reanchored) { /* the last trial never left the sample's own anchors */
        int64_t *sampleRuns = NULL, *sampleNRuns = NULL;
        rc = cpk_realigner_cigar_runs(t->r, sample, nSample, &sampleRuns, &sampleNRuns);
        if (rc == CPECAN_OK) keep_alignments(t, sampleRuns, sampleNRuns, nSample);
    }
    const double t2 = now_ms();
    if (rc == CPECAN_OK && trials > 1) /* expectationMaximisationTrials2: the trial with the highest likelihood */
        rc = cpecan_em_write_model(&hmms[bestTrial], runs + (size_t)bestTrial * (size_t)iters, iters, outputModel);
    if (rc == CPECAN_OK && t->blastFile) {
        int64_t gc = 0, total = 0;
        for (int i = 0; rc == CPECAN_OK && i < t->nFastas; i++)
            if (cpecan_em_fasta_gc(t->fastas[i], &gc, &total) < 0) rc = CPECAN_EINVAL;
        double scores[16], gapOpen = 0.0, gapExtend = 0.0;
        if (rc == CPECAN_OK && total == 0) {
            cpk_set_error("blastScoringMatrixFile: the sequences hold no bases");
            rc = CPECAN_EINVAL;
        }
        if (rc == CPECAN_OK) rc = cpecan_em_blast_matrix(&hmms[bestTrial], (double)gc / (double)total, scores, &gapOpen, &gapExtend);
        if (rc == CPECAN_OK) rc = cpecan_em_write_lastz_matrix(t->blastFile, scores, gapOpen, gapExtend);
    }
    if (rc != CPECAN_OK) keep_alignments(t, NULL, NULL, 0);
    if (rc == CPECAN_OK) {
        if (best) *best = hmms[bestTrial];
        if (running && iters > 0) memcpy(running, runs + (size_t)bestTrial * (size_t)iters, sizeof(double) * (size_t)iters);
        t->timing.setupMs = t1 - t0;
        t->timing.iterationsMs = t2 - t1;
        t->timing.iterations = (int64_t)iters * trials;
        t->timing.cigars = nSample;
        t->timing.jobs = nJobs;
    }
    cpecan_expect_set_destroy(set);
    cpecan_viterbi_destroy(vit);
    free(order);
    free(sample);
    free(runs);
    free(hmms);
    free(path);
    return rc;
}
