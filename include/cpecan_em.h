/*
 * cpecan_em.h -- pair-HMM training by expectation maximisation (cPecanEm.py: expectationMaximisation*,
 * calculateMaximisation, makeBlastScoringMatrix, writeLastzScoringMatrix) on top of the realign front end.
 *
 * The sampled alignments are prepared, planned and uploaded ONCE as resident EXPECT batches (cpecan_expect_set_*, one per
 * device shard); every iteration swaps the model of those batches (cpecan_batch_set_model), runs only the kernels and does
 * the M-step on the host.  The reference runs one cPecanRealign --outputExpectations process per job and iteration
 * instead.  Random-restart trials run one after another on the same resident batches, or -- after
 * cpecan_em_trainer_set_concurrent_trials(t, n) -- in rounds of up to n side by side: the batches reserve n model slots
 * (cpecan_batch_reserve_models, cpecan_hip.h) and an iteration of a round is ONE launch per shard for all its trials.
 *
 * Model files are written as cPecanEm.py's Hmm.write does -- "type t_0 .. t_{S*S-1} likelihood", then the S*16
 * emissions, then (after the last iteration) the running likelihoods, tab separated -- with every number printed to 17
 * significant digits.  cpecan_hmm_load and cpecan_realign --loadHmm read them unchanged (they ignore the third line).
 */
#ifndef CPECAN_EM_H_
#define CPECAN_EM_H_

#include "cpecan_realign.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cPecanEm.py's options (class Options, addExpectationMaximisationOptions) with its defaults. */
typedef struct cpecan_em_options {
    int32_t modelType;              /* CPECAN_FIVE_STATE; ignored with inputModel (the file's type is used) */
    int32_t iterations;             /* 10 */
    int32_t trials;                 /* 3, used only with randomStart and no inputModel */
    int32_t randomStart;            /* 0: the start model has all probabilities equal (Hmm.equalise) */
    int32_t useDefaultModelAsStart; /* 0; 1: iteration 0 runs the type's default state machine, not the start model */
    int32_t trainEmissions;         /* 0: the previous model's emissions are put back after normalising */
    int32_t tieEmissions;           /* 0; only with trainEmissions */
    int32_t outputTrialHmms;        /* 0; 1: trial i's final model is also written to <outputModel>_<i> */
    double setJukesCantorStartingEmissions; /* < 0: none; else the substitutions per site of the starting emissions */
    int64_t maxAlignmentLengthPerJob;       /* 1000000 */
    int64_t maxAlignmentLengthToSample;     /* 50000000 */
    uint64_t seed;                          /* drives the shuffle of the jobs and randomise; 0 */
    const char *inputModel;                 /* NULL */
    const char *blastScoringMatrixFile;     /* NULL */
    int32_t updateTheBand;                  /* 0; 1: after every M-step but the last the sample is realigned under the new
                                             * model with the realign options, and the next E-step runs on the new anchors */
} cpecan_em_options;
void cpecan_em_options_default(cpecan_em_options *o);

/* ---- the model operations of cPecanEm.py's Hmm (rows of the result sum to 1) ---- */
int cpecan_hmm_equalise(cpecan_hmm *h);                         /* Hmm.equalise */
int cpecan_hmm_set_jukes_cantor(cpecan_hmm *h, double divergence); /* Hmm.setEmissionsToJukesCantor */
int cpecan_hmm_tie_emissions(cpecan_hmm *h);                    /* Hmm.tieEmissions */
/* Hmm.randomise: every transition and emission uniform in [0, 1) from *state (splitmix64), then normalised. */
int cpecan_hmm_randomise(cpecan_hmm *h, uint64_t *state);
/* A uniform double in [0, 1) from *state (splitmix64): the generator of cpecan_hmm_randomise and of the job shuffle. */
double cpecan_em_random(uint64_t *state);

/* ---- sampling (expectationMaximisation) ----
 * Cuts the n cigars, in order, into jobs: a job closes after the cigar that takes its alignment length -- the sum of
 * (|end1 - start1| + |end2 - start2|) / 2 -- above maxPerJob.  The jobs are shuffled with `seed` (Fisher-Yates on
 * cpecan_em_random) and taken until their total length reaches maxToSample.  order receives the indices of the sampled
 * cigars (room for n), job by job; *nOut their count, *nJobs the number of sampled jobs, *length their total length. */
int cpecan_em_sample(const cpecan_cigar *in, int64_t n, int64_t maxPerJob, int64_t maxToSample, uint64_t seed,
                     int64_t *order, int64_t *nOut, int64_t *nJobs, double *length);

/* ---- makeBlastScoringMatrix + writeLastzScoringMatrix ----
 * The first three states of h as a three-state model, the match emissions against base frequencies from gcFraction, as
 * lastz scores: matchScores[x*4+y], gapOpen, gapExtend (unrounded).  _write prints them as writeLastzScoringMatrix. */
int cpecan_em_blast_matrix(const cpecan_hmm *h, double gcFraction, double matchScores[16], double *gapOpen,
                           double *gapExtend);
int cpecan_em_write_lastz_matrix(const char *path, const double matchScores[16], double gapOpen, double gapExtend);
/* Fraction of 'G' and 'C' (upper case, as the reference counts) over every record of a fasta file; *gc and *total are
 * added to.  Returns the number of records or < 0. */
int64_t cpecan_em_fasta_gc(const char *path, int64_t *gc, int64_t *total);

/* A model file as described above; running may be NULL (nRunning 0: no third line). */
int cpecan_em_write_model(const cpecan_hmm *h, const double *running, int nRunning, const char *path);

/* ---- the trainer ---- */
typedef struct cpecan_em_trainer cpecan_em_trainer;
/* Loads inputModel (CPECAN_EINVAL with a message for a file that cannot be read) and fixes the model type. */
int cpecan_em_trainer_create(cpecan_em_trainer **out, const cpecan_em_options *o, const cpecan_realign_options *ro,
                             int device);
void cpecan_em_trainer_destroy(cpecan_em_trainer *t);
/* The sequences the cigars refer to (cpecan_realigner_read_fasta); returns the number of records or < 0. */
int64_t cpecan_em_trainer_read_fasta(cpecan_em_trainer *t, const char *path);
int cpecan_em_trainer_add_sequence(cpecan_em_trainer *t, const char *header, const char *seq, int64_t length);
/* One resident shard per listed device (cpecan_realigner_set_devices); the shards' counts are summed on the host. */
int cpecan_em_trainer_set_devices(cpecan_em_trainer *t, const int *devices, int nDevices);
/* Trials per launch, 1 .. CPECAN_MAX_MODEL_SLOTS; 1 (the default): one trial after another.  With n > 1 cpecan_em_train
 * draws every start model first, in trial order (trial k starts from the model it starts from in a sequential run), and
 * runs the trials in rounds of up to n: an iteration of a round is one cpecan_expect_set_run_models plus the M-step of
 * each trial.  Trial files, outputTrialHmms, the choice of the best trial, running likelihoods and timing are the same. */
/* With updateTheBand n > 1 is CPECAN_EINVAL with a message, here and in cpecan_em_train, before any device is looked
 * for: the trials' bands differ, so one resident batch cannot serve them. */
int cpecan_em_trainer_set_concurrent_trials(cpecan_em_trainer *t, int n);
/* Samples the cigars, uploads them once and runs every trial's iterations.  Writes outputModel after every iteration
 * (with several trials: the trial's own file, <outputModel>_<i> with outputTrialHmms), then the trial with the highest
 * likelihood to outputModel, and the blast scoring matrix if one was asked for.  best (may be NULL) receives that model,
 * running (may be NULL, room for `iterations` values) its running likelihoods. */
int cpecan_em_train(cpecan_em_trainer *t, const cpecan_cigar *in, int64_t n, const char *outputModel, cpecan_hmm *best,
                    double *running);
/* Wall time of the last cpecan_em_train: setup (sampling, planning, upload) and the iterations, in ms; the number of
 * sampled cigars and jobs. */
typedef struct cpecan_em_timing {
    double setupMs, iterationsMs;
    int64_t iterations, cigars, jobs;
    /* updateTheBand, sums over the iterations of every trial and parts of iterationsMs: the realign batches
     * (cpecan_realigner_reanchor), of which the hand-off stage on the device took handoffMs, and planning and uploading the
     * new EXPECT sets (cpecan_expect_set_create_runs) */
    double realignMs, replanMs, handoffMs;
} cpecan_em_timing;
int cpecan_em_trainer_timing(const cpecan_em_trainer *t, cpecan_em_timing *out);
/* updateTheBand (cPecanEm.py:205-215).  A trial is then
 *     anchors = those of the sampled cigars
 *     for it in 0 .. iterations - 1:
 *         E-step on anchors, M-step, model file written
 *         if it + 1 < iterations: anchors = the sample realigned inside the band of `anchors` under the model of the
 *                                 M-step (cpecan_realigner_reanchor_runs); a new EXPECT set
 * The reference also realigns after the last iteration; nothing reads that run, so it is skipped.  Every trial starts again
 * from the input sample, as the reference re-splits the alignments file per trial.
 * cpecan_em_trainer_alignments: the anchors the last E-step of the last trial of the last cpecan_em_train with the option
 * ran on -- *n sampled cigars in sample order (cpecan_em_sample), (*nRuns)[i] quadruples (x, y, length,
 * expansion) each, one after the other in *runs, in the coordinates of the cigars' sub-sequences.  The trainer's memory,
 * valid until the next cpecan_em_train or cpecan_em_trainer_destroy; CPECAN_ESTATE when the last training ran without
 * the option, failed, or never happened. */
int cpecan_em_trainer_alignments(const cpecan_em_trainer *t, const int64_t **runs, const int64_t **nRuns, int64_t *n);
/* Viterbi training (hard EM).  on != 0: a trial is the same loop, except that its E-step is
 *     cpecan_hmm_init(&acc, type, pseudoCount)
 *     one cpecan_viterbi_run_counts (cpecan_viterbi.h) over a Viterbi object that cpecan_em_train creates once from the sampled
 *         cigars as cpecan_expect_set_create prepares them -- the sub-sequences, the exact-match anchors, the realigner's
 *         banding parameters, both ends ragged -- and that stays on the device for the whole training
 *     cpecan_viterbi_counts_add_to_hmm
 * The M-step, the model files and the choice of the best trial are untouched; the running likelihood of an iteration is the
 * sum of the most probable paths' log-probabilities.  pseudoCount is added to every transition and emission bin (1.0: add-one
 * smoothing, so that a transition no path took keeps a probability); not finite or < 0 is CPECAN_EINVAL.  With updateTheBand,
 * with more than one concurrent trial and with more than one device it is CPECAN_EINVAL with a message, here and in
 * cpecan_em_train, before any device is looked for: none of the three is built.  Off by default; on = 0 restores Baum-Welch. */
int cpecan_em_trainer_set_viterbi_training(cpecan_em_trainer *t, int on, double pseudoCount);

#ifdef __cplusplus
}
#endif
#endif /* CPECAN_EM_H_ */
