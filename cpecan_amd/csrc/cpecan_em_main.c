/*
 * cpecan_em -- command line of the pair-HMM trainer (include/cpecan_em.h) with cPecanEm.py's option names.
 *
 *   cpecan_em --sequences "a.fa b.fa" --alignments in.cigar --outputModel hmm.txt [EM options]
 *             [--optionsToRealign "..."] [--device N | --devices LIST] [--seed N]
 */
#define _POSIX_C_SOURCE 200809L
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_em.h"

static void usage(void) {
    fprintf(stderr,
            "cpecan_em --sequences \"a.fa b.fa\" --alignments FILE --outputModel FILE [options]\n"
            "--modelType fiveState|fiveStateAsymmetric|threeState|threeStateAsymmetric  --inputModel FILE\n"
            "--iterations N (10)  --trials N (3, with --randomStart and no --inputModel)  --randomStart  --outputTrialHmms\n"
            "--concurrentTrials N (1; up to 8 trials per kernel launch, more trials run in rounds)\n"
            "--useDefaultModelAsStart  --setJukesCantorStartingEmissions F  --trainEmissions  --tieEmissions\n"
            "--maxAlignmentLengthPerJob N (1000000)  --maxAlignmentLengthToSample N (50000000)  --seed N (0)\n"
            "--updateTheBand (realign the sample after every iteration; not with --concurrentTrials above 1)\n"
            "--viterbiTraining (hard EM: counts along the most probable paths; not with --updateTheBand, --concurrentTrials\n"
            "above 1 or several devices)  --viterbiPseudoCount C (1.0, added to every count)\n"
            "--blastScoringMatrixFile FILE  --optionsToRealign \"...\" (default \"--diagonalExpansion=10\n"
            "--splitMatrixBiggerThanThis=3000\"; -r/-o/-t/-l/-L and their long names)  --device N  --devices LIST\n"
            "--logLevel L (ignored)  -h --help\n");
}

static int fail(const char *what) {
    const char *e = cpecan_last_error();
    fprintf(stderr, "cpecan_em: %s%s%s\n", what, e && *e ? ": " : "", e ? e : "");
    return 1;
}

/* "0-3", "0,2,5", "1,1": a device list; returns the count or -1 */
static int parse_devices(const char *text, int *out, int cap) {
    int n = 0;
    for (const char *p = text; *p;) {
        char *end;
        const long a = strtol(p, &end, 10);
        if (end == p || a < 0) return -1;
        long b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            if (end == p + 1 || b < a) return -1;
            p = end;
        }
        for (long d = a; d <= b; d++) {
            if (n >= cap) return -1;
            out[n++] = (int)d;
        }
        if (*p == ',') p++;
        else if (*p) return -1;
    }
    return n;
}

static int model_type(const char *s) {
    const char *names[4] = {"fiveState", "fiveStateAsymmetric", "threeState", "threeStateAsymmetric"};
    for (int i = 0; i < 4; i++)
        if (strcmp(s, names[i]) == 0) return i;
    return -1;
}

/* The realign options of --optionsToRealign (cPecanRealign's names): "--name=value", "--name value" or "-r value". */
static int realign_options(const char *text, cpecan_realign_options *o) {
    char *copy = strdup(text), *save = NULL;
    if (!copy) return -1;
    int ok = 1;
    for (char *tok = strtok_r(copy, " \t\n", &save); ok && tok; tok = strtok_r(NULL, " \t\n", &save)) {
        char *value = strchr(tok, '=');
        if (value) *value++ = 0;
        else if (tok[0] == '-') value = strtok_r(NULL, " \t\n", &save);
        const char *name = tok;
        while (*name == '-') name++;
        long long v = 0;
        float f = 0.0f;
        if (!value) ok = 0;
        else if (!strcmp(name, "diagonalExpansion") || !strcmp(name, "r"))
            ok = sscanf(value, "%lld", &v) == 1 && (o->params.diagonalExpansion = v, 1);
        else if (!strcmp(name, "splitMatrixBiggerThanThis") || !strcmp(name, "o"))
            ok = sscanf(value, "%lld", &v) == 1 && v >= 0 && (o->params.splitMatrixBiggerThanThis = v * v, 1);
        else if (!strcmp(name, "constraintDiagonalTrim") || !strcmp(name, "t"))
            ok = sscanf(value, "%lld", &v) == 1 && (o->constraintDiagonalTrim = v, 1);
        else if (!strcmp(name, "gapGamma") || !strcmp(name, "l"))
            ok = sscanf(value, "%f", &f) == 1 && (o->gapGamma = f, 1);
        else if (!strcmp(name, "matchGamma") || !strcmp(name, "L"))
            ok = sscanf(value, "%f", &f) == 1 && (o->matchGamma = f, 1);
        else if (!strcmp(name, "logLevel") || !strcmp(name, "a"))
            ok = 1;
        else {
            fprintf(stderr, "cpecan_em: --optionsToRealign: %s does not change the expectations\n", tok);
            ok = 0;
        }
    }
    free(copy);
    return ok ? 0 : -1;
}

static int read_cigars(const char *path, cpecan_cigar **out, int64_t *n) {
    FILE *f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cpecan_em: cannot open %s\n", path);
        return -1;
    }
    char *line = NULL;
    size_t lineCap = 0;
    int64_t cap = 0;
    int status = 0;
    *out = NULL;
    *n = 0;
    while (status == 0 && getline(&line, &lineCap, f) >= 0) {
        if (line[strspn(line, " \t\r\n")] == 0) continue;
        if (*n == cap) {
            cap = cap ? 2 * cap : 1024;
            cpecan_cigar *grown = realloc(*out, sizeof(cpecan_cigar) * (size_t)cap);
            if (!grown) {
                status = -1;
                break;
            }
            *out = grown;
        }
        if (cpecan_cigar_parse(line, &(*out)[*n]) != CPECAN_OK) {
            status = fail("cigar");
            break;
        }
        (*n)++;
    }
    free(line);
    fclose(f);
    return status;
}

int main(int argc, char **argv) {
    cpecan_em_options o;
    cpecan_em_options_default(&o);
    cpecan_realign_options ro;
    cpecan_realign_options_default(&ro);
    if (realign_options("--diagonalExpansion=10 --splitMatrixBiggerThanThis=3000", &ro) != 0) return 1; /* cPecanEm.py */
    const char *sequences = NULL, *alignments = NULL, *outputModel = "hmm.txt", *toRealign = NULL;
    long long device = 0;
    int devices[64], nDevices = 0;
    enum {
        kModelType = 256, kInputModel, kOutputModel, kIterations, kTrials, kRandomStart, kTrialHmms, kDefaultStart,
        kJukesCantor, kTrainEmissions, kTieEmissions, kPerJob, kToSample, kSeed, kBlast, kToRealign, kSequences,
        kAlignments, kDevice, kDevices, kLogLevel, kXml, kUpdateBand, kConcurrent, kViterbi, kViterbiPseudo
    };
    static struct option longOpts[] = {{"modelType", required_argument, 0, kModelType},
                                       {"inputModel", required_argument, 0, kInputModel},
                                       {"outputModel", required_argument, 0, kOutputModel},
                                       {"iterations", required_argument, 0, kIterations},
                                       {"trials", required_argument, 0, kTrials},
                                       {"concurrentTrials", required_argument, 0, kConcurrent},
                                       {"randomStart", no_argument, 0, kRandomStart},
                                       {"outputTrialHmms", no_argument, 0, kTrialHmms},
                                       {"useDefaultModelAsStart", no_argument, 0, kDefaultStart},
                                       {"setJukesCantorStartingEmissions", required_argument, 0, kJukesCantor},
                                       {"trainEmissions", no_argument, 0, kTrainEmissions},
                                       {"tieEmissions", no_argument, 0, kTieEmissions},
                                       {"maxAlignmentLengthPerJob", required_argument, 0, kPerJob},
                                       {"maxAlignmentLengthToSample", required_argument, 0, kToSample},
                                       {"seed", required_argument, 0, kSeed},
                                       {"blastScoringMatrixFile", required_argument, 0, kBlast},
                                       {"optionsToRealign", required_argument, 0, kToRealign},
                                       {"sequences", required_argument, 0, kSequences},
                                       {"alignments", required_argument, 0, kAlignments},
                                       {"device", required_argument, 0, kDevice},
                                       {"devices", required_argument, 0, kDevices},
                                       {"logLevel", required_argument, 0, kLogLevel},
                                       {"outputXMLModelFile", required_argument, 0, kXml},
                                       {"updateTheBand", no_argument, 0, kUpdateBand},
                                       {"viterbiTraining", no_argument, 0, kViterbi},
                                       {"viterbiPseudoCount", required_argument, 0, kViterbiPseudo},
                                       {"help", no_argument, 0, 'h'},
                                       {0, 0, 0, 0}};
    long long v, concurrent = 1;
    int viterbiTraining = 0;
    double viterbiPseudoCount = 1.0;
    for (int key; (key = getopt_long(argc, argv, "h", longOpts, NULL)) != -1;) {
        switch (key) {
        case 'h': usage(); return 0;
        case kModelType:
            if ((o.modelType = model_type(optarg)) < 0) {
                fprintf(stderr, "cpecan_em: unknown --modelType %s\n", optarg);
                return 1;
            }
            break;
        case kInputModel: o.inputModel = optarg; break;
        case kOutputModel: outputModel = optarg; break;
        case kIterations: if (sscanf(optarg, "%lld", &v) != 1 || v < 0) return fail("--iterations"); o.iterations = (int)v; break;
        case kTrials: if (sscanf(optarg, "%lld", &v) != 1 || v < 1) return fail("--trials"); o.trials = (int)v; break;
        case kConcurrent:
            if (sscanf(optarg, "%lld", &v) != 1 || v < 1 || v > CPECAN_MAX_MODEL_SLOTS) {
                fprintf(stderr, "cpecan_em: --concurrentTrials %s: 1 to %d trials per launch\n", optarg, CPECAN_MAX_MODEL_SLOTS);
                return 1;
            }
            concurrent = v;
            break;
        case kRandomStart: o.randomStart = 1; break;
        case kTrialHmms: o.outputTrialHmms = 1; break;
        case kDefaultStart: o.useDefaultModelAsStart = 1; break;
        case kJukesCantor:
            if (sscanf(optarg, "%lf", &o.setJukesCantorStartingEmissions) != 1 || o.setJukesCantorStartingEmissions < 0)
                return fail("--setJukesCantorStartingEmissions");
            break;
        case kTrainEmissions: o.trainEmissions = 1; break;
        case kTieEmissions: o.tieEmissions = 1; break;
        case kPerJob: if (sscanf(optarg, "%lld", &v) != 1 || v < 0) return fail("--maxAlignmentLengthPerJob"); o.maxAlignmentLengthPerJob = v; break;
        case kToSample: if (sscanf(optarg, "%lld", &v) != 1 || v < 0) return fail("--maxAlignmentLengthToSample"); o.maxAlignmentLengthToSample = v; break;
        case kSeed: if (sscanf(optarg, "%lld", &v) != 1) return fail("--seed"); o.seed = (uint64_t)v; break;
        case kBlast: o.blastScoringMatrixFile = optarg; break;
        case kToRealign: toRealign = optarg; break;
        case kSequences: sequences = optarg; break;
        case kAlignments: alignments = optarg; break;
        case kDevice: if (sscanf(optarg, "%lld", &device) != 1 || device < 0) return fail("--device"); break;
        case kDevices:
            if ((nDevices = parse_devices(optarg, devices, 64)) < 1) {
                usage();
                return 1;
            }
            device = devices[0];
            break;
        case kLogLevel: break;
        case kXml: fprintf(stderr, "cpecan_em: --outputXMLModelFile is not supported\n"); return 1;
        case kUpdateBand:
            fprintf(stderr, "cpecan_em: --updateTheBand: the sampled alignments are realigned after every iteration\n");
            o.updateTheBand = 1;
            break;
        case kViterbi: viterbiTraining = 1; break;
        case kViterbiPseudo:
            if (sscanf(optarg, "%lf", &viterbiPseudoCount) != 1) {
                fprintf(stderr, "cpecan_em: --viterbiPseudoCount %s: a number >= 0\n", optarg);
                return 1;
            }
            break;
        default: usage(); return 1;
        }
    }
    if (!sequences || !alignments || optind < argc) {
        usage();
        return 1;
    }
    if (toRealign && realign_options(toRealign, &ro) != 0) return fail("--optionsToRealign");
    cpecan_em_trainer *t = NULL;
    if (cpecan_em_trainer_create(&t, &o, &ro, (int)device) != CPECAN_OK) return fail("options");
    if (nDevices > 1 && cpecan_em_trainer_set_devices(t, devices, nDevices) != CPECAN_OK) return fail("--devices");
    if (cpecan_em_trainer_set_concurrent_trials(t, (int)concurrent) != CPECAN_OK) return fail("--concurrentTrials");
    if (viterbiTraining && cpecan_em_trainer_set_viterbi_training(t, 1, viterbiPseudoCount) != CPECAN_OK) return fail("--viterbiTraining");
    int status = 0;
    char *seqs = strdup(sequences), *save = NULL;
    for (char *path = strtok_r(seqs, " \t", &save); status == 0 && path; path = strtok_r(NULL, " \t", &save))
        if (cpecan_em_trainer_read_fasta(t, path) < 0) status = fail(path);
    free(seqs);
    cpecan_cigar *in = NULL;
    int64_t n = 0;
    if (status == 0 && read_cigars(alignments, &in, &n) != 0) status = 1;
    cpecan_hmm best;
    if (status == 0 && cpecan_em_train(t, in, n, outputModel, &best, NULL) != CPECAN_OK) status = fail("training");
    if (status == 0) {
        cpecan_em_timing tm;
        cpecan_em_trainer_timing(t, &tm);
        fprintf(stderr, "cpecan_em: %lld alignments in %lld jobs, likelihood %.6f; setup %.1f ms, %lld iterations %.1f ms\n",
                (long long)tm.cigars, (long long)tm.jobs, best.likelihood, tm.setupMs, (long long)tm.iterations,
                tm.iterationsMs);
    }
    cpecan_cigars_free(in, n);
    cpecan_em_trainer_destroy(t);
    return status;
}
