/*
 * ref_driver.c -- our own main() around the reference's impl/pairwiseAligner.c and impl/stateMachine.c, built on the
 * stand-in headers of ref_standin/ (oracle/Makefile, targets `ref` and `ref-asan`).  Test infrastructure: it produces
 * the records of tests/golden/reference_runs.json.gz (tests/golden/make_reference_runs.py) and nothing else uses it.
 *
 *   cpecan_ref_driver CASEFILE > RECORDS
 *
 * The case file, one item per line, a case from `case` to `end`:
 *   case NAME OP[,OP...]      pairs indels forward expect mea reweight shift shifted_mea scores overlap
 *   model TYPE                0 fiveState, 2 threeState: the default machine of stateMachine5/3_construct
 *   hmm TYPE T.. E..          1, 3: the numbers go to a temporary file, hmm_loadFromFile + hmm_getStateMachine
 *   params THRESHOLD MINDIAGS TRACEBACK EXPANSION SPLIT DYNAMIC GAPGAMMA
 *   ragged LEFT RIGHT
 *   sx =SEQUENCE              (everything behind the `=`; may be empty)
 *   sy =SEQUENCE
 *   lens LX LY                for the ops that take lengths and no sequences
 *   anchors N x y e ...
 *   pairs N w x y ...         gx, gy likewise
 *   gamma G                   the double gapGamma of reweightAlignedPairs2
 *   end
 * Doubles are read with strtod (decimal with 17 digits or hex).  The record of a case: `case NAME`, then `list KEY N
 * ints...`, `ints KEY N ints...`, `double KEY hex`, `doubles KEY N hex...` lines, then `end`.  Every double is written
 * as a C99 hex float.
 */
#include <math.h>
#include <unistd.h>

#include "pairwiseAligner.h"

typedef struct {
    char name[128], ops[128];
    int modelType, hasHmm;
    double hmmT[25], hmmE[80];
    double threshold;
    int64_t minDiags, traceBack, expansion, split;
    int dynamic;
    float gapGamma;
    int raggedLeft, raggedRight;
    char *sx, *sy;
    int64_t lX, lY;
    int64_t *anchors, nAnchors, *pairs, nPairs, *gx, nGx, *gy, nGy;
    double gamma;
} Case;

static void fail(const char *what, const char *detail) {
    fprintf(stderr, "cpecan_ref_driver: %s: %s\n", what, detail);
    exit(2);
}

static char *copyOf(const char *s) {
    char *t = malloc(strlen(s) + 1);
    strcpy(t, s);
    return t;
}

static int64_t *readInts(char **cursor, int64_t per, int64_t *n) {
    *n = strtoll(*cursor, cursor, 10);
    int64_t *v = malloc(sizeof(int64_t) * (size_t) (*n * per + 1));
    for (int64_t i = 0; i < *n * per; i++) {
        char *end;
        v[i] = strtoll(*cursor, &end, 10);
        if (end == *cursor) {
            fail("short list", *cursor);
        }
        *cursor = end;
    }
    return v;
}

static void resetCase(Case *c) {
    free(c->sx);
    free(c->sy);
    free(c->anchors);
    free(c->pairs);
    free(c->gx);
    free(c->gy);
    memset(c, 0, sizeof(*c));
    c->threshold = 0.01;
    c->minDiags = 1000;
    c->traceBack = 40;
    c->expansion = 20;
    c->split = (int64_t) 3000 * 3000;
    c->gapGamma = 0.5f;
    c->sx = copyOf("");
    c->sy = copyOf("");
    c->lX = c->lY = -1;
}

static int hasOp(const Case *c, const char *op) {
    size_t n = strlen(op);
    for (const char *p = c->ops; *p != '\0';) {
        const char *e = strchr(p, ',');
        size_t len = e ? (size_t) (e - p) : strlen(p);
        if (len == n && strncmp(p, op, n) == 0) {
            return 1;
        }
        p += len + (e ? 1 : 0);
    }
    return 0;
}

static stList *triples(const int64_t *v, int64_t n) {
    stList *l = stList_construct3(0, (void (*)(void *)) stIntTuple_destruct);
    for (int64_t i = 0; i < n; i++) {
        stList_append(l, stIntTuple_construct3(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    }
    return l;
}

static void printList(const char *key, stList *l) {
    printf("list %s %" PRIi64, key, stList_length(l));
    for (int64_t i = 0; i < stList_length(l); i++) {
        stIntTuple *t = stList_get(l, i);
        printf(" %" PRIi64 " %" PRIi64 " %" PRIi64, stIntTuple_get(t, 0), stIntTuple_get(t, 1), stIntTuple_get(t, 2));
    }
    printf("\n");
}

static void printInts(const char *key, const int64_t *v, int64_t n) {
    printf("ints %s %" PRIi64, key, n);
    for (int64_t i = 0; i < n; i++) {
        printf(" %" PRIi64, v[i]);
    }
    printf("\n");
}

static void printDoubles(const char *key, const double *v, int64_t n) {
    printf("doubles %s %" PRIi64, key, n);
    for (int64_t i = 0; i < n; i++) {
        printf(" %a", v[i]);
    }
    printf("\n");
}

static StateMachine *machineOf(const Case *c) {
    if (!c->hasHmm) {
        return c->modelType == fiveState ? stateMachine5_construct(fiveState) : stateMachine3_construct(threeState);
    }
    /* the layout hmm_write gives a file, with 17 significant digits so that every double comes back bit for bit */
    char path[] = "/tmp/cpecan_ref_hmm_XXXXXX";
    int fd = mkstemp(path);
    if (fd < 0) {
        fail("mkstemp", path);
    }
    FILE *f = fdopen(fd, "w");
    int S = (c->modelType == fiveStateAsymmetric || c->modelType == fiveState) ? 5 : 3;
    fprintf(f, "%i\t", c->modelType);
    for (int i = 0; i < S * S; i++) {
        fprintf(f, "%.17g\t", c->hmmT[i]);
    }
    fprintf(f, "%.17g\n", 0.0);
    for (int i = 0; i < S * 16; i++) {
        fprintf(f, "%.17g\t", c->hmmE[i]);
    }
    fprintf(f, "\n");
    fclose(f);
    Hmm *hmm = hmm_loadFromFile(path);
    unlink(path);
    for (int i = 0; i < S * S; i++) {
        if (hmm->transitions[i] != c->hmmT[i]) {
            fail(c->name, "a transition did not survive the HMM file");
        }
    }
    for (int i = 0; i < S * 16; i++) {
        if (hmm->emissions[i] != c->hmmE[i]) {
            fail(c->name, "an emission did not survive the HMM file");
        }
    }
    StateMachine *sM = hmm_getStateMachine(hmm);
    hmm_destruct(hmm);
    return sM;
}

static void runCase(Case *c) {
    printf("case %s\n", c->name);
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    p->threshold = c->threshold;
    p->minDiagsBetweenTraceBack = c->minDiags;
    p->traceBackDiagonals = c->traceBack;
    p->diagonalExpansion = c->expansion;
    p->splitMatrixBiggerThanThis = c->split;
    p->dynamicAnchorExpansion = c->dynamic;
    p->gapGamma = c->gapGamma;
    int64_t lX = c->lX >= 0 ? c->lX : (int64_t) strlen(c->sx), lY = c->lY >= 0 ? c->lY : (int64_t) strlen(c->sy);
    int needsMachine = hasOp(c, "pairs") || hasOp(c, "indels") || hasOp(c, "forward") || hasOp(c, "expect") ||
                       hasOp(c, "shifted_mea");
    StateMachine *sM = needsMachine ? machineOf(c) : NULL;
    stList *anchors = triples(c->anchors, c->nAnchors);

    if (hasOp(c, "pairs")) {
        stList *l = getAlignedPairsUsingAnchors(sM, c->sx, c->sy, anchors, p, c->raggedLeft, c->raggedRight);
        printList("match", l);
        stList_destruct(l);
    }
    if (hasOp(c, "indels")) {
        stList *m, *gx, *gy;
        getAlignedPairsWithIndelsUsingAnchors(sM, c->sx, c->sy, anchors, p, &m, &gx, &gy, c->raggedLeft, c->raggedRight);
        printList("imatch", m);
        printList("gapx", gx);
        printList("gapy", gy);
        stList_destruct(m);
        stList_destruct(gx);
        stList_destruct(gy);
    }
    if (hasOp(c, "forward")) {
        double v = computeForwardProbability(c->sx, c->sy, anchors, p, sM, c->raggedLeft, c->raggedRight);
        printf("double fwd %a\n", v);
    }
    if (hasOp(c, "expect")) {
        Hmm *acc = hmm_constructEmpty(0.0, sM->type);
        getExpectationsUsingAnchors(sM, acc, c->sx, c->sy, anchors, p, c->raggedLeft, c->raggedRight);
        printDoubles("T", acc->transitions, acc->stateNumber * acc->stateNumber);
        printDoubles("E", acc->emissions, acc->stateNumber * 16);
        printf("double likelihood %a\n", acc->likelihood);
        hmm_destruct(acc);
    }
    if (hasOp(c, "shifted_mea")) {
        double score = 0.0;
        stList *l = getShiftedMEAAlignment(c->sx, c->sy, anchors, p, sM, c->raggedLeft, c->raggedRight, &score);
        printList("shifted_mea", l);
        printf("double shifted_mea_score %a\n", score);
        stList_destruct(l);
    }
    if (hasOp(c, "mea")) {
        stList *pairs = triples(c->pairs, c->nPairs), *gx = triples(c->gx, c->nGx), *gy = triples(c->gy, c->nGy);
        double score = 0.0;
        stList *l = getMaximalExpectedAccuracyPairwiseAlignment(pairs, gx, gy, lX, lY, &score, p);
        printList("mea", l);
        printf("double mea_score %a\n", score);
        stList_destruct(l);
        stList_destruct(pairs);
        stList_destruct(gx);
        stList_destruct(gy);
    }
    if (hasOp(c, "reweight")) {
        stList *pairs = triples(c->pairs, c->nPairs);
        int64_t *ix = getIndelProbabilities(pairs, lX, 1), *iy = getIndelProbabilities(pairs, lY, 0);
        printInts("indel_probs_x", ix, lX);
        printInts("indel_probs_y", iy, lY);
        free(ix);
        free(iy);
        stList *l = reweightAlignedPairs2(pairs, lX, lY, c->gamma); /* destroys `pairs` unless it hands it back */
        printList("reweighted", l);
        stList_destruct(l);
    }
    if (hasOp(c, "shift")) {
        stList *pairs = triples(c->pairs, c->nPairs);
        stList *l = leftShiftAlignment(pairs, c->sx, c->sy);
        printList("shifted", l);
        stList_destruct(l);
        stList_destruct(pairs);
    }
    if (hasOp(c, "scores")) {
        stList *pairs = triples(c->pairs, c->nPairs);
        printf("double identity %a\n", scoreByIdentity(c->sx, c->sy, lX, lY, pairs));
        printf("double identity_ignoring_gaps %a\n", scoreByIdentityIgnoringGaps(c->sx, c->sy, pairs));
        printf("double posterior %a\n", scoreByPosteriorProbability(lX, lY, pairs));
        printf("double posterior_ignoring_gaps %a\n", scoreByPosteriorProbabilityIgnoringGaps(pairs));
        stList_destruct(pairs);
    }
    if (hasOp(c, "overlap")) {
        stList *pairs = triples(c->pairs, c->nPairs);
        stList *l = filterToRemoveOverlap(pairs);
        printList("non_overlapping", l);
        stList_destruct(l);
        stList_destruct(pairs);
    }
    stList_destruct(anchors);
    if (sM != NULL) {
        stateMachine_destruct(sM);
    }
    pairwiseAlignmentBandingParameters_destruct(p);
    printf("end\n");
    fflush(stdout);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fail("usage", "cpecan_ref_driver CASEFILE");
    }
    FILE *f = fopen(argv[1], "r");
    if (f == NULL) {
        fail("cannot open", argv[1]);
    }
    Case c;
    memset(&c, 0, sizeof(c));
    resetCase(&c);
    char *line = NULL;
    size_t cap = 0;
    ssize_t len;
    while ((len = getline(&line, &cap, f)) >= 0) {
        while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) {
            line[--len] = '\0';
        }
        char *cursor = line;
        char key[32];
        int used = 0;
        if (sscanf(cursor, "%31s%n", key, &used) != 1) {
            continue;
        }
        cursor += used;
        if (strcmp(key, "case") == 0) {
            resetCase(&c);
            if (sscanf(cursor, "%127s %127s", c.name, c.ops) != 2) {
                fail("bad case line", line);
            }
        } else if (strcmp(key, "model") == 0) {
            c.modelType = (int) strtol(cursor, &cursor, 10);
            c.hasHmm = 0;
        } else if (strcmp(key, "hmm") == 0) {
            c.modelType = (int) strtol(cursor, &cursor, 10);
            c.hasHmm = 1;
            int S = (c.modelType == fiveStateAsymmetric || c.modelType == fiveState) ? 5 : 3;
            for (int i = 0; i < S * S + S * 16; i++) {
                char *end;
                double v = strtod(cursor, &end);
                if (end == cursor) {
                    fail("short hmm line", c.name);
                }
                cursor = end;
                if (i < S * S) {
                    c.hmmT[i] = v;
                } else {
                    c.hmmE[i - S * S] = v;
                }
            }
        } else if (strcmp(key, "params") == 0) {
            c.threshold = strtod(cursor, &cursor);
            c.minDiags = strtoll(cursor, &cursor, 10);
            c.traceBack = strtoll(cursor, &cursor, 10);
            c.expansion = strtoll(cursor, &cursor, 10);
            c.split = strtoll(cursor, &cursor, 10);
            c.dynamic = (int) strtol(cursor, &cursor, 10);
            c.gapGamma = (float) strtod(cursor, &cursor);
        } else if (strcmp(key, "ragged") == 0) {
            c.raggedLeft = (int) strtol(cursor, &cursor, 10);
            c.raggedRight = (int) strtol(cursor, &cursor, 10);
        } else if (strcmp(key, "sx") == 0 || strcmp(key, "sy") == 0) {
            char *eq = strchr(cursor, '=');
            if (eq == NULL) {
                fail("sequence line without =", line);
            }
            char **dst = key[1] == 'x' ? &c.sx : &c.sy;
            free(*dst);
            *dst = copyOf(eq + 1);
        } else if (strcmp(key, "lens") == 0) {
            c.lX = strtoll(cursor, &cursor, 10);
            c.lY = strtoll(cursor, &cursor, 10);
        } else if (strcmp(key, "anchors") == 0) {
            free(c.anchors);
            c.anchors = readInts(&cursor, 3, &c.nAnchors);
        } else if (strcmp(key, "pairs") == 0) {
            free(c.pairs);
            c.pairs = readInts(&cursor, 3, &c.nPairs);
        } else if (strcmp(key, "gx") == 0) {
            free(c.gx);
            c.gx = readInts(&cursor, 3, &c.nGx);
        } else if (strcmp(key, "gy") == 0) {
            free(c.gy);
            c.gy = readInts(&cursor, 3, &c.nGy);
        } else if (strcmp(key, "gamma") == 0) {
            c.gamma = strtod(cursor, &cursor);
        } else if (strcmp(key, "end") == 0) {
            runCase(&c);
        } else {
            fail("unknown key", key);
        }
    }
    free(line);
    fclose(f);
    resetCase(&c);
    free(c.sx);
    free(c.sy);
    return 0;
}
