/*
 * The intake of a batch (cpecan_amd/csrc/cpecan_host.c: add_many in its three stages) and the overflow scan of a download
 * (cpk_overflow_scan) without the library, HIP or a GPU, built with -fsanitize=address,undefined by tests/test_intake_c.py;
 * device_standins.h stands in for the device layer, which none of this reaches.
 *
 * Intake: batches of 70 problems (the OpenMP loops) and of 5 (the serial ones), each followed by a pair with lX == 0, one with
 * lY == 0, one without anchors and one whose anchors start in column 0, cut at gaps of more than 10 cells; as triples, as runs
 * and as runs with every third problem on the minus strand; anchors of stride 2 and 3; runs kept and not (CPECAN_KEEP_RUNS);
 * two calls per batch.  What the batch holds afterwards -- read through cpk_batch_intake_digest -- is held against a plain
 * sequential restatement: one problem at a time, one anchor at a time, everything appended where the arrays end.
 * Overflow scan: three hand-made regions, with one list and with three.  Everything is freed: the leak check stays on.
 */
#define _POSIX_C_SOURCE 200112L /* setenv */
#include "device_standins.h"

static uint64_t rngState = 0x2545F4914F6CDD1Dull;
static int64_t rnd(int64_t n) { /* 0 .. n - 1 */
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((rngState >> 33) % (uint64_t)n);
}

/* ---- problems ---- */
typedef struct {
    char *sX, *sY;
    int64_t lX, lY;
    int64_t *runs, nRuns;       /* (x, y, length, expansion) */
    int64_t *triples, nTriples; /* the same anchors, one per column: (x, y, expansion) */
    int rl, rr;                 /* ragged ends */
} Problem;

/* the runs' anchors one by one */
static void expand(Problem *p) {
    p->nTriples = 0;
    for (int64_t i = 0; i < p->nRuns; i++) p->nTriples += p->runs[4 * i + 2];
    p->triples = malloc(sizeof(int64_t) * 3 * (size_t)(p->nTriples + 1));
    int64_t at = 0;
    for (int64_t i = 0; i < p->nRuns; i++)
        for (int64_t q = 0; q < p->runs[4 * i + 2]; q++, at++) {
            p->triples[3 * at] = p->runs[4 * i] + q;
            p->triples[3 * at + 1] = p->runs[4 * i + 1] + q;
            p->triples[3 * at + 2] = p->runs[4 * i + 3];
        }
}

/* X: random letters, a few of them lower-case or N; Y: X with substitutions, deletions and insertions; anchors: the columns
 * that kept their letter (`anchored`), as runs of diagonal neighbours with expansions 2 * (0 .. 4). */
static void make_problem(Problem *p, int64_t lX, int anchored) {
    static const char letters[] = "ACGTacgtNR";
    memset(p, 0, sizeof *p);
    p->sX = malloc((size_t)lX + 1);
    p->sY = malloc(2 * (size_t)lX + 1);
    p->runs = malloc(sizeof(int64_t) * 4 * (size_t)(lX + 1));
    p->lX = lX;
    int64_t y = 0, open = 0; /* open: the last column was kept and extends the last run */
    for (int64_t x = 0; x < lX; x++) {
        p->sX[x] = letters[rnd(50) ? rnd(4) : 4 + rnd(6)];
        const int64_t r = rnd(100);
        if (r < 3) { /* deleted */
            open = 0;
            continue;
        }
        if (r < 6) { /* an inserted letter first */
            p->sY[y++] = letters[rnd(4)];
            open = 0;
        }
        if (r < 20) { /* substituted */
            p->sY[y++] = letters[rnd(8)];
            open = 0;
            continue;
        }
        p->sY[y] = p->sX[x];
        if (anchored && open) p->runs[4 * (p->nRuns - 1) + 2]++;
        else if (anchored) {
            int64_t *q = p->runs + 4 * p->nRuns++;
            q[0] = x, q[1] = y, q[2] = 1, q[3] = 2 * rnd(5);
        }
        open = 1;
        y++;
    }
    p->lY = y;
    expand(p);
}

static void free_problem(Problem *p) {
    free(p->sX);
    free(p->sY);
    free(p->runs);
    free(p->triples);
}

/* n problems of 30 .. 600 letters and the four edge pairs behind them */
static Problem *make_problems(int64_t n, int64_t *total) {
    Problem *ps = malloc(sizeof(Problem) * (size_t)(n + 4));
    for (int64_t i = 0; i < n; i++) {
        make_problem(&ps[i], 30 + rnd(571), 1);
        ps[i].rl = i % 5 == 2;
        ps[i].rr = i % 7 == 3;
    }
    make_problem(&ps[n], 40, 0); /* lX == 0 */
    ps[n].lX = 0;
    make_problem(&ps[n + 1], 40, 0); /* lY == 0 */
    ps[n + 1].lY = 0;
    make_problem(&ps[n + 2], 40, 0); /* no anchors */
    Problem *c = &ps[n + 3];     /* anchors from column 0 */
    make_problem(c, 30, 0);
    memcpy(c->sY, c->sX, (size_t)c->lX);
    c->lY = c->lX;
    c->nRuns = 2;
    c->runs[0] = 0, c->runs[1] = 0, c->runs[2] = 12, c->runs[3] = 4;
    c->runs[4] = 20, c->runs[5] = 21, c->runs[6] = 3, c->runs[7] = 6;
    free(c->triples);
    expand(c);
    *total = n + 4;
    return ps;
}

/* ---- the restatement ---- */
typedef struct {
    int64_t *v;
    int64_t n, cap;
} Ints;
typedef struct {
    uint8_t *v;
    int64_t n, cap;
} Bytes;
static void push_int(Ints *a, int64_t x) {
    if (a->n == a->cap) a->v = realloc(a->v, sizeof(int64_t) * (size_t)(a->cap = a->cap ? 2 * a->cap : 64));
    a->v[a->n++] = x;
}
static void push_byte(Bytes *a, uint8_t x) {
    if (a->n == a->cap) a->v = realloc(a->v, (size_t)(a->cap = a->cap ? 2 * a->cap : 64));
    a->v[a->n++] = x;
}

typedef struct {
    int runForm, stride;
    Ints problems, regions, regionRuns, values; /* values: anchor or run values */
    Bytes symbols, chars;
    int64_t nProblems, nRegions, nAnchors, nRuns;
} Model;

static uint8_t upper(uint8_t c) { return (uint8_t)((c >= 'a' && c <= 'z') ? c - 'a' + 'A' : c); }
static uint8_t symbol(uint8_t c) {
    switch (upper(c)) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return 4;
    }
}
static uint8_t complement(uint8_t c) { /* keeps the case */
    static const char from[] = "ACGTacgt", to[] = "TGCAtgca";
    const char *f = c ? strchr(from, c) : NULL;
    return f ? (uint8_t)to[f - from] : c;
}
static void push_symbols(Bytes *a, const uint8_t *s, int64_t l) {
    push_byte(a, 4);
    for (int64_t i = 0; i < l; i++) push_byte(a, symbol(s[i]));
    push_byte(a, 4);
}

static int64_t cutsSeen = 0; /* anchored problems that were cut into several rectangles */
/* one problem into the model, as an add call leaves it in the batch */
static void model_add(Model *m, const Problem *p, int viaRuns, int minus, int64_t split) {
    uint8_t *y = malloc((size_t)p->lY + 1);
    for (int64_t k = 0; k < p->lY; k++) y[k] = minus ? complement((uint8_t)p->sY[p->lY - 1 - k]) : (uint8_t)p->sY[k];
    int64_t *rects = malloc(sizeof(int64_t) * 4 * (size_t)(p->nTriples + 2));
    const int64_t nRects = cpecan_split_points(p->triples, p->nTriples, p->lX, p->lY, split, p->rl, p->rr, rects);
    CHECK(nRects >= 0);
    cutsSeen += nRects > 1 && p->nRuns > 0;
    const int64_t f[7] = {m->nRegions, nRects, p->lX, p->lY, m->chars.n, m->chars.n + p->lX, minus};
    for (int j = 0; j < 7; j++) push_int(&m->problems, f[j]);
    for (int64_t k = 0; k < p->lX; k++) push_byte(&m->chars, upper((uint8_t)p->sX[k]));
    for (int64_t k = 0; k < p->lY; k++) push_byte(&m->chars, upper(y[k]));
    /* the entries as the call carries them: a batch that keeps runs takes a triple for a run of one */
    const int64_t nEntries = viaRuns ? p->nRuns : p->nTriples;
    int64_t next = 0;
    for (int64_t k = 0; k < nRects; k++) {
        const int64_t x1 = rects[4 * k], y1 = rects[4 * k + 1], x2 = rects[4 * k + 2], y2 = rects[4 * k + 3];
        const int64_t seqX = m->symbols.n;
        push_symbols(&m->symbols, (const uint8_t *)p->sX + x1, x2 - x1);
        const int64_t seqY = m->symbols.n;
        push_symbols(&m->symbols, y + y1, y2 - y1);
        const int64_t anchorOff = m->nAnchors, runOff = m->nRuns;
        for (; next < nEntries; next++) {
            const int64_t *e = viaRuns ? p->runs + 4 * next : p->triples + 3 * next;
            const int64_t len = viaRuns ? e[2] : 1, expansion = viaRuns ? e[3] : e[2];
            if (e[0] + e[1] >= x2 + y2) break;
            if (m->runForm == 1) {
                const int64_t q[4] = {e[0] - x1, e[1] - y1, len, m->nAnchors};
                for (int j = 0; j < 4; j++) push_int(&m->values, q[j]);
                m->nRuns++;
                m->nAnchors += len;
                continue;
            }
            for (int64_t q = 0; q < len; q++, m->nAnchors++) {
                CHECK(e[0] + q < x2 && e[1] + q < y2); /* a rectangle never ends inside a run */
                push_int(&m->values, e[0] + q - x1);
                push_int(&m->values, e[1] + q - y1);
                if (m->stride == 3) push_int(&m->values, expansion);
            }
        }
        const int64_t g[11] = {m->nProblems, x1, y1, x2 - x1, y2 - y1, seqX, seqY, anchorOff, m->nAnchors - anchorOff, p->rl || k > 0, p->rr || k < nRects - 1};
        for (int j = 0; j < 11; j++) push_int(&m->regions, g[j]);
        push_int(&m->regionRuns, m->runForm == 1 ? runOff : 0);
        push_int(&m->regionRuns, m->nRuns - runOff);
        m->nRegions++;
    }
    CHECK(next == nEntries);
    m->nProblems++;
    free(rects);
    free(y);
}

static uint64_t fnv(const void *data, size_t n, uint64_t h) {
    const unsigned char *p = data;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

/* the five hashes of cpk_batch_intake_digest, of the model */
static void model_digest(const Model *m, uint64_t out[5]) {
    const uint64_t seed = 0xcbf29ce484222325ull;
    const int64_t form[2] = {m->runForm, m->stride};
    out[0] = fnv(m->problems.v, sizeof(int64_t) * (size_t)m->problems.n, seed);
    out[1] = fnv(m->regions.v, sizeof(int64_t) * (size_t)m->regions.n, seed);
    out[2] = fnv(m->symbols.v, (size_t)m->symbols.n, seed);
    out[3] = fnv(form, sizeof form, seed);
    if (m->runForm == 1) out[3] = fnv(m->regionRuns.v, sizeof(int64_t) * (size_t)m->regionRuns.n, out[3]);
    int32_t *v32 = malloc(sizeof(int32_t) * (size_t)(m->values.n + 1)); /* the batch keeps 32-bit values */
    for (int64_t i = 0; i < m->values.n; i++) v32[i] = (int32_t)m->values.v[i];
    out[3] = fnv(v32, sizeof(int32_t) * (size_t)m->values.n, out[3]);
    free(v32);
    out[4] = fnv(m->chars.v, (size_t)m->chars.n, seed);
}

static void model_free(Model *m) {
    free(m->problems.v);
    free(m->regions.v);
    free(m->regionRuns.v);
    free(m->values.v);
    free(m->symbols.v);
    free(m->chars.v);
}

/* ---- the batches ---- */
enum { TRIPLES, RUNS, STRANDED };
static int is_minus(int form, int64_t i) { return form == STRANDED && i % 3 == 1; }

/* problems [from, to) in one call of the given form; returns what the call returned */
static int64_t add_call(cpecan_batch *b, const Problem *ps, int64_t from, int64_t to, int form) {
    const int64_t n = to - from;
    int64_t rc;
    if (form == TRIPLES) {
        cpecan_problem *items = calloc((size_t)n + 1, sizeof *items);
        for (int64_t i = 0; i < n; i++) {
            const Problem *p = &ps[from + i];
            items[i] = (cpecan_problem){p->sX, p->lX, p->sY, p->lY, p->triples, p->nTriples, p->rl, p->rr};
        }
        rc = cpecan_batch_add_many(b, items, n);
        free(items);
        return rc;
    }
    cpecan_problem_runs *items = calloc((size_t)n + 1, sizeof *items);
    int32_t *minus = calloc((size_t)n + 1, sizeof *minus);
    for (int64_t i = 0; i < n; i++) {
        const Problem *p = &ps[from + i];
        items[i] = (cpecan_problem_runs){p->sX, p->lX, p->sY, p->lY, p->runs, p->nRuns, p->rl, p->rr};
        minus[i] = is_minus(form, from + i);
    }
    rc = form == RUNS ? cpecan_batch_add_many_runs(b, items, n) : cpecan_batch_add_many_runs_stranded(b, items, minus, n);
    free(items);
    free(minus);
    return rc;
}

static int same_digest(const uint64_t *a, const uint64_t *b) { return memcmp(a, b, sizeof(uint64_t) * 5) == 0; }

/* One batch: the problems in two calls, [0, cut) in `form` and [cut, n) in `form2`, a failed call in between; against the
 * restatement. */
static void one_batch(const Problem *ps, int64_t n, int64_t cut, int form, int form2, int stride3, int keepRuns) {
    const int64_t split = 10;
    cpecan_model model;
    cpecan_params params;
    CHECK(cpecan_model_default(&model, CPECAN_FIVE_STATE) == CPECAN_OK);
    CHECK(cpecan_params_default(&params) == CPECAN_OK);
    params.diagonalExpansion = 4;
    params.splitMatrixBiggerThanThis = split;
    params.dynamicAnchorExpansion = stride3;
    if (keepRuns) unsetenv("CPECAN_KEEP_RUNS");
    else setenv("CPECAN_KEEP_RUNS", "0", 1);
    cpecan_batch *b = NULL;
    CHECK(cpecan_batch_create(&b, &model, &params, CPECAN_EMIT_MATCH, 0) == CPECAN_OK);
    Model m;
    memset(&m, 0, sizeof m);
    m.stride = stride3 ? 3 : 2;
    m.runForm = (form != TRIPLES && !stride3 && keepRuns) ? 1 : 0; /* decided by the batch's first call */
    uint64_t got[5], want[5];

    CHECK(add_call(b, ps, 0, cut, form) == 0);
    for (int64_t i = 0; i < cut; i++) model_add(&m, &ps[i], form != TRIPLES, is_minus(form, i), split);
    CHECK(cpk_batch_intake_digest(b, got) == CPECAN_OK);
    model_digest(&m, want);
    CHECK(same_digest(got, want));

    /* a call with a bad problem in the middle (two runs swapped) fails, names it and changes nothing */
    const Problem *bad = &ps[cut + (n - cut) / 2];
    if (bad->nRuns >= 2) {
        int64_t t[4];
        memcpy(t, bad->runs, sizeof t);
        memcpy(bad->runs, bad->runs + 4, sizeof t);
        memcpy(bad->runs + 4, t, sizeof t);
        char expect[64];
        snprintf(expect, sizeof expect, "problem %lld of the call", (long long)((n - cut) / 2));
        CHECK(add_call(b, ps, cut, n, RUNS) == CPECAN_EINVAL);
        CHECK(strstr(cpk_last_error(), expect) != NULL);
        memcpy(bad->runs + 4, bad->runs, sizeof t);
        memcpy(bad->runs, t, sizeof t);
        CHECK(cpk_batch_intake_digest(b, got) == CPECAN_OK);
        CHECK(same_digest(got, want));
    }

    CHECK(add_call(b, ps, cut, n, form2) == cut);
    for (int64_t i = cut; i < n; i++) model_add(&m, &ps[i], form2 != TRIPLES, is_minus(form2, i), split);
    CHECK(cpk_batch_intake_digest(b, got) == CPECAN_OK);
    model_digest(&m, want);
    CHECK(same_digest(got, want));
    CHECK(m.nRegions > m.nProblems); /* problems were cut */
    for (int64_t i = 0; i < n; i++) CHECK(cpecan_batch_problem_strand(b, i) == (is_minus(i < cut ? form : form2, i) ? CPECAN_STRAND_MINUS : CPECAN_STRAND_PLUS));
    model_free(&m);
    cpecan_batch_destroy(b);
}

static void intake(void) {
    for (int size = 0; size < 2; size++) {
        int64_t n;
        Problem *ps = make_problems(size == 0 ? 70 : 5, &n);
        /* 70: a parallel call and a serial one, or two serial ones; 5: two serial calls */
        const int64_t cuts[2] = {size == 0 ? 70 : 2, size == 0 ? 30 : 7};
        for (int c = 0; c < 2; c++)
            for (int form = TRIPLES; form <= STRANDED; form++)
                for (int stride3 = 0; stride3 < 2; stride3++)
                    for (int keepRuns = 1; keepRuns >= (form == TRIPLES ? 1 : 0); keepRuns--) one_batch(ps, n, cuts[c], form, form, stride3, keepRuns);
        /* the form of the first call stays: triples then runs keep anchors, runs then triples keep runs */
        one_batch(ps, n, cuts[1], TRIPLES, STRANDED, 0, 1);
        one_batch(ps, n, cuts[1], RUNS, TRIPLES, 0, 1);
        for (int64_t i = 0; i < n; i++) free_problem(&ps[i]);
        free(ps);
    }
    unsetenv("CPECAN_KEEP_RUNS");
    CHECK(cutsSeen > 100); /* anchors fell on both sides of a cut */
    printf("%lld anchored problems were cut\n", (long long)cutsSeen);
}

/* ---- the overflow scan ---- */
static void overflow_scan(int nLists) {
    /* region 0: split, two segments, the second overflows (with three lists the first as well); region 1: whole, overflows;
     * region 2: whole, exactly full */
    CpkRegion rg[3];
    CpkSegment sg[4];
    memset(rg, 0, sizeof rg);
    memset(sg, 0, sizeof sg);
    rg[0].split = 1, rg[0].nSeg = 2, rg[0].segOff = 0, rg[0].outCap = 30, rg[0].outOff = 0;
    rg[1].nSeg = 1, rg[1].segOff = 2, rg[1].outCap = 50, rg[1].outOff = 30;
    rg[2].nSeg = 1, rg[2].segOff = 3, rg[2].outCap = 40, rg[2].outOff = 80;
    sg[0].outOff = 0, sg[0].outCap = 10;
    sg[1].outOff = 10, sg[1].outCap = 20;
    sg[2].outOff = 0, sg[2].outCap = 50;
    sg[3].outOff = 0, sg[3].outCap = 40;
    const int32_t countsIn[3][3] = {{-1, 60, 40}, {-1, 10, 0}, {-1, 70, 39}}; /* [list][region]; a split region's are made by the scan */
    const int32_t segCountsIn[3][4] = {{7, 25, 60, 40}, {12, 5, 10, 0}, {3, 20, 70, 39}};
    int32_t counts[9], segCounts[12];
    for (int l = 0; l < nLists; l++) {
        memcpy(counts + 3 * l, countsIn[l], sizeof countsIn[l]);
        memcpy(segCounts + 4 * l, segCountsIn[l], sizeof segCountsIn[l]);
    }
    int64_t total = -1;
    CHECK(cpk_overflow_scan(rg, 3, sg, 4, nLists, counts, segCounts, &total) == 1);
    if (nLists == 1) {
        CHECK(sg[0].outCap == 10 && sg[0].outOff == 0 && sg[1].outCap == 25 && sg[1].outOff == 10);
        CHECK(counts[0] == 7 + 20); /* clamped with the capacity the segment had */
        CHECK(rg[0].outCap == 35 && rg[1].outCap == 60 && rg[2].outCap == 40);
        CHECK(rg[0].outOff == 0 && rg[1].outOff == 35 && rg[2].outOff == 95 && total == 135);
    } else {
        CHECK(sg[0].outCap == 12 && sg[0].outOff == 0 && sg[1].outCap == 25 && sg[1].outOff == 12);
        CHECK(counts[0] == 7 + 20 && counts[3] == 10 + 5 && counts[6] == 3 + 20);
        CHECK(rg[0].outCap == 37 && rg[1].outCap == 70 && rg[2].outCap == 40);
        CHECK(rg[0].outOff == 0 && rg[1].outOff == 37 && rg[2].outOff == 107 && total == 147);
    }
    CHECK(sg[2].outCap == 50 && sg[3].outCap == 40 && sg[2].outOff == 0); /* a whole region's segments are not its business */
    for (int l = 0; l < nLists; l++) CHECK(counts[3 * l + 1] == countsIn[l][1] && counts[3 * l + 2] == countsIn[l][2]);
    /* the same counts against the grown capacities: nothing overflows, nothing is clamped, nothing moves */
    CpkRegion rg2[3];
    CpkSegment sg2[4];
    memcpy(rg2, rg, sizeof rg);
    memcpy(sg2, sg, sizeof sg);
    int64_t again = -1;
    CHECK(cpk_overflow_scan(rg, 3, sg, 4, nLists, counts, segCounts, &again) == 0 && again == total);
    CHECK(memcmp(rg, rg2, sizeof rg) == 0 && memcmp(sg, sg2, sizeof sg) == 0);
    CHECK(counts[0] == 7 + 25);
    if (nLists == 3) CHECK(counts[3] == 12 + 5 && counts[6] == 3 + 20);
}

int main(void) {
    intake();
    overflow_scan(1);
    overflow_scan(3);
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
