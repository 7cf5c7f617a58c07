/*
 * The host side of Viterbi decoding (cpecan_amd/csrc/cpecan_viterbi.c) without the library, HIP or a GPU, built together with
 * cpecan_host.c with -fsanitize=address,undefined by tests/test_viterbi_c.py: device_standins.h stands in for the device layer,
 * and the launch of cpk_viterbi.inl is a stub here that fails the program when it is reached.  main makes the host-only
 * calls from C: the argument checks of create / add / set_budget / set_form, info of problems of one and of several regions
 * against a restatement of the cut, run without a device, and cpecan_viterbi_replay and cpecan_viterbi_pairs over paths
 * written down here -- against the same additions spelled out, and with the malformed ops that must be refused.  Everything
 * is freed: the leak check of the sanitizer stays on.
 */
#include "device_standins.h"

#include <math.h>

#include "cpecan_viterbi.h"

int cpk_viterbi_launch(int device, const CpkModel *model, const CpkVitJob *job, double *sweepMs, double *tracebackMs) {
    (void)device, (void)model, (void)job, (void)sweepMs, (void)tracebackMs;
    NO_DEVICE;
}

static int same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static void argument_checks(void) {
    cpecan_model m5;
    cpecan_model_default(&m5, CPECAN_FIVE_STATE);
    cpecan_viterbi *v = NULL;
    CHECK(cpecan_viterbi_create(NULL, &m5, NULL, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_create(&v, NULL, NULL, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_create(&v, &m5, NULL, -1) == CPECAN_EINVAL);
    cpecan_model bad = m5;
    bad.type = 7;
    CHECK(cpecan_viterbi_create(&v, &bad, NULL, 0) == CPECAN_EINVAL);
    cpecan_params p;
    cpecan_params_default(&p);
    p.diagonalExpansion = 7;
    CHECK(cpecan_viterbi_create(&v, &m5, &p, 0) == CPECAN_EINVAL && v == NULL);
    CHECK(cpecan_viterbi_create(&v, &m5, NULL, 0) == CPECAN_OK && v != NULL);
    const int64_t notIncreasing[6] = {2, 2, 0, 1, 3, 0}, outside[3] = {4, 1, 0}, fine[3] = {1, 1, 0};
    CHECK(cpecan_viterbi_add(NULL, "ACGT", 4, "ACGT", 4, NULL, 0, 0, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_add(v, "ACGT", 4, "ACGT", 4, notIncreasing, 2, 0, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_add(v, "ACGT", 4, "ACGT", 4, outside, 1, 0, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_add(v, NULL, 4, "ACGT", 4, NULL, 0, 0, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_add(v, "ACGT", -1, "ACGT", 4, NULL, 0, 0, 0) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_add(v, "ACGT", 4, "ACGT", 4, NULL, 1, 0, 0) == CPECAN_EINVAL);
    cpecan_viterbi_info_t info;
    CHECK(cpecan_viterbi_info(v, 0, &info) == CPECAN_EINVAL); /* nothing was added */
    CHECK(cpecan_viterbi_add(v, "ACGT", 4, "ACGT", 4, fine, 1, 0, 0) == 0);
    CHECK(cpecan_viterbi_add(v, NULL, 0, NULL, 0, NULL, 0, 1, 1) == 1);
    CHECK(cpecan_viterbi_add(v, "ACGT", 4, NULL, 0, NULL, 0, 0, 1) == 2);
    CHECK(cpecan_viterbi_info(v, 0, &info) == CPECAN_OK && info.nRegions == 1 && info.nCells == 25 && info.nStates == 5 &&
          info.deviceBytes > 25);
    CHECK(cpecan_viterbi_info(v, 1, &info) == CPECAN_OK && info.nRegions == 1 && info.nCells == 1);
    CHECK(cpecan_viterbi_info(v, 2, &info) == CPECAN_OK && info.nRegions == 1 && info.nCells == 5);
    CHECK(cpecan_viterbi_info(v, 3, &info) == CPECAN_EINVAL && cpecan_viterbi_info(v, -1, &info) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_set_budget(v, 0) == CPECAN_EINVAL && cpecan_viterbi_set_budget(v, -5) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_set_form(v, -1) == CPECAN_EINVAL && cpecan_viterbi_set_form(v, 3) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_set_form(v, CPECAN_VITERBI_FORM_GLOBAL) == CPECAN_OK && cpecan_viterbi_set_form(v, CPECAN_VITERBI_FORM_LDS) == CPECAN_OK);
    cpecan_viterbi_result_t res;
    CHECK(cpecan_viterbi_result(v, 0, &res) == CPECAN_ESTATE);
    CHECK(cpecan_viterbi_run(v) == CPECAN_ENODEVICE && strstr(cpk_last_error(), "no usable HIP device"));
    CHECK(cpecan_viterbi_set_budget(v, 30) == CPECAN_OK);
    CHECK(cpecan_viterbi_run(v) == CPECAN_ENOMEM && strstr(cpk_last_error(), "bytes")); /* before the device is looked for */
    CHECK(cpecan_viterbi_result(v, 0, &res) == CPECAN_ESTATE);
    int64_t a = -1, b = -1, c = -1;
    double s = -1.0, t = -1.0;
    CHECK(cpecan_viterbi_launch_forms(v, &a, &b, &c) == CPECAN_OK && a == 0 && b == 0 && c == 0);
    CHECK(cpecan_viterbi_kernel_ms(v, &s, &t) == CPECAN_OK && s == 0.0 && t == 0.0);
    cpecan_viterbi_destroy(v);
    cpecan_viterbi_destroy(NULL);
}

/* Anchors with two large gaps and a small splitMatrixBiggerThanThis: the regions are those of cpecan_split_points, the
 * cells those of cpecan_band over each region's own anchors. */
static void regions_and_cells(int raggedLeft, int raggedRight) {
    enum { L = 400, NA = 18 };
    char sx[L], sy[L];
    for (int i = 0; i < L; i++) sx[i] = "ACGT"[(i * 7 + i / 5) % 4], sy[i] = "ACGT"[(i * 7 + i / 5 + (i % 11 == 0)) % 4];
    int64_t anchors[3 * NA];
    int64_t n = 0;
    for (int64_t x = 100; x < 390 && n < NA; x += 10) {
        if (x >= 160 && x < 260) continue; /* the second gap; the first is 0 .. 100 */
        anchors[3 * n] = x;
        anchors[3 * n + 1] = x;
        anchors[3 * n + 2] = 0;
        n++;
    }
    cpecan_model m3;
    cpecan_model_default(&m3, CPECAN_THREE_STATE);
    cpecan_params p;
    cpecan_params_default(&p);
    p.diagonalExpansion = 6;
    p.splitMatrixBiggerThanThis = 40 * 40;
    cpecan_viterbi *v = NULL;
    CHECK(cpecan_viterbi_create(&v, &m3, &p, 0) == CPECAN_OK);
    CHECK(cpecan_viterbi_add(v, sx, L, sy, L, anchors, n, raggedLeft, raggedRight) == 0);
    int64_t rects[4 * (NA + 2)], own[3 * NA];
    const int64_t nRects = cpecan_split_points(anchors, n, L, L, p.splitMatrixBiggerThanThis, raggedLeft, raggedRight, rects);
    CHECK(nRects == (raggedLeft ? 2 : 3));
    int64_t cells = 0, next = 0;
    for (int64_t k = 0; k < nRects; k++) {
        const int64_t x1 = rects[4 * k], y1 = rects[4 * k + 1], rX = rects[4 * k + 2] - x1, rY = rects[4 * k + 3] - y1;
        int64_t nOwn = 0;
        for (; next < n && anchors[3 * next] + anchors[3 * next + 1] < x1 + rX + y1 + rY; next++, nOwn++) {
            own[3 * nOwn] = anchors[3 * next] - x1;
            own[3 * nOwn + 1] = anchors[3 * next + 1] - y1;
            own[3 * nOwn + 2] = 0;
        }
        int64_t *band = malloc(sizeof(int64_t) * 3 * (size_t)(rX + rY + 1)); /* exactly the region's diagonals */
        CHECK(cpecan_band(own, nOwn, rX, rY, p.diagonalExpansion, 0, band) == CPECAN_OK);
        for (int64_t d = 0; d <= rX + rY; d++) cells += (band[3 * d + 2] - band[3 * d + 1]) / 2 + 1;
        free(band);
    }
    CHECK(next == n);
    cpecan_viterbi_info_t info;
    CHECK(cpecan_viterbi_info(v, 0, &info) == CPECAN_OK && info.nRegions == nRects && info.nCells == cells && info.nStates == 3);
    CHECK(info.deviceBytes > cells && info.deviceBytes < 8 * cells);
    CHECK(cpecan_viterbi_run(v) == CPECAN_ENODEVICE);
    cpecan_viterbi_destroy(v);
}

/* X = AGCG, Y = AGTTCG: match, match, two shortY, match, match. */
static void replay_and_pairs(void) {
    cpecan_model m5, m3;
    cpecan_model_default(&m5, CPECAN_FIVE_STATE);
    cpecan_model_default(&m3, CPECAN_THREE_STATE);
    CpkModel k;
    cpk_kernel_model(&m5, 0.0, &k);
    const char *sx = "AGCG", *sy = "AGTTCG";
    const int32_t ops[6] = {0, 2, 2, 2, 0, 2};
    const int sym[6] = {0, 2, 3, 3, 1, 2}; /* A G T T C G: A 0, C 1, G 2, T 3 */
    double want = k.start[0];
    want = want + (k.matchEm[0 * 5 + 0] + k.matchContinue);
    want = want + (k.matchEm[2 * 5 + 2] + k.matchContinue);
    want = want + (k.gapYEm[sym[2]] + k.shortOpenY);
    want = want + (k.gapYEm[sym[3]] + k.shortExtendY);
    want = want + (k.matchEm[1 * 5 + 1] + k.matchFromShortY);
    want = want + (k.matchEm[2 * 5 + 2] + k.matchContinue);
    want = want + k.end[0];
    double got = 0.0;
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 0, ops, 3, &got) == CPECAN_OK && same_bits(got, want) && isfinite(got));
    /* ragged ends: the ragged start prior of the match state is -inf in the five-state model */
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 1, 1, 0, 0, ops, 3, &got) == CPECAN_OK && got == -INFINITY);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 1, 1, 4, 0, ops, 3, &got) == CPECAN_OK && isfinite(got)); /* longY -> match */
    /* no ops: lX = lY = 0, start prior + end prior */
    CHECK(cpecan_viterbi_replay(&m5, NULL, 0, NULL, 0, 0, 0, 0, 0, NULL, 0, &got) == CPECAN_OK && same_bits(got, k.start[0] + k.end[0]));
    CHECK(cpecan_viterbi_replay(&m5, NULL, 0, NULL, 0, 0, 0, 0, 1, NULL, 0, &got) == CPECAN_EINVAL); /* nothing leads from 0 to 1 */
    /* malformed ops */
    const int32_t tooShort[4] = {0, 2, 2, 2}, tooLong[8] = {0, 2, 2, 2, 0, 2, 1, 1}, noSwitch[4] = {1, 4, 2, 6}, badState[4] = {5, 4, 2, 6},
                  zeroLength[6] = {0, 2, 2, 0, 0, 2}, longFromShort[6] = {0, 2, 2, 2, 4, 2};
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 2, tooShort, 2, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 1, tooLong, 4, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 2, noSwitch, 2, &got) == CPECAN_EINVAL && strstr(cpk_last_error(), "lacks"));
    CHECK(cpecan_viterbi_replay(&m3, sx, 4, sy, 6, 0, 0, 0, 2, noSwitch, 2, &got) == CPECAN_OK && isfinite(got)); /* three states switch */
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 2, badState, 2, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 0, zeroLength, 3, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 4, longFromShort, 3, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 1, ops, 3, &got) == CPECAN_EINVAL); /* ends in the match state, not in 1 */
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 5, 0, ops, 3, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(&m5, sx, 4, sy, 6, 0, 0, 0, 0, NULL, 3, &got) == CPECAN_EINVAL);
    CHECK(cpecan_viterbi_replay(NULL, sx, 4, sy, 6, 0, 0, 0, 0, ops, 3, &got) == CPECAN_EINVAL);
    /* pairs: two regions, the second at (10, 20); problem coordinates, 0-based */
    const int32_t two[10] = {0, 2, 2, 2, 0, 2, 1, 1, 0, 3};
    const cpecan_viterbi_region regs[3] = {{0, 0, 4, 6, -1.0, 0, 0, 0, 3}, {10, 20, 14, 23, -2.0, 3, 0, 3, 2}, {30, 30, 30, 30, -INFINITY, -1, -1, 5, 0}};
    const cpecan_viterbi_result_t res = {-3.0, 3, 5, regs, two};
    int64_t xy[2 * 7];
    const int64_t wantXy[14] = {0, 0, 1, 1, 2, 4, 3, 5, 11, 20, 12, 21, 13, 22};
    CHECK(cpecan_viterbi_pairs(&res, NULL, 0) == 7);
    CHECK(cpecan_viterbi_pairs(&res, xy, 7) == 7 && memcmp(xy, wantXy, sizeof wantXy) == 0);
    memset(xy, 0xff, sizeof xy);
    CHECK(cpecan_viterbi_pairs(&res, xy, 2) == 7 && memcmp(xy, wantXy, 4 * sizeof(int64_t)) == 0 && xy[4] == -1); /* no more than cap */
    CHECK(cpecan_viterbi_pairs(NULL, xy, 7) == CPECAN_EINVAL && cpecan_viterbi_pairs(&res, NULL, 7) == CPECAN_EINVAL);
}

int main(void) {
    argument_checks();
    for (int rl = 0; rl < 2; rl++)
        for (int rr = 0; rr < 2; rr++) regions_and_cells(rl, rr);
    replay_and_pairs();
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
