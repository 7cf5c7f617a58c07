/*
 * cpecan_band_edge_of_pairs (cpecan_amd/csrc/cpecan_host.c) without the library, HIP or a GPU, built with
 * -fsanitize=address,undefined by tests/test_band_edge_c.py: device_standins.h stands in for the device layer cpecan_host.c
 * calls, none of which the function under test reaches.  main runs the function over the edge shapes -- an empty list, lX or lY 0,
 * a diagonal of one cell, a pair on a region's last diagonal, pairs in the first and last cell of neighbouring regions,
 * pairs that lie in no region -- and over a few hundred random problems against a restatement that walks every region
 * for every pair.  Everything is freed: the leak check of the sanitizer stays on.
 */
#include "device_standins.h"

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static int64_t rnd(int64_t n) { /* 0 .. n - 1 */
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((rngState >> 33) % (uint64_t)n);
}

/* ---- the definition once more, the slow way: every region for every pair ---- */
static int restated(const int64_t *anchors, int64_t nAnchors, int64_t lX, int64_t lY, const cpecan_params *p, int rl, int rr,
                    const int32_t *t, int64_t n, cpecan_band_edge *out) {
    memset(out, 0, sizeof *out);
    int64_t *rects = malloc(sizeof(int64_t) * 4 * (size_t)(nAnchors + 2));
    int64_t *own = malloc(sizeof(int64_t) * 3 * (size_t)(nAnchors + 1));
    const int64_t nRects = cpecan_split_points(anchors, nAnchors, lX, lY, p->splitMatrixBiggerThanThis, rl, rr, rects);
    int64_t next = 0, placed = 0;
    int rc = nRects < 0 ? (int)nRects : CPECAN_OK;
    for (int64_t k = 0; rc == CPECAN_OK && k < nRects; k++) {
        const int64_t x1 = rects[4 * k], y1 = rects[4 * k + 1], rX = rects[4 * k + 2] - x1, rY = rects[4 * k + 3] - y1;
        int64_t nOwn = 0;
        for (; next < nAnchors && anchors[3 * next] + anchors[3 * next + 1] < x1 + rX + y1 + rY; next++, nOwn++) {
            own[3 * nOwn] = anchors[3 * next] - x1;
            own[3 * nOwn + 1] = anchors[3 * next + 1] - y1;
            own[3 * nOwn + 2] = anchors[3 * next + 2];
        }
        int64_t *band = malloc(sizeof(int64_t) * 3 * (size_t)(rX + rY + 1)); /* exactly the region's diagonals: a read past them is caught */
        rc = cpecan_band(own, nOwn, rX, rY, p->diagonalExpansion, p->dynamicAnchorExpansion, band);
        for (int64_t i = 0; rc == CPECAN_OK && i < n; i++) {
            const int64_t x = t[3 * i + 1] - x1 + 1, y = t[3 * i + 2] - y1 + 1; /* matrix coordinates of the region */
            if (x < 1 || y < 1 || x > rX || y > rY) continue;
            placed++;
            const int64_t lo = band[3 * (x + y) + 1], hi = band[3 * (x + y) + 2];
            if ((x - y == lo && x - 1 >= 0 && y + 1 <= rY) || (x - y == hi && x + 1 <= rX && y - 1 >= 0)) {
                out->edgePairs++;
                out->edgeScoreSum += t[3 * i];
                if (t[3 * i] > out->edgeScoreMax) out->edgeScoreMax = t[3 * i];
            }
        }
        free(band);
    }
    free(rects);
    free(own);
    if (rc == CPECAN_OK && placed != n) rc = CPECAN_EINVAL;
    return rc;
}

static int same(const cpecan_band_edge *a, const cpecan_band_edge *b) {
    return a->edgePairs == b->edgePairs && a->edgeScoreSum == b->edgeScoreSum && a->edgeScoreMax == b->edgeScoreMax && a->reserved == 0;
}

static void edge_shapes(void) {
    cpecan_params p;
    cpecan_params_default(&p);
    p.diagonalExpansion = 0;
    cpecan_band_edge e, zero;
    memset(&zero, 0, sizeof zero);
    /* an empty list, with and without anchors; NULL pairs are fine when there are none */
    memset(&e, 0xff, sizeof e);
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 5, 7, &p, 0, 0, NULL, 0, &e) == CPECAN_OK && same(&e, &zero));
    const int64_t one[3] = {2, 3, 0};
    memset(&e, 0xff, sizeof e);
    CHECK(cpecan_band_edge_of_pairs(one, 1, 5, 7, &p, 1, 1, NULL, 0, &e) == CPECAN_OK && same(&e, &zero));
    /* lX or lY 0: a matrix of one row or column holds no pair */
    const int32_t pair00[3] = {9, 0, 0};
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 0, 0, &p, 0, 0, NULL, 0, &e) == CPECAN_OK && same(&e, &zero));
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 0, 6, &p, 0, 0, NULL, 0, &e) == CPECAN_OK && same(&e, &zero));
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 6, 0, &p, 1, 0, NULL, 0, &e) == CPECAN_OK && same(&e, &zero));
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 0, 6, &p, 0, 0, pair00, 1, &e) == CPECAN_EINVAL && same(&e, &zero));
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 6, 0, &p, 0, 0, pair00, 1, &e) == CPECAN_EINVAL);
    /* E = 0 along the main diagonal of 6 x 6: the anchors' own diagonals hold one cell, cut on both sides and counted once;
     * the first and the last pair sit where the matrix cuts.  The last pair is on the region's last diagonal. */
    int64_t diag[3 * 4];
    int32_t onDiag[3 * 6];
    for (int i = 0; i < 4; i++) diag[3 * i] = diag[3 * i + 1] = i + 1, diag[3 * i + 2] = 0;
    for (int i = 0; i < 6; i++) onDiag[3 * i] = 100 + i, onDiag[3 * i + 1] = onDiag[3 * i + 2] = i;
    CHECK(cpecan_band_edge_of_pairs(diag, 4, 6, 6, &p, 0, 0, onDiag, 6, &e) == CPECAN_OK);
    CHECK(e.edgePairs == 4 && e.edgeScoreSum == 101 + 102 + 103 + 104 && e.edgeScoreMax == 104 && e.reserved == 0);
    CHECK(cpecan_band_edge_of_pairs(diag, 4, 6, 6, &p, 0, 0, onDiag + 15, 1, &e) == CPECAN_OK && same(&e, &zero)); /* (5, 5) alone */
    /* an anchor in the last cell: the last diagonal's one cell is the matrix corner */
    const int64_t corner[3] = {5, 5, 0};
    CHECK(cpecan_band_edge_of_pairs(corner, 1, 6, 6, &p, 0, 0, onDiag + 15, 1, &e) == CPECAN_OK && same(&e, &zero));
    /* two regions: (1, 1) and (58, 58) leave a gap of 56 x 56 > 100 cells, cut 10 deep at either side */
    p.diagonalExpansion = 4;
    p.splitMatrixBiggerThanThis = 100;
    const int64_t far[6] = {1, 1, 4, 58, 58, 4};
    int64_t rects[4 * 4];
    CHECK(cpecan_split_points(far, 2, 60, 60, 100, 0, 0, rects) == 2);
    const int32_t corners[3 * 4] = {5, (int32_t)rects[2] - 1, (int32_t)rects[3] - 1,  /* last cell of region 0: its last diagonal */
                                    6, (int32_t)rects[4], (int32_t)rects[5],          /* first cell of region 1 */
                                    7, 59, 59, 8, 0, 0};
    cpecan_band_edge want;
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, corners, 4, &e) == CPECAN_OK);
    CHECK(restated(far, 2, 60, 60, &p, 0, 0, corners, 4, &want) == CPECAN_OK && same(&e, &want));
    const int32_t between[3] = {5, 30, 30}, outside[3] = {5, 60, 3}, negative[3] = {5, -1, 3};
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, between, 1, &e) == CPECAN_EINVAL && same(&e, &zero));
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, outside, 1, &e) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, negative, 1, &e) == CPECAN_EINVAL);
    /* arguments */
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, NULL, 0, 0, corners, 4, &e) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, corners, 4, NULL) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, NULL, 4, &e) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(NULL, 2, 60, 60, &p, 0, 0, corners, 4, &e) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(far, 2, -1, 60, &p, 0, 0, corners, 4, &e) == CPECAN_EINVAL);
    CHECK(cpecan_band_edge_of_pairs(far, 2, 60, 60, &p, 0, 0, corners, -1, &e) == CPECAN_EINVAL);
    const int64_t backwards[6] = {8, 8, 4, 3, 9, 4};
    CHECK(cpecan_band_edge_of_pairs(backwards, 2, 60, 60, &p, 0, 0, corners + 9, 1, &e) == CPECAN_EINVAL);
    p.diagonalExpansion = 3;
    CHECK(cpecan_band_edge_of_pairs(NULL, 0, 6, 6, &p, 0, 0, pair00, 1, &e) == CPECAN_EINVAL);
}

static void random_problems(void) {
    int64_t withEdges = 0, split = 0;
    for (int trial = 0; trial < 400; trial++) {
        cpecan_params p;
        cpecan_params_default(&p);
        p.dynamicAnchorExpansion = trial % 3 == 0;
        p.diagonalExpansion = 2 * rnd(6);
        p.splitMatrixBiggerThanThis = trial % 2 ? 40 + rnd(100) : 9000000;
        const int64_t lX = 1 + rnd(90), lY = 1 + rnd(90);
        int64_t *anchors = malloc(sizeof(int64_t) * 3 * (size_t)(lX + 1)), nAnchors = 0;
        for (int64_t x = rnd(6), y = rnd(6); x < lX && y < lY; x += 1 + rnd(trial % 4 > 1 ? 3 : 25), y += 1 + rnd(trial % 4 > 1 ? 3 : 25)) {
            anchors[3 * nAnchors] = x;
            anchors[3 * nAnchors + 1] = y;
            anchors[3 * nAnchors++ + 2] = p.dynamicAnchorExpansion ? 2 * rnd(6) : p.diagonalExpansion;
        }
        const int rl = (int)rnd(2), rr = (int)rnd(2);
        int64_t *rects = malloc(sizeof(int64_t) * 4 * (size_t)(nAnchors + 2)), *band = NULL;
        const int64_t nRects = cpecan_split_points(anchors, nAnchors, lX, lY, p.splitMatrixBiggerThanThis, rl, rr, rects);
        CHECK(nRects >= 0); /* (0: both ends ragged and nothing but one large gap) */
        split += nRects > 1;
        /* pairs: cells of the regions' bands, most of them on a band's first or last cell */
        const int64_t n = rnd(120);
        int32_t *t = malloc(sizeof(int32_t) * 3 * (size_t)(n + 1));
        int64_t at = 0, next = 0;
        for (int64_t k = 0; k < nRects; k++) {
            const int64_t x1 = rects[4 * k], y1 = rects[4 * k + 1], rX = rects[4 * k + 2] - x1, rY = rects[4 * k + 3] - y1;
            int64_t *own = malloc(sizeof(int64_t) * 3 * (size_t)(nAnchors + 1)), nOwn = 0;
            for (; next < nAnchors && anchors[3 * next] + anchors[3 * next + 1] < x1 + rX + y1 + rY; next++, nOwn++) {
                own[3 * nOwn] = anchors[3 * next] - x1;
                own[3 * nOwn + 1] = anchors[3 * next + 1] - y1;
                own[3 * nOwn + 2] = anchors[3 * next + 2];
            }
            band = realloc(band, sizeof(int64_t) * 3 * (size_t)(rX + rY + 1));
            CHECK(cpecan_band(own, nOwn, rX, rY, p.diagonalExpansion, p.dynamicAnchorExpansion, band) == CPECAN_OK);
            free(own);
            for (int64_t q = 0; q < n / nRects && rX > 0 && rY > 0; q++) {
                const int64_t d = 2 + rnd(rX + rY - 1), lo = band[3 * d + 1], hi = band[3 * d + 2];
                const int64_t pick = rnd(3), xmy = pick == 0 ? lo : (pick == 1 ? hi : lo + 2 * rnd((hi - lo) / 2 + 1));
                const int64_t x = (d + xmy) / 2, y = (d - xmy) / 2;
                if (x < 1 || y < 1) continue; /* the matrix's first row or column: no pair */
                t[3 * at] = (int32_t)(1 + rnd(10000000));
                t[3 * at + 1] = (int32_t)(x - 1 + x1);
                t[3 * at++ + 2] = (int32_t)(y - 1 + y1);
            }
        }
        cpecan_band_edge got, want;
        CHECK(cpecan_band_edge_of_pairs(anchors, nAnchors, lX, lY, &p, rl, rr, t, at, &got) == CPECAN_OK);
        CHECK(restated(anchors, nAnchors, lX, lY, &p, rl, rr, t, at, &want) == CPECAN_OK);
        CHECK(same(&got, &want));
        withEdges += want.edgePairs > 0;
        free(band);
        free(t);
        free(rects);
        free(anchors);
    }
    CHECK(withEdges > 100 && split > 50);
    printf("%lld of 400 random problems have edge pairs, %lld are cut into several regions\n", (long long)withEdges, (long long)split);
}

int main(void) {
    CHECK(sizeof(cpecan_band_edge) == 24);
    edge_shapes();
    random_problems();
    printf("%d failure(s)\n", failures);
    return failures != 0;
}
