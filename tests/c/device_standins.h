/*
 * What a stand-alone test program of cpecan_amd/csrc/cpecan_host.c links in place of the device layer (cpecan_kernels.hip):
 * the host pool as plain malloc, the error text, and stubs that fail the program when the code under test reaches a device.
 * Included once, by the program's one source file (test_band_edge.c, test_intake.c); brings CHECK and the failure count.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_internal.h"

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

static char lastError[512];
void cpk_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(lastError, sizeof lastError, fmt, ap);
    va_end(ap);
}
const char *cpk_last_error(void) { return lastError; }
void *cpk_host_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void cpk_host_free(void *p) { free(p); }
void *cpk_host_grow(void *p, size_t usedBytes, size_t newBytes) {
    (void)usedBytes;
    return realloc(p, newBytes);
}
#define NO_DEVICE                      \
    do {                               \
        CHECK(!"the device layer ran"); \
        return CPECAN_ENODEVICE;       \
    } while (0)
int cpk_ref_cells(int device, const CpkModel *model, int mode, const CpkCellOp *ops, int64_t n, double *buf, int64_t nDoubles, double total) {
    (void)device, (void)model, (void)mode, (void)ops, (void)n, (void)buf, (void)nDoubles, (void)total;
    NO_DEVICE;
}
int cpk_device_count(void) { return 0; }
int64_t cpk_cache_trim(int device) {
    (void)device;
    return 0;
}
int cpk_current_device(void) { return 0; }
int cpk_device_create(CpkDevice **out, int device) {
    (void)out, (void)device;
    NO_DEVICE;
}
void cpk_device_destroy(CpkDevice *dev) { (void)dev; }
int cpk_device_upload(CpkDevice *dev, const CpkBatchPlan *plan, const CpkModel *model, double *h2dMs) {
    (void)dev, (void)plan, (void)model, (void)h2dMs;
    NO_DEVICE;
}
double cpk_device_h2d_ms(CpkDevice *dev) {
    (void)dev;
    return 0.0;
}
int cpk_device_update_regions(CpkDevice *dev, const CpkRegion *regions, const CpkSegment *segs, int64_t outTriplesPerList) {
    (void)dev, (void)regions, (void)segs, (void)outTriplesPerList;
    NO_DEVICE;
}
int cpk_device_set_model(CpkDevice *dev, const CpkModel *model) {
    (void)dev, (void)model;
    NO_DEVICE;
}
int cpk_device_set_models(CpkDevice *dev, const CpkModel *models, int n) {
    (void)dev, (void)models, (void)n;
    NO_DEVICE;
}
int cpk_device_run(CpkDevice *dev, void *stream) {
    (void)dev, (void)stream;
    NO_DEVICE;
}
int cpk_device_form(const CpkDevice *dev) {
    (void)dev;
    return 0;
}
int cpk_device_rerun(CpkDevice *dev) {
    (void)dev;
    NO_DEVICE;
}
int cpk_device_download(CpkDevice *dev, int32_t *counts, int32_t *segStarts, int32_t *segCounts, double *expect, double *kernelMs,
                        double *d2hMs) {
    (void)dev, (void)counts, (void)segStarts, (void)segCounts, (void)expect, (void)kernelMs, (void)d2hMs;
    NO_DEVICE;
}
int cpk_device_gather(CpkDevice *dev, const CpkChunk *chunks, int64_t nChunks, int64_t total) {
    (void)dev, (void)chunks, (void)nChunks, (void)total;
    NO_DEVICE;
}
int cpk_device_band_edge(CpkDevice *dev, int64_t nChunks0, const int32_t *chunkRegion, const int32_t *chunkProblem, int64_t nProblems,
                         cpecan_band_edge *out) {
    (void)dev, (void)nChunks0, (void)chunkRegion, (void)chunkProblem, (void)nProblems, (void)out;
    NO_DEVICE;
}
int cpk_device_fetch(CpkDevice *dev, int32_t *hostOut, int64_t total, double *d2hMs) {
    (void)dev, (void)hostOut, (void)total, (void)d2hMs;
    NO_DEVICE;
}
int cpk_device_post(CpkDevice *dev, const CpkPostJob *job) {
    (void)dev, (void)job;
    NO_DEVICE;
}
int cpk_post_lists(int device, int32_t *triples, int64_t total, const CpkPostJob *job) {
    (void)device, (void)triples, (void)total, (void)job;
    NO_DEVICE;
}
int cpk_device_debug_fetch(CpkDevice *dev, double *fb, int64_t cells, double *totals, int64_t diags) {
    (void)dev, (void)fb, (void)cells, (void)totals, (void)diags;
    NO_DEVICE;
}
int cpk_device_table_fetch(CpkDevice *dev, const CpkRegion *rg, int dynamic, CpkDiag *diags, int32_t *dpos, int *hasPos,
                           int64_t *ringDoubles) {
    (void)dev, (void)rg, (void)dynamic, (void)diags, (void)dpos, (void)hasPos, (void)ringDoubles;
    NO_DEVICE;
}
int64_t cpk_device_bytes(const CpkDevice *dev) {
    (void)dev;
    return 0;
}
int cpk_device_waves(const CpkDevice *dev) {
    (void)dev;
    return 0;
}
