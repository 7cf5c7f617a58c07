/*
 * cpecan_internal.h -- structures shared by the C host code (cpecan_host.c) and the HIP
 * translation unit (cpecan_kernels.hip).  Not part of the public ABI.
 */
#ifndef CPECAN_INTERNAL_H_
#define CPECAN_INTERNAL_H_

#include <stddef.h>
#include <stdint.h>

#include "cpecan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CPK_MAX_STATES 5
#define CPK_SYM_N 4
#define CPK_WAVE 64
#define CPK_REFRESH_PERIOD 10 /* total probability is refreshed every 10th emitted diagonal, pairwiseAligner.c:830 */

/* One anti-diagonal of a region's band, as the kernels read it (one 16-byte scalar load). */
typedef struct {
    int32_t xmyL;    /* smallest x-y on the diagonal */
    int32_t width;   /* number of cells */
    int32_t ringOff; /* first cell of this diagonal inside the region's forward ring (in cells) */
    int32_t cellOff; /* number of band cells on earlier diagonals of the region */
} CpkDiag;

/* One traceback segment (pairwiseAligner.c:791-862): the forward sweep runs up to dTop, then the
 * backward sweep runs from dTop down to tbPrev+1 and diagonals tbPrev+1..tbFrom are emitted. */
typedef struct {
    int32_t tbPrev;   /* tracedBackTo on entry */
    int32_t dTop;     /* diagonal the traceback starts from */
    int32_t tbFrom;   /* tracedBackFrom: highest emitted diagonal */
    int32_t atEnd;    /* dTop == lX+lY */
    int32_t nRefresh; /* number of total-probability refresh points in the segment */
    int32_t outOff;   /* the segment's own part of the region's output slice (per list), used when the tracebacks of a */
    int32_t outCap;   /* region run as separate queue items (split classes): first triple and capacity */
    int32_t emitCells; /* band cells on the emitted diagonals tbPrev+1..tbFrom: no list of the segment can be longer */
} CpkSegment;

/* One traceback work item of a split class: segment `seg` (index within its region) of device region `region`.
 * seg = -K < 0: a CHAIN -- the forward sweep of the region's segments K .. last, resumed from the two diagonals the ring
 * holds at the top of segment K - 1, and then their tracebacks, by one wave (cpk_sweep.inl "CHAIN"; cpk_plan.inl). */
typedef struct {
    int32_t region, seg;
} CpkItem;

/* One DP region (a whole problem, or one rectangle of getSplitPoints). */
typedef struct {
    int64_t seqXOff, seqYOff; /* byte offsets of the padded symbol strings (symbol[0] = N, symbol[i] = base i-1) */
    int64_t diagOff;          /* index of the region's first CpkDiag */
    int64_t segOff;           /* index of the region's first CpkSegment */
    int64_t outOff;           /* first output triple slot of the region (per output list) */
    int64_t dbgCellOff;       /* debug: first cell in the debug fb array */
    int64_t dbgDiagOff;       /* debug: first diagonal in the debug total array */
    int64_t anchorOff;        /* first anchor triple of the region (coordinates relative to the region) */
    int64_t ringBase;         /* split classes: first cell of the region's own forward ring (it holds every segment) */
    int64_t cells;            /* band cells of the region */
    int32_t lX, lY;
    int32_t nSeg;
    int32_t outCap;           /* capacity in triples (per output list) */
    int32_t raggedLeft, raggedRight;
    int32_t maxWidth;
    int32_t ringCap;          /* cells of forward ring the region needs: its longest live span + its widest diagonal */
    int32_t nAnchors;
    int32_t split;            /* set by the device layer: the region's tracebacks run as separate queue items */
    int32_t absOk;            /* planning: the band's edges move by one x-y step per diagonal (absolute-position sweeps allowed) */
} CpkRegion;

/* Model constants as the kernels use them: per-state priors, named transitions and padded emissions. */
typedef struct {
    int32_t nStates;
    int32_t type;
    double start[CPK_MAX_STATES], raggedStart[CPK_MAX_STATES];
    double end[CPK_MAX_STATES], raggedEnd[CPK_MAX_STATES];
    /* transitions, log space */
    double matchContinue;
    double matchFromShortX, matchFromShortY, matchFromLongX, matchFromLongY;
    double shortOpenX, shortOpenY, shortExtendX, shortExtendY, shortSwitchToX, shortSwitchToY;
    double longOpenX, longOpenY, longExtendX, longExtendY;
    /* emissions with the N row/column filled in (stateMachine.c:351-366) */
    double matchEm[25]; /* [cX*5+cY] */
    double gapXEm[5], gapYEm[5];
    double threshold;
} CpkModel;

#define CPK_WIDE_CLASSES 8
/* Per-launch geometry computed on the host. */
typedef struct {
    int32_t nRegions;
    int32_t nStates;
    int32_t emit;
    int32_t maxWidth;     /* widest diagonal in the batch */
    int32_t rollStride;   /* doubles per state row of a rolling buffer (maxWidth + the -inf guard at position 0) */
    int32_t maxRefresh;   /* most refresh points in any segment */
    int32_t useGlobalRoll;/* slow path: rolling buffers and symbol strings stay in global memory (too big for LDS) */
    int32_t seqLdsBytes;  /* fast path: bytes of LDS for the two padded symbol strings of the largest region */
    int32_t debug;        /* 0 or 1: the sweeps fill the debug buffers (F + B of every emitted cell, the totals used) */
    int32_t fusedSpin;    /* one-launch form: polls of an item for its region's forward values before it gives up (reported, re-run in two launches) */
    int32_t expInSweep;   /* expectation emitter: the events are formed inside the traceback (every diagonal of the class fits one 64-lane group) */
    int32_t absWholeStrings; /* absolute-position sweeps stage both whole symbol strings, not a window per segment (CPECAN_ABS_WINDOWS=0) */
    int64_t ringCells;    /* forward ring capacity per slot, in cells */
    int64_t fbCells;      /* posterior-candidate scratch per slot, in cells (most emitted cells of one segment) */
    int64_t refreshCells; /* c/m scratch per slot = maxWidth * maxRefresh (each) */
    int64_t rollDoubles;  /* global rolling buffer per slot, doubles (only when useGlobalRoll) */
    /* Narrow regions come first in the device order, by class: every diagonal at most 8 / 16 / 32 cells wide.  Class k
     * is run by the packed kernel with groups of 8 << k lanes (64 / (8 << k) regions per wave); the fields above then
     * describe the remaining (wide) regions only and these the narrow classes.  nPacked[k] == 0: no launch. */
    int32_t nPacked[3];
    int32_t pMaxRefresh[3];
    int64_t pRingCells[3], pFbCells[3];
    /* The wide regions follow, again by class: widest diagonal at most 128 / 192 / 256 / 384 / 512 cells, wider but
     * still inside the 64 KiB LDS budget, or wider still (global-memory rolling buffers).  Every class is one launch of the sweep kernel with LDS and per-wave scratch sized
     * for ITS largest region, so that one very wide region neither takes the LDS that decides how many waves the others
     * get nor multiplies everybody's scratch.  The scalar fields above are filled per launch from these. */
    int32_t nWide[CPK_WIDE_CLASSES];
    int32_t wMaxWidth[CPK_WIDE_CLASSES], wMaxRefresh[CPK_WIDE_CLASSES], wSeqLdsBytes[CPK_WIDE_CLASSES];
    int32_t wWinLdsBytes[CPK_WIDE_CLASSES]; /* the same for a class that stages symbol windows per traceback segment (absolute positions) */
    int64_t wRingCells[CPK_WIDE_CLASSES], wFbCells[CPK_WIDE_CLASSES];
} CpkGeometry;

/* One run of consecutive triples to move into the compact, list-ordered result buffer: the triples of one traceback
 * segment of one region, shifted by the region's offset inside its problem (pairwiseAligner.c:1411-1418). */
typedef struct {
    int64_t src;     /* first triple in the kernel's output (list offset included) */
    int64_t dst;     /* first triple in the compact buffer */
    int32_t len;
    int32_t dx, dy;  /* added to x and y */
    int32_t pad;
} CpkChunk;

/* Device-side mirror of a frozen batch; owned by the HIP TU. */
typedef struct CpkDevice CpkDevice;

/* One operation of cpk_ref_cells (cpk_cells.inl): offsets, in doubles, of the cells in the flat buffer; -1 = NULL.
 * Layout shared with include/cpecan_hip.h's cpecan_cell_op. */
typedef struct {
    int32_t cur, lower, middle, upper;
    int32_t cX, cY;
} CpkCellOp;

/* ---- implemented in cpecan_kernels.hip ---- */
/* The reference's cell-level primitives on the current device: `n` operations applied in order by one lane to the
 * `nDoubles` doubles of buf (copied up, changed in place, copied back).  mode 0 forward, 1 backward, 2 posterior. */
int cpk_ref_cells(int device, const CpkModel *model, int mode, const CpkCellOp *ops, int64_t n, double *buf, int64_t nDoubles,
                  double total);
/* Host blocks of a batch: pinned and recycled when a HIP device is present, plain malloc below 256 KB or without a GPU. */
void *cpk_host_alloc(size_t bytes);
void cpk_host_free(void *p);
void *cpk_host_grow(void *p, size_t usedBytes, size_t newBytes); /* NULL on failure: p is still valid then */
int cpk_device_count(void);
int64_t cpk_cache_trim(int device); /* idle device blocks of `device` (-1: all) and idle host blocks -> driver / OS; bytes */
int cpk_current_device(void); /* the calling thread's current HIP device (0 when there is none) */
const char *cpk_last_error(void);
int cpk_device_create(CpkDevice **out, int device);
void cpk_device_destroy(CpkDevice *dev);
/* A planned batch as the device layer is told about it: built in one place (cpecan_host.c, batch_plan_record) from the
 * batch, its plan and the geometry; read by cpk_device_upload and, without a device, by cpk_plan_describe / cpk_plan_chains. */
typedef struct {
    CpkGeometry geo;
    CpkRegion *regions;     /* device order.  Regions of a class that is split (see CpkItem) get ringCap / ringBase / split set
                             * here, in the caller's array, by cpk_device_upload and cpk_plan_chains */
    const CpkSegment *segs; /* the regions' traceback segments (CpkRegion::segOff) */
    int64_t nSegs, nDiags;  /* nDiags: entries of the per-diagonal table, built on the device from the anchors (cpecan_band.inl) */
    const int32_t *anchors; /* cpk_anchor_t (cpecan_band.inl), anchorStride values each; NULL for a batch that holds runs */
    const int32_t *runs;    /* or: (x, y, length, first anchor) per run, expanded on the device */
    int64_t nAnchors, nRuns; /* nAnchors: one per column, whichever form they are held in */
    int64_t expansion;
    const uint8_t *symbols;
    int64_t nSymbolBytes, outTriplesPerList, dbgCells, dbgDiags;
    int32_t anchorStride, nLists;
    int32_t dynamic;        /* per-anchor expansions are in force */
    int32_t modelSlots;     /* models reserved per run (cpecan_batch_reserve_models); 0: a plain batch -- expectation and forward
                             * emitters only; wave counts and everything per wave are planned for that many times the regions */
} CpkBatchPlan;
/* Plans the launches of the batch (cpk_plan.inl), copies the packed inputs to the GPU and sizes every scratch buffer. */
int cpk_device_upload(CpkDevice *dev, const CpkBatchPlan *plan, const CpkModel *model, double *h2dMs);
double cpk_device_h2d_ms(CpkDevice *dev); /* the upload's copy time; waits for the copies */
int cpk_device_update_regions(CpkDevice *dev, const CpkRegion *regions, const CpkSegment *segs, int64_t outTriplesPerList);
/* Replaces the model the next cpk_device_run uses (kernel-argument transitions and the device CpkModel); the copy is
 * ordered behind the last run on the batch's own stream and in front of the next sweep. */
int cpk_device_set_model(CpkDevice *dev, const CpkModel *model);
/* Model slots (CpkBatchPlan::modelSlots = nSlots > 0): the n models of the next run, 1 <= n <= nSlots, ordered on the stream
 * as cpk_device_set_model orders its one.  cpk_device_download then fills `expect` per slot: [n][106] sums, or [n][nRegions]
 * forward probabilities. */
int cpk_device_set_models(CpkDevice *dev, const CpkModel *models, int n);
int cpk_device_run(CpkDevice *dev, void *stream);
int cpk_device_form(const CpkDevice *dev); /* CPECAN_FORM_* of the batch's last (widest) size class */
/* Once more on the stream of the last run (after an output overflow); kernel times of a batch's launches add up. */
int cpk_device_rerun(CpkDevice *dev);
/* Blocks until the run is complete and copies back the per-region counts and per-segment start offsets (and the
 * expectation sums / forward probabilities). The triples stay on the device: see cpk_device_gather. */
int cpk_device_download(CpkDevice *dev, int32_t *counts /* [nLists][nRegions] */,
                        int32_t *segStarts /* [nLists][nSegsTotal] */, int32_t *segCounts /* [nLists][nSegsTotal]: split regions */,
                        double *expect /* [106] */, double *kernelMs, double *d2hMs);
/* Moves the chunks into one compact buffer on the device (reference list order, region offsets applied). */
int cpk_device_gather(CpkDevice *dev, const CpkChunk *chunks, int64_t nChunks, int64_t total);
/* Posterior mass on the band's edge (cpecan_band_edge, cpecan_hip.h), behind cpk_device_gather and in front of
 * cpk_device_post: the first nChunks0 chunks of the gather -- those of list 0 -- each with its device region and its
 * problem; out receives nProblems records.  Counters and the two index arrays live for the duration of the call. */
int cpk_device_band_edge(CpkDevice *dev, int64_t nChunks0, const int32_t *chunkRegion, const int32_t *chunkProblem,
                         int64_t nProblems, cpecan_band_edge *out);
/* Copies the compact buffer -- `total` triples, nothing else -- to hostOut. */
int cpk_device_fetch(CpkDevice *dev, int32_t *hostOut, int64_t total, double *d2hMs);

/* ---- consumers of the posterior lists, one descriptor per alignment problem ---- */
typedef struct {
    int64_t off[3];          /* first triple of the aligned / gapX / gapY list in the triple buffer */
    int32_t n[3];            /* their lengths */
    int32_t lX, lY;
    int32_t pad;
    int64_t seqOff;          /* first of lX + lY scratch slots (unaligned mass, cumulative gap mass) */
    int64_t chainOff;        /* first of n[0] + 1 chain-DP slots */
    int64_t charX, charY;    /* raw upper-case sequences (left shift) */
    int64_t meaOut;          /* first of n[0] output triples */
    int64_t shiftOut;        /* first of n[0] + min(lX, lY) + 1 output triples */
    int64_t nextOff;         /* first of 2 lX scratch words of the next-runs stage (y of every column, distance to the block's start) */
} CpkPostProblem;

#define CPK_POST_SCORES 5
typedef struct {
    int flags;               /* CPECAN_POST_* */
    double gapGamma;
    double matchGamma;       /* ORDERED: the float of cPecanRealign.c:355 widened to double */
    int64_t nProblems;
    const CpkPostProblem *problems;
    const uint8_t *chars;    /* host: raw upper-case sequences, or NULL (then no left shift, no identity scores) */
    int64_t nChars;
    int64_t seqSlots, chainSlots, meaCap, shiftCap; /* totals over the problems */
    /* outputs (host) */
    double *scores;          /* [nProblems][CPK_POST_SCORES]: byPosterior, byPosteriorIgnoringGaps, MEA alignment score,
                              * byIdentity, byIdentityIgnoringGaps (the last two only when chars are given) */
    int32_t *counts;         /* [nProblems][2]: MEA or ordered pairs, left-shifted pairs */
    int32_t *mea;            /* [meaCap*3] or NULL */
    int32_t *shift;          /* [shiftCap*3] or NULL */
    /* the quintuple stage (include/cpecan_sets.h), behind every consumer; names NULL: not selected, nothing of it is
     * allocated or launched */
    const int32_t *names;    /* host: [nProblems][2] */
    int32_t *quints;         /* host out: [meaCap*5], problem i at 5 * problems[i].meaOut */
    int64_t *sums;           /* host out: [nProblems] */
    double *stageMs;         /* host out, or NULL: HIP-event time of the stage's kernel */
    /* the next-runs stage (cpecan_batch_set_next_runs, include/cpecan_realign.h), behind ORDERED; nextRuns 0: not selected,
     * nothing of it is allocated or launched */
    int nextRuns;
    int32_t nextTrim, nextExpansion;
    int64_t nextSlots;       /* total of the problems' 2 lX scratch words */
    int32_t *runCounts;      /* host out: [nProblems] */
    int64_t *runOffsets;     /* host out: [nProblems + 1] prefix sums of runCounts */
    int32_t **runsOut;       /* host out: *runsOut is allocated by the stage (cpk_host_free), runOffsets[nProblems] quadruples */
    double *nextMs;          /* host out, or NULL: HIP-event time of the stage's two kernels and the copy between them */
} CpkPostJob;

/* Runs the job on the batch's compact result buffer (after cpk_device_gather, before cpk_device_fetch). */
int cpk_device_post(CpkDevice *dev, const CpkPostJob *job);
/* Runs the job on lists given by the host: `triples` (total*3 int32) is uploaded, processed and copied back. */
int cpk_post_lists(int device, int32_t *triples, int64_t total, const CpkPostJob *job);
int cpk_device_debug_fetch(CpkDevice *dev, double *fb, int64_t cells, double *totals, int64_t diags);
/* The table the device built for one region of the uploaded plan (rg: its entry as cpk_device_upload left it): waits for the
 * batch's own stream and copies the region's lX + lY + 1 entries, and its position words where the batch has them and
 * `dynamic` is 0 (*hasPos).  diags NULL: only *hasPos and *ringDoubles (what a split region's ring was given).  No launch. */
int cpk_device_table_fetch(CpkDevice *dev, const CpkRegion *rg, int dynamic, CpkDiag *diags, int32_t *dpos, int *hasPos,
                           int64_t *ringDoubles);
int64_t cpk_device_bytes(const CpkDevice *dev);
int cpk_device_waves(const CpkDevice *dev);
void cpk_set_error(const char *fmt, ...);
int cpk_host_threads(void); /* threads of the host's parallel loops (cpecan_host.c) */
/* Plans an unfrozen batch as cpecan_batch_upload would, without a device, and returns FNV-1a hashes of the plan: the
 * CpkRegion array in device order, devToHost, the CpkSegment slots, CpkGeometry with the output and debug totals.  For
 * tests: the plan is dropped again (cpecan_host.c). */
int cpk_batch_plan_digest(cpecan_batch *b, uint64_t out[4]);
/* For tests: what the add calls packed into a batch, as FNV-1a hashes; reads only.  out[0]: per problem firstRegion, nRegions,
 * lX, lY, charX, charY, minus; out[1]: per region every field an add call fills that does not depend on the form the anchors
 * are held in; out[2]: the symbols; out[3]: runForm, anchorStride and the anchor values, or every region's runOff and nRuns
 * and the run values; out[4]: the raw letters (cpecan_host.c). */
int cpk_batch_intake_digest(const cpecan_batch *b, uint64_t out[5]);
/* The overflow scan of a download, on arrays: counts [nLists][nRegions] and segCounts [nLists][nSegs] as the device left them
 * against the capacities of the device-order regions and their segments.  A split region's count per list becomes the sum of
 * its segments' counts, each clamped with the segment's capacity as it stood; capacities grow to what was needed and every
 * outOff follows.  Returns whether anything overflowed; *outTriples: the new total per list. */
int cpk_overflow_scan(CpkRegion *regions, int64_t nRegions, CpkSegment *segs, int64_t nSegs, int nLists, int32_t *counts,
                      const int32_t *segCounts, int64_t *outTriples);
/* After the download of a batch with cpecan_batch_set_quintuples: hands the three arrays of cpecan_batch_quintuples over to
 * the caller -- quints goes back with cpk_host_free, offsets and sums with free -- with the stage's kernel time; the batch
 * forgets them (cpecan_sets.c keeps them as its result). */
int cpk_batch_take_quintuples(cpecan_batch *b, int32_t **quints, int64_t **offsets, int64_t **sums, double *stageMs);
/* HIP-event time of the next-runs stage of the last download (cpecan_batch_set_next_runs): both kernels and the copy of
 * the counts between them. */
double cpk_batch_next_runs_ms(const cpecan_batch *b);
struct cpecan_realigner;
/* The same of the last cpecan_realigner_reanchor: the slowest shard's (cpecan_realign.c). */
double cpk_realigner_reanchor_ms(const struct cpecan_realigner *r);
struct cpecan_cigar;
/* The exact-match anchor runs of n cigars as every realign and expectations call makes them (cPecanRealign.c:511-529), on the
 * host: *nRuns n counts, *runs the quadruples one cigar after the other, both malloc'd (cpecan_realign.c). */
int cpk_realigner_cigar_runs(const struct cpecan_realigner *r, const struct cpecan_cigar *in, int64_t n, int64_t **runs,
                             int64_t **nRuns);
struct cpecan_viterbi;
/* A Viterbi object (cpecan_viterbi.h) over n cigars as cpecan_expect_set_create prepares them: the cigars' sub-sequences, their
 * exact-match anchor runs expanded into triples, the realigner's banding parameters and device, both ends ragged; one
 * problem per cigar, in order (cpecan_realign.c).  No device is touched. */
int cpk_realigner_viterbi_create(const struct cpecan_realigner *r, const cpecan_model *m, const struct cpecan_cigar *in, int64_t n,
                                 struct cpecan_viterbi **out);
/* The devices a call of the realigner is spread over (1 unless cpecan_realigner_set_devices listed more). */
int cpk_realigner_device_count(const struct cpecan_realigner *r);
/* Plans an unfrozen batch as cpecan_batch_upload would and then its launches (cpk_plan.inl, plan_batch) for a device of
 * numCUs compute units and memBytes of free memory that is not there: a kernel is taken to use the registers its build
 * allows.  out receives CPK_LAUNCH_PLAN_FIELDS numbers per launch class, in launch order (cpk_plan_describe); returns
 * the number of classes, or an error code (< 0).  For tests: the plan is dropped again.
 * The 23rd number counts the traceback SEGMENTS the class's queue hands out.  Without chains that is the length of the queue;
 * a chain item (below) counts as the segments it covers, so the number is the same with and without chains.  The length
 * of the queue itself is what cpk_batch_chain_plan returns in *nItems (and per class by counting its item records). */
#define CPK_LAUNCH_PLAN_FIELDS 25
int cpk_batch_launch_plan(cpecan_batch *b, int numCUs, int64_t memBytes, int64_t *out, int maxClasses);
int cpk_plan_describe(const CpkBatchPlan *plan, int numCUs, int64_t memBytes, int64_t *out, int maxClasses);
/* The chains of the same plan (cpk_plan.inl, plan_chains), beside cpk_batch_launch_plan, whose record keeps its layout:
 * chainsOut receives CPK_CHAIN_PLAN_FIELDS numbers per launch class, in launch order -- the first segment of the class's
 * chains (0: it has none) and their number.  itemsOut (may be null) receives the traceback queues built from the plan,
 * CPK_CHAIN_ITEM_FIELDS numbers per item in queue order -- class, device region, segment (-K: a chain from segment K), cost in
 * cells, segments of the region, leading segments of the region that the forward launch sweeps --, at most maxItems of them;
 * *nItems their number.  Returns the number of classes, or an
 * error code (< 0).  For tests: the plan is dropped again. */
#define CPK_CHAIN_PLAN_FIELDS 2
#define CPK_CHAIN_ITEM_FIELDS 6
int cpk_batch_chain_plan(cpecan_batch *b, int numCUs, int64_t memBytes, int64_t *chainsOut, int maxClasses, int64_t *itemsOut,
                         int64_t maxItems, int64_t *nItems);
int cpk_plan_chains(const CpkBatchPlan *plan, int numCUs, int64_t memBytes, int64_t *chainsOut, int maxClasses, int64_t *itemsOut,
                    int64_t maxItems, int64_t *nItems);
/* The plan an uploaded batch really got (valid after cpecan_batch_upload): the launch classes of its device, planned with
 * the registers and static LDS the loaded kernels report -- the same CPK_LAUNCH_PLAN_FIELDS numbers per class, in the same
 * order; returns the number of classes (0: a batch without regions), or an error code (< 0).  For tests.  The classes
 * are shown as they stand: after a download that re-ran a one-launch class in two launches (an item gave up waiting,
 * cpk_device_download) that class has the two-launch form, so reading the plan again behind the download tells whether
 * the one launch produced the results. */
int cpk_batch_launch_forms(cpecan_batch *b, int64_t *out, int maxClasses);
int cpk_device_launch_forms(const CpkDevice *dev, int64_t *out, int maxClasses);
/* The table of kernel variants that are built (cpk_kernel_table.inl) as data, CPK_KERNEL_FORM_FIELDS numbers per entry:
 * family, S, emit, mode, fast, wps, abs, inSweep, slots, dynamic, width, gang.  Returns the number of entries, or
 * CPECAN_EINVAL where maxEntries is too few.  No device needed.  cpk_kernel_table_chain: in step with it, one number per
 * entry -- 1 for a CHAIN build (KernelForm::chain), which the twelve fields do not tell from the gang it stands in for. */
#define CPK_KERNEL_FORM_FIELDS 12
int cpk_kernel_table_forms(int64_t *out, int maxEntries);
int cpk_kernel_table_chain(int64_t *out, int maxEntries);

/* ---- the anchor finder (cpk_anchor.inl; host side in cpecan_anchor.c) ---- */
/* One problem of an anchor pass: two substrings of the context's symbol buffer.  The host fills the first block, the
 * device layer sizes the lists (second block) and the kernels leave the counts (third block).
 * flags: CPK_ANCHOR_RC_Y -- the pass first writes the reverse complement of the lY symbols at yFwd (forward symbols of the
 * buffer) to yOff, which is even and lies in the area cpk_anchor_open reserved behind them; CPK_ANCHOR_SHARE_X -- the
 * minus twin of the problem in front of it in the list: same xOff and lX, and it reads that problem's sorted X keys
 * instead of making its own; CPK_ANCHOR_GAPPED -- the problem's chain is extended into its gaps (step 5b) with the
 * problem's yDrop and the CPK_ANCHOR_DIAGS(flags) anti-diagonals per extension that the flags hold above the bits.  The
 * three values of cpecan_anchor_options travel with the problem, not with CpkAnchorPass: tests/anchor_stages.py mirrors
 * that structure at its 160 bytes and hands buffers of that size to cpk_anchor_check and cpk_anchor_pass_plan. */
#define CPK_ANCHOR_RC_Y 1
#define CPK_ANCHOR_SHARE_X 2
#define CPK_ANCHOR_GAPPED 4
#define CPK_ANCHOR_DIAGS_SHIFT 8
#define CPK_ANCHOR_DIAGS(flags) ((flags) >> CPK_ANCHOR_DIAGS_SHIFT)
#define CPK_ANCHOR_GAPPED_BAND 31           /* cells with |i - j| <= 31: 63 matrix diagonals, one lane each */
#define CPK_ANCHOR_GAPPED_Y_DROP 9400       /* CPECAN_ANCHOR_GAP_OPEN + 300 * CPECAN_ANCHOR_GAP_EXTEND */
#define CPK_ANCHOR_GAPPED_MAX_DIAGS 4096
#define CPK_ANCHOR_GAPPED_MIN_DIAGS 64
typedef struct {
    int64_t xOff, yOff; /* first symbol of X / Y in the context's buffer */
    int32_t lX, lY;
    int32_t softMask;   /* windows with a lower-case base at a seed position are skipped */
    int32_t capX, capY; /* key slots: the window counts rounded up to a power of two */
    int32_t hspCap;     /* HSP slots, and hit-list slots with seedTransitions: the hit count rounded up to a power of two */
    int64_t keyXOff, keyYOff, hspOff;
    int32_t hits, hsps, chained, nRuns, capped, flags;
    int64_t columns;
    int64_t yFwd;  /* CPK_ANCHOR_RC_Y: first symbol of the forward Y */
    int32_t score; /* the chain score of step 4 (sum of the chained HSPs' scores; 0 without an HSP) */
    int32_t yDrop; /* CPK_ANCHOR_GAPPED: > 0; otherwise 0.  The host fills it */
} CpkAnchorProblem;

typedef struct {
    int32_t scores[25]; /* [a*5+b], symbols a c g t n */
    int32_t maxSeedOccurrences, xDrop, hspThreshold, maxHsps;
} CpkAnchorParams;

/* What a pass needs beside its problems; cpk_anchor_check (cpecan_anchor.c) builds it once per call. */
typedef struct {
    CpkAnchorParams prm;      /* handed to the kernels by value */
    char seed[32];            /* '0' / '1', terminated */
    int32_t seedTransitions;  /* 0, or 1 for hits that carry one transition (cpecan_anchor_params) */
    int32_t variantThreshold; /* what an HSP must score that only such hits extend to (cpecan_anchor_options);
                               * >= prm.hspThreshold, and equal to it for no threshold of its own */
    int32_t trim;
} CpkAnchorPass;

/* What cpk_anchor_pass_plan works out of a pass and its problem list without a device, and cpk_anchor_pass_size of the
 * hit counts that come back in the middle of the pass. */
typedef struct {
    struct {
        int32_t span, weight;
        uint8_t pos[16];
    } seed;                /* the layout of the kernels' CpkAnchorSeed (cpk_anchor.inl) */
    int32_t transitions;   /* the pass takes the transition path: join, hit lists, extend */
    int32_t maxCap, maxRc; /* most key slots of one sequence; longest reverse complement to write (0: none) */
    int32_t maxHits;       /* sizing: most hits of one problem, at least 1 */
    int64_t hitsPerWindow; /* most hits a Y window can have */
    int64_t nKeys;         /* key slots of the pass */
    int64_t nSlots;        /* sizing: HSP slots of the pass */
    int64_t nCounters;     /* sizing: per problem the HSPs handed out and, on the transition path, the hits written */
} CpkAnchorPlan;

typedef struct CpkAnchorCtx CpkAnchorCtx;
/* Copies the nBytes raw sequence bytes to `device` and packs them into symbols there; behind them (from the next even
 * symbol index on) the buffer has room for nExtra symbols more, for the reverse complements of a pass. */
int cpk_anchor_open(CpkAnchorCtx **out, int device, const uint8_t *bytes, int64_t nBytes, int64_t nExtra);
/* The host half of a pass; touches no device.  Parses the seed, checks the pass and the contract of the problem list
 * against a buffer of nSym symbols of which the first nForward are the packed bytes (CPECAN_EINVAL), and fills capX, capY,
 * keyXOff, keyYOff and zeroed counters into every problem. */
int cpk_anchor_pass_plan(const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int64_t nSym, int64_t nForward,
                         CpkAnchorPlan *plan);
/* The second sizing step: hspCap and hspOff of every problem from its hit count. */
void cpk_anchor_pass_size(CpkAnchorProblem *probs, int64_t n, CpkAnchorPlan *plan);
/* The sizing step of a pass that extends chains (step 5b), after the chains came back: nRows -- the 64-byte scratch rows of
 * all extensions, one per anti-diagonal; nRuns -- the run triples the assembly may write; maxGaps -- most gaps of one
 * problem.  cpk_anchor_gapped_size also fills where every problem's rows and runs start (n + 1 values each, the last the
 * total); touches no device.  A pass whose rows pass CPK_ANCHOR_GAPPED_BUDGET_ROWS runs its gaps in several launches,
 * each ending at the gap boundary cpk_anchor_gapped_slice_end picks. */
typedef struct {
    int64_t nRows, nRuns;
    int32_t maxGaps, pad;
} CpkAnchorGappedPlan;
#define CPK_ANCHOR_GAPPED_BUDGET_ROWS ((int64_t)4 << 20) /* 256 MiB of scratch */
void cpk_anchor_gapped_size(const CpkAnchorProblem *probs, int64_t n, int64_t *rowBase, int64_t *runBase, CpkAnchorGappedPlan *plan);
int64_t cpk_anchor_gapped_slice_end(const int64_t *bounds, int64_t nBounds, int64_t lo, int64_t budgetRows);
/* Steps 1-5 of the anchor finder on n problems of the context's buffer.  *runs receives a malloc'd array of triples
 * (x, y, length) relative to each problem (NULL for n == 0); problem i owns triples hspOff .. hspOff + nRuns - 1, and
 * nothing else is promised about where a problem's triples lie: a pass that extends chains (CPK_ANCHOR_GAPPED) moves
 * hspOff, because a problem can then have more runs than HSP slots.  *ms: kernel time added. */
int cpk_anchor_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int32_t **runs, double *ms);
void cpk_anchor_close(CpkAnchorCtx *c);

/* ---- the stages of a call (cpecan_anchor.c); none of them touches a device ---- */
/* What a call carries beside the pass: the entry point's arguments and outputs. */
typedef struct {
    const char *who; /* the entry point, for the error texts */
    const cpecan_anchor_problem *problems;
    int64_t n;
    int64_t expansion, anchorMatrixBiggerThanThis, repeatMaskMatrixBiggerThanThis;
    int32_t device, strandMode;
    int32_t once;        /* steps 1-5 alone on every problem whatever its size, no recursion (cpecan_find_anchor_runs_once) */
    int32_t softMaskTop; /* soft masking of the top level; only `once` asks for 0 (:1168) */
    int64_t **runs;
    int64_t *nRuns;
    cpecan_anchor_stats *stats;    /* or NULL */
    cpecan_strand_result *strands; /* or NULL */
} CpkAnchorCall;

/* The problems of one pass.  owner: the caller's problem (top level) or the index in the top-level list (gaps); before:
 * the top-level run a gap stands in front of, nRuns for the gap behind the last. */
typedef struct {
    CpkAnchorProblem *probs;
    int64_t *owner, *before;
    int64_t n, cap;
} CpkAnchorList;
void cpk_anchor_list_free(CpkAnchorList *l);

/* Check: arguments, params (NULL: the defaults) and options (or NULL) into *pass; outputs zeroed, strands at their defaults. */
int cpk_anchor_check(const CpkAnchorCall *c, int64_t trim, const cpecan_anchor_params *params,
                     const cpecan_anchor_options *options, CpkAnchorPass *pass);
/* Layout: the top-level list, twins included, and the malloc'd buffer of its sequences (NULL for an empty list). */
int cpk_anchor_layout(const CpkAnchorCall *c, CpkAnchorList *top, uint8_t **bytes, int64_t *nBytes, int64_t *nExtra);
/* Strand pick, after the top-level pass: scores into c->strands, the list compacted to what goes on. */
void cpk_anchor_pick(const CpkAnchorCall *c, CpkAnchorList *top);
/* Gaps: the rectangles between the top-level runs that are still too large become the list of the second pass. */
int cpk_anchor_gaps(const CpkAnchorCall *c, const CpkAnchorList *top, const int32_t *topRuns, CpkAnchorList *sub);
/* Splice: both run lists into c->runs, c->nRuns and c->stats. */
int cpk_anchor_splice(const CpkAnchorCall *c, const CpkAnchorList *top, const int32_t *topRuns, const CpkAnchorList *sub,
                      const int32_t *subRuns, double kernelMs);

/* ---- local chains (cpk_local.inl; host side in cpecan_local.c) ---- */
#define CPK_LOCAL_MAX_CHAINS 16
/* One caller problem of a local pass: the one problem of the pass list it stands for, or its pair of orientation twins
 * (`first`, then the CPK_ANCHOR_SHARE_X twin).  The kernel leaves the counts. */
typedef struct {
    int64_t first;
    int32_t twins;   /* 1 or 2 */
    int32_t nChains; /* chains recorded, at most maxChains */
    int32_t nRuns;   /* runs of all of them */
    int32_t rounds;  /* rounds that found a chain: nChains, or one more for the chain under minChainScore that ended them */
} CpkLocalProblem;
/* One chain as the kernel records it: the rectangle and the runs in the coordinates of its orientation, relative to the
 * problem; runOff counts triples from the problem's first. */
typedef struct {
    int32_t strand, score, nHsps, runOff, nRuns;
    int32_t x0, x1, y0, y1, pad;
} CpkLocalChain;
typedef struct {
    int32_t maxChains, minChainScore; /* minChainScore as the kernel compares it: never 0 for "the threshold" */
} CpkLocalPass;
/* Steps 0-3 of cpk_anchor_pass on the n problems, then the rounds of step 7 per caller problem.  *chains: malloc'd,
 * maxChains records per caller problem, of which the first nChains hold; *runs: malloc'd triples, those of caller problem k
 * from 3 * probs[lprobs[k].first].hspOff on.  Both NULL for n == 0.  probs gets hits, hsps and capped; *ms: kernel time added.
 * Problems that carry CPK_ANCHOR_GAPPED (all of the pass or none; yDrop and the diagonals as for an anchor pass) have their
 * chains extended behind the peel (step 7b): the records then hold the extended rectangle and runs, a chain may have more
 * runs than HSPs, and hspOff of a problem's first twin has moved to a run list of its own. */
int cpk_local_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, const CpkLocalPass *lp, CpkAnchorProblem *probs, int64_t n,
                   CpkLocalProblem *lprobs, int64_t nLocal, CpkLocalChain **chains, int32_t **runs, double *ms);

/* The stages of cpecan_find_local_chains_many (cpecan_local.c); none of them touches a device. */
struct cpecan_local_options;
struct cpecan_local_chain;
struct cpecan_local_stats;
typedef struct {
    const char *who;
    const cpecan_anchor_problem *problems;
    int64_t n, expansion;
    int32_t device, strandMode;
    struct cpecan_local_chain **chains;
    int64_t *nChains;
    int64_t **runs;
    int64_t *nRuns;
    struct cpecan_local_stats *stats; /* or NULL */
} CpkLocalCall;
/* Check: arguments, params (NULL: the defaults), both option records (either NULL: its defaults) into *pass and *lp;
 * outputs zeroed. */
int cpk_local_check(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params, const cpecan_anchor_options *anchorOptions,
                    const struct cpecan_local_options *localOptions, CpkAnchorPass *pass, CpkLocalPass *lp);
/* The same with anchorOptions->gappedExtension = 1 admitted (cpecan_find_local_chains_many_gapped), and what carries the
 * three gapped options of a checked call into the list of its layout: CPK_ANCHOR_GAPPED, the diagonals and yDrop of every
 * problem, as an anchor pass takes them. */
int cpk_local_check_gapped(const CpkLocalCall *c, int64_t trim, const cpecan_anchor_params *params,
                           const cpecan_anchor_options *anchorOptions, const struct cpecan_local_options *localOptions,
                           CpkAnchorPass *pass, CpkLocalPass *lp);
void cpk_local_mark_gapped(CpkAnchorList *top, const cpecan_anchor_options *anchorOptions);
/* Layout: cpk_anchor_layout's list with the whole of every non-empty pair in it, soft-masked, twins for BOTH; and the
 * malloc'd record per caller problem that is in the list (*lprobs, *nLocal). */
int cpk_local_layout(const CpkLocalCall *c, CpkAnchorList *top, uint8_t **bytes, int64_t *nBytes, int64_t *nExtra,
                     CpkLocalProblem **lprobs, int64_t *nLocal);
/* Assemble: what a pass left becomes the caller's arrays and statistics. */
int cpk_local_assemble(const CpkLocalCall *c, const CpkAnchorList *top, const CpkLocalProblem *lprobs, int64_t nLocal,
                       const CpkLocalChain *chains, const int32_t *runs, int32_t maxChains, double kernelMs);

/* ---- dense forward / backward rows (cpk_dense.inl; host side in cpecan_dense.c) ---- */
/* One anti-diagonal of a dense problem: its band and the band cells on the problem's earlier diagonals. */
typedef struct {
    int32_t xmyL, width;
    int64_t cellOff;
} CpkDenseDiag;
/* One problem = one region (the dense path never splits). */
typedef struct {
    int64_t symX, symY; /* first byte of the padded symbol strings (symbol[0] = N, symbol[i] = base i - 1, symbol[l + 1] = N) */
    int64_t diagOff;    /* first of the problem's lX + lY + 1 CpkDenseDiag, and of its totalUsed entries */
    int64_t cellBase;   /* first cell of the problem in F and B */
    int32_t lX, lY;
    int32_t raggedLeft, raggedRight;
} CpkDenseProblem;
/* One traceback (pairwiseAligner.c:791-862) of a problem: the work item of the backward kernel.  The backward rows of
 * diagonals tbFrom + 1 .. dTop, which the traceback computes and does not emit, go to `side`: the first of them is Bnext. */
typedef struct {
    int32_t tbPrev, dTop, tbFrom, problem;
    int64_t sideBase; /* first cell of the traceback's rows in the side array */
} CpkDenseSeg;
/* All problems of a cpecan_dense object in one launch sequence: the forward kernel over the problems, then the backward
 * kernel over the tracebacks.  F and B: totalCells * S doubles; side: sideCells * S; totals: nDiags.  Host arrays in, host
 * arrays out; *kernelMs (or NULL): HIP-event time of the two kernels. */
typedef struct {
    const CpkDenseProblem *problems;
    const CpkDenseDiag *diags;
    const CpkDenseSeg *segs;
    const uint8_t *symbols;
    int64_t nProblems, nDiags, nSegs, nSymbolBytes, totalCells, sideCells;
    double *F, *B, *side, *totals;
} CpkDenseJob;
int64_t cpk_dense_device_bytes(const CpkDenseJob *job, int nStates);
int cpk_dense_run(int device, const CpkModel *model, const CpkDenseJob *job, double *kernelMs);
/* cpecan_host.c: the kernels' view of a model, and the symbol of a sequence byte */
void cpk_kernel_model(const cpecan_model *m, double threshold, CpkModel *k);
uint8_t cpk_symbol_of(unsigned char c);

/* ---- Viterbi decoding (cpk_viterbi.inl; host side in cpecan_viterbi.c) ---- */
#define CPK_VIT_BLOCK_DIAGS 64   /* diagonals whose pointer bytes the traceback stages in LDS at a time */
#define CPK_VIT_LDS_MAX_WIDTH 256 /* CPECAN_VITERBI_LDS_MAX_WIDTH */
/* One anti-diagonal of a region: its band and the band cells on the region's earlier diagonals. */
typedef struct {
    int32_t xmyL, width;
    int64_t cellOff;
} CpkVitDiag;
/* One region of a launch.  All offsets are into the launch's own arrays. */
typedef struct {
    int64_t symX, symY; /* first byte of the padded symbol strings (symbol[0] = N, symbol[i] = base i - 1, symbol[l + 1] = N) */
    int64_t diagOff;    /* first of the region's lX + lY + 1 CpkVitDiag */
    int64_t ptrBase;    /* first of its pointer bytes, one per band cell */
    int64_t rollBase;   /* first double of its three global rolling rows (3 * S * maxWidth) */
    int64_t opBase;     /* first (state, length) pair of its ops: room for lX + lY pairs, written last run first */
    int32_t lX, lY;
    int32_t raggedLeft, raggedRight;
    int32_t maxWidth, pad;
} CpkVitRegion;
/* What the kernels leave per region. */
typedef struct {
    double logP;
    int32_t startState, endState, nOps, pad;
} CpkVitOut;
/* The regions of one launch: the sweep over `order[0 .. nLds)` with the rows in LDS and over `order[nLds .. nRegions)` with
 * the rows in global memory, then the traceback over all.  Host arrays in, host arrays out (out: nRegions; ops: 2 * nOpPairs). */
typedef struct {
    const CpkVitRegion *regions;
    const CpkVitDiag *diags;
    const uint8_t *symbols;
    const int32_t *order;
    int64_t nRegions, nLds, nDiags, nSymbolBytes, nPtrBytes, nRollDoubles, nOpPairs;
    int32_t ldsMaxWidth; /* widest diagonal among the LDS-form regions */
    CpkVitOut *out;
    int32_t *ops;
} CpkVitJob;
int cpk_viterbi_launch(int device, const CpkModel *model, const CpkVitJob *job, double *sweepMs, double *tracebackMs);

/* The resident form (cpecan_viterbi_run_counts): the inputs of every launch of a planned run uploaded
 * once, one scratch (pointer bytes, rolling rows, out records, op slots, count slabs) at the largest launch's size, the run's
 * int64 bins.  The ops never leave the device. */
#define CPK_VIT_MAX_BINS (25 + 80) /* S * S transitions, then S * 16 emissions */
typedef struct CpkVitResident CpkVitResident;
/* inputBytes / scratchBytes: what the uploads and the scratch will take; CPECAN_ENOMEM, with the bytes named, where the
 * device has not that much free. */
int cpk_viterbi_resident_create(CpkVitResident **out, int device, int nStates, int64_t nLaunches, int64_t inputBytes, int64_t scratchBytes);
/* Copies the job's regions, diags, symbols and order to the device as launch `launch`; its out / ops pointers are not read. */
int cpk_viterbi_resident_upload(CpkVitResident *r, int64_t launch, const CpkVitJob *job);
/* After the last upload: the scratch. */
int cpk_viterbi_resident_reserve(CpkVitResident *r);
/* Zeroes the run's bins. */
int cpk_viterbi_resident_begin(CpkVitResident *r);
/* Sweep, traceback, count, reduce of one launch; out: its nRegions records; slabs (or NULL): its nRegions * nBins uint32;
 * ms[4]: HIP-event times of sweep, traceback, count, reduce. */
int cpk_viterbi_resident_run(CpkVitResident *r, int64_t launch, const CpkModel *model, CpkVitOut *out, uint32_t *slabs, double ms[4]);
/* bins[nBins] of the launches since cpk_viterbi_resident_begin. */
int cpk_viterbi_resident_bins(CpkVitResident *r, int64_t *bins);
void cpk_viterbi_resident_destroy(CpkVitResident *r);

#ifdef __cplusplus
}
#endif
#endif
