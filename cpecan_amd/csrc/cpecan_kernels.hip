/*
 * cpecan_kernels.hip -- hand-written gfx950 (MI355X / CDNA4) kernels for cPecan's banded pair-HMM
 * forward / backward / posterior path, plus the device-memory plumbing behind them.  One translation unit; the
 * device code is split over the cpk_*.inl files included below, the host side (memory, launches, timing) is here.
 *
 * What the reference does per alignment (impl/pairwiseAligner.c:756-877, getPosteriorProbsWithBanding):
 * a forward sweep over anti-diagonals with periodic partial tracebacks; each traceback runs the
 * backward recurrence from an end-state prior, refreshes the total probability every 10th diagonal
 * and emits thresholded posteriors.  The arithmetic is log-space fp64 with a piecewise-cubic logAdd
 * (:287-307) whose fold ORDER is part of the result, so the kernels reproduce it term for term.
 *
 * How it is mapped to CDNA4 (DESIGN.md sections 3-5):
 *   - sweep kernel (cpk_sweep.inl): one 64-lane wavefront per DP region, persistent, work-queue fed; lanes <-> cells
 *     of the current anti-diagonal; the previous diagonals live in LDS, position-major, with a -inf guard position so
 *     band edges need no branches; the backward recurrence is a GATHER in the reference's scatter order; forward
 *     values stream to a per-wave ring in HBM holding one traceback segment; the sequential logAdd fold of the
 *     per-diagonal total is transposed (one lane per refresh point); posteriors are thresholded and compacted with
 *     wave ballots straight into the output list order;
 *   - packed kernel (cpk_packed.inl): narrow bands, 64/GW regions per wave, the same cell functions;
 *   - team kernel (cpk_team.inl): bands of several hundred cells, four or eight waves of a workgroup per region, one
 *     barrier per diagonal, the same cell functions;
 *   - every launch of a run is one size class of regions (narrow 8/16/32, wide 128 ... LDS-sized, global) with LDS,
 *     occupancy and scratch for its own largest region (LaunchClass below);
 *   - cpk_table_gather.inl: the per-diagonal band table from the anchors, the lists' re-ordering;
 *   - cpk_post.inl: reweighting, posterior and identity scores, ordered chain, MEA chain, left shift on the device.
 * No MFMA: an fp64 stencil bounded by vector-instruction issue (HBM traffic is ~1/3 of the algorithmic figure).
 *
 * Built with -ffp-contract=off; the logAdd cubic's three FMAs are explicit (cpk_device_common.inl: what the shipped
 * build changes against the reference's operation sequence, and the EXACT=1 diagnostic build that does not).
 */
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <algorithm>
#include <atomic>
#include <utility>
#include <thread>
#include <type_traits>
#include <vector>

#include "cpecan_internal.h"
#include "cpecan_band.inl"

#define NEG_INF (-__builtin_huge_val())

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

extern "C" void cpk_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char *cpk_last_error(void) { return g_err; }

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            cpk_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return CPECAN_EHIP;                                                                     \
        }                                                                                           \
    } while (0)

#include "cpk_device_common.inl"
#include "cpk_sweep.inl"
#include "cpk_team.inl"
#include "cpk_table_gather.inl"
#include "cpk_packed.inl"
#include "cpk_post.inl"
#include "cpk_cells.inl"
#include "cpk_anchor.inl"
#include "cpk_local.inl"
#include "cpk_dense.inl"
#include "cpk_viterbi.inl"

// ------------------------------------------------------------------------------------------------
// host side of the HIP TU: memory, launch, timing
// ------------------------------------------------------------------------------------------------
#include "cpk_kernel_table.inl"
#include "cpk_plan.inl"

// ------------------------------------------------------------------------------------------------
// Device memory and device shells are recycled: a batch of one small problem (the single-call entry points, a caller's
// loop over alignments) would otherwise spend ~40 ms in hipMalloc / hipFree / stream creation around a 1 ms kernel, and
// a pipeline of large batches cannot afford hipFree at all: it waits for the whole device, i.e. for the other batch's
// sweep kernel.  Freed blocks up to a bounded total (CPECAN_CACHE_MB, default HALF of the device's memory) wait in a
// per-device list and serve later requests of about their size; what the list will not hold goes back to the driver, and
// all of it does when an allocation fails, on cpecan_cache_trim(), or after the device has had no live batch for
// CPECAN_CACHE_IDLE_S seconds (the idle reaper below).  A block is recycled only after its batch's own streams and
// events have completed.
// ------------------------------------------------------------------------------------------------
namespace {
struct CachedBlock {
    void *ptr;
    size_t bytes;
};
struct BlockCache {
    std::vector<CachedBlock> blocks;
    size_t bytes = 0;
};
constexpr int kMaxDevices = 64;
constexpr size_t kCacheMaxBlock = (size_t)256 << 30;  // the rings of a batch's split regions are ONE block (60 GB at config B)
constexpr int kCacheMaxBlocks = 512;
// What the idle blocks of one device may hold: CPECAN_CACHE_MB, default HALF of the device's memory (the process may
// share the GPU with torch / RCCL allocations that cannot reclaim what this library hoards; cpecan_cache_trim gives
// everything back on request, and a device without live batches drops its large blocks after an idle time, below).
// The current device is `device`.
size_t cache_max_bytes(int device) {
    static const double envMb = [] {
        const char *mb = getenv("CPECAN_CACHE_MB");
        return mb ? atof(mb) : -1.0;
    }();
    if (envMb >= 0.0) return (size_t)(envMb * 1048576.0);
    static std::atomic<size_t> half[kMaxDevices];
    if (device < 0 || device >= kMaxDevices) return (size_t)16 << 30;
    size_t v = half[device].load(std::memory_order_relaxed);
    if (v == 0) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) {
            (void)hipGetLastError();
            totalB = (size_t)32 << 30;
        }
        v = totalB / 2 + 1;
        half[device].store(v, std::memory_order_relaxed);
    }
    return v;
}
// Idle blocks above this size go back to the driver once a device has had no live batch for cache_idle_seconds()
// (CPECAN_CACHE_KEEP_MB, default 256; negative: keep everything, as rounds 1-2 did).  Round 3 dropped them the moment
// the last live batch of a device was destroyed: a caller that runs one big batch at a time then paid hipFree +
// hipMalloc of its rings around every batch -- ~0.08 s per GB, seconds at config B (VERDICT r3 "post-trim stall").
double cache_keep_mb() {
    static const double v = [] {
        const char *mb = getenv("CPECAN_CACHE_KEEP_MB");
        return mb ? atof(mb) : 256.0;
    }();
    return v;
}
// seconds without a live batch after which a device's large idle blocks are given back (CPECAN_CACHE_IDLE_S, default
// 20; 0: at once, as round 3 did; negative: never -- only cpecan_cache_trim and failed allocations do)
double cache_idle_seconds() {
    static const double v = [] {
        const char *s = getenv("CPECAN_CACHE_IDLE_S");
        return s ? atof(s) : 20.0;
    }();
    return v;
}
std::mutex g_cacheMutex;
BlockCache g_blockCache[kMaxDevices];
std::atomic<int> g_liveShells[kMaxDevices];  // batches (device shells) created and not destroyed yet, per device
// batches of this process that have run on a device and are not destroyed yet: the consumers of such a batch (list
// gather, reweight, MEA, ...) may still have to run beside the sweep of the batch that is being planned
static std::atomic<int> g_ranAlive[kMaxDevices];

// CPECAN_TRACE_HOST=1: every hipMalloc / hipFree of 64 MB or more with its wall time, on stderr (diagnostic)
bool trace_alloc() {
    static const bool on = getenv("CPECAN_TRACE_HOST") != nullptr;
    return on;
}
hipError_t traced_malloc(void **out, size_t bytes) {
    if (!trace_alloc() || bytes < ((size_t)64 << 20)) return hipMalloc(out, bytes);
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(out, bytes);
    fprintf(stderr, "[cpecan] hipMalloc %.1f MB: %.3f ms%s\n", bytes / 1048576.0,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), e == hipSuccess ? "" : " FAILED");
    return e;
}
void traced_free(void *ptr, size_t bytes) {
    if (!trace_alloc() || bytes < ((size_t)64 << 20)) {
        (void)hipFree(ptr);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    (void)hipFree(ptr);
    fprintf(stderr, "[cpecan] hipFree %.1f MB: %.3f ms\n", bytes / 1048576.0,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

size_t round_alloc(size_t bytes) {  // coarser sizes make blocks fit later requests
    const size_t g = bytes <= (64u << 10) ? 4096 : (bytes <= (16u << 20) ? (64u << 10) : (1u << 20));
    return (bytes + g - 1) / g * g;
}

// the current device is `device`
hipError_t cache_alloc(int device, void **out, size_t bytes) {
    bytes = round_alloc(bytes ? bytes : 1);
    if (device >= 0 && device < kMaxDevices) {
        std::lock_guard<std::mutex> lock(g_cacheMutex);
        BlockCache &c = g_blockCache[device];
        int best = -1;
        for (int i = 0; i < (int)c.blocks.size(); i++)
            if (c.blocks[i].bytes >= bytes && c.blocks[i].bytes <= 2 * bytes + (1u << 20) &&
                (best < 0 || c.blocks[i].bytes < c.blocks[best].bytes))
                best = i;
        if (best >= 0) {
            *out = c.blocks[best].ptr;
            c.bytes -= c.blocks[best].bytes;
            c.blocks[best] = c.blocks.back();
            c.blocks.pop_back();
            return hipSuccess;
        }
    }
    hipError_t e = traced_malloc(out, bytes);
    if (e != hipSuccess && device >= 0 && device < kMaxDevices) {  // give the cached blocks back and try once more
        std::vector<CachedBlock> drop;
        {
            std::lock_guard<std::mutex> lock(g_cacheMutex);
            drop.swap(g_blockCache[device].blocks);
            g_blockCache[device].bytes = 0;
        }
        for (const CachedBlock &b : drop) traced_free(b.ptr, b.bytes);
        (void)hipGetLastError();
        e = traced_malloc(out, bytes);
    }
    return e;
}

// the device must be idle with respect to this block (callers synchronise first)
size_t cache_bytes(int device) {
    if (device < 0 || device >= kMaxDevices) return 0;
    std::lock_guard<std::mutex> lock(g_cacheMutex);
    return g_blockCache[device].bytes;
}

void cache_free(int device, void *ptr, size_t bytes) {
    if (!ptr) return;
    bytes = round_alloc(bytes ? bytes : 1);
    if (device >= 0 && device < kMaxDevices && bytes <= kCacheMaxBlock) {
        std::lock_guard<std::mutex> lock(g_cacheMutex);
        BlockCache &c = g_blockCache[device];
        if (c.bytes + bytes <= cache_max_bytes(device) && (int)c.blocks.size() < kCacheMaxBlocks) {
            c.blocks.push_back({ptr, bytes});
            c.bytes += bytes;
            return;
        }
    }
    traced_free(ptr, bytes);
}

// Gives the idle blocks of `device` that are larger than keepBelow bytes back to the driver (hipFree waits for the
// device).  The current device is `device`.  Returns the bytes freed.
size_t cache_trim(int device, size_t keepBelow) {
    if (device < 0 || device >= kMaxDevices) return 0;
    std::vector<CachedBlock> drop;
    {
        std::lock_guard<std::mutex> lock(g_cacheMutex);
        BlockCache &c = g_blockCache[device];
        for (size_t i = 0; i < c.blocks.size();) {
            if (c.blocks[i].bytes > keepBelow) {
                drop.push_back(c.blocks[i]);
                c.bytes -= c.blocks[i].bytes;
                c.blocks[i] = c.blocks.back();
                c.blocks.pop_back();
            } else {
                i++;
            }
        }
    }
    size_t freed = 0;
    for (const CachedBlock &b : drop) {
        traced_free(b.ptr, b.bytes);
        freed += b.bytes;
    }
    return freed;
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// Host blocks.  The large host arrays of a batch (symbols, anchors, region and segment tables, the result triples)
// come from here: pinned memory when a HIP device is present, recycled like the device blocks.  A realignment batch
// (BASELINE config 4: 50 000 alignments, 60 M anchors, 74 M result triples) holds ~2 GB of them; from malloc every batch
// paid ~90 ms of first-touch page faults while filling them, ~200 ms of munmap in cpecan_batch_destroy, a staging copy
// on the way up and a pageable (pin-as-you-go) copy on the way down (profiles/r02_e2e_stages_config4_before.txt).
// A block is pinned (hipHostRegister) when it is REUSED, not when it is first allocated: pinning costs ~0.2 ms per MB,
// twice the first-touch faults it replaces, and a process that runs one batch and exits (the cpecan_realign command
// line on one file) would only pay for it -- its copies go the pageable way, as before.  From its second life on a
// block is read and written by the copy engines in place.
// Blocks below 256 KB are plain malloc.  CPECAN_HOST_CACHE_MB bounds what idle blocks may hold (default 16 GiB);
// CPECAN_PINNED=0 keeps everything pageable.
// ------------------------------------------------------------------------------------------------
namespace {
struct HostBlock {
    void *ptr;
    size_t bytes;
    bool pinned;
    bool registered;  // pinned by hipHostRegister (memory of posix_memalign) rather than allocated by hipHostMalloc
};
constexpr size_t kHostPoolMin = (size_t)256 << 10;
std::mutex g_hostMutex;
std::vector<HostBlock> g_hostLive, g_hostIdle;
size_t g_hostIdleBytes = 0;
size_t host_cache_max_bytes() {
    static const size_t v = [] {
        const char *mb = getenv("CPECAN_HOST_CACHE_MB");
        return mb ? (size_t)(atof(mb) * 1048576.0) : ((size_t)16 << 30);
    }();
    return v;
}
bool host_pinning_enabled() {
    static const bool v = [] {
        const char *e = getenv("CPECAN_PINNED");
        if (e && atoi(e) == 0) return false;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return n > 0;
    }();
    return v;
}
// Blocks that are not hipHostMalloc'ed are anonymous mappings of whole pages: page-aligned for hipHostRegister, and
// mremap grows them without a copy.
void *host_map(size_t bytes) {
    void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    return p == MAP_FAILED ? nullptr : p;
}
void host_release(const HostBlock &b) {
    if (b.pinned && !b.registered) {
        (void)hipHostFree(b.ptr);
        return;
    }
    if (b.registered) (void)hipHostUnregister(b.ptr);
    (void)munmap(b.ptr, b.bytes);
}
}  // namespace

// mustPin: the block will be written by kernels (it has to be device-visible whatever CPECAN_PINNED says)
static void *host_alloc_impl(size_t bytes, bool mustPin) {
    if (bytes < kHostPoolMin && !mustPin) return malloc(bytes ? bytes : 1);
    bytes = (bytes + ((size_t)2 << 20) - 1) / ((size_t)2 << 20) * ((size_t)2 << 20);
    {
        std::unique_lock<std::mutex> lock(g_hostMutex);
        int best = -1;
        // a block serves requests of its own size and up to a quarter less (round 4; rounds 1-3: down to half).  The wide
        // window let the arrays of a batch trade places -- a 480 MB anchor request took the idle 890 MB result block of
        // another batch, whose next result request then found nothing and mapped a fresh, unpinned block -- so a pipeline
        // of BASELINE config-4 batches kept meeting blocks in their first life (a pageable 890 MB copy: 200 ms) and their
        // second (pinning: 180 ms) long after its first batches.
        for (int i = 0; i < (int)g_hostIdle.size(); i++)
            if (g_hostIdle[i].bytes >= bytes && g_hostIdle[i].bytes <= bytes + bytes / 4 + ((size_t)8 << 20) &&
                // kernels store through the HOST pointer of a mustPin block: only hipHostMalloc'ed memory is guaranteed to
                // map at the same device address; a range pinned later by hipHostRegister is not (no hipHostGetDevicePointer
                // is ever asked for), so such blocks never serve a mustPin request
                ((g_hostIdle[i].pinned && !g_hostIdle[i].registered) || !mustPin) &&
                (best < 0 || g_hostIdle[i].bytes < g_hostIdle[best].bytes))
                best = i;
        if (best >= 0) {
            HostBlock b = g_hostIdle[best];
            g_hostIdle[best] = g_hostIdle.back();
            g_hostIdle.pop_back();
            g_hostIdleBytes -= b.bytes;
            if (!b.pinned && host_pinning_enabled()) {  // a second life: worth pinning now (its pages are resident)
                // (outside the lock: 0.2 ms per MB, and the other threads of a pipeline -- the batches' download helpers,
                // the caller packing the next batch -- allocate and free all the time; the block is in neither list meanwhile)
                lock.unlock();
                const auto t0 = std::chrono::steady_clock::now();
                const hipError_t e = hipHostRegister(b.ptr, b.bytes, hipHostRegisterPortable);
                if (e == hipSuccess) b.pinned = b.registered = true;
                else (void)hipGetLastError();
                if (trace_alloc() && b.bytes >= ((size_t)64 << 20))
                    fprintf(stderr, "[cpecan] hipHostRegister %.1f MB: %.3f ms%s\n", b.bytes / 1048576.0,
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                            e == hipSuccess ? "" : " FAILED");
                lock.lock();
            }
            g_hostLive.push_back(b);
            return b.ptr;
        }
    }
    HostBlock b{nullptr, bytes, false, false};
    if (mustPin) {
        if (hipHostMalloc(&b.ptr, bytes, hipHostMallocPortable) == hipSuccess) b.pinned = true;
        else {
            (void)hipGetLastError();
            b.ptr = nullptr;
        }
    }
    if (!b.ptr && (mustPin || (b.ptr = host_map(bytes)) == nullptr)) return nullptr;
    if (trace_alloc() && bytes >= ((size_t)64 << 20)) fprintf(stderr, "[cpecan] new host block %.1f MB%s\n", bytes / 1048576.0, mustPin ? " (pinned)" : "");
    std::lock_guard<std::mutex> lock(g_hostMutex);
    g_hostLive.push_back(b);
    return b.ptr;
}
extern "C" void *cpk_host_alloc(size_t bytes) { return host_alloc_impl(bytes, false); }

extern "C" void cpk_host_free(void *p) {
    if (!p) return;
    HostBlock b{nullptr, 0, false, false};
    {
        std::lock_guard<std::mutex> lock(g_hostMutex);
        for (size_t i = 0; i < g_hostLive.size(); i++)
            if (g_hostLive[i].ptr == p) {
                b = g_hostLive[i];
                g_hostLive[i] = g_hostLive.back();
                g_hostLive.pop_back();
                break;
            }
        if (b.ptr && g_hostIdleBytes + b.bytes <= host_cache_max_bytes() && g_hostIdle.size() < 256) {
            g_hostIdle.push_back(b);
            g_hostIdleBytes += b.bytes;
            return;
        }
    }
    if (b.ptr) host_release(b);
    else free(p);  // a small block
}

// Releases every idle host block (pinned ones included).  Returns the bytes released.
static size_t host_trim(void) {
    std::vector<HostBlock> drop;
    {
        std::lock_guard<std::mutex> lock(g_hostMutex);
        drop.swap(g_hostIdle);
        g_hostIdleBytes = 0;
    }
    size_t freed = 0;
    for (const HostBlock &b : drop) {
        host_release(b);
        freed += b.bytes;
    }
    return freed;
}

// Grows a block to newBytes keeping its first usedBytes.  A block that is not pinned grows in place where the C library
// can do that (realloc: mremap for large blocks, no copy and no new page faults for the part that exists) -- a batch that
// is filled a slice at a time grows its arrays a dozen times.
extern "C" void *cpk_host_grow(void *p, size_t usedBytes, size_t newBytes) {
    if (!p) return cpk_host_alloc(newBytes);
    bool pooled = false, pinned = false;
    size_t oldBytes = 0;
    {
        std::lock_guard<std::mutex> lock(g_hostMutex);
        for (size_t i = 0; i < g_hostLive.size(); i++)
            if (g_hostLive[i].ptr == p) {
                pooled = true;
                pinned = g_hostLive[i].pinned;
                oldBytes = g_hostLive[i].bytes;
                if (!pinned) {  // out of the books while it may move
                    g_hostLive[i] = g_hostLive.back();
                    g_hostLive.pop_back();
                }
                break;
            }
    }
    if (pooled && !pinned) {
        const size_t rounded = (newBytes + ((size_t)2 << 20) - 1) / ((size_t)2 << 20) * ((size_t)2 << 20);
        void *q = rounded <= oldBytes ? p : mremap(p, oldBytes, rounded, MREMAP_MAYMOVE);
        if (q == MAP_FAILED) q = nullptr;
        std::lock_guard<std::mutex> lock(g_hostMutex);
        g_hostLive.push_back(HostBlock{q ? q : p, q ? (rounded > oldBytes ? rounded : oldBytes) : oldBytes, false, false});
        return q;  // on failure the old block is still the caller's (and back in the books)
    }
    if (!pooled && newBytes < kHostPoolMin) return realloc(p, newBytes);
    void *q = cpk_host_alloc(newBytes);
    if (!q) return nullptr;
    memcpy(q, p, usedBytes);
    cpk_host_free(p);
    return q;
}

// is [p, p + bytes) inside a pinned block of the pool?  (then a copy needs no staging)
static bool host_is_pinned(const void *p, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_hostMutex);
    for (const HostBlock &b : g_hostLive)
        if (b.pinned && (const char *)p >= (const char *)b.ptr && (const char *)p + bytes <= (const char *)b.ptr + b.bytes) return true;
    return false;
}

// Every entry point works on its batch's device and leaves the calling thread's current device as it found it: in a
// one-process-per-GPU job (torch.distributed, RCCL) the caller's allocations and collectives follow hipGetDevice().
namespace {
struct DeviceGuard {
    int prev = -1, dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) : dev(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
}  // namespace
#define CPK_ON_DEVICE(dev)        \
    DeviceGuard guard_(dev);      \
    HIP_TRY(guard_.err)

// ------------------------------------------------------------------------------------------------
// The idle reaper: one helper thread per process, started when a device first runs out of live batches.  A device
// that stays without a live batch for cache_idle_seconds() has its idle blocks above CPECAN_CACHE_KEEP_MB handed back
// to the driver -- so a finished alignment phase does not leave tens of GB hoarded beside torch / RCCL -- while a caller
// that runs one big batch after the other (create, run, download, destroy: zero live batches in between) keeps its
// blocks: hipFree + hipMalloc of a config-B ring block cost seconds (tests/test_gpu_parity.py:
// test_one_batch_at_a_time_does_not_stall).  The thread sleeps on a condition variable and is joined at exit, before the
// HIP runtime's own teardown (atexit handlers run in reverse order of registration; ours is registered after the first
// HIP call of the process).
// ------------------------------------------------------------------------------------------------
namespace {
struct IdleReaper {
    std::mutex m;
    std::condition_variable cv;
    std::thread th;
    bool started = false, stop = false;
    bool armed[kMaxDevices] = {};
    std::chrono::steady_clock::time_point since[kMaxDevices];
};
IdleReaper *g_reaper = nullptr;  // heap object that is never destroyed: the thread may outlive static destructors
std::once_flag g_reaperOnce;

void reaper_main() {
    IdleReaper &r = *g_reaper;
    const auto idle = std::chrono::duration_cast<std::chrono::steady_clock::duration>(
        std::chrono::duration<double>(cache_idle_seconds()));
    std::unique_lock<std::mutex> lock(r.m);
    while (!r.stop) {
        bool any = false;
        std::chrono::steady_clock::time_point next{};
        for (int dev = 0; dev < kMaxDevices; dev++)
            if (r.armed[dev] && (!any || r.since[dev] + idle < next)) {
                next = r.since[dev] + idle;
                any = true;
            }
        if (!any) {
            r.cv.wait(lock);
            continue;
        }
        if (std::chrono::steady_clock::now() < next) {
            r.cv.wait_until(lock, next);
            continue;
        }
        for (int dev = 0; dev < kMaxDevices && !r.stop; dev++) {
            if (!r.armed[dev] || std::chrono::steady_clock::now() < r.since[dev] + idle) continue;
            r.armed[dev] = false;
            if (g_liveShells[dev].load() > 0) continue;  // a batch came back in the meantime
            lock.unlock();
            if (hipSetDevice(dev) == hipSuccess)
                (void)cache_trim(dev, (size_t)(cache_keep_mb() * 1048576.0));
            else
                (void)hipGetLastError();
            lock.lock();
        }
    }
}

void reaper_stop() {
    IdleReaper *r = g_reaper;
    if (!r) return;
    {
        std::lock_guard<std::mutex> lock(r->m);
        r->stop = true;
    }
    r->cv.notify_all();
    if (r->th.joinable()) r->th.join();
}

// the last live batch of `device` has just been destroyed (the current device is `device`)
void reaper_arm(int device) {
    if (cache_keep_mb() < 0.0 || cache_idle_seconds() < 0.0) return;
    if (cache_idle_seconds() == 0.0) {  // round 3's behaviour: at once
        (void)cache_trim(device, (size_t)(cache_keep_mb() * 1048576.0));
        return;
    }
    std::call_once(g_reaperOnce, [] { g_reaper = new IdleReaper(); });
    IdleReaper &r = *g_reaper;
    {
        std::lock_guard<std::mutex> lock(r.m);
        if (r.stop) return;
        r.armed[device] = true;
        r.since[device] = std::chrono::steady_clock::now();
        if (!r.started) {
            r.started = true;
            r.th = std::thread(reaper_main);
            atexit(reaper_stop);
        }
    }
    r.cv.notify_all();
}

// a batch is being created on `device`: its idle blocks are about to be wanted again
void reaper_disarm(int device) {
    IdleReaper *r = g_reaper;
    if (!r) return;
    std::lock_guard<std::mutex> lock(r->m);
    r->armed[device] = false;
}
}  // namespace

struct CpkDevice;
static std::vector<CpkDevice *> g_shells[kMaxDevices];  // idle device shells (guarded by g_cacheMutex)

struct CpkDevice {
    int device = 0;
    int numCUs = 0;
    CpkGeometry geo{};
    KConsts kc{};
    int nLists = 1;
    int64_t nSegs = 0, nDiags = 0;
    int64_t outTriplesPerList = 0;
    int64_t dbgCells = 0, dbgDiags = 0;
    std::vector<LaunchClass> classes;  // one launch each: the wide classes (sweep kernel), then the narrow ones (packed)
    int totalWaves = 0;
    // device buffers
    CpkRegion *dRegions = nullptr;
    CpkDiag *dDiags = nullptr;
    int32_t *dDiagPos = nullptr;  // positions of the absolute-position sweeps, one word per diagonal (fixed expansions only)
    CpkSegment *dSegs = nullptr;
    uint8_t *dSymbols = nullptr;
    CpkModel *dModel = nullptr;
    double *dRing = nullptr; Candidate *dCand = nullptr; double *dForward = nullptr, *dExpect = nullptr; double *dC = nullptr, *dM = nullptr, *dTotals = nullptr, *dGroll = nullptr, *dBring = nullptr;
    // The per-region counts and per-segment offsets the sweeps write (a few integers per region, never read back on the
    // device) live in PINNED HOST memory that the kernels store to directly: the host reads them as soon as the sweep's
    // stop event has completed.  As device buffers they needed three small copies on the batch's stream, and those
    // queued behind the NEXT batch's upload in a pipeline: 18 ms per config-4 batch (profiles/r02_e2e_stages_config4.txt).
    int32_t *dCounts = nullptr, *dSegStarts = nullptr, *dSegCounts = nullptr, *dTriples = nullptr;
    void *hostCounts = nullptr;  // the block of the host pool that holds the three
    CpkItem *dItems = nullptr;
    int *dProgress = nullptr;  // fused classes: per region, segments whose forward values are complete (+ an error word)
    bool fusedRetried = false; // a fused class timed out once and runs as two launches now (cpk_device_download)
    int32_t *dCompact = nullptr; CpkChunk *dChunks = nullptr; int64_t compactCap = 0, chunkCap = 0;
    unsigned int *dQueue = nullptr;
    double *dDbgFb = nullptr, *dDbgTotals = nullptr;
    int64_t bytes = 0;
    std::vector<CachedBlock> allocs;  // every device block this batch holds, with its size (for the block cache)
    size_t compactBytes = 0, chunkBytes = 0;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    hipEvent_t evA = nullptr, evB = nullptr;  // copy timing (owned by the shell: nothing to leak on an error path)
    hipEvent_t evUp0 = nullptr, evUp1 = nullptr;  // around the upload's copies; the sweep waits for evUp1 (cpk_device_run)
    // cpk_device_set_model: the pinned source of the last model copy and the event that says it has been read
    CpkModel *hModel = nullptr;
    hipEvent_t evModel = nullptr;
    // Model slots (CpkBatchPlan::modelSlots): the reserved count (0: a plain batch), the models of the next run, the
    // device table the SLOTS kernels read and its pinned source, and the doubles of dExpect ([slot][wave][128] per class)
    int modelSlots = 0, activeModels = 1;
    CpkSlotModel *dSlots = nullptr, *hSlots = nullptr;
    int64_t expectDoubles = 0;
    bool uploadTimed = true;
    double h2dMs = 0.0;
    hipStream_t lastStream = nullptr;
    // Copies, memsets and the small kernels around the sweep (table build, list gather, consumers) run on this
    // non-blocking stream of the batch's own, never on the null stream, and the batch waits on ITS events and streams,
    // never on the device: batch k+1 is planned and uploaded and batch k-1 is gathered and downloaded while the sweep
    // kernel of batch k runs (a pipeline of batches from one host thread, or batches on several host threads).
    hipStream_t io = nullptr;
    double kernelMsAccum = 0.0;  // launches before the last one (an overflow re-run)
    // Host-to-device copies go through this pinned buffer of the shell's own.  A copy from the caller's pageable memory
    // makes the runtime pin and unpin those pages around the transfer -- GPU page-table updates that stall whatever
    // kernel is running: a batch uploaded beside another batch's sweep cost that sweep 25-30 ms
    // (profiles/r02_interference.txt).
    void *hStage = nullptr;
    size_t hStageBytes = 0;
    // every class but the first runs beside it on a stream of its own (fork / join around cpk_device_run)
    hipStream_t sideStream[kMaxClasses] = {};
    hipEvent_t sideDone[kMaxClasses] = {};
    bool ran = false;
};

extern "C" int cpk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int cpk_current_device(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    return dev;
}

static void shell_delete(CpkDevice *d) {  // the shell's device is current
    if (d->hStage) (void)hipHostFree(d->hStage);
    if (d->evStart) (void)hipEventDestroy(d->evStart);
    if (d->evStop) (void)hipEventDestroy(d->evStop);
    if (d->evA) (void)hipEventDestroy(d->evA);
    if (d->evB) (void)hipEventDestroy(d->evB);
    if (d->evUp0) (void)hipEventDestroy(d->evUp0);
    if (d->evUp1) (void)hipEventDestroy(d->evUp1);
    if (d->evModel) (void)hipEventDestroy(d->evModel);
    if (d->hModel) (void)hipHostFree(d->hModel);
    if (d->hSlots) (void)hipHostFree(d->hSlots);
    if (d->io) (void)hipStreamDestroy(d->io);
    for (int k = 0; k < kMaxClasses; k++) {
        if (d->sideStream[k]) (void)hipStreamDestroy(d->sideStream[k]);
        if (d->sideDone[k]) (void)hipEventDestroy(d->sideDone[k]);
    }
    delete d;
}

static int shell_init(CpkDevice *d, int device) {
    d->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    d->numCUs = prop.multiProcessorCount;
    HIP_TRY(hipEventCreate(&d->evStart));
    HIP_TRY(hipEventCreate(&d->evStop));
    HIP_TRY(hipEventCreate(&d->evA));
    HIP_TRY(hipEventCreate(&d->evB));
    HIP_TRY(hipEventCreate(&d->evUp0));
    HIP_TRY(hipEventCreate(&d->evUp1));
    {
        // The batch's own stream (copies, the table build, gather and consumers) has the high priority: its small kernels
        // then take the wave slots a draining sweep of ANOTHER batch gives back before that sweep's own queued workgroups
        // do -- the table build of batch k + 1 runs beside the tail of sweep k instead of behind it (CPECAN_IO_PRIORITY=0:
        // the default priority, as rounds 1-3).
        int prLow = 0, prHigh = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prLow, &prHigh));
        const char *env = getenv("CPECAN_IO_PRIORITY");
        if (env && atoi(env) == 0) prHigh = 0;
        HIP_TRY(hipStreamCreateWithPriority(&d->io, hipStreamNonBlocking, prHigh));
    }
    // The side streams of a multi-class batch are created when a batch first needs them (cpk_device_run): the runtime
    // maps streams onto a handful of hardware queues (4 by default), and ten idle streams per shell put a batch's sweep
    // into the same hardware queue as another batch's copies -- a pipeline of batches then ran its sweeps ~100 ms late
    // (profiles/r02_pipeline_trace.txt).
    return CPECAN_OK;
}

extern "C" int cpk_device_create(CpkDevice **out, int device) {
    int n = cpk_device_count();
    if (n <= 0 || device < 0 || device >= n) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", n, device);
        return CPECAN_ENODEVICE;
    }
    CPK_ON_DEVICE(device);
    if (device < kMaxDevices) {  // an idle shell of an earlier batch: its streams and events are ready
        std::lock_guard<std::mutex> lock(g_cacheMutex);
        if (!g_shells[device].empty()) {
            *out = g_shells[device].back();
            g_shells[device].pop_back();
            g_liveShells[device]++;
            reaper_disarm(device);
            return CPECAN_OK;
        }
    }
    CpkDevice *d = new CpkDevice();
    if (int rc = shell_init(d, device)) {
        shell_delete(d);  // whatever was created before the failure
        return rc;
    }
    if (device < kMaxDevices) {
        g_liveShells[device]++;
        reaper_disarm(device);
    }
    *out = d;
    return CPECAN_OK;
}

// Idle device blocks of `device` (-1: every device) and idle host blocks go back to the driver / the OS.  For a process
// that shares the GPU with another allocator (torch, RCCL): call it when a phase of alignment work is over.
extern "C" int64_t cpk_cache_trim(int device) {
    int64_t freed = 0;
    const int n = cpk_device_count();
    for (int dev = 0; dev < n && dev < kMaxDevices; dev++) {
        if (device >= 0 && dev != device) continue;
        {  // a device this process never used has nothing cached: do not create a context on it
            std::lock_guard<std::mutex> lock(g_cacheMutex);
            if (g_blockCache[dev].blocks.empty()) continue;
        }
        DeviceGuard guard(dev);
        if (guard.err != hipSuccess) continue;
        freed += (int64_t)cache_trim(dev, 0);
    }
    freed += (int64_t)host_trim();
    return freed;
}

// Waits for everything this batch has in flight: its sweep launches (the stop event on the caller's stream) and its own
// stream.  Nothing else ever touches the batch's blocks, so they may be recycled afterwards -- without draining the
// device, which may be busy with another batch.
static void batch_quiesce(CpkDevice *d) {
    if (d->ran) (void)hipEventSynchronize(d->evStop);
    if (d->io) (void)hipStreamSynchronize(d->io);
}

static void free_all(CpkDevice *d) {
    if (!d->allocs.empty() || d->dCompact || d->dChunks) batch_quiesce(d);  // nothing in flight uses them
    for (const CachedBlock &b : d->allocs) cache_free(d->device, b.ptr, b.bytes);
    d->allocs.clear();
    cache_free(d->device, d->dCompact, d->compactBytes);
    cache_free(d->device, d->dChunks, d->chunkBytes);
    d->compactBytes = d->chunkBytes = 0;
    d->dRegions = nullptr; d->dDiags = nullptr; d->dDiagPos = nullptr; d->dSegs = nullptr; d->dSymbols = nullptr; d->dModel = nullptr;
    d->dRing = d->dC = d->dM = d->dTotals = d->dGroll = d->dBring = nullptr;
    d->dCand = nullptr;
    d->dForward = nullptr;
    d->dExpect = nullptr;
    d->dSlots = nullptr;
    d->dCounts = d->dSegStarts = d->dSegCounts = d->dTriples = nullptr;
    cpk_host_free(d->hostCounts);
    d->hostCounts = nullptr;
    d->dItems = nullptr;
    d->dProgress = nullptr;
    d->dCompact = nullptr; d->dChunks = nullptr; d->compactCap = d->chunkCap = 0;
    d->dQueue = nullptr;
    d->dDbgFb = d->dDbgTotals = nullptr;
    d->bytes = 0;
}

static void ran_set(CpkDevice *d, bool ran) {
    if (d->ran != ran && d->device >= 0 && d->device < kMaxDevices) g_ranAlive[d->device] += ran ? 1 : -1;
    d->ran = ran;
}

extern "C" void cpk_device_destroy(CpkDevice *d) {
    if (!d) return;
    DeviceGuard guard(d->device);
    free_all(d);
    if (d->device >= 0 && d->device < kMaxDevices) {
        // When the last batch leaves a device its large idle blocks (a config-B batch's rings are ONE block of 60 GB) go
        // back to the driver -- not now (round 3 did, and the next big batch paid seconds of hipMalloc for it) but once
        // the device has stayed without a live batch for CPECAN_CACHE_IDLE_S: the idle reaper above.
        const bool last = --g_liveShells[d->device] <= 0;
        if (last) reaper_arm(d->device);
    }
    if (d->device < kMaxDevices) {  // keep the shell (streams, events) for the next batch on this device
        d->classes.clear();
        ran_set(d, false);
        d->lastStream = nullptr;
        d->modelSlots = 0;
        d->activeModels = 1;
        std::lock_guard<std::mutex> lock(g_cacheMutex);
        if (g_shells[d->device].size() < 16) {
            g_shells[d->device].push_back(d);
            return;
        }
    }
    shell_delete(d);
}

template <typename T>
static int dev_alloc(CpkDevice *d, T **p, size_t count) {
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIP_TRY(cache_alloc(d->device, (void **)p, bytes));
    d->allocs.push_back({(void *)*p, bytes});
    d->bytes += (int64_t)bytes;
    return CPECAN_OK;
}
// gives one block of the batch back (the device is idle)
static void dev_release(CpkDevice *d, void *p) {
    for (size_t i = 0; i < d->allocs.size(); i++)
        if (d->allocs[i].ptr == p) {
            cache_free(d->device, p, d->allocs[i].bytes);
            d->bytes -= (int64_t)d->allocs[i].bytes;
            d->allocs[i] = d->allocs.back();
            d->allocs.pop_back();
            return;
        }
}

// Queues dst <- src (host) on the batch's stream through the shell's pinned buffer; `at` is the running offset in it.
constexpr size_t kStageMaxCopy = (size_t)64 << 20;  // larger sources are never copied through the shell's staging buffer
static int staged_h2d(CpkDevice *d, void *dst, const void *src, size_t bytes, size_t *at) {
    if (bytes == 0) return CPECAN_OK;
    // a pinned block of the host pool: the copy engine reads it where it lies.  A large block in its first life is not
    // pinned yet: the runtime copies it the pageable way (through its own staging), which only hurts beside a running
    // sweep -- and in a pipeline the blocks are in their second life.
    if (bytes > kStageMaxCopy || host_is_pinned(src, bytes)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->io));
        return CPECAN_OK;
    }
    const size_t off = (*at + 255) / 256 * 256;
    if (off + bytes > d->hStageBytes) {
        cpk_set_error("internal: staging buffer too small");
        return CPECAN_ESTATE;
    }
    memcpy((char *)d->hStage + off, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, (char *)d->hStage + off, bytes, hipMemcpyHostToDevice, d->io));
    *at = off + bytes;
    return CPECAN_OK;
}
static int stage_reserve(CpkDevice *d, size_t bytes) {
    if (bytes <= d->hStageBytes) return CPECAN_OK;
    HIP_TRY(hipStreamSynchronize(d->io));
    if (d->hStage) (void)hipHostFree(d->hStage);
    d->hStage = nullptr;
    d->hStageBytes = 0;
    const size_t want = (bytes + (bytes >> 2) + (1u << 20)) / 4096 * 4096;
    HIP_TRY(hipHostMalloc(&d->hStage, want, hipHostMallocDefault));
    d->hStageBytes = want;
    return CPECAN_OK;
}

// split classes: the regions get rings of their own (no wrap: every segment stays readable) and their tracebacks
// become queue items, longest first.  A class with chains (plan_chains): one chain item (seg = -chainFrom) for every region
// with more than chainFrom segments in place of the plain items of those segments, in the same list by the same measure.
// costs (tests): the measure of every item, in step with *items.
static void build_item_queue(std::vector<LaunchClass> &classes, CpkRegion *regions, const CpkSegment *segs, int S, std::vector<CpkItem> *items,
                             std::vector<int64_t> *costs = nullptr) {
    for (LaunchClass &c : classes) {
        if (!c.split()) continue;
        int64_t ringAt = 0;  // in doubles, from the class's ring pointer (dRing + oRing)
        c.itemBase = (int64_t)items->size();
        std::vector<std::pair<int64_t, CpkItem>> byCost;
        for (int64_t di = c.regionBase; di < c.regionBase + c.regionCount; di++) {
            CpkRegion &rg = regions[di];
            rg.ringCap = 0x7fffffff;  // never wraps: the ring holds every diagonal of the region
            rg.ringBase = ringAt;
            rg.split = 1;
            ringAt += split_ring_doubles(rg, S);
            const bool chained = c.chainFrom > 0 && rg.nSeg > c.chainFrom;
            if (chained) byCost.push_back({chain_cost(rg, segs, c.chainFrom), CpkItem{(int32_t)di, -c.chainFrom}});
            for (int32_t si = 0; si < (chained ? c.chainFrom : rg.nSeg); si++) {
                const CpkSegment &sg = segs[rg.segOff + si];
                // fused: a segment's forward values exist when the forward wave has passed its top diagonal -- items in
                // the order in which they become ready (that diagonal), longest first among equals
                const int64_t cost = item_cost(rg, sg);
                byCost.push_back({c.fused() ? ((int64_t)0x7fffffff - sg.dTop) * ((int64_t)1 << 32) + (cost >> 8) : cost, CpkItem{(int32_t)di, si}});
            }
        }
        std::stable_sort(byCost.begin(), byCost.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
        for (const auto &e : byCost) {
            items->push_back(e.second);
            if (costs) costs->push_back(e.first);
        }
        c.itemCount = (int64_t)items->size() - c.itemBase;
    }
}

static KConsts kconsts_of(const CpkModel *model) {
    return KConsts{model->matchContinue, model->matchFromShortX, model->matchFromShortY, model->matchFromLongX,
                   model->matchFromLongY, model->shortOpenX, model->shortOpenY, model->shortExtendX,
                   model->shortExtendY, model->shortSwitchToX, model->shortSwitchToY, model->longOpenX,
                   model->longOpenY, model->longExtendX, model->longExtendY, model->threshold};
}
// the waves of a run with the batch's active models, over all classes (cpecan_stats::wavesPerLaunch)
static void count_waves(CpkDevice *d) {
    d->totalWaves = 0;
    for (const LaunchClass &c : d->classes)
        d->totalWaves += (c.split() && c.wavesTrace > c.waves ? c.wavesTrace : c.wavesWith(d->activeModels)) * (c.threads / CPK_WAVE);
}

// CPK_LAUNCH_PLAN_FIELDS numbers per class, in launch order: what cpk_plan_describe and cpk_device_launch_forms answer.
// (The 23rd number, "items" to the tests, is the TRACEBACK SEGMENTS the class's queue hands out, not the queue's length: a
// chain counts as the segments it covers, so the number does not move with the chains -- tests/test_gang_plan_cpu.py holds
// the default plan to that of CPECAN_GANG=0 in it.  The length of the queue itself: cpk_plan_chains, *nItems.)
static int describe_classes(const std::vector<LaunchClass> &classes, int64_t *out, int maxClasses) {
    if ((int)classes.size() > maxClasses) return CPECAN_EINVAL;
    for (size_t i = 0; i < classes.size(); i++) {
        const LaunchClass &c = classes[i];
        const int64_t f[CPK_LAUNCH_PLAN_FIELDS] = {
            c.packed, c.k, c.regionCount, c.geo.maxWidth, c.geo.nStates, c.form.family, c.form.mode, c.form.wps, c.form.abs, c.form.gang,
            c.split() && !c.fused() ? c.formTrace.wps : 0, c.split() && !c.fused() ? c.formTrace.gang : 0, c.waves, c.wavesTrace, c.gang,
            c.gangTrace, (int64_t)c.ldsBytes, (int64_t)c.ldsBytesFwd, (int64_t)c.firstLdsBytes(), (int64_t)c.traceLdsBytes(), c.subSlots,
            c.threads, c.itemCount + c.chainedSegs - c.chains, c.firstGrid(1), c.geo.useGlobalRoll};
        for (int j = 0; j < CPK_LAUNCH_PLAN_FIELDS; j++) out[i * CPK_LAUNCH_PLAN_FIELDS + j] = f[j];
    }
    return (int)classes.size();
}

// The launches of a batch on a device that is not there (tests of the plan): CPK_LAUNCH_PLAN_FIELDS numbers per class.
static int plan_without_device(const CpkBatchPlan *plan, int numCUs, int64_t memBytes, std::vector<LaunchClass> *classes) {
    const PlanKnobs knobs;  // (reads the environment)
    PlanDevice dev;
    dev.numCUs = numCUs;
    dev.freeBytes = dev.totalBytes = (size_t)memBytes;
    dev.queryKernels = false;
    return plan_batch(*plan, dev, knobs, classes);
}
extern "C" int cpk_plan_describe(const CpkBatchPlan *plan, int numCUs, int64_t memBytes, int64_t *out, int maxClasses) {
    std::vector<LaunchClass> classes;
    if (int rc = plan_without_device(plan, numCUs, memBytes, &classes)) return rc;
    return describe_classes(classes, out, maxClasses);
}
// The chains of the same plan (plan_chains) and the item queues built from it, for tests.  chainsOut: CPK_CHAIN_PLAN_FIELDS
// numbers per class, in launch order -- the first segment of its chains (0: none) and how many there are.  itemsOut (may be
// null): CPK_CHAIN_ITEM_FIELDS numbers per queue item of every split class, in queue order -- class, device region, segment
// (-K: a chain from segment K), cost, segments of the region, leading segments of the region that the class's forward launch
// sweeps (forward_launch_segments; the whole region where the forward sweep is not a launch of its own); *nItems receives their
// number (no more than maxItems are written).  Returns the number of classes.  The plan's regions get their rings set as an upload sets them.
extern "C" int cpk_plan_chains(const CpkBatchPlan *plan, int numCUs, int64_t memBytes, int64_t *chainsOut, int maxClasses, int64_t *itemsOut,
                               int64_t maxItems, int64_t *nItems) {
    CpkRegion *regions = plan->regions;
    const CpkSegment *segs = plan->segs;
    std::vector<LaunchClass> classes;
    if (int rc = plan_without_device(plan, numCUs, memBytes, &classes)) return rc;
    if ((int)classes.size() > maxClasses) return CPECAN_EINVAL;
    for (size_t i = 0; i < classes.size(); i++) {
        chainsOut[i * CPK_CHAIN_PLAN_FIELDS] = classes[i].chainFrom;
        chainsOut[i * CPK_CHAIN_PLAN_FIELDS + 1] = classes[i].chains;
    }
    if (itemsOut && nItems) {
        std::vector<CpkItem> items;
        std::vector<int64_t> costs;
        build_item_queue(classes, regions, segs, plan->geo.nStates, &items, &costs);
        *nItems = (int64_t)items.size();
        for (size_t ci = 0; ci < classes.size(); ci++) {
            const LaunchClass &c = classes[ci];
            if (!c.split()) continue;
            for (int64_t i = c.itemBase; i < c.itemBase + c.itemCount && i < maxItems; i++) {
                const CpkRegion &rg = regions[items[i].region];
                const int64_t f[CPK_CHAIN_ITEM_FIELDS] = {(int64_t)ci, items[i].region, items[i].seg, costs[i], rg.nSeg, forward_launch_segments(c.chainFrom, rg.nSeg)};
                for (int j = 0; j < CPK_CHAIN_ITEM_FIELDS; j++) itemsOut[i * CPK_CHAIN_ITEM_FIELDS + j] = f[j];
            }
        }
    }
    return (int)classes.size();
}
// ... and of an uploaded batch on the device it was planned for, with the registers the loaded kernels report: the same numbers.
extern "C" int cpk_device_launch_forms(const CpkDevice *d, int64_t *out, int maxClasses) { return describe_classes(d->classes, out, maxClasses); }
// kKernelTable as data (tests: every built variant has a test that runs it): CPK_KERNEL_FORM_FIELDS numbers per entry, the
// fields of KernelForm in their order; returns the number of entries.  No device needed.
// ... and, in step with it, whether an entry is a CHAIN build (KernelForm::chain): one number per entry.
extern "C" int cpk_kernel_table_chain(int64_t *out, int maxEntries) {
    const int n = (int)(sizeof kKernelTable / sizeof kKernelTable[0]);
    if (n > maxEntries) return CPECAN_EINVAL;
    for (int i = 0; i < n; i++) out[i] = kKernelTable[i].form.chain;
    return n;
}
extern "C" int cpk_kernel_table_forms(int64_t *out, int maxEntries) {
    const int n = (int)(sizeof kKernelTable / sizeof kKernelTable[0]);
    if (n > maxEntries) return CPECAN_EINVAL;
    for (int i = 0; i < n; i++) {
        const KernelForm &k = kKernelTable[i].form;
        const int64_t f[CPK_KERNEL_FORM_FIELDS] = {k.family, k.S, k.emit, k.mode, k.fast, k.wps, k.abs, k.inSweep, k.slots, k.dynamic, k.width, k.gang};
        for (int j = 0; j < CPK_KERNEL_FORM_FIELDS; j++) out[i * CPK_KERNEL_FORM_FIELDS + j] = f[j];
    }
    return n;
}

extern "C" int cpk_device_upload(CpkDevice *d, const CpkBatchPlan *plan, const CpkModel *model, double *h2dMs) {
    if (plan->modelSlots < 0 || plan->modelSlots > CPECAN_MAX_MODEL_SLOTS) return CPECAN_EINVAL;
    CPK_ON_DEVICE(d->device);
    free_all(d);
    d->kernelMsAccum = 0.0;
    d->fusedRetried = false;
    d->geo = plan->geo;
    d->kc = kconsts_of(model);
    d->modelSlots = plan->modelSlots;
    d->activeModels = 1;
    d->nLists = plan->nLists;
    d->nSegs = plan->nSegs;
    d->nDiags = plan->nDiags;
    d->outTriplesPerList = plan->outTriplesPerList;
    d->dbgCells = plan->dbgCells;
    d->dbgDiags = plan->dbgDiags;
    ran_set(d, false);
    const int S = plan->geo.nStates;

    // ---- the launches of a run: planned (cpk_plan.inl), then carried out ----
    const PlanKnobs knobs;  // (reads the environment)
    PlanDevice dev;
    dev.numCUs = d->numCUs;
    HIP_TRY(hipMemGetInfo(&dev.freeBytes, &dev.totalBytes));
    dev.idleCachedBytes = cache_bytes(d->device);
    dev.othersAlive = d->device >= 0 && d->device < kMaxDevices && g_ranAlive[d->device] > 0;  // (this batch no longer counts: ran_set above)
    if (int rc = plan_batch(*plan, dev, knobs, &d->classes)) return rc;
    const int slotCount = d->modelSlots > 0 ? d->modelSlots : 1;
    {
        // (the rings start 64 doubles into their block and the block ends 256 doubles behind them: the streamed traceback's
        // prefetch reads up to 63 words in front of a diagonal's row and up to 191 behind it, Sweep::tracebackAbs)
        int64_t oRing = 64, oCand = 0, oRef = 0, oTot = 0, oBring = 0, oGroll = 0, oExpect = 0;
        for (LaunchClass &c : d->classes) {
            c.oRing = oRing;
            c.oCand = oCand;
            c.oRef = oRef;
            c.oTot = oTot;
            c.oBring = oBring;
            c.oGroll = oGroll;
            c.oExpect = oExpect;
            oRing += c.split() ? c.ringTotal : c.subSlots * c.ringEl;
            oRing = (oRing + 1) & ~(int64_t)1;  // the rings of a split class start on 16 bytes (Sweep::ringPut)
            oCand += c.subSlots * c.candEl;
            oRef += c.subSlots * c.refEl;
            oTot += c.subSlots * c.totEl;
            oBring += c.subSlots * c.bringEl;
            oGroll += c.subSlots * c.grollEl;
            oExpect += (int64_t)slotCount * c.waves * (c.threads / CPK_WAVE) * 128;  // a partial result per wave (and slot)
            if (c.ldsBytes > kLdsPathMaxBytes) {
                HIP_TRY(hipFuncSetAttribute((const void *)c.fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.ldsBytes));
                if (c.fnTrace())
                    HIP_TRY(hipFuncSetAttribute((const void *)c.fnTrace(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.ldsBytes));
            }
            // a gang may declare the whole LDS of a CU (the same bound for every batch that launches the kernel)
            if (c.gang > 1) HIP_TRY(hipFuncSetAttribute((const void *)c.fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCuLdsBytes));
            if (c.gangTrace > 1) HIP_TRY(hipFuncSetAttribute((const void *)c.fnTrace(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCuLdsBytes));
        }
        if (int rc = dev_alloc(d, &d->dRing, (size_t)oRing + 256)) return rc;
        if (int rc = dev_alloc(d, &d->dCand, (size_t)oCand)) return rc;
        if (int rc = dev_alloc(d, &d->dC, (size_t)oRef)) return rc;
        if (int rc = dev_alloc(d, &d->dM, (size_t)oRef)) return rc;
        if (int rc = dev_alloc(d, &d->dTotals, (size_t)oTot)) return rc;
        if (oGroll > 0)
            if (int rc = dev_alloc(d, &d->dGroll, (size_t)oGroll)) return rc;
        if (oBring > 0)
            if (int rc = dev_alloc(d, &d->dBring, (size_t)oBring)) return rc;
        d->expectDoubles = oExpect > 0 ? oExpect : 128;
        if (int rc = dev_alloc(d, &d->dExpect, (size_t)d->expectDoubles)) return rc;
        count_waves(d);
    }

    if (int rc = dev_alloc(d, &d->dRegions, (size_t)plan->geo.nRegions)) return rc;
    if (int rc = dev_alloc(d, &d->dDiags, (size_t)plan->nDiags)) return rc;
    {
        bool anyAbs = false;
        for (const LaunchClass &c : d->classes) anyAbs = anyAbs || c.abs;
        if (anyAbs)
            if (int rc = dev_alloc(d, &d->dDiagPos, (size_t)plan->nDiags)) return rc;
    }
    if (int rc = dev_alloc(d, &d->dSegs, (size_t)plan->nSegs)) return rc;
    if (int rc = dev_alloc(d, &d->dSymbols, (size_t)plan->nSymbolBytes)) return rc;
    if (int rc = dev_alloc(d, &d->dModel, 1)) return rc;
    if (int rc = dev_alloc(d, &d->dForward, (size_t)slotCount * plan->geo.nRegions)) return rc;
    if (d->modelSlots > 0)
        if (int rc = dev_alloc(d, &d->dSlots, (size_t)d->modelSlots)) return rc;
    {
        const size_t nC = (size_t)plan->nLists * plan->geo.nRegions, nS = (size_t)plan->nLists * (plan->nSegs ? plan->nSegs : 1);
        const size_t words = (nC + 63) / 64 * 64 + 2 * ((nS + 63) / 64 * 64);
        const size_t bytes = sizeof(int32_t) * words;
        d->hostCounts = host_alloc_impl(bytes, true);
        if (!d->hostCounts) {
            cpk_set_error("no pinned host memory for the result counts (%zu bytes)", bytes);
            return CPECAN_ENOMEM;
        }
        memset(d->hostCounts, 0, sizeof(int32_t) * words);  // the block is idle: nothing is in flight for this batch yet
        d->dCounts = static_cast<int32_t *>(d->hostCounts);
        d->dSegStarts = d->dCounts + (nC + 63) / 64 * 64;
        d->dSegCounts = d->dSegStarts + (nS + 63) / 64 * 64;
    }
    std::vector<CpkItem> items;
    build_item_queue(d->classes, plan->regions, plan->segs, S, &items);
    if (int rc = dev_alloc(d, &d->dItems, items.empty() ? 1 : items.size())) return rc;
    {
        bool anyFused = false;
        for (const LaunchClass &c : d->classes) anyFused = anyFused || c.fused();
        if (anyFused)
            if (int rc = dev_alloc(d, &d->dProgress, (size_t)plan->geo.nRegions + 1)) return rc;
    }
    if (int rc = dev_alloc(d, &d->dTriples, (size_t)plan->nLists * plan->outTriplesPerList * 3)) return rc;
    if (int rc = dev_alloc(d, &d->dQueue, (size_t)2 * kMaxClasses)) return rc;
    hipStream_t io = d->io;

    if (plan->geo.debug) {
        if (int rc = dev_alloc(d, &d->dDbgFb, (size_t)plan->dbgCells)) return rc;
        if (int rc = dev_alloc(d, &d->dDbgTotals, (size_t)plan->dbgDiags)) return rc;
        HIP_TRY(hipMemsetAsync(d->dDbgFb, 0xff, sizeof(double) * (size_t)plan->dbgCells, io));      // NaN pattern
        HIP_TRY(hipMemsetAsync(d->dDbgTotals, 0xff, sizeof(double) * (size_t)plan->dbgDiags, io));
    }

    // Everything below is ordered on the batch's own stream and the call returns WITHOUT waiting for it: the sources are
    // either blocks of the host pool that the batch owns until it is destroyed, or already copied into the shell's
    // staging buffer; cpk_device_run makes the sweep wait for evUp1.  (The host goes on planning the next batch while
    // the copy engine works: 19 ms per config-4 batch.)  The anchor block stays with the batch until it is destroyed.
    size_t stageAt = 0;
    // (anchors as runs: 16 bytes per run cross the bus and cpecan_expand_runs writes the anchors the table builders read)
    const size_t anchorBytes = plan->runs ? sizeof(int32_t) * 4 * (size_t)(plan->nRuns > 0 ? plan->nRuns : 1)
                                    : sizeof(cpk_anchor_t) * (size_t)plan->anchorStride * (size_t)(plan->nAnchors > 0 ? plan->nAnchors : 1);
    {
        auto staged = [](const void *p, size_t bytes) { return (bytes > kStageMaxCopy || host_is_pinned(p, bytes)) ? (size_t)0 : bytes + 256; };
        if (int rc = stage_reserve(d, staged(plan->regions, sizeof(CpkRegion) * (size_t)plan->geo.nRegions) + staged(plan->runs ? (const void *)plan->runs : (const void *)plan->anchors, anchorBytes) +
                                      staged(plan->segs, sizeof(CpkSegment) * (size_t)plan->nSegs) + staged(plan->symbols, (size_t)plan->nSymbolBytes) +
                                      sizeof(CpkModel) + sizeof(CpkSlotModel) + sizeof(CpkItem) * items.size() + 9 * 256))
            return rc;
    }
    if (!items.empty())
        if (int rc = staged_h2d(d, d->dItems, items.data(), sizeof(CpkItem) * items.size(), &stageAt)) return rc;
    HIP_TRY(hipEventRecord(d->evUp0, io));
    if (int rc = staged_h2d(d, d->dRegions, plan->regions, sizeof(CpkRegion) * (size_t)plan->geo.nRegions, &stageAt)) return rc;
    {
        // anchors -> per-diagonal table, on the device (the anchors are only needed for this)
        cpk_anchor_t *dAnchors = nullptr;
        if (int rc = dev_alloc(d, &dAnchors, (size_t)plan->anchorStride * (size_t)(plan->nAnchors > 0 ? plan->nAnchors : 1))) return rc;
        if (plan->runs && plan->nRuns > 0) {
            int32_t *dRuns = nullptr;
            if (int rc = dev_alloc(d, &dRuns, (size_t)4 * (size_t)plan->nRuns)) return rc;
            if (int rc = staged_h2d(d, dRuns, plan->runs, sizeof(int32_t) * 4 * (size_t)plan->nRuns, &stageAt)) return rc;
            const int64_t blocks = (plan->nRuns + 255) / 256;
            hipLaunchKernelGGL(cpecan_expand_runs, dim3((unsigned)(blocks < 65535 * 16 ? blocks : 65535 * 16)), dim3(256), 0, io,
                               reinterpret_cast<const int4 *>(dRuns), plan->nRuns, dAnchors);
            HIP_TRY(hipGetLastError());
        } else if (plan->nAnchors > 0)
            if (int rc = staged_h2d(d, dAnchors, plan->anchors, sizeof(cpk_anchor_t) * (size_t)plan->anchorStride * (size_t)plan->nAnchors, &stageAt)) return rc;
        if (int rc = staged_h2d(d, d->dSegs, plan->segs, sizeof(CpkSegment) * (size_t)plan->nSegs, &stageAt)) return rc;  // the builder reads the schedule
        // (the symbols and the model go first: nothing but the table build is then between the last copy and the sweep)
        if (int rc = staged_h2d(d, d->dSymbols, plan->symbols, (size_t)plan->nSymbolBytes, &stageAt)) return rc;
        if (int rc = staged_h2d(d, d->dModel, model, sizeof(CpkModel), &stageAt)) return rc;
        if (d->dSlots) {  // a reserved batch starts with its own model in slot 0
            const CpkSlotModel s0{d->kc, *model};
            if (int rc = staged_h2d(d, d->dSlots, &s0, sizeof s0, &stageAt)) return rc;
        }
        // the regions of split classes: one wave per region (cpk_table_gather.inl); every other region: one thread
        // (CPECAN_TABLE_WAVE=0: one thread for all, as rounds 1-3 -- tests compare the two)
        const char *twEnv = getenv("CPECAN_TABLE_WAVE");
        const bool tableWave = !(twEnv && atoi(twEnv) == 0);
        int64_t nSplitRegions = 0;
        for (const LaunchClass &c : d->classes)
            if (c.split() && tableWave) {
                hipLaunchKernelGGL(cpecan_build_diag_table_wave, dim3((unsigned)c.regionCount), dim3(64), 0, io, d->dRegions, c.regionBase,
                                   dAnchors, plan->anchorStride, d->dSegs, plan->geo.nStates, d->dDiags, d->dDiagPos, plan->expansion, plan->dynamic);
                HIP_TRY(hipGetLastError());
                nSplitRegions += c.regionCount;
            }
        if (nSplitRegions < plan->geo.nRegions) {
            hipLaunchKernelGGL(cpecan_build_diag_table, dim3((unsigned)((plan->geo.nRegions + 63) / 64)), dim3(64), 0, io,
                               d->dRegions, plan->geo.nRegions, dAnchors, plan->anchorStride, d->dSegs, plan->geo.nStates, d->dDiags, d->dDiagPos, plan->expansion,
                               plan->dynamic, tableWave ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(d->evUp1, io));
    }
    d->uploadTimed = false;
    d->h2dMs = 0.0;
    if (h2dMs) *h2dMs = 0.0;  // known once the copies are done: cpk_device_download reports it
    return CPECAN_OK;
}

// A new model for the next run of an uploaded batch.  The transitions travel in the kernel arguments (d->kc, read at the
// next launch); the priors and padded emissions are copied into dModel on the batch's own stream, behind the stop event
// of the last run -- a sweep still in flight reads the old table to its end -- and the next sweep waits for the copy
// through evUp1, as it waits for the upload's copies.
// n models (cpk_device_set_models) go the same way into the slot table of a reserved batch; slot 0 is *dModel as well.
extern "C" int cpk_device_set_models(CpkDevice *d, const CpkModel *models, int n) {
    CPK_ON_DEVICE(d->device);
    if (!d->dModel) {
        cpk_set_error("set_model before upload");
        return CPECAN_ESTATE;
    }
    if (n < 1 || n > (d->modelSlots > 0 ? d->modelSlots : 1)) {
        cpk_set_error("set_models: %d models for a batch that reserved %d", n, d->modelSlots);
        return CPECAN_EINVAL;
    }
    if (!d->hModel) HIP_TRY(hipHostMalloc(&d->hModel, sizeof(CpkModel), hipHostMallocDefault));
    if (d->dSlots && !d->hSlots) HIP_TRY(hipHostMalloc(&d->hSlots, sizeof(CpkSlotModel) * CPECAN_MAX_MODEL_SLOTS, hipHostMallocDefault));
    if (!d->evModel) HIP_TRY(hipEventCreateWithFlags(&d->evModel, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(d->evModel));  // the previous model copy has left the pinned block
    *d->hModel = models[0];
    hipStream_t io = d->io;
    if (d->ran) HIP_TRY(hipStreamWaitEvent(io, d->evStop, 0));
    HIP_TRY(hipMemcpyAsync(d->dModel, d->hModel, sizeof(CpkModel), hipMemcpyHostToDevice, io));
    if (d->dSlots) {
        for (int k = 0; k < n; k++) d->hSlots[k] = CpkSlotModel{kconsts_of(&models[k]), models[k]};
        HIP_TRY(hipMemcpyAsync(d->dSlots, d->hSlots, sizeof(CpkSlotModel) * (size_t)n, hipMemcpyHostToDevice, io));
    }
    HIP_TRY(hipEventRecord(d->evModel, io));
    HIP_TRY(hipEventRecord(d->evUp1, io));
    d->kc = kconsts_of(&models[0]);
    d->activeModels = n;
    count_waves(d);
    return CPECAN_OK;
}
extern "C" int cpk_device_set_model(CpkDevice *d, const CpkModel *model) { return cpk_device_set_models(d, model, 1); }

// duration of the upload's copies (valid once the batch has run: the sweep waited for them)
extern "C" double cpk_device_h2d_ms(CpkDevice *d) {
    if (!d->uploadTimed && d->evUp1 && hipEventSynchronize(d->evUp1) == hipSuccess) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, d->evUp0, d->evUp1) == hipSuccess) d->h2dMs = ms;
        d->uploadTimed = true;
    }
    return d->h2dMs;
}

extern "C" int cpk_device_update_regions(CpkDevice *d, const CpkRegion *regions, const CpkSegment *segs, int64_t outTriplesPerList) {
    CPK_ON_DEVICE(d->device);
    batch_quiesce(d);  // the run that overflowed has finished with the triples and the regions
    if (outTriplesPerList != d->outTriplesPerList) {
        if (d->dTriples) {
            dev_release(d, d->dTriples);
            d->dTriples = nullptr;
        }
        d->outTriplesPerList = outTriplesPerList;
        if (int rc = dev_alloc(d, &d->dTriples, (size_t)d->nLists * outTriplesPerList * 3)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(d->dRegions, regions, sizeof(CpkRegion) * (size_t)d->geo.nRegions, hipMemcpyHostToDevice, d->io));
    if (segs && d->nSegs > 0)
        HIP_TRY(hipMemcpyAsync(d->dSegs, segs, sizeof(CpkSegment) * (size_t)d->nSegs, hipMemcpyHostToDevice, d->io));
    HIP_TRY(hipStreamSynchronize(d->io));
    return CPECAN_OK;
}

// Runs the batch once more on the stream of its last run (after an output overflow); the time of the launches so far
// is kept so that the batch's kernel time covers all of them.
extern "C" int cpk_device_rerun(CpkDevice *d) {
    CPK_ON_DEVICE(d->device);
    if (d->ran) {
        HIP_TRY(hipEventSynchronize(d->evStop));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, d->evStart, d->evStop));
        d->kernelMsAccum += ms;
    }
    return cpk_device_run(d, (void *)d->lastStream);
}

extern "C" int cpk_device_run(CpkDevice *d, void *stream) {
    CPK_ON_DEVICE(d->device);
    hipStream_t st = (hipStream_t)stream;
    KArgs a{};
    a.kc = d->kc;
    a.regions = d->dRegions;
    a.diags = d->dDiags;
    a.dpos = d->dDiagPos;
    a.segs = d->dSegs;
    a.symbols = d->dSymbols;
    a.model = d->dModel;
    a.geo = d->geo;
    a.ring = d->dRing;
    a.cand = d->dCand;
    a.cbuf = d->dC;
    a.mbuf = d->dM;
    a.totals = d->dTotals;
    a.groll = d->dGroll;
    a.bring = d->dBring;
    a.outCounts = d->dCounts;
    a.segStarts = d->dSegStarts;
    a.segCounts = d->dSegCounts;
    a.items = d->dItems;
    a.progress = d->dProgress;
    a.itemCount = 0;
    a.triples = d->dTriples;
    a.outTriplesPerList = d->outTriplesPerList;
    a.nSegsTotal = d->nSegs;
    a.queue = d->dQueue;
    a.forwardOut = d->dForward;
    a.expectOut = d->dExpect;
    a.dbgFb = d->dDbgFb;
    a.dbgTotals = d->dDbgTotals;
    a.slotModels = d->dSlots;
    a.nModels = d->dSlots ? d->activeModels : 0;
    HIP_TRY(hipStreamWaitEvent(st, d->evUp1, 0));  // the upload's copies and the table build (the batch's own stream)
    HIP_TRY(hipMemsetAsync(d->dQueue, 0, 2 * kMaxClasses * sizeof(unsigned int), st));
    if (d->dProgress) HIP_TRY(hipMemsetAsync(d->dProgress, 0, sizeof(int) * ((size_t)d->geo.nRegions + 1), st));
    if (d->geo.emit == CPECAN_EMIT_EXPECT)
        HIP_TRY(hipMemsetAsync(d->dExpect, 0, sizeof(double) * (size_t)(d->dSlots ? d->expectDoubles : 128 * (int64_t)(d->totalWaves > 0 ? d->totalWaves : 1)), st));
    HIP_TRY(hipEventRecord(d->evStart, st));
    // one launch per size class, side by side: the last class (the widest regions, usually the bulk of the work) on the
    // caller's stream, the others on streams of their own, joined below
    const int nClasses = (int)d->classes.size();
    for (int i = 0; i < nClasses; i++) {
        const LaunchClass &c = d->classes[i];
        KArgs p = a;
        p.geo = c.geo;
        p.geo.debug = a.geo.debug;
        p.regionBase = c.regionBase;
        p.regionCount = c.regionCount;
        p.ring = d->dRing + c.oRing;
        p.cand = d->dCand + c.oCand;
        p.cbuf = d->dC + c.oRef;
        p.mbuf = d->dM + c.oRef;
        p.totals = d->dTotals + c.oTot;
        p.groll = d->dGroll ? d->dGroll + c.oGroll : nullptr;
        p.bring = d->dBring ? d->dBring + c.oBring : nullptr;
        p.expectOut = d->dExpect + c.oExpect;
        p.queue = d->dQueue + i;
        p.fwdSegs = c.chainFrom;  // (the kernel: forward_launch_segments(a.fwdSegs, rg.nSeg))
        if (c.fused()) {
            p.items = d->dItems + c.itemBase;
            p.itemCount = (int32_t)c.itemCount;
        }
        const bool onCaller = i == nClasses - 1;
        if (!onCaller && !d->sideStream[i]) {
            // A priority of its own: the runtime maps the streams of one priority onto a handful of hardware queues, and a
            // pipeline of batches has more streams alive than that -- a side stream that shares its hardware queue with
            // the caller's stream runs its class BEHIND the caller's instead of beside it (BASELINE config 4, two narrow
            // classes: 45 ms per batch instead of 28 whenever that happened, profiles/r04_config4_pipeline.txt).  The
            // queues of the high priority hold nothing but these side streams.
            {
                int prLow = 0, prHigh = 0;
                HIP_TRY(hipDeviceGetStreamPriorityRange(&prLow, &prHigh));
                const char *env = getenv("CPECAN_SIDE_PRIORITY");  // 0: the default priority, as rounds 1-3 (A/B runs)
                if (env && atoi(env) == 0) prHigh = 0;
                HIP_TRY(hipStreamCreateWithPriority(&d->sideStream[i], hipStreamNonBlocking, prHigh));
            }
            HIP_TRY(hipEventCreateWithFlags(&d->sideDone[i], hipEventDisableTiming));
        }
        hipStream_t cs = onCaller ? st : d->sideStream[i];
        if (!onCaller) HIP_TRY(hipStreamWaitEvent(cs, d->evStart, 0));
        hipLaunchKernelGGL(c.fn(), dim3(c.firstGrid(d->activeModels)), dim3(c.firstThreads()), c.firstLdsBytes(), cs, p);
        HIP_TRY(hipGetLastError());
        if (c.split() && !c.fused()) {  // the tracebacks of the class's regions, one queue item each, behind the forward launch
            KArgs t = p;
            t.items = d->dItems + c.itemBase;
            t.regionCount = (int32_t)c.itemCount;
            t.queue = d->dQueue + kMaxClasses + i;
            hipLaunchKernelGGL(c.fnTrace(), dim3(c.traceGrid()), dim3(c.traceThreads()), c.traceLdsBytes(), cs, t);
            HIP_TRY(hipGetLastError());
        }
        if (!onCaller) HIP_TRY(hipEventRecord(d->sideDone[i], cs));
    }
    for (int i = 0; i + 1 < nClasses; i++)  // join: the caller's stream continues when every class is done
        HIP_TRY(hipStreamWaitEvent(st, d->sideDone[i], 0));
    HIP_TRY(hipEventRecord(d->evStop, st));
    d->lastStream = st;
    ran_set(d, true);
    return CPECAN_OK;
}

extern "C" int cpk_device_download(CpkDevice *d, int32_t *counts, int32_t *segStarts, int32_t *segCounts, double *expect,
                                   double *kernelMs, double *d2hMs) {
    CPK_ON_DEVICE(d->device);
    if (!d->ran) {
        cpk_set_error("download before run");
        return CPECAN_ESTATE;
    }
    // the batch's own stop event, not the caller's stream: that stream may already hold the next batch's launches
    const bool trace = getenv("CPECAN_TRACE_HOST") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventSynchronize(d->evStop));
    if (trace) fprintf(stderr, "cpecan download: waited %.1f ms for the sweep\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->evStart, d->evStop));
    if (kernelMs) *kernelMs = d->kernelMsAccum + ms;  // every launch of the batch (an overflow re-run included)
    hipStream_t io = d->io;
    HIP_TRY(hipEventRecord(d->evA, io));
    if (d->dProgress) {  // a fused launch reports a traceback whose forward values never came (it waits a bounded time)
        int err = 0;
        HIP_TRY(hipMemcpyAsync(&err, d->dProgress + d->geo.nRegions, sizeof(int), hipMemcpyDeviceToHost, io));
        HIP_TRY(hipStreamSynchronize(io));
        if (err) {
            // An item gave up waiting for its region's forward values (a bounded poll).  The rings of the class are whole:
            // run it again as two launches -- all forward sweeps, then all items -- which needs no hand-off inside a launch.
            bool any = false;
            for (LaunchClass &c : d->classes) {
                if (!c.fused()) continue;
                any = true;
                unfuse(c);
            }
            if (!any || d->fusedRetried) {
                cpk_set_error("fused launch: a traceback item waited in vain for its region's forward sweep");
                return CPECAN_EHIP;
            }
            d->fusedRetried = true;
            if (int rc = cpk_device_rerun(d)) return rc;
            return cpk_device_download(d, counts, segStarts, segCounts, expect, kernelMs, d2hMs);
        }
    }
    // written by the sweeps straight into pinned host memory; complete with the stop event
    memcpy(counts, d->dCounts, sizeof(int32_t) * (size_t)d->nLists * d->geo.nRegions);
    memcpy(segStarts, d->dSegStarts, sizeof(int32_t) * (size_t)d->nLists * d->nSegs);
    memcpy(segCounts, d->dSegCounts, sizeof(int32_t) * (size_t)d->nLists * d->nSegs);
    HIP_TRY(hipEventRecord(d->evB, io));
    HIP_TRY(hipStreamSynchronize(io));
    HIP_TRY(hipEventElapsedTime(&ms, d->evA, d->evB));
    if (d2hMs) *d2hMs = ms;
    if (expect && d->geo.emit == kEmitForward) {  // [slot][nRegions]
        HIP_TRY(hipMemcpyAsync(expect, d->dForward, sizeof(double) * (size_t)d->activeModels * d->geo.nRegions, hipMemcpyDeviceToHost, io));
        HIP_TRY(hipStreamSynchronize(io));
    }
    if (expect && d->geo.emit == CPECAN_EMIT_EXPECT && d->dSlots) {
        // [slot][106]: per slot, the partials of every class's waves in class and wave order, as below for a plain batch
        std::vector<double> part((size_t)d->expectDoubles);
        HIP_TRY(hipMemcpyAsync(part.data(), d->dExpect, sizeof(double) * part.size(), hipMemcpyDeviceToHost, io));
        HIP_TRY(hipStreamSynchronize(io));
        for (int s = 0; s < d->activeModels; s++) {
            double *sum = expect + (size_t)s * 106;
            for (int i = 0; i < 106; i++) sum[i] = 0.0;
            for (const LaunchClass &c : d->classes) {
                const int64_t nW = (int64_t)c.wavesWith(d->activeModels) * (c.threads / CPK_WAVE);
                const double *base = part.data() + c.oExpect + (size_t)s * nW * 128;
                for (int64_t w = 0; w < nW; w++)
                    for (int i = 0; i < 106; i++) sum[i] += base[(size_t)w * 128 + i];
            }
        }
    } else
    if (expect && d->geo.emit == CPECAN_EMIT_EXPECT) {
        // sum the per-wave partials (every launched wave wrote its 106 values, zeros included)
        const int nWaves = d->totalWaves;
        std::vector<double> part((size_t)nWaves * 128);
        HIP_TRY(hipMemcpyAsync(part.data(), d->dExpect, sizeof(double) * part.size(), hipMemcpyDeviceToHost, io));
        HIP_TRY(hipStreamSynchronize(io));
        for (int i = 0; i < 106; i++) expect[i] = 0.0;
        for (int w = 0; w < nWaves; w++)
            for (int i = 0; i < 106; i++) expect[i] += part[(size_t)w * 128 + i];
    }
    return CPECAN_OK;
}

extern "C" int cpk_device_gather(CpkDevice *d, const CpkChunk *chunks, int64_t nChunks, int64_t total) {
    CPK_ON_DEVICE(d->device);
    if (nChunks <= 0 || total <= 0) return CPECAN_OK;
    if (nChunks > d->chunkCap || total > d->compactCap) batch_quiesce(d);  // before blocks are recycled
    if (nChunks > d->chunkCap) {
        cache_free(d->device, d->dChunks, d->chunkBytes);
        d->dChunks = nullptr;
        d->chunkBytes = sizeof(CpkChunk) * (size_t)nChunks;
        HIP_TRY(cache_alloc(d->device, (void **)&d->dChunks, d->chunkBytes));
        d->chunkCap = nChunks;
    }
    if (total > d->compactCap) {
        cache_free(d->device, d->dCompact, d->compactBytes);
        d->dCompact = nullptr;
        d->compactBytes = sizeof(int32_t) * 3 * (size_t)total;
        HIP_TRY(cache_alloc(d->device, (void **)&d->dCompact, d->compactBytes));
        d->compactCap = total;
    }
    // the caller (cpecan_batch_download) has waited for the sweep; the chunk array is the caller's until the copy is done
    HIP_TRY(hipMemcpyAsync(d->dChunks, chunks, sizeof(CpkChunk) * (size_t)nChunks, hipMemcpyHostToDevice, d->io));
    const int64_t blocks = nChunks < 16384 ? nChunks : 16384;
    hipLaunchKernelGGL(cpecan_gather_lists, dim3((unsigned)blocks), dim3(256), 0, d->io, d->dChunks, nChunks, d->dTriples,
                       d->dCompact);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d->io));
    return CPECAN_OK;
}

extern "C" int cpk_device_fetch(CpkDevice *d, int32_t *hostOut, int64_t total, double *d2hMs) {
    CPK_ON_DEVICE(d->device);
    if (total <= 0) return CPECAN_OK;
    HIP_TRY(hipEventRecord(d->evA, d->io));
    HIP_TRY(hipMemcpyAsync(hostOut, d->dCompact, sizeof(int32_t) * 3 * (size_t)total, hipMemcpyDeviceToHost, d->io));
    HIP_TRY(hipEventRecord(d->evB, d->io));
    HIP_TRY(hipStreamSynchronize(d->io));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->evA, d->evB));
    if (d2hMs) *d2hMs += ms;
    return CPECAN_OK;
}

// The consumers on a device-resident triple buffer.  Scratch lives for the duration of the call.
namespace {
struct PostScratch {  // device blocks of one consumer stage, on the current device, used on ONE stream
    std::vector<CachedBlock> blocks;
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    explicit PostScratch(hipStream_t st) : stream(st) {
        (void)hipGetDevice(&device);
        if (!stream) {  // lists given by the host (no batch): a stream of the call's own, never the null stream
            ownStream = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
            if (!ownStream) stream = nullptr;
        }
    }
    ~PostScratch() {
        if (!blocks.empty()) (void)hipStreamSynchronize(stream);  // the stage's kernels are done with them
        for (const CachedBlock &b : blocks) cache_free(device, b.ptr, b.bytes);
        if (ownStream) (void)hipStreamDestroy(stream);
    }
    template <typename T>
    int alloc(T **out, size_t count) {
        void *p = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (cache_alloc(device, &p, bytes) != hipSuccess) {
            cpk_set_error("out of device memory in the list consumers");
            return CPECAN_ENOMEM;
        }
        blocks.push_back({p, bytes});
        *out = static_cast<T *>(p);
        return CPECAN_OK;
    }
};
}  // namespace

static int post_core(PostScratch &sc, int32_t *dTriples, const CpkPostJob *job) {
    const int64_t nP = job->nProblems;
    if (nP <= 0) return CPECAN_OK;
    hipStream_t st = sc.stream;
    CpkPostProblem *dProblems = nullptr;
    double *dScores = nullptr;
    int32_t *dCounts = nullptr;
    if (int rc = sc.alloc(&dProblems, (size_t)nP)) return rc;
    if (int rc = sc.alloc(&dScores, (size_t)nP * kPostScores)) return rc;
    if (int rc = sc.alloc(&dCounts, (size_t)nP * 2)) return rc;
    HIP_TRY(hipMemcpyAsync(dProblems, job->problems, sizeof(CpkPostProblem) * (size_t)nP, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dScores, 0, sizeof(double) * (size_t)nP * kPostScores, st));
    HIP_TRY(hipMemsetAsync(dCounts, 0, sizeof(int32_t) * (size_t)nP * 2, st));
    {
        int32_t *dMass = nullptr;
        const bool rw = (job->flags & kPostReweight) != 0;
        if (int rc = sc.alloc(&dMass, rw ? (size_t)job->seqSlots : 1)) return rc;
        hipLaunchKernelGGL(cpecan_post_reweight, dim3((unsigned)nP), dim3(256), 0, st, dProblems, dTriples, dMass,
                           job->gapGamma, rw ? 1 : 0, dScores);
        HIP_TRY(hipGetLastError());
    }
    int32_t *dMea = nullptr, *dShift = nullptr;
    uint8_t *dChars = nullptr;
    const unsigned laneBlocks = (unsigned)((nP + 63) / 64);
    if (job->flags & (kPostMea | kPostLeftShift | kPostOrdered))
        if (int rc = sc.alloc(&dMea, (size_t)job->meaCap * 3)) return rc;
    if (job->chars) {
        if (int rc = sc.alloc(&dChars, (size_t)(job->nChars > 0 ? job->nChars : 1))) return rc;
        if (job->nChars > 0) HIP_TRY(hipMemcpyAsync(dChars, job->chars, (size_t)job->nChars, hipMemcpyHostToDevice, st));
    }
    if (job->flags & kPostOrdered) {
        int32_t *dSeq = nullptr, *dPrev = nullptr, *dNext = nullptr;
        double *dBest = nullptr;
        uint8_t *dChosen = nullptr;
        if (int rc = sc.alloc(&dSeq, (size_t)(job->seqSlots > 0 ? job->seqSlots : 1))) return rc;
        if (int rc = sc.alloc(&dBest, (size_t)job->chainSlots)) return rc;
        if (int rc = sc.alloc(&dPrev, (size_t)job->chainSlots)) return rc;
        if (int rc = sc.alloc(&dNext, (size_t)job->chainSlots)) return rc;
        if (int rc = sc.alloc(&dChosen, (size_t)job->chainSlots)) return rc;
        const char *lanesEnv = getenv("CPECAN_POST_LANES");  // 1: one lane per problem (the form of rounds 1-2; tests, A/B runs)
        if (lanesEnv && atoi(lanesEnv) != 0) {
            hipLaunchKernelGGL(cpecan_post_ordered, dim3(laneBlocks), dim3(64), 0, st, dProblems, nP, dTriples, dSeq,
                               dBest, dPrev, dNext, dChosen, job->matchGamma, dMea, dCounts);
        } else {
            // one wave per problem: the pairs in column order take four more words a pair
            int32_t *dSortX = nullptr, *dSortY = nullptr;
            double *dSortW = nullptr;
            if (int rc = sc.alloc(&dSortX, (size_t)job->chainSlots)) return rc;
            if (int rc = sc.alloc(&dSortY, (size_t)job->chainSlots)) return rc;
            if (int rc = sc.alloc(&dSortW, (size_t)job->chainSlots)) return rc;
            hipLaunchKernelGGL(cpecan_post_ordered_wave, dim3((unsigned)nP), dim3(64), 0, st, dProblems, dTriples, dSeq, dBest,
                               dPrev, dNext, dSortX, dSortY, dSortW, dChosen, job->matchGamma, dMea, dCounts);
        }
        HIP_TRY(hipGetLastError());
    }
    if ((job->flags & kPostOrdered) || dChars) {
        const int fromOut = (job->flags & kPostOrdered) ? 1 : 0;
        hipLaunchKernelGGL(cpecan_post_list_scores, dim3((unsigned)nP), dim3(256), 0, st, dProblems, dTriples, dMea,
                           dCounts, fromOut, fromOut, dChars, dScores);
        HIP_TRY(hipGetLastError());
    }
    if (job->flags & kPostMea) {
        long long *dCum = nullptr;
        double *dBest = nullptr;
        int32_t *dPrev = nullptr;
        uint8_t *dRecord = nullptr;
        if (int rc = sc.alloc(&dCum, (size_t)job->seqSlots)) return rc;
        if (int rc = sc.alloc(&dBest, (size_t)job->chainSlots)) return rc;
        if (int rc = sc.alloc(&dPrev, (size_t)job->chainSlots)) return rc;
        if (int rc = sc.alloc(&dRecord, (size_t)job->chainSlots)) return rc;
        const char *lanesEnv = getenv("CPECAN_POST_LANES");  // 1: one lane per problem (the form of rounds 1-2; tests, A/B runs)
        if (lanesEnv && atoi(lanesEnv) != 0) {
            hipLaunchKernelGGL(cpecan_post_mea, dim3(laneBlocks), dim3(64), 0, st, dProblems, nP, dTriples, dCum, dBest,
                               dPrev, dRecord, (float)job->gapGamma, dMea, dCounts, dScores);
        } else {
            long long *dG = nullptr, *dH = nullptr, *dT = nullptr;  // the gap masses around every pair (cpecan_post_mea_wave)
            if (int rc = sc.alloc(&dG, (size_t)job->chainSlots)) return rc;
            if (int rc = sc.alloc(&dH, (size_t)job->chainSlots)) return rc;
            if (int rc = sc.alloc(&dT, (size_t)job->chainSlots)) return rc;
            hipLaunchKernelGGL(cpecan_post_mea_wave, dim3((unsigned)nP), dim3(64), 0, st, dProblems, dTriples, dCum, dBest, dPrev,
                               dRecord, dG, dH, dT, (float)job->gapGamma, dMea, dCounts, dScores);
        }
        HIP_TRY(hipGetLastError());
    } else if (job->flags & kPostLeftShift) {
        hipLaunchKernelGGL(cpecan_post_copy_chain, dim3((unsigned)nP), dim3(256), 0, st, dProblems, dTriples, dMea,
                           dCounts);
        HIP_TRY(hipGetLastError());
    }
    if (job->flags & kPostLeftShift) {
        if (!dChars) {
            cpk_set_error("left shift needs the raw sequences");
            return CPECAN_EINVAL;
        }
        if (int rc = sc.alloc(&dShift, (size_t)job->shiftCap * 3)) return rc;
        hipLaunchKernelGGL(cpecan_post_left_shift, dim3(laneBlocks), dim3(64), 0, st, dProblems, nP, dMea, dChars,
                           dShift, dCounts);
        HIP_TRY(hipGetLastError());
    }
    // the quintuple stage of the sets layer: behind every consumer, on list 0 as they left it
    int32_t *dQuints = nullptr;
    long long *dSums = nullptr;
    hipEvent_t evStage[2] = {nullptr, nullptr};
    struct StageEvents {  // (released on every way out)
        hipEvent_t *ev;
        ~StageEvents() {
            for (int k = 0; k < 2; k++)
                if (ev[k]) (void)hipEventDestroy(ev[k]);
        }
    } stageEvents{evStage};
    if (job->names) {
        int32_t *dNames = nullptr;
        if (int rc = sc.alloc(&dNames, (size_t)nP * 2)) return rc;
        if (int rc = sc.alloc(&dQuints, (size_t)job->meaCap * 5)) return rc;
        if (int rc = sc.alloc(&dSums, (size_t)nP)) return rc;
        HIP_TRY(hipMemcpyAsync(dNames, job->names, sizeof(int32_t) * 2 * (size_t)nP, hipMemcpyHostToDevice, st));
        if (job->stageMs) {
            HIP_TRY(hipEventCreate(&evStage[0]));
            HIP_TRY(hipEventCreate(&evStage[1]));
            HIP_TRY(hipEventRecord(evStage[0], st));
        }
        hipLaunchKernelGGL(cpecan_post_quintuples, dim3((unsigned)nP), dim3(256), 0, st, dProblems, dTriples, dNames, dQuints,
                           dSums);
        HIP_TRY(hipGetLastError());
        if (job->stageMs) HIP_TRY(hipEventRecord(evStage[1], st));
        if (job->quints && job->meaCap > 0)
            HIP_TRY(hipMemcpyAsync(job->quints, dQuints, sizeof(int32_t) * 5 * (size_t)job->meaCap, hipMemcpyDeviceToHost, st));
        if (job->sums) HIP_TRY(hipMemcpyAsync(job->sums, dSums, sizeof(long long) * (size_t)nP, hipMemcpyDeviceToHost, st));
    }
    // the next-runs stage: the ordered alignment as the anchor runs of the next E-step; only counts and runs leave the device
    hipEvent_t evNext[2] = {nullptr, nullptr};
    StageEvents nextEvents{evNext};
    if (job->nextRuns) {
        if (!(job->flags & kPostOrdered) || !dChars || !dMea || !job->runCounts || !job->runOffsets || !job->runsOut) {
            cpk_set_error("the next-runs stage needs the ordered alignment and the raw sequences");
            return CPECAN_EINVAL;
        }
        int32_t *dNext = nullptr, *dRunCounts = nullptr;
        int4 *dRuns = nullptr, *dPacked = nullptr;
        int64_t *dPackedOff = nullptr;
        if (int rc = sc.alloc(&dNext, (size_t)job->nextSlots)) return rc;
        if (int rc = sc.alloc(&dRunCounts, (size_t)nP)) return rc;
        if (int rc = sc.alloc(&dRuns, (size_t)job->meaCap)) return rc;
        if (job->nextMs) {
            HIP_TRY(hipEventCreate(&evNext[0]));
            HIP_TRY(hipEventCreate(&evNext[1]));
            HIP_TRY(hipEventRecord(evNext[0], st));
        }
        hipLaunchKernelGGL(cpecan_post_next_runs, dim3((unsigned)nP), dim3(64), 0, st, dProblems, dMea, dCounts, dChars, dNext,
                           job->nextTrim, job->nextExpansion, dRuns, dRunCounts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(job->runCounts, dRunCounts, sizeof(int32_t) * (size_t)nP, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int64_t total = 0;
        for (int64_t i = 0; i < nP; i++) {
            if (job->runCounts[i] < 0 || job->runCounts[i] > job->problems[i].n[0]) {
                cpk_set_error("internal: the next-runs stage counted %d runs for the %d pairs of problem %lld", job->runCounts[i],
                              job->problems[i].n[0], (long long)i);
                return CPECAN_ESTATE;
            }
            job->runOffsets[i] = total;
            total += job->runCounts[i];
        }
        job->runOffsets[nP] = total;
        int32_t *hostRuns = static_cast<int32_t *>(cpk_host_alloc(sizeof(int32_t) * 4 * (size_t)(total ? total : 1)));
        if (!hostRuns) return CPECAN_ENOMEM;
        *job->runsOut = hostRuns;
        if (total > 0) {
            if (int rc = sc.alloc(&dPackedOff, (size_t)nP)) return rc;
            if (int rc = sc.alloc(&dPacked, (size_t)total)) return rc;
            HIP_TRY(hipMemcpyAsync(dPackedOff, job->runOffsets, sizeof(int64_t) * (size_t)nP, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(cpecan_post_pack_runs, dim3((unsigned)nP), dim3(64), 0, st, dProblems, dRuns, dRunCounts, dPackedOff,
                               dPacked);
            HIP_TRY(hipGetLastError());
        }
        if (job->nextMs) HIP_TRY(hipEventRecord(evNext[1], st));
        if (total > 0) HIP_TRY(hipMemcpyAsync(hostRuns, dPacked, sizeof(int4) * (size_t)total, hipMemcpyDeviceToHost, st));
    }
    if (job->scores)
        HIP_TRY(hipMemcpyAsync(job->scores, dScores, sizeof(double) * (size_t)nP * kPostScores, hipMemcpyDeviceToHost, st));
    if (job->counts) HIP_TRY(hipMemcpyAsync(job->counts, dCounts, sizeof(int32_t) * (size_t)nP * 2, hipMemcpyDeviceToHost, st));
    if (job->mea && dMea)
        HIP_TRY(hipMemcpyAsync(job->mea, dMea, sizeof(int32_t) * 3 * (size_t)job->meaCap, hipMemcpyDeviceToHost, st));
    if (job->shift && dShift)
        HIP_TRY(hipMemcpyAsync(job->shift, dShift, sizeof(int32_t) * 3 * (size_t)job->shiftCap, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (job->names && job->stageMs) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, evStage[0], evStage[1]));
        *job->stageMs = ms;
    }
    if (job->nextRuns && job->nextMs) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, evNext[0], evNext[1]));
        *job->nextMs = ms;
    }
    return CPECAN_OK;
}

extern "C" int cpk_device_post(CpkDevice *d, const CpkPostJob *job) {
    CPK_ON_DEVICE(d->device);
    if (!d->dCompact && job->nProblems > 0) {
        // every list is empty: the consumers still need a valid base pointer
        d->compactBytes = sizeof(int32_t) * 3;
        HIP_TRY(cache_alloc(d->device, (void **)&d->dCompact, d->compactBytes));
        d->compactCap = 1;
    }
    PostScratch sc(d->io);
    return post_core(sc, d->dCompact, job);
}

extern "C" int cpk_device_band_edge(CpkDevice *d, int64_t nChunks0, const int32_t *chunkRegion, const int32_t *chunkProblem,
                                    int64_t nProblems, cpecan_band_edge *out) {
    CPK_ON_DEVICE(d->device);
    memset(out, 0, sizeof(cpecan_band_edge) * (size_t)nProblems);
    if (nChunks0 <= 0 || nProblems <= 0) return CPECAN_OK;  // no pair was emitted
    if (nChunks0 > d->chunkCap || !d->dChunks || !d->dCompact || !d->dDiags) {
        cpk_set_error("band edge statistic without a gathered list");
        return CPECAN_ESTATE;
    }
    PostScratch sc(d->io);
    int32_t *dRegion = nullptr, *dProblem = nullptr;
    cpecan_band_edge *dOut = nullptr;
    if (int rc = sc.alloc(&dRegion, (size_t)nChunks0)) return rc;
    if (int rc = sc.alloc(&dProblem, (size_t)nChunks0)) return rc;
    if (int rc = sc.alloc(&dOut, (size_t)nProblems)) return rc;
    HIP_TRY(hipMemcpyAsync(dRegion, chunkRegion, sizeof(int32_t) * (size_t)nChunks0, hipMemcpyHostToDevice, d->io));
    HIP_TRY(hipMemcpyAsync(dProblem, chunkProblem, sizeof(int32_t) * (size_t)nChunks0, hipMemcpyHostToDevice, d->io));
    HIP_TRY(hipMemsetAsync(dOut, 0, sizeof(cpecan_band_edge) * (size_t)nProblems, d->io));
    const int64_t blocks = nChunks0 < 65536 ? nChunks0 : 65536;
    hipLaunchKernelGGL(cpecan_post_band_edge, dim3((unsigned)blocks), dim3(CPK_WAVE), 0, d->io, d->dChunks, dRegion, dProblem,
                       nChunks0, d->dRegions, d->dDiags, d->dCompact, dOut);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dOut, sizeof(cpecan_band_edge) * (size_t)nProblems, hipMemcpyDeviceToHost, d->io));
    HIP_TRY(hipStreamSynchronize(d->io));
    return CPECAN_OK;
}

extern "C" int cpk_post_lists(int device, int32_t *triples, int64_t total, const CpkPostJob *job) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    CPK_ON_DEVICE(device);
    PostScratch sc(nullptr);
    if (!sc.stream) {
        cpk_set_error("hipStreamCreate failed in the list consumers");
        return CPECAN_EHIP;
    }
    int32_t *dTriples = nullptr;
    if (int rc = sc.alloc(&dTriples, (size_t)(total > 0 ? total : 1) * 3)) return rc;
    if (total > 0)
        HIP_TRY(hipMemcpyAsync(dTriples, triples, sizeof(int32_t) * 3 * (size_t)total, hipMemcpyHostToDevice, sc.stream));
    if (int rc = post_core(sc, dTriples, job)) return rc;
    if (total > 0) {
        HIP_TRY(hipMemcpyAsync(triples, dTriples, sizeof(int32_t) * 3 * (size_t)total, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(hipStreamSynchronize(sc.stream));
    }
    return CPECAN_OK;
}

extern "C" int cpk_device_debug_fetch(CpkDevice *d, double *fb, int64_t cells, double *totals, int64_t diags) {
    CPK_ON_DEVICE(d->device);
    batch_quiesce(d);
    if (!d->geo.debug || !d->dDbgFb) {
        cpk_set_error("debug buffers were not enabled before upload");
        return CPECAN_ESTATE;
    }
    if (cells > d->dbgCells || diags > d->dbgDiags) {
        cpk_set_error("debug fetch larger than the debug buffers");
        return CPECAN_EINVAL;
    }
    HIP_TRY(hipMemcpy(fb, d->dDbgFb, sizeof(double) * (size_t)cells, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(totals, d->dDbgTotals, sizeof(double) * (size_t)diags, hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

// The table of one region as the builders of cpk_table_gather.inl left it, for tests: read-only, no launch.  The build is
// ordered on the batch's own stream (cpk_device_upload), so waiting for that stream is enough whether the batch has run.
extern "C" int cpk_device_table_fetch(CpkDevice *d, const CpkRegion *rg, int dynamic, CpkDiag *diags, int32_t *dpos, int *hasPos,
                                      int64_t *ringDoubles) {
    CPK_ON_DEVICE(d->device);
    if (!d->dDiags) {
        cpk_set_error("table fetch before upload");
        return CPECAN_ESTATE;
    }
    const int64_t n = (int64_t)rg->lX + rg->lY + 1;
    if (rg->diagOff < 0 || rg->diagOff + n > d->nDiags) {
        cpk_set_error("table fetch: region outside the batch's table");
        return CPECAN_EINVAL;
    }
    *hasPos = d->dDiagPos && !dynamic;  // (the builders return in front of the position chains otherwise)
    *ringDoubles = rg->split ? split_ring_doubles(*rg, d->geo.nStates) : 0;
    if (!diags) return CPECAN_OK;
    HIP_TRY(hipStreamSynchronize(d->io));
    HIP_TRY(hipMemcpy(diags, d->dDiags + rg->diagOff, sizeof(CpkDiag) * (size_t)n, hipMemcpyDeviceToHost));
    if (*hasPos && dpos) HIP_TRY(hipMemcpy(dpos, d->dDiagPos + rg->diagOff, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

// The reference's unit-test primitives (cpk_cells.inl): a few hundred cells at most, one lane, blocking copies.
extern "C" int cpk_ref_cells(int device, const CpkModel *model, int mode, const CpkCellOp *ops, int64_t n, double *buf,
                             int64_t nDoubles, double total) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    if (n <= 0 || nDoubles <= 0) return CPECAN_OK;
    CPK_ON_DEVICE(device);
    void *dOps = nullptr, *dBuf = nullptr;
    const size_t opBytes = sizeof(CpkCellOp) * (size_t)n, bufBytes = sizeof(double) * (size_t)nDoubles;
    HIP_TRY(cache_alloc(device, &dOps, opBytes));
    if (hipError_t e = cache_alloc(device, &dBuf, bufBytes); e != hipSuccess) {
        cache_free(device, dOps, opBytes);
        HIP_TRY(e);
    }
    int rc = CPECAN_OK;
    hipError_t e = hipMemcpy(dOps, ops, opBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dBuf, buf, bufBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpecan_ref_cells, dim3(1), dim3(CPK_WAVE), 0, nullptr, *model, mode, (const CpkCellOp *)dOps, (int)n,
                           (double *)dBuf, total);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(buf, dBuf, bufBytes, hipMemcpyDeviceToHost);  // waits for the kernel (null stream)
    if (e != hipSuccess) {
        cpk_set_error("cpk_ref_cells: %s", hipGetErrorString(e));
        rc = CPECAN_EHIP;
    }
    cache_free(device, dOps, opBytes);
    cache_free(device, dBuf, bufBytes);
    return rc;
}

// Dense rows (cpk_dense.inl): device bytes of a job, and the job itself -- blocking copies around two launches on the null stream.
extern "C" int64_t cpk_dense_device_bytes(const CpkDenseJob *j, int S) {
    return (int64_t)sizeof(double) * ((2 * j->totalCells + j->sideCells) * S + j->nDiags) + (int64_t)sizeof(CpkDenseDiag) * j->nDiags +
           (int64_t)sizeof(CpkDenseProblem) * j->nProblems + (int64_t)sizeof(CpkDenseSeg) * j->nSegs + j->nSymbolBytes;
}
extern "C" int cpk_dense_run(int device, const CpkModel *model, const CpkDenseJob *j, double *kernelMs) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    if (kernelMs) *kernelMs = 0.0;
    if (j->nDiags <= 0) return CPECAN_OK;  // nothing but problems without rows
    CPK_ON_DEVICE(device);
    const int S = model->nStates;
    const size_t cellBytes = sizeof(double) * (size_t)j->totalCells * S, sideBytes = sizeof(double) * (size_t)j->sideCells * S;
    const size_t bytes[8] = {sizeof(CpkDenseProblem) * (size_t)j->nProblems, sizeof(CpkDenseDiag) * (size_t)j->nDiags,
                             sizeof(CpkDenseSeg) * (size_t)j->nSegs, (size_t)j->nSymbolBytes, cellBytes, cellBytes, sideBytes,
                             sizeof(double) * (size_t)j->nDiags};
    const void *src[4] = {j->problems, j->diags, j->segs, j->symbols};
    void *dst[4] = {j->F, j->B, j->side, j->totals};
    void *dp[8] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 8 && e == hipSuccess; i++) e = cache_alloc(device, &dp[i], bytes[i]);
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipMemcpy(dp[i], src[i], bytes[i], hipMemcpyHostToDevice);
    hipEvent_t ev[2] = {};
    if (e == hipSuccess) e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) {
        const DenseArgs a = {(const CpkDenseProblem *)dp[0], (const CpkDenseDiag *)dp[1], (const CpkDenseSeg *)dp[2], (const uint8_t *)dp[3],
                             (double *)dp[4], (double *)dp[5], (double *)dp[6], (double *)dp[7]};
        (void)hipEventRecord(ev[0], nullptr);
        hipLaunchKernelGGL(cpecan_dense_forward, dim3((unsigned)j->nProblems), dim3(CPK_WAVE), 0, nullptr, *model, a);
        hipLaunchKernelGGL(cpecan_dense_backward, dim3((unsigned)j->nSegs), dim3(CPK_WAVE), 0, nullptr, *model, a);
        e = hipGetLastError();
        (void)hipEventRecord(ev[1], nullptr);
    }
    for (int i = 0; i < 4 && e == hipSuccess; i++)  // waits for the kernels (null stream)
        if (bytes[4 + i]) e = hipMemcpy(dst[i], dp[4 + i], bytes[4 + i], hipMemcpyDeviceToHost);
    if (e == hipSuccess && kernelMs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *kernelMs = ms;
    }
    for (int i = 0; i < 2; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < 8; i++) cache_free(device, dp[i], bytes[i]);
    if (e != hipSuccess) {
        cpk_set_error("cpk_dense_run: %s", hipGetErrorString(e));
        return CPECAN_EHIP;
    }
    return CPECAN_OK;
}

// Viterbi decoding (cpk_viterbi.inl): one launch of a cpecan_viterbi run -- blocking copies around the sweep (its LDS-form and
// its global-form regions) and the traceback on the null stream.  The caller has checked that a device exists.
extern "C" int cpk_viterbi_launch(int device, const CpkModel *model, const CpkVitJob *j, double *sweepMs, double *tracebackMs) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    if (j->nRegions <= 0) return CPECAN_OK;
    CPK_ON_DEVICE(device);
    const int S = model->nStates;
    const size_t bytes[8] = {sizeof(CpkVitRegion) * (size_t)j->nRegions, sizeof(CpkVitDiag) * (size_t)j->nDiags, (size_t)j->nSymbolBytes,
                             sizeof(int32_t) * (size_t)j->nRegions, (size_t)j->nPtrBytes, sizeof(double) * (size_t)j->nRollDoubles,
                             sizeof(CpkVitOut) * (size_t)j->nRegions, sizeof(int32_t) * 2 * (size_t)j->nOpPairs};
    const void *src[4] = {j->regions, j->diags, j->symbols, j->order};
    void *dp[8] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 8 && e == hipSuccess; i++) e = cache_alloc(device, &dp[i], bytes[i] ? bytes[i] : 8);
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipMemcpy(dp[i], src[i], bytes[i], hipMemcpyHostToDevice);
    hipEvent_t ev[3] = {};
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) {
        VitArgs a = {(const CpkVitRegion *)dp[0], (const CpkVitDiag *)dp[1], (const uint8_t *)dp[2], (const int32_t *)dp[3],
                     (uint8_t *)dp[4], (double *)dp[5], (CpkVitOut *)dp[6], (int32_t *)dp[7], j->ldsMaxWidth};
        const size_t ldsRows = sizeof(double) * (kVitEm + (size_t)3 * S * (size_t)j->ldsMaxWidth), ldsNone = sizeof(double) * kVitEm;
        (void)hipEventRecord(ev[0], nullptr);
        if (j->nLds > 0) hipLaunchKernelGGL(cpecan_viterbi_sweep<true>, dim3((unsigned)j->nLds), dim3(CPK_WAVE), ldsRows, nullptr, *model, a);
        if (j->nRegions > j->nLds) {
            VitArgs g = a;
            g.order = a.order + j->nLds;
            hipLaunchKernelGGL(cpecan_viterbi_sweep<false>, dim3((unsigned)(j->nRegions - j->nLds)), dim3(CPK_WAVE), ldsNone, nullptr, *model, g);
        }
        (void)hipEventRecord(ev[1], nullptr);
        hipLaunchKernelGGL(cpecan_viterbi_traceback, dim3((unsigned)j->nRegions), dim3(CPK_WAVE), 0, nullptr, S, a);
        e = hipGetLastError();
        (void)hipEventRecord(ev[2], nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(j->out, dp[6], bytes[6], hipMemcpyDeviceToHost);  // waits for the kernels (null stream)
    if (e == hipSuccess && bytes[7]) e = hipMemcpy(j->ops, dp[7], bytes[7], hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        float ms = 0.f;
        if (sweepMs && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *sweepMs = ms;
        if (tracebackMs && hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) *tracebackMs = ms;
    }
    for (int i = 0; i < 3; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < 8; i++) cache_free(device, dp[i], bytes[i] ? bytes[i] : 8);
    if (e != hipSuccess) {
        cpk_set_error("cpk_viterbi_launch: %s", hipGetErrorString(e));
        return CPECAN_EHIP;
    }
    return CPECAN_OK;
}

// The resident form of a cpecan_viterbi run (cpecan_viterbi_run_counts): every launch's inputs on the device, one scratch, the
// run's bins.  Everything on the null stream; the copy of a launch's out records home waits for its kernels.
struct CpkVitResident {
    int device = 0, nStates = 0, nBins = 0;
    struct Launch {
        void *d[4] = {};  // regions, diags, symbols, order
        size_t bytes[4] = {};
        int64_t nRegions = 0, nLds = 0, nPtrBytes = 0, nRollDoubles = 0, nOpPairs = 0;
        int32_t ldsMaxWidth = 0;
    };
    std::vector<Launch> launches;
    void *scratch[5] = {};  // pointer bytes, rolling rows, out records, op slots, count slabs
    size_t scratchBytes[5] = {};
    int64_t *bins = nullptr;
    hipEvent_t ev[5] = {};
};

extern "C" void cpk_viterbi_resident_destroy(CpkVitResident *r) {
    if (!r) return;
    DeviceGuard guard(r->device);
    (void)hipDeviceSynchronize();
    for (auto &l : r->launches)
        for (int i = 0; i < 4; i++) cache_free(r->device, l.d[i], l.bytes[i]);
    for (int i = 0; i < 5; i++) cache_free(r->device, r->scratch[i], r->scratchBytes[i]);
    cache_free(r->device, r->bins, sizeof(int64_t) * CPK_VIT_MAX_BINS);
    for (int i = 0; i < 5; i++)
        if (r->ev[i]) (void)hipEventDestroy(r->ev[i]);
    delete r;
}

extern "C" int cpk_viterbi_resident_create(CpkVitResident **out, int device, int nStates, int64_t nLaunches, int64_t inputBytes,
                                           int64_t scratchBytes) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    CPK_ON_DEVICE(device);
    size_t freeBytes = 0, totalBytes = 0;
    HIP_TRY(hipMemGetInfo(&freeBytes, &totalBytes));
    if ((size_t)inputBytes + (size_t)scratchBytes > freeBytes + cache_bytes(device)) {
        cpk_set_error("cpecan_viterbi_run_counts: the resident inputs need %lld bytes beside %lld bytes of scratch, the device has %lld free",
                      (long long)inputBytes, (long long)scratchBytes, (long long)(freeBytes + cache_bytes(device)));
        return CPECAN_ENOMEM;
    }
    CpkVitResident *r = new CpkVitResident;
    r->device = device;
    r->nStates = nStates;
    r->nBins = nStates * nStates + nStates * 16;
    r->launches.resize((size_t)nLaunches);
    hipError_t e = cache_alloc(device, (void **)&r->bins, sizeof(int64_t) * CPK_VIT_MAX_BINS);
    for (int i = 0; i < 5 && e == hipSuccess; i++) e = hipEventCreate(&r->ev[i]);
    if (e != hipSuccess) {
        cpk_set_error("cpk_viterbi_resident_create: %s", hipGetErrorString(e));
        cpk_viterbi_resident_destroy(r);
        return CPECAN_EHIP;
    }
    *out = r;
    return CPECAN_OK;
}

extern "C" int cpk_viterbi_resident_upload(CpkVitResident *r, int64_t launch, const CpkVitJob *j) {
    if (launch < 0 || launch >= (int64_t)r->launches.size() || r->launches[(size_t)launch].d[0]) return CPECAN_EINVAL;
    CPK_ON_DEVICE(r->device);
    CpkVitResident::Launch &l = r->launches[(size_t)launch];
    const size_t bytes[4] = {sizeof(CpkVitRegion) * (size_t)j->nRegions, sizeof(CpkVitDiag) * (size_t)j->nDiags, (size_t)j->nSymbolBytes,
                             sizeof(int32_t) * (size_t)j->nRegions};
    const void *src[4] = {j->regions, j->diags, j->symbols, j->order};
    for (int i = 0; i < 4; i++) {
        l.bytes[i] = bytes[i] ? bytes[i] : 8;
        HIP_TRY(cache_alloc(r->device, &l.d[i], l.bytes[i]));
        HIP_TRY(hipMemcpy(l.d[i], src[i], bytes[i], hipMemcpyHostToDevice));
    }
    l.nRegions = j->nRegions;
    l.nLds = j->nLds;
    l.nPtrBytes = j->nPtrBytes;
    l.nRollDoubles = j->nRollDoubles;
    l.nOpPairs = j->nOpPairs;
    l.ldsMaxWidth = j->ldsMaxWidth;
    return CPECAN_OK;
}

extern "C" int cpk_viterbi_resident_reserve(CpkVitResident *r) {
    CPK_ON_DEVICE(r->device);
    size_t need[5] = {8, 8, 8, 8, 8};
    for (const auto &l : r->launches) {
        const size_t b[5] = {(size_t)l.nPtrBytes, sizeof(double) * (size_t)l.nRollDoubles, sizeof(CpkVitOut) * (size_t)l.nRegions,
                             sizeof(int32_t) * 2 * (size_t)l.nOpPairs, sizeof(uint32_t) * (size_t)r->nBins * (size_t)l.nRegions};
        for (int i = 0; i < 5; i++)
            if (b[i] > need[i]) need[i] = b[i];
    }
    for (int i = 0; i < 5; i++) {
        if (r->scratch[i]) return CPECAN_ESTATE;
        r->scratchBytes[i] = need[i];
        HIP_TRY(cache_alloc(r->device, &r->scratch[i], need[i]));
    }
    return CPECAN_OK;
}

extern "C" int cpk_viterbi_resident_begin(CpkVitResident *r) {
    CPK_ON_DEVICE(r->device);
    HIP_TRY(hipMemsetAsync(r->bins, 0, sizeof(int64_t) * CPK_VIT_MAX_BINS, nullptr));
    return CPECAN_OK;
}

extern "C" int cpk_viterbi_resident_run(CpkVitResident *r, int64_t launch, const CpkModel *model, CpkVitOut *out, uint32_t *slabs,
                                        double ms[4]) {
    if (launch < 0 || launch >= (int64_t)r->launches.size() || !r->scratch[0] || model->nStates != r->nStates) return CPECAN_EINVAL;
    const CpkVitResident::Launch &l = r->launches[(size_t)launch];
    for (int i = 0; i < 4; i++) ms[i] = 0.0;
    if (l.nRegions <= 0) return CPECAN_OK;
    CPK_ON_DEVICE(r->device);
    const int S = r->nStates;
    VitArgs a = {(const CpkVitRegion *)l.d[0], (const CpkVitDiag *)l.d[1], (const uint8_t *)l.d[2], (const int32_t *)l.d[3],
                 (uint8_t *)r->scratch[0], (double *)r->scratch[1], (CpkVitOut *)r->scratch[2], (int32_t *)r->scratch[3], l.ldsMaxWidth};
    uint32_t *dSlabs = (uint32_t *)r->scratch[4];
    const size_t ldsRows = sizeof(double) * (kVitEm + (size_t)3 * S * (size_t)l.ldsMaxWidth), ldsNone = sizeof(double) * kVitEm;
    (void)hipEventRecord(r->ev[0], nullptr);
    if (l.nLds > 0) hipLaunchKernelGGL(cpecan_viterbi_sweep<true>, dim3((unsigned)l.nLds), dim3(CPK_WAVE), ldsRows, nullptr, *model, a);
    if (l.nRegions > l.nLds) {
        VitArgs g = a;
        g.order = a.order + l.nLds;
        hipLaunchKernelGGL(cpecan_viterbi_sweep<false>, dim3((unsigned)(l.nRegions - l.nLds)), dim3(CPK_WAVE), ldsNone, nullptr, *model, g);
    }
    (void)hipEventRecord(r->ev[1], nullptr);
    hipLaunchKernelGGL(cpecan_viterbi_traceback, dim3((unsigned)l.nRegions), dim3(CPK_WAVE), 0, nullptr, S, a);
    (void)hipEventRecord(r->ev[2], nullptr);
    hipLaunchKernelGGL(cpecan_viterbi_count, dim3((unsigned)l.nRegions), dim3(CPK_WAVE), 0, nullptr, S, a, dSlabs);
    (void)hipEventRecord(r->ev[3], nullptr);
    hipLaunchKernelGGL(cpecan_viterbi_count_reduce, dim3((unsigned)r->nBins), dim3(kVitReduceThreads), 0, nullptr, (const uint32_t *)dSlabs,
                       (int)l.nRegions, r->nBins, r->bins);
    hipError_t e = hipGetLastError();
    (void)hipEventRecord(r->ev[4], nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, r->scratch[2], sizeof(CpkVitOut) * (size_t)l.nRegions, hipMemcpyDeviceToHost);  // waits (null stream)
    if (e == hipSuccess && slabs)
        e = hipMemcpy(slabs, dSlabs, sizeof(uint32_t) * (size_t)r->nBins * (size_t)l.nRegions, hipMemcpyDeviceToHost);
    for (int i = 0; i < 4 && e == hipSuccess; i++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r->ev[i], r->ev[i + 1]) == hipSuccess) ms[i] = t;
    }
    if (e != hipSuccess) {
        cpk_set_error("cpk_viterbi_resident_run: %s", hipGetErrorString(e));
        return CPECAN_EHIP;
    }
    return CPECAN_OK;
}

extern "C" int cpk_viterbi_resident_bins(CpkVitResident *r, int64_t *bins) {
    CPK_ON_DEVICE(r->device);
    HIP_TRY(hipMemcpy(bins, r->bins, sizeof(int64_t) * (size_t)r->nBins, hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

extern "C" int64_t cpk_device_bytes(const CpkDevice *d) { return d->bytes; }
static int form_code(const KernelForm &f) {  // CPECAN_FORM_* of a class, from the form of its first launch
    return (f.mode == kModeFused ? CPECAN_FORM_FUSED : f.mode != kModeWhole ? CPECAN_FORM_SPLIT : CPECAN_FORM_WHOLE) | (f.abs ? CPECAN_FORM_ABS : 0);
}
extern "C" int cpk_device_form(const CpkDevice *d) { return d->classes.empty() ? CPECAN_FORM_WHOLE : form_code(d->classes.back().form); }
extern "C" int cpk_device_waves(const CpkDevice *d) { return d->totalWaves; }

// ------------------------------------------------------------------------------------------------
// The anchor finder (cpk_anchor.inl).  A context holds the packed symbols of one call; a pass runs steps 1-5 on a list of
// problems (the top level, then the gaps of the recursion).  The host sizes lists and launches; two small copies per pass
// come back in the middle (the hit counts size the HSP lists).
// ------------------------------------------------------------------------------------------------
struct CpkAnchorCtx {
    int device = 0;
    PostScratch *sc = nullptr;
    uint8_t *dSym = nullptr;
    int64_t nSym = 0;     // symbols the buffer holds: the packed bytes, then the area of the reverse complements
    int64_t nForward = 0; // the packed bytes
    hipEvent_t evA = nullptr, evB = nullptr;
};

static int anchor_pow2(int64_t v) {
    int64_t c = 1;
    while (c < v) c <<= 1;
    return (int)c;
}

extern "C" void cpk_anchor_close(CpkAnchorCtx *c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->evA) (void)hipEventDestroy(c->evA);
    if (c->evB) (void)hipEventDestroy(c->evB);
    delete c->sc;
    delete c;
}

extern "C" int cpk_anchor_open(CpkAnchorCtx **out, int device, const uint8_t *bytes, int64_t nBytes, int64_t nExtra) {
    const int nDev = cpk_device_count();
    if (nDev <= 0 || device < 0 || device >= nDev) {
        cpk_set_error("no usable HIP device (count=%d, requested=%d): the HIP path has no CPU fallback", nDev, device);
        return CPECAN_ENODEVICE;
    }
    CPK_ON_DEVICE(device);
    CpkAnchorCtx *c = new CpkAnchorCtx;
    c->device = device;
    c->sc = new PostScratch(nullptr);
    *out = c;  // the caller closes it on every path
    if (!c->sc->stream) {
        cpk_set_error("hipStreamCreate failed in the anchor finder");
        return CPECAN_EHIP;
    }
    HIP_TRY(hipEventCreate(&c->evA));
    HIP_TRY(hipEventCreate(&c->evB));
    c->nForward = nBytes;
    c->nSym = nExtra > 0 ? ((nBytes + 1) & ~(int64_t)1) + nExtra : nBytes;
    uint8_t *dRaw = nullptr;
    if (int rc = c->sc->alloc(&dRaw, (size_t)nBytes)) return rc;
    if (int rc = c->sc->alloc(&c->dSym, (size_t)((c->nSym + 1) / 2))) return rc;
    if (nBytes > 0) {
        HIP_TRY(hipMemcpyAsync(dRaw, bytes, (size_t)nBytes, hipMemcpyHostToDevice, c->sc->stream));
        const unsigned blocks = (unsigned)std::min<int64_t>(((nBytes + 1) / 2 + 255) / 256, 65535);
        hipLaunchKernelGGL(cpk_anchor_pack, dim3(blocks), dim3(256), 0, c->sc->stream, dRaw, nBytes, c->dSym);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->sc->stream));  // `bytes` is the caller's again
    }
    return CPECAN_OK;
}

static_assert(sizeof(CpkAnchorSeed) == sizeof(CpkAnchorPlan().seed), "CpkAnchorPlan holds the seed as the kernels take it");

// The host half of a pass (cpecan_internal.h): the seed, the checks on the pass and on the problem list, the key slots.
extern "C" int cpk_anchor_pass_plan(const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int64_t nSym, int64_t nForward,
                                    CpkAnchorPlan *plan) {
    const CpkAnchorParams &prm = pass->prm;
    *plan = CpkAnchorPlan{};
    auto &seed = plan->seed;
    seed.span = (int32_t)strnlen(pass->seed, sizeof pass->seed);
    for (int i = 0; i < seed.span; i++) {
        if (pass->seed[i] == '1') {
            if (seed.weight < CPK_ANCHOR_MAX_WEIGHT) seed.pos[seed.weight] = (uint8_t)i;
            seed.weight++;
        } else if (pass->seed[i] != '0') {
            seed.weight = 0;
            break;
        }
    }
    if (seed.span < 1 || seed.span > 31 || seed.weight < 1 || seed.weight > CPK_ANCHOR_MAX_WEIGHT || prm.maxSeedOccurrences < 1 ||
        prm.maxHsps < 1 || prm.xDrop < 0 || pass->trim < 0 || pass->seedTransitions < 0 || pass->seedTransitions > 1 ||
        pass->variantThreshold < prm.hspThreshold) {
        cpk_set_error("anchor parameters: the seed is 1..31 characters of 0 / 1 with 1..%d ones; maxSeedOccurrences, maxHsps >= 1; "
                      "xDrop, trim >= 0; seedTransitions 0 or 1; the threshold of variant-seeded HSPs >= hspThreshold",
                      CPK_ANCHOR_MAX_WEIGHT);
        return CPECAN_EINVAL;
    }
    plan->transitions = pass->seedTransitions;
    // A Y window has at most maxSeedOccurrences hits per word it is looked up under: its own and, with seedTransitions, one
    // per compared base.  The bound below keeps a problem's hit count, an int32 like its list sizes, at or under 2^30.
    plan->hitsPerWindow = (int64_t)prm.maxSeedOccurrences * (plan->transitions ? 1 + seed.weight : 1);
    plan->maxCap = plan->maxHits = 1;
    for (int64_t i = 0; i < n; i++) {
        CpkAnchorProblem &p = probs[i];
        // a reverse complement is written from the forward symbols into the area behind them, at an even index
        if ((p.flags & CPK_ANCHOR_RC_Y) && (p.yFwd < 0 || p.lY < 0 || p.yFwd + p.lY > nForward || (p.yOff & 1) ||
                                            p.yOff < ((nForward + 1) & ~(int64_t)1))) {
            cpk_set_error("anchor problem %lld: the reverse complement does not go from the forward symbols to the area behind them",
                          (long long)i);
            return CPECAN_EINVAL;
        }
        if ((p.flags & CPK_ANCHOR_SHARE_X) && (i == 0 || probs[i - 1].xOff != p.xOff || probs[i - 1].lX != p.lX ||
                                               probs[i - 1].softMask != p.softMask || (probs[i - 1].flags & CPK_ANCHOR_SHARE_X))) {
            cpk_set_error("anchor problem %lld: a twin follows the problem whose X it shares", (long long)i);
            return CPECAN_EINVAL;
        }
        const int diags = CPK_ANCHOR_DIAGS(p.flags);
        if ((p.flags & CPK_ANCHOR_GAPPED) ? p.yDrop <= 0 || diags < CPK_ANCHOR_GAPPED_MIN_DIAGS || diags > CPK_ANCHOR_GAPPED_MAX_DIAGS
                                          : p.yDrop != 0 || diags != 0) {
            cpk_set_error("anchor problem %lld: a gapped extension has a yDrop > 0 and %d .. %d anti-diagonals, and no other problem "
                          "has either", (long long)i, CPK_ANCHOR_GAPPED_MIN_DIAGS, CPK_ANCHOR_GAPPED_MAX_DIAGS);
            return CPECAN_EINVAL;
        }
        if (p.flags & CPK_ANCHOR_RC_Y) plan->maxRc = std::max(plan->maxRc, p.lY);
        if (p.lX < 0 || p.lY < 0 || p.xOff < 0 || p.yOff < 0 || p.xOff + p.lX > nSym || p.yOff + p.lY > nSym ||
            p.lX > (1 << 24) || p.lY > (1 << 24) || (int64_t)p.lY * plan->hitsPerWindow > (1 << 30)) {
            cpk_set_error("anchor problem %lld: sequences outside the buffer, longer than 2^24, or too many seed occurrences allowed",
                          (long long)i);
            return CPECAN_EINVAL;
        }
        p.capX = anchor_pow2(std::max(p.lX - seed.span + 1, 1));
        p.capY = anchor_pow2(std::max(p.lY - seed.span + 1, 1));
        if (p.flags & CPK_ANCHOR_SHARE_X) {  // X's words are made and sorted once per pair
            p.keyXOff = probs[i - 1].keyXOff;
            p.keyYOff = plan->nKeys;
            plan->nKeys += p.capY;
        } else {
            p.keyXOff = plan->nKeys;
            p.keyYOff = plan->nKeys + p.capX;
            plan->nKeys += (int64_t)p.capX + p.capY;
        }
        plan->maxCap = std::max(plan->maxCap, std::max(p.capX, p.capY));
        p.hits = p.hsps = p.chained = p.nRuns = p.capped = p.score = 0;
        p.columns = 0;
        p.hspCap = 0;
        p.hspOff = 0;
    }
    return CPECAN_OK;
}

// The hit counts are back: the HSP list of every problem, which is its hit list too on the transition path.
extern "C" void cpk_anchor_pass_size(CpkAnchorProblem *probs, int64_t n, CpkAnchorPlan *plan) {
    plan->nSlots = 0;
    plan->maxHits = 1;
    for (int64_t i = 0; i < n; i++) {
        probs[i].hspCap = anchor_pow2(std::max(probs[i].hits, 1));
        probs[i].hspOff = plan->nSlots;
        plan->nSlots += probs[i].hspCap;
        plan->maxHits = std::max(plan->maxHits, probs[i].hits);
    }
    plan->nCounters = n * (plan->transitions ? 2 : 1);  // HSPs handed out, then the hits written
}

// Step 5b, after the chains are back: where the scratch rows and the runs of every problem start.  rowBase and runBase
// hold n + 1 values each, the last the total.
extern "C" void cpk_anchor_gapped_size(const CpkAnchorProblem *probs, int64_t n, int64_t *rowBase, int64_t *runBase,
                                       CpkAnchorGappedPlan *plan) {
    *plan = CpkAnchorGappedPlan{};
    for (int64_t i = 0; i < n; i++) {
        const bool gapped = probs[i].flags & CPK_ANCHOR_GAPPED;
        rowBase[i] = plan->nRows;
        runBase[i] = plan->nRuns;
        plan->nRows += gapped ? probs[i].columns : 0;  // cpk_anchor_chain_untrimmed left the rows there
        // every block takes a row at least, and the chained HSPs come on top; a chain that is not extended is trimmed already
        plan->nRuns += gapped ? probs[i].columns + probs[i].chained : probs[i].nRuns;
        if (gapped) plan->maxGaps = std::max(plan->maxGaps, probs[i].chained + 1);
    }
    rowBase[n] = plan->nRows;
    runBase[n] = plan->nRuns;
}

// The end of the launch that starts at row lo: the last of the gap boundaries (ascending, the last one the total) that is
// at most budgetRows behind lo.  A gap has at most 2 * CPK_ANCHOR_GAPPED_MAX_DIAGS rows, so with a budget of that much the
// end lies behind lo.
extern "C" int64_t cpk_anchor_gapped_slice_end(const int64_t *bounds, int64_t nBounds, int64_t lo, int64_t budgetRows) {
    int64_t a = 0, b = nBounds;  // the first boundary beyond lo + budgetRows
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (bounds[mid] <= lo + budgetRows) a = mid + 1;
        else b = mid;
    }
    return a > 0 ? bounds[a - 1] : lo;
}

// The end of a pass that extends chains (step 5b); evA is recorded.  The chains come back untrimmed with their row counts,
// the host sizes scratch, block list and runs, the extensions run -- in several launches when the scratch would pass the
// budget -- and the assembly trims.
static int anchor_pass_gapped(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, PostScratch &sc,
                              CpkAnchorProblem *dProbs, int4 *dHsps, int32_t *dCount, int32_t *dBest, int32_t *dPred, int32_t *dChain,
                              size_t nSlots, int32_t **runsOut, double *ms) {
    hipStream_t st = sc.stream;
    const size_t probBytes = sizeof(CpkAnchorProblem) * (size_t)n, nGaps = nSlots + (size_t)n;  // chained + 1 <= hspCap + 1 per problem
    float part = 0.f;
    int32_t *dGapRow = nullptr;
    int2 *dCounts = nullptr;
    if (int rc = sc.alloc(&dGapRow, nGaps)) return rc;
    if (int rc = sc.alloc(&dCounts, nGaps)) return rc;
    HIP_TRY(hipMemsetAsync(dGapRow, 0, sizeof(int32_t) * nGaps, st));
    HIP_TRY(hipMemsetAsync(dCounts, 0, sizeof(int2) * nGaps, st));
    hipLaunchKernelGGL(cpk_anchor_chain_untrimmed, dim3((unsigned)n), dim3(256), 0, st, dProbs, dHsps, dCount, dBest, dPred, dChain,
                       pass->prm.maxHsps, pass->trim, dGapRow);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    HIP_TRY(hipMemcpyAsync(probs, dProbs, probBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&part, c->evA, c->evB));
    *ms += part;

    // round 3: the extensions and the assembly
    CpkAnchorGappedPlan plan;
    std::vector<int64_t> base(2 * ((size_t)n + 1));
    int64_t *rowBase = base.data(), *runBase = rowBase + n + 1;
    cpk_anchor_gapped_size(probs, n, rowBase, runBase, &plan);
    const int64_t budget = CPK_ANCHOR_GAPPED_BUDGET_ROWS;
    std::vector<int64_t> bounds;  // only a pass over the budget needs the gap boundaries
    if (plan.nRows > budget) {
        std::vector<int32_t> gapRow(nGaps);
        HIP_TRY(hipMemcpy(gapRow.data(), dGapRow, sizeof(int32_t) * nGaps, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++)
            for (int g = 0; (probs[i].flags & CPK_ANCHOR_GAPPED) && g <= probs[i].chained; g++)
                bounds.push_back(rowBase[i] + gapRow[(size_t)probs[i].hspOff + (size_t)i + (size_t)g]);
        bounds.push_back(plan.nRows);
    }
    int64_t *dBase = nullptr;
    uint8_t *dTrace = nullptr;
    int32_t *dBlocks = nullptr, *dRunsOut = nullptr;
    const size_t nRunsCap = (size_t)std::max<int64_t>(plan.nRuns, 1);
    if (int rc = sc.alloc(&dBase, base.size())) return rc;
    if (int rc = sc.alloc(&dTrace, (size_t)std::max<int64_t>(std::min(plan.nRows, budget), 1) * 64)) return rc;
    if (int rc = sc.alloc(&dBlocks, (size_t)std::max<int64_t>(plan.nRows, 1) * 3)) return rc;
    if (int rc = sc.alloc(&dRunsOut, nRunsCap * 3)) return rc;
    HIP_TRY(hipMemcpyAsync(dBase, base.data(), sizeof(int64_t) * base.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->evA, st));
    for (int64_t lo = 0; lo < plan.nRows;) {
        const int64_t hi = bounds.empty() ? plan.nRows : cpk_anchor_gapped_slice_end(bounds.data(), (int64_t)bounds.size(), lo, budget);
        if (hi <= lo) {
            cpk_set_error("anchor finder: a gap's extensions do not fit the scratch budget");
            return CPECAN_EINVAL;
        }
        hipLaunchKernelGGL(cpk_anchor_gapped, dim3((unsigned)n, (unsigned)plan.maxGaps), dim3(64), 0, st, dProbs, c->dSym, pass->prm,
                           dChain, dGapRow, dBase, lo, hi, dTrace, dBlocks, dCounts);
        HIP_TRY(hipGetLastError());
        lo = hi;
    }
    hipLaunchKernelGGL(cpk_anchor_assemble, dim3((unsigned)n), dim3(64), 0, st, dProbs, dChain, dGapRow, dBase, dBase + n + 1, dBlocks,
                       dCounts, dRunsOut, pass->trim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    int32_t *runs = (int32_t *)malloc(sizeof(int32_t) * 3 * nRunsCap);
    if (!runs) {
        cpk_set_error("out of memory");
        return CPECAN_ENOMEM;
    }
    hipError_t e = hipMemcpyAsync(probs, dProbs, probBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(runs, dRunsOut, sizeof(int32_t) * 3 * nRunsCap, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(&part, c->evA, c->evB);
    if (e != hipSuccess) {
        free(runs);
        HIP_TRY(e);
    }
    *ms += part;
    *runsOut = runs;
    return CPECAN_OK;
}

// The device lists of a pass once steps 1-3 are queued: the HSP slots of every problem as cpk_anchor_hits / cpk_anchor_extend
// fill them, their counters, and the scratch words and run slots that the kernel behind them works in.
struct AnchorPassLists {
    CpkAnchorProblem *dProbs = nullptr;
    int4 *dHsps = nullptr;
    int32_t *dCount = nullptr, *dBest = nullptr, *dPred = nullptr, *dRuns = nullptr;
    size_t nSlots = 0;
};

// Steps 0-3 of a pass (n > 0), the part every chain kernel shares (cpk_anchor_pass, cpk_local_pass): round 1 counts the
// hits, the host sizes the lists, round 2 queues the extension.  On return the stream holds the launches that fill the HSP
// lists, evA is recorded in front of them, and probs has the hit counts and the slots.  sc: the caller's, on c's stream.
static int anchor_pass_lists(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, PostScratch &sc,
                             AnchorPassLists *lists, double *ms) {
    CpkAnchorPlan plan;
    if (int rc = cpk_anchor_pass_plan(pass, probs, n, c->nSym, c->nForward, &plan)) return rc;
    const CpkAnchorParams &prm = pass->prm;
    CpkAnchorSeed seed;
    memcpy(&seed, &plan.seed, sizeof seed);
    hipStream_t st = sc.stream;
    const size_t probBytes = sizeof(CpkAnchorProblem) * (size_t)n;
    const dim3 perChunk((unsigned)n, (unsigned)std::min(64, (plan.maxCap + 1023) / 1024));
    CpkAnchorProblem *dProbs = nullptr;
    unsigned long long *dKeys = nullptr;
    if (int rc = sc.alloc(&dProbs, (size_t)n)) return rc;
    if (int rc = sc.alloc(&dKeys, (size_t)plan.nKeys)) return rc;
    float part = 0.f;

    // round 1: steps 0 and 1, the hits counted
    HIP_TRY(hipMemcpyAsync(dProbs, probs, probBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->evA, st));
    if (plan.maxRc > 0) {  // step 0, only in a pass that has a minus strand
        const unsigned rcChunks = (unsigned)std::min(1024, (plan.maxRc / 2 + 256) / 256);
        hipLaunchKernelGGL(cpk_anchor_revcomp, dim3((unsigned)n, rcChunks), dim3(256), 0, st, dProbs, c->dSym);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cpk_anchor_words, dim3(perChunk.x, perChunk.y, 2), dim3(256), 0, st, dProbs, c->dSym, seed, dKeys);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpk_anchor_sort_keys, dim3((unsigned)n, 2), dim3(plan.maxCap >= 4096 ? 1024 : 256), 0, st, dProbs, dKeys);
    HIP_TRY(hipGetLastError());
    if (plan.transitions)
        hipLaunchKernelGGL(cpk_anchor_join<false>, perChunk, dim3(256), 0, st, dProbs, dKeys, prm.maxSeedOccurrences, seed.weight,
                           (int2 *)nullptr, (int32_t *)nullptr);
    else
        hipLaunchKernelGGL(cpk_anchor_hits<false>, perChunk, dim3(256), 0, st, dProbs, c->dSym, dKeys, prm, seed.span,
                           (int4 *)nullptr, (int32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    HIP_TRY(hipMemcpyAsync(probs, dProbs, probBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&part, c->evA, c->evB));
    *ms += part;

    // round 2: the lists sized by the hit counts; steps 2 to 5
    cpk_anchor_pass_size(probs, n, &plan);
    const size_t nSlots = (size_t)plan.nSlots;
    int4 *dHsps = nullptr;
    int2 *dHits = nullptr;  // transition path: the hit list of every problem, the HSP list's slots and offsets
    int32_t *dCount = nullptr, *dBest = nullptr, *dPred = nullptr, *dRuns = nullptr;
    if (int rc = sc.alloc(&dHsps, nSlots)) return rc;
    if (plan.transitions) {
        if (int rc = sc.alloc(&dHits, nSlots)) return rc;
    }
    if (int rc = sc.alloc(&dCount, (size_t)plan.nCounters)) return rc;
    if (int rc = sc.alloc(&dBest, nSlots)) return rc;
    if (int rc = sc.alloc(&dPred, nSlots)) return rc;
    if (int rc = sc.alloc(&dRuns, nSlots * 3)) return rc;
    HIP_TRY(hipMemcpyAsync(dProbs, probs, probBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dCount, 0, sizeof(int32_t) * (size_t)plan.nCounters, st));
    HIP_TRY(hipEventRecord(c->evA, st));
    if (plan.transitions) {
        hipLaunchKernelGGL(cpk_anchor_join<true>, perChunk, dim3(256), 0, st, dProbs, dKeys, prm.maxSeedOccurrences, seed.weight, dHits,
                           dCount + n);
        HIP_TRY(hipGetLastError());
        const unsigned hitChunks = (unsigned)std::min(1024, (plan.maxHits + 255) / 256);
        hipLaunchKernelGGL(cpk_anchor_extend, dim3((unsigned)n, hitChunks), dim3(256), 0, st, dProbs, c->dSym, dHits, prm,
                           pass->variantThreshold, seed.span, dHsps, dCount);
    } else {
        hipLaunchKernelGGL(cpk_anchor_hits<true>, perChunk, dim3(256), 0, st, dProbs, c->dSym, dKeys, prm, seed.span, dHsps, dCount);
    }
    HIP_TRY(hipGetLastError());
    *lists = AnchorPassLists{dProbs, dHsps, dCount, dBest, dPred, dRuns, nSlots};
    return CPECAN_OK;
}

extern "C" int cpk_anchor_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, CpkAnchorProblem *probs, int64_t n, int32_t **runsOut,
                               double *ms) {
    *runsOut = nullptr;
    if (n <= 0) return CPECAN_OK;
    CPK_ON_DEVICE(c->device);
    PostScratch sc(c->sc->stream);  // this pass's blocks go back to the cache when it returns
    hipStream_t st = sc.stream;
    AnchorPassLists lists;
    if (int rc = anchor_pass_lists(c, pass, probs, n, sc, &lists, ms)) return rc;
    const CpkAnchorParams &prm = pass->prm;
    const size_t probBytes = sizeof(CpkAnchorProblem) * (size_t)n, nSlots = lists.nSlots;
    const dim3 perProblem((unsigned)n);
    CpkAnchorProblem *dProbs = lists.dProbs;
    int4 *dHsps = lists.dHsps;
    int32_t *dCount = lists.dCount, *dBest = lists.dBest, *dPred = lists.dPred, *dRuns = lists.dRuns;
    float part = 0.f;
    bool gapped = false;
    for (int64_t i = 0; i < n; i++) gapped = gapped || (probs[i].flags & CPK_ANCHOR_GAPPED);
    if (gapped) return anchor_pass_gapped(c, pass, probs, n, sc, dProbs, dHsps, dCount, dBest, dPred, dRuns, nSlots, runsOut, ms);
    hipLaunchKernelGGL(cpk_anchor_chain, perProblem, dim3(256), 0, st, dProbs, dHsps, dCount, dBest, dPred, dRuns, prm.maxHsps,
                       pass->trim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    int32_t *runs = (int32_t *)malloc(sizeof(int32_t) * 3 * nSlots);
    if (!runs) {
        cpk_set_error("out of memory");
        return CPECAN_ENOMEM;
    }
    hipError_t e = hipMemcpyAsync(probs, dProbs, probBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(runs, dRuns, sizeof(int32_t) * 3 * nSlots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(&part, c->evA, c->evB);
    if (e != hipSuccess) {
        free(runs);
        HIP_TRY(e);
    }
    *ms += part;
    *runsOut = runs;
    return CPECAN_OK;
}

// Step 7b, the host's part: where the gaps, scratch rows and runs of a pass that extends its chains lie.  Built from the
// chain records and the HSP triples that came back behind the peel (trim 0: a problem's run slots hold its chains' HSPs).
// Gaps are numbered problem by problem, chain by chain; rows round by round, so that a round's rows lie together and the
// scratch of one round serves the next.  A gap has the rows of the unfenced rectangle (anchor_gap_rows): the fences only
// shrink an extension.
struct LocalGappedLayout {
    std::vector<int64_t> gapBase;  // nLocal * maxChains + 1: first gap of every chain slot
    std::vector<int64_t> gapRow;   // per gap: its first row, and the first row of its left extension
    std::vector<int64_t> runBase;  // nLocal + 1: first run triple of every caller problem
    std::vector<std::vector<int64_t>> bounds;  // per round: where the rows of its gaps start, ascending, then the round's end
    std::vector<int> roundGaps;    // per round: most gaps of one chain
    int64_t nRows = 0, maxRoundRows = 0;
};

static int local_gapped_layout(const CpkAnchorProblem *probs, const CpkLocalProblem *lprobs, int64_t nLocal,
                               const CpkLocalChain *chains, const int32_t *hsps, int maxChains, LocalGappedLayout *out) {
    LocalGappedLayout &L = *out;
    L.gapBase.assign((size_t)nLocal * maxChains + 1, 0);
    L.runBase.assign((size_t)nLocal + 1, 0);
    L.bounds.assign((size_t)maxChains, {});
    L.roundGaps.assign((size_t)maxChains, 0);
    int64_t nGaps = 0;
    for (int64_t k = 0; k < nLocal; k++)
        for (int r = 0; r < maxChains; r++) {
            L.gapBase[(size_t)(k * maxChains + r)] = nGaps;
            if (r < lprobs[k].nChains) nGaps += chains[k * maxChains + r].nHsps + 1;
        }
    L.gapBase.back() = nGaps;
    L.gapRow.assign(2 * (size_t)nGaps, 0);
    std::vector<int64_t> rowsOf((size_t)nLocal * maxChains, 0);
    for (int r = 0; r < maxChains; r++) {
        const int64_t roundStart = L.nRows;
        for (int64_t k = 0; k < nLocal; k++) {
            if (r >= lprobs[k].nChains) continue;
            const CpkAnchorProblem &p = probs[lprobs[k].first];
            const CpkLocalChain &ch = chains[k * maxChains + r];
            const int32_t *h = hsps + 3 * (p.hspOff + ch.runOff);
            const int c = ch.nHsps, maxDiags = CPK_ANCHOR_DIAGS(p.flags);
            if (c < 1 || ch.runOff < 0 || ch.runOff + c > lprobs[k].nRuns) {
                cpk_set_error("local chains: a chain record does not name HSPs of its problem");
                return CPECAN_EHIP;
            }
            L.roundGaps[(size_t)r] = std::max(L.roundGaps[(size_t)r], c + 1);
            int pX = 0, pY = 0;
            for (int g = 0; g <= c; g++) {
                const int bX = g < c ? h[3 * g] : p.lX, bY = g < c ? h[3 * g + 1] : p.lY;
                if (bX < pX || bY < pY) {
                    cpk_set_error("local chains: the HSPs of a chain do not ascend");
                    return CPECAN_EHIP;
                }
                const int rows = std::min(bX - pX + bY - pY, maxDiags);
                const int64_t q = L.gapBase[(size_t)(k * maxChains + r)] + g;
                L.gapRow[2 * (size_t)q] = L.nRows;
                L.gapRow[2 * (size_t)q + 1] = L.nRows + (g >= 1 ? rows : 0);
                L.bounds[(size_t)r].push_back(L.nRows);
                L.nRows += (g >= 1 ? rows : 0) + (g < c ? rows : 0);
                if (g < c) pX = bX + h[3 * g + 2], pY = bY + h[3 * g + 2];
            }
            rowsOf[(size_t)(k * maxChains + r)] = L.nRows - L.bounds[(size_t)r][L.bounds[(size_t)r].size() - (size_t)(c + 1)];
        }
        L.bounds[(size_t)r].push_back(L.nRows);
        L.maxRoundRows = std::max(L.maxRoundRows, L.nRows - roundStart);
    }
    for (int64_t k = 0; k < nLocal; k++) {  // every block takes a row at least, and the chained HSPs come on top
        int64_t cap = 0;
        for (int r = 0; r < lprobs[k].nChains; r++) cap += rowsOf[(size_t)(k * maxChains + r)] + chains[k * maxChains + r].nHsps;
        L.runBase[(size_t)k + 1] = L.runBase[(size_t)k] + cap;
    }
    return CPECAN_OK;
}

// The end of a local pass that extends its chains (step 7b); the peel's records are on the host and still on the device.
// Per round one launch of cpk_local_gapped -- several, cut at gap boundaries, where the round's rows pass the scratch budget --
// then the assembly.  *runsOut (the HSP triples on entry) is replaced by the runs, and hspOff of every problem's first twin
// moves to them.
static int local_pass_gapped(CpkAnchorCtx *c, const CpkAnchorPass *pass, const CpkLocalPass *lp, CpkAnchorProblem *probs,
                             CpkLocalProblem *lprobs, int64_t nLocal, PostScratch &sc, const AnchorPassLists &lists,
                             CpkLocalProblem *dLocal, CpkLocalChain *dChains, CpkLocalChain *chains, int32_t **runsOut, double *ms) {
    hipStream_t st = sc.stream;
    const int K = lp->maxChains;
    LocalGappedLayout L;
    if (int rc = local_gapped_layout(probs, lprobs, nLocal, chains, *runsOut, K, &L)) return rc;
    const int64_t budget = CPK_ANCHOR_GAPPED_BUDGET_ROWS, nGaps = L.gapBase.back(), nRunsCap = std::max<int64_t>(L.runBase.back(), 1);
    int64_t *dGapBase = nullptr, *dGapRow = nullptr, *dRunBase = nullptr;
    uint8_t *dTrace = nullptr;
    int32_t *dBlocks = nullptr, *dRunsOut = nullptr;
    int2 *dCounts = nullptr;
    const size_t nCounts = (size_t)std::max<int64_t>(nGaps, 1);
    if (int rc = sc.alloc(&dGapBase, L.gapBase.size())) return rc;
    if (int rc = sc.alloc(&dGapRow, std::max<size_t>(L.gapRow.size(), 2))) return rc;
    if (int rc = sc.alloc(&dRunBase, L.runBase.size())) return rc;
    if (int rc = sc.alloc(&dTrace, (size_t)std::max<int64_t>(std::min(L.maxRoundRows, budget), 1) * 64)) return rc;
    if (int rc = sc.alloc(&dBlocks, (size_t)std::max<int64_t>(L.nRows, 1) * 3)) return rc;
    if (int rc = sc.alloc(&dCounts, nCounts)) return rc;
    if (int rc = sc.alloc(&dRunsOut, (size_t)nRunsCap * 3)) return rc;
    HIP_TRY(hipMemcpyAsync(dGapBase, L.gapBase.data(), sizeof(int64_t) * L.gapBase.size(), hipMemcpyHostToDevice, st));
    if (!L.gapRow.empty())
        HIP_TRY(hipMemcpyAsync(dGapRow, L.gapRow.data(), sizeof(int64_t) * L.gapRow.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dRunBase, L.runBase.data(), sizeof(int64_t) * L.runBase.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dCounts, 0, sizeof(int2) * nCounts, st));
    HIP_TRY(hipEventRecord(c->evA, st));
    for (int r = 0; r < K; r++) {
        const std::vector<int64_t> &bounds = L.bounds[(size_t)r];
        const int64_t end = bounds.back();
        for (int64_t lo = bounds.front(); lo < end;) {
            const int64_t hi = end - lo <= budget ? end : cpk_anchor_gapped_slice_end(bounds.data(), (int64_t)bounds.size(), lo, budget);
            if (hi <= lo) {
                cpk_set_error("local chains: a gap's extensions do not fit the scratch budget");
                return CPECAN_EINVAL;
            }
            hipLaunchKernelGGL(cpk_local_gapped, dim3((unsigned)nLocal, (unsigned)L.roundGaps[(size_t)r]), dim3(64), 0, st, lists.dProbs,
                               dLocal, dChains, c->dSym, pass->prm, lists.dRuns, dGapBase, dGapRow, K, r, lo, hi, dTrace, dBlocks,
                               dCounts);
            HIP_TRY(hipGetLastError());
            lo = hi;
        }
    }
    hipLaunchKernelGGL(cpk_local_gapped_assemble, dim3((unsigned)nLocal), dim3(64), 0, st, lists.dProbs, dLocal, dChains, lists.dRuns,
                       dGapBase, dGapRow, dRunBase, dBlocks, dCounts, dRunsOut, K, pass->trim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    int32_t *runs = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)nRunsCap);
    if (!runs) {
        cpk_set_error("out of memory");
        return CPECAN_ENOMEM;
    }
    float part = 0.f;
    hipError_t e = hipMemcpyAsync(lprobs, dLocal, sizeof(CpkLocalProblem) * (size_t)nLocal, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(chains, dChains, sizeof(CpkLocalChain) * (size_t)nLocal * (size_t)K, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(runs, dRunsOut, sizeof(int32_t) * 3 * (size_t)nRunsCap, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(&part, c->evA, c->evB);
    if (e != hipSuccess) {
        free(runs);
        HIP_TRY(e);
    }
    *ms += part;
    for (int64_t k = 0; k < nLocal; k++) probs[lprobs[k].first].hspOff = L.runBase[(size_t)k];
    free(*runsOut);
    *runsOut = runs;
    return CPECAN_OK;
}

// Local chains (cpk_local.inl): steps 0-3 as in cpk_anchor_pass, then cpk_local_peel with one workgroup per caller problem
// over the pools of its twins.  *chains: malloc'd, lp->maxChains records per caller problem; *runs: malloc'd triples, the
// runs of caller problem k from 3 * probs[lprobs[k].first].hspOff on, chain by chain.  lprobs gets the counts.  Where the
// problems carry CPK_ANCHOR_GAPPED -- all of them or none -- the chains are then extended (step 7b, local_pass_gapped).
extern "C" int cpk_local_pass(CpkAnchorCtx *c, const CpkAnchorPass *pass, const CpkLocalPass *lp, CpkAnchorProblem *probs, int64_t n,
                              CpkLocalProblem *lprobs, int64_t nLocal, CpkLocalChain **chainsOut, int32_t **runsOut, double *ms) {
    *chainsOut = nullptr;
    *runsOut = nullptr;
    if (n <= 0 || nLocal <= 0) return CPECAN_OK;
    if (lp->maxChains < 1 || lp->maxChains > CPK_LOCAL_MAX_CHAINS) {
        cpk_set_error("local chains: maxChains is 1 .. %d", CPK_LOCAL_MAX_CHAINS);
        return CPECAN_EINVAL;
    }
    for (int64_t k = 0; k < nLocal; k++) {  // the twins of a caller problem follow each other, so do their slots
        const CpkLocalProblem &q = lprobs[k];
        if (q.twins < 1 || q.twins > 2 || q.first < 0 || q.first + q.twins > n ||
            (q.twins == 2 && !(probs[q.first + 1].flags & CPK_ANCHOR_SHARE_X))) {
            cpk_set_error("local chains: problem %lld does not name one problem of the pass or a pair of twins", (long long)k);
            return CPECAN_EINVAL;
        }
    }
    int64_t nGapped = 0;
    for (int64_t i = 0; i < n; i++) nGapped += (probs[i].flags & CPK_ANCHOR_GAPPED) != 0;
    if (nGapped != 0 && nGapped != n) {
        cpk_set_error("local chains: either every problem of a pass extends its chains or none does");
        return CPECAN_EINVAL;
    }
    const bool gapped = nGapped != 0;
    CPK_ON_DEVICE(c->device);
    PostScratch sc(c->sc->stream);
    hipStream_t st = sc.stream;
    AnchorPassLists lists;
    if (int rc = anchor_pass_lists(c, pass, probs, n, sc, &lists, ms)) return rc;
    const size_t probBytes = sizeof(CpkAnchorProblem) * (size_t)n, localBytes = sizeof(CpkLocalProblem) * (size_t)nLocal;
    const size_t nChainSlots = (size_t)nLocal * (size_t)lp->maxChains, nSlots = lists.nSlots;
    CpkLocalProblem *dLocal = nullptr;
    CpkLocalChain *dChains = nullptr;
    if (int rc = sc.alloc(&dLocal, (size_t)nLocal)) return rc;
    if (int rc = sc.alloc(&dChains, nChainSlots)) return rc;
    HIP_TRY(hipMemcpyAsync(dLocal, lprobs, localBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dChains, 0, sizeof(CpkLocalChain) * nChainSlots, st));
    hipLaunchKernelGGL(cpk_local_peel, dim3((unsigned)nLocal), dim3(256), 0, st, lists.dProbs, dLocal, lists.dHsps, lists.dCount,
                       lists.dBest, lists.dPred, lists.dRuns, dChains, pass->prm.maxHsps, gapped ? 0 : pass->trim, lp->maxChains,
                       lp->minChainScore);  // trim 0: the run slots keep every chained HSP for step 7b, which trims behind it
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evB, st));
    CpkLocalChain *chains = (CpkLocalChain *)malloc(sizeof(CpkLocalChain) * nChainSlots);
    int32_t *runs = (int32_t *)malloc(sizeof(int32_t) * 3 * nSlots);
    float part = 0.f;
    const bool noMemory = !chains || !runs;
    hipError_t e = noMemory ? hipErrorOutOfMemory : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(probs, lists.dProbs, probBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(lprobs, dLocal, localBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(chains, dChains, sizeof(CpkLocalChain) * nChainSlots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(runs, lists.dRuns, sizeof(int32_t) * 3 * nSlots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(&part, c->evA, c->evB);
    if (e != hipSuccess) {
        free(chains);
        free(runs);
        if (noMemory) {
            cpk_set_error("out of memory");
            return CPECAN_ENOMEM;
        }
        HIP_TRY(e);
    }
    *ms += part;
    if (gapped) {
        if (int rc = local_pass_gapped(c, pass, lp, probs, lprobs, nLocal, sc, lists, dLocal, dChains, chains, &runs, ms)) {
            free(chains);
            free(runs);
            return rc;
        }
    }
    *chainsOut = chains;
    *runsOut = runs;
    return CPECAN_OK;
}
