// tvz_handle.h — the corpus handle of tvz_match.hip (its only includer): the types that own its GPU resources, the
// index's device image, and their small helpers.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <ctime>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "tvz_index_kernels.h"

namespace {

// The owning types below free what they hold in their destructors, so they are not copied.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// A device buffer of `cap` elements, grown by ensure(); it frees itself.
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    int64_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// A pinned host buffer (pinned_alloc); a MAPPED one is also addressable from the device at `d`, where the
// single-query kernels write their hits.  It frees itself.
template <typename T>
struct Pinned : NoCopy {
    T *h = nullptr;
    T *d = nullptr;
    ~Pinned() { if (h) (void)hipHostFree(h); }
};

// A stream (`s`) or an event (`e`) that its owner creates in place, with flags or with a priority; it destroys itself.
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// Per-thread-of-control scratch of tvz_find_duplicates: its own stream, a pinned query buffer
// and a pinned, device-mapped hit buffer the kernel writes into.  Sized at create / reserve /
// upload for the reserved row count, so a query allocates nothing.
struct Staging {
    Stream stream;
    Pinned<int64_t> query;           // {0, n} + canonical-order query keys (as double bits)
    DevBuf<int64_t> d_query;         // device copy of the same
    Pinned<int32_t> hits;            // mapped: [blocks][region][3]
    Pinned<int32_t> counts;          // mapped: [kQ1MaxBlocks] per sweep block, then one per sub-index
    int64_t hit_slots = 0;           // capacity of `hits` in hits
    Pinned<int32_t> ix_hits;         // mapped: hits of the index lookup [ix_slots][3]
    int64_t ix_slots = 0;
    DevBuf<int32_t> d_hits;          // device hit list [3 per hit] for the paths that need a fix-up pass
    DevBuf<int32_t> d_hits_n;
    DevBuf<int64_t> d_sq;            // long queries: sorted distinct keys + multiplicities
    DevBuf<int32_t> d_smult;
    // tvz_find_duplicates_tol: the sorted query (values, then positions) of up to kMaxQueryLen timestamps,
    // pinned + its device copy; longer queries use the growable d_tol_big
    Pinned<unsigned char> tol;
    DevBuf<unsigned char> d_tol;
    DevBuf<unsigned char> d_tol_big;
    std::vector<std::pair<double, int32_t>> tol_sort;   // host sort scratch (keeps its capacity)
    std::atomic<int> busy{0};        // a sweep of this staging is in flight (drain() waits for it)
    int gen = 0;                     // index generation that sweep reads
};

constexpr int kQ1MaxBlocks = 2048;
constexpr int kStageGroups = kIxBlock / kGroup;   // row groups of the widest sweep block (the fused lookup's): every
                                                  // block's hit region rounds up to whole row groups
constexpr int64_t kQueryStageKeys = kMaxQueryLen + 1;
// a query's sorted values + positions (12 B per timestamp), then for min_match > 5 the raw query (8 B per timestamp)
constexpr size_t kTolStageBytes = (size_t)kQueryStageKeys * 20 + 64;
constexpr int kRingSlots = 16;                    // pinned upsert payload ring
constexpr int64_t kRingSlotKeys = 8192;           // 64 KiB each

struct RingSlot {
    Pinned<int64_t> buf;
    Event ev;
    bool pending = false;
};

// Inverted index over rows [0, n_main) as they were when it was built (tvz_index_kernels.h) plus
// the DELTA table: the current entry of every row that was added or replaced since.  A match with
// the index = index lookup (rows that are unchanged since the build) + a sweep of the delta table.
constexpr int kLdsPerWorkgroup = 160 * 1024;        // gfx950
constexpr int kIxResidentBlocks = 256 * 4;          // lookup blocks (512 threads, <= 40 KiB of LDS) resident on an MI355X
constexpr int kQ1StaticLds = kQ1Stage * 12 + 64;    // ts_match_q1_kernel: per-block hit staging + a few words (3,088 B in the code object)
constexpr int kIxMaxLds = 159 * 1024;               // gfx950: 160 KiB of LDS per workgroup, less the static part
constexpr int64_t kIxSliceBytes = 32 * 1024;        // a directory slice, built by one block in LDS
constexpr int64_t kIxSliceBytesMax = 128 * 1024;
constexpr int kIxSliceLdsFloor = 40 * 1024;         // LDS asked for per slice block: at most 3 per CU, 40 KB stay free
// Directory load.  Every probe step of a lookup is a dependent random line fetch, and a wave waits for its
// LONGEST chain - the 13 % of a shard batch's keys that are in no row of the shard walk to the next free slot.
// Measured on rank 0's 1/8 shard of config 4 (Q = 4096, lookup kernel, rocprofv3): load <= 0.9 / 0.8: 86 us,
// <= 0.5: 60.4, <= 0.25: 57.7, <= 0.12: 57.8 (full corpus 347 -> 341 us).  Memory is not the constraint
// (64 MB of directory at config 4 on a 288 GB device).
constexpr int kIxDirLoadPct = 25;
#ifndef TVZ_BK_FILL_PCT
#define TVZ_BK_FILL_PCT 35
#endif
constexpr int kBkFillPct = TVZ_BK_FILL_PCT;       // bucket directory (one-sub-index handles): payload bytes in use, target
constexpr int64_t kIndexMinRows = 4096;           // a corpus grown by upserts gets its first index here
constexpr int64_t kIndexMinDelta = 512;           // rebuilt when the delta exceeds max(this, n_main / 256)

// One directory of a generation and its postings (tvz_index_kernels.h).
struct Directory {
    DevBuf<unsigned char> dir;        // 2^log2 entries of 16 + 2 ks bytes
    DevBuf<uint16_t> post;
    int log2 = 0;
    int slice_log2 = 0;               // entries per directory slice (probing wraps inside a slice)
    int ks = 0;                       // uint16 counts per directory entry
    bool partitioned = false;         // built slice by slice (build_classic); a one-slice partitioned build has
                                      // slice_log2 == log2 too, so the sizes alone do not tell
    // A handle of ONE sub-index keeps the BUCKET directory of tvz_bucket_dir.h: nb buckets of 128 bytes - a key's
    // entry and its postings in one line - + the external lists behind them, all in `dir`; `post` is unused.
    // 0 = the classic format (the cell directory always).
    uint32_t nb = 0;
    int64_t n_post = 0, n_distinct = 0;
    int bits() const { return nb ? -(int)nb : ix_dir_bits(log2, slice_log2); }   // the kernels' argument
    const uint16_t *post_ptr() const { return nb ? reinterpret_cast<const uint16_t *>(dir.p) : post.p; }
};

struct DirHint { int64_t post = 0, distinct = 0; };   // postings / distinct keys of a directory's last build (sizes the next)

// One generation of the index's device image (tvz_index_kernels.h).  There are two: matches read
// `cur`, a rebuild fills the other one (the SHADOW) while they keep running, and a swap under the
// handle's lock makes it current - no reader ever waits for a rebuild.
struct IndexBuf {
    Directory keys;                   // over the keys of rows [0, n_main)
    DevBuf<int32_t> ivid;
    DevBuf<Row> drows;                // the delta table that goes with this generation
    int n_sub = 0;                    // sub-indexes of kSubRows rows
    int64_t n_main = 0;               // rows [0, n_main) are indexed
    int64_t n_spilled = 0, n_ext = 0, max_spill = 0, ext_used = 0;   // bucket directory: keys outside their home bucket / with external lists
    // Cell postings of the tolerant lookup (tvz_tol_index_kernels.h), carried only while the handle asks for them
    // (t_cell > 0: the cell width this generation was built with): a classic directory over the CELL ids of the same
    // rows [0, n_main), built from the same snapshot, and the rows' 16-byte entries as they were at that snapshot.
    Directory cells;
    DevBuf<Row> irows;
    double t_cell = 0.0;
};

struct Index {
    Stream bstream;                   // background builds run here, not on the mutation stream
    Event snap_ev;
    Event build_ev;                   // polled by the builder (wait_stream_polling)
    IndexBuf buf[2];
    int cur = 0;                      // the generation matches read (valid only if `valid`)
    bool valid = false;
    int64_t n_delta = 0;
    int64_t builds = 0;
    DirHint key_hint, cell_hint;
    double tol_cell = 0.0;            // tvz_corpus_tol_index: > 0 = every build also makes cell postings of this width
    int64_t tol_builds = 0;           // builds that carried them
    std::unordered_map<int64_t, int32_t> delta_slot;   // row index -> slot in buf[cur].drows
    // build scratch (only the builder touches it)
    DevBuf<IxBuildInfo> info;
    DevBuf<uint32_t> fillc;           // per (entry, sub-index pair) fill cursors (unpartitioned build only)
    DevBuf<int64_t> pkeys;            // partitioned build: the (key, row) pairs grouped by directory slice
    DevBuf<uint32_t> prows;
    DevBuf<uint32_t> pcnt;            // per slice: pair counts | first pair (+1 entry) | scatter cursors
    DevBuf<Row> snap_rows;            // the row table as it was when a background build started
    DevBuf<int32_t> dead_rows;        // rows upserted during that build (dead in the new generation)
    // a background build is running (its thread has released the handle's lock)
    bool building = false;
    std::vector<int64_t> since_snap;  // rows upserted since its snapshot
    // PINNED host buffers: a copy to or from pageable memory makes the runtime wait for the stream
    // while it holds internal locks - a lookup issued meanwhile waited for the whole count pass
    Pinned<IxBuildInfo> h_info;       // read-back of `info`
    Pinned<Row> h_swap_rows;          // sources of the swap's two small copies: they stay untouched until
    Pinned<int32_t> h_swap_dead;      // the next swap, so the swap needs no synchronisation
    int64_t h_swap_cap = 0;
    std::condition_variable_any cv;   // signalled when it ends
    IndexBuf &now() { return buf[cur]; }
    const IndexBuf &now() const { return buf[cur]; }
};

}  // namespace

// Every GPU resource of the handle is a member that frees itself, in reverse order of declaration.
// tvz_corpus_destroy drains every stream first, so no order could free something in use; each struct
// still declares its streams first, then its events, then its buffers: buffers go first, streams last.
struct tvz_corpus {
    int device = 0;
    std::shared_mutex mu;        // exclusive: host bookkeeping of a mutation; shared: enqueueing a match
    std::mutex ev_mu;
    std::mutex stage_mu;
    // mutation stream: upsert payload copies + row swaps, in order
    Stream mstream;
    Event mut_done;              // re-recorded after every mutation; matches wait on it
    bool mut_any = false;
    // matches in flight (only compaction / reallocation / upload / destroy wait for them)
    static constexpr int kEvents = 32;
    Event events[kEvents];
    bool ev_pending[kEvents] = {};
    int ev_gen[kEvents] = {};    // index generation the match behind the event reads
    int ev_next = 0;
    DevBuf<int64_t> keys;
    DevBuf<Row> rows;
    std::vector<int64_t> h_keys;  // host mirror of the arena (for compaction)
    std::vector<Row> h_rows;
    std::unordered_map<int32_t, int64_t> first_row;  // video_id -> first row index
    int64_t live_keys = 0;
    RingSlot ring[kRingSlots];
    int ring_next = 0;
    std::vector<Staging *> free_staging;
    std::vector<Staging *> all_staging;   // every staging ever made (checked out or free)
    int64_t stage_rows = 0;          // rows the stagings are sized for
    Index ix;
    int64_t ix_next_try_rows = 0;    // a corpus without an index tries to build one from this size on
    // tvz_corpus_gap_index: a handle of its own whose rows are this one's rows in the same order, same ids, keys = the
    // rows' gap codes (tvz_gap_codes.h).  Owned; NULL while off.  Read under mu, changed under mu held exclusively;
    // its own lock is only ever taken with this one's held (parent, then child).
    tvz_corpus *gap = nullptr;
    double gap_eps = 0.0;
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// (re)allocate a device buffer of exactly n elements; old contents are lost
template <typename T>
int dev_alloc(DevBuf<T> &b, int64_t n) {
    if (b.p) (void)hipFree(b.p);
    b.cap = 0;
    if (hipMalloc(&b.p, (size_t)n * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();                  // not sticky: the next launch check must not report it
        b.p = nullptr;
        return tvz::fail(TVZ_ERR_NOMEM, "hipMalloc of %lld bytes failed", (long long)(n * (int64_t)sizeof(T)));
    }
    b.cap = n;
    return TVZ_OK;
}

// grow a device buffer (the caller has drained every reader); old contents [0, keep) survive
template <typename T>
int ensure(DevBuf<T> &b, int64_t need, int64_t keep) {
    if (need <= b.cap) return TVZ_OK;
    const int64_t cap = std::max<int64_t>({need, b.cap * 2, 1024});
    DevBuf<T> nb;
    if (int rc = dev_alloc(nb, cap)) return rc;
    if (b.p && keep > 0) {
        const hipError_t e = hipMemcpy(nb.p, b.p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e != hipSuccess)
            return tvz::fail(TVZ_ERR_HIP, "device copy while growing a corpus buffer failed: %s", hipGetErrorString(e));
    }
    std::swap(b.p, nb.p);                         // (nb frees the old buffer)
    std::swap(b.cap, nb.cap);
    return TVZ_OK;
}

// (re)allocate a pinned buffer of n elements, mapped into the device's address space if asked; old contents are lost
template <typename T>
int pinned_alloc(Pinned<T> &b, int64_t n, bool mapped) {
    if (b.h) (void)hipHostFree(b.h);
    b.h = b.d = nullptr;
    TVZ_HIP(hipHostMalloc(&b.h, (size_t)n * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault));
    if (mapped) TVZ_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&b.d), b.h, 0));
    return TVZ_OK;
}

// wait for every match enqueued so far and for the mutation stream (caller holds mu exclusively)
int drain(tvz_corpus *c) {
    {
        std::lock_guard<std::mutex> lk(c->ev_mu);
        for (int i = 0; i < tvz_corpus::kEvents; ++i)
            if (c->ev_pending[i]) {
                TVZ_HIP(hipEventSynchronize(c->events[i].e));
                c->ev_pending[i] = false;
            }
    }
    TVZ_HIP(hipStreamSynchronize(c->mstream.s));
    for (RingSlot &s : c->ring) s.pending = false;
    // single-query sweeps are not event-tracked (their caller waits for them itself): a few us each
    {
        std::lock_guard<std::mutex> lk(c->stage_mu);
        for (Staging *s : c->all_staging)
            while (s->busy.load(std::memory_order_acquire)) std::this_thread::yield();
    }
    return TVZ_OK;
}

int record(tvz_corpus *c, hipStream_t st) {
    std::lock_guard<std::mutex> lk(c->ev_mu);
    const int i = c->ev_next;
    c->ev_next = (i + 1) % tvz_corpus::kEvents;
    if (c->ev_pending[i]) TVZ_HIP(hipEventSynchronize(c->events[i].e));
    TVZ_HIP(hipEventRecord(c->events[i].e, st));
    c->ev_pending[i] = true;
    c->ev_gen[i] = c->ix.cur;
    return TVZ_OK;
}

// every sweep enqueued from now on sees the mutations that have returned (caller holds mu shared)
int wait_mutations(tvz_corpus *c, hipStream_t st) {
    if (c->mut_any) TVZ_HIP(hipStreamWaitEvent(st, c->mut_done.e, 0));
    return TVZ_OK;
}

static bool tvz_debug() { static const bool on = getenv("TVZ_DEBUG") != nullptr; return on; }
static double tvz_now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

}  // namespace
