// tvz_match.hip — timestamp-corpus matcher for MI355X (gfx950, wave64): host side.
//
// Replaces /root/reference inspector/db.py:76-94 (find_duplicates) and the per-prefix
// loop around it, inspector/app.py:231-255.  Semantics (db.py:85-91): for every corpus
// row, count the query elements that are `in` the row (exact float64 ==; the query keeps
// its multiplicity, the row acts as a set); a row is a hit iff count >= min_match.
//
// Device image of `video_timestamps` (db.py:21-27):
//   rows[r] = {key offset, key count, video_id}           16 B each, swapped by ONE store
//   keys    = arena of canonical float64 bit patterns (int64): per row sorted, unique,
//             NaN dropped, -0.0 folded to +0.0; every row starts 16-byte aligned.
// The arena is APPEND-ONLY between compactions: add_timestamps (db.py:43-64) copies the new
// keys to fresh arena space and then swaps the 16-byte row entry, both on the handle's mutation
// stream; matches enqueued later wait for that stream's event on the device.  Nothing on the
// upsert path waits for the host or for matches in flight (only a compaction or a growth of the
// arena beyond its reservation drains them).
//
// Kernels: tvz_match_kernels.h; the handle: tvz_handle.h; its index build: tvz_index_build.h.  No process-global
// mutable state: the sweep algorithm is a per-call argument and scratch is the caller's workspace.
#include <cfloat>
#include <optional>
#include <type_traits>

#include "tvz_match_kernels.h"
#include "tvz_index_kernels.h"
#include "tvz_index_wave_kernels.h"
#include "tvz_tol_kernels.h"
#include "tvz_tol_index_kernels.h"
#include "tvz_align_kernels.h"
#include "tvz_align_parts_kernels.h"
#include "tvz_gap_kernels.h"
#include "tvz_gap_long_kernels.h"
#include "tvz_gap.h"
#include "tvz_gap_shards.h"
#include "tvz_gap_rates.h"
#include "tvz_gap_rates_shards.h"
#include "tvz_gap_long.h"
#include "tvz_parts_flags.h"
#include "tvz_handle.h"
#include "tvz_index_build.h"

namespace {

// canonical, sorted, unique keys of one row appended to `out` (padded to an even count)
int64_t canon_row(const double *src, int64_t n, std::vector<int64_t> &out) {
    const size_t start = out.size();
    for (int64_t i = 0; i < n; ++i) {
        int64_t k;
        if (canon_key(src[i], k)) out.push_back(k);
    }
    std::sort(out.begin() + start, out.end());
    out.erase(std::unique(out.begin() + start, out.end()), out.end());
    const int64_t len = (int64_t)(out.size() - start);
    if (out.size() & 1) out.push_back(kEmpty);  // keep every row 16-byte aligned
    return len;
}

// whole host mirror -> device (caller holds mu exclusively and has drained)
int upload_all(tvz_corpus *c, int64_t want_rows, int64_t want_keys) {
    want_keys = std::max<int64_t>(want_keys, (int64_t)c->h_keys.size() + 2);
    want_rows = std::max<int64_t>(want_rows, (int64_t)c->h_rows.size() + 1);
    if (int rc = ensure(c->keys, want_keys, 0)) return rc;
    if (int rc = ensure(c->rows, want_rows, 0)) return rc;
    if (!c->h_keys.empty())
        TVZ_HIP(hipMemcpy(c->keys.p, c->h_keys.data(), c->h_keys.size() * 8, hipMemcpyHostToDevice));
    if (!c->h_rows.empty())
        TVZ_HIP(hipMemcpy(c->rows.p, c->h_rows.data(), c->h_rows.size() * sizeof(Row),
                          hipMemcpyHostToDevice));
    return TVZ_OK;
}

int compact(tvz_corpus *c) {
    std::vector<int64_t> nk;
    nk.reserve((size_t)c->live_keys + c->h_rows.size());
    for (Row &r : c->h_rows) {
        const int64_t off = (int64_t)nk.size();
        nk.insert(nk.end(), c->h_keys.begin() + r.off, c->h_keys.begin() + r.off + r.len);
        if (nk.size() & 1) nk.push_back(kEmpty);
        r.off = off;
    }
    c->h_keys.swap(nk);
    return upload_all(c, 0, 0);
}

// ---- single-query staging --------------------------------------------------------------------
// room for the hits of `rows` corpus rows (every block's region rounds up to whole row groups)
int staging_size(Staging *s, int64_t rows) {
    const int64_t slots = rows + (int64_t)kQ1MaxBlocks * kStageGroups;
    if (slots <= s->hit_slots) return TVZ_OK;
    // index lookups: one region of kSubRows hits and one count per sub-index
    const int64_t subs = tvz::ceil_div(std::max<int64_t>(rows, 1), kSubRows);
    s->hit_slots = 0;
    s->ix_slots = 0;
    if (int rc = pinned_alloc(s->hits, slots * 3, true)) return rc;
    if (int rc = pinned_alloc(s->ix_hits, subs * kSubRows * 3, true)) return rc;
    if (int rc = pinned_alloc(s->counts, kQ1MaxBlocks + subs, true)) return rc;
    s->hit_slots = slots;
    s->ix_slots = subs * kSubRows;
    return TVZ_OK;
}

int staging_new(tvz_corpus *c, Staging **out) {
    Staging *s = new Staging();
    struct Guard { Staging *s; ~Guard() { delete s; } } g{s};
    {                                    // single-query lookups: ahead of background index builds
        int least = 0, greatest = 0;
        TVZ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        TVZ_HIP(hipStreamCreateWithPriority(&s->stream.s, hipStreamNonBlocking, greatest));
    }
    if (int rc = pinned_alloc(s->query, kQueryStageKeys + 2, false)) return rc;
    if (int rc = ensure(s->d_query, kQueryStageKeys + 2, 0)) return rc;
    if (int rc = ensure(s->d_hits_n, 1, 0)) return rc;
    if (int rc = pinned_alloc(s->tol, (int64_t)kTolStageBytes, false)) return rc;
    if (int rc = ensure(s->d_tol, (int64_t)kTolStageBytes, 0)) return rc;
    if (int rc = staging_size(s, c->stage_rows)) return rc;
    g.s = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->stage_mu);
        c->all_staging.push_back(s);
    }
    *out = s;
    return TVZ_OK;
}

int staging_get(tvz_corpus *c, Staging **out) {
    {
        std::lock_guard<std::mutex> lk(c->stage_mu);
        if (!c->free_staging.empty()) {
            *out = c->free_staging.back();
            c->free_staging.pop_back();
            return TVZ_OK;
        }
    }
    return staging_new(c, out);   // more concurrent callers than pre-built stagings
}

void staging_put(tvz_corpus *c, Staging *s) {
    std::lock_guard<std::mutex> lk(c->stage_mu);
    c->free_staging.push_back(s);
}

// reserve device + staging capacity (caller holds mu exclusively; drains only if it must grow)
int reserve_locked(tvz_corpus *c, int64_t n_rows, int64_t n_keys) {
    if (n_keys + 2 > c->keys.cap || n_rows + 1 > c->rows.cap) {
        if (int rc = drain(c)) return rc;
        if (int rc = ensure(c->keys, n_keys + 2, (int64_t)c->h_keys.size())) return rc;
        if (int rc = ensure(c->rows, n_rows + 1, (int64_t)c->h_rows.size())) return rc;
    }
    // the host mirrors and maps follow the device reservation: inside it an upsert never reallocates
    // a vector or rehashes a map under the exclusive lock (growing the 32 MB key mirror of a 100k-row
    // corpus was a 9 ms stall for every lookup waiting for the lock)
    c->h_keys.reserve((size_t)c->keys.cap);
    c->h_rows.reserve((size_t)c->rows.cap);
    c->first_row.reserve((size_t)c->rows.cap);
    c->ix.delta_slot.reserve((size_t)delta_capacity(c->rows.cap));
    c->ix.since_snap.reserve((size_t)delta_capacity(c->rows.cap));
    if (delta_capacity(c->rows.cap) > c->ix.h_swap_cap) {
        Index &ix = c->ix;
        const int64_t cap = delta_capacity(c->rows.cap);
        ix.h_swap_cap = 0;
        if (int rc = pinned_alloc(ix.h_swap_rows, cap, false)) return rc;
        if (int rc = pinned_alloc(ix.h_swap_dead, cap, false)) return rc;
        ix.h_swap_cap = cap;
    }
    if (n_rows > c->stage_rows) {
        std::lock_guard<std::mutex> lk(c->stage_mu);
        c->stage_rows = n_rows;
        for (Staging *s : c->free_staging)
            if (int rc = staging_size(s, c->stage_rows)) return rc;
    }
    return TVZ_OK;
}

// ---- what a batched call hands to its launches (next to the Batch of tvz_common.h) ------------
// Plain aggregates.  `exclude_one`, the single-query exclusion, is no batch property: it stays an argument by name.
struct HitSink {                     // where the hits of the queries go
    int32_t cap;                     // hits a query's list holds
    int32_t *d_hits;                 // [Q][cap][3]
    int32_t *d_hits_n;               // [Q] counters, `ns` int32 apart
    int32_t ns;
    // the caller's dense counters / the workspace's one-counter-per-line scratch
    static HitSink dense(int32_t cap, int32_t *d_hits, int32_t *d_hits_n) { return {cap, d_hits, d_hits_n, 1}; }
    static HitSink per_line(int32_t cap, int32_t *d_hits, int32_t *counters) { return {cap, d_hits, counters, kCountStride}; }
};
struct JoinScratch {                 // the hash join's tables and, where the batch may hold long queries, their tail
    unsigned char *ws = nullptr;
    size_t ws_bytes = 0;
    unsigned char *lq = nullptr;
    size_t lq_bytes = 0;
};
struct TolSorted {                   // the tolerant calls' queries as ts_tol_sort_kernel (or the host) left them
    const double *sv;                // sorted values
    const int32_t *sp;               // their positions in the query
    const int32_t *qm;               // [Q] values per query; NULL: one query of m_one values
    int32_t m_one;
    int32_t lds_keys;                // > 0: every query has at most this many values, they go to LDS
    double tol;
};
const QByVal kNoQuery = {};          // a launch whose query does not travel in the kernel arguments
const HitSink kHostSink = HitSink::dense(0, nullptr, nullptr);   // ... whose hits go to pinned host memory (HostOut)

// ---- workspace layout of the batched calls -------------------------------------------------
struct JoinShape {
    int n_tiles = 0;
    int q_per_tile = 0;
    int s_log2 = 0;
    size_t bytes() const { return (size_t)n_tiles * ((size_t)4 << s_log2); }
};

// Tiles of up to 1024 queries whose elements fit a table of at most 2^19 four-byte slots (2 MiB:
// L2 resident) at load factor <= 0.55: one corpus sweep per tile.
JoinShape join_shape(int32_t Q, int32_t max_query_len) {
    JoinShape j;
    if (Q <= 0 || max_query_len <= 0) return j;
    int64_t qpt = (int64_t)(0.55 * (double)((int64_t)1 << kJoinMaxSlotsLog2)) / max_query_len;
    qpt = std::max<int64_t>(1, std::min<int64_t>(qpt, kJoinQ));
    qpt = std::min<int64_t>(qpt, Q);
    j.q_per_tile = (int)qpt;
    j.n_tiles = (int)tvz::ceil_div(Q, qpt);
    j.s_log2 = 12;
    while (j.s_log2 < kJoinMaxSlotsLog2 && (double)((int64_t)1 << j.s_log2) * 0.55 < (double)qpt * max_query_len) ++j.s_log2;
    return j;
}

// ---- the one carver of every workspace layout ----
// Walks a caller's buffer: the base is aligned up to 256 once, then take<T>(count) hands out regions, each rounded to 256
// bytes.  used() is what the regions occupy from the aligned base on; walked from NULL that is what a sizing function
// starts from.  The caller's base need not be aligned, so every size adds slack for it - in one of three ways, all of
// them part of the ABI (callers size buffers with the answers):
//   + 256          WsLayout::total: a whole line for the base.
//   + 255          the `fixed` of a front part (TolFront): the most the base's alignment can cost.
//   256 + 2 * 255  kTolWsSlack, tol_ws_bytes: a line for the base and, since the sorted queries take whatever is left
//                  (tol_ws_room divides it by TolWs::kPerKey), the most the roundings of their two regions can cost.
// The slack of a front part and that of the TolWs behind it simply add up (tvz_match_tol_topk_workspace_bytes).
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
    const unsigned char *base;
    uintptr_t p0, p;
    explicit Carver(const void *b) : base(static_cast<const unsigned char *>(b)), p0(al256(reinterpret_cast<uintptr_t>(b))), p(p0) {}
    template <typename T>
    T *take(size_t count) {
        T *r = reinterpret_cast<T *>(p);
        p += al256(count * sizeof(T));
        return r;
    }
    size_t used() const { return (size_t)(p - p0); }
    size_t fixed() const { return used() + 255; }       // as a front part: what it costs a caller's buffer at most
    // of a buffer of `bytes` at the base: what lies behind the regions taken so far
    size_t left(size_t bytes) const {
        const uintptr_t end = reinterpret_cast<uintptr_t>(base) + bytes;
        return end > p ? (size_t)(end - p) : 0;
    }
};

// scratch the long queries of a batch need (ts_longq_sort_kernel): per query of n keys a power-of-two sort buffer
// (< 2 n x 8 B), n + 1 distinct keys (8 B) and multiplicities (4 B), a counter; T = keys of all long queries, L = how many
inline size_t longq_bytes_bound(int64_t T, int64_t L) { return (size_t)(28 * T + 64 * L + 512); }

struct WsLayout {
    unsigned char *join = nullptr;  size_t join_bytes = 0;
    int32_t *counters = nullptr;    // [Q] one per 128-byte line
    int32_t *hits = nullptr;        // [Q][cap][3]
    int32_t *hits_n = nullptr;      // [Q]
    int32_t *local = nullptr;       // [Q][k+1][3]
    int32_t *gathered = nullptr;    // [n_ranks][Q][k+1][3]
    int32_t *flags = nullptr;       // [Q] queries the one-wave top-k left to the block kernels
    int32_t *pair = nullptr;        // [2][Q][k+1][3] fused lookup: the index's block + the delta sweep's, merged into `local`
    unsigned char *longq = nullptr; // scratch of the batch's long queries (> 4,095 timestamps): LAST, so that a larger
    size_t longq_bytes = 0;         //   workspace (tvz_match_workspace_bytes_long) simply has more of it: its whole tail
    size_t total = 0;
    HitSink sink(int32_t cap) const { return HitSink::per_line(cap, hits, counters); }
    JoinScratch scratch() const { return {join, join_bytes, longq, longq_bytes}; }
};

// the layout in a workspace of `bytes` at `base`; from NULL: its size
WsLayout ws_layout(void *base, size_t bytes, int32_t Q, int32_t max_query_len, int32_t cap, int32_t k, int32_t n_ranks,
                   int64_t total_query_keys = 0) {
    WsLayout w;
    Carver cv(base);
    const int32_t true_max_len = max_query_len;
    if (max_query_len > kMaxQueryLen) max_query_len = kMaxQueryLen;   // longer queries do not use the tables
    w.join_bytes = join_shape(Q, max_query_len).bytes();
    w.join = cv.take<unsigned char>(w.join_bytes);
    w.counters = cv.take<int32_t>((size_t)Q * kCountStride);
    if (k > 0) {
        const size_t block = (size_t)Q * (size_t)(k + 1) * 3;
        w.hits = cv.take<int32_t>((size_t)Q * (size_t)cap * 3);
        w.hits_n = cv.take<int32_t>((size_t)Q);
        w.local = cv.take<int32_t>(block);
        w.gathered = cv.take<int32_t>((size_t)(n_ranks > 1 ? n_ranks : 1) * block);
        w.flags = cv.take<int32_t>((size_t)Q);
        if (k <= kIxTkMaxK) w.pair = cv.take<int32_t>(2 * block);
    }
    if (true_max_len > kMaxQueryLen) {
        // without the batch's key count: room for ONE query of max_query_len keys (tvz_match_workspace_bytes);
        // with it (tvz_match_workspace_bytes_long): for any split of the keys into long queries
        const int64_t T = total_query_keys > 0 ? total_query_keys : (int64_t)true_max_len;
        const int64_t L = std::min<int64_t>(Q > 0 ? Q : 1, T / (kMaxQueryLen + 1) + 1);
        w.longq_bytes = cv.left(bytes);
        w.longq = cv.take<unsigned char>(longq_bytes_bound(T, L));
    }
    w.total = cv.used() + 256;
    return w;
}

// Dispatch, from the A/B grid profiles/r2_match_ab.txt (C in 5k..100k x Q in 16..1024): the
// per-query sweep only for a lone query (each query streams the corpus once; from a handful of
// queries on, sharing one LDS table per 16 wins); the hash join once its fixed cost (2 MiB table
// clear + build, ~40 us) is amortised - from about 3 M (query, row) pairs at 64+ queries it is
// 1.1x (C=50k x Q=64) to 4.6x (C=100k x Q=1024) faster than the LDS tile; the tile in between and
// for min_match outside 1..2.
constexpr int kQ1MaxQ = 1;
constexpr int kQ1SmallRows = 20000;       // up to 4 queries also sweep one by one below this
constexpr int kJoinMinQ = 64;
// The hash join pays ~80 us per tile of 1024 queries before it reads a row (table build + launches);
// the LDS tile kernel pays per (tile of 16 queries, row).  Measured crossover
// (profiles/r3_ab_small_corpus.txt; rows x Q in 64..12000 x 64..4096): the join wins from
// ~2,100 rows for thousands of queries, ~3,400 rows for 256, ~7,400 rows for 64.
constexpr int64_t kJoinMinRows = 2100;
constexpr int64_t kJoinRowsTimesQ = 340000;

int pick_algo(int32_t algo, int32_t Q, int64_t n_rows, int32_t max_query_len, int32_t min_match) {
    const bool join_legal = min_match >= 1 && min_match <= 2 && max_query_len > 0;
    if (algo == TVZ_ALGO_AUTO) {
        if (Q <= kQ1MaxQ || (Q <= 4 && n_rows <= kQ1SmallRows)) return TVZ_ALGO_Q1;
        if (join_legal && Q >= kJoinMinQ && n_rows >= kJoinMinRows + kJoinRowsTimesQ / Q) return TVZ_ALGO_JOIN;
        return TVZ_ALGO_TILE;
    }
    if (algo == TVZ_ALGO_JOIN && !join_legal) return TVZ_ALGO_TILE;   // documented: min_match <= 2 only
    return algo;
}

// the status of the launch just enqueued
int launched() {
    TVZ_HIP(hipGetLastError());
    return TVZ_OK;
}

int launch_prep(int32_t *d_hits_n, int32_t ns, int32_t Q, void *ones, size_t ones_bytes, void *zeros,
                size_t zero_bytes, hipStream_t st) {
    const size_t work = std::max<size_t>((size_t)Q, std::max(ones_bytes, zero_bytes) / 16);
    const int blocks = (int)std::min<size_t>(std::max<size_t>(1, tvz::ceil_div((int64_t)work, kBlock * 4)), 1024);
    hipLaunchKernelGGL(ts_prep_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_hits_n, ns, Q,
                       reinterpret_cast<uint4 *>(ones), ones_bytes / 16,
                       reinterpret_cast<uint4 *>(zeros), zero_bytes / 16);
    return launched();
}

// hit counters of Q queries = 0
int zero_counts(const HitSink &out, int32_t Q, hipStream_t st) {
    return launch_prep(out.d_hits_n, out.ns, Q, nullptr, 0, nullptr, 0, st);
}

// The rows a sweep reads: the whole row table, or the delta table of an indexed corpus.
struct RowSpan {
    const Row *p;
    int64_t n;
};

int launch_join(tvz_corpus *c, RowSpan span, bool zero, const Batch &b, const HitSink &out, const JoinScratch &scratch,
                hipStream_t st) {
    const int64_t n_rows = span.n;
    const JoinShape j = join_shape(b.Q, b.max_query_len);
    if (scratch.ws == nullptr || scratch.ws_bytes < j.bytes())
        return tvz::fail(TVZ_ERR_WORKSPACE, "hash join needs a workspace of %zu bytes (got %zu): size it "
                                            "with tvz_match_workspace_bytes", j.bytes(), scratch.ws_bytes);
    uint32_t *table = reinterpret_cast<uint32_t *>(scratch.ws);
    // one launch: hit counters = 0, every table slot = free
    if (int rc = launch_prep(out.d_hits_n, out.ns, zero ? b.Q : 0, table, j.bytes(), nullptr, 0, st)) return rc;
    hipLaunchKernelGGL(ts_join_build_kernel, dim3((unsigned)tvz::ceil_div(b.Q, kBlock / 64)), dim3(kBlock), 0, st,
                       b.d_queries, b.d_q_offsets, b.Q, b.max_query_len, j.q_per_tile, j.s_log2, table, out.d_hits_n, out.ns);
    TVZ_HIP(hipGetLastError());
    // ONE launch per tile, each filling the chip (two 16-wave blocks per CU): tiles that ran side by
    // side (a 2-D grid) had their 2 MiB tables compete for the same 4 MiB of L2 - 4 tiles cost
    // 0.69 ms per 1024 queries instead of 0.51.  A small shard gets one row per wave rather than
    // fewer, longer-lived waves: a row is ~5 dependent round trips, and on a 12.5k-row shard (100k
    // videos over 8 GPUs) that latency is the sweep.
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(512, tvz::ceil_div(n_rows, kJoinWaves)));
    for (int t = 0; t < j.n_tiles; ++t) {
        hipLaunchKernelGGL(ts_match_join_kernel, dim3((unsigned)chunks), dim3(kJoinBlock), kJoinLds, st, span.p,
                           n_rows, c->keys.p, b.d_queries, b.d_q_offsets, table, j.s_log2, b.Q, j.q_per_tile, t,
                           b.min_match, b.d_exclude_ids, out.cap, out.d_hits, out.d_hits_n, out.ns);
        TVZ_HIP(hipGetLastError());
    }
    return TVZ_OK;
}

// launch(std::integral_constant<int, kth_mode(min_match)>{}): the one place a launch turns min_match into its kernel's
// MODE.  COUNT = false: the kernel has no count-only form, its callers admit min_match 1..5 only.
template <bool COUNT = true, typename Launch>
int by_mode(int32_t min_match, Launch &&launch) {
    switch (kth_mode(min_match)) {
    case kModeM2: return launch(std::integral_constant<int, kModeM2>{});
    case kModeTop5: return launch(std::integral_constant<int, kModeTop5>{});
    }
    if constexpr (COUNT) return launch(std::integral_constant<int, kModeCount>{});
    else return tvz::fail(TVZ_ERR_UNSUPPORTED, "internal: min_match %d without a count-only kernel", (int)min_match);
}

template <bool HOSTOUT>
int launch_q1(tvz_corpus *c, RowSpan span, const Batch &b, int32_t exclude_one, const HitSink &out, int blocks_x,
              HostOut ho, hipStream_t st, const QByVal *byval = nullptr) {
    const QByVal &qv = byval ? *byval : kNoQuery;
    const int64_t n_rows = span.n;
    const int s_log2 = q1_slots_log2(b.max_query_len);
    const size_t lds = q1_lds_bytes(s_log2);
    // The launch limit, named: a workgroup gets at most 160 KiB of LDS on gfx950, and this
    // kernel's request is dynamic (query table + Bloom words, up to 112 KiB at 4095 timestamps) PLUS static
    // (the per-block hit staging, 3 KiB) - a launch beyond it fails in the runtime with an error string that
    // names neither.  (One launch of this kernel did fail on 2026-10-04 in a working tree between two commits,
    // "out of memory" in test_golden_kat, gpurun_out/r3_t12.log: that tree is not in the history; the two
    // resources a launch can run out of are this one and scratch, and tests/test_codeobj_cpu.py now pins the
    // kernel's scratch at 0 bytes.)
    TVZ_REQUIRE(lds + kQ1StaticLds <= (size_t)kLdsPerWorkgroup,
                "single-query sweep: %zu B of dynamic + %d B of static LDS exceed the %d B a gfx950 workgroup can have",
                lds, kQ1StaticLds, kLdsPerWorkgroup);
    const dim3 grid((unsigned)blocks_x, (unsigned)b.Q);
    return by_mode(b.min_match, [&](auto mode) {
        hipLaunchKernelGGL((ts_match_q1_kernel<mode.value, HOSTOUT>), grid, dim3(kQ1Block), lds, st, span.p, n_rows,
                           c->keys.p, b.d_queries, b.d_q_offsets, b.min_match, b.d_exclude_ids, exclude_one, out.cap,
                           out.d_hits, out.d_hits_n, out.ns, s_log2, ho, qv);
        return launched();
    });
}

int q1_blocks(int64_t n_rows, int32_t Q) {
    // every row group gets >= 1 row; about 8 blocks per CU in total over the Q block columns
    int64_t b = tvz::ceil_div(n_rows, kQ1Groups);
    const int64_t per_q = std::max<int64_t>(256, kQ1MaxBlocks / std::max(1, Q));
    b = std::max<int64_t>(1, std::min(b, per_q));
    return (int)b;
}

// min_match > 5: the hits left with kth = -2 - row (a row of `rows`) are resolved by a walk of the row
int launch_kth_fixup(tvz_corpus *c, const Row *rows, const Batch &b, const HitSink &out, hipStream_t st) {
    hipLaunchKernelGGL(ts_kth_fixup_kernel, dim3((unsigned)b.Q), dim3(kBlock), 0, st, rows, c->keys.p, b.d_queries,
                       b.d_q_offsets, b.min_match, out.cap, out.d_hits, out.d_hits_n, out.ns);
    return launched();
}

// one sweep of `span` with a resolved scan algorithm (Q1 / TILE / JOIN); appends to the hit lists
int launch_scan(tvz_corpus *c, RowSpan span, int a, bool zero, const Batch &b, const HitSink &out,
                const JoinScratch &scratch, hipStream_t st) {
    const int64_t n_rows = span.n;
    if (zero && (n_rows == 0 || a != TVZ_ALGO_JOIN))
        if (int rc = zero_counts(out, b.Q, st)) return rc;
    if (n_rows == 0 || b.Q == 0) return TVZ_OK;
    if (a == TVZ_ALGO_JOIN) return launch_join(c, span, zero, b, out, scratch, st);
    if (a == TVZ_ALGO_Q1) {
        if (int rc = launch_q1<false>(c, span, b, /* exclude_one */ -1, out, q1_blocks(n_rows, b.Q), HostOut{nullptr, nullptr, 0}, st))
            return rc;
    } else {
        // queries per tile: as many as keep the shared table at load <= 0.5 (at most 16)
        int nq = b.max_query_len > 0 ? kTileMaxEntries / b.max_query_len : kTileQ;
        nq = std::max(1, std::min(nq, kTileQ));
        const int64_t tiles = tvz::ceil_div(b.Q, nq);
        // one 1024-thread block per CU (LDS): aim at just under two full rounds of 256 blocks (a
        // third, mostly empty round costs a whole block time), but >= 2 rows per 16-lane group so
        // that building the tile's table (per block) stays a small part of the block's life
        int64_t chunks = std::max<int64_t>(1, 512 / tiles);
        chunks = std::min(chunks, std::max<int64_t>(1, n_rows / (2 * kTileGroups)));
        const int64_t rpb = tvz::round_up(tvz::ceil_div(n_rows, chunks), kTileGroups);
        chunks = tvz::ceil_div(n_rows, rpb);
        if (tiles > 65535)
            return tvz::fail(TVZ_ERR_UNSUPPORTED, "too many query tiles (%lld)", (long long)tiles);
        auto tile = b.min_match <= 2 ? ts_match_tile_kernel<false> : ts_match_tile_kernel<true>;
        hipLaunchKernelGGL(tile, dim3((unsigned)chunks, (unsigned)tiles), dim3(kTileBlock), kTileLds, st, span.p, n_rows,
                           c->keys.p, b.d_queries, b.d_q_offsets, b.Q, nq, b.min_match, b.d_exclude_ids, out.cap, out.d_hits,
                           out.d_hits_n, out.ns, (int32_t)rpb);
        TVZ_HIP(hipGetLastError());
    }
    if (b.min_match > kTop) return launch_kth_fixup(c, span.p, b, out, st);
    return TVZ_OK;
}

// the index answers every min_match >= 1: 1..5 from the smallest query positions kept per candidate,
// more than 5 by count + the kth fix-up walk (min_match <= 0 makes every row a hit: a sweep's job)
bool index_usable(const tvz_corpus *c, int32_t min_match) {
    return c->ix.valid && min_match >= 1;
}


// How many sub-indexes one block walks.  A big batch gives every query ONE block (the query's keys
// are probed once and the hit list needs no atomics); a small batch spreads a query over up to
// n_sub blocks so that the chip is filled and a lone query's latency is one sub-index deep.
int index_subs_per_block(int32_t Q, int n_sub, int32_t max_query_len, bool hostout) {
    int groups = hostout ? n_sub : (int)std::min<int64_t>(n_sub, std::max<int64_t>(1, tvz::ceil_div(2048, std::max(Q, 1))));
    int spb = (int)tvz::ceil_div(n_sub, std::max(groups, 1));
    while (spb > 1 && ix_lds_bytes(max_query_len, spb) > (size_t)kIxMaxLds) --spb;
    return std::max(spb, 1);
}

// index lookup of Q queries.  *alone_out = the kernel OWNS the hit counters (one block per query:
// it stores them; nothing has to be zeroed before).  Otherwise the blocks ADD to the queries'
// counters, which this zeroes first - or, HOSTOUT, every sub-index writes its own region and count.
// Callers check index_usable first: min_match >= 1, so min_match > 5 is the only count-only case (the
// kth fix-up below), and HOSTOUT (tvz_find_duplicates) only ever sees 1..5.
template <bool HOSTOUT>
int launch_index(tvz_corpus *c, const Batch &b, int32_t exclude_one, const HitSink &out, hipStream_t st,
                 const QByVal *byval = nullptr) {
    const IndexBuf &ix = c->ix.now();
    const int spb = index_subs_per_block(b.Q, ix.n_sub, b.max_query_len, HOSTOUT);
    const int groups = (int)tvz::ceil_div(ix.n_sub, spb);
    if (!HOSTOUT && groups > 1)
        if (int rc = zero_counts(out, b.Q, st)) return rc;
    const size_t lds = ix_lds_bytes(b.max_query_len, spb);
    if (int rc = by_mode<!HOSTOUT>(b.min_match, [&](auto mode) {
            hipLaunchKernelGGL((ts_match_index_kernel<HOSTOUT, mode.value>), dim3((unsigned)b.Q, (unsigned)groups),
                               dim3(kIxBlock), lds, st, ix.keys.dir.p, ix.keys.bits(), ix.keys.ks, ix.keys.post_ptr(), ix.ivid.p,
                               ix.n_main, ix.n_sub, spb, b.d_queries, b.d_q_offsets, b.max_query_len, b.min_match,
                               b.d_exclude_ids, exclude_one, out.cap, out.d_hits, out.d_hits_n, out.ns,
                               byval ? *byval : kNoQuery);
            return launched();
        }))
        return rc;
    // (the fix-up's rows are of the MAIN table: unchanged since the build, or they would be dead in the index; it runs
    // here, before a delta sweep appends codes of its own table)
    if (!HOSTOUT && b.min_match > kTop) return launch_kth_fixup(c, c->rows.p, b, out, st);
    return TVZ_OK;
}

// Can the lookup keep the per-shard top-k itself (ts_match_index_topk_kernel)?  One block per query
// over all sub-indexes, kth known inside the block (min_match 1..5), k <= 64.
bool index_topk_usable(const tvz_corpus *c, int32_t Q, int32_t max_query_len, int32_t min_match, int32_t k) {
    if (!c->ix.valid || min_match < 1 || min_match > kTop || k < 1 || k > kIxTkMaxK || Q < 1) return false;
    if (max_query_len > kMaxQueryLen) return false;
    const IndexBuf &ix = c->ix.now();
    if (index_subs_per_block(Q, ix.n_sub, max_query_len, false) != ix.n_sub) return false;   // a query over several blocks
    return ix_lds_bytes(max_query_len, ix.n_sub, true) <= (size_t)kIxMaxLds;
}

// Can the one-wave lookup (tvz_index_wave_kernels.h) answer the batch?  A handle of ONE sub-index (a rank's share of
// an 8-way sharded 100k-video table) of up to kWqRows rows in the bucket format, queries of up to kWqMaxLen timestamps,
// and what the fused lookup takes (index_topk_usable).
bool wave_usable(const tvz_corpus *c, int32_t max_query_len, int32_t min_match, int32_t k, int32_t algo) {
    if (!kWqUsable || !c->ix.valid || (algo != TVZ_ALGO_AUTO && algo != TVZ_ALGO_INDEX)) return false;
    const IndexBuf &ix = c->ix.now();
    return ix.n_sub == 1 && ix.keys.nb > 0 && ix.n_main <= kWqRows && max_query_len <= kWqMaxLen && min_match >= 1 &&
           min_match <= kTop && k <= kIxTkMaxK;
}

// (A separate probe pass in front of this kernel - every directory probe of the batch in one launch, the
// lookup blocks starting from coalesced records - was measured in round 4 and lost: the lookup got 10.7 us
// faster on a 1/8 shard, the probe pass cost 27 us: profiles/r4_probe_prepass.txt.)
int launch_index_topk(tvz_corpus *c, const Batch &b, int32_t cap, int32_t k, int32_t *d_block, bool wave, int32_t flags,
                      hipStream_t st) {
    const IndexBuf &ix = c->ix.now();
    const int32_t Q = b.Q, max_query_len = b.max_query_len;
    // wave (wave_usable and asked for): one WAVE per query - no barriers, every probe of the query in flight at once,
    // the postings in registers between the passes.
    if (wave) {
        const size_t lds = wq_lds_bytes(max_query_len);
        return by_mode<false>(b.min_match, [&](auto mode) {
            hipLaunchKernelGGL((ts_match_wq_topk_kernel<mode.value>), dim3((unsigned)Q), dim3(64), lds, st, ix.keys.dir.p,
                               ix.keys.bits(), ix.keys.post_ptr(), ix.ivid.p, ix.n_main, b.d_queries, b.d_q_offsets, Q,
                               max_query_len, b.min_match, b.d_exclude_ids, cap, k, d_block);
            return launched();
        });
    }
    // Two queries per block - their directory probes share the block's one probe phase (profiles/r4_pair.txt) -
    // when the LDS of both still leaves four blocks on a CU, and when half as many blocks still fill the chip
    // (256 CUs x 4 blocks: below that a batch is one round of blocks, and blocks twice as long would only make it
    // twice as long).
    const int one = max_query_len > 0 ? max_query_len : 1;
    const size_t lds2 = ix_lds_bytes(2 * one, ix.n_sub, true);
    const bool no_pair = (flags & TVZ_ALGO_NO_PAIR) != 0, force_pair = (flags & TVZ_ALGO_PAIR) != 0;   // per call, like the algorithm
    // (On a handle of ONE sub-index pairs answered a stream of batches sooner - 42 against 46 us - and a lone batch
    // later - 66 against 62: streams of batches take the wave kernel there now, so the block kernel's default on such
    // a handle is the shape that answers a lone batch soonest.)
    const bool pair = Q >= 2 && ((Q >= 2 * kIxResidentBlocks && ix.keys.nb == 0) || force_pair) &&
                      lds2 + 256 <= (size_t)kLdsPerWorkgroup / 4 && !no_pair;   // (+ the body's static LDS)
    const size_t lds = pair ? lds2 : ix_lds_bytes(max_query_len, ix.n_sub, true);
    const unsigned grid = pair ? (unsigned)((Q + 1) / 2) : (unsigned)Q;
    return by_mode<false>(b.min_match, [&](auto mode) {
        auto lookup = pair ? ts_match_index_topk_kernel<mode.value, 2> : ts_match_index_topk_kernel<mode.value, 1>;
        hipLaunchKernelGGL(lookup, dim3(grid), dim3(kIxBlock), lds, st, ix.keys.dir.p, ix.keys.bits(), ix.keys.ks,
                           ix.keys.post_ptr(), ix.ivid.p, ix.n_main, ix.n_sub, b.d_queries, b.d_q_offsets, Q, max_query_len,
                           b.min_match, b.d_exclude_ids, cap, k, d_block);
        return launched();
    });
}

int launch_match_short(tvz_corpus *c, const Batch &b, const HitSink &out, const JoinScratch &scratch, int32_t algo,
                       hipStream_t st) {
    const int32_t Q = b.Q, max_query_len = b.max_query_len, min_match = b.min_match;
    if (int rc = wait_mutations(c, st)) return rc;
    RowSpan span{c->rows.p, (int64_t)c->h_rows.size()};
    bool zero = true;
    if (algo == TVZ_ALGO_INDEX && !index_usable(c, min_match))
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "TVZ_ALGO_INDEX: %s", c->ix.valid
                             ? "the index answers min_match >= 1 only" : "this corpus has no index (tvz_corpus_build_index)");
    if ((algo == TVZ_ALGO_AUTO || algo == TVZ_ALGO_INDEX) && index_usable(c, min_match) && Q > 0) {
        // unchanged rows through the index, rows added or replaced since its build through a sweep
        // of the delta table - a row is in exactly one of the two
        if (int rc = launch_index<false>(c, b, /* exclude_one */ -1, out, st)) return rc;
        if (c->ix.n_delta == 0) return TVZ_OK;
        span = RowSpan{c->ix.now().drows.p, c->ix.n_delta};
        zero = false;
        algo = TVZ_ALGO_AUTO;
    }
    int a = pick_algo(algo, Q, span.n, max_query_len, min_match);
    // AUTO never fails for want of scratch: without the join's tables it takes the LDS tile
    if (a == TVZ_ALGO_JOIN && algo == TVZ_ALGO_AUTO &&
        (scratch.ws == nullptr || scratch.ws_bytes < join_shape(Q, max_query_len).bytes()))
        a = TVZ_ALGO_TILE;
    return launch_scan(c, span, a, zero, b, out, scratch, st);
}

// sorted distinct canonical keys + multiplicities of one query (what ts_match_longq_kernel searches)
void sorted_distinct(const double *q, int64_t n, std::vector<int64_t> &uq, std::vector<int32_t> &mult) {
    std::vector<int64_t> sk;
    sk.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        int64_t k;
        if (canon_key(q[i], k)) sk.push_back(k);
    }
    std::sort(sk.begin(), sk.end());
    uq.clear();
    mult.clear();
    for (size_t i = 0; i < sk.size(); ++i) {
        if (!uq.empty() && uq.back() == sk[i]) ++mult.back();
        else { uq.push_back(sk[i]); mult.push_back(1); }
    }
}

// db.py:87 has no limit on the length of new_timestamps.  A batch that holds queries of more than
// 4095 timestamps (a video with thousands of cuts: rare) takes this detour: the host reads the
// offsets back - the one place a batched call synchronises and allocates - the short queries go
// the normal way (which marks the long ones INT32_MIN), and every long query is then swept on its
// own: its sorted distinct keys + multiplicities are searched per row key (ts_match_longq_kernel),
// kth resolved by the fix-up walk - the path tvz_find_duplicates takes for such a query.
int launch_match_with_long(tvz_corpus *c, const Batch &b, const HitSink &out, const JoinScratch &scratch, int32_t algo,
                           hipStream_t st) {
    const int32_t Q = b.Q, min_match = b.min_match;
    unsigned char *lq = scratch.lq;
    // The ONE synchronisation of this path: the host has to learn which queries are long (their launches are
    // shaped by their lengths).  Everything after it is enqueued: no allocation (the scratch is a tail of the
    // caller's workspace), no further copy, no wait - VERDICT r4 item 7.
    std::vector<int64_t> h_off((size_t)Q + 1);
    TVZ_HIP(hipMemcpyAsync(h_off.data(), b.d_q_offsets, ((size_t)Q + 1) * 8, hipMemcpyDeviceToHost, st));
    TVZ_HIP(hipStreamSynchronize(st));
    int64_t short_max = 0;
    std::vector<int32_t> longs;
    for (int32_t q = 0; q < Q; ++q) {
        const int64_t n = h_off[(size_t)q + 1] - h_off[(size_t)q];
        TVZ_REQUIRE(n >= 0 && n <= INT32_MAX, "query %d has a bad length", q);
        if (n > kMaxQueryLen) longs.push_back(q);
        else short_max = std::max(short_max, n);
    }
    if (int rc = launch_match_short(c, Batch{b.d_queries, b.d_q_offsets, Q, (int32_t)short_max, min_match, b.d_exclude_ids}, out,
                                    scratch, algo, st))
        return rc;
    if (longs.empty()) return TVZ_OK;
    const int64_t n_rows = (int64_t)c->h_rows.size();
    // places in the long-query area: the counters of distinct keys, then per query its sort scratch, distinct keys
    // and multiplicities (8-byte units for the int64 arrays, 4-byte units for the int32 ones)
    std::vector<LongQ> table(longs.size());
    size_t cursor = (longs.size() * 4 + 15) & ~(size_t)15;
    for (size_t i = 0; i < longs.size(); ++i) {
        const int32_t q = longs[i];
        const int64_t n = h_off[(size_t)q + 1] - h_off[(size_t)q];
        if (n > ((int64_t)1 << 22))
            return tvz::fail(TVZ_ERR_UNSUPPORTED, "query %d of a batch has %lld timestamps: more than 4,194,304 are taken "
                             "one query at a time (tvz_find_duplicates)", q, (long long)n);
        int64_t p2 = 1;
        while (p2 < n) p2 <<= 1;
        LongQ &e = table[i];
        e.q_off = h_off[(size_t)q];
        e.n = (int32_t)n;
        e.pow2 = (int32_t)p2;
        e.m_at = (int64_t)i;
        e.sort_at = (int64_t)(cursor / 8);
        cursor += (size_t)p2 * 8;
        e.uq_at = (int64_t)(cursor / 8);
        cursor += (size_t)(n + 1) * 8;
        e.mult_at = (int64_t)(cursor / 4);
        cursor = (cursor + (size_t)(n + 1) * 4 + 15) & ~(size_t)15;
    }
    if (lq == nullptr || cursor > scratch.lq_bytes)
        return tvz::fail(TVZ_ERR_WORKSPACE, "the batch's %zu queries of more than %d timestamps need %zu bytes of scratch, the "
                         "workspace has %zu for them: size it with tvz_match_workspace_bytes_long (the batch's key count)",
                         longs.size(), kMaxQueryLen, cursor, lq ? scratch.lq_bytes : (size_t)0);
    int64_t *area = reinterpret_cast<int64_t *>(lq);
    for (size_t i0 = 0; i0 < table.size(); i0 += kLongPerLaunch) {
        LongQTable t{};
        const size_t cnt = std::min<size_t>(kLongPerLaunch, table.size() - i0);
        for (size_t i = 0; i < cnt; ++i) t.e[i] = table[i0 + i];
        hipLaunchKernelGGL(ts_longq_sort_kernel, dim3((unsigned)cnt), dim3(kLongSortBlock), 0, st, b.d_queries, t, area);
        TVZ_HIP(hipGetLastError());
    }
    for (size_t i = 0; i < longs.size(); ++i) {
        const int32_t q = longs[i];
        const LongQ &e = table[i];
        const HitSink one{out.cap, out.d_hits + (int64_t)q * out.cap * 3, out.d_hits_n + (size_t)q * out.ns, out.ns};
        if (int rc = zero_counts(one, 1, st)) return rc;    // un-poison: 0 hits so far
        if (!n_rows) continue;
        // (no distinct key: min_match <= 0 makes every row a hit with count 0, db.py:90: 0 >= min_match)
        hipLaunchKernelGGL(ts_match_longq_kernel, dim3((unsigned)tvz::ceil_div(n_rows, kGroupsPerBlock)), dim3(kBlock),
                           0, st, c->rows.p, n_rows, c->keys.p, area + e.uq_at, reinterpret_cast<int32_t *>(lq) + e.mult_at,
                           0, min_match, -1, one.cap, one.d_hits, one.d_hits_n, reinterpret_cast<int32_t *>(lq) + e.m_at,
                           b.d_exclude_ids ? b.d_exclude_ids + q : nullptr);
        TVZ_HIP(hipGetLastError());
        if (min_match > 0) {
            hipLaunchKernelGGL(ts_kth_fixup_kernel, dim3(1), dim3(kBlock), 0, st, c->rows.p, c->keys.p, b.d_queries,
                               b.d_q_offsets + q, min_match, one.cap, one.d_hits, one.d_hits_n, one.ns);
            TVZ_HIP(hipGetLastError());
        }
    }
    return TVZ_OK;
}

int launch_match(tvz_corpus *c, const Batch &b, const HitSink &out, const JoinScratch &scratch, int32_t algo,
                 hipStream_t st) {
    TVZ_REQUIRE(algo >= TVZ_ALGO_AUTO && algo <= TVZ_ALGO_INDEX, "unknown algo %d", algo);
    if (b.max_query_len > kMaxQueryLen) {
        if (int rc = wait_mutations(c, st)) return rc;
        return launch_match_with_long(c, b, out, scratch, algo, st);
    }
    return launch_match_short(c, b, out, scratch, algo, st);
}

// ---- the top-k launchers (forms and kernels: tvz_topk_kernels.h) ----
constexpr int kTopkFallbackBlocks = 256 * 5;     // the block kernels behind the one-wave kernel: a chip-full, grid-stride

int check_topk_k(int32_t k) {
    TVZ_REQUIRE(k >= 1 && k <= kSortCap / 2, "k=%d out of range [1, %d]", k, kSortCap / 2);
    return TVZ_OK;
}

// one hit list per query (plain) / with its counter, into a block (shard)
int launch_topk_local(const int32_t *d_hits, const int32_t *d_hits_n, int32_t ns, int32_t Q, int32_t cap,
                      int32_t k, int32_t *d_out, TopkForm form, int32_t *d_flags, hipStream_t st) {
    // with a flag array (the batched calls' workspace): short lists by one wave each, the block kernel
    // follows with a small grid for the queries that were flagged
    const int32_t *flags = nullptr;
    unsigned grid = (unsigned)Q;
    if (d_flags && k <= kWsK) {
        hipLaunchKernelGGL(ts_topk_wave_kernel, dim3((unsigned)tvz::ceil_div(Q, kBlock / 64)), dim3(kBlock), 0, st,
                           d_hits, d_hits_n, ns, 1, Q, cap, k, d_out, form, nullptr, d_flags, 0);
        flags = d_flags;
        grid = (unsigned)std::min<int64_t>(Q, kTopkFallbackBlocks);
    }
    if (k <= kSelSmallK)
        hipLaunchKernelGGL(ts_topk_select_kernel<4 * kSelSmallK>, dim3(grid), dim3(kBlock), 0, st, d_hits,
                           d_hits_n, ns, Q, cap, k, d_out, form, flags);
    else
        hipLaunchKernelGGL(ts_topk_select_kernel<kSortCap>, dim3(grid), dim3(kBlock), 0, st, d_hits,
                           d_hits_n, ns, Q, cap, k, d_out, form, flags);
    TVZ_HIP(hipGetLastError());
    return TVZ_OK;
}

// merge of n_lists per-rank blocks of k + 1 rows (merge) / top-k over n_lists lists (plain)
int launch_topk_lists(const int32_t *d_lists, const int32_t *d_lists_n, int32_t n_lists, int32_t Q, int32_t cap,
                      int32_t k, int32_t *d_topk, TopkForm form, int32_t *d_totals, hipStream_t st) {
    if (form == kTopkMerge && n_lists <= kMsMaxLists && k <= kMsMaxK) {
        // the gathered blocks are sorted (tvz_match_topk / tvz_topk_shard wrote them): a k-way merge, 64 / G queries
        // per wave, instead of a selection over an unordered set
        int G = 1;
        while (G < n_lists) G <<= 1;
        const unsigned blocks = (unsigned)tvz::ceil_div((int64_t)Q * G, 64);
        const size_t lds = (size_t)64 * (3 * (size_t)k + 1) * 4;
#define TVZ_MS(GG) hipLaunchKernelGGL(ts_topk_merge_sorted_kernel<GG>, dim3(blocks), dim3(64), lds, st, d_lists, n_lists, Q, k, d_topk, d_totals)
        switch (G) {
            case 1: TVZ_MS(1); break;
            case 2: TVZ_MS(2); break;
            case 4: TVZ_MS(4); break;
            case 8: TVZ_MS(8); break;
            default: TVZ_MS(16); break;
        }
#undef TVZ_MS
        TVZ_HIP(hipGetLastError());
        return TVZ_OK;
    }
    if (form == kTopkMerge && k <= kWsK && (int64_t)n_lists * k <= kWsMax) {
        // n_lists x k entries fit one wave's registers: no block kernel, no flags
        hipLaunchKernelGGL(ts_topk_wave_kernel, dim3((unsigned)tvz::ceil_div(Q, kBlock / 64)), dim3(kBlock), 0, st,
                           d_lists, nullptr, 1, n_lists, Q, cap, k, d_topk, form, d_totals, nullptr, 0);
        TVZ_HIP(hipGetLastError());
        return TVZ_OK;
    }
    hipLaunchKernelGGL(ts_topk_kernel, dim3((unsigned)Q), dim3(kBlock), 0, st, d_lists, d_lists_n, n_lists, Q,
                       cap, k, d_topk, form, d_totals);
    TVZ_HIP(hipGetLastError());
    return TVZ_OK;
}

// the index lookup's block and the delta table's, side by side in pair_blocks -> one block; a total above hit_cap
// is negated: the one hit list of an unfused match would have overflowed
int launch_topk_pair(const int32_t *pair_blocks, int32_t Q, int32_t k, int32_t hit_cap, int32_t *d_out, hipStream_t st) {
    hipLaunchKernelGGL(ts_topk_wave_kernel, dim3((unsigned)tvz::ceil_div(Q, kBlock / 64)), dim3(kBlock), 0, st,
                       pair_blocks, nullptr, 1, 2, Q, k + 1, k, d_out, kTopkPair, nullptr, nullptr, hit_cap);
    TVZ_HIP(hipGetLastError());
    return TVZ_OK;
}

int check_batch_args(tvz_corpus *c, const Batch &b, int32_t cap) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    TVZ_REQUIRE(b.Q >= 0 && b.Q <= 65535, "Q=%d out of range [0, 65535]", b.Q);
    TVZ_REQUIRE(b.max_query_len >= 0 && cap >= 0, "negative size");
    TVZ_REQUIRE(b.Q == 0 || b.d_q_offsets, "NULL query offsets");
    TVZ_REQUIRE(b.d_queries || b.max_query_len == 0 || b.Q == 0, "d_queries is NULL");
    return TVZ_OK;
}

}  // namespace

// used by tvz_comm.hip (same shared object, not exported)
int tvz_match_topk_local(tvz_corpus *c, const Batch &b, int32_t cap, int32_t k, int32_t *d_out, Workspace ws,
                         int32_t n_ranks, int32_t algo, void *hip_stream, ShardBlocks *blocks) {
    const int32_t Q = b.Q, max_query_len = b.max_query_len, min_match = b.min_match;
    if (int rc = check_batch_args(c, b, cap)) return rc;
    if (int rc = check_topk_k(k)) return rc;
    constexpr int32_t kShape = TVZ_ALGO_PAIR | TVZ_ALGO_NO_PAIR | TVZ_ALGO_WAVE | TVZ_ALGO_NO_WAVE | TVZ_ALGO_PREFER_WAVE;
    const int32_t flags = algo & kShape;                                  // shape of the fused lookup (tvz.h)
    algo &= ~kShape;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(ws.p != nullptr, "d_workspace is NULL");
    const WsLayout w = ws_layout(ws.p, ws.bytes, Q, max_query_len, cap, k, n_ranks);
    if (ws.bytes < w.total)
        return tvz::fail(TVZ_ERR_WORKSPACE, "workspace of %zu bytes, need %zu", ws.bytes, w.total);
    if (d_out == nullptr) d_out = w.local;
    if (blocks) *blocks = ShardBlocks{d_out, w.gathered};
    const HitSink out = w.sink(cap);   // (one-counter-per-line scratch: the select kernel reads it as it is)
    DeviceGuard dg(c->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const bool wave_ok = wave_usable(c, max_query_len, min_match, k, algo);
    if ((flags & TVZ_ALGO_WAVE) && !wave_ok)          // asked for by name: say why not, instead of quietly taking another path
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "TVZ_ALGO_WAVE: the one-wave lookup takes an indexed handle of ONE sub-index "
                         "(this one: %d) of up to %d rows, queries of up to %d timestamps (max_query_len %d), min_match 1..5, "
                         "k <= %d", c->ix.valid ? c->ix.now().n_sub : 0, kWqRows, kWqMaxLen, max_query_len, kIxTkMaxK);
    const bool wave = wave_ok && (flags & (TVZ_ALGO_WAVE | TVZ_ALGO_PREFER_WAVE)) && !(flags & (TVZ_ALGO_NO_WAVE | TVZ_ALGO_PAIR));
    if ((algo == TVZ_ALGO_AUTO || algo == TVZ_ALGO_INDEX) && index_topk_usable(c, Q, max_query_len, min_match, k)) {
        // the lookup keeps the k best itself: no hit list, no top-k launch.  Rows added or replaced since
        // the build are swept as usual; their block and the lookup's are merged (k + 1 rows each).
        if (int rc = wait_mutations(c, st)) return rc;
        const int64_t n_delta = c->ix.n_delta;
        int32_t *blk = n_delta ? w.pair : d_out;
        if (int rc = launch_index_topk(c, b, cap, k, blk, wave, flags, st)) return rc;
        if (n_delta) {
            const RowSpan span{c->ix.now().drows.p, n_delta};
            int a = pick_algo(TVZ_ALGO_AUTO, Q, span.n, max_query_len, min_match);
            if (int rc = launch_scan(c, span, a, true, b, out, w.scratch(), st)) return rc;
            int32_t *blk2 = w.pair + (size_t)Q * (size_t)(k + 1) * 3;
            if (int rc = launch_topk_local(out.d_hits, out.d_hits_n, out.ns, Q, cap, k, blk2, kTopkShard, w.flags, st)) return rc;
            if (int rc = launch_topk_pair(w.pair, Q, k, cap, d_out, st)) return rc;
        }
        return record(c, st);
    }
    if (int rc = launch_match(c, b, out, w.scratch(), algo, st)) return rc;
    if (int rc = launch_topk_local(out.d_hits, out.d_hits_n, out.ns, Q, cap, k, d_out, kTopkShard, w.flags, st)) return rc;
    return record(c, st);
}

// a kernel may ask for up to `bytes` of dynamic LDS
template <typename K>
int max_dynamic_lds(K *kernel, int bytes) {
    TVZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return TVZ_OK;
}

static int tvz_corpus_create_impl(tvz_corpus **out, int device) {
    TVZ_REQUIRE(out != nullptr, "out is NULL");
    int n = 0;
    TVZ_HIP(hipGetDeviceCount(&n));
    TVZ_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
    DeviceGuard dg(device);
    tvz_corpus *c = new tvz_corpus();
    c->device = device;
    struct Guard { tvz_corpus *c; ~Guard() { if (c) (void)tvz_corpus_destroy(c); } } g{c};
    for (Event &ev : c->events) TVZ_HIP(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
    TVZ_HIP(hipStreamCreateWithFlags(&c->mstream.s, hipStreamNonBlocking));
    TVZ_HIP(hipEventCreateWithFlags(&c->mut_done.e, hipEventDisableTiming));
    {   // background index builds: their own stream, lowest priority (lookups and upserts go first).
        // Created here, not at the first rebuild: creating a stream takes milliseconds and holds
        // runtime locks a lookup in flight would wait for
        int least = 0, greatest = 0;
        TVZ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        TVZ_HIP(hipStreamCreateWithPriority(&c->ix.bstream.s, hipStreamNonBlocking, least));
        TVZ_HIP(hipEventCreateWithFlags(&c->ix.snap_ev.e, hipEventDisableTiming));
        TVZ_HIP(hipEventCreateWithFlags(&c->ix.build_ev.e, hipEventDisableTiming));
        if (int rc = dev_alloc(c->ix.info, 1)) return rc;
        if (int rc = pinned_alloc(c->ix.h_info, 1, false)) return rc;
    }
    for (RingSlot &s : c->ring) {
        if (int rc = pinned_alloc(s.buf, kRingSlotKeys, false)) return rc;
        TVZ_HIP(hipEventCreateWithFlags(&s.ev.e, hipEventDisableTiming));
    }
    if (int rc = max_dynamic_lds(ts_match_tile_kernel<false>, (int)kTileLds)) return rc;
    if (int rc = max_dynamic_lds(ts_match_tile_kernel<true>, (int)kTileLds)) return rc;
    if (int rc = max_dynamic_lds(ts_match_join_kernel, (int)kJoinLds)) return rc;
    for (auto *k : {ts_match_index_kernel<false, kModeM2>, ts_match_index_kernel<false, kModeTop5>,
                    ts_match_index_kernel<false, kModeCount>, ts_match_index_kernel<true, kModeM2>,
                    ts_match_index_kernel<true, kModeTop5>})
        if (int rc = max_dynamic_lds(k, kIxMaxLds)) return rc;
    for (auto *k : {ts_match_index_topk_kernel<kModeM2, 1>, ts_match_index_topk_kernel<kModeTop5, 1>,
                    ts_match_index_topk_kernel<kModeM2, 2>, ts_match_index_topk_kernel<kModeTop5, 2>})
        if (int rc = max_dynamic_lds(k, kIxMaxLds)) return rc;
    if (int rc = max_dynamic_lds(ts_match_wq_topk_kernel<kModeM2>, (int)wq_lds_bytes(kWqMaxLen))) return rc;
    if (int rc = max_dynamic_lds(ts_match_wq_topk_kernel<kModeTop5>, (int)wq_lds_bytes(kWqMaxLen))) return rc;
    if (int rc = max_dynamic_lds(bk_slice_build_kernel, (int)kBkBuildLds)) return rc;
    if (int rc = max_dynamic_lds(ix_slice_count_kernel, (int)kIxSliceBytesMax)) return rc;
    if (int rc = max_dynamic_lds(ix_slice_fill_kernel, (int)kIxSliceBytesMax)) return rc;
    if (int rc = max_dynamic_lds(ix_scatter_kernel, kIxStagePairs * 12 + (3 * kIxMaxParts + 1) * 4)) return rc;
    if (int rc = max_dynamic_lds(ts_find_fused_kernel<false>, kIxMaxLds)) return rc;
    if (int rc = max_dynamic_lds(ts_find_fused_kernel<true>, kIxMaxLds)) return rc;
    for (auto *k : {ts_match_q1_kernel<kModeM2, false>, ts_match_q1_kernel<kModeM2, true>,
                    ts_match_q1_kernel<kModeTop5, false>, ts_match_q1_kernel<kModeTop5, true>,
                    ts_match_q1_kernel<kModeCount, false>, ts_match_q1_kernel<kModeCount, true>})
        if (int rc = max_dynamic_lds(k, (int)q1_lds_bytes(kQ1MaxLog2))) return rc;
    // default reservation: 64 Ki rows / 2 Mi keys (16 MiB) and two single-query stagings, so a
    // fresh service handles its first uploads without allocating on the hot calls
    c->stage_rows = 1 << 16;
    if (int rc = ensure(c->keys, (int64_t)1 << 21, 0)) return rc;
    if (int rc = ensure(c->rows, (int64_t)1 << 16, 0)) return rc;
    if (int rc = reserve_locked(c, ((int64_t)1 << 16) - 1, ((int64_t)1 << 21) - 2)) return rc;   // host mirrors, pinned buffers
    for (int i = 0; i < 2; ++i) {
        Staging *s = nullptr;
        if (int rc = staging_new(c, &s)) return rc;
        c->free_staging.push_back(s);
    }
    g.c = nullptr;
    *out = c;
    return TVZ_OK;
}

// ---- the gap codes of the rows (include/tvz_gap.h): a child handle kept in step with this one --------------------
static int tvz_corpus_destroy_impl(tvz_corpus *c);
static int tvz_corpus_upload_impl(tvz_corpus *c, const int32_t *h_video_ids, const int64_t *h_offsets, const double *h_keys,
                                  int64_t n_rows, int64_t n_keys);
static int tvz_corpus_upsert_impl(tvz_corpus *c, int32_t video_id, const double *h_keys, int64_t n);

namespace {

// the child's whole table from the parent's host mirror (caller holds the parent's mu exclusively; c->gap exists)
int gap_upload(tvz_corpus *c) {
    const int64_t n_rows = (int64_t)c->h_rows.size();
    std::vector<int32_t> ids((size_t)n_rows);
    std::vector<int64_t> offs((size_t)n_rows + 1, 0);
    std::vector<double> codes, vals;
    codes.reserve((size_t)c->live_keys);
    for (int64_t r = 0; r < n_rows; ++r) {
        const Row &row = c->h_rows[(size_t)r];
        ids[(size_t)r] = row.vid;
        tvz_gap::row_codes(c->h_keys.data() + row.off, row.len, c->gap_eps, vals, codes);
        offs[(size_t)r + 1] = (int64_t)codes.size();
    }
    return tvz_corpus_upload_impl(c->gap, ids.data(), offs.data(), codes.data(), n_rows, (int64_t)codes.size());
}

// one row's codes to the child, from the row's canonical keys (caller holds the parent's mu exclusively)
int gap_upsert(tvz_corpus *c, int32_t video_id, const int64_t *keys, int64_t len) {
    thread_local std::vector<double> codes, vals;
    codes.clear();
    tvz_gap::row_codes(keys, len, c->gap_eps, vals, codes);
    return tvz_corpus_upsert_impl(c->gap, video_id, codes.data(), (int64_t)codes.size());
}

}  // namespace

static int tvz_corpus_destroy_impl(tvz_corpus *c) {
    if (!c) return TVZ_OK;
    DeviceGuard dg(c->device);
    {
        std::unique_lock<std::shared_mutex> lk(c->mu);
        wait_no_build(c, lk);
        if (c->gap) {
            (void)tvz_corpus_destroy_impl(c->gap);
            c->gap = nullptr;
        }
        if (c->mstream.s) (void)drain(c);
        for (Staging *s : c->all_staging) delete s;
    }
    delete c;
    return TVZ_OK;
}

static int tvz_corpus_reserve_impl(tvz_corpus *c, int64_t n_rows, int64_t n_keys) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    TVZ_REQUIRE(n_rows >= 0 && n_keys >= 0, "negative size");
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    if (int rc = reserve_locked(c, n_rows, n_keys + n_rows /* padding to even row lengths */)) return rc;
    return c->gap ? tvz_corpus_reserve_impl(c->gap, n_rows, n_keys) : TVZ_OK;   // (a row has fewer codes than keys)
}

static int tvz_corpus_upload_impl(tvz_corpus *c, const int32_t *h_video_ids,
                                 const int64_t *h_offsets, const double *h_keys, int64_t n_rows,
                                 int64_t n_keys) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    TVZ_REQUIRE(n_rows >= 0 && n_keys >= 0, "negative size");
    TVZ_REQUIRE(n_rows < INT32_MAX - 2, "too many rows");
    TVZ_REQUIRE(n_rows == 0 || (h_video_ids && h_offsets), "NULL row arrays");
    TVZ_REQUIRE(n_keys == 0 || h_keys, "NULL keys");
    for (int64_t r = 0; r < n_rows; ++r) {
        TVZ_REQUIRE(h_offsets[r] <= h_offsets[r + 1] && h_offsets[r] >= 0 &&
                        h_offsets[r + 1] <= n_keys,
                    "offsets of row %lld are not monotone within [0, n_keys]", (long long)r);
        TVZ_REQUIRE(h_offsets[r + 1] - h_offsets[r] <= INT32_MAX, "row %lld too long", (long long)r);
        // videos.id is a Postgres serial (db.py:14); negative ids mark padding in the top-k lists
        TVZ_REQUIRE(h_video_ids[r] >= 0, "row %lld has a negative video_id (%d)", (long long)r,
                    h_video_ids[r]);
    }
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    if (int rc = drain(c)) return rc;
    c->h_keys.clear();
    c->h_rows.clear();
    c->first_row.clear();
    c->h_keys.reserve((size_t)n_keys + (size_t)n_rows);
    c->h_rows.reserve((size_t)n_rows);
    c->live_keys = 0;
    // canonicalise + sort + dedupe every row: independent per row, so a bulk load (the reload of a
    // 100k-row table: 20 M keys) is cut into row ranges for the host's cores; the ranges' key runs are
    // appended in row order afterwards
    const int n_thr = n_rows >= 8192 ? (int)std::min<int64_t>(16, std::max(1u, std::thread::hardware_concurrency())) : 1;
    struct Part { std::vector<int64_t> keys; std::vector<int32_t> lens; };
    std::vector<Part> parts((size_t)n_thr);
    auto canon_part = [&](int t) {       // rows [r0, r1) -> their canonical keys + lengths
        const int64_t r0 = n_rows * t / n_thr, r1 = n_rows * (t + 1) / n_thr;
        if (r0 == r1) return;            // (no rows: h_offsets may be NULL)
        Part &p = parts[(size_t)t];
        p.keys.reserve((size_t)(h_offsets[r1] - h_offsets[r0] + (r1 - r0)));
        p.lens.reserve((size_t)(r1 - r0));
        for (int64_t r = r0; r < r1; ++r)
            p.lens.push_back((int32_t)canon_row(h_keys + h_offsets[r], h_offsets[r + 1] - h_offsets[r], p.keys));
    };
    if (n_thr == 1) {
        canon_part(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < n_thr; ++t) pool.emplace_back(canon_part, t);
        for (std::thread &th : pool) th.join();
    }
    int64_t r = 0;
    for (const Part &p : parts) {
        int64_t off = (int64_t)c->h_keys.size();
        c->h_keys.insert(c->h_keys.end(), p.keys.begin(), p.keys.end());
        for (const int32_t len : p.lens) {
            const Row row{off, len, h_video_ids[r]};
            off += (len + 1) & ~(int64_t)1;                  // (canon_row pads every row to an even count)
            c->first_row.emplace(row.vid, r);
            c->h_rows.push_back(row);
            c->live_keys += len;
            ++r;
        }
    }
    // room for the table to double before anything has to grow
    const int64_t want_rows = 2 * n_rows + 1024, want_keys = 2 * (int64_t)c->h_keys.size() + 65536;
    if (int rc = upload_all(c, want_rows, want_keys)) return rc;
    if (int rc = reserve_locked(c, want_rows, want_keys)) return rc;
    // a failed index build leaves the corpus without one (every match sweeps): not an upload error
    (void)build_index(c);
    return c->gap ? gap_upload(c) : TVZ_OK;
}

static int tvz_corpus_upsert_impl(tvz_corpus *c, int32_t video_id, const double *h_keys, int64_t n) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    TVZ_REQUIRE(n >= 0 && n <= INT32_MAX && (n == 0 || h_keys), "bad key array");
    TVZ_REQUIRE(video_id >= 0, "negative video_id (%d)", video_id);
    DeviceGuard dg(c->device);
    // canonicalise + sort outside the lock
    thread_local std::vector<int64_t> tmp;
    tmp.clear();
    const int64_t len = canon_row(h_keys, n, tmp);
    const int64_t added = (int64_t)tmp.size();
    std::unique_lock<std::shared_mutex> lk(c->mu);
    Index &ix = c->ix;
    int64_t off, rows_before, r;
    bool is_new, gc, full;
    while (true) {
        off = (int64_t)c->h_keys.size();
        rows_before = (int64_t)c->h_rows.size();
        auto it = c->first_row.find(video_id);
        is_new = it == c->first_row.end();
        r = is_new ? rows_before : it->second;
        TVZ_REQUIRE(rows_before < INT32_MAX - 3, "too many rows");
        const int64_t rows_after = rows_before + (is_new ? 1 : 0);
        const int64_t live_after = c->live_keys + len - (is_new ? 0 : c->h_rows[r].len);
        // garbage-collect the arena when more than half of it is dead, or grow what is full: the only
        // paths that wait for matches in flight (amortised: reservations double)
        gc = off + added > 2 * (live_after + rows_after) + 4096;
        full = off + added + 2 > c->keys.cap || rows_after + 1 > c->rows.cap;
        const bool delta_full = ix.valid && ix.delta_slot.find(r) == ix.delta_slot.end() &&
                                ix.n_delta >= std::min<int64_t>(ix.now().drows.cap, delta_capacity(ix.now().n_main));
        if (!(gc || full || delta_full)) break;
        if (ix.building) {            // gc / growth would move what the build reads; a full delta table
            ix.cv.wait(lk);           // waits for the generation being built.  Then look again.
            continue;
        }
        if (!delta_full) break;
        // the delta table filled up before a rebuild could be started (it is started at half full):
        // rebuild now - the lock is released meanwhile - and look again
        if (rebuild_in_background(c, lk) != TVZ_OK) index_drop(c);      // no index: every match sweeps
    }
    // host mirror first; every failure below leaves host and device consistent again through
    // the full re-upload of the slow path, or rolls the host mirror back
    const Row old_row = is_new ? Row{0, 0, 0} : c->h_rows[r];
    c->h_keys.insert(c->h_keys.end(), tmp.begin(), tmp.end());
    const Row new_row{off, (int32_t)len, video_id};
    if (is_new) {
        c->h_rows.push_back(new_row);
        c->first_row.emplace(video_id, r);
    } else {
        c->h_rows[r] = new_row;
    }
    c->live_keys += len - (is_new ? 0 : old_row.len);
    // with an index: the row's current entry also goes to the delta table (which the sweeps read),
    // and an indexed row that changes for the first time has its stale postings marked dead
    int32_t slot = -1;
    bool slot_new = false;
    if (ix.valid) {
        auto ds = ix.delta_slot.find(r);
        if (ds != ix.delta_slot.end()) {
            slot = ds->second;
        } else {                       // room was checked above
            slot = (int32_t)ix.n_delta++;
            slot_new = true;
            ix.delta_slot.emplace(r, slot);
        }
    }
    auto rollback = [&]() {
        c->h_keys.resize((size_t)off);
        c->live_keys -= len - (is_new ? 0 : old_row.len);
        if (is_new) { c->h_rows.pop_back(); c->first_row.erase(video_id); }
        else c->h_rows[r] = old_row;
        if (slot_new) { ix.delta_slot.erase(r); --ix.n_delta; }
    };
    if (gc || full) {                  // no background build is running (see above)
        if (tvz_debug()) fprintf(stderr, "[tvz] upsert slow path: gc %d full %d (arena %lld, live %lld, rows %lld)\n", (int)gc,
                                 (int)full, (long long)c->h_keys.size(), (long long)c->live_keys, (long long)c->h_rows.size());
        int rc = drain(c);
        if (!rc) rc = gc ? compact(c) : TVZ_OK;
        if (!rc && !gc) rc = upload_all(c, 2 * (int64_t)c->h_rows.size() + 1024,
                                        2 * (int64_t)c->h_keys.size() + 65536);
        if (!rc) rc = reserve_locked(c, 2 * (int64_t)c->h_rows.size() + 1024, 0);
        if (rc) { rollback(); index_drop(c); return rc; }
        // compaction moved every row's keys: the delta table's offsets are stale - start afresh
        // (readers are drained anyway)
        if (ix.valid || (int64_t)c->h_rows.size() >= std::max(kIndexMinRows, c->ix_next_try_rows)) {
            c->ix_next_try_rows = 2 * (int64_t)c->h_rows.size();
            (void)build_index(c);
        }
        return c->gap ? gap_upsert(c, video_id, c->h_keys.data() + c->h_rows[r].off, len) : rc;
    }
    // fast path: payload -> pinned ring slot -> async copy into FRESH arena space -> 16-byte row
    // swap, all on the mutation stream; no wait for the host or for running matches
    if (added > kRingSlotKeys) {
        // a row too long for a ring slot (> 8192 cuts): copy straight from the mirror, synchronously
        hipError_t e = hipMemcpyAsync(c->keys.p + off, c->h_keys.data() + off, (size_t)added * 8,
                                      hipMemcpyHostToDevice, c->mstream.s);
        if (e == hipSuccess) e = hipStreamSynchronize(c->mstream.s);
        if (e != hipSuccess) {
            rollback();
            return tvz::fail(TVZ_ERR_HIP, "upsert copy failed: %s", hipGetErrorString(e));
        }
    } else if (added) {
        RingSlot &s = c->ring[c->ring_next];
        c->ring_next = (c->ring_next + 1) % kRingSlots;
        hipError_t e = hipSuccess;
        if (s.pending) e = hipEventSynchronize(s.ev.e);      // 16 upserts ago: long done
        if (e == hipSuccess) {
            memcpy(s.buf.h, tmp.data(), (size_t)added * 8);
            e = hipMemcpyAsync(c->keys.p + off, s.buf.h, (size_t)added * 8, hipMemcpyHostToDevice, c->mstream.s);
        }
        if (e == hipSuccess) e = hipEventRecord(s.ev.e, c->mstream.s);
        if (e != hipSuccess) {
            rollback();
            return tvz::fail(TVZ_ERR_HIP, "upsert copy failed: %s", hipGetErrorString(e));
        }
        s.pending = true;
    }
    hipError_t e = hipSuccess;
    if (slot >= 0) {
        const bool kills_postings = slot_new && r < ix.now().n_main;
        // A match in flight captured the delta table's size when it was enqueued: it does not sweep
        // this row's NEW delta entry, so it must still find the row through its postings.  Marking
        // them dead therefore waits - on the device - for every match enqueued so far; those matches
        // see the old row, every later one the new row, none neither (db.py:83 under Postgres MVCC
        // cannot lose a row either).
        if (kills_postings && stream_wait_readers(c, c->mstream.s) != TVZ_OK) e = hipErrorUnknown;
        if (e == hipSuccess)
            hipLaunchKernelGGL(ts_row_write3_kernel, dim3(1), dim3(1), 0, c->mstream.s, c->rows.p + r,
                               ix.now().drows.p + slot, kills_postings ? ix.now().ivid.p + r : nullptr, new_row);
    } else {
        hipLaunchKernelGGL(ts_row_write_kernel, dim3(1), dim3(1), 0, c->mstream.s, c->rows.p + r, new_row);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(c->mut_done.e, c->mstream.s);
    if (e != hipSuccess) {
        rollback();
        return tvz::fail(TVZ_ERR_HIP, "upsert row swap failed: %s", hipGetErrorString(e));
    }
    c->mut_any = true;
    if (ix.building) ix.since_snap.push_back(r);       // dead in the generation being built
    // the row's codes follow before the lock is let go of (a rebuild below releases it): the code table sees the
    // upserts in the order of the rows
    if (c->gap)
        if (int rc = gap_upsert(c, video_id, tmp.data(), len)) return rc;
    // time for a (new) index?  Built in the background by this thread: the lock is released while
    // the GPU builds, matches and other upserts go on
    const bool want = ix.valid ? ix.n_delta >= delta_trigger(ix.now().n_main)
                               : (int64_t)c->h_rows.size() >= std::max(kIndexMinRows, c->ix_next_try_rows);
    if (want && !ix.building) {
        c->ix_next_try_rows = 2 * (int64_t)c->h_rows.size();   // if this build fails: not at every upsert
        (void)rebuild_in_background(c, lk);            // a failed build leaves the current state in force
    }
    return TVZ_OK;
}

static int tvz_corpus_clear_impl(tvz_corpus *c) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    // Matches in flight keep sweeping the rows they were launched with: the memory stays valid, and
    // it stays UNCHANGED - the arena is reused from offset 0 by the next upsert, whose copy runs on
    // the mutation stream, so that stream is made to wait (on the device) for every match enqueued
    // so far.  No host stall.
    if (int rc = stream_wait_readers(c, c->mstream.s)) return rc;
    c->h_keys.clear();
    c->h_rows.clear();
    c->first_row.clear();
    c->live_keys = 0;
    index_drop(c);
    c->ix_next_try_rows = 0;
    return c->gap ? tvz_corpus_clear_impl(c->gap) : TVZ_OK;
}

static int tvz_corpus_stats_impl(tvz_corpus *c, int64_t *n_rows, int64_t *n_keys,
                                int64_t *arena_keys) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (n_rows) *n_rows = (int64_t)c->h_rows.size();
    if (n_keys) *n_keys = c->live_keys;
    if (arena_keys) *arena_keys = (int64_t)c->h_keys.size();
    return TVZ_OK;
}

static int tvz_corpus_build_index_impl(tvz_corpus *c) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    if (int rc = drain(c)) return rc;
    c->ix_next_try_rows = 2 * (int64_t)c->h_rows.size();
    return build_index(c);
}

static int tvz_corpus_index_stats_impl(tvz_corpus *c, int64_t *n_indexed, int64_t *n_delta, int64_t *n_post,
                                       int64_t *n_distinct, int64_t *n_builds) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const Index &ix = c->ix;
    if (n_indexed) *n_indexed = ix.valid ? ix.now().n_main : 0;
    if (n_delta) *n_delta = ix.valid ? ix.n_delta : 0;
    if (n_post) *n_post = ix.valid ? ix.now().keys.n_post : 0;
    if (n_distinct) *n_distinct = ix.valid ? ix.now().keys.n_distinct : 0;
    if (n_builds) *n_builds = ix.builds;
    return TVZ_OK;
}

static int tvz_corpus_tol_index_impl(tvz_corpus *c, double cell) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    if (!(cell == 0.0 || (cell >= TVZ_TOL_CELL_MIN && cell <= DBL_MAX)))     // refuses NaN, inf, negatives, tiny cells
        return tvz::fail(TVZ_ERR_INVALID, "cell must be 0 (off) or finite and >= %g s (got %g)", TVZ_TOL_CELL_MIN, cell);
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    Index &ix = c->ix;
    const double before = ix.tol_cell;
    ix.tol_cell = cell;
    if (cell == 0.0 || !ix.valid || ix.now().t_cell == cell) return TVZ_OK;   // off: the next build drops the postings
    int rc = drain(c);
    if (!rc) {
        c->ix_next_try_rows = 2 * (int64_t)c->h_rows.size();
        rc = build_index(c);
    }
    // a build that failed (no memory for the postings) leaves the handle as it was asked before this call - and, as
    // after any failed build, without an index until the next one: every match sweeps
    if (rc) ix.tol_cell = before;
    return rc;
}

static int tvz_corpus_tol_index_stats_impl(tvz_corpus *c, double *cell, int64_t *out) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const Index &ix = c->ix;
    const bool on = ix.valid && ix.now().t_cell > 0.0;
    if (cell) *cell = on ? ix.now().t_cell : 0.0;
    if (out) {
        out[0] = on ? ix.now().cells.n_distinct : 0;
        out[1] = on ? ix.now().cells.n_post : 0;
        out[2] = ix.tol_builds;
        out[3] = on ? ix.n_delta : 0;
    }
    return TVZ_OK;
}

static int tvz_match_impl(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
                         int32_t Q, int32_t max_query_len, int32_t min_match,
                         const int32_t *d_exclude_ids, int32_t cap, int32_t *d_hits,
                         int32_t *d_hits_n, void *d_workspace, size_t workspace_bytes, int32_t algo,
                         void *hip_stream) {
    const Batch b{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids};
    if (int rc = check_batch_args(c, b, cap)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_hits_n && (cap == 0 || d_hits), "NULL output");
    DeviceGuard dg(c->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    // with a workspace (tvz_match_workspace_bytes(Q, max_query_len, 0, 0, 1)) the sweeps count into
    // one-counter-per-cache-line scratch and may use the hash join; without one they fall back to
    // the caller's dense counters and the LDS kernels
    JoinScratch scratch;
    HitSink out = HitSink::dense(cap, d_hits, d_hits_n);
    if (d_workspace) {
        const WsLayout w = ws_layout(d_workspace, workspace_bytes, Q, max_query_len, cap, 0, 1);
        if (workspace_bytes >= w.total) {
            scratch = w.scratch();
            // (a lone query's counter shares its line with nobody: no gather launch)
            if (Q > 1) out = HitSink::per_line(cap, d_hits, w.counters);
        } else if (algo == TVZ_ALGO_JOIN) {
            return tvz::fail(TVZ_ERR_WORKSPACE, "workspace of %zu bytes, the hash join needs %zu: size it with "
                                                "tvz_match_workspace_bytes", workspace_bytes, w.total);
        }
    }
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (int rc = launch_match(c, b, out, scratch, algo, st)) return rc;
    if (out.ns != 1) {
        hipLaunchKernelGGL(ts_counts_gather_kernel, dim3((unsigned)tvz::ceil_div(Q, kBlock)), dim3(kBlock), 0, st,
                           out.d_hits_n, out.ns, d_hits_n, Q);
        TVZ_HIP(hipGetLastError());
    }
    return record(c, st);
}

static int tvz_match_topk_impl(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
                              int32_t Q, int32_t max_query_len, int32_t min_match,
                              const int32_t *d_exclude_ids, int32_t cap, int32_t k, int32_t *d_out,
                              void *d_workspace, size_t workspace_bytes, int32_t algo,
                              void *hip_stream) {
    TVZ_REQUIRE(d_out != nullptr || Q == 0, "d_out is NULL");
    return tvz_match_topk_local(c, Batch{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids}, cap, k, d_out,
                                Workspace{d_workspace, workspace_bytes}, 1, algo, hip_stream, nullptr);
}

namespace {

struct Hit { int32_t vid, cnt, kth; };

// the argument checks of tvz_find_duplicates and tvz_find_duplicates_tol
int check_find_args(const tvz_corpus *c, const double *h_query, int64_t n, int64_t cap, const int32_t *h_out_ids,
                    const int32_t *h_out_counts, const int64_t *n_out) {
    TVZ_REQUIRE(c != nullptr && n_out != nullptr, "NULL argument");
    TVZ_REQUIRE(n >= 0 && cap >= 0 && cap <= INT32_MAX, "bad size");
    TVZ_REQUIRE(n == 0 || h_query, "h_query is NULL");
    TVZ_REQUIRE(cap == 0 || (h_out_ids && h_out_counts), "NULL outputs");
    TVZ_REQUIRE(n <= INT32_MAX, "query too long");
    return TVZ_OK;
}

// eps and max_offset of tvz_align and of every form of the alignment top-k; *nb = the offset bins on either side of
// zero, at most max_bins in all.  A call whose limit is a constant of the header says so by its name (wide_limit).
int check_align_bins(double eps, double max_offset, int32_t max_bins, const char *wide_limit, int32_t *nb_out) {
    TVZ_REQUIRE(eps > 0.0 && max_offset >= 0.0, "eps must be > 0 and max_offset >= 0");
    const double nb = floor(max_offset / eps + 0.5);
    if (!(2 * nb + 1 <= max_bins)) {                    // also refuses max_offset = inf and NaN (eps = max_offset = inf)
        if (wide_limit)
            return tvz::fail(TVZ_ERR_UNSUPPORTED, "max_offset/eps = %.0f bins on either side of zero, above %s = %d", nb,
                             wide_limit, (max_bins - 1) / 2);
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "max_offset/eps = %.0f needs more than %d bins", nb, max_bins);
    }
    *nb_out = (int32_t)nb;
    return TVZ_OK;
}

// the rate list of the forms that take one: 1..kArMaxRates finite rates > 0 on the host -> the sweep's by-value argument
int check_align_rates(const double *h_rates, int32_t n_rates, AlRates *out) {
    if (n_rates < 1 || n_rates > kArMaxRates)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment top-k with rates: n_rates=%d outside 1..%d (TVZ_ALIGN_MAX_RATES)",
                         (int)n_rates, kArMaxRates);
    TVZ_REQUIRE(h_rates != nullptr, "h_rates is NULL");
    *out = AlRates{};
    for (int32_t i = 0; i < n_rates; ++i) {
        TVZ_REQUIRE(std::isfinite(h_rates[i]) && h_rates[i] > 0.0, "rate %d is %g: every rate must be finite and > 0", (int)i,
                    h_rates[i]);
        out->r[i] = h_rates[i];
    }
    out->n = n_rates;
    return TVZ_OK;
}

// a staging checked out for one call (staging_get fills s); it goes back on every exit
struct StagingLease {
    tvz_corpus *c;
    Staging *s = nullptr;
    ~StagingLease() { if (s) staging_put(c, s); }
};

// The output rules of the single-query calls: hits[0, n_have) sorted by (video_id, count, kth), the first `cap` of
// them written out, and *n_out = n_found - the true count, so that a truncated caller can retry with cap >= *n_out.
void copy_out(Hit *hits, int64_t n_have, int64_t n_found, int64_t cap, int32_t *h_out_ids, int32_t *h_out_counts,
              int32_t *h_out_kth, int64_t *n_out) {
    std::sort(hits, hits + n_have, [](const Hit &a, const Hit &b) {
        if (a.vid != b.vid) return a.vid < b.vid;
        if (a.cnt != b.cnt) return a.cnt < b.cnt;
        return a.kth < b.kth;
    });
    const int64_t w = std::min<int64_t>(n_have, cap);
    for (int64_t i = 0; i < w; ++i) {
        h_out_ids[i] = hits[i].vid;
        h_out_counts[i] = hits[i].cnt;
        if (h_out_kth) h_out_kth[i] = hits[i].kth;
    }
    *n_out = n_found;
}

// The pinned single-query sweep of tvz_find_duplicates (find_pinned) and tvz_find_duplicates_tol: the kernels write
// their hits into the staging's pinned, mapped memory, and ONE synchronisation waits for all of them.  For a corpus
// of n_rows > 0 rows, launch(n_rows, blocks, region) enqueues them on s->stream - under the shared lock, behind every
// mutation that has returned - and says where the sweep's hits land: `blocks` regions of `region` hits, counted in
// s->counts.  s->busy (drain() and its kin wait on it) is set just before the launch and cleared after the
// synchronisation or on any failure; the synchronisation is made outside the lock, so an upsert never waits behind
// it.  Leaves the sweep's hits compacted at the start of s->hits, *n_hits of them; `what` names the call in errors.
template <typename Launch>
int pinned_sweep(tvz_corpus *c, Staging *s, const char *what, Launch &&launch, int64_t *n_hits) {
    int blocks = 0, region = 0;
    {
        struct Busy { Staging *s; ~Busy() { s->busy.store(0, std::memory_order_release); } } busy{s};
        {
            std::shared_lock<std::shared_mutex> lk(c->mu);
            const int64_t n_rows = (int64_t)c->h_rows.size();
            if (n_rows) {
                if (n_rows > c->stage_rows || n_rows + (int64_t)kQ1MaxBlocks * kStageGroups > s->hit_slots ||
                    n_rows > s->ix_slots) {
                    // the corpus outgrew its reservation (see tvz_corpus_reserve): grow this staging
                    if (int rc = staging_size(s, std::max<int64_t>(2 * n_rows, c->stage_rows))) return rc;
                }
                if (int rc = wait_mutations(c, s->stream.s)) return rc;
                s->busy.store(1, std::memory_order_release);
                if (int rc = launch(n_rows, blocks, region)) return rc;
            }
        }
        // (polling the per-block counts from the host instead was tried: it needs a system-scope
        // release per block, which saved 1.5 us at 5k rows and cost 60 us at 100k)
        const hipError_t e = hipStreamSynchronize(s->stream.s);
        if (e != hipSuccess) return tvz::fail(TVZ_ERR_HIP, "%ssingle-query match failed: %s", what, hipGetErrorString(e));
    }
    // compact the per-block regions in place (block order; sorted by the caller anyway)
    Hit *hh = reinterpret_cast<Hit *>(s->hits.h);
    int64_t w = 0;
    for (int b = 0; b < blocks; ++b) {
        const int32_t nb = s->counts.h[b];
        if (nb < 0) return tvz::fail(TVZ_ERR_INVALID, "internal: %squery table overflow", what);
        const Hit *src = hh + (int64_t)b * region;
        if (src != hh + w) memmove(hh + w, src, (size_t)nb * sizeof(Hit));
        w += nb;
    }
    *n_hits = w;
    return TVZ_OK;
}

// tvz_find_duplicates of a query of up to 4,095 timestamps with min_match <= 5: ONE launch + ONE synchronisation
// (pinned_sweep); a query of up to 440 timestamps travels in the kernel arguments (no copy at all).  Leaves the hits
// at the start of s->hits, *n_hits of them.
int find_pinned(tvz_corpus *c, Staging *s, const double *h_query, int64_t n, int32_t min_match, int32_t excl,
                int64_t *n_hits) {
    *n_hits = 0;
    const bool by_value = n <= kQ1ByValKeys;
    QByVal qv;
    if (by_value) {
        qv.n = (int32_t)n;
        qv.pad = 0;
        if (n) memcpy(qv.k, h_query, (size_t)n * 8);
    } else {
        s->query.h[0] = 0;
        s->query.h[1] = n;
        memcpy(s->query.h + 2, h_query, (size_t)n * 8);
        TVZ_HIP(hipMemcpyAsync(s->d_query.p, s->query.h, (size_t)(n + 2) * 8, hipMemcpyHostToDevice, s->stream.s));
    }
    const double *dq = by_value ? nullptr : reinterpret_cast<const double *>(s->d_query.p + 2);
    const int64_t *dqo = by_value ? nullptr : s->d_query.p;
    const Batch one{dq, dqo, 1, (int32_t)n, min_match, nullptr};
    // with an index: rows unchanged since its build are answered by the lookup kernel (one
    // block), rows in the delta table by the sweep - both write to pinned host memory, one
    // synchronisation for the two.  A query the lookup refuses (> 4 G postings) is swept.
    for (int attempt = 0; attempt < 2; ++attempt) {
        int n_sub = 0;
        auto launch = [&](int64_t n_rows, int &blocks, int &region) -> int {
            RowSpan span{c->rows.p, n_rows};
            if (attempt == 0 && index_usable(c, min_match)) {
                const IndexBuf &ib = c->ix.now();
                n_sub = ib.n_sub;
                s->gen = c->ix.cur;
                span = RowSpan{ib.drows.p, c->ix.n_delta};
                const int s_log2 = q1_slots_log2((int32_t)n);
                const size_t lds = std::max(ix_lds_bytes((int32_t)n, 1), q1_lds_bytes(s_log2));
                if (span.n && lds <= (size_t)kIxMaxLds) {
                    // lookup + delta sweep in ONE launch (the streaming driver's call: its own row is
                    // always in the delta table)
                    constexpr int kFG = kIxBlock / kGroup;                // row groups per sweep block
                    blocks = (int)std::max<int64_t>(1, std::min<int64_t>(tvz::ceil_div(span.n, kFG), kQ1MaxBlocks));
                    region = (int)(tvz::ceil_div(span.n, (int64_t)blocks * kFG) * kFG);
                    const HostOut ho{s->hits.d, s->counts.d, region};
                    return by_mode<false>(min_match, [&](auto mode) -> int {
                        hipLaunchKernelGGL((ts_find_fused_kernel<mode.value == kModeTop5>), dim3((unsigned)(n_sub + blocks)),
                                           dim3(kIxBlock), lds, s->stream.s, ib.keys.dir.p, ib.keys.bits(), ib.keys.ks, ib.keys.post_ptr(),
                                           ib.ivid.p, ib.n_main, ib.n_sub, 1, n_sub, dq, dqo, (int32_t)n, min_match, excl,
                                           s->ix_hits.d, s->counts.d + kQ1MaxBlocks, span.p, span.n, c->keys.p, s_log2,
                                           ho, by_value ? qv : kNoQuery);
                        if (hipGetLastError() != hipSuccess) return tvz::fail(TVZ_ERR_HIP, "fused lookup launch failed");
                        return TVZ_OK;
                    });
                }
                // (one region and one count per sub-index)
                if (int rc = launch_index<true>(c, one, excl, HitSink::dense(0, s->ix_hits.d, s->counts.d + kQ1MaxBlocks),
                                                s->stream.s, by_value ? &qv : nullptr))
                    return rc;
            }
            if (!span.n) return TVZ_OK;
            blocks = q1_blocks(span.n, 1);
            region = (int)(tvz::ceil_div(span.n, (int64_t)blocks * kQ1Groups) * kQ1Groups);
            const HostOut ho{s->hits.d, s->counts.d, region};
            return launch_q1<true>(c, span, one, excl, kHostSink, blocks, ho, s->stream.s, by_value ? &qv : nullptr);
        };
        if (int rc = pinned_sweep(c, s, "", launch, n_hits)) return rc;
        bool refused = false;
        for (int b = 0; b < n_sub; ++b) refused = refused || s->counts.h[kQ1MaxBlocks + b] < 0;
        if (refused) continue;                                        // sweep everything instead
        Hit *hh = reinterpret_cast<Hit *>(s->hits.h);
        for (int b = 0; b < n_sub; ++b) {                              // the lookup's regions, one per sub-index
            const int64_t nb = std::min<int64_t>(s->counts.h[kQ1MaxBlocks + b], kSubRows);
            if (nb) memcpy(hh + *n_hits, reinterpret_cast<const Hit *>(s->ix_hits.h) + (int64_t)b * kSubRows,
                           (size_t)nb * sizeof(Hit));
            *n_hits += nb;
        }
        break;
    }
    return TVZ_OK;
}

// tvz_find_duplicates on the rare paths (min_match > 5, or a query longer than a tile): a device hit list, a fix-up
// pass for kth, explicit copies back, and the exclusion applied here.  *n_found: the hits the device reported, less
// the excluded ones (`hits` holds at most max(cap, 1) of them).
int find_device(tvz_corpus *c, Staging *s, const double *h_query, int64_t n, int32_t min_match, int32_t excl,
                int64_t cap, std::vector<Hit> &hits, int64_t *n_found) {
    const int64_t want = std::max<int64_t>(cap, 1);
    if (int rc = ensure(s->d_hits, want * 3, 0)) return rc;
    std::vector<int64_t> uq;
    std::vector<int32_t> mult;
    const bool longq = n > kMaxQueryLen;
    int64_t *d_q = s->d_query.p;
    if (longq) {
        // sorted distinct keys + multiplicities, searched per row key; the raw query (for the
        // fix-up walk) travels behind them
        sorted_distinct(h_query, n, uq, mult);
        const int64_t m = (int64_t)uq.size();
        if (int rc = ensure(s->d_sq, m + n + 3, 0)) return rc;
        if (int rc = ensure(s->d_smult, m + 1, 0)) return rc;
        d_q = s->d_sq.p + m;                                 // {0, n} + raw query
        const int64_t qoff[2] = {0, n};
        TVZ_HIP(hipMemcpyAsync(d_q, qoff, 16, hipMemcpyHostToDevice, s->stream.s));
        TVZ_HIP(hipMemcpyAsync(d_q + 2, h_query, (size_t)n * 8, hipMemcpyHostToDevice, s->stream.s));
        if (m) {
            TVZ_HIP(hipMemcpyAsync(s->d_sq.p, uq.data(), (size_t)m * 8, hipMemcpyHostToDevice, s->stream.s));
            TVZ_HIP(hipMemcpyAsync(s->d_smult.p, mult.data(), (size_t)m * 4, hipMemcpyHostToDevice, s->stream.s));
        }
    } else {
        s->query.h[0] = 0;
        s->query.h[1] = n;
        if (n) memcpy(s->query.h + 2, h_query, (size_t)n * 8);
        TVZ_HIP(hipMemcpyAsync(s->d_query.p, s->query.h, (size_t)(n + 2) * 8, hipMemcpyHostToDevice, s->stream.s));
    }
    {
        std::shared_lock<std::shared_mutex> lk(c->mu);
        const int64_t n_rows = (int64_t)c->h_rows.size();
        if (int rc = wait_mutations(c, s->stream.s)) return rc;
        const HitSink out = HitSink::dense((int32_t)want, s->d_hits.p, s->d_hits_n.p);
        if (int rc = zero_counts(out, 1, s->stream.s)) return rc;
        if (n_rows) {
            if (longq) {
                hipLaunchKernelGGL(ts_match_longq_kernel, dim3((unsigned)tvz::ceil_div(n_rows, kGroupsPerBlock)),
                                   dim3(kBlock), 0, s->stream.s, c->rows.p, n_rows, c->keys.p, s->d_sq.p,
                                   s->d_smult.p, (int32_t)uq.size(), min_match, -1, (int32_t)want, s->d_hits.p,
                                   s->d_hits_n.p, static_cast<const int32_t *>(nullptr), static_cast<const int32_t *>(nullptr));
                TVZ_HIP(hipGetLastError());
                if (min_match > 0) {
                    hipLaunchKernelGGL(ts_kth_fixup_kernel, dim3(1), dim3(kBlock), 0, s->stream.s, c->rows.p,
                                       c->keys.p, reinterpret_cast<const double *>(d_q + 2), d_q, min_match,
                                       (int32_t)want, s->d_hits.p, s->d_hits_n.p, 1);
                    TVZ_HIP(hipGetLastError());
                }
            } else {
                // min_match > 5 (or <= 0): what a batch of one takes - on an indexed handle the lookup with a
                // count-only pass B + the kth fix-up walk and a sweep of the delta table, else the single-query
                // sweep; the fix-ups are part of those paths
                const Batch one{reinterpret_cast<const double *>(d_q + 2), d_q, 1, (int32_t)n, min_match, nullptr};
                if (int rc = launch_match_short(c, one, out, JoinScratch{}, TVZ_ALGO_AUTO, s->stream.s)) return rc;
            }
        }
        if (int rc = record(c, s->stream.s)) return rc;
    }
    int32_t h_n = 0;
    TVZ_HIP(hipMemcpyAsync(&h_n, s->d_hits_n.p, 4, hipMemcpyDeviceToHost, s->stream.s));
    TVZ_HIP(hipStreamSynchronize(s->stream.s));   // also: uq / mult / h_query were read by now
    *n_found = h_n;
    hits.resize((size_t)std::min<int64_t>(h_n, want));
    if (!hits.empty()) {
        TVZ_HIP(hipMemcpyAsync(hits.data(), s->d_hits.p, hits.size() * 12, hipMemcpyDeviceToHost, s->stream.s));
        TVZ_HIP(hipStreamSynchronize(s->stream.s));
    }
    if (excl >= 0) {
        const size_t before = hits.size();
        hits.erase(std::remove_if(hits.begin(), hits.end(), [&](const Hit &h) { return h.vid == excl; }), hits.end());
        *n_found -= (int64_t)(before - hits.size());
    }
    return TVZ_OK;
}

}  // namespace

static int tvz_find_duplicates_impl(tvz_corpus *c, const double *h_query, int64_t n,
                                   int32_t min_match, int32_t exclude_id, int64_t cap,
                                   int32_t *h_out_ids, int32_t *h_out_counts, int32_t *h_out_kth,
                                   int64_t *n_out) {
    if (int rc = check_find_args(c, h_query, n, cap, h_out_ids, h_out_counts, n_out)) return rc;
    DeviceGuard dg(c->device);
    StagingLease lease{c};
    if (int rc = staging_get(c, &lease.s)) return rc;
    const int32_t excl = exclude_id >= 0 ? exclude_id : -1;
    int64_t n_found = 0;                   // hits the device reported (before the cap)
    if (n <= kMaxQueryLen && min_match <= kTop) {
        if (int rc = find_pinned(c, lease.s, h_query, n, min_match, excl, &n_found)) return rc;
        copy_out(reinterpret_cast<Hit *>(lease.s->hits.h), n_found, n_found, cap, h_out_ids, h_out_counts, h_out_kth,
                 n_out);
    } else {
        std::vector<Hit> hits;             // only the rare paths use it
        if (int rc = find_device(c, lease.s, h_query, n, min_match, excl, cap, hits, &n_found)) return rc;
        copy_out(hits.data(), (int64_t)hits.size(), n_found, cap, h_out_ids, h_out_counts, h_out_kth, n_out);
    }
    return TVZ_OK;
}

static int tvz_topk_impl(const int32_t *d_lists, const int32_t *d_lists_n, int32_t n_lists,
                        int32_t Q, int32_t cap, int32_t k, int32_t *d_topk, void *hip_stream) {
    TVZ_REQUIRE(n_lists >= 1 && Q >= 0 && cap >= 0, "bad list shape");
    if (int rc = check_topk_k(k)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE((d_lists || cap == 0) && d_topk, "NULL argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (n_lists == 1) return launch_topk_local(d_lists, d_lists_n, 1, Q, cap, k, d_topk, kTopkPlain, nullptr, st);
    return launch_topk_lists(d_lists, d_lists_n, n_lists, Q, cap, k, d_topk, kTopkPlain, nullptr, st);
}

static int tvz_topk_shard_impl(const int32_t *d_hits, const int32_t *d_hits_n, int32_t Q,
                              int32_t cap, int32_t k, int32_t *d_out, void *hip_stream) {
    TVZ_REQUIRE(Q >= 0 && cap >= 0, "bad list shape");
    if (int rc = check_topk_k(k)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE((d_hits || cap == 0) && d_hits_n && d_out, "NULL argument");
    return launch_topk_local(d_hits, d_hits_n, 1, Q, cap, k, d_out, kTopkShard, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

static int tvz_topk_merge_impl(const int32_t *d_gathered, int32_t n_ranks, int32_t Q, int32_t k,
                              int32_t *d_topk, int32_t *d_totals, void *hip_stream) {
    TVZ_REQUIRE(n_ranks >= 1 && Q >= 0, "bad list shape");
    if (int rc = check_topk_k(k)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_gathered && d_topk, "NULL argument");
    return launch_topk_lists(d_gathered, nullptr, n_ranks, Q, k + 1, k, d_topk, kTopkMerge, d_totals,
                             reinterpret_cast<hipStream_t>(hip_stream));
}

static int tvz_match_topk_shards_impl(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                      const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                      int32_t min_match, const int32_t *d_exclude_ids, int32_t cap, int32_t k,
                                      int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                      size_t workspace_bytes, int32_t algo, void *hip_stream) {
    TVZ_REQUIRE(shards != nullptr && n_shards >= 1, "no shards");
    TVZ_REQUIRE(Q == 0 || (d_blocks && d_topk && d_totals), "NULL output");
    if (Q == 0) return TVZ_OK;
    const Batch b{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids};
    for (int32_t r = 0; r < n_shards; ++r) {
        TVZ_REQUIRE(shards[r] != nullptr && shards[r]->device == shards[0]->device,
                    "shard %d is NULL or on another device than shard 0", r);
        if (int rc = tvz_match_topk_local(shards[r], b, cap, k, d_blocks + (size_t)r * (size_t)Q * (size_t)(k + 1) * 3,
                                          Workspace{d_workspace, workspace_bytes}, 1, algo, hip_stream, nullptr))
            return rc;
    }
    DeviceGuard dg(shards[0]->device);
    return tvz_topk_merge_impl(d_blocks, n_shards, Q, k, d_topk, d_totals, hip_stream);
}

static int tvz_align_impl(tvz_corpus *c, const double *d_query, int32_t n, double eps,
                         double max_offset, int32_t *d_out, int64_t out_rows, int64_t *n_rows_out,
                         void *hip_stream) {
    TVZ_REQUIRE(c != nullptr && n_rows_out != nullptr, "NULL argument");
    TVZ_REQUIRE(n >= 0 && (n == 0 || d_query), "bad query");
    TVZ_REQUIRE(out_rows >= 0, "out_rows must be >= 0");
    int32_t nb = 0;
    if (int rc = check_align_bins(eps, max_offset, kAlignMaxBins, nullptr, &nb)) return rc;
    DeviceGuard dg(c->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const int64_t n_rows = (int64_t)c->h_rows.size();
    *n_rows_out = n_rows;
    // the caller sized d_out before this call; rows upserted since then are counted, not written
    const int64_t n_write = std::min(n_rows, out_rows);
    if (n_write == 0) return TVZ_OK;
    TVZ_REQUIRE(d_out != nullptr, "d_out is NULL");
    if (int rc = wait_mutations(c, st)) return rc;
    const int64_t blocks = std::min<int64_t>(tvz::ceil_div(n_write, kBlock / 64), 256 * 8);
    hipLaunchKernelGGL(ts_align_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, c->rows.p, n_write,
                       c->keys.p, d_query, n, eps, nb, d_out);
    TVZ_HIP(hipGetLastError());
    return record(c, st);
}

// ---- tolerant match (tvz_tol_kernels.h) ---------------------------------------------------------------------
namespace {

int check_tol(double tol) {
    if (!(tol >= 0.0 && tol <= DBL_MAX))                // refuses NaN, +-inf and negative values
        return tvz::fail(TVZ_ERR_INVALID, "tol must be finite and >= 0 (got %g)", tol);
    return TVZ_OK;
}

// The sweep, one launch: the sorted queries (q.sv, q.sp: per query, see ts_match_tol_kernel), in LDS when q.lds_keys > 0
// (every query of the launch has at most that many values).
template <bool HOSTOUT>
int launch_tol(tvz_corpus *c, RowSpan span, const Batch &b, const TolSorted &q, int32_t exclude_one, const HitSink &out,
               int blocks_x, HostOut ho, hipStream_t st) {
    const size_t lds = q.lds_keys > 0 ? tol_lds_bytes(q.lds_keys) : 0;
    TVZ_REQUIRE(lds + kQ1Stage * 12 + 64 <= (size_t)kLdsPerWorkgroup, "tolerant sweep: %zu B of LDS exceed a gfx950 workgroup's",
                lds);
    const dim3 grid((unsigned)blocks_x, (unsigned)b.Q);
    return by_mode(b.min_match, [&](auto mode) {
        auto sweep = q.lds_keys > 0 ? ts_match_tol_kernel<mode.value, HOSTOUT, true> : ts_match_tol_kernel<mode.value, HOSTOUT, false>;
        hipLaunchKernelGGL(sweep, grid, dim3(kTolBlock), lds, st, span.p, span.n, c->keys.p, q.sv, q.sp, b.d_q_offsets, q.qm,
                           q.m_one, q.lds_keys, q.tol, b.min_match, b.d_exclude_ids, exclude_one, out.cap, out.d_hits,
                           out.d_hits_n, ho);
        return launched();
    });
}

// Workspace of the sorted queries (every tolerant batched call ends in it): per query its count of non-NaN values,
// then room for `room` sorted values + positions.
struct TolWs {
    int32_t *qm = nullptr;
    double *sv = nullptr;
    int32_t *sp = nullptr;
    int64_t room = 0;
    static constexpr size_t kPerKey = sizeof(double) + sizeof(int32_t);
};
constexpr size_t kTolWsSlack = 256 + 2 * 255;         // (see Carver)

TolWs tol_ws_layout(Carver &cv, int32_t Q, int64_t keys) {
    TolWs w;
    w.qm = cv.take<int32_t>((size_t)Q);
    w.sv = cv.take<double>((size_t)keys);
    w.sp = cv.take<int32_t>((size_t)keys);
    w.room = keys;
    return w;
}

// bytes for `keys` sorted values next to Q counts; the most values a workspace of `bytes` holds (-1: not even the
// counts) - tol_ws_room(Q, tol_ws_bytes(Q, keys)) is `keys`
size_t tol_ws_bytes(int32_t Q, int64_t keys) {
    Carver cv(nullptr);
    tol_ws_layout(cv, Q, 0);
    return cv.used() + kTolWsSlack + (size_t)keys * TolWs::kPerKey;
}
int64_t tol_ws_room(int32_t Q, size_t bytes) {
    return bytes < tol_ws_bytes(Q, 0) ? -1 : (int64_t)((bytes - tol_ws_bytes(Q, 0)) / TolWs::kPerKey);
}

// ---- the lookup through cell postings (tvz_tol_index_kernels.h) ----
// Taken when the current generation carries cell postings at least as wide as the tolerance, min_match is one the row
// walk resolves itself (1..5) and the sorted queries fit LDS; every other call sweeps as before.  Caller holds mu.
bool tol_index_usable(const tvz_corpus *c, double tol, int32_t min_match, int32_t lds_keys) {
    const Index &ix = c->ix;
    return ix.valid && ix.now().t_cell > 0.0 && tol <= ix.now().t_cell && min_match >= 1 && min_match <= kTop &&
           lds_keys > 0 && tol_index_lds_bytes(lds_keys, lds_keys <= kTolIxSlotKeys) + kTolIxStaticLds <= (size_t)kLdsPerWorkgroup;
}

// Blocks per query: a large batch fills the chip with one block per query, which then walks every sub-index; a small
// one gives every sub-index (or run of them) a block of its own and, below that, splits a sub-index's candidates over
// up to eight blocks (each repeats the cheap pass A) - about 1,024 blocks in all, at most kTolIxMaxGroups per query.
struct TolIxShape {
    int spb = 1, groups = 1, split = 1;
    int blocks() const { return groups * split; }
};
TolIxShape tol_index_shape(int n_sub, int32_t Q) {
    TolIxShape sh;
    const int want = std::max(1, 1024 / std::max(Q, 1));
    sh.groups = std::max(1, std::min(std::min(n_sub, kTolIxMaxGroups), want));
    sh.spb = (int)tvz::ceil_div(n_sub, sh.groups);
    sh.groups = (int)tvz::ceil_div(n_sub, sh.spb);
    sh.split = std::max(1, std::min(std::min(8, want / sh.groups), kTolIxMaxGroups / sh.groups));
    return sh;
}

template <bool TOPK>
int launch_tol_index(tvz_corpus *c, const TolIxShape &sh, const Batch &b, const TolSorted &q, const HitSink &out, int32_t k,
                     unsigned long long *part, int32_t n_lists, hipStream_t st) {
    const IndexBuf &ib = c->ix.now();
    const dim3 grid((unsigned)sh.blocks(), (unsigned)b.Q);
    const bool keep_slots = sh.spb > 1 && q.lds_keys <= kTolIxSlotKeys;
    return by_mode<false>(b.min_match, [&](auto mode) {
        hipLaunchKernelGGL((ts_tol_index_kernel<mode.value, TOPK>), grid, dim3(kTolBlock),
                           tol_index_lds_bytes(q.lds_keys, keep_slots), st,
                           ib.cells.dir.p, ib.cells.bits(), ib.cells.ks, ib.cells.post.p, ib.ivid.p, ib.irows.p, ib.n_main, ib.n_sub,
                           sh.spb, sh.split, ib.t_cell, c->keys.p, q.sv, q.sp, b.d_q_offsets, q.qm, q.lds_keys, q.tol, b.min_match,
                           b.d_exclude_ids, out.cap, out.d_hits, out.d_hits_n, k, part, n_lists, keep_slots ? 1 : 0);
        return launched();
    });
}

// What a tolerant batched call does with the rows: with usable cell postings (tol_index_usable) the indexed rows are
// answered by the lookup, in front, and the sweep is left the delta table - every row is in exactly one; otherwise the
// sweep reads all rows.
struct TolPlan {
    RowSpan sweep;
    bool lookup = false;
    TolIxShape sh;
};
TolPlan tol_plan(const tvz_corpus *c, const Batch &b, const TolSorted &q, int64_t n_rows) {
    TolPlan p{RowSpan{c->rows.p, n_rows}};
    if (tol_index_usable(c, q.tol, b.min_match, q.lds_keys)) {
        p.lookup = true;
        p.sh = tol_index_shape(c->ix.now().n_sub, b.Q);
        p.sweep = RowSpan{c->ix.now().drows.p, c->ix.n_delta};
    }
    return p;
}

// The opening of every tolerant batched call.  The entry point has carved its own regions (f.cv; `fixed` bytes, none:
// 0); this checks the workspace of `have` bytes against them plus the sorted queries' fixed part and `min_keys`
// values, runs the entry point's remaining checks (args_ok), carves TolWs from all that is left, launches the sort
// (per query: sorted values + positions, counts, f.zeroed[q] = 0), takes the shared lock and waits for the mutations.
struct TolFront {
    Carver cv;
    size_t fixed;
    int32_t *zeroed;                 // [Q] hit counters or totals
    const char *what, *sizer;        // the workspace error names the call and its sizing function
};
struct TolCall {
    std::optional<DeviceGuard> dg;
    std::shared_lock<std::shared_mutex> lk;
    TolWs ws;
    int64_t n_rows = 0;
};
template <typename ArgsOk>
int tol_prelude(tvz_corpus *c, const Batch &b, TolFront f, size_t have, int64_t min_keys, hipStream_t st, ArgsOk &&args_ok,
                TolCall &t) {
    const size_t need = f.fixed + tol_ws_bytes(b.Q, min_keys);
    if (have < need)
        return tvz::fail(TVZ_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu bytes missing (size it with %s)", f.what, have,
                         need - have, f.sizer);
    if (int rc = args_ok()) return rc;
    t.ws = tol_ws_layout(f.cv, b.Q, tol_ws_room(b.Q, have - f.fixed));
    t.dg.emplace(c->device);
    hipLaunchKernelGGL(ts_tol_sort_kernel, dim3((unsigned)tvz::ceil_div(std::max(b.max_query_len, 1), kTolSortBlock), (unsigned)b.Q),
                       dim3(kTolSortBlock), 0, st, b.d_queries, b.d_q_offsets, b.max_query_len, t.ws.room, t.ws.sv, t.ws.sp,
                       t.ws.qm, f.zeroed);
    TVZ_HIP(hipGetLastError());
    t.lk = std::shared_lock<std::shared_mutex>(c->mu);
    t.n_rows = (int64_t)c->h_rows.size();
    return wait_mutations(c, st);
}

}  // namespace

static int tvz_find_duplicates_tol_impl(tvz_corpus *c, const double *h_query, int64_t n, double tol,
                                        int32_t min_match, int32_t exclude_id, int64_t cap, int32_t *h_out_ids,
                                        int32_t *h_out_counts, int32_t *h_out_kth, int64_t *n_out) {
    if (int rc = check_find_args(c, h_query, n, cap, h_out_ids, h_out_counts, n_out)) return rc;
    if (int rc = check_tol(tol)) return rc;
    DeviceGuard dg(c->device);
    StagingLease lease{c};
    if (int rc = staging_get(c, &lease.s)) return rc;
    Staging *s = lease.s;
    const int32_t excl = exclude_id >= 0 ? exclude_id : -1;
    // the query, sorted by value with its original positions, NaNs dropped (-0.0 folded to +0.0)
    std::vector<std::pair<double, int32_t>> &srt = s->tol_sort;
    srt.clear();
    srt.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (h_query[i] == h_query[i]) srt.emplace_back(h_query[i] == 0.0 ? 0.0 : h_query[i], (int32_t)i);
    std::sort(srt.begin(), srt.end());
    const int64_t m = (int64_t)srt.size();
    const int64_t m_even = (m + 1) & ~(int64_t)1;
    const bool fixup = min_match > kTop;                 // kth by the fix-up pass, which walks the raw query
    const size_t sorted_bytes = (size_t)m_even * 8 + (size_t)m * 4;
    const size_t raw_at = (sorted_bytes + 15) & ~(size_t)15;
    const size_t bytes = fixup ? raw_at + (size_t)n * 8 : sorted_bytes;
    std::vector<unsigned char> big;                      // queries of more than kMaxQueryLen timestamps only
    unsigned char *h = s->tol.h, *d = s->d_tol.p;
    if (n > kMaxQueryLen || bytes > kTolStageBytes) {
        if (int rc = ensure(s->d_tol_big, (int64_t)bytes, 0)) return rc;
        big.resize(bytes);
        h = big.data();
        d = s->d_tol_big.p;
    }
    double *hv = reinterpret_cast<double *>(h);
    int32_t *hp = reinterpret_cast<int32_t *>(h + (size_t)m_even * 8);
    for (int64_t t = 0; t < m; ++t) {
        hv[t] = srt[t].first;
        hp[t] = srt[t].second;
    }
    if (fixup && n) memcpy(h + raw_at, h_query, (size_t)n * 8);
    if (bytes) TVZ_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s->stream.s));
    const double *dv = reinterpret_cast<const double *>(d);
    const int32_t *dp = reinterpret_cast<const int32_t *>(d + (size_t)m_even * 8);
    auto launch = [&](int64_t n_rows, int &blocks, int &region) -> int {
        blocks = q1_blocks(n_rows, 1);
        region = (int)(tvz::ceil_div(n_rows, (int64_t)blocks * kTolGroups) * kTolGroups);
        const HostOut ho{s->hits.d, s->counts.d, region};
        const int32_t lds_keys = m <= kTolLdsKeys ? (int32_t)std::max<int64_t>(m, 1) : 0;
        const Batch one{nullptr, nullptr, 1, (int32_t)m, min_match, nullptr};      // (the sorted form is all the sweep reads)
        if (int rc = launch_tol<true>(c, RowSpan{c->rows.p, n_rows}, one, TolSorted{dv, dp, nullptr, (int32_t)m, lds_keys, tol},
                                      excl, kHostSink, blocks, ho, s->stream.s))
            return rc;
        if (!fixup) return TVZ_OK;
        hipLaunchKernelGGL(ts_tol_kth_fixup_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s->stream.s, c->rows.p,
                           c->keys.p, reinterpret_cast<const double *>(d + raw_at), static_cast<const int64_t *>(nullptr),
                           (int32_t)n, tol, min_match, s->hits.d, s->counts.d, region);
        return launched();
    };
    int64_t n_hits = 0;
    if (int rc = pinned_sweep(c, s, "tolerant ", launch, &n_hits)) return rc;
    copy_out(reinterpret_cast<Hit *>(s->hits.h), n_hits, n_hits, cap, h_out_ids, h_out_counts, h_out_kth, n_out);
    return TVZ_OK;
}

static int tvz_match_tol_impl(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                              int32_t max_query_len, double tol, int32_t min_match, const int32_t *d_exclude_ids,
                              int32_t cap, int32_t *d_hits, int32_t *d_hits_n, void *d_workspace,
                              size_t workspace_bytes, void *hip_stream) {
    const Batch b{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids};
    if (int rc = check_batch_args(c, b, cap)) return rc;
    if (int rc = check_tol(tol)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_hits_n && (cap == 0 || d_hits), "NULL output");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    TolCall t;
    if (int rc = tol_prelude(c, b, TolFront{Carver(d_workspace), 0, d_hits_n, "tolerant match", "tvz_match_tol_workspace_bytes"},
                             d_workspace ? workspace_bytes : 0, 0, st, [] { return TVZ_OK; }, t))
        return rc;
    const TolSorted q{t.ws.sv, t.ws.sp, t.ws.qm, 0, max_query_len <= kTolLdsKeys ? std::max(max_query_len, 1) : 0, tol};
    const HitSink out = HitSink::dense(cap, d_hits, d_hits_n);
    const TolPlan plan = tol_plan(c, b, q, t.n_rows);
    if (plan.lookup)
        if (int rc = launch_tol_index<false>(c, plan.sh, b, q, out, 0, nullptr, 0, st)) return rc;
    if (!plan.lookup || plan.sweep.n)      // (behind the lookup an empty delta table needs no launch)
        if (int rc = launch_tol<false>(c, plan.sweep, b, q, /* exclude_one */ -1, out, q1_blocks(plan.sweep.n, Q), HostOut{}, st))
            return rc;
    if (min_match > kTop && t.n_rows) {    // (never behind the lookup: it takes min_match 1..5)
        hipLaunchKernelGGL(ts_tol_kth_fixup_kernel, dim3((unsigned)Q), dim3(kBlock), 0, st, c->rows.p, c->keys.p,
                           d_queries, d_q_offsets, 0, tol, min_match, d_hits, d_hits_n, cap);
        TVZ_HIP(hipGetLastError());
    }
    return record(c, st);
}

namespace {

// Workspace of the top-k form, in front of the sorted queries (TolWs, which takes the rest): the queries' hit totals,
// one kept list per sweep block, the local block and the gathered ones.  The sizing function knows no row count:
// the lists are sized by the grid's upper bound, Q * tol_topk_max_blocks(Q) <= tol_topk_max_lists(Q).
struct TolTopkWs {
    int32_t *totals = nullptr;             // [Q]
    unsigned long long *part = nullptr;    // [Q][blocks][k]
    int32_t *local = nullptr;              // [Q][k+1][3]
    int32_t *gathered = nullptr;           // [n_ranks][Q][k+1][3]
};

TolTopkWs tol_topk_ws_layout(Carver &cv, int32_t Q, int32_t k, int32_t n_ranks) {
    TolTopkWs w;
    const size_t block = (size_t)Q * (size_t)(k + 1) * 3;
    w.totals = cv.take<int32_t>((size_t)Q);
    w.part = cv.take<unsigned long long>((size_t)tol_topk_max_lists(Q) * (size_t)k);
    w.local = cv.take<int32_t>(block);
    w.gathered = cv.take<int32_t>((size_t)(n_ranks > 1 ? n_ranks : 1) * block);
    return w;
}

}  // namespace

// used by tvz_comm.hip (same shared object, not exported): sort -> sweep that keeps the k best -> per-query
// selection.  d_out = NULL writes the block into the workspace's own area; `blocks` is told where it went and where
// the all-gather's target is.
int tvz_match_tol_topk_local(tvz_corpus *c, const Batch &b, double tol, int32_t k, int32_t *d_out, Workspace ws,
                             int32_t n_ranks, void *hip_stream, ShardBlocks *blocks) {
    const int32_t Q = b.Q, max_query_len = b.max_query_len, min_match = b.min_match;
    if (int rc = check_batch_args(c, b, 0)) return rc;
    if (int rc = check_tol(tol)) return rc;
    if (min_match < 1 || min_match > kTop)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "tolerant top-k: min_match %d outside 1..%d (kth needs the hit lists of "
                                              "tvz_match_tol)", (int)min_match, kTop);
    if (k < 1 || k > kTolTopkMaxK)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "tolerant top-k: k=%d outside 1..%d", (int)k, kTolTopkMaxK);
    if (max_query_len > kTolTopkMaxLen)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "tolerant top-k: max_query_len %d above %d (use tvz_match_tol)",
                         (int)max_query_len, kTolTopkMaxLen);
    if (Q == 0) return TVZ_OK;
    Carver cv(ws.p);
    const TolTopkWs w = tol_topk_ws_layout(cv, Q, k, n_ranks);
    const int32_t lds_keys = std::max(max_query_len, 1);
    const size_t lds = tol_lds_bytes(lds_keys);
    auto args_ok = [&]() -> int {
        TVZ_REQUIRE(d_out || blocks, "NULL output");
        if (d_out == nullptr) d_out = w.local;
        if (blocks) *blocks = ShardBlocks{d_out, w.gathered};
        TVZ_REQUIRE(lds + kTolTopkStaticLds <= (size_t)kLdsPerWorkgroup,
                    "tolerant top-k sweep: %zu B of dynamic + %d B of static LDS exceed a gfx950 workgroup's", lds,
                    kTolTopkStaticLds);
        return TVZ_OK;
    };
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    TolCall t;
    if (int rc = tol_prelude(c, b, TolFront{cv, cv.fixed(), w.totals, "tolerant top-k", "tvz_match_tol_topk_workspace_bytes"},
                             ws.p ? ws.bytes : 0, 0, st, args_ok, t))
        return rc;
    // The lists in front of the sweep's own: one per block of the lookup; the selection takes all lists alike.
    const TolSorted q{t.ws.sv, t.ws.sp, t.ws.qm, 0, lds_keys, tol};
    const TolPlan plan = tol_plan(c, b, q, t.n_rows);
    const int lists0 = plan.lookup ? plan.sh.blocks() : 0;
    // (lists0 <= kTolIxMaxGroups < kTolTopkMinBlocks: the workspace's tol_topk_max_lists(Q) lists still suffice)
    const int n_blocks = plan.sweep.n ? std::min(q1_blocks(plan.sweep.n, Q), tol_topk_max_blocks(Q) - lists0) : 0;
    const int n_lists = lists0 + n_blocks;
    if (lists0)
        if (int rc = launch_tol_index<true>(c, plan.sh, b, q, HitSink::dense(0, nullptr, w.totals), k, w.part, n_lists, st))
            return rc;
    if (n_blocks) {
        const dim3 grid((unsigned)n_blocks, (unsigned)Q);
        if (int rc = by_mode<false>(min_match, [&](auto mode) {
                hipLaunchKernelGGL((ts_tol_topk_kernel<mode.value>), grid, dim3(kTolBlock), lds, st, plan.sweep.p, plan.sweep.n,
                                   c->keys.p, q.sv, q.sp, b.d_q_offsets, q.qm, lds_keys, tol, min_match, b.d_exclude_ids, k,
                                   w.part, n_lists, lists0, w.totals);
                return launched();
            }))
            return rc;
    }
    hipLaunchKernelGGL(ts_tol_topk_reduce_kernel, dim3((unsigned)Q), dim3(kTolReduceBlock), 0, st, w.part, n_lists, k,
                       q.qm, lds_keys, w.totals, d_out);
    TVZ_HIP(hipGetLastError());
    return record(c, st);
}

static int tvz_match_tol_topk_impl(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                   int32_t max_query_len, double tol, int32_t min_match,
                                   const int32_t *d_exclude_ids, int32_t k, int32_t *d_out, void *d_workspace,
                                   size_t workspace_bytes, void *hip_stream) {
    TVZ_REQUIRE(Q <= 0 || d_out != nullptr, "d_out is NULL");
    return tvz_match_tol_topk_local(c, Batch{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids}, tol, k,
                                    d_out, Workspace{d_workspace, workspace_bytes}, 1, hip_stream, nullptr);
}

// ---- alignment top-k: the forms of one call (tvz_align_kernels.h) -----------------------------------------------
namespace {

// Workspace of every form, in front of the sorted queries (TolWs, which takes the rest): the queries' hit totals and
// one kept list per sweep block, as a structure of arrays - k words and k payloads, and behind them the form's part32
// lists of k uint32: the raw votes, the rate indexes, the index pairs and the key counts (AlHit::Parts, AwHit::Parts,
// ArHit::Parts, AsHit::Parts).  The sizing function knows no row count: the lists are sized by the grid's upper bound,
// as the tolerant top-k's are.  The sharded forms (n_blocks > 0: the communicator's ranks, at least 1) add the local
// block and the gathered ones behind them; the plain calls (n_blocks = 0) have neither.
struct AlignTopkWs {
    int32_t *totals = nullptr;             // [Q]
    unsigned long long *part_w = nullptr;  // [Q][blocks][k]
    unsigned long long *part_p = nullptr;  // [Q][blocks][k]
    uint32_t *part32[4] = {};              // [Q][blocks][k] each, the form's first part32 of them
    int32_t *local = nullptr;              // [Q][k+1][cols]
    int32_t *gathered = nullptr;           // [n_blocks][Q][k+1][cols]
};

// Everything a form's sweep or selection launch may need; each kernel takes the part of it that is its own.
struct AlignLaunch {
    dim3 grid;
    size_t lds;                      // dynamic, of the sweep
    hipStream_t st;
    const tvz_corpus *c;
    int64_t n_rows;
    const Batch *b;
    const TolWs *q;                  // the sorted queries
    const AlignCall *a;
    const AlRates *rates;
    uint32_t flags;
    int32_t lds_keys, B, width, k, n_lists;
    const AlignTopkWs *w;
    int32_t *d_out;
};
struct AlignMergeArgs {              // ... and its merge launch
    dim3 grid;
    hipStream_t st;
    const int32_t *d_gathered;
    int32_t n_lists, Q, k;
    uint32_t flags;
    const double *d_queries;
    const int64_t *d_q_offsets;
    int32_t *d_topk, *d_totals;
};

// What a form of the alignment top-k is, on the host: tvz_align_topk, tvz_align_wide_topk, tvz_align_rates_topk and
// tvz_align_span_topk are one entry each of kAlignForms (indexed by AlignForm, tvz_common.h), and nothing below the
// table asks which form it has.  The kernels' argument lists differ (the window width, the flags, the rates, the lists
// behind the first two), so every kernel is launched from its form's entry.  A new form, or the RCCL variant of an
// existing one, is an entry here (and its exports); only what is genuinely new needs code.
struct AlignTopkForm {
    int cols;                        // int32 columns of a block row
    int part32;                      // uint32 lists behind the two uint64 ones: a kept hit is 16 + 4 * part32 bytes
    bool takes_rates;                // the call has a rate list (check_align_rates)
    bool limits_first;               // the flags and the limits are refused before the handle is looked at
    const char *what, *sizer;        // the call in messages; the sizing function the workspace message names
    const char *sharded_sizer;       // ... and the one it names for the sharded form (n_ranks >= 1) of the bounded and the
                                     // wide form; NULL for the forms with rates, whose RCCL calls came later: the host
                                     // program that walks this table's layouts (tests/align_sharded_host_main.hip) sizes
                                     // exactly the forms that have one here, so theirs is `rccl_sizer` below
    int32_t max_bins;                // 2B + 1 at most
    const char *bins_limit;          // the header's name of that limit, if it has one (check_align_bins)
    uint32_t flags;                  // the permitted ones
    uint32_t exclusive;              // ... of which these two are two score kinds: one of them
    int static_lds;                  // of the sweep
    void (*sweep)(const AlignLaunch &);
    void (*reduce)(const AlignLaunch &);
    void (*merge)(const AlignMergeArgs &);
    const char *rccl_sizer = nullptr;  // the sharded sizing function of a form with rates (see sharded_sizer)
    // the sizing function a workspace refusal of the sharded form names
    constexpr const char *sharded_name() const { return sharded_sizer ? sharded_sizer : rccl_sizer; }
};

AlignTopkWs align_topk_ws_layout(Carver &cv, const AlignTopkForm &f, int32_t Q, int32_t k, int32_t n_blocks) {
    AlignTopkWs w;
    const size_t lists = (size_t)tol_topk_max_lists(Q) * (size_t)k;
    w.totals = cv.take<int32_t>((size_t)Q);
    w.part_w = cv.take<unsigned long long>(lists);
    w.part_p = cv.take<unsigned long long>(lists);
    for (int i = 0; i < f.part32; ++i) w.part32[i] = cv.take<uint32_t>(lists);
    if (n_blocks > 0) {
        const size_t block = (size_t)Q * (size_t)(k + 1) * (size_t)f.cols;
        w.local = cv.take<int32_t>(block);
        w.gathered = cv.take<int32_t>((size_t)n_blocks * block);
    }
    return w;
}

size_t align_topk_ws_bytes(const AlignTopkForm &f, int32_t Q, int64_t keys, int32_t k, int32_t n_blocks) {
    Carver cv(nullptr);
    align_topk_ws_layout(cv, f, Q, k, n_blocks);
    return cv.fixed() + tol_ws_bytes(Q, keys);
}

// The table: each kernel is launched once, here, with its own argument list out of the aggregate.
constexpr AlignTopkForm kAlignForms[] = {
    // kAlignBounded: tvz_align_topk.  It has no flags argument (its callers pass 0), and its B <= 2047 fits the window:
    // all its bins, and no resume positions
    {4, 0, false, false, "alignment top-k", "tvz_align_topk_workspace_bytes", "tvz_align_topk_sharded_workspace_bytes",
     kAlignMaxBins, nullptr, 0u, 0u, al_static_lds<AlHit>(),
     [](const AlignLaunch &l) {
         hipLaunchKernelGGL(ts_align_topk_kernel, l.grid, dim3(kAlBlock), l.lds, l.st, l.c->rows.p, l.n_rows, l.c->keys.p,
                            l.q->sv, l.b->d_q_offsets, l.q->qm, l.lds_keys, l.a->eps, l.B, l.a->min_votes, l.a->min_score,
                            l.b->d_exclude_ids, l.k, l.w->part_w, l.w->part_p, l.n_lists, l.w->totals);
     },
     [](const AlignLaunch &l) {
         hipLaunchKernelGGL(ts_align_topk_reduce_kernel, l.grid, dim3(kAlReduceBlock), 0, l.st, l.w->part_w, l.w->part_p,
                            l.n_lists, l.k, l.q->qm, l.lds_keys, l.w->totals, l.d_out);
     },
     [](const AlignMergeArgs &m) {
         hipLaunchKernelGGL(ts_align_topk_merge_kernel, m.grid, dim3(kAlMergeBlock), 0, m.st, m.d_gathered, m.n_lists, m.Q,
                            m.k, m.d_queries, m.d_q_offsets, m.d_topk, m.d_totals);
     }},
    // kAlignWide: tvz_align_wide_topk
    {4, 1, false, false, "wide alignment top-k", "tvz_align_wide_topk_workspace_bytes",
     "tvz_align_wide_topk_sharded_workspace_bytes", 2 * kAwMaxB + 1, "TVZ_ALIGN_WIDE_MAX_B", kAwContain | kAlTwoBins, 0u,
     al_static_lds<AwHit>(),
     [](const AlignLaunch &l) {
         const auto sweep = (l.flags & kAlTwoBins) ? ts_alignw2_sweep_kernel : ts_alignw_sweep_kernel;   // (one argument list)
         hipLaunchKernelGGL(sweep, l.grid, dim3(kAlBlock), l.lds, l.st, l.c->rows.p, l.n_rows, l.c->keys.p,
                            l.q->sv, l.b->d_q_offsets, l.q->qm, l.lds_keys, l.a->eps, l.B, l.width, l.a->min_votes,
                            l.a->min_score, l.flags, l.b->d_exclude_ids, l.k, l.w->part_w, l.w->part_p, l.w->part32[0],
                            l.n_lists, l.w->totals);
     },
     [](const AlignLaunch &l) {
         hipLaunchKernelGGL(ts_alignw_reduce_kernel, l.grid, dim3(kAlReduceBlock), 0, l.st, l.w->part_w, l.w->part_p,
                            l.w->part32[0], l.n_lists, l.k, l.q->qm, l.lds_keys, l.w->totals, l.d_out);
     },
     [](const AlignMergeArgs &m) {
         hipLaunchKernelGGL(ts_alignw_merge_kernel, m.grid, dim3(kAlMergeBlock), 0, m.st, m.d_gathered, m.n_lists, m.Q, m.k,
                            m.flags, m.d_queries, m.d_q_offsets, m.d_topk, m.d_totals);
     }},
    // kAlignRates: tvz_align_rates_topk - the wide call with the rate loop
    {5, 2, true, false, "alignment top-k with rates", "tvz_align_rates_topk_workspace_bytes", nullptr, 2 * kAwMaxB + 1,
     "TVZ_ALIGN_WIDE_MAX_B", kAwContain | kAlTwoBins, 0u, al_static_lds<ArHit>(),
     [](const AlignLaunch &l) {
         const auto sweep = (l.flags & kAlTwoBins) ? ts_alignr2_sweep_kernel : ts_alignr_sweep_kernel;   // (one argument list)
         hipLaunchKernelGGL(sweep, l.grid, dim3(kAlBlock), l.lds, l.st, l.c->rows.p, l.n_rows, l.c->keys.p,
                            l.q->sv, l.b->d_q_offsets, l.q->qm, l.lds_keys, l.a->eps, l.B, l.width, *l.rates,
                            l.a->min_votes, l.a->min_score, l.flags, l.b->d_exclude_ids, l.k, l.w->part_w, l.w->part_p,
                            l.w->part32[0], l.w->part32[1], l.n_lists, l.w->totals);
     },
     [](const AlignLaunch &l) {
         hipLaunchKernelGGL(ts_alignr_reduce_kernel, l.grid, dim3(kAlReduceBlock), 0, l.st, l.w->part_w, l.w->part_p,
                            l.w->part32[0], l.w->part32[1], l.n_lists, l.k, l.q->qm, l.lds_keys, l.w->totals, l.d_out);
     },
     [](const AlignMergeArgs &m) {
         hipLaunchKernelGGL(ts_alignr_merge_kernel, m.grid, dim3(kAlMergeBlock), 0, m.st, m.d_gathered, m.n_lists, m.Q, m.k,
                            m.flags, m.d_queries, m.d_q_offsets, m.d_topk, m.d_totals);
     },
     "tvz_align_rates_topk_sharded_workspace_bytes"},
    // kAlignSpan: tvz_align_span_topk - the call with rates and the span pass
    {8, 4, true, true, "alignment top-k with spans", "tvz_align_span_topk_workspace_bytes", nullptr, 2 * kAwMaxB + 1,
     "TVZ_ALIGN_WIDE_MAX_B", kAwContain | kAsLocal | kAlTwoBins, kAwContain | kAsLocal, al_static_lds<AsHit>(),
     [](const AlignLaunch &l) {
         const auto sweep = (l.flags & kAlTwoBins) ? ts_aligns2_sweep_kernel : ts_aligns_sweep_kernel;   // (one argument list)
         hipLaunchKernelGGL(sweep, l.grid, dim3(kAlBlock), l.lds, l.st, l.c->rows.p, l.n_rows, l.c->keys.p,
                            l.q->sv, l.b->d_q_offsets, l.q->qm, l.lds_keys, l.a->eps, l.B, l.width, *l.rates,
                            l.a->min_votes, l.a->min_score, l.flags, l.b->d_exclude_ids, l.k, l.w->part_w, l.w->part_p,
                            l.w->part32[0], l.w->part32[1], l.w->part32[2], l.w->part32[3], l.n_lists, l.w->totals);
     },
     [](const AlignLaunch &l) {
         hipLaunchKernelGGL(ts_aligns_reduce_kernel, l.grid, dim3(kAlReduceBlock), 0, l.st, l.w->part_w, l.w->part_p,
                            l.w->part32[0], l.w->part32[1], l.w->part32[2], l.w->part32[3], l.n_lists, l.k, l.q->qm,
                            l.lds_keys, l.w->totals, l.d_out);
     },
     [](const AlignMergeArgs &m) {
         hipLaunchKernelGGL(ts_aligns_merge_kernel, m.grid, dim3(kAlMergeBlock), 0, m.st, m.d_gathered, m.n_lists, m.Q, m.k,
                            m.flags, m.d_queries, m.d_q_offsets, m.d_topk, m.d_totals);
     },
     "tvz_align_span_topk_sharded_workspace_bytes"},
};
static_assert(sizeof(kAlignForms) / sizeof(kAlignForms[0]) == kAlignFormCount, "one entry per AlignForm, in its order");

// what every form's merge refuses, apart from its pointers and flags
int check_align_merge(int32_t n_lists, int32_t k) {
    if (n_lists < 1 || n_lists > kAlMergeMaxLists)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment top-k merge: %d lists outside 1..%d", (int)n_lists, kAlMergeMaxLists);
    if (k < 1 || k > kAlMaxK)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment top-k: k=%d outside 1..%d", (int)k, kAlMaxK);
    return TVZ_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the flags of a call (where = "") or of its merge (" merge"): the form's own, and of two score kinds one
int check_align_flags(const AlignTopkForm &f, uint32_t flags, const char *where) {
    TVZ_REQUIRE((flags & ~f.flags) == 0u, "%s%s: unknown flag bits 0x%x", f.what, where, (unsigned)(flags & ~f.flags));
    TVZ_REQUIRE(f.exclusive == 0u || (flags & f.exclusive) != f.exclusive,
                "%s: TVZ_ALIGN_CONTAIN and TVZ_ALIGN_LOCAL are two score kinds: one of them", f.what);
    return TVZ_OK;
}

// the limits of every call that need neither the handle nor the device
int check_align_limits(const AlignTopkForm &f, const AlignCall &a, int32_t k, int32_t max_query_len) {
    TVZ_REQUIRE(a.min_votes >= 1, "%s: min_votes %d below 1", f.what, (int)a.min_votes);
    TVZ_REQUIRE(a.min_score >= 0 && a.min_score <= kAlScoreOne, "%s: min_score %d outside 0..%d", f.what, (int)a.min_score,
                kAlScoreOne);
    if (k < 1 || k > kAlMaxK) return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: k=%d outside 1..%d", f.what, (int)k, kAlMaxK);
    if (max_query_len > kAlMaxLen)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: max_query_len %d above %d", f.what, (int)max_query_len, kAlMaxLen);
    return TVZ_OK;
}

// The arguments of a call and of its _shards form beyond the batch and the sink.
struct AlignAsk {
    AlignCall a;
    const double *h_rates;           // the forms that take rates; NULL, 0 otherwise
    int32_t n_rates;
    uint32_t flags;                  // 0 for the form that has none
    int32_t k;
};

// What a form refuses before any handle is looked at, for the call and for its _shards form alike: the rate list
// (-> *rates, the sweep's by-value argument), then - limits_first - the flags and the limits.
int check_align_early(const AlignTopkForm &f, const AlignAsk &s, int32_t max_query_len, AlRates *rates) {
    if (f.takes_rates)
        if (int rc = check_align_rates(s.h_rates, s.n_rates, rates)) return rc;
    if (f.limits_first) {
        if (int rc = check_align_flags(f, s.flags, "")) return rc;
        if (int rc = check_align_limits(f, s.a, s.k, max_query_len)) return rc;
    }
    return TVZ_OK;
}

// The dynamic LDS of a block of row walks (aw_lds_bytes) for a call of B bins on either side and queries of at most
// max_query_len values, and whether it fits a gfx950 workgroup beside the static LDS the kernel declares.  The caller
// words the refusal.
struct AlignLds {
    int32_t lds_keys, width;
    size_t bytes;
    AlignLds(int32_t max_query_len, int32_t B)
        : lds_keys(std::max(max_query_len, 1)), width(aw_width(B)), bytes(aw_lds_bytes(lds_keys, B, width)) {}
    bool fits(int static_lds) const { return bytes + (size_t)static_lds <= (size_t)kLdsPerWorkgroup; }
};

// One handle: sort -> sweep that keeps the k best -> per-query selection.  `rates`: checked (check_align_early).
// n_ranks = 0: d_out is the caller's.  n_ranks >= 1: the workspace also holds the local block and n_ranks gathered ones
// (the form's sharded sizing function); d_out = NULL writes the block into the workspace's own, and `blocks` is told
// where it went and where the all-gather's target is.  `late`: the sharded call's own refusals, made behind all of
// these and in front of the first launch.
int align_topk_run(const AlignTopkForm &f, tvz_corpus *c, const Batch &b, const AlignAsk &s, const AlRates &rates,
                   int32_t *d_out, Workspace ws, int32_t n_ranks, void *hip_stream, ShardBlocks *blocks, LateCheck late = {}) {
    const AlignCall &a = s.a;
    const int32_t Q = b.Q, max_query_len = b.max_query_len, k = s.k;
    if (int rc = check_batch_args(c, b, 0)) return rc;
    int32_t B = 0;
    if (int rc = check_align_bins(a.eps, a.max_offset, f.max_bins, f.bins_limit, &B)) return rc;
    if (int rc = check_align_flags(f, s.flags, "")) return rc;
    if (int rc = check_align_limits(f, a, k, max_query_len)) return rc;
    if (Q == 0) return TVZ_OK;
    Carver cv(ws.p);
    const AlignTopkWs w = align_topk_ws_layout(cv, f, Q, k, n_ranks);
    const AlignLds lds(max_query_len, B);
    auto args_ok = [&]() -> int {
        TVZ_REQUIRE(d_out != nullptr || w.local != nullptr, "d_out is NULL");
        if (d_out == nullptr) d_out = w.local;
        if (blocks) *blocks = ShardBlocks{d_out, w.gathered};
        TVZ_REQUIRE(lds.fits(f.static_lds), "%s sweep: %zu B of dynamic + %d B of static LDS exceed a gfx950 workgroup's", f.what,
                    lds.bytes, f.static_lds);
        return late();
    };
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    // the fixed parts and room for ONE query of max_query_len values; what the caller gave beyond that holds more
    // (the sorted positions are unused here)
    TolCall t;
    if (int rc = tol_prelude(c, b, TolFront{cv, cv.fixed(), w.totals, f.what,
                                            n_ranks > 0 ? f.sharded_name() : f.sizer},
                             ws.p ? ws.bytes : 0, max_query_len, st, args_ok, t))
        return rc;
    const int64_t n_rows = t.n_rows;
    const int n_blocks = n_rows ? (int)std::min<int64_t>(tvz::ceil_div(n_rows, (int64_t)kAlWaves), tol_topk_max_blocks(Q)) : 0;
    AlignLaunch l{dim3((unsigned)n_blocks, (unsigned)Q), lds.bytes, st, c, n_rows, &b, &t.ws, &a, &rates, s.flags, lds.lds_keys,
                  B, lds.width, k, n_blocks, &w, d_out};
    if (n_blocks) {
        f.sweep(l);
        TVZ_HIP(hipGetLastError());
    }
    l.grid = dim3((unsigned)Q);
    f.reduce(l);
    TVZ_HIP(hipGetLastError());
    return record(c, st);
}

// A call of the C ABI: what the form refuses early, then the handle.
int align_topk_call(AlignForm form, tvz_corpus *c, const Batch &b, const AlignAsk &s, int32_t *d_out, Workspace ws,
                    int32_t n_ranks, void *hip_stream, ShardBlocks *blocks, LateCheck late = {}) {
    const AlignTopkForm &f = kAlignForms[form];
    AlRates rates{};
    if (int rc = check_align_early(f, s, b.max_query_len, &rates)) return rc;
    return align_topk_run(f, c, b, s, rates, d_out, ws, n_ranks, hip_stream, blocks, late);
}

// The shards of one process, for any form: every handle's call into its block of d_blocks, then the merge.
int align_shards_impl(AlignForm form, tvz_corpus *const *shards, int32_t n_shards, const Batch &b, const AlignAsk &s,
                      int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, Workspace ws, void *hip_stream) {
    const AlignTopkForm &f = kAlignForms[form];
    const int32_t Q = b.Q, k = s.k;
    AlRates rates{};
    if (int rc = check_align_early(f, s, b.max_query_len, &rates)) return rc;
    TVZ_REQUIRE(shards != nullptr && n_shards >= 1, "no shards");
    TVZ_REQUIRE(Q >= 0, "Q=%d is negative", (int)Q);
    if (int rc = check_align_merge(n_shards, k)) return rc;
    for (int32_t r = 0; r < n_shards; ++r)
        TVZ_REQUIRE(shards[r] != nullptr && shards[r]->device == shards[0]->device,
                    "shard %d is NULL or on another device than shard 0", r);
    TVZ_REQUIRE(Q == 0 || (d_blocks && d_topk && d_totals && b.d_queries && b.d_q_offsets), "NULL argument");
    TVZ_REQUIRE(aligned16(d_blocks) && aligned16(d_topk), "alignment top-k merge: the blocks and d_topk must be 16-byte aligned");
    if (Q == 0) return TVZ_OK;
    // every handle's call makes the same checks of the same arguments (the flags among them): what one refuses, the
    // first one refuses, before anything is enqueued
    for (int32_t r = 0; r < n_shards; ++r)
        if (int rc = align_topk_run(f, shards[r], b, s, rates,
                                    d_blocks + (size_t)r * (size_t)Q * (size_t)(k + 1) * (size_t)f.cols, ws, 0, hip_stream,
                                    nullptr))
            return rc;
    DeviceGuard dg(shards[0]->device);
    return tvz_align_merge_local(form, d_blocks, n_shards, Q, k, s.flags, b.d_queries, b.d_q_offsets, d_topk, d_totals,
                                 hip_stream);
}

Batch align_batch(const double *d_queries, const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                  const int32_t *d_exclude_ids) {
    return Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, d_exclude_ids};
}

// What the sizing exports share: the argument refusals, the `keys` default and the room for one longest query.
size_t align_sizing(AlignForm form, int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k, int32_t n_blocks) {
    if (Q < 0 || max_query_len < 0 || total_query_keys < 0 || k < 1) return 0;
    const int64_t keys = total_query_keys > 0 ? total_query_keys : (int64_t)Q * max_query_len;
    return align_topk_ws_bytes(kAlignForms[form], Q, std::max<int64_t>(keys, max_query_len), k, n_blocks);
}

// ---- every aligned part of a named stored video (tvz_align_parts; tvz_align_parts_kernels.h) ----------------------
// Workspace in front of the sorted queries (TolWs, which takes the rest): per pair the count of rows that carry its id,
// the candidate slots' row indices and every slot's result.
// The sharded form (n_blocks > 0: the communicator's ranks, at least 1) adds the local answer and the gathered ones
// behind them, as the alignment top-k's sharded forms do; the plain call and the _shards form (n_blocks = 0) have neither.
struct AlignPartsWs {
    int32_t *counts = nullptr;             // [Q][k]
    int64_t *slots = nullptr;              // [Q][k][kApMaxRows]
    int32_t *scratch = nullptr;            // [Q][k][kApMaxRows][1 + max_parts][6]
    int32_t *local = nullptr;              // [Q][k][1 + max_parts][6]
    int32_t *gathered = nullptr;           // [n_blocks][Q][k][1 + max_parts][6]
};

AlignPartsWs align_parts_ws_layout(Carver &cv, int32_t Q, int32_t k, int32_t max_parts, int32_t n_blocks = 0) {
    AlignPartsWs w;
    const size_t pairs = (size_t)Q * (size_t)k;
    w.counts = cv.take<int32_t>(pairs);
    w.slots = cv.take<int64_t>(pairs * kApMaxRows);
    w.scratch = cv.take<int32_t>(pairs * kApMaxRows * (size_t)ap_words(max_parts));
    if (n_blocks > 0) {
        const size_t block = pairs * (size_t)ap_words(max_parts);
        w.local = cv.take<int32_t>(block);
        w.gathered = cv.take<int32_t>((size_t)n_blocks * block);
    }
    return w;
}

size_t align_parts_ws_bytes(int32_t Q, int64_t keys, int32_t k, int32_t max_parts, int32_t n_blocks) {
    Carver cv(nullptr);
    align_parts_ws_layout(cv, Q, k, max_parts, n_blocks);
    return cv.fixed() + tol_ws_bytes(Q, keys);
}

// what the two sizing exports share: the argument refusals, the `keys` default and the room for one longest query
size_t align_parts_sizing(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k, int32_t max_parts,
                          int32_t n_blocks) {
    if (Q < 0 || max_query_len < 0 || total_query_keys < 0 || k < 1 || max_parts < 1 || max_parts > kApMaxParts) return 0;
    const int64_t keys = total_query_keys > 0 ? total_query_keys : (int64_t)Q * max_query_len;
    return align_parts_ws_bytes(Q, std::max<int64_t>(keys, max_query_len), k, max_parts, n_blocks);
}

// The call in messages and limits: no entry of kAlignForms (it keeps no hit), only what the shared checks read of one -
// the name, the two sizing functions and the bins' limit.
constexpr AlignTopkForm kAlignPartsForm = {kApCols, 0, true, true, "alignment parts", "tvz_align_parts_workspace_bytes",
                                           "tvz_align_parts_sharded_workspace_bytes", 2 * kAwMaxB + 1, "TVZ_ALIGN_WIDE_MAX_B",
                                           kAlTwoBins, 0u, 0, nullptr, nullptr, nullptr};

// Everything of a parts call that needs neither the handle nor the device is refused first, for the call and for its
// _shards and _sharded forms alike, in the span call's order: the rate list (-> *rates), min_votes, k, the query limit;
// then max_parts, the flags (tvz_align_parts_flags; 0 from the calls that have none) and the bins (-> *B).
int check_align_parts_early(const Batch &b, const AlignPartsCall &p, AlRates *rates, int32_t *B) {
    const AlignTopkForm &f = kAlignPartsForm;
    if (int rc = check_align_rates(p.h_rates, p.n_rates, rates)) return rc;
    if (int rc = check_align_limits(f, AlignCall{p.eps, p.max_offset, p.min_votes, 0}, p.k, b.max_query_len)) return rc;
    if (p.max_parts < 1 || p.max_parts > kApMaxParts)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: max_parts=%d outside 1..%d (TVZ_ALIGN_MAX_PARTS)", f.what, (int)p.max_parts,
                         kApMaxParts);
    if (int rc = check_align_flags(f, p.flags, "")) return rc;
    return check_align_bins(p.eps, p.max_offset, f.max_bins, f.bins_limit, B);
}

// One handle: sort -> locate the ids' rows -> walk every (pair, candidate row) -> pick per pair.  `rates`, `B`: checked
// (check_align_parts_early).  n_ranks = 0: d_parts is the caller's.  n_ranks >= 1: the workspace also holds the local
// answer and n_ranks gathered ones; d_parts = NULL writes into the workspace's own, and `blocks` is told where.  `late`:
// the sharded call's own refusals, behind all of these and in front of the first launch.
int align_parts_run(tvz_corpus *c, const Batch &b, const AlignPartsCall &p, const AlRates &rates, int32_t B, int32_t *d_parts,
                    Workspace ws, int32_t n_ranks, void *hip_stream, ShardBlocks *blocks, LateCheck late = {}) {
    const AlignTopkForm &f = kAlignPartsForm;
    const int32_t Q = b.Q, max_query_len = b.max_query_len, k = p.k, max_parts = p.max_parts, min_votes = p.min_votes;
    const int32_t *d_video_ids = p.d_video_ids;
    const int64_t id_stride = p.id_stride, query_id_stride = p.query_id_stride;
    const double eps = p.eps;
    if (int rc = check_batch_args(c, b, 0)) return rc;
    if (Q == 0) return TVZ_OK;
    Carver cv(ws.p);
    const AlignPartsWs w = align_parts_ws_layout(cv, Q, k, max_parts, n_ranks);
    const AlignLds lds(max_query_len, B);
    auto args_ok = [&]() -> int {
        TVZ_REQUIRE(d_video_ids != nullptr && (d_parts != nullptr || w.local != nullptr), "NULL argument");
        if (d_parts == nullptr) d_parts = w.local;
        if (blocks) *blocks = ShardBlocks{d_parts, w.gathered};
        TVZ_REQUIRE(lds.fits(/* static LDS: none */ 0), "%s walk: %zu B of dynamic LDS exceed a gfx950 workgroup's", f.what,
                    lds.bytes);
        return late();
    };
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    TolCall t;                                                                // (the sort zeroes counts[0 .. Q) too)
    if (int rc = tol_prelude(c, b, TolFront{cv, cv.fixed(), w.counts, f.what, n_ranks > 0 ? f.sharded_sizer : f.sizer},
                             ws.p ? ws.bytes : 0, max_query_len, st, args_ok, t))
        return rc;
    const int64_t n_rows = t.n_rows;
    TVZ_HIP(hipMemsetAsync(w.counts, 0, (size_t)Q * (size_t)k * sizeof(int32_t), st));
    if (n_rows) {
        const unsigned row_blocks = (unsigned)std::min<int64_t>(tvz::ceil_div(n_rows, (int64_t)kApLocateBlock), kApLocateMaxBlocks);
        hipLaunchKernelGGL(ts_alignp_locate_kernel, dim3(row_blocks, (unsigned)Q), dim3(kApLocateBlock), 0, st, c->rows.p, n_rows,
                           d_video_ids, id_stride, query_id_stride, k, w.counts, w.slots);
        TVZ_HIP(hipGetLastError());
        const auto walk = (p.flags & kAlTwoBins) ? ts_alignp2_walk_kernel : ts_alignp_walk_kernel;   // (one argument list)
        hipLaunchKernelGGL(walk, dim3((unsigned)k, (unsigned)Q), dim3(kAlBlock), lds.bytes, st, c->rows.p,
                           c->keys.p, t.ws.sv, b.d_q_offsets, t.ws.qm, lds.lds_keys, eps, B, lds.width, rates, min_votes, max_parts,
                           d_video_ids, id_stride, query_id_stride, k, w.counts, w.slots, w.scratch);
        TVZ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ts_alignp_pick_kernel, dim3((unsigned)tvz::ceil_div((int64_t)Q * k, (int64_t)kApPickWaves)),
                       dim3(kApPickBlock), 0, st, d_video_ids, id_stride, query_id_stride, Q, k, max_parts, t.ws.qm, lds.lds_keys,
                       w.counts, w.slots, w.scratch, d_parts);
    TVZ_HIP(hipGetLastError());
    return record(c, st);
}

// A call of the C ABI, or the sharded form's local part: what is refused early, then the handle.
int align_parts_call(tvz_corpus *c, const Batch &b, const AlignPartsCall &p, int32_t *d_parts, Workspace ws, int32_t n_ranks,
                     void *hip_stream, ShardBlocks *blocks, LateCheck late = {}) {
    AlRates rates{};
    int32_t B = 0;
    if (int rc = check_align_parts_early(b, p, &rates, &B)) return rc;
    return align_parts_run(c, b, p, rates, B, d_parts, ws, n_ranks, hip_stream, blocks, late);
}

// what the parts merge refuses, apart from its pointers
int check_align_parts_merge(int32_t n_lists, int32_t k, int32_t max_parts) {
    if (n_lists < 1 || n_lists > kAlMergeMaxLists)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment parts merge: %d lists outside 1..%d", (int)n_lists, kAlMergeMaxLists);
    if (k < 1 || k > kAlMaxK) return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment parts merge: k=%d outside 1..%d", (int)k, kAlMaxK);
    if (max_parts < 1 || max_parts > kApMaxParts)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment parts merge: max_parts=%d outside 1..%d (TVZ_ALIGN_MAX_PARTS)",
                         (int)max_parts, kApMaxParts);
    return TVZ_OK;
}

// The shards of one process: every handle's call into its block of d_blocks, then the merge.
int align_parts_shards_impl(tvz_corpus *const *shards, int32_t n_shards, const Batch &b, const AlignPartsCall &p,
                            int32_t *d_blocks, int32_t *d_parts, Workspace ws, void *hip_stream) {
    const int32_t Q = b.Q;
    AlRates rates{};
    int32_t B = 0;
    if (int rc = check_align_parts_early(b, p, &rates, &B)) return rc;
    TVZ_REQUIRE(shards != nullptr && n_shards >= 1, "no shards");
    TVZ_REQUIRE(Q >= 0, "Q=%d is negative", (int)Q);
    if (int rc = check_align_parts_merge(n_shards, p.k, p.max_parts)) return rc;
    for (int32_t r = 0; r < n_shards; ++r)
        TVZ_REQUIRE(shards[r] != nullptr && shards[r]->device == shards[0]->device,
                    "shard %d is NULL or on another device than shard 0", r);
    TVZ_REQUIRE(Q == 0 || (d_blocks && d_parts && b.d_queries && b.d_q_offsets && p.d_video_ids), "NULL argument");
    if (Q == 0) return TVZ_OK;
    // every handle's call makes the same checks of the same arguments: what one refuses, the first one refuses, before
    // anything is enqueued
    const size_t block = (size_t)Q * (size_t)p.k * (size_t)ap_words(p.max_parts);
    for (int32_t r = 0; r < n_shards; ++r)
        if (int rc = align_parts_run(shards[r], b, p, rates, B, d_blocks + (size_t)r * block, ws, 0, hip_stream, nullptr)) return rc;
    DeviceGuard dg(shards[0]->device);
    return tvz_align_parts_merge_local(d_blocks, n_shards, Q, p.k, p.max_parts, d_parts, hip_stream);
}

}  // namespace

// used by tvz_comm.hip (same shared object, not exported): the parts call with the sharded form's blocks ...
int tvz_align_parts_local(tvz_corpus *c, const Batch &b, const AlignPartsCall &p, int32_t *d_parts, Workspace ws, int32_t n_ranks,
                          void *hip_stream, ShardBlocks *blocks, LateCheck late) {
    return align_parts_call(c, b, p, d_parts, ws, n_ranks, hip_stream, blocks, late);
}

// ... and the merge of the gathered answers
int tvz_align_parts_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, int32_t max_parts,
                                int32_t *d_parts, void *hip_stream) {
    TVZ_REQUIRE(Q >= 0, "Q=%d is negative", (int)Q);
    if (int rc = check_align_parts_merge(n_lists, k, max_parts)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_gathered && d_parts, "NULL argument");
    const int64_t pairs = (int64_t)Q * k;
    hipLaunchKernelGGL(ts_alignp_merge_kernel, dim3((unsigned)tvz::ceil_div(pairs, (int64_t)kApMergeGroups)), dim3(kApMergeBlock), 0,
                       reinterpret_cast<hipStream_t>(hip_stream), d_gathered, n_lists, pairs, max_parts, d_parts);
    return launched();
}

// used by tvz_comm.hip (same shared object, not exported): a form's call with the sharded forms' blocks
int tvz_align_topk_local(AlignForm form, tvz_corpus *c, const Batch &b, const AlignCall &a, const double *h_rates,
                         int32_t n_rates, uint32_t flags, int32_t k, int32_t *d_out, Workspace ws, int32_t n_ranks,
                         void *hip_stream, ShardBlocks *blocks, LateCheck late) {
    return align_topk_call(form, c, b, AlignAsk{a, h_rates, n_rates, flags, k}, d_out, ws, n_ranks, hip_stream, blocks, late);
}

int tvz_align_form_cols(AlignForm form) { return kAlignForms[form].cols; }

// ... and the merge of a form's blocks, rows of f.cols columns (the form without flags: 0)
int tvz_align_merge_local(AlignForm form, const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                          const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals,
                          void *hip_stream) {
    const AlignTopkForm &f = kAlignForms[form];
    TVZ_REQUIRE(Q >= 0, "Q=%d is negative", (int)Q);
    if (int rc = check_align_merge(n_lists, k)) return rc;
    if (int rc = check_align_flags(f, flags, " merge")) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_gathered && d_queries && d_q_offsets && d_topk && d_totals, "NULL argument");
    TVZ_REQUIRE(aligned16(d_gathered) && aligned16(d_topk), "alignment top-k merge: the blocks and d_topk must be 16-byte aligned");
    f.merge(AlignMergeArgs{dim3((unsigned)tvz::ceil_div(Q, kAlMergeWaves)), reinterpret_cast<hipStream_t>(hip_stream),
                           d_gathered, n_lists, Q, k, flags, d_queries, d_q_offsets, d_topk, d_totals});
    return launched();
}

// ---- candidate ids from the gap codes (include/tvz_gap.h; kernels: tvz_gap_kernels.h) ------------------------------
static int tvz_corpus_gap_index_impl(tvz_corpus *c, double gap_eps) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    if (!(gap_eps >= 0.0 && gap_eps <= DBL_MAX))          // refuses NaN, inf and negative values
        return tvz::fail(TVZ_ERR_INVALID, "gap_eps must be 0 (off) or finite and > 0 (got %g)", gap_eps);
    DeviceGuard dg(c->device);
    std::unique_lock<std::shared_mutex> lk(c->mu);
    wait_no_build(c, lk);
    if (int rc = drain(c)) return rc;
    if (gap_eps == 0.0) {
        if (c->gap) (void)tvz_corpus_destroy_impl(c->gap);    // (waits for the lookups in flight on it)
        c->gap = nullptr;
        c->gap_eps = 0.0;
        return TVZ_OK;
    }
    if (c->gap && c->gap_eps == gap_eps) return TVZ_OK;
    if (!c->gap)
        if (int rc = tvz_corpus_create_impl(&c->gap, c->device)) { c->gap = nullptr; return rc; }
    c->gap_eps = gap_eps;
    int rc = gap_upload(c);
    if (rc) {                                             // no half-made table: off, the caller may ask again
        char msg[512];
        snprintf(msg, sizeof msg, "%s", tvz::err_buf());
        (void)tvz_corpus_destroy_impl(c->gap);
        c->gap = nullptr;
        c->gap_eps = 0.0;
        snprintf(tvz::err_buf(), 512, "%s", msg);
    }
    return rc;
}

static int tvz_corpus_gap_index_stats_impl(tvz_corpus *c, double *gap_eps, int64_t *out) {
    TVZ_REQUIRE(c != nullptr, "corpus is NULL");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (gap_eps) *gap_eps = c->gap ? c->gap_eps : 0.0;
    if (!out) return TVZ_OK;
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!c->gap) return TVZ_OK;
    if (int rc = tvz_corpus_stats_impl(c->gap, &out[0], &out[1], nullptr)) return rc;
    return tvz_corpus_index_stats_impl(c->gap, &out[2], &out[3], nullptr, nullptr, &out[4]);
}

namespace {

// what the call refuses before it looks at the workspace or the handle, in the header's order
int check_candidates_args(int32_t max_query_len, int32_t min_count, int32_t cap, int32_t C) {
    if (C < 1 || C > tvz_gap::kMaxC)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: C=%d outside 1..%d", (int)C, tvz_gap::kMaxC);
    if (cap < C) return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: cap=%d below C=%d", (int)cap, (int)C);
    TVZ_REQUIRE(min_count >= 1, "alignment candidates: min_count %d below 1", (int)min_count);
    if (max_query_len > kAlMaxLen)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: max_query_len %d above %d", (int)max_query_len, kAlMaxLen);
    return TVZ_OK;
}

// the lookup's own workspace: `lists` probe lists of up to max_probe_len slots, hit lists in the caller's (this call's) regions
size_t candidates_match_bytes(int32_t lists, int32_t max_query_len) {
    return ws_layout(nullptr, 0, lists, tvz_gap::max_probe_len(max_query_len), 0, 0, 1).total;
}

constexpr int32_t kGaprMaxLists = 65535;      // probe lists of one lookup: Q * n_rates

// What a form of the candidates call is, on the host: tvz_align_candidates and tvz_align_candidates_rates are one entry
// each, and candidates_plan / candidates_enqueue below ask the entry, never which form they have.  The forms share the
// sorted queries, the offsets, the probes and the lookup over Q * n_rates probe lists (the plain form: one list per
// query at the rate 1.0); they differ in their last launch and in the row it writes.  A sharded form of the rates call
// would be its exports and a merge - the front in the workspace is already a parameter of the plan.
struct CandidatesPlan;
struct CandidatesForm {
    int cols;                        // int32 columns of a block row
    int out_align;                   // bytes d_out must be aligned to: a row is one vector store
    bool takes_rates;                // the call has a rate list, and with it a region for the lists' exclusion ids
    const char *what, *sizer;        // the call in messages; the sizing function the workspace message names
    void (*last)(const CandidatesPlan &);    // the launch behind the lookup
    // the merge of n_lists gathered blocks of the form's rows (the sharded calls)
    void (*merge)(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out, hipStream_t st);
};

struct CandidatesCall {              // what a call asks, apart from its queries; h_rates, n_rates: NULL, 1 without a rate list
    const double *h_rates;
    int32_t n_rates, min_count, cap, C;
    int32_t *d_out;
};
// The sharded form's blocks take `bytes` of the caller's buffer in front of the call's part - the plan is given the
// WHOLE buffer's size and where the call's part starts - and a workspace refusal names `sizer` (NULL: the form's).
struct CandidatesFront {
    size_t bytes = 0;
    const char *sizer = nullptr;
};

// Everything candidates_plan decided, for candidates_enqueue to launch from.  It holds the handle's lock (parent, then
// - inside the lookup - child) from the plan's look at the handle to the end of the enqueue: a plan is made, enqueued
// and dropped inside one call, one handle at a time.  Q = 0: nothing planned, nothing held, nothing to enqueue.
struct CandidatesPlan {
    const CandidatesForm *f = nullptr;
    tvz_corpus *c = nullptr;
    Batch b{};
    CandidatesCall a{};
    AlRates rates{};
    int32_t lists = 0;               // Q * n_rates
    size_t match_bytes = 0;
    int64_t room = 0;
    int32_t *hits = nullptr, *hits_n = nullptr, *excl = nullptr, *qm = nullptr, *sp = nullptr;
    int64_t *p_off = nullptr;
    double *sv = nullptr, *probes = nullptr;
    unsigned char *match = nullptr;
    double gap_eps = 0.0;            // the width of the handle's codes, read under its lock
    void *hip_stream = nullptr;
    std::optional<DeviceGuard> dg;   // (declared in front of the lock: the lock goes first)
    std::shared_lock<std::shared_mutex> lk;
    hipStream_t st() const { return reinterpret_cast<hipStream_t>(hip_stream); }
};

constexpr CandidatesForm kCandidatesPlain = {
    2, 8, false, "alignment candidates", "tvz_align_candidates_workspace_bytes", [](const CandidatesPlan &p) {
        hipLaunchKernelGGL(ts_gapc_select_kernel, dim3((unsigned)p.b.Q), dim3(kBlock), 0, p.st(), p.hits, p.hits_n, p.qm, p.a.cap,
                           p.a.C, p.a.d_out);
    },
    [](const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out, hipStream_t st) {
        hipLaunchKernelGGL(ts_gapc_merge_kernel, dim3((unsigned)tvz::ceil_div(Q, kGapMergeWaves)), dim3(kGapMergeBlock),
                           gapc_merge_lds_bytes(n_lists, C), st, d_gathered, n_lists, Q, C, d_out);
    }};
constexpr CandidatesForm kCandidatesRates = {
    3, 4, true, "alignment candidates with rates", "tvz_align_candidates_rates_workspace_bytes", [](const CandidatesPlan &p) {
        hipLaunchKernelGGL(ts_gapr_fold_kernel, dim3((unsigned)p.b.Q), dim3(kBlock), 0, p.st(), p.hits, p.hits_n, p.qm, p.rates.n,
                           p.a.cap, p.a.C, p.a.d_out);
    },
    [](const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out, hipStream_t st) {
        hipLaunchKernelGGL(ts_gapr_merge_kernel, dim3((unsigned)Q), dim3(kBlock), 0, st, d_gathered, n_lists, Q, C, d_out);
    }};

// What a form refuses of its arguments before it looks at the handle, the queries or the workspace, in the headers'
// order; the checked rate list goes to `rates` (the plain form: {1.0}).
int check_candidates_front(const CandidatesForm &f, const Batch &b, const CandidatesCall &a, AlRates *rates) {
    if (int rc = check_candidates_args(b.max_query_len, a.min_count, a.cap, a.C)) return rc;
    *rates = AlRates{{1.0}, 1};
    if (f.takes_rates) {
        if (int rc = check_align_rates(a.h_rates, a.n_rates, rates)) return rc;
        if ((int64_t)b.Q * a.n_rates > kGaprMaxLists)
            return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: Q=%d x n_rates=%d is above %d probe lists", f.what, (int)b.Q, (int)a.n_rates,
                             kGaprMaxLists);
    }
    return TVZ_OK;
}

// Everything in front of the first launch: the refusals in the headers' order, the carving of `ws` (the call's part of
// the caller's buffer; ws.bytes: the whole buffer's, `front` included), the handle's lock and what is read under it.
// `late`: what a sharded form still refuses behind all of the call's own refusals.
int candidates_plan(const CandidatesForm &f, tvz_corpus *c, const Batch &b, const CandidatesCall &a, Workspace ws,
                    void *hip_stream, LateCheck late, CandidatesFront front, CandidatesPlan &p) {
    if (int rc = check_candidates_front(f, b, a, &p.rates)) return rc;
    if (int rc = check_batch_args(c, b, a.cap)) return rc;
    p.f = &f, p.c = c, p.b = b, p.a = a, p.hip_stream = hip_stream;
    if (b.Q == 0) return TVZ_OK;
    const int32_t R = p.rates.n;
    p.lists = b.Q * R;
    p.match_bytes = candidates_match_bytes(p.lists, b.max_query_len);
    const size_t whole = ws.p ? ws.bytes : 0;
    const size_t need = tvz_gap::ws_bytes(b.Q, R, f.takes_rates, a.cap, p.match_bytes, b.max_query_len) + front.bytes;
    if (whole < need)
        return tvz::fail(TVZ_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu bytes missing (size it with %s)", f.what, whole,
                         need - whole, front.sizer ? front.sizer : f.sizer);
    TVZ_REQUIRE(a.d_out != nullptr && (reinterpret_cast<uintptr_t>(a.d_out) & (uintptr_t)(f.out_align - 1)) == 0,
                "d_out is NULL or not %d-byte aligned", f.out_align);
    p.room = tvz_gap::ws_room(b.Q, R, f.takes_rates, a.cap, p.match_bytes, whole - front.bytes);
    const tvz_gap::WsRegions r = tvz_gap::ws_regions(b.Q, R, f.takes_rates, a.cap, p.match_bytes, p.room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(reinterpret_cast<uintptr_t>(ws.p)));
    p.hits = reinterpret_cast<int32_t *>(base + r.hits), p.hits_n = reinterpret_cast<int32_t *>(base + r.hits_n);
    p.p_off = reinterpret_cast<int64_t *>(base + r.p_off);
    // (the lists' exclusion ids: a form with several lists per query has the region, a call with exclusions uses it)
    p.excl = f.takes_rates && b.d_exclude_ids ? reinterpret_cast<int32_t *>(base + r.excl) : nullptr;
    p.match = base + r.match;
    p.qm = reinterpret_cast<int32_t *>(base + r.qm), p.sp = reinterpret_cast<int32_t *>(base + r.sp);
    p.sv = reinterpret_cast<double *>(base + r.sv), p.probes = reinterpret_cast<double *>(base + r.probes);
    p.dg.emplace(c->device);
    p.lk = std::shared_lock<std::shared_mutex>(c->mu);        // parent, then (inside the lookup) child
    if (!c->gap)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: this corpus keeps no gap codes (tvz_corpus_gap_index)");
    p.gap_eps = c->gap_eps;
    return late();
}

// The launches of a plan: the sort, the offsets, the probes, ONE lookup over the probe lists, the form's last launch.
int candidates_enqueue(const CandidatesPlan &p) {
    const Batch &b = p.b;
    if (b.Q == 0) return TVZ_OK;
    hipStream_t st = p.st();
    // the sorted queries, once for all rates (it zeroes the first Q counts; the lookup writes every one of the lists')
    hipLaunchKernelGGL(ts_tol_sort_kernel, dim3((unsigned)tvz::ceil_div(std::max(b.max_query_len, 1), kTolSortBlock), (unsigned)b.Q),
                       dim3(kTolSortBlock), 0, st, b.d_queries, b.d_q_offsets, b.max_query_len, p.room, p.sv, p.sp, p.qm, p.hits_n);
    TVZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(ts_gapc_offsets_kernel, dim3(1), dim3(kGapOffBlock), 0, st, p.qm, b.Q, p.rates.n, b.d_exclude_ids, p.p_off,
                       p.excl);
    TVZ_HIP(hipGetLastError());
    if (b.max_query_len >= 4) {
        hipLaunchKernelGGL(ts_gapc_probe_kernel,
                           dim3((unsigned)tvz::ceil_div(b.max_query_len - 3, kGapProbeBlock), (unsigned)b.Q, (unsigned)p.rates.n),
                           dim3(kGapProbeBlock), 0, st, p.sv, b.d_q_offsets, p.qm, p.gap_eps, p.rates, p.p_off, p.probes);
        TVZ_HIP(hipGetLastError());
    }
    // count_i(q, r) is the exact match's count of list q R + i over the codes: the index, its delta table, the
    // exclusions - one id per list, the caller's own where the lists are the queries
    if (int rc = tvz_match_impl(p.c->gap, p.probes, p.p_off, p.lists, tvz_gap::max_probe_len(b.max_query_len), p.a.min_count,
                                p.excl ? p.excl : b.d_exclude_ids, p.a.cap, p.hits, p.hits_n, p.match, p.match_bytes,
                                TVZ_ALGO_AUTO, p.hip_stream))
        return rc;
    p.f->last(p);
    TVZ_HIP(hipGetLastError());
    return record(p.c, st);
}

// a call of the C ABI: its plan, enqueued
int candidates_call(const CandidatesForm &f, tvz_corpus *c, const Batch &b, const CandidatesCall &a, Workspace ws, void *hip_stream,
                    LateCheck late = {}, CandidatesFront front = {}) {
    CandidatesPlan p;
    if (int rc = candidates_plan(f, c, b, a, ws, hip_stream, late, front, p)) return rc;
    return candidates_enqueue(p);
}

// What the sizing exports share: the argument refusals, the `keys` default and the room for one longest query.
size_t candidates_sizing(const CandidatesForm &f, int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t n_rates,
                         int32_t cap, int32_t C) {
    if (Q < 0 || Q > 65535 || max_query_len < 0 || max_query_len > kAlMaxLen || total_query_keys < 0 || C < 1 ||
        C > tvz_gap::kMaxC || cap < C)
        return 0;
    if (f.takes_rates && (n_rates < 1 || n_rates > kArMaxRates || (int64_t)Q * n_rates > kGaprMaxLists)) return 0;
    const int64_t keys = total_query_keys > 0 ? total_query_keys : (int64_t)Q * max_query_len;
    return tvz_gap::ws_bytes(Q, n_rates, f.takes_rates, cap, candidates_match_bytes(Q * n_rates, max_query_len),
                             std::max<int64_t>(keys, max_query_len));
}

// ---- the candidates for long uploads (include/tvz_gap_long.h; kernels: tvz_gap_long_kernels.h) ----------------------
// The plain call's steps with S probe lists per query, S the segments of the call's longest query: the sorted queries,
// the lists' offsets and the probes (kernels of their own), ONE lookup over the Q S lists, the fold that sums per id.
// It stands beside the form table, whose entries and whose plan are what they were: it shares their argument checks
// (check_candidates_args, check_batch_args), the lookup's sizing and nothing else.
constexpr const char *kCandidatesLongWhat = "alignment candidates";

// what the call refuses behind the plain call's own refusals, in the header's order; -> the lists per query
int check_candidates_long(const Batch &b, int32_t min_count, int32_t cap, int32_t C, int32_t *S) {
    if (int rc = check_candidates_args(b.max_query_len, min_count, cap, C)) return rc;
    *S = tvz_gap::long_lists(b.max_query_len);
    if ((int64_t)b.Q * *S > kGaprMaxLists)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: Q=%d x %d segments is above %d probe lists", kCandidatesLongWhat, (int)b.Q, (int)*S,
                         kGaprMaxLists);
    if ((int64_t)*S * cap * tvz_gap::kLongSegSlots > INT32_MAX)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: %d segments x cap=%d x %d probe slots is above %d", kCandidatesLongWhat, (int)*S,
                         (int)cap, tvz_gap::kLongSegSlots, INT32_MAX);
    return TVZ_OK;
}

int candidates_long_call(tvz_corpus *c, const Batch &b, int32_t min_count, int32_t cap, int32_t C, int32_t *d_out, Workspace ws,
                         void *hip_stream) {
    int32_t S = 1;
    if (int rc = check_candidates_long(b, min_count, cap, C, &S)) return rc;
    if (int rc = check_batch_args(c, b, cap)) return rc;
    if (b.Q == 0) return TVZ_OK;
    const int32_t lists = b.Q * S;
    const size_t match_bytes = candidates_match_bytes(lists, b.max_query_len);
    const size_t whole = ws.p ? ws.bytes : 0;
    const size_t need = tvz_gap::ws_long_bytes(b.Q, S, cap, match_bytes, b.max_query_len);
    if (whole < need)
        return tvz::fail(TVZ_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu bytes missing (size it with %s)", kCandidatesLongWhat, whole,
                         need - whole, "tvz_align_candidates_long_workspace_bytes");
    TVZ_REQUIRE(d_out != nullptr && (reinterpret_cast<uintptr_t>(d_out) & (uintptr_t)7) == 0, "d_out is NULL or not %d-byte aligned", 8);
    const int64_t room = tvz_gap::ws_long_room(b.Q, S, cap, match_bytes, whole);
    const tvz_gap::WsLongRegions r = tvz_gap::ws_long_regions(b.Q, S, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(reinterpret_cast<uintptr_t>(ws.p)));
    int32_t *hits = reinterpret_cast<int32_t *>(base + r.hits), *hits_n = reinterpret_cast<int32_t *>(base + r.hits_n);
    int64_t *p_off = reinterpret_cast<int64_t *>(base + r.p_off);
    // (the lists' exclusion ids: the lookup reads one id per probe list; a call with exclusions copies the query's to each)
    int32_t *excl = b.d_exclude_ids ? reinterpret_cast<int32_t *>(base + r.excl) : nullptr;
    unsigned char *match = base + r.match;
    int32_t *qm = reinterpret_cast<int32_t *>(base + r.qm), *sp = reinterpret_cast<int32_t *>(base + r.sp);
    double *sv = reinterpret_cast<double *>(base + r.sv), *probes = reinterpret_cast<double *>(base + r.probes);
    int2 *table = reinterpret_cast<int2 *>(base + r.table);
    const size_t table_slots = tvz_gap::long_ws_table_slots(S, cap);
    DeviceGuard dg(c->device);
    std::shared_lock<std::shared_mutex> lk(c->mu);            // parent, then (inside the lookup) child
    if (!c->gap)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: this corpus keeps no gap codes (tvz_corpus_gap_index)");
    const double gap_eps = c->gap_eps;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(ts_tol_sort_kernel, dim3((unsigned)tvz::ceil_div(std::max(b.max_query_len, 1), kTolSortBlock), (unsigned)b.Q),
                       dim3(kTolSortBlock), 0, st, b.d_queries, b.d_q_offsets, b.max_query_len, room, sv, sp, qm, hits_n);
    TVZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(ts_gapl_offsets_kernel, dim3(1), dim3(kGapOffBlock), 0, st, qm, b.Q, S, b.d_exclude_ids, p_off, excl);
    TVZ_HIP(hipGetLastError());
    if (b.max_query_len >= 4) {
        hipLaunchKernelGGL(ts_gapl_probe_kernel, dim3((unsigned)tvz::ceil_div(b.max_query_len - 3, kGapProbeBlock), (unsigned)b.Q),
                           dim3(kGapProbeBlock), 0, st, sv, b.d_q_offsets, qm, gap_eps, S, p_off, probes);
        TVZ_HIP(hipGetLastError());
    }
    if (int rc = tvz_match_impl(c->gap, probes, p_off, lists, tvz_gap::max_probe_len(b.max_query_len), min_count,
                                excl ? excl : b.d_exclude_ids, cap, hits, hits_n, match, match_bytes, TVZ_ALGO_AUTO, hip_stream))
        return rc;
    hipLaunchKernelGGL(ts_gapl_fold_kernel, dim3((unsigned)b.Q), dim3(kBlock), 0, st, hits, hits_n, qm, S, cap, C, table, table_slots,
                       d_out);
    TVZ_HIP(hipGetLastError());
    return record(c, st);
}

size_t candidates_long_sizing(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap, int32_t C) {
    if (Q < 0 || Q > 65535 || max_query_len < 0 || max_query_len > kAlMaxLen || total_query_keys < 0 || C < 1 ||
        C > tvz_gap::kMaxC || cap < C)
        return 0;
    const int32_t S = tvz_gap::long_lists(max_query_len);
    if ((int64_t)Q * S > kGaprMaxLists || (int64_t)S * cap * tvz_gap::kLongSegSlots > INT32_MAX) return 0;
    const int64_t keys = total_query_keys > 0 ? total_query_keys : (int64_t)Q * max_query_len;
    return tvz_gap::ws_long_bytes(Q, S, cap, candidates_match_bytes(Q * S, max_query_len), std::max<int64_t>(keys, max_query_len));
}

}  // namespace

// ---- the candidates over a sharded table (include/tvz_gap_shards.h) ---------------------------------------------
namespace {

// what the candidates merge refuses, apart from its pointers
int check_candidates_merge(int32_t n_lists, int32_t C) {
    if (n_lists < 1 || n_lists > kGapMergeMaxLists)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates merge: %d lists outside 1..%d", (int)n_lists, kGapMergeMaxLists);
    if (C < 1 || C > tvz_gap::kMaxC)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates merge: C=%d outside 1..%d", (int)C, tvz_gap::kMaxC);
    return TVZ_OK;
}

// a pointer to rows of a form's block: aligned to the row's vector store
bool aligned_rows(const CandidatesForm &f, const void *p) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(f.out_align - 1)) == 0; }
size_t form_block_bytes(const CandidatesForm &f, int32_t Q, int32_t C) { return (size_t)Q * ((size_t)C + 1) * (size_t)f.cols * sizeof(int32_t); }

// the merge of n_lists gathered blocks of a form: its refusals, then the form's one launch
int candidates_merge_local(const CandidatesForm &f, const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C,
                           int32_t *d_out, void *hip_stream) {
    if (int rc = check_candidates_merge(n_lists, C)) return rc;
    TVZ_REQUIRE(Q >= 0, "Q=%d is negative", (int)Q);
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_gathered && d_out, "NULL argument");
    TVZ_REQUIRE(aligned_rows(f, d_gathered) && aligned_rows(f, d_out),
                "alignment candidates merge: the blocks and d_out must be %d-byte aligned", f.out_align);
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(d_gathered), o0 = reinterpret_cast<uintptr_t>(d_out);
    const size_t block = form_block_bytes(f, Q, C);
    TVZ_REQUIRE(o0 + block <= g0 || g0 + (size_t)n_lists * block <= o0, "alignment candidates merge: d_out lies inside the blocks");
    f.merge(d_gathered, n_lists, Q, C, d_out, reinterpret_cast<hipStream_t>(hip_stream));
    return launched();
}

// The local call of a form with the sharded form's blocks in front of its workspace (tvz_gap_codes.h: ws_shard_carve
// with the form's columns).
int candidates_local(const CandidatesForm &f, const char *sharded_sizer, tvz_corpus *c, const Batch &b, const double *h_rates,
                     int32_t n_rates, int32_t min_count, int32_t cap, int32_t C, Workspace ws, int32_t n_ranks, void *hip_stream,
                     ShardBlocks *blocks, LateCheck late) {
    // (arguments the carving cannot take are refused by the call itself, in front of its look at the workspace)
    const bool carve = ws.p != nullptr && b.Q > 0 && b.Q <= 65535 && C >= 1 && C <= tvz_gap::kMaxC;
    tvz_gap::ShardWs s{0, 0, 0};
    if (carve) s = tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(ws.p), ws.bytes, b.Q, C, n_ranks, f.cols);
    int32_t *local = reinterpret_cast<int32_t *>(s.front);
    if (carve && blocks) {
        const tvz_gap::ShardWsRegions r = tvz_gap::ws_shard_regions(b.Q, C, n_ranks, f.cols);
        *blocks = ShardBlocks{local, reinterpret_cast<int32_t *>(s.front + r.gathered)};
    }
    // the call judges the WHOLE buffer's size, front included, and lays its own part out from s.plain on
    const size_t front_bytes = carve ? tvz_gap::ws_shard_front_bytes(b.Q, C, n_ranks, f.cols) : 0;
    return candidates_call(f, c, b, CandidatesCall{h_rates, n_rates, min_count, cap, C, local},
                           Workspace{carve ? reinterpret_cast<void *>(s.plain) : nullptr, ws.bytes}, hip_stream, late,
                           CandidatesFront{front_bytes, sharded_sizer});
}

// The shards of one process: every handle's call of the form into its block of d_blocks, then the merge.
int candidates_shards(const CandidatesForm &f, tvz_corpus *const *shards, int32_t n_shards, const Batch &b, const double *h_rates,
                      int32_t n_rates, int32_t min_count, int32_t cap, int32_t C, int32_t *d_blocks, int32_t *d_out, Workspace ws,
                      void *hip_stream) {
    const int32_t Q = b.Q;
    AlRates rates;
    if (int rc = check_candidates_front(f, b, CandidatesCall{h_rates, n_rates, min_count, cap, C, nullptr}, &rates)) return rc;
    TVZ_REQUIRE(shards != nullptr && n_shards >= 1, "no shards");
    if (int rc = check_candidates_merge(n_shards, C)) return rc;
    for (int32_t r = 0; r < n_shards; ++r)
        TVZ_REQUIRE(shards[r] != nullptr && shards[r]->device == shards[0]->device,
                    "shard %d is NULL or on another device than shard 0", r);
    if (int rc = check_batch_args(shards[0], b, cap)) return rc;
    if (Q == 0) return TVZ_OK;
    TVZ_REQUIRE(d_blocks && d_out && aligned_rows(f, d_blocks) && aligned_rows(f, d_out),
                "d_blocks or d_out is NULL or not %d-byte aligned", f.out_align);
    const size_t block = form_block_bytes(f, Q, C);
    {
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(d_blocks), o0 = reinterpret_cast<uintptr_t>(d_out);
        TVZ_REQUIRE(o0 + block <= g0 || g0 + (size_t)n_shards * block <= o0, "alignment candidates merge: d_out lies inside the blocks");
    }
    auto call_of = [&](int32_t r) {
        return CandidatesCall{h_rates, n_rates, min_count, cap, C, d_blocks + (size_t)r * (block / sizeof(int32_t))};
    };
    // Every handle is planned first - the arguments' refusals are the same for all, the handle's own (no gap codes) are
    // not - and the widths compared: nothing is enqueued before all of them agree.  A plan holds its handle's lock, and
    // the locks are taken one handle at a time (the shards may name a handle twice, and two callers may name them in
    // different orders), so these plans are dropped again and every shard is planned anew where it is enqueued.
    double eps0 = 0.0;
    for (int32_t r = 0; r < n_shards; ++r) {
        CandidatesPlan p;
        if (int rc = candidates_plan(f, shards[r], b, call_of(r), ws, hip_stream, {}, {}, p)) return rc;
        if (r == 0) eps0 = p.gap_eps;
        if (p.gap_eps != eps0)
            return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment candidates: shard %d keeps gap codes of gap_eps=%.17g, shard 0 of %.17g",
                             (int)r, p.gap_eps, eps0);
    }
    for (int32_t r = 0; r < n_shards; ++r)
        if (int rc = candidates_call(f, shards[r], b, call_of(r), ws, hip_stream)) return rc;
    DeviceGuard dg(shards[0]->device);
    return candidates_merge_local(f, d_blocks, n_shards, Q, C, d_out, hip_stream);
}

}  // namespace

// used by tvz_comm.hip too (same shared object, not exported): the merges of the gathered blocks ...
int tvz_align_candidates_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                     void *hip_stream) {
    return candidates_merge_local(kCandidatesPlain, d_gathered, n_lists, Q, C, d_out, hip_stream);
}
int tvz_align_candidates_rates_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                           void *hip_stream) {
    return candidates_merge_local(kCandidatesRates, d_gathered, n_lists, Q, C, d_out, hip_stream);
}

// ... and the local calls with the sharded forms' blocks in front of their workspaces
int tvz_align_candidates_local(tvz_corpus *c, const Batch &b, int32_t min_count, int32_t cap, int32_t C, Workspace ws,
                               int32_t n_ranks, void *hip_stream, ShardBlocks *blocks, LateCheck late) {
    return candidates_local(kCandidatesPlain, "tvz_align_candidates_sharded_workspace_bytes", c, b, nullptr, 1, min_count, cap, C, ws,
                            n_ranks, hip_stream, blocks, late);
}
int tvz_align_candidates_rates_local(tvz_corpus *c, const Batch &b, const double *h_rates, int32_t n_rates, int32_t min_count,
                                     int32_t cap, int32_t C, Workspace ws, int32_t n_ranks, void *hip_stream, ShardBlocks *blocks,
                                     LateCheck late) {
    return candidates_local(kCandidatesRates, "tvz_align_candidates_rates_sharded_workspace_bytes", c, b, h_rates, n_rates, min_count,
                            cap, C, ws, n_ranks, hip_stream, blocks, late);
}

size_t tvz_align_candidates_sharded_sizing(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap, int32_t C,
                                           int32_t n_ranks) {
    const size_t plain = tvz_align_candidates_workspace_bytes(Q, max_query_len, total_query_keys, cap, C);
    if (plain == 0 || n_ranks < 0) return 0;
    return plain + tvz_gap::ws_shard_front_bytes(Q, C, n_ranks);
}

TVZ_EXPORT int tvz_align_candidates_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                          void *hip_stream) {
    TVZ_GUARDED(tvz_align_candidates_merge_local(d_gathered, n_lists, Q, C, d_out, hip_stream));
}

TVZ_EXPORT int tvz_align_candidates_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                           const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, int32_t min_count,
                                           const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_blocks,
                                           int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(candidates_shards(kCandidatesPlain, shards, n_shards, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  nullptr, 1, min_count, cap, C, d_blocks, d_out, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_candidates_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                               int32_t cap, int32_t C, int32_t n_ranks) {
    return tvz_align_candidates_sharded_sizing(Q, max_query_len, total_query_keys, cap, C, n_ranks);
}

TVZ_EXPORT int tvz_corpus_gap_index(tvz_corpus *c, double gap_eps) {
    TVZ_GUARDED(tvz_corpus_gap_index_impl(c, gap_eps));
}

TVZ_EXPORT int tvz_corpus_gap_index_stats(tvz_corpus *c, double *gap_eps, int64_t out[5]) {
    TVZ_GUARDED(tvz_corpus_gap_index_stats_impl(c, gap_eps, out));
}

TVZ_EXPORT size_t tvz_align_candidates_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap,
                                                       int32_t C) {
    return candidates_sizing(kCandidatesPlain, Q, max_query_len, total_query_keys, 1, cap, C);
}

TVZ_EXPORT int tvz_align_candidates(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                    int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap, int32_t C,
                                    int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(candidates_call(kCandidatesPlain, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                CandidatesCall{nullptr, 1, min_count, cap, C, d_out}, Workspace{d_workspace, workspace_bytes},
                                hip_stream));
}

// ---- the candidates for long uploads (include/tvz_gap_long.h) -----------------------------------------------------
TVZ_EXPORT size_t tvz_align_candidates_long_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap,
                                                            int32_t C) {
    return candidates_long_sizing(Q, max_query_len, total_query_keys, cap, C);
}

TVZ_EXPORT int tvz_align_candidates_long(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                         int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap,
                                         int32_t C, int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(candidates_long_call(c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids), min_count, cap, C, d_out,
                                     Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_candidates_rates_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                             int32_t n_rates, int32_t cap, int32_t C) {
    return candidates_sizing(kCandidatesRates, Q, max_query_len, total_query_keys, n_rates, cap, C);
}

TVZ_EXPORT int tvz_align_candidates_rates(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                          int32_t max_query_len, const double *h_rates, int32_t n_rates, int32_t min_count,
                                          const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_out,
                                          void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(candidates_call(kCandidatesRates, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                CandidatesCall{h_rates, n_rates, min_count, cap, C, d_out}, Workspace{d_workspace, workspace_bytes},
                                hip_stream));
}

// ---- the rates call over a sharded table (include/tvz_gap_rates_shards.h) ------------------------------------------
TVZ_EXPORT int tvz_align_candidates_rates_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                                void *hip_stream) {
    TVZ_GUARDED(tvz_align_candidates_rates_merge_local(d_gathered, n_lists, Q, C, d_out, hip_stream));
}

TVZ_EXPORT int tvz_align_candidates_rates_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                                 const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, const double *h_rates,
                                                 int32_t n_rates, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap,
                                                 int32_t C, int32_t *d_blocks, int32_t *d_out, void *d_workspace,
                                                 size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(candidates_shards(kCandidatesRates, shards, n_shards, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  h_rates, n_rates, min_count, cap, C, d_blocks, d_out, Workspace{d_workspace, workspace_bytes},
                                  hip_stream));
}

TVZ_EXPORT size_t tvz_align_candidates_rates_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                                     int32_t n_rates, int32_t cap, int32_t C, int32_t n_ranks) {
    const size_t rates = tvz_align_candidates_rates_workspace_bytes(Q, max_query_len, total_query_keys, n_rates, cap, C);
    if (rates == 0 || n_ranks < 0) return 0;
    return rates + tvz_gap::ws_shard_front_bytes(Q, C, n_ranks, kCandidatesRates.cols);
}

#ifdef TVZ_IX_STAMP
// diagnostic build only: read (and clear) the per-phase cycle totals of ts_match_index_kernel
TVZ_EXPORT int tvz_debug_ix_stamps(unsigned long long *out16) {
    TVZ_HIP(hipDeviceSynchronize());
    TVZ_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ix_stamps), 16 * 8));
    unsigned long long z[16] = {};
    TVZ_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_ix_stamps), z, 16 * 8));
    return TVZ_OK;
}
#endif

TVZ_EXPORT size_t tvz_match_workspace_bytes(int32_t Q, int32_t max_query_len, int32_t cap, int32_t k,
                                            int32_t n_ranks) {
    if (Q < 0 || max_query_len < 0 || cap < 0 || k < 0) return 0;
    return ws_layout(nullptr, 0, Q, max_query_len, cap, k, n_ranks).total;
}

TVZ_EXPORT size_t tvz_match_workspace_bytes_long(int32_t Q, int32_t max_query_len, int32_t cap, int32_t k,
                                                 int32_t n_ranks, int64_t total_query_keys) {
    if (Q < 0 || max_query_len < 0 || cap < 0 || k < 0 || total_query_keys < 0) return 0;
    return ws_layout(nullptr, 0, Q, max_query_len, cap, k, n_ranks, std::max<int64_t>(total_query_keys, max_query_len)).total;
}

TVZ_EXPORT int tvz_corpus_create(tvz_corpus **out, int device) {
    TVZ_GUARDED(tvz_corpus_create_impl(out, device));
}

TVZ_EXPORT int tvz_corpus_destroy(tvz_corpus *c) {
    TVZ_GUARDED(tvz_corpus_destroy_impl(c));
}

TVZ_EXPORT int tvz_corpus_reserve(tvz_corpus *c, int64_t n_rows, int64_t n_keys) {
    TVZ_GUARDED(tvz_corpus_reserve_impl(c, n_rows, n_keys));
}

TVZ_EXPORT int tvz_corpus_upload(tvz_corpus *c, const int32_t *h_video_ids,
                                 const int64_t *h_offsets, const double *h_keys, int64_t n_rows,
                                 int64_t n_keys) {
    TVZ_GUARDED(tvz_corpus_upload_impl(c, h_video_ids, h_offsets, h_keys, n_rows, n_keys));
}

TVZ_EXPORT int tvz_corpus_build_index(tvz_corpus *c) {
    TVZ_GUARDED(tvz_corpus_build_index_impl(c));
}

static int tvz_corpus_bucket_stats_impl(tvz_corpus *c, int64_t *out) {
    TVZ_REQUIRE(c != nullptr && out != nullptr, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const Index &ix = c->ix;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!ix.valid) return TVZ_OK;
    const IndexBuf &b = ix.now();
    out[0] = b.keys.nb;
    out[1] = b.keys.nb ? b.n_spilled : 0;
    out[2] = b.keys.nb ? b.max_spill : 0;
    out[3] = b.keys.nb ? b.n_ext : 0;
    out[4] = b.keys.nb ? b.ext_used : 0;
    out[5] = b.n_sub;
    return TVZ_OK;
}

TVZ_EXPORT int tvz_corpus_bucket_stats(tvz_corpus *c, int64_t out[6]) {
    TVZ_GUARDED(tvz_corpus_bucket_stats_impl(c, out));
}

static int tvz_corpus_index_layout_impl(tvz_corpus *c, int64_t *out) {
    TVZ_REQUIRE(c != nullptr && out != nullptr, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    const Index &ix = c->ix;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!ix.valid || ix.now().keys.nb) return TVZ_OK;
    const IndexBuf &b = ix.now();
    const Directory *dirs[2] = {&b.keys, b.t_cell > 0.0 ? &b.cells : nullptr};
    for (int i = 0; i < 2; ++i) {
        if (!dirs[i]) continue;
        out[4 * i + 0] = ix_entry_bytes(dirs[i]->ks);
        out[4 * i + 1] = dirs[i]->log2;
        out[4 * i + 2] = dirs[i]->slice_log2;
        out[4 * i + 3] = dirs[i]->partitioned ? 1 : 0;
    }
    return TVZ_OK;
}

TVZ_EXPORT int tvz_corpus_index_layout(tvz_corpus *c, int64_t out[8]) {
    TVZ_GUARDED(tvz_corpus_index_layout_impl(c, out));
}

TVZ_EXPORT int tvz_corpus_index_stats(tvz_corpus *c, int64_t *n_indexed_rows, int64_t *n_delta_rows,
                                      int64_t *n_postings, int64_t *n_distinct_keys, int64_t *n_builds) {
    TVZ_GUARDED(tvz_corpus_index_stats_impl(c, n_indexed_rows, n_delta_rows, n_postings, n_distinct_keys, n_builds));
}

TVZ_EXPORT int tvz_corpus_tol_index(tvz_corpus *c, double cell) {
    TVZ_GUARDED(tvz_corpus_tol_index_impl(c, cell));
}

TVZ_EXPORT int tvz_corpus_tol_index_stats(tvz_corpus *c, double *cell, int64_t out[4]) {
    TVZ_GUARDED(tvz_corpus_tol_index_stats_impl(c, cell, out));
}

TVZ_EXPORT int tvz_corpus_upsert(tvz_corpus *c, int32_t video_id, const double *h_keys, int64_t n) {
    TVZ_GUARDED(tvz_corpus_upsert_impl(c, video_id, h_keys, n));
}

TVZ_EXPORT int tvz_corpus_clear(tvz_corpus *c) {
    TVZ_GUARDED(tvz_corpus_clear_impl(c));
}

TVZ_EXPORT int tvz_corpus_stats(tvz_corpus *c, int64_t *n_rows, int64_t *n_keys,
                                int64_t *arena_keys) {
    TVZ_GUARDED(tvz_corpus_stats_impl(c, n_rows, n_keys, arena_keys));
}

TVZ_EXPORT int tvz_match(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
                         int32_t Q, int32_t max_query_len, int32_t min_match,
                         const int32_t *d_exclude_ids, int32_t cap, int32_t *d_hits,
                         int32_t *d_hits_n, void *d_workspace, size_t workspace_bytes, int32_t algo,
                         void *hip_stream) {
    TVZ_GUARDED(tvz_match_impl(c, d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids, cap, d_hits, d_hits_n, d_workspace, workspace_bytes, algo, hip_stream));
}

TVZ_EXPORT int tvz_match_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
                              int32_t Q, int32_t max_query_len, int32_t min_match,
                              const int32_t *d_exclude_ids, int32_t cap, int32_t k, int32_t *d_out,
                              void *d_workspace, size_t workspace_bytes, int32_t algo,
                              void *hip_stream) {
    TVZ_GUARDED(tvz_match_topk_impl(c, d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids, cap, k, d_out, d_workspace, workspace_bytes, algo, hip_stream));
}

TVZ_EXPORT int tvz_find_duplicates(tvz_corpus *c, const double *h_query, int64_t n,
                                   int32_t min_match, int32_t exclude_id, int64_t cap,
                                   int32_t *h_out_ids, int32_t *h_out_counts, int32_t *h_out_kth,
                                   int64_t *n_out) {
    TVZ_GUARDED(tvz_find_duplicates_impl(c, h_query, n, min_match, exclude_id, cap, h_out_ids, h_out_counts, h_out_kth, n_out));
}

TVZ_EXPORT int tvz_topk(const int32_t *d_lists, const int32_t *d_lists_n, int32_t n_lists,
                        int32_t Q, int32_t cap, int32_t k, int32_t *d_topk, void *hip_stream) {
    TVZ_GUARDED(tvz_topk_impl(d_lists, d_lists_n, n_lists, Q, cap, k, d_topk, hip_stream));
}

TVZ_EXPORT int tvz_topk_shard(const int32_t *d_hits, const int32_t *d_hits_n, int32_t Q,
                              int32_t cap, int32_t k, int32_t *d_out, void *hip_stream) {
    TVZ_GUARDED(tvz_topk_shard_impl(d_hits, d_hits_n, Q, cap, k, d_out, hip_stream));
}

TVZ_EXPORT int tvz_match_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                     const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, int32_t min_match,
                                     const int32_t *d_exclude_ids, int32_t cap, int32_t k, int32_t *d_blocks,
                                     int32_t *d_topk, int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                                     int32_t algo, void *hip_stream) {
    TVZ_GUARDED(tvz_match_topk_shards_impl(shards, n_shards, d_queries, d_q_offsets, Q, max_query_len, min_match,
                                           d_exclude_ids, cap, k, d_blocks, d_topk, d_totals, d_workspace,
                                           workspace_bytes, algo, hip_stream));
}

TVZ_EXPORT int tvz_topk_merge(const int32_t *d_gathered, int32_t n_ranks, int32_t Q, int32_t k,
                              int32_t *d_topk, int32_t *d_totals, void *hip_stream) {
    TVZ_GUARDED(tvz_topk_merge_impl(d_gathered, n_ranks, Q, k, d_topk, d_totals, hip_stream));
}

TVZ_EXPORT int tvz_align(tvz_corpus *c, const double *d_query, int32_t n, double eps,
                         double max_offset, int32_t *d_out, int64_t out_rows, int64_t *n_rows,
                         void *hip_stream) {
    TVZ_GUARDED(tvz_align_impl(c, d_query, n, eps, max_offset, d_out, out_rows, n_rows, hip_stream));
}

// The alignment top-k's exports: each names its form (kAlignForms) and hands its arguments on.

TVZ_EXPORT size_t tvz_align_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k) {
    return align_sizing(kAlignBounded, Q, max_query_len, total_query_keys, k, 0);
}

TVZ_EXPORT size_t tvz_align_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                         int32_t k, int32_t n_ranks) {
    return n_ranks < 0 ? 0 : align_sizing(kAlignBounded, Q, max_query_len, total_query_keys, k, std::max(n_ranks, 1));
}

TVZ_EXPORT int tvz_align_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                              int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                              int32_t min_score, const int32_t *d_exclude_ids, int32_t k, int32_t *d_out,
                              void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_call(kAlignBounded, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                AlignAsk{{eps, max_offset, min_votes, min_score}, nullptr, 0, 0u, k}, d_out,
                                Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT size_t tvz_align_wide_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k) {
    return align_sizing(kAlignWide, Q, max_query_len, total_query_keys, k, 0);
}

TVZ_EXPORT int tvz_align_wide_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                   int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                                   int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                   int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_call(kAlignWide, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                AlignAsk{{eps, max_offset, min_votes, min_score}, nullptr, 0, flags, k}, d_out,
                                Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT int tvz_align_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k,
                                    const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk,
                                    int32_t *d_totals, void *hip_stream) {
    TVZ_GUARDED(tvz_align_merge_local(kAlignBounded, d_gathered, n_lists, Q, k, 0u, d_queries, d_q_offsets, d_topk, d_totals,
                                      hip_stream));
}

TVZ_EXPORT int tvz_align_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                     const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                     double max_offset, int32_t min_votes, int32_t min_score,
                                     const int32_t *d_exclude_ids, int32_t k, int32_t *d_blocks, int32_t *d_topk,
                                     int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_shards_impl(kAlignBounded, shards, n_shards,
                                  align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  AlignAsk{{eps, max_offset, min_votes, min_score}, nullptr, 0, 0u, k}, d_blocks, d_topk,
                                  d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_align_wide_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                                         const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk,
                                         int32_t *d_totals, void *hip_stream) {
    TVZ_GUARDED(tvz_align_merge_local(kAlignWide, d_gathered, n_lists, Q, k, flags, d_queries, d_q_offsets, d_topk, d_totals,
                                      hip_stream));
}

TVZ_EXPORT int tvz_align_wide_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                          const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                          double max_offset, int32_t min_votes, int32_t min_score, uint32_t flags,
                                          const int32_t *d_exclude_ids, int32_t k, int32_t *d_blocks, int32_t *d_topk,
                                          int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_shards_impl(kAlignWide, shards, n_shards,
                                  align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  AlignAsk{{eps, max_offset, min_votes, min_score}, nullptr, 0, flags, k}, d_blocks, d_topk,
                                  d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_rates_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k) {
    return align_sizing(kAlignRates, Q, max_query_len, total_query_keys, k, 0);
}

TVZ_EXPORT int tvz_align_rates_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                    int32_t max_query_len, double eps, double max_offset, const double *h_rates,
                                    int32_t n_rates, int32_t min_votes, int32_t min_score, uint32_t flags,
                                    const int32_t *d_exclude_ids, int32_t k, int32_t *d_out, void *d_workspace,
                                    size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_call(kAlignRates, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                AlignAsk{{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k}, d_out,
                                Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT int tvz_align_rates_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                                          const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk,
                                          int32_t *d_totals, void *hip_stream) {
    TVZ_GUARDED(tvz_align_merge_local(kAlignRates, d_gathered, n_lists, Q, k, flags, d_queries, d_q_offsets, d_topk, d_totals,
                                      hip_stream));
}

TVZ_EXPORT int tvz_align_rates_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                           const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                           double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                           int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                           int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                           size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_shards_impl(kAlignRates, shards, n_shards,
                                  align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  AlignAsk{{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k}, d_blocks,
                                  d_topk, d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_span_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k) {
    return align_sizing(kAlignSpan, Q, max_query_len, total_query_keys, k, 0);
}

TVZ_EXPORT int tvz_align_span_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                   int32_t max_query_len, double eps, double max_offset, const double *h_rates,
                                   int32_t n_rates, int32_t min_votes, int32_t min_score, uint32_t flags,
                                   const int32_t *d_exclude_ids, int32_t k, int32_t *d_out, void *d_workspace,
                                   size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_call(kAlignSpan, c, align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                AlignAsk{{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k}, d_out,
                                Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT int tvz_align_span_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                                         const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk,
                                         int32_t *d_totals, void *hip_stream) {
    TVZ_GUARDED(tvz_align_merge_local(kAlignSpan, d_gathered, n_lists, Q, k, flags, d_queries, d_q_offsets, d_topk, d_totals,
                                      hip_stream));
}

TVZ_EXPORT int tvz_align_span_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                          const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                          double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                          int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                          int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                          size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_shards_impl(kAlignSpan, shards, n_shards,
                                  align_batch(d_queries, d_q_offsets, Q, max_query_len, d_exclude_ids),
                                  AlignAsk{{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k}, d_blocks,
                                  d_topk, d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_parts_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                                  int32_t max_parts) {
    return align_parts_sizing(Q, max_query_len, total_query_keys, k, max_parts, 0);
}

TVZ_EXPORT int tvz_align_parts(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                               int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride,
                               int32_t k, double eps, double max_offset, const double *h_rates, int32_t n_rates,
                               int32_t min_votes, int32_t max_parts, int32_t *d_parts, void *d_workspace,
                               size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_parts_call(c, align_batch(d_queries, d_q_offsets, Q, max_query_len, nullptr),
                                 AlignPartsCall{d_video_ids, id_stride, query_id_stride, k, eps, max_offset, h_rates, n_rates,
                                                min_votes, max_parts},
                                 d_parts, Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT int tvz_align_parts_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, int32_t max_parts,
                                     int32_t *d_parts, void *hip_stream) {
    TVZ_GUARDED(tvz_align_parts_merge_local(d_gathered, n_lists, Q, k, max_parts, d_parts, hip_stream));
}

TVZ_EXPORT int tvz_align_parts_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                      const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                      const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride, int32_t k,
                                      double eps, double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                      int32_t max_parts, int32_t *d_blocks, int32_t *d_parts, void *d_workspace,
                                      size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_parts_shards_impl(shards, n_shards, align_batch(d_queries, d_q_offsets, Q, max_query_len, nullptr),
                                        AlignPartsCall{d_video_ids, id_stride, query_id_stride, k, eps, max_offset, h_rates,
                                                       n_rates, min_votes, max_parts},
                                        d_blocks, d_parts, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

// include/tvz_parts_flags.h: the two calls above with `flags` behind max_parts (0: the same walk; TVZ_ALIGN_TWO_BINS)
TVZ_EXPORT int tvz_align_parts_flags(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                     int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride,
                                     int64_t query_id_stride, int32_t k, double eps, double max_offset, const double *h_rates,
                                     int32_t n_rates, int32_t min_votes, int32_t max_parts, uint32_t flags, int32_t *d_parts,
                                     void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_parts_call(c, align_batch(d_queries, d_q_offsets, Q, max_query_len, nullptr),
                                 AlignPartsCall{d_video_ids, id_stride, query_id_stride, k, eps, max_offset, h_rates, n_rates,
                                                min_votes, max_parts, flags},
                                 d_parts, Workspace{d_workspace, workspace_bytes}, 0, hip_stream, nullptr));
}

TVZ_EXPORT int tvz_align_parts_flags_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                            const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                            const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride, int32_t k,
                                            double eps, double max_offset, const double *h_rates, int32_t n_rates,
                                            int32_t min_votes, int32_t max_parts, uint32_t flags, int32_t *d_blocks,
                                            int32_t *d_parts, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_parts_shards_impl(shards, n_shards, align_batch(d_queries, d_q_offsets, Q, max_query_len, nullptr),
                                        AlignPartsCall{d_video_ids, id_stride, query_id_stride, k, eps, max_offset, h_rates,
                                                       n_rates, min_votes, max_parts, flags},
                                        d_blocks, d_parts, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT size_t tvz_align_parts_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                                          int32_t max_parts, int32_t n_ranks) {
    return n_ranks < 0 ? 0 : align_parts_sizing(Q, max_query_len, total_query_keys, k, max_parts, std::max(n_ranks, 1));
}

TVZ_EXPORT size_t tvz_align_rates_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                               int32_t k, int32_t n_ranks) {
    return n_ranks < 0 ? 0 : align_sizing(kAlignRates, Q, max_query_len, total_query_keys, k, std::max(n_ranks, 1));
}

TVZ_EXPORT size_t tvz_align_span_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                              int32_t k, int32_t n_ranks) {
    return n_ranks < 0 ? 0 : align_sizing(kAlignSpan, Q, max_query_len, total_query_keys, k, std::max(n_ranks, 1));
}

// (unlike its bounded twin this one sizes n_ranks < 0 as one rank instead of answering 0: callers' buffers were sized by
// it, so the difference is kept on purpose)
TVZ_EXPORT size_t tvz_align_wide_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                              int32_t k, int32_t n_ranks) {
    return align_sizing(kAlignWide, Q, max_query_len, total_query_keys, k, std::max(n_ranks, 1));
}

TVZ_EXPORT int tvz_find_duplicates_tol(tvz_corpus *c, const double *h_query, int64_t n, double tol, int32_t min_match,
                                       int32_t exclude_id, int64_t cap, int32_t *h_out_ids, int32_t *h_out_counts,
                                       int32_t *h_out_kth, int64_t *n_out) {
    TVZ_GUARDED(tvz_find_duplicates_tol_impl(c, h_query, n, tol, min_match, exclude_id, cap, h_out_ids, h_out_counts,
                                             h_out_kth, n_out));
}

TVZ_EXPORT size_t tvz_match_tol_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys) {
    if (Q < 0 || max_query_len < 0 || total_query_keys < 0) return 0;
    const int64_t keys = total_query_keys > 0 ? total_query_keys : (int64_t)Q * max_query_len;
    return tol_ws_bytes(Q, keys);
}

TVZ_EXPORT int tvz_match_tol(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                             int32_t max_query_len, double tol, int32_t min_match, const int32_t *d_exclude_ids,
                             int32_t cap, int32_t *d_hits, int32_t *d_hits_n, void *d_workspace, size_t workspace_bytes,
                             void *hip_stream) {
    TVZ_GUARDED(tvz_match_tol_impl(c, d_queries, d_q_offsets, Q, max_query_len, tol, min_match, d_exclude_ids, cap,
                                   d_hits, d_hits_n, d_workspace, workspace_bytes, hip_stream));
}

TVZ_EXPORT size_t tvz_match_tol_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                     int32_t k, int32_t n_ranks) {
    if (Q < 0 || max_query_len < 0 || total_query_keys < 0 || k < 1 || n_ranks < 0) return 0;
    Carver cv(nullptr);
    tol_topk_ws_layout(cv, Q, k, n_ranks);
    return cv.fixed() + tvz_match_tol_workspace_bytes(Q, max_query_len, total_query_keys);
}

TVZ_EXPORT int tvz_match_tol_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                                  int32_t max_query_len, double tol, int32_t min_match, const int32_t *d_exclude_ids,
                                  int32_t k, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                                  void *hip_stream) {
    TVZ_GUARDED(tvz_match_tol_topk_impl(c, d_queries, d_q_offsets, Q, max_query_len, tol, min_match, d_exclude_ids, k,
                                        d_out, d_workspace, workspace_bytes, hip_stream));
}
