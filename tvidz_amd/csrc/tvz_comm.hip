// tvz_comm.hip — the multi-GPU exchange step of the corpus match behind the C ABI.
//
// One process per GPU; the corpus rows are sharded over the ranks, queries are replicated.  Per
// query batch every rank runs its local sweep + per-shard top-k (tvz_match.hip), ONE ncclAllGather
// moves the [Q][k+1][3] int32 blocks (k best hits + a totals row: <= 204 B per query and rank at
// k = 16, latency-bound on xGMI), and every rank runs the identical merge.  The reference has no
// counterpart: it scans one Postgres table in one Python process (inspector/db.py:83-91).
//
// RCCL is bound at run time with dlopen/dlsym - the copy the process has already mapped (e.g.
// PyTorch's) if there is one - so libtvz.so has no link-time dependency on it and a host language
// other than Python gets the whole multi-GPU path from this library alone.
#include <dlfcn.h>

#include <algorithm>
#include <mutex>

#include "tvz_common.h"
#include "tvz_gap_shards.h"
#include "tvz_gap_rates_shards.h"

namespace {

// ABI of the few RCCL entry points used (rccl.h: ncclUniqueId is 128 opaque bytes passed by value,
// ncclInt32 = 2, ncclSuccess = 0)
struct NcclId { char internal[TVZ_UNIQUE_ID_BYTES]; };
using NcclComm = void *;
constexpr int kNcclInt32 = 2;

struct Api {
    void *lib = nullptr;
    int (*GetUniqueId)(NcclId *) = nullptr;
    int (*CommInitRank)(NcclComm *, int, NcclId, int) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, NcclComm, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};

Api g_api;                 // written once under g_api_mu, read-only afterwards
std::once_flag g_api_once;

void load_api() {
    const char *names[] = {"librccl.so", "librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names)                       // a copy the process already mapped
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    const char *paths[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : paths)
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    g_api.lib = h;
    g_api.GetUniqueId = reinterpret_cast<decltype(g_api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_api.CommInitRank = reinterpret_cast<decltype(g_api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_api.CommDestroy = reinterpret_cast<decltype(g_api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_api.AllGather = reinterpret_cast<decltype(g_api.AllGather)>(dlsym(h, "ncclAllGather"));
    g_api.GetErrorString = reinterpret_cast<decltype(g_api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    g_api.ok = g_api.GetUniqueId && g_api.CommInitRank && g_api.CommDestroy && g_api.AllGather;
}

int need_api() {
    std::call_once(g_api_once, load_api);
    if (!g_api.ok)
        return tvz::fail(TVZ_ERR_COMM, "RCCL is not available (dlopen of librccl.so failed: %s)",
                         g_api.lib ? "symbols missing" : "library not found");
    return TVZ_OK;
}

int nccl_fail(const char *what, int rc) {
    return tvz::fail(TVZ_ERR_COMM, "%s failed: %s (%d)", what,
                     g_api.GetErrorString ? g_api.GetErrorString(rc) : "?", rc);
}

}  // namespace

struct tvz_comm {
    NcclComm comm = nullptr;
    int32_t n_ranks = 0, rank = 0, device = 0;
    // The collectives of ONE communicator are issued from whichever stream the caller passes (two
    // alternating streams in sharded.RcclShardedMatcher).  Their order is made explicit: a collective
    // on a stream other than the previous one's waits for an event recorded behind the previous one,
    // so the communicator never has two collectives in flight whatever RCCL does about stream changes.
    std::mutex mu;
    hipStream_t last_stream = nullptr;
    bool any = false;
    hipEvent_t last_ev = nullptr;       // created on first use
};

static int tvz_comm_unique_id_impl(void *out_id) {
    TVZ_REQUIRE(out_id != nullptr, "out_id is NULL");
    if (int rc = need_api()) return rc;
    NcclId id;
    if (int rc = g_api.GetUniqueId(&id)) return nccl_fail("ncclGetUniqueId", rc);
    memcpy(out_id, id.internal, TVZ_UNIQUE_ID_BYTES);
    return TVZ_OK;
}

static int tvz_comm_init_impl(tvz_comm **out, const void *unique_id, int32_t n_ranks, int32_t rank,
                              int32_t device) {
    TVZ_REQUIRE(out != nullptr && unique_id != nullptr, "NULL argument");
    TVZ_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank %d of %d", rank, n_ranks);
    if (int rc = need_api()) return rc;
    int n = 0;
    TVZ_HIP(hipGetDeviceCount(&n));
    TVZ_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
    int prev = -1;
    (void)hipGetDevice(&prev);
    TVZ_HIP(hipSetDevice(device));                  // RCCL binds the communicator to the current device
    NcclId id;
    memcpy(id.internal, unique_id, TVZ_UNIQUE_ID_BYTES);
    tvz_comm *c = new tvz_comm();
    c->n_ranks = n_ranks;
    c->rank = rank;
    c->device = device;
    const int rc = g_api.CommInitRank(&c->comm, n_ranks, id, rank);
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    if (rc) {
        delete c;
        return nccl_fail("ncclCommInitRank", rc);
    }
    *out = c;
    return TVZ_OK;
}

static int tvz_comm_destroy_impl(tvz_comm *comm) {
    if (!comm) return TVZ_OK;
    if (comm->comm && g_api.ok) (void)g_api.CommDestroy(comm->comm);
    if (comm->last_ev) (void)hipEventDestroy(comm->last_ev);
    delete comm;
    return TVZ_OK;
}

// The exchange behind a local per-shard top-k: ONE ncclAllGather of the ranks' blocks of `count` int32 (Q x (k+1) rows
// of 3, of the form's 4, 5 or 8 for the alignment top-k; Q x k answers for the parts call) on `hip_stream`, ordered behind the communicator's previous collective, then
// `merge`, which every rank runs alike on the gathered blocks.
template <typename Merge>
static int gather_and_merge(tvz_comm *comm, const int32_t *local, int32_t *gathered, size_t count, void *hip_stream,
                            Merge &&merge) {
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    // RCCL enqueues on the communicator's device: make it current for the call (a host that drives
    // several GPUs from one thread may have another one selected)
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != comm->device) TVZ_HIP(hipSetDevice(comm->device));
    int grc = 0;
    hipError_t herr = hipSuccess;
    {
        std::lock_guard<std::mutex> lk(comm->mu);
        if (!comm->last_ev) herr = hipEventCreateWithFlags(&comm->last_ev, hipEventDisableTiming);
        if (herr == hipSuccess && comm->any && comm->last_stream != st) herr = hipStreamWaitEvent(st, comm->last_ev, 0);
        if (herr == hipSuccess) {
            grc = g_api.AllGather(local, gathered, count, kNcclInt32, comm->comm, st);
            if (!grc) herr = hipEventRecord(comm->last_ev, st);
            comm->last_stream = st;
            comm->any = true;
        }
    }
    // the merge is launched like the collective, with the communicator's device current
    const int mrc = herr == hipSuccess && !grc ? merge() : TVZ_OK;
    if (prev >= 0 && prev != comm->device) (void)hipSetDevice(prev);
    if (herr != hipSuccess) return tvz::fail(TVZ_ERR_HIP, "ordering the collective failed: %s", hipGetErrorString(herr));
    if (grc) return nccl_fail("ncclAllGather", grc);
    return mrc;
}

// the merge of the exact and the tolerant match: blocks of rows of 3
static int gather_and_merge_topk(tvz_comm *comm, const ShardBlocks &blk, int32_t Q, int32_t k, int32_t *d_topk,
                                 int32_t *d_totals, void *hip_stream) {
    return gather_and_merge(comm, blk.local, blk.gathered, (size_t)Q * (size_t)(k + 1) * 3, hip_stream, [&] {
        return tvz_topk_merge(blk.gathered, comm->n_ranks, Q, k, d_topk, d_totals, hip_stream);
    });
}

static int tvz_match_sharded_impl(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                  const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                  int32_t min_match, const int32_t *d_exclude_ids, int32_t cap,
                                  int32_t k, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                  size_t workspace_bytes, int32_t algo, void *hip_stream) {
    TVZ_REQUIRE(comm != nullptr && comm->comm != nullptr, "communicator is NULL");
    TVZ_REQUIRE(Q == 0 || d_topk != nullptr, "d_topk is NULL");
    if (Q == 0) return TVZ_OK;
    ShardBlocks blk;
    // local sweep + per-shard top-k into the workspace's own block
    if (int rc = tvz_match_topk_local(c, Batch{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids}, cap, k,
                                      nullptr, Workspace{d_workspace, workspace_bytes}, comm->n_ranks, algo, hip_stream,
                                      &blk))
        return rc;
    return gather_and_merge_topk(comm, blk, Q, k, d_topk, d_totals, hip_stream);
}

static int tvz_match_tol_sharded_impl(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                      const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double tol,
                                      int32_t min_match, const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk,
                                      int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                                      void *hip_stream) {
    TVZ_REQUIRE(comm != nullptr && comm->comm != nullptr, "communicator is NULL");
    TVZ_REQUIRE(Q <= 0 || d_topk != nullptr, "d_topk is NULL");
    ShardBlocks blk;
    // the tolerant sweep keeps its k best itself and writes them into the workspace's own block
    if (int rc = tvz_match_tol_topk_local(c, Batch{d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids}, tol,
                                          k, nullptr, Workspace{d_workspace, workspace_bytes}, comm->n_ranks, hip_stream,
                                          &blk))
        return rc;
    if (Q == 0) return TVZ_OK;
    return gather_and_merge_topk(comm, blk, Q, k, d_topk, d_totals, hip_stream);
}

// What the sharded alignment calls refuse of their communicator and of the merge's outputs.
struct AlignCommCheck {
    const tvz_comm *comm;
    int32_t Q;
    const int32_t *d_rows, *d_totals;    // the merge's outputs (d_totals: NULL for the parts call, which has none)
    bool with_totals, aligned16;
};
static int check_align_comm(const void *ctx) {
    const AlignCommCheck &s = *static_cast<const AlignCommCheck *>(ctx);
    TVZ_REQUIRE(s.comm != nullptr && s.comm->comm != nullptr, "communicator is NULL");
    if (s.with_totals)
        TVZ_REQUIRE(s.Q <= 0 || (s.d_rows != nullptr && s.d_totals != nullptr), "d_topk or d_totals is NULL");
    else
        TVZ_REQUIRE(s.Q <= 0 || s.d_rows != nullptr, "d_parts is NULL");
    TVZ_REQUIRE(!s.aligned16 || (reinterpret_cast<uintptr_t>(s.d_rows) & 15) == 0, "d_topk must be 16-byte aligned");
    if (s.comm->n_ranks > 16)        // (the merge's limit: refused before the local call enqueues anything)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "alignment top-k: %d ranks, the merge takes up to 16", (int)s.comm->n_ranks);
    return TVZ_OK;
}

// The alignment top-k's RCCL forms (tvz_<stem>_sharded of every entry of kAlignForms): the local sweep keeps its k best
// itself and writes them into the workspace's own block, then the gather of Q x (k + 1) rows of the form's width and the
// form's merge.  `comm_first`: the bounded and the wide form refuse their communicator before anything else; the forms
// with rates make the unsharded call's refusals first, in its order and words, and the communicator's behind them -
// either way before anything is enqueued.
static int align_topk_sharded_impl(AlignForm form, bool comm_first, tvz_corpus *c, tvz_comm *comm, const Batch &b,
                                   const AlignCall &a, const double *h_rates, int32_t n_rates, uint32_t flags, int32_t k,
                                   int32_t *d_topk, int32_t *d_totals, Workspace ws, void *hip_stream) {
    const int32_t Q = b.Q;
    const AlignCommCheck chk{comm, Q, d_topk, d_totals, true, true};
    if (comm_first)
        if (int rc = check_align_comm(&chk)) return rc;
    // (a NULL communicator is sized as one rank until it is refused)
    const int32_t n_ranks = comm ? std::max<int32_t>(comm->n_ranks, 1) : 1;
    ShardBlocks blk;
    if (int rc = tvz_align_topk_local(form, c, b, a, h_rates, n_rates, flags, k, nullptr, ws, n_ranks, hip_stream, &blk,
                                      LateCheck{check_align_comm, &chk}))
        return rc;
    if (int rc = check_align_comm(&chk)) return rc;          // (Q = 0: the local call returned in front of its late checks)
    if (Q == 0) return TVZ_OK;
    const size_t cols = (size_t)tvz_align_form_cols(form);
    return gather_and_merge(comm, blk.local, blk.gathered, (size_t)Q * (size_t)(k + 1) * cols, hip_stream, [&] {
        return tvz_align_merge_local(form, blk.gathered, comm->n_ranks, Q, k, flags, b.d_queries, b.d_q_offsets, d_topk,
                                     d_totals, hip_stream);
    });
}

// tvz_align_parts_sharded: the local call into the workspace's own block, ONE all-gather of Q x k x (1 + max_parts) x 6
// int32, the merge.  The call's own refusals come first, the communicator's behind them.
static int align_parts_sharded_impl(tvz_corpus *c, tvz_comm *comm, const Batch &b, const AlignPartsCall &p, int32_t *d_parts,
                                    Workspace ws, void *hip_stream) {
    const int32_t Q = b.Q;
    const AlignCommCheck chk{comm, Q, d_parts, nullptr, false, false};
    const int32_t n_ranks = comm ? std::max<int32_t>(comm->n_ranks, 1) : 1;
    ShardBlocks blk;
    if (int rc = tvz_align_parts_local(c, b, p, nullptr, ws, n_ranks, hip_stream, &blk, LateCheck{check_align_comm, &chk}))
        return rc;
    if (int rc = check_align_comm(&chk)) return rc;
    if (Q == 0) return TVZ_OK;
    const size_t count = (size_t)Q * (size_t)p.k * (size_t)(1 + p.max_parts) * 6;
    return gather_and_merge(comm, blk.local, blk.gathered, count, hip_stream, [&] {
        return tvz_align_parts_merge_local(blk.gathered, comm->n_ranks, Q, p.k, p.max_parts, d_parts, hip_stream);
    });
}

// tvz_align_candidates_sharded (include/tvz_gap_shards.h): the local call into the workspace's own block, ONE all-gather
// of Q x (C + 1) x 2 int32, the merge.  The call's own refusals come first, the communicator's behind them.
struct CandidatesCommCheck {
    const tvz_comm *comm;
    int32_t Q;
    const int32_t *d_out;
    int out_align = 8;                              // bytes of a row's vector store: 8, the rates form 4
    const char *what = "alignment candidates";      // the call in the message
};
static int check_candidates_comm(const void *ctx) {
    const CandidatesCommCheck &s = *static_cast<const CandidatesCommCheck *>(ctx);
    TVZ_REQUIRE(s.comm != nullptr && s.comm->comm != nullptr, "communicator is NULL");
    TVZ_REQUIRE(s.Q <= 0 || (s.d_out != nullptr && (reinterpret_cast<uintptr_t>(s.d_out) & (uintptr_t)(s.out_align - 1)) == 0),
                "d_out is NULL or not %d-byte aligned", s.out_align);
    if (s.comm->n_ranks > 16)        // (the merge's limit: refused before the local call enqueues anything)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%s: %d ranks, the merge takes up to 16", s.what, (int)s.comm->n_ranks);
    return TVZ_OK;
}

static int align_candidates_sharded_impl(tvz_corpus *c, tvz_comm *comm, const Batch &b, int32_t min_count, int32_t cap,
                                         int32_t C, int32_t *d_out, Workspace ws, void *hip_stream) {
    const int32_t Q = b.Q;
    const CandidatesCommCheck chk{comm, Q, d_out};
    // (a NULL communicator is sized as one rank until it is refused)
    const int32_t n_ranks = comm ? std::max<int32_t>(comm->n_ranks, 1) : 1;
    ShardBlocks blk;
    if (int rc = tvz_align_candidates_local(c, b, min_count, cap, C, ws, n_ranks, hip_stream, &blk,
                                            LateCheck{check_candidates_comm, &chk}))
        return rc;
    if (int rc = check_candidates_comm(&chk)) return rc;     // (Q = 0: the local call returned in front of its late checks)
    if (Q == 0) return TVZ_OK;
    return gather_and_merge(comm, blk.local, blk.gathered, (size_t)Q * (size_t)(C + 1) * 2, hip_stream, [&] {
        return tvz_align_candidates_merge_local(blk.gathered, comm->n_ranks, Q, C, d_out, hip_stream);
    });
}

TVZ_EXPORT int tvz_align_candidates_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                            int32_t Q, int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids,
                                            int32_t cap, int32_t C, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                                            void *hip_stream) {
    TVZ_GUARDED(align_candidates_sharded_impl(c, comm, Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0,
                                                              d_exclude_ids},
                                              min_count, cap, C, d_out, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

// tvz_align_candidates_rates_sharded (include/tvz_gap_rates_shards.h): the same with the rates call and rows of 3 -
// ONE all-gather of Q x (C + 1) x 3 int32, the block-per-query merge.
static int align_candidates_rates_sharded_impl(tvz_corpus *c, tvz_comm *comm, const Batch &b, const double *h_rates,
                                               int32_t n_rates, int32_t min_count, int32_t cap, int32_t C, int32_t *d_out,
                                               Workspace ws, void *hip_stream) {
    const int32_t Q = b.Q;
    const CandidatesCommCheck chk{comm, Q, d_out, 4, "alignment candidates with rates"};
    // (a NULL communicator is sized as one rank until it is refused)
    const int32_t n_ranks = comm ? std::max<int32_t>(comm->n_ranks, 1) : 1;
    ShardBlocks blk;
    if (int rc = tvz_align_candidates_rates_local(c, b, h_rates, n_rates, min_count, cap, C, ws, n_ranks, hip_stream, &blk,
                                                  LateCheck{check_candidates_comm, &chk}))
        return rc;
    if (int rc = check_candidates_comm(&chk)) return rc;   // (Q = 0: the local call returned in front of its late checks)
    if (Q == 0) return TVZ_OK;
    return gather_and_merge(comm, blk.local, blk.gathered, (size_t)Q * (size_t)(C + 1) * 3, hip_stream, [&] {
        return tvz_align_candidates_rates_merge_local(blk.gathered, comm->n_ranks, Q, C, d_out, hip_stream);
    });
}

TVZ_EXPORT int tvz_align_candidates_rates_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                                  const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                                  const double *h_rates, int32_t n_rates, int32_t min_count,
                                                  const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_out,
                                                  void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_candidates_rates_sharded_impl(c, comm, Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0,
                                                                    d_exclude_ids},
                                                    h_rates, n_rates, min_count, cap, C, d_out,
                                                    Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_comm_unique_id(void *out_id) { TVZ_GUARDED(tvz_comm_unique_id_impl(out_id)); }

TVZ_EXPORT int tvz_comm_init(tvz_comm **out, const void *unique_id, int32_t n_ranks, int32_t rank,
                             int32_t device) {
    TVZ_GUARDED(tvz_comm_init_impl(out, unique_id, n_ranks, rank, device));
}

TVZ_EXPORT int tvz_comm_info(tvz_comm *comm, int32_t *n_ranks, int32_t *rank) {
    TVZ_REQUIRE(comm != nullptr, "communicator is NULL");
    if (n_ranks) *n_ranks = comm->n_ranks;
    if (rank) *rank = comm->rank;
    return TVZ_OK;
}

TVZ_EXPORT int tvz_comm_destroy(tvz_comm *comm) { TVZ_GUARDED(tvz_comm_destroy_impl(comm)); }

TVZ_EXPORT int tvz_match_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                 const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                                 int32_t min_match, const int32_t *d_exclude_ids, int32_t cap,
                                 int32_t k, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                 size_t workspace_bytes, int32_t algo, void *hip_stream) {
    TVZ_GUARDED(tvz_match_sharded_impl(c, comm, d_queries, d_q_offsets, Q, max_query_len, min_match, d_exclude_ids, cap, k, d_topk, d_totals, d_workspace, workspace_bytes, algo, hip_stream));
}

TVZ_EXPORT int tvz_match_tol_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                     const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double tol,
                                     int32_t min_match, const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk,
                                     int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(tvz_match_tol_sharded_impl(c, comm, d_queries, d_q_offsets, Q, max_query_len, tol, min_match, d_exclude_ids, k, d_topk, d_totals, d_workspace, workspace_bytes, hip_stream));
}

TVZ_EXPORT int tvz_align_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                      int32_t Q, int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                                      int32_t min_score, const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk,
                                      int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_sharded_impl(kAlignBounded, /* comm_first */ true, c, comm,
                                        Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, d_exclude_ids},
                                        AlignCall{eps, max_offset, min_votes, min_score}, nullptr, 0, 0u, k, d_topk, d_totals,
                                        Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_align_wide_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                           const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                           double max_offset, int32_t min_votes, int32_t min_score, uint32_t flags,
                                           const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk, int32_t *d_totals,
                                           void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_topk_sharded_impl(kAlignWide, /* comm_first */ true, c, comm,
                                        Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, d_exclude_ids},
                                        AlignCall{eps, max_offset, min_votes, min_score}, nullptr, 0, flags, k, d_topk, d_totals,
                                        Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_align_rates_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                            const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                            double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                            int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                            int32_t *d_topk, int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                                            void *hip_stream) {
    TVZ_GUARDED(align_topk_sharded_impl(kAlignRates, /* comm_first */ false, c, comm,
                                        Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, d_exclude_ids},
                                        AlignCall{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k, d_topk,
                                        d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_align_span_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                                           const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                           double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                           int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                           int32_t *d_topk, int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                                           void *hip_stream) {
    TVZ_GUARDED(align_topk_sharded_impl(kAlignSpan, /* comm_first */ false, c, comm,
                                        Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, d_exclude_ids},
                                        AlignCall{eps, max_offset, min_votes, min_score}, h_rates, n_rates, flags, k, d_topk,
                                        d_totals, Workspace{d_workspace, workspace_bytes}, hip_stream));
}

TVZ_EXPORT int tvz_align_parts_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                       int32_t Q, int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride,
                                       int64_t query_id_stride, int32_t k, double eps, double max_offset,
                                       const double *h_rates, int32_t n_rates, int32_t min_votes, int32_t max_parts,
                                       int32_t *d_parts, void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    TVZ_GUARDED(align_parts_sharded_impl(c, comm, Batch{d_queries, d_q_offsets, Q, max_query_len, /* min_match: none */ 0, nullptr},
                                         AlignPartsCall{d_video_ids, id_stride, query_id_stride, k, eps, max_offset, h_rates,
                                                        n_rates, min_votes, max_parts},
                                         d_parts, Workspace{d_workspace, workspace_bytes}, hip_stream));
}
