// tvz_common.h — shared host-side helpers for libtvz.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>

#include "tvz.h"

#define TVZ_EXPORT extern "C" __attribute__((visibility("default")))

// Diagnostic builds (profiles/variant_build.sh: s_memtime stamps, made-up postings - which return WRONG results
// on purpose) are quarantined: any of these defines makes tvz_version() return the
// NEGATED version, which every binding refuses (tvidz_amd/_lib.py loads such a library only with
// TVZ_ALLOW_DIAGNOSTIC=1, the profile scripts' own environment).
#if defined(TVZ_IX_FAKEPOST) || defined(TVZ_IX_STAMP) || defined(TVZ_DIAGNOSTIC)
#define TVZ_DIAGNOSTIC_BUILD 1
#else
#define TVZ_DIAGNOSTIC_BUILD 0
#endif

namespace tvz {

char *err_buf();  // thread-local, 512 bytes

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define TVZ_HIP(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return tvz::fail(TVZ_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                 \
                             hipGetErrorString(_e), __FILE__, __LINE__);                  \
    } while (0)

#define TVZ_REQUIRE(cond, ...)                                                            \
    do {                                                                                  \
        if (!(cond)) return tvz::fail(TVZ_ERR_INVALID, __VA_ARGS__);                      \
    } while (0)

// No C++ exception may cross the C ABI: allocation failures become TVZ_ERR_NOMEM.
#define TVZ_GUARDED(call)                                                                 \
    try {                                                                                 \
        return (call);                                                                    \
    } catch (const std::bad_alloc &) {                                                    \
        return tvz::fail(TVZ_ERR_NOMEM, "host allocation failed");                        \
    } catch (const std::exception &e) {                                                   \
        return tvz::fail(TVZ_ERR_INVALID, "unexpected C++ exception: %s", e.what());      \
    } catch (...) {                                                                       \
        return tvz::fail(TVZ_ERR_INVALID, "unexpected C++ exception");                    \
    }

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace tvz

// What the batched calls pass around between the C ABI and the launches: plain aggregates, no behaviour.
struct Batch {                       // the queries of one call
    const double *d_queries;
    const int64_t *d_q_offsets;
    int32_t Q, max_query_len, min_match;
    const int32_t *d_exclude_ids;
};
struct Workspace {                   // the caller's scratch
    void *p;
    size_t bytes;
};
struct AlignCall {                   // what an alignment top-k call asks of a (query, row) pair
    double eps, max_offset;
    int32_t min_votes, min_score;
};
struct ShardBlocks {                 // where a local top-k left its block, and the all-gather's target next to it
    int32_t *local = nullptr;        // int32[Q][k+1][3]: d_out, or the workspace's own area for d_out = NULL
    int32_t *gathered = nullptr;     // int32[n_ranks][Q][k+1][3] in the workspace  (rows of the form's width for the
                                     // alignment top-k; [n_ranks][Q][k][1 + max_parts][6] for the parts call)
};

// Internal (not exported): local sweep + per-shard top-k with the hit lists in the workspace (tvz_match.hip);
// `blocks` (may be NULL) is told where the block went.
int tvz_match_topk_local(tvz_corpus *c, const Batch &b, int32_t cap, int32_t k, int32_t *d_out, Workspace ws,
                         int32_t n_ranks, int32_t algo, void *hip_stream, ShardBlocks *blocks);
// The tolerant counterpart (tvz_match.hip): the sweep keeps the k best itself.
int tvz_match_tol_topk_local(tvz_corpus *c, const Batch &b, double tol, int32_t k, int32_t *d_out, Workspace ws,
                             int32_t n_ranks, void *hip_stream, ShardBlocks *blocks);
// The forms of the alignment top-k, in the order of tvz_match.hip's table kAlignForms, which says what each one is.
enum AlignForm { kAlignBounded, kAlignWide, kAlignRates, kAlignSpan, kAlignFormCount };
// What a sharded call still has to refuse once the local call has made all of its own refusals and before it enqueues
// anything: the communicator's (tvz_comm.hip).  fn = NULL: nothing.
struct LateCheck {
    int (*fn)(const void *ctx) = nullptr;
    const void *ctx = nullptr;
    int operator()() const { return fn ? fn(ctx) : TVZ_OK; }
};
// A form's call (tvz_match.hip): n_ranks = 0 is the call of the C ABI, whose workspace holds no blocks; n_ranks >= 1 is
// the workspace of the form's sharded sizing function.  `flags`: 0 for the form that has none; `h_rates`, `n_rates`:
// NULL, 0 for the forms without a rate list.
int tvz_align_topk_local(AlignForm form, tvz_corpus *c, const Batch &b, const AlignCall &a, const double *h_rates,
                         int32_t n_rates, uint32_t flags, int32_t k, int32_t *d_out, Workspace ws, int32_t n_ranks,
                         void *hip_stream, ShardBlocks *blocks, LateCheck late = {});
// ... the int32 columns of a row of its block ...
int tvz_align_form_cols(AlignForm form);
// ... and the merge of its gathered blocks.
int tvz_align_merge_local(AlignForm form, const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                          const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals,
                          void *hip_stream);
// tvz_align_parts with the sharded form's blocks in its workspace (n_ranks >= 1, d_parts = NULL: the answer goes into
// the workspace's own block), and the merge of the gathered answers (tvz_match.hip).
struct AlignPartsCall {
    const int32_t *d_video_ids;
    int64_t id_stride, query_id_stride;
    int32_t k;
    double eps, max_offset;
    const double *h_rates;
    int32_t n_rates, min_votes, max_parts;
    uint32_t flags = 0;              // tvz_align_parts_flags: 0 or TVZ_ALIGN_TWO_BINS; the calls without flags leave it 0
};
int tvz_align_parts_local(tvz_corpus *c, const Batch &b, const AlignPartsCall &p, int32_t *d_parts, Workspace ws, int32_t n_ranks,
                          void *hip_stream, ShardBlocks *blocks, LateCheck late = {});
int tvz_align_parts_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, int32_t max_parts,
                                int32_t *d_parts, void *hip_stream);
// tvz_align_candidates with the sharded form's blocks in front of its workspace (the answer goes into the workspace's
// own block: `blocks` is told where), and the merge of the gathered blocks (tvz_match.hip).
int tvz_align_candidates_local(tvz_corpus *c, const Batch &b, int32_t min_count, int32_t cap, int32_t C, Workspace ws,
                               int32_t n_ranks, void *hip_stream, ShardBlocks *blocks, LateCheck late = {});
int tvz_align_candidates_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                     void *hip_stream);
// The same two for tvz_align_candidates_rates (blocks of rows of 3; include/tvz_gap_rates_shards.h).
int tvz_align_candidates_rates_local(tvz_corpus *c, const Batch &b, const double *h_rates, int32_t n_rates, int32_t min_count,
                                     int32_t cap, int32_t C, Workspace ws, int32_t n_ranks, void *hip_stream, ShardBlocks *blocks,
                                     LateCheck late = {});
int tvz_align_candidates_rates_merge_local(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                           void *hip_stream);
