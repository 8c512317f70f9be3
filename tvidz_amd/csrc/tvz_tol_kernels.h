// tvz_tol_kernels.h — opt-in tolerant duplicate match (tvz_find_duplicates_tol / tvz_match_tol), gfx950 wave64.
// Included by tvz_match.hip only.  From tvz_match_kernels.h: Row, the kth modes and kth_of, HostOut and the block's
// hit sink, the fix-up walk; from tvz_index_kernels.h: ix_tk_pack; from tvz_wave.h: the group reductions.
//
// Contract (include/tvz.h): query element q[i] matches row r iff q[i] is not NaN and some key of r has
//   key == q[i]  or  fabs(q[i] - key) <= tol       (ONE IEEE double subtraction, rounded to nearest)
// count = matching elements (query multiplicity counts), kth = index of the min_match-th of them.
//
// Why a sorted search is exact: for a fixed key, fl(q - key) never decreases as q grows, so the query values
// that match one key form ONE contiguous run [lo, hi) of the numerically sorted query, and lo, hi never
// decrease as the key grows.  A row's count is the size of the union of its keys' runs.  The arena keeps a
// row's keys sorted by their int64 bit pattern: the p negative keys first in DECREASING numeric order, then
// +0.0 and the positive keys in increasing order.  Walking the arena order, key j's new elements are
//   negative key:  [lo_j, min(hi_j, lo_{j-1}))      (its numerically larger neighbour j-1 was seen first)
//   positive key:  [max(lo_j, hi_{j-1}), hi_j)      (the first positive key takes hi of arena key 0, the
//                                                    numerically largest negative one, as its hi_{j-1})
// so every union element is visited exactly once: the count is the sum of the new runs and the kth comes
// from the smallest original positions kept in registers per lane (min_match 1..5) or a fix-up pass.
//
// ts_tol_sort_kernel      batch query preparation: per query the non-NaN values sorted (rank sort over LDS
//                         tiles) with their original positions, into the caller's workspace.
// ts_match_tol_kernel     one sweep of the row table + key arena per query: a 16-lane group per row,
//                         unconditional 16-byte key loads, the next row entry fetched one row ahead; per key
//                         two searches of the sorted query (LDS table, or device memory for a long query).
// ts_tol_kth_fixup_kernel kth for min_match > 5: per hit, the query walked in its original order.
// ts_tol_topk_kernel      the sweep that keeps the k best hits of its block on chip (min_match 1..5) and
// ts_tol_topk_reduce_kernel  the per-query selection over the blocks' lists: tvz_match_tol_topk.
#pragma once
#include "tvz_index_kernels.h"
#include "tvz_match_kernels.h"
#include "tvz_wave.h"

namespace {

constexpr int kTolBlock = 256;
constexpr int kTolGroups = kTolBlock / kGroup;        // rows in flight per block
constexpr int kTolLd = 4;                              // 16-byte key loads per lane and step
constexpr int kTolStepKeys = kTolLd * 2 * kGroup;      // 128 keys of a row per step
// Sorted queries of up to this many values live in LDS (8 B value + 4 B position each: 96 KiB at the limit);
// a longer one is searched where the preparation left it, in device memory.  Same results either way.
constexpr int kTolLdsKeys = 8192;
constexpr int kTolSortBlock = 256;
constexpr int kTolSortTile = 2048;                     // query values per LDS tile of the rank sort

inline size_t tol_lds_bytes(int64_t keys) {
    const int64_t k = (keys + 1) & ~(int64_t)1;        // positions start 16-byte aligned
    return (size_t)k * 12;
}

// the contract's predicate, verbatim: no rewrite to q >= key - tol (that rounds differently)
__device__ __forceinline__ bool tol_match(double q, double k, double tol) {
    return q == k || fabs(q - k) <= tol;
}

// lo = #{t : s[t] < k and s[t] does not match k}: a prefix of the sorted query
__device__ __forceinline__ int tol_lo(const double *s, int m, double k, double tol) {
    int lo = 0, len = m;
    while (len > 0) {
        const int half = len >> 1;
        const double v = s[lo + half];
        if (v < k && !(fabs(v - k) <= tol)) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// hi = first t >= from with s[t] > k and s[t] not matching k (everything in [from, hi) matches).  Runs are
// short at the tolerances this is for: two linear probes, then a binary search of the rest.
__device__ __forceinline__ int tol_hi(const double *s, int m, int from, double k, double tol) {
    int t = from;
    for (int probe = 0; probe < 2; ++probe) {
        if (t >= m) return t;
        const double v = s[t];
        if (v > k && !(fabs(v - k) <= tol)) return t;
        ++t;
    }
    int len = m - t;
    while (len > 0) {
        const int half = len >> 1;
        const double v = s[t + half];
        if (v > k && !(fabs(v - k) <= tol)) {
            len = half;
        } else {
            t += half + 1;
            len -= half + 1;
        }
    }
    return t;
}

__device__ __forceinline__ void tol_insert5(uint32_t (&tk)[kTop], uint32_t v) {
#pragma unroll
    for (int t = 0; t < kTop; ++t) {
        const uint32_t lo = tk[t] < v ? tk[t] : v;
        v = tk[t] < v ? v : tk[t];
        tk[t] = lo;
    }
}

// One row against the sorted query s[0 .. m) (positions pos[..]): the 16 lanes of a group walk the row's keys
// rk[0 .. len), 128 per step.  Returns cnt summed over the group and, per lane, the smallest positions it met
// (m1, m2 or tk by MODE; tol_row_kth reduces them).  `keys` is any readable address for the lanes past the end.
template <int MODE>
__device__ __forceinline__ void tol_row_scan(const int64_t *__restrict__ keys, const int64_t *rk, int len, const double *s,
                                             const int32_t *pos, int m, double tol, int gl, uint32_t &cnt, uint32_t &m1,
                                             uint32_t &m2, uint32_t (&tk)[kTop]) {
    cnt = 0;
    m1 = m2 = 0xffffffffu;
#pragma unroll
    for (int t = 0; t < kTop; ++t) tk[t] = 0xffffffffu;
    auto acc_range = [&](int a, int b) {
        if (b <= a) return;
        cnt += (uint32_t)(b - a);
        if constexpr (MODE == kModeM2) {
            for (int t = a; t < b; ++t) {
                const uint32_t p = (uint32_t)pos[t];
                const uint32_t lo = m1 < p ? m1 : p, hi = m1 < p ? p : m1;
                m1 = lo;
                m2 = m2 < hi ? m2 : hi;
            }
        } else if constexpr (MODE == kModeTop5) {
            for (int t = a; t < b; ++t) tol_insert5(tk, (uint32_t)pos[t]);
        }
    };
    // packed union state a key hands to its arena successor: (neg ? lo : hi) | neg << 31
    uint32_t carry = 0;
    int64_t k0 = 0;                      // the row's first arena key (numerically largest negative, if any)
    int hi0 = -1;                        // its hi, computed by the lane that needs it
    for (int base = 0; base < len; base += kTolStepKeys) {
        longlong2 cur[kTolLd];
#pragma unroll
        for (int j = 0; j < kTolLd; ++j) {
            const int i = base + gl * 2 + j * 2 * kGroup;
            const int64_t *p = (i < len) ? rk + i : keys;                 // unconditional 16-byte loads
            cur[j] = *reinterpret_cast<const longlong2 *>(p);
        }
        if (base == 0) k0 = __shfl(cur[0].x, 0, kGroup);               // group-uniform step
#pragma unroll
        for (int j = 0; j < kTolLd; ++j) {
            const int i = base + gl * 2 + j * 2 * kGroup;
            const bool vx = i < len, vy = i + 1 < len;
            const int64_t bx_ = cur[j].x, by_ = cur[j].y;
            const bool nx = bx_ < 0, ny = by_ < 0;
            int lox = 0, hix = 0, loy = 0, hiy = 0;
            if (vx) {
                const double kx = __longlong_as_double(bx_);
                lox = tol_lo(s, m, kx, tol);
                hix = tol_hi(s, m, lox, kx, tol);
            }
            if (vy) {
                const double ky = __longlong_as_double(by_);
                loy = tol_lo(s, m, ky, tol);
                hiy = tol_hi(s, m, loy, ky, tol);
            }
            const uint32_t cy = (uint32_t)(ny ? loy : hiy) | (ny ? 0x80000000u : 0u);
            // arena predecessor of x: y of lane gl-1; for lane 0 the y of lane 15 one load earlier
            const uint32_t t = group16_prev(cy);
            const uint32_t px = gl == 0 ? carry : t;
            carry = t;
            auto first_pos_prev = [&]() -> int {                         // hi of arena key 0
                if (hi0 < 0) {
                    const double kk = __longlong_as_double(k0);
                    hi0 = tol_hi(s, m, tol_lo(s, m, kk, tol), kk, tol);
                }
                return hi0;
            };
            if (vx) {
                const bool none = i == 0;
                const bool pneg = (px >> 31) != 0;
                const int pv = (int)(px & 0x7fffffffu);
                if (nx) {
                    acc_range(lox, none ? hix : (hix < pv ? hix : pv));
                } else {
                    const int prev = none ? 0 : (pneg ? first_pos_prev() : pv);
                    acc_range(lox > prev ? lox : prev, hix);
                }
            }
            if (vy) {
                if (ny) {
                    acc_range(loy, hiy < lox ? hiy : lox);
                } else {
                    const int prev = nx ? first_pos_prev() : hix;
                    acc_range(loy > prev ? loy : prev, hiy);
                }
            }
        }
    }
    cnt = group16_sum(cnt);
}

// The butterfly behind tol_row_scan: every lane of the group leaves with the group's smallest positions.
template <int MODE>
__device__ __forceinline__ void tol_row_reduce(uint32_t &m1, uint32_t &m2, uint32_t (&tk)[kTop]) {
    if constexpr (MODE == kModeM2) {
        group16_min2(m1, m2);
    } else if constexpr (MODE == kModeTop5) {
        // each step merges two DISJOINT sets of positions (every union element is visited once)
#define TVZ_T5_STEP(C) { uint32_t o[kTop]; \
        _Pragma("unroll") for (int t = 0; t < kTop; ++t) o[t] = dpp16<C>(tk[t]); \
        _Pragma("unroll") for (int t = 0; t < kTop; ++t) tol_insert5(tk, o[t]); }
        TVZ_ROW16_BUTTERFLY(TVZ_T5_STEP)
#undef TVZ_T5_STEP
    }
}

// A sorted query: m values ascending and their positions in the query as it was given.
struct TolQuery {
    const double *s;
    const int32_t *pos;
};
// The sorted query at sv/sp[at ..) into dynamic LDS laid out for lds_keys values (tol_lds_bytes).  The caller's next
// block barrier publishes the copy.
__device__ __forceinline__ TolQuery tol_query_to_lds(unsigned char *smem, int32_t lds_keys, const double *sv,
                                                     const int32_t *sp, int64_t at, int32_t m) {
    double *lv = reinterpret_cast<double *>(smem);
    int32_t *lp = reinterpret_cast<int32_t *>(smem + (size_t)((lds_keys + 1) & ~1) * 8);
    for (int e = threadIdx.x; e < m; e += kTolBlock) {
        lv[e] = sv[at + e];
        lp[e] = sp[at + e];
    }
    return TolQuery{lv, lp};
}

// Batch query preparation.  grid = (ceil(max_query_len / kTolSortBlock), Q).  Query q's non-NaN values go,
// ascending (ties by position; -0.0 folded to +0.0), to sv/sp[(q_offsets[q] - q_offsets[0]) + rank];
// qm[q] = how many.  A query longer than max_query_len, or one that does not fit the workspace's
// `room` values, gets qm[q] = -1 (the sweep flags it).  hits_n[q] = 0 for the sweep that follows.
__global__ __launch_bounds__(kTolSortBlock) void ts_tol_sort_kernel(
    const double *__restrict__ queries, const int64_t *__restrict__ q_offsets, int32_t max_len, int64_t room,
    double *__restrict__ sv, int32_t *__restrict__ sp, int32_t *__restrict__ qm, int32_t *__restrict__ hits_n) {
    __shared__ double tile[kTolSortTile];
    __shared__ int32_t s_nan;
    const int q = blockIdx.y;
    const int64_t o0 = q_offsets[0];
    const int64_t qo = q_offsets[q];
    const int64_t n = q_offsets[q + 1] - qo;
    const int64_t at = qo - o0;
    const bool lead = blockIdx.x == 0;
    if (lead && threadIdx.x == 0) {
        hits_n[q] = 0;
        s_nan = 0;
    }
    if (n > max_len || n < 0 || at < 0 || at + n > room) {
        if (lead && threadIdx.x == 0) qm[q] = -1;
        return;                                              // block-uniform
    }
    if (!lead && (int64_t)blockIdx.x * kTolSortBlock >= n) return;
    const int64_t i = (int64_t)blockIdx.x * kTolSortBlock + threadIdx.x;
    const double vi = i < n ? queries[qo + i] : 0.0;
    const bool live = i < n && vi == vi;
    int32_t rank = 0, nan_local = 0;
    for (int64_t t0 = 0; t0 < n; t0 += kTolSortTile) {
        const int tn = (int)(n - t0 < kTolSortTile ? n - t0 : kTolSortTile);
        __syncthreads();
        for (int e = threadIdx.x; e < tn; e += kTolSortBlock) {
            const double v = queries[qo + t0 + e];
            tile[e] = v;
            nan_local += (v != v);
        }
        __syncthreads();
        if (live) {
            const int before_me = (int)(i - t0 < 0 ? 0 : (i - t0 < tn ? i - t0 : tn));   // tile elements ahead of i
            for (int e = 0; e < tn; ++e) {
                const double v = tile[e];                    // the same address in every lane: a broadcast
                rank += (v < vi) | ((v == vi) & (e < before_me));
            }
        }
    }
    if (live) {
        sv[at + rank] = vi == 0.0 ? 0.0 : vi;
        sp[at + rank] = (int32_t)i;
    }
    if (lead) {
        if (nan_local) atomicAdd(&s_nan, nan_local);
        __syncthreads();
        if (threadIdx.x == 0) qm[q] = (int32_t)(n - s_nan);
    }
}

// The sweep.  grid = (row blocks, Q).  Sorted query q: values sv[at .. at+m), positions sp[..], with
// at = q_offsets[q] - q_offsets[0] and m = qm[q] (batch); q_offsets == nullptr: one query of m_one values at 0.
// LDSQ: the sorted query is copied to LDS first (m <= the dynamic LDS the launch gave: lds_keys).
template <int MODE, bool HOSTOUT, bool LDSQ>
__global__ __launch_bounds__(kTolBlock) void ts_match_tol_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys,
    const double *__restrict__ sv, const int32_t *__restrict__ sp, const int64_t *__restrict__ q_offsets,
    const int32_t *__restrict__ qm, int32_t m_one, int32_t lds_keys, double tol, int32_t min_match,
    const int32_t *__restrict__ exclude_ids, int32_t exclude_one, int32_t cap, int32_t *__restrict__ hits,
    int32_t *__restrict__ hits_n, HostOut ho) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    int64_t at = 0;
    int32_t m = m_one;
    if (q_offsets) {
        at = q_offsets[q] - q_offsets[0];
        m = qm[q];
    }
    if (m < 0 || (LDSQ && m > lds_keys)) {
        // longer than the caller's max_query_len, or no room for it in the workspace
        if (!HOSTOUT && threadIdx.x == 0 && bx == 0) hits_n[q] = INT32_MIN;
        if (HOSTOUT && threadIdx.x == 0) ho.counts[bx] = INT32_MIN;
        return;                                                      // block-uniform
    }
    const double *s = sv + at;
    const int32_t *pos = sp + at;
    if constexpr (LDSQ) {
        const TolQuery lq = tol_query_to_lds(smem, lds_keys, sv, sp, at, m);
        s = lq.s;
        pos = lq.pos;
    }
    if (threadIdx.x == 0) hit_open();
    __syncthreads();

    const int gl = threadIdx.x & (kGroup - 1);
    const int g = threadIdx.x / kGroup;
    const int32_t excl = exclude_ids ? exclude_ids[q] : exclude_one;
    auto dest = [&] { return HitList{hits, &hits_n[q], q, cap}; };
    const int64_t stride = (int64_t)gridDim.x * kTolGroups;
    int64_t r = (int64_t)bx * kTolGroups + g;
    const int64_t last_row = n_rows - 1;
    Row row = {};
    if (r < n_rows) row = load_row(rows + r);
    while (r < n_rows) {
        const int64_t rn = r + stride;
        const Row nrow = load_row(rows + (rn < n_rows ? rn : last_row)); // lands while this row is searched
        uint32_t cnt, m1, m2, tk[kTop];
        tol_row_scan<MODE>(keys, keys + row.off, row.len, s, pos, m, tol, gl, cnt, m1, m2, tk);
        const bool hit = (int64_t)cnt >= (int64_t)min_match && row.vid != excl;
        if (__ballot(hit) != 0ull) tol_row_reduce<MODE>(m1, m2, tk);
        if (hit && gl == 0) {
            const int32_t kth = min_match <= 0 ? -1 : kth_of<MODE>(min_match, m1, m2, tk, r);   // (count: ts_tol_kth_fixup_kernel)
            hit_emit<HOSTOUT>(row.vid, (int32_t)cnt, kth, ho, bx, dest);
        }
        row = nrow;
        r = rn;
    }
    __syncthreads();
    hit_flush<HOSTOUT, kTolBlock>(ho, bx, dest);
}

// does some key of the row match q?  The row's numeric order is arena [p-1 .. 0] then [p .. len-1] (p = negative
// keys); the keys matching q are contiguous in it, so if any does, the nearest key below or at q, or the
// nearest above it, does.
__device__ __forceinline__ bool tol_row_has(const int64_t *rk, int len, int p, double q, double tol) {
    int lo = 0, n = len;                          // first numeric index t with key(t) >= q
    while (n > 0) {
        const int half = n >> 1;
        const int t = lo + half;
        const double v = __longlong_as_double(rk[t < p ? p - 1 - t : t]);
        if (v < q) {
            lo = t + 1;
            n -= half + 1;
        } else {
            n = half;
        }
    }
    bool hit = false;
    if (lo < len) hit = tol_match(q, __longlong_as_double(rk[lo < p ? p - 1 - lo : lo]), tol);
    if (lo > 0) {
        const int t = lo - 1;
        hit = hit || tol_match(q, __longlong_as_double(rk[t < p ? p - 1 - t : t]), tol);
    }
    return hit;
}

// kth for min_match > 5: list b (a query's hit list, or one block's region of a single query's pinned hits)
// holds min(counts[b], region) hits whose kth field is -2 - row; the query (raw, in its original order) is
// queries[q_offsets[b] ..) or, with q_offsets == nullptr, queries[0 .. n_one).  A 16-lane group per hit.
__global__ __launch_bounds__(kBlock) void ts_tol_kth_fixup_kernel(
    const Row *__restrict__ rows, const int64_t *__restrict__ keys, const double *__restrict__ queries,
    const int64_t *__restrict__ q_offsets, int32_t n_one, double tol, int32_t min_match,
    int32_t *__restrict__ hits, const int32_t *__restrict__ counts, int32_t region) {
    const int b = blockIdx.x;
    const int gl = threadIdx.x & (kGroup - 1);
    const int g = threadIdx.x / kGroup;
    int n = counts[b];
    if (n > region) n = region;
    int64_t qo = 0, qlen = n_one;
    if (q_offsets) {
        qo = q_offsets[b];
        qlen = q_offsets[b + 1] - qo;
    }
    const double *qv = queries + qo;
    for (int j = g; j < n; j += kGroupsPerBlock) {
        int32_t *h = hits + ((int64_t)b * region + j) * 3;
        const int32_t code = h[2];
        if (code > -2) continue;
        const Row row = load_row(rows + (-2 - (int64_t)code));
        const int64_t *rk = keys + row.off;
        int p0 = 0, pn = row.len;                     // p = keys with a negative bit pattern (they come first)
        while (pn > 0) {
            const int half = pn >> 1;
            if (rk[p0 + half] < 0) {
                p0 += half + 1;
                pn -= half + 1;
            } else {
                pn = half;
            }
        }
        const int kth = kth_walk(qlen, min_match, [&](int64_t i) {
            const double x = qv[i];
            return x == x && tol_row_has(rk, row.len, p0, x, tol);
        });
        if (gl == 0) h[2] = kth;
    }
}

// ---- the top-k form (tvz_match_tol_topk / tvz_match_tol_sharded) ------------------------------------------------
// The same row walk; a hit becomes the index lookups' sortable word kth << 44 | video_id << 12 | count
// (ix_tk_pack: its numeric order is the (kth, video_id, count) order of the blocks tvz_topk_merge takes) and stays
// on chip.  Each WAVE keeps the k smallest words it has met, ascending and padded with all-ones, in 64 LDS words of
// its own, next to a 64-word stage that takes the hits below the list's current k-th word.  When the stage may
// overflow the wave alone ranks list + stage (rank = words below, ties by slot: equal words are all kept) and
// writes the k smallest back - no block barrier inside the row loop.  Behind the loop's one barrier the block
// takes the other three lists into the first wave's the same way and writes its k words to part[q][block][..]; nothing grows with the hit count.
constexpr int kTolTopkMaxK = 64;                       // one word per lane
constexpr int kTolTopkWaves = kTolBlock / 64;
constexpr int kTolTopkStaticLds = kTolTopkWaves * 64 * 8 * 2 + 64;   // lists + stages + a few words
constexpr int kTolTopkMaxLen = 4095;                   // count fits the word's 12 bits; the query fits LDS
constexpr int kTolReduceBlock = 1024;
constexpr int kTolReduceWaves = kTolReduceBlock / 64;
constexpr int kTolReduceLd = 8;                        // lists a wave loads per step (their loads in flight together)
constexpr unsigned long long kTolPad = ~0ull;

// Row blocks per query of the top-k sweep (one partial list each): about 6,080 blocks in all, at most 2,048 (q1_blocks' own limit: a lone query fills the machine) and at
// least 95 per query.  The sweep is bound by its searches, not by the lists, and more, shorter blocks balance
// better (profiles/tol_topk.txt: 64 per query cost 3 % against 96); 95 is what the workspace allows at Q >= 64 -
// 95 lists of k = 64 words and the query's hit total fit the 4,096 x 12 B of the hit list they replace
// (include/tvz.h states the formula).
constexpr int kTolTopkMinBlocks = 95;
constexpr int kTolTopkGridBlocks = kTolTopkMinBlocks * 64;
inline int tol_topk_max_blocks(int32_t Q) {
    const int per_q = kTolTopkGridBlocks / (Q > 0 ? Q : 1);
    return per_q < kTolTopkMinBlocks ? kTolTopkMinBlocks : per_q > 2048 ? 2048 : per_q;
}
// ... so a batch never has more partial lists than this (the workspace's size, monotone in Q)
inline int64_t tol_topk_max_lists(int32_t Q) {
    const int64_t big = (int64_t)kTolTopkMinBlocks * Q;
    return big > kTolTopkGridBlocks ? big : kTolTopkGridBlocks;
}

// One wave: kept[0..64) (ascending, padded) and stage[0 .. n_stage) -> kept = the k smallest of both, ascending,
// padded.  Returns the new k-th word (kTolPad while fewer than k are known).
__device__ __forceinline__ unsigned long long tol_topk_compact(unsigned long long *kept, const unsigned long long *stage,
                                                               int n_stage, int k, int lane) {
    const unsigned long long a = kept[lane];
    const unsigned long long b = lane < n_stage ? stage[lane] : kTolPad;
    int ra = 0, rb = 0;
#pragma unroll 4
    for (int t = 0; t < 64; ++t) {
        const unsigned long long v = kept[t];                 // the same address in every lane: a broadcast
        ra += (v < a) | ((v == a) & (t < lane));
        rb += v <= b;                                         // list slots come before stage slots
    }
#pragma unroll 4
    for (int t = 0; t < n_stage; ++t) {
        const unsigned long long v = stage[t];
        ra += v < a;
        rb += (v < b) | ((v == b) & (t < lane));
    }
    __builtin_amdgcn_wave_barrier();                          // every lane has read before any lane writes
    // the 64 + n_stage ranks are distinct and cover 0..63: every list slot is written exactly once
    if (ra < 64) kept[ra] = ra < k ? a : kTolPad;
    if (lane < n_stage && rb < 64) kept[rb] = rb < k ? b : kTolPad;
    __builtin_amdgcn_wave_barrier();
    return kept[k - 1];
}

// What a wave knows of its list (wave-uniform) and where the list lives.
struct TolTopkWave {
    unsigned long long *kept, *stage;      // 64 LDS words each, the wave's own
    unsigned long long thr;                // the list's k-th word: words at or above it cannot enter
    int n_stage, n_hits;                   // words in the stage; hits offered so far
};

// the lanes of ballot `cb` append their word to the stage (the caller has made sure they fit)
__device__ __forceinline__ void tol_topk_place(TolTopkWave &w, bool cand, unsigned long long cb, unsigned long long word) {
    if (cand) w.stage[w.n_stage + (int)lanes_below(cb)] = word;
    w.n_stage += __popcll(cb);
}

// the stage into the list
__device__ __forceinline__ void tol_topk_settle(TolTopkWave &w, int k, int lane) {
    __builtin_amdgcn_wave_barrier();
    w.thr = tol_topk_compact(w.kept, w.stage, w.n_stage, k, lane);
    w.n_stage = 0;
}
__device__ __forceinline__ void tol_topk_flush(TolTopkWave &w, int k, int lane) {
    if (w.n_stage != 0) tol_topk_settle(w, k, lane);
}

// One wave takes up to 64 more words (one per lane, kTolPad where there is none) towards its list: those below the
// list's k-th word are appended to the stage, which is compacted only when they would not fit - a sorted list
// from another block rarely has more than a few words below a live threshold, so most lists cost their load and a
// ballot.  tol_topk_flush compacts what is left.
__device__ __forceinline__ void tol_topk_take(TolTopkWave &w, unsigned long long word, int k, int lane) {
    bool cand = word < w.thr;
    unsigned long long cb = __ballot(cand);
    if (cb == 0ull) return;
    if (w.n_stage + __popcll(cb) > 64) {
        tol_topk_settle(w, k, lane);
        cand = word < w.thr;
        cb = __ballot(cand);
        if (cb == 0ull) return;
    }
    tol_topk_place(w, cand, cb, word);
}

// The sweeps' step: the leads of the wave's groups (`lead`) offer the word of their row's hit.  At most one word per
// group and step, so the stage is compacted as soon as the next step might not fit.
__device__ __forceinline__ void tol_topk_offer(TolTopkWave &w, bool lead, unsigned long long word, int k, int lane) {
    w.n_hits += __popcll(__ballot(lead));
    const bool cand = lead && word < w.thr;
    const unsigned long long cb = __ballot(cand);
    if (cb == 0ull) return;
    tol_topk_place(w, cand, cb, word);
    if (w.n_stage > 64 - 64 / kGroup) tol_topk_settle(w, k, lane);
}

// A sweep block's side: the lists of its waves and its hit count, in static LDS of the kernel (kTolTopkStaticLds).
__shared__ unsigned long long s_topk_kept[kTolTopkWaves * 64], s_topk_stg[kTolTopkWaves * 64];
__shared__ int32_t s_topk_nhits;
// before a block barrier: the block's lists, empty, and this wave's view of its own
__device__ __forceinline__ TolTopkWave tol_topk_open(int wv, int lane) {
    s_topk_kept[wv * 64 + lane] = kTolPad;
    if (threadIdx.x == 0) s_topk_nhits = 0;
    return TolTopkWave{s_topk_kept + wv * 64, s_topk_stg + wv * 64, kTolPad, 0, 0};
}
struct TolTopkOut {
    unsigned long long *list;              // the block's k words of part[q][..][k]
    int32_t *total;                        // the query's hit total
};
// Behind the row loop, the whole block: every wave settles its stage; behind the one barrier wave 0 takes the other
// waves' lists into its own and writes the block's k words, and the block's hits go to the total in one atomic.
// `out` is a callable that returns the TolTopkOut, called where it is needed (as hit_emit's `dest`).
template <class OUT>
__device__ __forceinline__ void tol_topk_finish(TolTopkWave &w, int k, int wv, int lane, OUT out) {
    tol_topk_flush(w, k, lane);
    if (lane == 0 && w.n_hits) atomicAdd(&s_topk_nhits, w.n_hits);   // LDS
    __syncthreads();
    if (wv == 0) {
#pragma unroll 1
        for (int j = 1; j < kTolTopkWaves; ++j) tol_topk_take(w, s_topk_kept[j * 64 + lane], k, lane);
        tol_topk_flush(w, k, lane);
        if (lane < k) out().list[lane] = w.kept[lane];
    }
    if (threadIdx.x == 0 && s_topk_nhits) atomicAdd(out().total, s_topk_nhits);
}

// grid = (row blocks, Q), the sorted query always in LDS (lds_keys >= every query's length, <= kTolTopkMaxLen).
// part: uint64[Q][n_lists][k], block bx writes list list0 + bx (the sweep alone: n_lists = gridDim.x, list0 = 0; behind
// the cell-posting lookup of tvz_tol_index_kernels.h: the lookup's lists come first); totals[q] (zeroed by
// ts_tol_sort_kernel) += the block's hits, one atomic.
template <int MODE>
__global__ __launch_bounds__(kTolBlock) void ts_tol_topk_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int32_t *__restrict__ sp, const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm,
    int32_t lds_keys, double tol, int32_t min_match, const int32_t *__restrict__ exclude_ids, int32_t k,
    unsigned long long *__restrict__ part, int32_t n_lists, int32_t list0, int32_t *__restrict__ totals) {
    static_assert(MODE == kModeM2 || MODE == kModeTop5, "kth is known inside the sweep for min_match 1..5");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int32_t m = qm[q];
    if (m < 0 || m > lds_keys) return;       // refused by the preparation: ts_tol_topk_reduce_kernel flags it
    const TolQuery lq = tol_query_to_lds(smem, lds_keys, sv, sp, at, m);
    const double *s = lq.s;
    const int32_t *pos = lq.pos;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    TolTopkWave tw = tol_topk_open(wv, lane);
    __syncthreads();

    const int gl = threadIdx.x & (kGroup - 1);
    const int g = threadIdx.x / kGroup;
    const int32_t excl = exclude_ids ? exclude_ids[q] : -1;
    const int64_t stride = (int64_t)gridDim.x * kTolGroups;
    int64_t r = (int64_t)bx * kTolGroups + g;
    int64_t r_wave = (int64_t)bx * kTolGroups + wv * (64 / kGroup);    // the wave's first group: its longest loop
    const int64_t last_row = n_rows - 1;
    Row row = load_row(rows + (r < n_rows ? r : last_row));
    while (r_wave < n_rows) {                // wave-uniform: the wave compacts as one
        const int64_t rn = r + stride;
        const Row nrow = load_row(rows + (rn < n_rows ? rn : last_row));
        const bool live = r < n_rows;
        uint32_t cnt, m1, m2, tk[kTop];
        tol_row_scan<MODE>(keys, keys + row.off, live ? row.len : 0, s, pos, m, tol, gl, cnt, m1, m2, tk);
        const bool hit = live && (int64_t)cnt >= (int64_t)min_match && row.vid != excl;
        if (__ballot(hit) != 0ull) {
            tol_row_reduce<MODE>(m1, m2, tk);
            const unsigned long long word = ix_tk_pack(kth_of<MODE>(min_match, m1, m2, tk, r), row.vid, cnt);
            tol_topk_offer(tw, hit && gl == 0, word, k, lane);
        }
        row = nrow;
        r = rn;
        r_wave += stride;
    }
    tol_topk_finish(tw, k, wv, lane, [&] {
        return TolTopkOut{part + ((int64_t)q * n_lists + list0 + bx) * k, &totals[q]};
    });
}

// One block per query: the k smallest words of its n_lists sorted partial lists -> d_out[q] = int32[k+1][3]: k rows
// (video_id, count, kth) ascending, padding (-1, 0, TVZ_KTH_NEVER), then (-1, n_hits, TVZ_KTH_NEVER).  A wave takes
// every kTolReduceWaves-th list, kTolReduceLd lists per step (their loads in flight together), and keeps its k best as
// the sweep does; a list whose words are all at or above the wave's k-th word costs its load only.
// A query the preparation refused (qm < 0 or > lds_keys): all padding, n_hits = INT32_MIN.
__global__ __launch_bounds__(kTolReduceBlock) void ts_tol_topk_reduce_kernel(
    const unsigned long long *__restrict__ part, int32_t n_lists, int32_t k, const int32_t *__restrict__ qm,
    int32_t lds_keys, const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    __shared__ unsigned long long s_kept[kTolReduceWaves * 64], s_stg[kTolReduceWaves * 64];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    int32_t *out = d_out + (int64_t)q * (k + 1) * 3;
    const int32_t m = qm[q];
    const bool refused = m < 0 || m > lds_keys;
    TolTopkWave tw{s_kept + wv * 64, s_stg + wv * 64, kTolPad, 0, 0};
    tw.kept[lane] = kTolPad;
    if (!refused) {
        const unsigned long long *lists = part + (int64_t)q * n_lists * k;
        for (int l0 = wv; l0 < n_lists; l0 += kTolReduceLd * kTolReduceWaves) {   // wave-uniform
            unsigned long long w[kTolReduceLd];
#pragma unroll
            for (int j = 0; j < kTolReduceLd; ++j) {
                const int l = l0 + j * kTolReduceWaves;
                w[j] = (l < n_lists && lane < k) ? lists[(int64_t)l * k + lane] : kTolPad;
            }
#pragma unroll
            for (int j = 0; j < kTolReduceLd; ++j) tol_topk_take(tw, w[j], k, lane);
        }
        tol_topk_flush(tw, k, lane);
        __syncthreads();
        if (wv == 0) {
#pragma unroll 1
            for (int j = 1; j < kTolReduceWaves; ++j) tol_topk_take(tw, s_kept[j * 64 + lane], k, lane);
            tol_topk_flush(tw, k, lane);
        }
    }
    if (wv != 0) return;
    const unsigned long long w = tw.kept[lane];                          // all padding for a refused query
    if (lane < k) {
        const bool pad = w == kTolPad;
        out[lane * 3 + 0] = pad ? -1 : (int32_t)((w >> 12) & 0xffffffffu);
        out[lane * 3 + 1] = pad ? 0 : (int32_t)(w & 0xfffu);
        out[lane * 3 + 2] = pad ? TVZ_KTH_NEVER : (int32_t)(w >> 44);
    }
    if (lane == 0) {
        out[k * 3 + 0] = -1;
        out[k * 3 + 1] = refused ? INT32_MIN : totals[q];
        out[k * 3 + 2] = TVZ_KTH_NEVER;
    }
}

}  // namespace
