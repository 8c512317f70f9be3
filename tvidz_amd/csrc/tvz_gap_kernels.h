// tvz_gap_kernels.h — the kernels of tvz_align_candidates (include/tvz_gap.h) and tvz_align_candidates_rates
// (include/tvz_gap_rates.h); gfx950, wave64.  The two calls share every step but the last:
//
//   ts_gapc_offsets_kernel  where every probe list goes: an exclusive scan of the probe slots of the Q R lists.
//   ts_gapc_probe_kernel    the probes: a thread per (query, rate, position) writes its 8 slots.
//   (the internal match over the handle's code table: the probe lists are its queries)
//   ts_gapc_select_kernel   the plain call's last step: per query the C best of its hit list, the block and the total.
//   ts_gapr_fold_kernel     the rates call's: per query its R hit lists folded per id, the C best, the block, the total.
//
//   ts_gapc_merge_kernel    per query the C best of up to 16 blocks of the plain call (tvz_align_candidates_merge).
//   ts_gapr_merge_kernel    ... of up to 16 blocks of the rates call, one row per id (tvz_align_candidates_rates_merge).
//
// The plain call is the shared steps at R = 1 with the rate list {1.0}.  The queries come sorted from ts_tol_sort_kernel (tvz_tol_kernels.h): sv[at .. at + m), at = q_offsets[q] -
// q_offsets[0], m = qm[q]; qm[q] < 0: longer than the call's max_query_len.  From tvz_topk_kernels.h: bitonic_sort,
// sort_and_keep, topk_total; from tvz_wave.h: wave_scan_incl, waves_sum, wave_lds_fence; from tvz_align_kernels.h: AlRates, al_scaled.  Included by tvz_match.hip behind them.
#pragma once
#include "tvz_gap_codes.h"
#include "tvz_topk_kernels.h"

namespace {

constexpr int kGapOffBlock = 1024;             // one block scans every query of the call (Q <= 65,535: 64 per thread)
constexpr int kGapProbeBlock = 256;

// Probe slots of a query of m sorted values (tvz_gap::probe_slots); a refused query has none.
__device__ __forceinline__ bool gapc_refused(int32_t m) { return tvz_gap::probe_slots(m) < 0; }
__device__ __forceinline__ int32_t gapc_slots(int32_t m) { return gapc_refused(m) ? 0 : tvz_gap::probe_slots(m); }

// The lookup sees Q R probe lists: list p = q R + i is query q at rate i (R = 1, the rate 1.0: the plain call).
// p_off[p] = the slots of the lists before p (a list has its query's, p / R), p_off[Q R] = all of them; with somewhere
// to put them (excl_out != NULL), excl_out[p] = exclude_ids[p / R]: the lookup reads one id per probe list, and the
// plain call, whose lists are its queries, hands it the caller's array instead.  grid = 1; Q R <= 65,535: 64 per thread.
__global__ __launch_bounds__(kGapOffBlock) void ts_gapc_offsets_kernel(const int32_t *__restrict__ qm, int32_t Q, int32_t R,
                                                                        const int32_t *__restrict__ exclude_ids,
                                                                        int64_t *__restrict__ p_off,
                                                                        int32_t *__restrict__ excl_out) {
    __shared__ uint32_t s_w[kGapOffBlock / 64];
    const int n = Q * R;
    const int per = (n + kGapOffBlock - 1) / kGapOffBlock;
    const int p0 = (int)threadIdx.x * per;
    uint32_t mine = 0;
    for (int p = p0; p < p0 + per && p < n; ++p) mine += (uint32_t)gapc_slots(qm[p / R]);
    const uint32_t incl = wave_scan_incl(mine);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before, all;
    waves_sum<kGapOffBlock / 64>(s_w, wave, before, all);
    uint32_t at = before + incl - mine;
    for (int p = p0; p < p0 + per && p < n; ++p) {
        p_off[p] = (int64_t)at;
        at += (uint32_t)gapc_slots(qm[p / R]);
        if (excl_out) excl_out[p] = exclude_ids[p / R];
    }
    if (threadIdx.x == 0) p_off[n] = (int64_t)all;
}

// The query side of the contract on x' = x * rho (al_scaled of tvz_align_kernels.h: the alignment calls' one
// multiplication, never contracted).  grid = (ceil(positions / kGapProbeBlock), Q, R); thread i of query q at rate
// z = blockIdx.z takes position i (i + 3 < m) and writes probes[p_off[q R + z] + 8 i ..+ 8): slot v chooses
// a_j + ((v >> j) & 1) for gap j.  A choice with an invalid bin is written as NaN: the lookup drops a NaN before it
// probes (canon_key: "NaN never matches", in every match kernel), so such a slot can match nothing and the slots keep
// their fixed places.  The division is al_bin's: a subtraction, then a true division.  Four 16-byte stores per thread
// (p_off is a multiple of 8 slots).
// The plain call is R = 1 with the rate list {1.0}, and its probes are bit for bit those of a kernel without the
// multiplication: x * 1.0 == x for every double (the product is never contracted into what follows: al_scaled is
// compiled with fp contract(off)), a NaN stays a NaN, and from the four scaled values on the expressions are the same.
__global__ __launch_bounds__(kGapProbeBlock) void ts_gapc_probe_kernel(const double *__restrict__ sv,
                                                                        const int64_t *__restrict__ q_offsets,
                                                                        const int32_t *__restrict__ qm, double gap_eps,
                                                                        AlRates rates, const int64_t *__restrict__ p_off,
                                                                        double *__restrict__ probes) {
    const int q = blockIdx.y;
    const int32_t m = qm[q];
    if (gapc_slots(m) == 0) return;                                  // refused, or fewer than 4 values (block-uniform)
    const int i = (int)blockIdx.x * kGapProbeBlock + (int)threadIdx.x;
    if (i + 3 >= m) return;
    const double rho = rates.r[blockIdx.z];                          // (a uniform index: scalar loads of the argument)
    const double *s = sv + (q_offsets[q] - q_offsets[0]) + i;
    const double s0 = al_scaled(s[0], rho), s1 = al_scaled(s[1], rho), s2 = al_scaled(s[2], rho), s3 = al_scaled(s[3], rho);
    double a[3];
    a[0] = floor((s1 - s0) / gap_eps);
    a[1] = floor((s2 - s1) / gap_eps);
    a[2] = floor((s3 - s2) / gap_eps);
    double lo[3], hi[3];                                             // a gap's two choices, scaled to their place; NaN: invalid
    const double place[3] = {1.0, tvz_gap::kBin1, tvz_gap::kBin2};
    const double none = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double b = a[j] + 1.0;
        lo[j] = (a[j] >= 0.0 && a[j] <= tvz_gap::kMaxBin) ? a[j] * place[j] : none;
        hi[j] = (b >= 0.0 && b <= tvz_gap::kMaxBin) ? b * place[j] : none;
    }
    const int64_t p = (int64_t)q * rates.n + blockIdx.z;
    double2 *o = reinterpret_cast<double2 *>(probes + p_off[p] + (int64_t)tvz_gap::kVariants * i);
#pragma unroll
    for (int v = 0; v < tvz_gap::kVariants; v += 2) {                // (NaN + x = NaN: an invalid choice poisons its slots)
        const double rest = ((v & 2) ? hi[1] : lo[1]) + ((v & 4) ? hi[2] : lo[2]);
        o[v >> 1] = make_double2(lo[0] + rest, hi[0] + rest);
    }
}

// The selection.  grid = Q.  Query q's hit list hits[q][min(hits_n[q], cap)][3] = (video_id, count, kth) -> the C
// largest by the word count << 32 | (2^31 - 1 - video_id), i.e. count descending, then video_id ascending, written as
// rows (video_id, count), padded with (-1, 0), and the row (-1, total): topk_total's rule (negated when the list
// overflowed `cap`).  A refused query: padding and INT32_MIN.  The word is kept complemented, so that the ascending
// bitonic sort of tvz_topk_kernels.h keeps the largest first and its "no entry" (~0) is the word 0, which no hit has
// (count >= min_count >= 1).  One 8-byte store per row.
__global__ __launch_bounds__(kBlock) void ts_gapc_select_kernel(const int32_t *__restrict__ hits,
                                                                 const int32_t *__restrict__ hits_n,
                                                                 const int32_t *__restrict__ qm, int32_t cap, int32_t C,
                                                                 int32_t *__restrict__ out) {
    __shared__ uint64_t key[kSortCap];
    __shared__ int32_t cnt[kSortCap];
    const int q = blockIdx.x;
    int2 *o = reinterpret_cast<int2 *>(out) + (int64_t)q * (C + 1);
    if (gapc_refused(qm[q])) {                                       // block-uniform
        for (int i = threadIdx.x; i <= C; i += kBlock) o[i] = make_int2(-1, i == C ? INT32_MIN : 0);
        return;
    }
    const int32_t total = hits_n[q];
    const int n = total > cap ? cap : (total < 0 ? 0 : total);
    const int32_t *src = hits + (int64_t)q * cap * 3;
    int pos = 0;                                                     // block-uniform fill level
    int j = 0;
    while (j < n) {
        int take = n - j;
        if (take > kSortCap - pos) take = kSortCap - pos;
        for (int i = threadIdx.x; i < take; i += kBlock) {
            const int32_t vid = src[(j + i) * 3], c = src[(j + i) * 3 + 1];
            key[pos + i] = vid < 0 ? ~0ULL : ~(((uint64_t)(uint32_t)c << 32) | (uint32_t)(0x7fffffff - vid));
            cnt[pos + i] = c;
        }
        pos += take;
        j += take;
        __syncthreads();
        if (pos == kSortCap) sort_and_keep(key, cnt, pos, C);
    }
    __syncthreads();
    sort_and_keep(key, cnt, pos, C);
    for (int i = threadIdx.x; i < C; i += kBlock) {
        const uint64_t w = i < pos ? ~key[i] : 0ULL;
        o[i] = w == 0ULL ? make_int2(-1, 0) : make_int2(0x7fffffff - (int32_t)(uint32_t)w, (int32_t)(w >> 32));
    }
    if (threadIdx.x == 0) o[C] = make_int2(-1, topk_total(total < 0 ? 0 : total, total > cap));
}

// ---- the merge of the shards' blocks (tvz_align_candidates_merge, include/tvz_gap_shards.h) -------------------------
constexpr int kGapMergeBlock = 256;
constexpr int kGapMergeWaves = kGapMergeBlock / 64;    // queries per block: a wave each
constexpr int kGapMergeMaxLists = 16;                  // one total per lane; 16 x kMaxC = 1,024 rows of a query at most

// dynamic LDS of a launch: every wave's n_lists x C words
inline size_t gapc_merge_lds_bytes(int32_t n_lists, int32_t C) {
    return (size_t)kGapMergeWaves * (size_t)n_lists * (size_t)C * sizeof(uint64_t);
}

// gathered int32[n_lists][Q][C + 1][2] -> out int32[Q][C + 1][2], both in the block format of ts_gapc_select_kernel.
// grid = ceil(Q / kGapMergeWaves); one wave per query, no block barrier.  A row (video_id >= 0, count >= 0) becomes the
// word 2^63 | count << 32 | (2^31 - 1 - video_id), padding the word 0, so that "larger word" is the contract's order
// and padding is last; the words of list l lie in the wave's LDS at [l C, l C + C).  PRECONDITION: every list is sorted
// by that order (descending words).  The rank of row p of list l is p + over the lists before it their words >= w +
// over the lists behind it their words > w: equal words are ordered by (list, position), so the ranks of a query's
// rows are the distinct numbers 0 .. n - 1, and the rows of rank < C are the output - each written by the lane that
// holds it, the rest of the C rows padded.  A count in a sorted list is a branch-free binary search over LDS.  Whatever
// the lists hold, a rank is >= 0 and only ranks < C are written: nothing is stored outside the query's block.
// The total: the lists' last rows by topk_total's rule (|t| summed in 64 bits, saturated, negated if any was negative);
// INT32_MIN in any list refuses the query (all padding, INT32_MIN).  One 8-byte store per row.
__global__ __launch_bounds__(kGapMergeBlock) void ts_gapc_merge_kernel(const int32_t *__restrict__ gathered, int32_t n_lists,
                                                                       int32_t Q, int32_t C, int32_t *__restrict__ out) {
    extern __shared__ uint64_t gapc_merge_sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kGapMergeWaves + wave;
    if (q >= Q) return;                                              // wave-uniform
    const int n = n_lists * C;                                       // <= 1,024
    uint64_t *w = gapc_merge_sh + (size_t)wave * n;
    const int64_t c1 = (int64_t)C + 1;
    const int2 *blocks = reinterpret_cast<const int2 *>(gathered);   // [n_lists][Q][C + 1] rows of 8 bytes
    int2 *o = reinterpret_cast<int2 *>(out) + q * c1;
    // the lists' totals, one per lane
    const int32_t t = lane < n_lists ? blocks[((int64_t)lane * Q + q) * c1 + C].y : 0;
    long long sum = t == INT32_MIN ? 0 : (t < 0 ? -(long long)t : (long long)t);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (__ballot(t == INT32_MIN) != 0ull) {                          // refused: wave-uniform
        for (int i = lane; i <= C; i += 64) o[i] = make_int2(-1, i == C ? INT32_MIN : 0);
        return;
    }
    const bool over = __ballot(t < 0) != 0ull;
    int n_rows = 0;                                                  // wave-uniform: the rows that are no padding
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        uint64_t word = 0;
        if (i < n) {
            const int l = i / C, p = i - l * C;
            const int2 r = blocks[((int64_t)l * Q + q) * c1 + p];
            if (r.x >= 0) word = (1ULL << 63) | ((uint64_t)((uint32_t)r.y & 0x7fffffffu) << 32) | (uint32_t)(0x7fffffff - r.x);
            w[i] = word;
        }
        n_rows += __popcll(__ballot(word != 0ULL));
    }
    wave_lds_fence();
    int top = 1;                                                     // the largest power of two <= C
    while (top * 2 <= C) top *= 2;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const uint64_t word = i < n ? w[i] : 0ULL;
        if (word == 0ULL) continue;
        const int l = i / C;
        int rank = i - l * C;                                        // the rows before it in its own list
        for (int m = 0; m < n_lists && rank < C; ++m) {
            if (m == l) continue;
            const uint64_t thr = word + (m > l ? 1ULL : 0ULL);       // (a word is below 2^64 - 1: the id's field is 31 bits)
            const uint64_t *lm = w + m * C;
            int at = 0;                                              // the words of list m that are >= thr
            for (int step = top; step > 0; step >>= 1)
                if (at + step <= C && lm[at + step - 1] >= thr) at += step;
            rank += at;
        }
        if (rank < C)
            o[rank] = make_int2(0x7fffffff - (int32_t)(uint32_t)(word & 0x7fffffffu), (int32_t)((word >> 32) & 0x7fffffffu));
    }
    for (int i = n_rows + lane; i < C; i += 64) o[i] = make_int2(-1, 0);
    if (lane == 0) o[C] = make_int2(-1, topk_total(sum, over));
}

// ---- the fold of the call with a rate list (tvz_align_candidates_rates, include/tvz_gap_rates.h) --------------------
// Behind the shared offsets, probes and lookup, query q has R hit lists, one per rate (list q R + i): per id the best
// (count, smallest rate index), then the C best ids, the block and the total.

// The words of the fold.  A count is at most kGaprMaxCount (a query has at most 4,095 probe slots), a rate index at
// most 7, a video id at most 2^31 - 1: the three fit one 64-bit word, in two orders.  Both are ASCENDING orders for
// bitonic_sort, whose "no entry" ~0 is above every word (the top bit of a word is clear).
//   by id:     id << 32 | (4,095 - count) << 4 | rate    id ascending, then count descending, then rate ascending:
//                                                        the FIRST entry of an id is its best, at its smallest rate
//   by output: (4,095 - count) << 35 | id << 4 | rate    count descending, then id ascending: the contract's order
constexpr uint32_t kGaprMaxCount = 4095;
__device__ __forceinline__ uint64_t gapr_by_id(int32_t vid, int32_t count, int rate) {
    const uint32_t c = (uint32_t)count > kGaprMaxCount ? kGaprMaxCount : (uint32_t)count;
    return ((uint64_t)(uint32_t)vid << 32) | ((uint64_t)(kGaprMaxCount - c) << 4) | (uint32_t)rate;
}
__device__ __forceinline__ uint64_t gapr_to_output(uint64_t w) {
    return ((w & 0xfff0ULL) << 31) | ((w >> 32) << 4) | (w & 0xfULL);
}
__device__ __forceinline__ uint64_t gapr_to_id(uint64_t w) {
    return (((w >> 4) & 0x7fffffffULL) << 32) | ((w >> 31) & 0xfff0ULL) | (w & 0xfULL);
}
// one output row: a 12-byte vector store (the rows of a block are 4-byte aligned, no more)
struct GaprRow {                                                     // 12 bytes, 4-byte aligned: never widened to 16
    int32_t id, best, rate;
};
__device__ __forceinline__ void gapr_store_row(int32_t *out, int64_t row, int32_t a, int32_t b, int32_t c) {
    reinterpret_cast<GaprRow *>(out)[row] = GaprRow{a, b, c};
}

// The fold and the selection.  grid = Q.  Query q's R hit lists hits[q R + i][min(hits_n[q R + i], cap)][3] =
// (video_id, count, kth) -> out[q][C + 1][3] as include/tvz_gap_rates.h has it.
// The lists are streamed as ONE sequence in chunks that fill the sort buffer.  Per chunk: the kept entries (at most C,
// one per id, in the by-id word) and the chunk's are sorted by id; every entry whose predecessor has its id is dropped -
// what stays of an id is its largest count at its smallest rate index, for ANY number of entries per id; the rest,
// turned into the by-output word, is sorted again and the C first are kept.  This is exact: the kept set is the C best
// of the per-id maxima so far in the order (count, id), an id that is dropped was behind C others, whose maxima only
// grow, so it can come back only with a larger count - and then that count is its maximum; with an equal count it
// stays out, rightly, since its place in the order has not changed.
// n_pairs: the lists' counts summed in 64 bits, negated if any list overflowed `cap` (topk_total).  A refused query:
// padding and INT32_MIN, through the same two store sites as every other.  cnt[] rides along as zeros (bitonic_sort's second key).  One 12-byte store per row.
__global__ __launch_bounds__(kBlock) void ts_gapr_fold_kernel(const int32_t *__restrict__ hits,
                                                               const int32_t *__restrict__ hits_n,
                                                               const int32_t *__restrict__ qm, int32_t R, int32_t cap,
                                                               int32_t C, int32_t *__restrict__ out) {
    __shared__ uint64_t key[kSortCap];
    __shared__ int32_t cnt[kSortCap];
    __shared__ int32_t s_start[kArMaxRates + 1];                     // where list i starts in the one sequence
    const int q = blockIdx.x;
    const int64_t row0 = (int64_t)q * (C + 1);
    const bool refused = gapc_refused(qm[q]);                        // block-uniform, like everything up to the loop:
    long long pairs = 0;                                             // a refused query folds nothing and pads every row
    bool over = false;
    int n = 0;
    for (int i = 0; i < R && !refused; ++i) {
        const int32_t t = hits_n[(int64_t)q * R + i];
        if (threadIdx.x == 0) s_start[i] = n;
        pairs += t < 0 ? 0 : t;
        over = over || t > cap;
        n += t > cap ? cap : (t < 0 ? 0 : t);                        // (at most 8 x cap: cap x 12 bytes exist, so cap < 2^28)
    }
    if (threadIdx.x == 0) s_start[R] = n;
    __syncthreads();
    const int32_t *src = hits + (int64_t)q * R * cap * 3;            // list i starts at src + i * cap * 3
    int pos = 0;                                                     // the kept entries: by-id words, one per id
    int j = 0;
    while (j < n) {
        int take = n - j;
        if (take > kSortCap - pos) take = kSortCap - pos;
        for (int e = threadIdx.x; e < take; e += kBlock) {
            const int f = j + e;
            int i = 0;
            while (f >= s_start[i + 1]) ++i;                         // (f < n = s_start[R]: it ends)
            const int32_t *h = src + ((int64_t)i * cap + (f - s_start[i])) * 3;
            const int32_t vid = h[0];
            key[pos + e] = vid < 0 ? ~0ULL : gapr_by_id(vid, h[1], i);
            cnt[pos + e] = 0;
        }
        pos += take;
        j += take;
        __syncthreads();
        sort_and_keep(key, cnt, pos, kSortCap);                      // by id; keeps all
        // who repeats its predecessor's id (read everywhere before anyone rewrites)
        for (int e = threadIdx.x; e < pos; e += kBlock)
            cnt[e] = e > 0 && key[e] != ~0ULL && (key[e] >> 32) == (key[e - 1] >> 32);
        __syncthreads();
        for (int e = threadIdx.x; e < pos; e += kBlock) {
            const uint64_t w = key[e];
            key[e] = (cnt[e] || w == ~0ULL) ? ~0ULL : gapr_to_output(w);
            cnt[e] = 0;
        }
        __syncthreads();
        sort_and_keep(key, cnt, pos, C);                             // by output; pos = min(pos, C)
        const bool mine = (int)threadIdx.x < pos && key[threadIdx.x] != ~0ULL;      // (C <= 64 < kBlock)
        pos = __syncthreads_count(mine);                             // the entries are in front of the dropped ones
        if (j < n) {                                                 // back to the by-id word for the next chunk
            if (mine) key[threadIdx.x] = gapr_to_id(key[threadIdx.x]);
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < C; i += kBlock) {
        if (i < pos) {
            const uint64_t w = key[i];
            gapr_store_row(out, row0 + i, (int32_t)((w >> 4) & 0x7fffffffULL), (int32_t)(kGaprMaxCount - (uint32_t)(w >> 35)),
                           (int32_t)(w & 0xfULL));
        } else {
            gapr_store_row(out, row0 + i, -1, 0, 0);
        }
    }
    if (threadIdx.x == 0) gapr_store_row(out, row0 + C, -1, refused ? INT32_MIN : topk_total(pairs, over), 0);
}

// ---- the merge of the shards' blocks of the rates call (tvz_align_candidates_rates_merge, -------------------------
// ---- include/tvz_gap_rates_shards.h) -------------------------------------------------------------------------------
constexpr int kGaprMergeMaxLists = 16;
constexpr int kGaprMergeCap = kGaprMergeMaxLists * tvz_gap::kMaxC;   // 1,024 rows of a query at most: 12 KiB of LDS

// gathered int32[n_lists][Q][C + 1][3] -> out int32[Q][C + 1][3], both in the block format of ts_gapr_fold_kernel.
// grid = Q: one block per query (the wave-per-query plain merge above spends ~1,700 dependent LDS round trips per
// lane at 16 x 64, and ranks by binary search cannot drop a repeated id).  It is ONE chunk of the fold's procedure, in
// the fold's words: every row (video_id >= 0) becomes gapr_by_id(id, best, rate index & 15), padding ~0; sorted by id,
// every entry whose predecessor has its id is dropped - what stays of an id is its largest best at its smallest rate
// index, however many lists hold it; the rest, as by-output words, is sorted again and the C first are written.  The
// lists need not be sorted.  The sort buffers are this kernel's own (kGaprMergeCap entries, not the fold's kSortCap),
// and the chunk body is a copy of the fold's, not a function shared with it: the fold's machine code stays as it was.
// sort_and_keep pads to the next power of two of n_lists x C only.
// The total: the lists' last rows through LDS, reduced by every thread alike in 64 bits (16 |t| of up to 2^31 do not
// fit waves_sum's 32-bit words) by topk_total's rule; INT32_MIN in any list refuses the query, which then folds no row
// and goes through the same two store sites as every other.  A rate index is masked to its 4 bits and a best clamped
// to kGaprMaxCount (gapr_by_id), so a row out of the contract's ranges changes this query's rows only; only rows
// row0 .. row0 + C are ever written.  One 12-byte store per row.
// LDS as built: 12,608 bytes - the three arrays' 12,352 and 256 more, which the fold carries over its arrays too and
// ts_gapc_select_kernel (24,576, exactly its arrays) does not: the two kernels that call __syncthreads_count have them,
// so they are taken to be that call's own words (read off the code objects' metadata, not off the compiler's source).
__global__ __launch_bounds__(kBlock) void ts_gapr_merge_kernel(const int32_t *__restrict__ gathered, int32_t n_lists,
                                                                int32_t Q, int32_t C, int32_t *__restrict__ out) {
    __shared__ uint64_t key[kGaprMergeCap];
    __shared__ int32_t cnt[kGaprMergeCap];
    __shared__ int32_t s_t[kGaprMergeMaxLists];
    const int64_t q = blockIdx.x;
    const int64_t c1 = (int64_t)C + 1;
    const int64_t row0 = q * c1;
    if ((int)threadIdx.x < n_lists) s_t[threadIdx.x] = gathered[(((int64_t)threadIdx.x * Q + q) * c1 + C) * 3 + 1];
    __syncthreads();
    long long sum = 0;                                               // block-uniform, like everything below
    bool over = false, refused = false;
    for (int l = 0; l < n_lists; ++l) {
        const int32_t t = s_t[l];
        refused = refused || t == INT32_MIN;
        over = over || t < 0;
        sum += t == INT32_MIN ? 0 : (t < 0 ? -(long long)t : (long long)t);
    }
    const int n = refused ? 0 : n_lists * C;                         // <= kGaprMergeCap
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const int l = e / C, p = e - l * C;
        const int32_t *r = gathered + (((int64_t)l * Q + q) * c1 + p) * 3;
        const int32_t vid = r[0];
        key[e] = vid < 0 ? ~0ULL : gapr_by_id(vid, r[1], r[2] & 0xf);
        cnt[e] = 0;
    }
    int pos = n;
    __syncthreads();
    sort_and_keep(key, cnt, pos, kGaprMergeCap);                     // by id; keeps all
    // who repeats its predecessor's id (read everywhere before anyone rewrites)
    for (int e = threadIdx.x; e < pos; e += kBlock)
        cnt[e] = e > 0 && key[e] != ~0ULL && (key[e] >> 32) == (key[e - 1] >> 32);
    __syncthreads();
    for (int e = threadIdx.x; e < pos; e += kBlock) {
        const uint64_t w = key[e];
        key[e] = (cnt[e] || w == ~0ULL) ? ~0ULL : gapr_to_output(w);
        cnt[e] = 0;
    }
    __syncthreads();
    sort_and_keep(key, cnt, pos, C);                                 // by output; pos = min(pos, C)
    const bool mine = (int)threadIdx.x < pos && key[threadIdx.x] != ~0ULL;          // (C <= 64 < kBlock)
    pos = __syncthreads_count(mine);                                 // the entries are in front of the dropped ones
    for (int i = threadIdx.x; i < C; i += kBlock) {
        if (i < pos) {
            const uint64_t w = key[i];
            gapr_store_row(out, row0 + i, (int32_t)((w >> 4) & 0x7fffffffULL), (int32_t)(kGaprMaxCount - (uint32_t)(w >> 35)),
                           (int32_t)(w & 0xfULL));
        } else {
            gapr_store_row(out, row0 + i, -1, 0, 0);
        }
    }
    if (threadIdx.x == 0) gapr_store_row(out, row0 + C, -1, refused ? INT32_MIN : topk_total(sum, over), 0);
}

}  // namespace
