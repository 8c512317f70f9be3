// tvz_align_parts_kernels.h — every aligned part of a NAMED stored video (tvz_align_parts), gfx950
// wave64.  Included by tvz_match.hip only, behind tvz_align_kernels.h, whose functions for one row it shares: al_wave /
// al_wave_clear (a wave's part of the LDS, aw_lds_bytes), al_key_range, al_bin_extremes (where a bin's votes lie, with
// ApOutside below as the rule for which pairs count) and al_best_bin; also al_bin, al_x, al_lo, AlRates, Row, load_row.
// The window walk itself, ap_votes, is the one copy left of al_sweep's loop: it stays because moving both into one
// function moved the sweeps' machine code.  The queries are sorted by ts_tol_sort_kernel.
//
// The call is a refinement: the search (tvz_align_span_topk), an exact match or a user has named up to k stored video
// ids per upload, and every (upload, id) pair is aligned in full - Q x k row walks, not one per row of the table.
//
// Contract (include/tvz.h): part 0 of a row is the span call's - per rate the best bin of [-B, B] under the wide call's
// tie rule, the rate with the most votes kept (the smaller index on a tie), and over the pairs (key c, index t of the
// sorted query) that vote into that bin the extremes t_first / t_last / c_lo / c_hi.  Part i >= 1, at the kept rate:
// the same over the pairs whose t lies outside every earlier [t_first, t_last] and whose c lies outside every earlier
// [c_lo, c_hi]; nq / nr count the indices / row keys inside the part's own ranges and outside the earlier ones.  The
// list ends at the first part with fewer than min_votes votes, or at max_parts.
//
// Three launches:
//   ts_alignp_locate_kernel  grid (row blocks, Q): one pass over the row table, a thread per row, the query's ids in
//                            LDS; a row whose video_id is the id of pair (q, j) takes a slot of that pair through the
//                            pair's atomic counter (zeroed by the host's memset) - kApMaxRows slots, and the counter
//                            keeps counting past them: it is n_rows.
//   ts_alignp_walk_kernel    grid (k, Q): one block of kAlWaves waves per pair, a wave per candidate slot, then slots
//                            4..7.  The sorted query lies in LDS once per block and every wave has a histogram
//                            window, a touched list and resume positions of its own - the sweep's layout (al_wave)
//                            - so the only block barrier stands in front of the row walks.  Part 0 is the sweep's
//                            window walk over the rates (ap_votes<false>); every later part the same walk at the
//                            kept rate where a pair votes only if its t and c pass the at most three exclusion
//                            ranges, which live in registers (ApRanges: constant indices only).  After each part
//                            the four extremes (al_bin_extremes with ApOutside) and one counting pass each for nr
//                            and nq.  A slot's result goes to the workspace: int32[1 + max_parts][6].
//   ts_alignp2_walk_kernel   the same walk under TVZ_ALIGN_TWO_BINS (tvz_align_parts_flags, include/tvz_parts_flags.h;
//                            DESIGN.md 4.20): every part is the best WINDOW of two adjacent bins (ap_votes<.., true>,
//                            al_bin_extremes<ApOutside, true>), launched in the walk's place; locate and pick are shared.
//   ts_alignp_pick_kernel    a wave per pair: the slot with the most part-0 votes, the earlier row of the table on a
//                            tie (the slots fill in no fixed order: the row's index decides), is copied out with
//                            n_rows and m in its header and zeros behind n_parts; or the refused / absent / no-pair
//                            form is written.
// And, for a table in shards, one more launch behind the shards' calls (tvz_align_parts_merge):
//   ts_alignp_merge_kernel   a 16-lane group per pair, a lane per shard's answer: the answer with the most part-0 votes
//                            among the shards that hold a row of the id, n_rows summed, a refusal kept.
// No scratch memory, no block barrier inside a row walk; global memory is written with vector stores only.
#pragma once
#include "tvz_align_kernels.h"
#include "tvz_wave.h"

namespace {

constexpr int kApMaxParts = 4;                         // TVZ_ALIGN_MAX_PARTS
constexpr int kApMaxRows = 8;                          // TVZ_ALIGN_PARTS_MAX_ROWS: candidate slots of a pair
constexpr int kApCols = 6;                             // int32 columns of a row of d_parts
constexpr int kApLocateBlock = 256;
constexpr int kApLocateMaxBlocks = 1024;               // per query: a thread then takes a few rows of a large table
constexpr int kApPickBlock = 256;
constexpr int kApPickWaves = kApPickBlock / 64;        // pairs per block: a wave each

// int32 words of one slot's (and one pair's) result
__host__ __device__ inline int ap_words(int32_t max_parts) { return (1 + max_parts) * kApCols; }

// The index and key ranges of the earlier parts, at most kApMaxParts - 1 of them.  Members are only ever named with
// constant indices (unrolled loops, ap_push's shift), so the struct stays in registers.  An unused entry is the empty
// range: no t is >= 1 and <= 0, no c is >= +inf and <= -inf.
struct ApRanges {
    int tf[kApMaxParts - 1], tl[kApMaxParts - 1];
    double lo[kApMaxParts - 1], hi[kApMaxParts - 1];
};
__device__ __forceinline__ ApRanges ap_no_ranges() {
    ApRanges ex;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int i = 0; i < kApMaxParts - 1; ++i) {
        ex.tf[i] = 1;
        ex.tl[i] = 0;
        ex.lo[i] = inf;
        ex.hi[i] = -inf;
    }
    return ex;
}
// one more part's ranges; the oldest entry falls out (the caller never has more than kApMaxParts - 1: its last part
// pushes nothing that is read)
__device__ __forceinline__ void ap_push(ApRanges &ex, int tf, int tl, double lo, double hi) {
#pragma unroll
    for (int i = kApMaxParts - 2; i > 0; --i) {
        ex.tf[i] = ex.tf[i - 1];
        ex.tl[i] = ex.tl[i - 1];
        ex.lo[i] = ex.lo[i - 1];
        ex.hi[i] = ex.hi[i - 1];
    }
    ex.tf[0] = tf;
    ex.tl[0] = tl;
    ex.lo[0] = lo;
    ex.hi[0] = hi;
}
__device__ __forceinline__ bool ap_t_free(const ApRanges &ex, int t) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kApMaxParts - 1; ++i) ok = ok && !(t >= ex.tf[i] && t <= ex.tl[i]);
    return ok;
}
__device__ __forceinline__ bool ap_c_free(const ApRanges &ex, double c) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kApMaxParts - 1; ++i) ok = ok && !(c >= ex.lo[i] && c <= ex.hi[i]);
    return ok;
}

// The parts' rule for al_bin_extremes: only the pairs whose t and c lie outside the ranges count
struct ApOutside {
    const ApRanges &ex;
    __device__ __forceinline__ bool key(double c) const { return ap_c_free(ex, c); }
    __device__ __forceinline__ bool index(int t) const { return ap_t_free(ex, t); }
};

// The best bin of one row at one rate, as the sweep finds it (al_sweep's window loop: see tvz_align_kernels.h for why
// the lane that makes a bin's last increment sees its final count, why the windows descend and what the resume
// positions are) -> count << 33 | (2^33 - 1 - order), reduced over the wave; 0: no pair votes.  kExcl: only the pairs
// whose t and c lie outside the ranges of `ex` vote - a key inside a range is skipped whole, an index inside one is
// walked over (the run's end is found by the expression, which does not know the ranges).  c_min / c_max: the row's
// smallest and largest key.  The histogram is clean on entry and on return.  m >= 1, len >= 1.
// kTwoBins (tvz_align_parts_flags with TVZ_ALIGN_TWO_BINS): the best WINDOW of two adjacent bins, as
// al_sweep<.., kTwoBins> finds it -> J << 33 | (2^33 - 1 - order of the lower bin).  The vote loop tracks nothing; the
// windows' counts are read in the pass over the touched list, where every count is final.  The count of the bin above a
// window's last slot is carried in one word, read from hist[0] before the clearing: it starts at 0 in every call - per
// rate, per part, per row - and under kExcl it is a count of ALLOWED votes, because only those reach the histogram.
template <bool kExcl, bool kTwoBins = false>
__device__ __forceinline__ unsigned long long ap_votes(const int64_t *__restrict__ rk, int len, const double *s, int m, double eps,
                                                       int32_t B, double c_min, double c_max, double rho, const AlWave &w,
                                                       const ApRanges &ex, int lane) {
    const double Bd = (double)B;
    const double x_min = al_x<true>(s, 0, rho), x_max = al_x<true>(s, m - 1, rho);     // the products stay sorted
    // the row's offset range [bin(c_min, x_max), bin(c_max, x_min)], clipped to [-B, B]; a NaN end clips to the bound
    const double d_lo = al_bin(c_min, x_max, eps), d_hi = al_bin(c_max, x_min, eps);
    const double r_lo = d_lo >= -Bd ? d_lo : -Bd, r_hi = d_hi <= Bd ? d_hi : Bd;
    int w0 = 0, w1 = -1;
    if (r_lo <= r_hi) {                                                   // -B <= r_lo <= r_hi <= B: both finite
        w0 = ((int)r_lo + B) / w.width;
        w1 = ((int)r_hi + B) / w.width;
    }
    w0 = __builtin_amdgcn_readfirstlane(w0);
    w1 = __builtin_amdgcn_readfirstlane(w1);
    w1 = w1 < w.max_windows - 1 ? w1 : w.max_windows - 1;
    unsigned long long best = 0;
    [[maybe_unused]] uint32_t jbest = 0;                                  // kTwoBins: the lane's best window (J, h << 33 | ..)
    [[maybe_unused]] uint32_t carry = 0;                                  // ... and the lowest bin's count of the window above
    for (int wi = w1; wi >= w0; --wi) {                                   // wave-uniform
        const int w_lo = wi * w.width - B;
        const int w_hi = w_lo + w.width - 1 < B ? w_lo + w.width - 1 : B;
        const double lo_d = (double)w_lo, hi_d = (double)w_hi;
        for (int j = lane; j < len; j += 64) {
            const double c = __longlong_as_double(rk[j]);
            const bool kept_pos = j < w.resume_keys;
            int t = kept_pos && wi != w1 ? (int)w.resume[j] : al_lo<true>(s, m, c, eps, hi_d, rho);
            const bool c_ok = !kExcl || ap_c_free(ex, c);
            for (; t < m; ++t) {
                const double d = al_bin(c, al_x<true>(s, t, rho), eps);
                if (!(d >= lo_d)) break;                                  // behind the window (or NaN there)
                if (!(d <= hi_d)) continue;                               // (never, behind al_lo: keeps the index in bounds)
                if (kExcl && !(c_ok && ap_t_free(ex, t))) continue;
                const int bin = (int)d;                                   // w_lo <= bin <= w_hi
                const uint32_t slot = (uint32_t)(bin - w_lo);             // 0 .. width - 1
                const uint32_t cnt = atomicAdd(&w.hist[slot], 1u) + 1u;
                if (cnt == 1u) w.dirty[atomicAdd(w.n_dirty, 1u)] = (uint16_t)slot;      // at most once per slot: < width
                if constexpr (!kTwoBins) {
                    const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                    const unsigned long long key = ((unsigned long long)cnt << 33) | (kAlOrderMask - order);
                    best = key > best ? key : best;
                }
            }
            if (kept_pos) w.resume[j] = (uint16_t)t;                      // t <= m <= 4095
        }
        wave_lds_fence();
        const int nd = (int)*w.n_dirty;
        if constexpr (kTwoBins) {
            // every count is final.  Slot + 1 inside the histogram is bin b + 1, the padding slot or a bin beyond B,
            // which no vote reaches (0); behind the last slot b + 1 is the lowest bin of the window above: the carry
            for (int i = lane; i < nd; i += 64) {
                const int slot = (int)w.dirty[i];                         // < width
                const uint32_t h = w.hist[slot];
                const uint32_t up = slot + 1 < w.width ? w.hist[slot + 1] : carry;
                const int bin = w_lo + slot;
                const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                const uint32_t j = h + up;
                const unsigned long long key = ((unsigned long long)h << 33) | (kAlOrderMask - order);
                const bool better = j > jbest || (j == jbest && key > best);
                jbest = better ? j : jbest;
                best = better ? key : best;
            }
            carry = w.hist[0];                                            // (the same word in every lane)
        }
        for (int i = lane; i < nd; i += 64) w.hist[w.dirty[i]] = 0;
        wave_lds_fence();
        if (lane == 0) *w.n_dirty = 0;
    }
    if constexpr (kTwoBins) {
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t oj = __shfl_xor(jbest, off);
            const unsigned long long o = __shfl_xor(best, off);
            const bool better = oj > jbest || (oj == jbest && o > best);
            jbest = better ? oj : jbest;
            best = better ? o : best;
        }
        best = ((unsigned long long)jbest << 33) | (best & kAlOrderMask);     // the window's count and its lower bin
    } else {
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
    }
    return best;
}

// grid = (row blocks, Q), any number of row blocks.  ids: the id of pair (q, j) is ids[q * query_id_stride + j *
// id_stride]; a negative id names no pair.  counts int32[Q][k], zeroed before the launch: += 1 per matching row, so
// it ends as n_rows; slots int64[Q][k][kApMaxRows]: the first kApMaxRows matching rows' indices, in no fixed order.
__global__ __launch_bounds__(kApLocateBlock) void ts_alignp_locate_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int32_t *__restrict__ ids, int64_t id_stride, int64_t query_id_stride,
    int32_t k, int32_t *__restrict__ counts, int64_t *__restrict__ slots) {
    __shared__ int32_t s_ids[kAlMaxK];
    const int q = blockIdx.y;
    if ((int)threadIdx.x < k) s_ids[threadIdx.x] = ids[(int64_t)q * query_id_stride + (int64_t)threadIdx.x * id_stride];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kApLocateBlock;
    for (int64_t r = (int64_t)blockIdx.x * kApLocateBlock + threadIdx.x; r < n_rows; r += stride) {
        const int32_t vid = load_row(rows + r).vid;
        if (vid < 0) continue;
        for (int j = 0; j < k; ++j) {                                     // the same LDS address in every lane: a broadcast
            if (s_ids[j] != vid) continue;
            const int64_t pair = (int64_t)q * k + j;
            const int32_t n = atomicAdd(&counts[pair], 1);
            if (n >= 0 && n < kApMaxRows) slots[pair * kApMaxRows + n] = r;
        }
    }
}

// grid = (k, Q), kAlBlock threads; dynamic LDS: aw_lds_bytes(lds_keys, B, width), width = aw_width(B).  Sorted query q:
// sv[at .. at + m), at = q_offsets[q] - q_offsets[0], m = qm[q] (ts_tol_sort_kernel).  A pair with a refused query, a
// negative id, no row or more than kApMaxRows rows is left to the pick.  Slot n of pair p writes scratch[(p *
// kApMaxRows + n) * ap_words(max_parts) ..): the header (video_id, row_len, rate_index, n_parts, 0, m) and per part
// (bin, votes, t_first, t_last, nq, nr) - part 0's row always (zeros without a vote: the pick orders the slots by its
// votes), a later part's only when it is reported.  1 <= max_parts <= kApMaxParts, min_votes >= 1, rates.n >= 1.
// kTwoBins (ts_alignp2_walk_kernel): every part is the best window of two adjacent bins - bin = the lower one, votes = J,
// the extremes and nq / nr over the pairs of both bins, the upper one only inside [-B, B].
template <bool kTwoBins>
__device__ __forceinline__ void ap_walk(
    const Row *__restrict__ rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B, int32_t width,
    const AlRates &rates, int32_t min_votes, int32_t max_parts, const int32_t *__restrict__ ids, int64_t id_stride,
    int64_t query_id_stride, int32_t k, const int32_t *__restrict__ counts, const int64_t *__restrict__ slots,
    int32_t *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int j = blockIdx.x, q = blockIdx.y;
    const int64_t pair = (int64_t)q * k + j;
    const int32_t m = qm[q];
    const int32_t id = ids[(int64_t)q * query_id_stride + (int64_t)j * id_stride];
    const int32_t n_slots = counts[pair];
    if (m < 0 || m > lds_keys || id < 0 || n_slots <= 0 || n_slots > kApMaxRows) return;     // block-uniform
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    double *s = reinterpret_cast<double *>(smem);
    const AlWave w = al_wave<true>(smem, lds_keys, B, width, wv);
    for (int e = threadIdx.x; e < m; e += kAlBlock) s[e] = sv[at + e];
    al_wave_clear(w, lane);
    __syncthreads();

    const int words = ap_words(max_parts);
    for (int slot = wv; slot < n_slots; slot += kAlWaves) {               // wave-uniform: no block barrier inside
        const Row row = load_row(rows + slots[pair * kApMaxRows + slot]);
        const int64_t *rk = keys + row.off;
        int32_t *o = scratch + (pair * kApMaxRows + slot) * words;
        const AlKeyRange kr = al_key_range(rk, row.len, lane);
        ApRanges ex = ap_no_ranges();
        unsigned long long best = 0;                                      // part 0: the kept rate's
        uint32_t best_rate = 0;
        if (m > 0 && row.len > 0) {
            for (int ri = 0; ri < rates.n; ++ri) {                        // wave-uniform
                const unsigned long long rbest =
                    ap_votes<false, kTwoBins>(rk, row.len, s, m, eps, B, kr.c_min, kr.c_max, rates.r[ri], w, ex, lane);
                if ((rbest >> 33) > (best >> 33)) {                       // strictly more votes: a tie keeps the smaller index
                    best = rbest;
                    best_rate = (uint32_t)ri;
                }
            }
        }
        const double rho = rates.r[best_rate];
        int32_t n_parts = 0;
        for (int p = 0; p < max_parts; ++p) {                             // wave-uniform
            if (p > 0) best = ap_votes<true, kTwoBins>(rk, row.len, s, m, eps, B, kr.c_min, kr.c_max, rho, w, ex, lane);
            const int32_t votes = (int32_t)(best >> 33);
            if (votes < min_votes && p > 0) break;
            int32_t part[kApCols] = {0, 0, 0, 0, 0, 0};
            if (votes > 0) {
                const int bin = al_best_bin(best);
                const AlExtremes x = al_bin_extremes<ApOutside, kTwoBins>(rk, row.len, s, m, eps, bin, rho, ApOutside{ex}, lane,
                                                                          bin < B ? bin + 1 : bin);
                int32_t nq = 0, nr = 0;
                for (int t = x.t_first + lane; t <= x.t_last; t += 64) nq += ap_t_free(ex, t) ? 1 : 0;
                for (int i = lane; i < row.len; i += 64) {
                    const double c = __longlong_as_double(rk[i]);
                    nr += c >= x.c_lo && c <= x.c_hi && ap_c_free(ex, c) ? 1 : 0;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    nq += __shfl_xor(nq, off);
                    nr += __shfl_xor(nr, off);
                }
                part[0] = bin;
                part[1] = votes;
                part[2] = x.t_first;
                part[3] = x.t_last;
                part[4] = nq;
                part[5] = nr;
                ap_push(ex, x.t_first, x.t_last, x.c_lo, x.c_hi);
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kApCols; ++i) o[(1 + p) * kApCols + i] = part[i];
            }
            if (votes < min_votes) break;                                 // part 0 below the bar: written, not reported
            n_parts = p + 1;
        }
        if (lane == 0) {
            o[0] = row.vid;
            o[1] = row.len;
            o[2] = (int32_t)best_rate;
            o[3] = n_parts;
            o[4] = 0;
            o[5] = m;
        }
    }
}

// The single-bin walk keeps a body of its own, word for word ap_walk<false>: forwarding it to the template moved its
// machine code (9,348 -> 9,296 bytes, 95 -> 93 SGPRs, by value or by reference alike), as moving ap_votes and al_sweep
// into one function did.  A change of the walk is made in both.
__global__ __launch_bounds__(kAlBlock) void ts_alignp_walk_kernel(
    const Row *__restrict__ rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B, int32_t width,
    AlRates rates, int32_t min_votes, int32_t max_parts, const int32_t *__restrict__ ids, int64_t id_stride,
    int64_t query_id_stride, int32_t k, const int32_t *__restrict__ counts, const int64_t *__restrict__ slots,
    int32_t *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int j = blockIdx.x, q = blockIdx.y;
    const int64_t pair = (int64_t)q * k + j;
    const int32_t m = qm[q];
    const int32_t id = ids[(int64_t)q * query_id_stride + (int64_t)j * id_stride];
    const int32_t n_slots = counts[pair];
    if (m < 0 || m > lds_keys || id < 0 || n_slots <= 0 || n_slots > kApMaxRows) return;     // block-uniform
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    double *s = reinterpret_cast<double *>(smem);
    const AlWave w = al_wave<true>(smem, lds_keys, B, width, wv);
    for (int e = threadIdx.x; e < m; e += kAlBlock) s[e] = sv[at + e];
    al_wave_clear(w, lane);
    __syncthreads();

    const int words = ap_words(max_parts);
    for (int slot = wv; slot < n_slots; slot += kAlWaves) {               // wave-uniform: no block barrier inside
        const Row row = load_row(rows + slots[pair * kApMaxRows + slot]);
        const int64_t *rk = keys + row.off;
        int32_t *o = scratch + (pair * kApMaxRows + slot) * words;
        const AlKeyRange kr = al_key_range(rk, row.len, lane);
        ApRanges ex = ap_no_ranges();
        unsigned long long best = 0;                                      // part 0: the kept rate's
        uint32_t best_rate = 0;
        if (m > 0 && row.len > 0) {
            for (int ri = 0; ri < rates.n; ++ri) {                        // wave-uniform
                const unsigned long long rbest =
                    ap_votes<false>(rk, row.len, s, m, eps, B, kr.c_min, kr.c_max, rates.r[ri], w, ex, lane);
                if ((rbest >> 33) > (best >> 33)) {                       // strictly more votes: a tie keeps the smaller index
                    best = rbest;
                    best_rate = (uint32_t)ri;
                }
            }
        }
        const double rho = rates.r[best_rate];
        int32_t n_parts = 0;
        for (int p = 0; p < max_parts; ++p) {                             // wave-uniform
            if (p > 0) best = ap_votes<true>(rk, row.len, s, m, eps, B, kr.c_min, kr.c_max, rho, w, ex, lane);
            const int32_t votes = (int32_t)(best >> 33);
            if (votes < min_votes && p > 0) break;
            int32_t part[kApCols] = {0, 0, 0, 0, 0, 0};
            if (votes > 0) {
                const int bin = al_best_bin(best);
                const AlExtremes x = al_bin_extremes(rk, row.len, s, m, eps, bin, rho, ApOutside{ex}, lane);
                int32_t nq = 0, nr = 0;
                for (int t = x.t_first + lane; t <= x.t_last; t += 64) nq += ap_t_free(ex, t) ? 1 : 0;
                for (int i = lane; i < row.len; i += 64) {
                    const double c = __longlong_as_double(rk[i]);
                    nr += c >= x.c_lo && c <= x.c_hi && ap_c_free(ex, c) ? 1 : 0;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    nq += __shfl_xor(nq, off);
                    nr += __shfl_xor(nr, off);
                }
                part[0] = bin;
                part[1] = votes;
                part[2] = x.t_first;
                part[3] = x.t_last;
                part[4] = nq;
                part[5] = nr;
                ap_push(ex, x.t_first, x.t_last, x.c_lo, x.c_hi);
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kApCols; ++i) o[(1 + p) * kApCols + i] = part[i];
            }
            if (votes < min_votes) break;                                 // part 0 below the bar: written, not reported
            n_parts = p + 1;
        }
        if (lane == 0) {
            o[0] = row.vid;
            o[1] = row.len;
            o[2] = (int32_t)best_rate;
            o[3] = n_parts;
            o[4] = 0;
            o[5] = m;
        }
    }
}

// TVZ_ALIGN_TWO_BINS (tvz_align_parts_flags): a kernel of its own, the same argument list
__global__ __launch_bounds__(kAlBlock) void ts_alignp2_walk_kernel(
    const Row *__restrict__ rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B, int32_t width,
    AlRates rates, int32_t min_votes, int32_t max_parts, const int32_t *__restrict__ ids, int64_t id_stride,
    int64_t query_id_stride, int32_t k, const int32_t *__restrict__ counts, const int64_t *__restrict__ slots,
    int32_t *__restrict__ scratch) {
    ap_walk<true>(rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, rates, min_votes, max_parts, ids, id_stride,
                  query_id_stride, k, counts, slots, scratch);
}

// grid = ceil(Q * k / kApPickWaves), a wave per pair -> d_parts int32[Q][k][1 + max_parts][6].  Row 0 is (video_id,
// row_len, rate_index, n_parts, n_rows, m), the part rows follow, zeros behind n_parts.  A negative id: (-1, 0, 0, 0,
// 0, m).  No row of that id: (id, 0, 0, 0, 0, m).  Refused - a query the preparation refused (m reads 0 then), or
// more than kApMaxRows rows of the id -: (id, 0, 0, INT32_MIN, n_rows, m).
__global__ __launch_bounds__(kApPickBlock) void ts_alignp_pick_kernel(
    const int32_t *__restrict__ ids, int64_t id_stride, int64_t query_id_stride, int32_t Q, int32_t k, int32_t max_parts,
    const int32_t *__restrict__ qm, int32_t lds_keys, const int32_t *__restrict__ counts, const int64_t *__restrict__ slots,
    const int32_t *__restrict__ scratch, int32_t *__restrict__ d_parts) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * kApPickWaves + (threadIdx.x >> 6);
    if (pair >= (int64_t)Q * k) return;                                   // wave-uniform
    const int q = (int)(pair / k), j = (int)(pair % k);
    const int words = ap_words(max_parts);                                // <= 30: a lane per word
    const int32_t id = ids[(int64_t)q * query_id_stride + (int64_t)j * id_stride];
    const int32_t qmv = qm[q];
    const bool bad_query = qmv < 0 || qmv > lds_keys;
    const int32_t m = bad_query ? 0 : qmv;
    const int32_t n_rows = id < 0 ? 0 : counts[pair];
    int32_t *out = d_parts + pair * words;
    if (id < 0 || bad_query || n_rows <= 0 || n_rows > kApMaxRows) {
        const bool refused = id >= 0 && (bad_query || n_rows > kApMaxRows);
        int32_t v = 0;
        v = lane == 0 ? (id < 0 ? -1 : id) : v;
        v = lane == 3 && refused ? INT32_MIN : v;
        v = lane == 4 ? n_rows : v;
        v = lane == 5 ? m : v;
        if (lane < words) out[lane] = v;
        return;
    }
    // the winner: most part-0 votes, then the earlier row of the table; lanes without a slot lose to every slot
    const bool has = lane < n_rows;
    int32_t votes = has ? scratch[(pair * kApMaxRows + lane) * words + kApCols + 1] : -1;
    int64_t row = has ? slots[pair * kApMaxRows + lane] : INT64_MAX;
    int slot = lane;
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t ov = __shfl_xor(votes, off);
        const int64_t orow = __shfl_xor(row, off);
        const int os = __shfl_xor(slot, off);
        const bool take = ov > votes || (ov == votes && orow < row);
        votes = take ? ov : votes;
        row = take ? orow : row;
        slot = take ? os : slot;
    }
    const int32_t *src = scratch + (pair * kApMaxRows + slot) * words;
    const int32_t n_parts = src[3];
    if (lane < words) {
        int32_t v = src[lane];
        v = lane == 4 ? n_rows : v;
        v = lane == 5 ? m : v;
        v = lane >= kApCols && lane / kApCols - 1 >= n_parts ? 0 : v;
        out[lane] = v;
    }
}

// The shards' answers to ONE tvz_align_parts call -> one answer (tvz_align_parts_merge, include/tvz.h).  grid =
// ceil(Q * k / kApMergeGroups), a 16-lane group per pair, lane = list: gathered int32[n_lists][pairs][words] -> d_parts
// int32[pairs][words], words = ap_words(max_parts).  Per pair the winner is, among the lists whose n_rows > 0, the one
// with the most part-0 votes, the lower list on a tie, and list 0 where no list holds a row: one signed 64-bit key per
// lane, (votes + 1 or 0) * 16 + (15 - list), and its maximum over the group (lanes without a list hold the smallest
// key).  n_rows is summed in 64 bits and saturates; one refused list refuses the pair.  A block is words x 4 bytes, 48
// to 120: every access is one 32-bit word.  1 <= n_lists <= 16, 1 <= max_parts <= kApMaxParts.
constexpr int kApMergeBlock = 256;
constexpr int kApMergeGroups = kApMergeBlock / 16;     // pairs per block: a group each
__global__ __launch_bounds__(kApMergeBlock) void ts_alignp_merge_kernel(const int32_t *__restrict__ gathered, int32_t n_lists,
                                                                        int64_t pairs, int32_t max_parts,
                                                                        int32_t *__restrict__ d_parts) {
    const int list = threadIdx.x & 15;
    const int64_t pair = (int64_t)blockIdx.x * kApMergeGroups + (threadIdx.x >> 4);
    if (pair >= pairs) return;                                            // group-uniform: the moves below stay inside a group
    const int words = ap_words(max_parts);                                // <= 30: two words per lane
    const bool has_list = list < n_lists;
    const int32_t *mine = gathered + ((int64_t)(has_list ? list : 0) * pairs + pair) * words;
    const int32_t n_rows = has_list ? mine[4] : 0;
    const int32_t votes = has_list ? mine[kApCols + 1] : 0;
    const uint32_t is_refused = has_list && mine[3] == INT32_MIN ? 1u : 0u;
    long long key = has_list ? (n_rows > 0 ? (long long)votes + 1 : 0ll) * 16 + (15 - list) : INT64_MIN;
    long long total = n_rows;
#define TVZ_AP_MERGE_STEP(C) { const long long ok = (long long)dpp16_64<C>((unsigned long long)key); \
    key = ok > key ? ok : key; total += (long long)dpp16_64<C>((unsigned long long)total); }
    TVZ_ROW16_BUTTERFLY(TVZ_AP_MERGE_STEP)
#undef TVZ_AP_MERGE_STEP
    const bool refused = group16_sum<uint32_t>(is_refused) != 0u;
    const int winner = 15 - (int)(key & 15);                              // (the low four bits, whatever the key's sign)
    const int32_t n_sum = total > (long long)INT32_MAX ? INT32_MAX : (int32_t)total;
    const int32_t *src = gathered + ((int64_t)winner * pairs + pair) * words;
    int32_t *out = d_parts + pair * words;
    for (int w = list; w < words; w += 16) {
        int32_t v = src[w];
        v = refused && w != 0 && w != 5 ? 0 : v;                          // a refused pair keeps the winner's id and m
        v = refused && w == 3 ? INT32_MIN : v;
        v = w == 4 ? n_sum : v;
        out[w] = v;
    }
}

}  // namespace
