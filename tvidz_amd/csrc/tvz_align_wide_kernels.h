// tvz_align_wide_kernels.h — the alignment top-k over up to 2^22 offset bins on either side of zero
// (tvz_align_wide_topk), gfx950 wave64.  Included by tvz_match.hip only.  From tvz_align_kernels.h: the vote's
// expression (al_bin), the start of a key's voting run (al_lo / al_left) and the sweep's block shape.
//
// Contract (include/tvz.h): votes, bins and the best bin are tvz_align_topk's, with B up to kAwMaxB; the score is
// the tolerant Jaccard or, with TVZ_ALIGN_CONTAIN, v / min(nv, row_len); a row's hit is ordered by the tuple
// (score descending, video_id, best_bin, row_len, votes).
//
// The window walk: a wave's histogram holds `width` bins (aw_width: all 2B + 1 of them while they fit kAwOneWindow, so
// a call with B <= 2047 is ONE window and does the bounded sweep's work; kAwWidth beyond).  Window w of the global grid covers the bins
// [w * width - B, w * width - B + width - 1], clipped to B.  A row's pairs can only vote inside
// [bin(c_min, x_max), bin(c_max, x_min)] - every step of the vote's expression is monotone in c and in x - so only
// the windows that meet that range (clipped to [-B, B]) are visited, from the highest down.  Per window every key's
// voting run is found by al_lo with the WINDOW's upper bin as the bound (the vote's own expression, never a
// comparison on x), and walked until the expression falls below the window's lower bin: all votes of one bin fall
// into one window, so the lane that makes a bin's last increment sees its final count there, and the lane-wise best
//   count << 33 | (2^33 - 1 - order),   order = 2 |bin| + (bin > 0) on the GLOBAL bin
// carries the tie rule across windows.  Between windows the histogram is cleared through the touched list.
//
// The resume position: a key's runs move to larger x as the windows descend, and the position where a window's walk
// stops - the first value whose bin lies below the window - is al_lo's answer for the next window (whose upper bin is
// this one's lower bin - 1; a walk that stops at a NaN has met a key that never votes).  So only a row's highest
// window searches; the later ones read the position back, for the row's first kAwResume keys (a u16 per key and
// wave in LDS, written and read by the same lane); keys beyond them search in every window.
//
// ts_alignw_sweep_kernel    grid = (row blocks, Q): a wave per row, as ts_align_topk_kernel.  A kept hit is three
//                           words, one per lane: (2^20 - score) << 31 | video_id, (best_bin + 2^22) << 32 | row_len,
//                           and the raw votes (32 bits).
// ts_alignw_reduce_kernel   one block per query: the k smallest of the blocks' lists -> d_out[q].
#pragma once
#include "tvz_align_kernels.h"

namespace {

constexpr int kAwMaxB = 1 << 22;                       // TVZ_ALIGN_WIDE_MAX_B
constexpr int kAwOneWindow = 4096;                     // a call of at most this many bins is one window: the bounded sweep's shape
constexpr int kAwWidth = 1024;                         // bins of a window otherwise (measured against 256..4096)
constexpr int kAwResume = 512;                         // keys of a row whose resume position is kept (a multiple of 64)
constexpr uint32_t kAwContain = 1u;                    // TVZ_ALIGN_CONTAIN
constexpr int kAwStaticLds = kAlWaves * 64 * 20 + 64;  // the waves' lists at the block's end + a few words
constexpr unsigned long long kAwOrderMask = (1ull << 33) - 1;

// bins of a wave's histogram (even: the touched list behind the histograms stays 4-byte aligned)
__host__ __device__ inline int aw_width(int32_t B) { return al_bins_padded(B) <= kAwOneWindow ? al_bins_padded(B) : kAwWidth; }
// the most windows a row can take: ceil((2B + 1) / width)
__host__ __device__ inline int aw_max_windows(int32_t B, int width) { return (2 * B + width) / width; }
// dynamic LDS of the sweep: the sorted query, then per wave a histogram (u32 per bin), the touched bins (u16 per
// bin), their count and the resume positions (u16 per key; none where the call has one window)
__host__ __device__ inline int aw_resume_keys(int32_t B, int width) { return aw_max_windows(B, width) > 1 ? kAwResume : 0; }
inline size_t aw_lds_bytes(int32_t lds_keys, int32_t B, int width) {
    return (size_t)lds_keys * 8 + (size_t)kAlWaves * ((size_t)width * 6 + 4 + (size_t)aw_resume_keys(B, width) * 2);
}

// (word, payload, votes) order of the kept lists
__device__ __forceinline__ bool aw_le(unsigned long long w1, unsigned long long p1, uint32_t v1, unsigned long long w2,
                                      unsigned long long p2, uint32_t v2) {
    return w1 < w2 || (w1 == w2 && (p1 < p2 || (p1 == p2 && v1 <= v2)));
}

// al_insert for the three-word entries: lane i holds the wave's i-th best hit, kAlPad words behind them
__device__ __forceinline__ bool aw_insert(unsigned long long &kw, unsigned long long &kp, uint32_t &kv, unsigned long long w,
                                          unsigned long long p, uint32_t v, int k, int lane) {
    const int pos = __popcll(__ballot(aw_le(kw, kp, kv, w, p, v)));  // the kept hits that stay in front: a prefix
    if (pos >= k) return false;
    const unsigned long long uw = __shfl_up(kw, 1), up = __shfl_up(kp, 1);
    const uint32_t uv = __shfl_up(kv, 1);
    if (lane > pos) {
        kw = uw;
        kp = up;
        kv = uv;
    }
    if (lane == pos) {
        kw = w;
        kp = p;
        kv = v;
    }
    if (lane >= k) {
        kw = kp = kAlPad;
        kv = ~0u;
    }
    return true;
}

// ... and a whole sorted list held one entry per lane: entry e is offered until one is refused
__device__ __forceinline__ void aw_take(unsigned long long &kw, unsigned long long &kp, uint32_t &kv, unsigned long long ew,
                                        unsigned long long ep, uint32_t ev, int k, int lane) {
    for (int e = 0; e < k; ++e) {                                    // wave-uniform
        const unsigned long long w = __shfl(ew, e), p = __shfl(ep, e);
        const uint32_t v = __shfl(ev, e);
        if (w == kAlPad || !aw_insert(kw, kp, kv, w, p, v, k, lane)) break;
    }
}

// grid = (row blocks, Q).  Sorted query q: sv[at .. at + m) with at = q_offsets[q] - q_offsets[0], m = qm[q]
// (ts_tol_sort_kernel).  part_w / part_p: uint64[Q][n_lists][k], part_v: uint32[Q][n_lists][k], block bx writes list
// bx; totals[q] (zeroed by the preparation) += the block's hits, one atomic.  width = aw_width(B); dynamic LDS:
// aw_lds_bytes(lds_keys, B, width).  0 <= B <= kAwMaxB (the host refuses anything else before the launch).
__global__ __launch_bounds__(kAlBlock) void ts_alignw_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, int32_t min_votes, int32_t min_score, uint32_t flags, const int32_t *__restrict__ exclude_ids,
    int32_t k, unsigned long long *__restrict__ part_w, unsigned long long *__restrict__ part_p,
    uint32_t *__restrict__ part_v, int32_t n_lists, int32_t *__restrict__ totals) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long s_w[kAlWaves * 64], s_p[kAlWaves * 64];
    __shared__ uint32_t s_v[kAlWaves * 64];
    __shared__ int32_t s_nhits;
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    const int32_t m = qm[q];
    if (m <= 0 || m > lds_keys) return;       // empty: no hit; refused by the preparation: the selection flags it
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    double *s = reinterpret_cast<double *>(smem);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem + (size_t)lds_keys * 8) + (size_t)wv * width;
    uint16_t *dirty = reinterpret_cast<uint16_t *>(smem + (size_t)lds_keys * 8 + (size_t)kAlWaves * width * 4) + (size_t)wv * width;
    uint32_t *n_dirty = reinterpret_cast<uint32_t *>(smem + (size_t)lds_keys * 8 + (size_t)kAlWaves * width * 6) + wv;
    uint16_t *resume = reinterpret_cast<uint16_t *>(smem + (size_t)lds_keys * 8 + (size_t)kAlWaves * ((size_t)width * 6 + 4)) +
                       (size_t)wv * aw_resume_keys(B, width);
    for (int e = threadIdx.x; e < m; e += kAlBlock) s[e] = sv[at + e];
    for (int b = lane; b < width; b += 64) hist[b] = 0;
    if (lane == 0) *n_dirty = 0;
    if (threadIdx.x == 0) s_nhits = 0;
    __syncthreads();

    const double Bd = (double)B;
    const double x_min = s[0], x_max = s[m - 1];                             // sorted numerically, no NaN
    const int max_windows = aw_max_windows(B, width);
    const int resume_keys = aw_resume_keys(B, width);
    const bool contain = (flags & kAwContain) != 0u;
    const int32_t excl = exclude_ids ? exclude_ids[q] : -1;
    const int64_t stride = (int64_t)gridDim.x * kAlWaves;
    const int64_t last_row = n_rows - 1;
    unsigned long long kw = kAlPad, kp = kAlPad;
    uint32_t kv = ~0u;
    int32_t n_hits = 0;
    int64_t r = (int64_t)bx * kAlWaves + wv;
    Row row = load_row(rows + (r < n_rows ? r : last_row));
    while (r < n_rows) {                      // wave-uniform: no block barrier inside
        const int64_t rn = r + stride;
        const Row nrow = load_row(rows + (rn < n_rows ? rn : last_row));      // lands while this row votes
        const int64_t *rk = keys + row.off;
        // the row's offset range [bin(c_min, x_max), bin(c_max, x_min)], clipped to [-B, B]; a NaN end (inf - inf)
        // clips to the bound
        double c_min = __longlong_as_double(0x7ff0000000000000ll), c_max = -c_min;
        for (int j = lane; j < row.len; j += 64) {
            const double c = __longlong_as_double(rk[j]);
            c_min = c < c_min ? c : c_min;
            c_max = c > c_max ? c : c_max;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double lo = __shfl_xor(c_min, off), hi = __shfl_xor(c_max, off);
            c_min = lo < c_min ? lo : c_min;
            c_max = hi > c_max ? hi : c_max;
        }
        const double d_lo = al_bin(c_min, x_max, eps), d_hi = al_bin(c_max, x_min, eps);
        const double r_lo = d_lo >= -Bd ? d_lo : -Bd, r_hi = d_hi <= Bd ? d_hi : Bd;
        int w0 = 0, w1 = -1;                                                  // no window: an empty row, a range outside
        if (row.len > 0 && r_lo <= r_hi) {                                    // -B <= r_lo <= r_hi <= B: both finite
            w0 = ((int)r_lo + B) / width;
            w1 = ((int)r_hi + B) / width;
        }
        w0 = __builtin_amdgcn_readfirstlane(w0);                              // (equal in every lane already)
        w1 = __builtin_amdgcn_readfirstlane(w1);
        w1 = w1 < max_windows - 1 ? w1 : max_windows - 1;                     // (never: (2B) / width is the last window)
        unsigned long long best = 0;
        for (int w = w1; w >= w0; --w) {                                      // wave-uniform, at most max_windows rounds
            const int w_lo = w * width - B;                                   // >= -B
            const int w_hi = w_lo + width - 1 < B ? w_lo + width - 1 : B;
            const double lo_d = (double)w_lo, hi_d = (double)w_hi;
            for (int j = lane; j < row.len; j += 64) {
                const double c = __longlong_as_double(rk[j]);
                const bool kept = j < resume_keys;                            // (the same in every lane of a round)
                int t = w == w1 || !kept ? al_lo(s, m, c, eps, hi_d) : (int)resume[j];
                for (; t < m; ++t) {
                    const double d = al_bin(c, s[t], eps);
                    if (!(d >= lo_d)) break;                                  // behind the window (or NaN there)
                    if (!(d <= hi_d)) continue;                               // (never, behind al_lo: keeps the index in bounds)
                    const int bin = (int)d;                                   // w_lo <= bin <= w_hi
                    const uint32_t slot = (uint32_t)(bin - w_lo);             // 0 .. width - 1
                    const uint32_t cnt = atomicAdd(&hist[slot], 1u) + 1u;
                    if (cnt == 1u) dirty[atomicAdd(n_dirty, 1u)] = (uint16_t)slot;      // at most once per slot: < width
                    const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                    const unsigned long long key = ((unsigned long long)cnt << 33) | (kAwOrderMask - order);
                    best = key > best ? key : best;
                }
                if (kept) resume[j] = (uint16_t)t;                            // t <= m <= 4095
            }
            // LDS ops of one wave complete in order: the notes above are visible to the clearing below
            wave_lds_fence();
            const int nd = (int)*n_dirty;
            for (int i = lane; i < nd; i += 64) hist[dirty[i]] = 0;
            wave_lds_fence();
            if (lane == 0) *n_dirty = 0;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        const uint32_t votes = (uint32_t)(best >> 33);
        const uint32_t rl = (uint32_t)row.len;
        uint32_t v = votes < (uint32_t)m ? votes : (uint32_t)m;
        v = v < rl ? v : rl;
        if (v >= (uint32_t)min_votes && row.vid != excl) {                  // min_votes >= 1: v >= 1, so m, rl, u >= 1
            const uint32_t u = contain ? ((uint32_t)m < rl ? (uint32_t)m : rl) : (uint32_t)m + rl - v;
            const uint32_t score = (v << 20) / u;                           // v <= 4095: the shift fits 32 bits; v <= u
            if (score >= (uint32_t)min_score) {
                const uint32_t order = (uint32_t)(kAwOrderMask - (best & kAwOrderMask));
                const int mag = (int)(order >> 1);
                const int bin = (order & 1u) ? mag : -mag;
                ++n_hits;
                aw_insert(kw, kp, kv,
                          ((unsigned long long)(kAlScoreOne - score) << 31) | (unsigned long long)((uint32_t)row.vid & 0x7fffffffu),
                          ((unsigned long long)(uint32_t)(bin + kAwMaxB) << 32) | rl, votes, k, lane);
            }
        }
        row = nrow;
        r = rn;
    }
    s_w[wv * 64 + lane] = kw;
    s_p[wv * 64 + lane] = kp;
    s_v[wv * 64 + lane] = kv;
    if (lane == 0 && n_hits) atomicAdd(&s_nhits, n_hits);                    // LDS
    __syncthreads();
    if (wv == 0) {
#pragma unroll 1
        for (int j = 1; j < kAlWaves; ++j) aw_take(kw, kp, kv, s_w[j * 64 + lane], s_p[j * 64 + lane], s_v[j * 64 + lane], k, lane);
        if (lane < k) {
            const int64_t o = ((int64_t)q * n_lists + bx) * k + lane;
            part_w[o] = kw;
            part_p[o] = kp;
            part_v[o] = kv;
        }
    }
    if (threadIdx.x == 0 && s_nhits) atomicAdd(&totals[q], s_nhits);
}

// One block per query: the k smallest (word, payload, votes) of its n_lists sorted partial lists -> d_out[q] =
// int32[k+1][4], as ts_align_topk_reduce_kernel writes it: k rows (video_id, row_len, best_bin, votes), padding
// (-1, 0, 0, 0), then (-1, n_hits, 0, 0).  A query the preparation refused (qm < 0 or > lds_keys): all padding,
// n_hits = INT32_MIN.
__global__ __launch_bounds__(kAlReduceBlock) void ts_alignw_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p,
    const uint32_t *__restrict__ part_v, int32_t n_lists, int32_t k, const int32_t *__restrict__ qm, int32_t lds_keys,
    const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    __shared__ unsigned long long s_w[kAlReduceWaves * 64], s_p[kAlReduceWaves * 64];
    __shared__ uint32_t s_v[kAlReduceWaves * 64];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int32_t m = qm[q];
    const bool refused = m < 0 || m > lds_keys;
    unsigned long long kw = kAlPad, kp = kAlPad;
    uint32_t kv = ~0u;
    if (!refused && m > 0) {                                                 // (an empty query's lists were never written)
        const int64_t base = (int64_t)q * n_lists;
        for (int l0 = wv; l0 < n_lists; l0 += kAlReduceLd * kAlReduceWaves) {   // wave-uniform
            unsigned long long ew[kAlReduceLd], ep[kAlReduceLd];
            uint32_t ev[kAlReduceLd];
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {
                const int l = l0 + j * kAlReduceWaves;
                const bool live = l < n_lists && lane < k;
                ew[j] = live ? part_w[(base + l) * k + lane] : kAlPad;
                ep[j] = live ? part_p[(base + l) * k + lane] : kAlPad;
                ev[j] = live ? part_v[(base + l) * k + lane] : ~0u;
            }
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) aw_take(kw, kp, kv, ew[j], ep[j], ev[j], k, lane);
        }
    }
    s_w[wv * 64 + lane] = kw;
    s_p[wv * 64 + lane] = kp;
    s_v[wv * 64 + lane] = kv;
    __syncthreads();
    if (wv != 0) return;
#pragma unroll 1
    for (int j = 1; j < kAlReduceWaves; ++j) aw_take(kw, kp, kv, s_w[j * 64 + lane], s_p[j * 64 + lane], s_v[j * 64 + lane], k, lane);
    int32_t *out = d_out + (int64_t)q * (k + 1) * 4;
    if (lane < k) {
        const bool pad = kw == kAlPad;
        out[lane * 4 + 0] = pad ? -1 : (int32_t)(kw & 0x7fffffffu);
        out[lane * 4 + 1] = pad ? 0 : (int32_t)(kp & 0xffffffffu);
        out[lane * 4 + 2] = pad ? 0 : (int32_t)(kp >> 32) - kAwMaxB;
        out[lane * 4 + 3] = pad ? 0 : (int32_t)kv;
    }
    if (lane == 0) {
        out[k * 4 + 0] = -1;
        out[k * 4 + 1] = refused ? INT32_MIN : totals[q];
        out[k * 4 + 2] = 0;
        out[k * 4 + 3] = 0;
    }
}

}  // namespace
