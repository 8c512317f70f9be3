// tvz_align_kernels.h — batched alignment score with the k best rows kept inside the sweep (tvz_align_topk),
// gfx950 wave64.  Included by tvz_match.hip only.  From tvz_match_kernels.h: Row, load_row; from tvz_tol_kernels.h:
// ts_tol_sort_kernel (the batch's queries sorted numerically, NaNs dropped, qm = the non-NaN count) and the
// sweep's block count (tol_topk_max_blocks); from tvz_wave.h: wave_lds_fence.
//
// Contract (include/tvz.h): votes and bins are tvz_align's - the pair (row key c, query value x) votes into
//   d = floor((c - x) / eps + 0.5)      (one IEEE subtraction, one true division)
// when -B <= d <= B - and a row's hit is ordered by the word (2^20 - score) << 43 | video_id << 12 | bin + 2048,
// then by (row_len, votes).
//
// The window: for a fixed key c each of c - x, / eps, + 0.5 and floor never increases as x grows, so the query
// values that vote are ONE contiguous run of the sorted query.  Its start is found by a binary search with the
// vote's own expression (al_left below; never a rewrite such as x >= c - max_offset, which rounds differently);
// from there the run is walked, voting, until the expression itself says the run has ended.  A NaN (inf - inf, or
// inf / inf with an infinite eps) is outside the window on the side its x lies on.
//
// ts_align_topk_kernel         grid = (row blocks, Q): a wave per row.  Per wave a histogram sized by the call's
//                              bin count, and a list of the bins it has touched.  A vote is a returning LDS add;
//                              every lane keeps the largest (count << 14 | 16383 - order) it has seen - the lane
//                              that makes a bin's last increment sees its final count, so the wave's maximum is
//                              the best bin under the tie rule with no scan of the histogram - and the lane that
//                              finds a bin at zero notes it, so clearing costs the bins touched, not 2B + 1.
//                              The wave's k best hits live in registers, one (word, payload) per lane, ascending:
//                              a hit below the k-th is inserted by one ballot and one lane shift.
// ts_align_topk_reduce_kernel  one block per query: the k smallest of the blocks' lists -> d_out[q].
#pragma once
#include "tvz_match_kernels.h"
#include "tvz_tol_kernels.h"
#include "tvz_wave.h"

namespace {

constexpr int kAlBlock = 256;
constexpr int kAlWaves = kAlBlock / 64;                // rows in flight per block
constexpr int kAlMaxK = 64;                            // one kept hit per lane
constexpr int kAlMaxLen = 4095;                        // v << 20 fits 32 bits; the sorted query fits LDS
constexpr int kAlScoreOne = 1 << 20;
constexpr int kAlStaticLds = kAlWaves * 64 * 16 + 64;  // the waves' lists at the block's end + a few words
constexpr int kAlReduceBlock = 1024;
constexpr int kAlReduceWaves = kAlReduceBlock / 64;
constexpr int kAlReduceLd = 4;                         // lists a wave loads per step (their loads in flight together)
constexpr unsigned long long kAlPad = ~0ull;           // no word is all ones: its top field is at most 2^20

// dynamic LDS of the sweep: the sorted query, then per wave a histogram (u32 per bin), the touched bins (u16 per
// bin) and their count
__host__ __device__ inline int al_bins_padded(int32_t B) { return (2 * B + 1 + 1) & ~1; }
inline size_t al_lds_bytes(int32_t lds_keys, int32_t B) {
    return (size_t)lds_keys * 8 + (size_t)kAlWaves * ((size_t)al_bins_padded(B) * 6 + 4);
}

// d of the contract, verbatim
__device__ __forceinline__ double al_bin(double c, double x, double eps) { return floor((c - x) / eps + 0.5); }

// is x in front of key c's window?  d > B; a NaN d counts by the side x lies on (x == c only for two equal
// infinities: -inf is the smallest query value, +inf the largest)
__device__ __forceinline__ bool al_left(double c, double x, double eps, double Bd) {
    const double d = al_bin(c, x, eps);
    return d > Bd || (d != d && (x < c || (x == c && x < 0.0)));
}

// first t with s[t] not in front of the window: a prefix of the sorted query
__device__ __forceinline__ int al_lo(const double *s, int m, double c, double eps, double Bd) {
    int lo = 0, len = m;
    while (len > 0) {
        const int half = len >> 1;
        if (al_left(c, s[lo + half], eps, Bd)) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// (word, payload) order of the kept lists
__device__ __forceinline__ bool al_le(unsigned long long w1, unsigned long long p1, unsigned long long w2,
                                      unsigned long long p2) {
    return w1 < w2 || (w1 == w2 && p1 <= p2);
}

// One wave's list: lane i holds its i-th best hit (ascending, kAlPad behind them and from lane k on).  The wave
// takes one more hit (wave-uniform w, p): false when it does not come before the k-th.  Equal hits are all kept.
__device__ __forceinline__ bool al_insert(unsigned long long &kw, unsigned long long &kp, unsigned long long w,
                                          unsigned long long p, int k, int lane) {
    const int pos = __popcll(__ballot(al_le(kw, kp, w, p)));       // the kept hits that stay in front: a prefix
    if (pos >= k) return false;
    const unsigned long long uw = __shfl_up(kw, 1), up = __shfl_up(kp, 1);
    if (lane > pos) {
        kw = uw;
        kp = up;
    }
    if (lane == pos) {
        kw = w;
        kp = p;
    }
    if (lane >= k) kw = kp = kAlPad;
    return true;
}

// ... and a whole sorted list held one entry per lane (ew, ep): entry e is offered until one is refused
__device__ __forceinline__ void al_take(unsigned long long &kw, unsigned long long &kp, unsigned long long ew,
                                        unsigned long long ep, int k, int lane) {
    for (int e = 0; e < k; ++e) {                                  // wave-uniform
        const unsigned long long w = __shfl(ew, e), p = __shfl(ep, e);
        if (w == kAlPad || !al_insert(kw, kp, w, p, k, lane)) break;
    }
}

__device__ __forceinline__ unsigned long long al_word(uint32_t score, int32_t vid, int bin) {
    return ((unsigned long long)(kAlScoreOne - score) << 43) | ((unsigned long long)((uint32_t)vid & 0x7fffffffu) << 12) |
           (unsigned long long)(uint32_t)(bin + 2048);
}

// grid = (row blocks, Q).  Sorted query q: sv[at .. at + m) with at = q_offsets[q] - q_offsets[0], m = qm[q]
// (ts_tol_sort_kernel).  part_w / part_p: uint64[Q][n_lists][k], block bx writes list bx; totals[q] (zeroed by the
// preparation) += the block's hits, one atomic.  Dynamic LDS: al_lds_bytes(lds_keys, B).
__global__ __launch_bounds__(kAlBlock) void ts_align_topk_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t min_votes, int32_t min_score, const int32_t *__restrict__ exclude_ids, int32_t k,
    unsigned long long *__restrict__ part_w, unsigned long long *__restrict__ part_p, int32_t n_lists,
    int32_t *__restrict__ totals) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long s_w[kAlWaves * 64], s_p[kAlWaves * 64];
    __shared__ int32_t s_nhits;
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    const int32_t m = qm[q];
    if (m <= 0 || m > lds_keys) return;       // empty: no hit; refused by the preparation: the selection flags it
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int nbp = al_bins_padded(B);
    double *s = reinterpret_cast<double *>(smem);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem + (size_t)lds_keys * 8) + (size_t)wv * nbp;
    uint16_t *dirty = reinterpret_cast<uint16_t *>(smem + (size_t)lds_keys * 8 + (size_t)kAlWaves * nbp * 4) + (size_t)wv * nbp;
    uint32_t *n_dirty = reinterpret_cast<uint32_t *>(smem + (size_t)lds_keys * 8 + (size_t)kAlWaves * nbp * 6) + wv;
    for (int e = threadIdx.x; e < m; e += kAlBlock) s[e] = sv[at + e];
    for (int b = lane; b < nbp; b += 64) hist[b] = 0;
    if (lane == 0) *n_dirty = 0;
    if (threadIdx.x == 0) s_nhits = 0;
    __syncthreads();

    const double Bd = (double)B;
    const int32_t excl = exclude_ids ? exclude_ids[q] : -1;
    const int64_t stride = (int64_t)gridDim.x * kAlWaves;
    const int64_t last_row = n_rows - 1;
    unsigned long long kw = kAlPad, kp = kAlPad;
    int32_t n_hits = 0;
    int64_t r = (int64_t)bx * kAlWaves + wv;
    Row row = load_row(rows + (r < n_rows ? r : last_row));
    while (r < n_rows) {                      // wave-uniform: no block barrier inside
        const int64_t rn = r + stride;
        const Row nrow = load_row(rows + (rn < n_rows ? rn : last_row));      // lands while this row votes
        const int64_t *rk = keys + row.off;
        unsigned long long best = 0;
        for (int j = lane; j < row.len; j += 64) {
            const double c = __longlong_as_double(rk[j]);
            for (int t = al_lo(s, m, c, eps, Bd); t < m; ++t) {
                const double d = al_bin(c, s[t], eps);
                if (!(d >= -Bd)) break;                                     // behind the window (or NaN there)
                if (!(d <= Bd)) continue;                                   // (never, behind al_lo: keeps the index in bounds)
                const int bin = (int)d;
                const uint32_t cnt = atomicAdd(&hist[bin + B], 1u) + 1u;
                if (cnt == 1u) dirty[atomicAdd(n_dirty, 1u)] = (uint16_t)(bin + B);
                const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                const unsigned long long key = ((unsigned long long)cnt << 14) | (16383u - order);
                best = key > best ? key : best;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        // LDS ops of one wave complete in order: the notes above are visible to the clearing below
        wave_lds_fence();
        const int nd = (int)*n_dirty;
        for (int i = lane; i < nd; i += 64) hist[dirty[i]] = 0;
        wave_lds_fence();
        if (lane == 0) *n_dirty = 0;
        const uint32_t votes = (uint32_t)(best >> 14);
        const uint32_t rl = (uint32_t)row.len;
        uint32_t v = votes < (uint32_t)m ? votes : (uint32_t)m;
        v = v < rl ? v : rl;
        if (v >= (uint32_t)min_votes && row.vid != excl) {                  // min_votes >= 1: v >= 1, u >= 1
            const uint32_t u = (uint32_t)m + rl - v;
            const uint32_t score = (v << 20) / u;                           // v <= 4095: the shift fits 32 bits
            if (score >= (uint32_t)min_score) {
                const uint32_t order = 16383u - (uint32_t)(best & 16383u);
                const int mag = (int)(order >> 1);
                ++n_hits;
                al_insert(kw, kp, al_word(score, row.vid, (order & 1u) ? mag : -mag),
                          ((unsigned long long)rl << 32) | votes, k, lane);
            }
        }
        row = nrow;
        r = rn;
    }
    s_w[wv * 64 + lane] = kw;
    s_p[wv * 64 + lane] = kp;
    if (lane == 0 && n_hits) atomicAdd(&s_nhits, n_hits);                    // LDS
    __syncthreads();
    if (wv == 0) {
#pragma unroll 1
        for (int j = 1; j < kAlWaves; ++j) al_take(kw, kp, s_w[j * 64 + lane], s_p[j * 64 + lane], k, lane);
        if (lane < k) {
            const int64_t o = ((int64_t)q * n_lists + bx) * k + lane;
            part_w[o] = kw;
            part_p[o] = kp;
        }
    }
    if (threadIdx.x == 0 && s_nhits) atomicAdd(&totals[q], s_nhits);
}

// One block per query: the k smallest (word, payload) of its n_lists sorted partial lists -> d_out[q] =
// int32[k+1][4]: k rows (video_id, row_len, best_bin, votes), padding (-1, 0, 0, 0), then (-1, n_hits, 0, 0).
// A query the preparation refused (qm < 0 or > lds_keys): all padding, n_hits = INT32_MIN.
__global__ __launch_bounds__(kAlReduceBlock) void ts_align_topk_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p, int32_t n_lists,
    int32_t k, const int32_t *__restrict__ qm, int32_t lds_keys, const int32_t *__restrict__ totals,
    int32_t *__restrict__ d_out) {
    __shared__ unsigned long long s_w[kAlReduceWaves * 64], s_p[kAlReduceWaves * 64];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int32_t m = qm[q];
    const bool refused = m < 0 || m > lds_keys;
    unsigned long long kw = kAlPad, kp = kAlPad;
    if (!refused && m > 0) {                                                 // (an empty query's lists were never written)
        const int64_t base = (int64_t)q * n_lists;
        for (int l0 = wv; l0 < n_lists; l0 += kAlReduceLd * kAlReduceWaves) {   // wave-uniform
            unsigned long long ew[kAlReduceLd], ep[kAlReduceLd];
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {
                const int l = l0 + j * kAlReduceWaves;
                const bool live = l < n_lists && lane < k;
                ew[j] = live ? part_w[(base + l) * k + lane] : kAlPad;
                ep[j] = live ? part_p[(base + l) * k + lane] : kAlPad;
            }
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) al_take(kw, kp, ew[j], ep[j], k, lane);
        }
    }
    s_w[wv * 64 + lane] = kw;
    s_p[wv * 64 + lane] = kp;
    __syncthreads();
    if (wv != 0) return;
#pragma unroll 1
    for (int j = 1; j < kAlReduceWaves; ++j) al_take(kw, kp, s_w[j * 64 + lane], s_p[j * 64 + lane], k, lane);
    int32_t *out = d_out + (int64_t)q * (k + 1) * 4;
    if (lane < k) {
        const bool pad = kw == kAlPad;
        out[lane * 4 + 0] = pad ? -1 : (int32_t)((kw >> 12) & 0x7fffffffu);
        out[lane * 4 + 1] = pad ? 0 : (int32_t)(kp >> 32);
        out[lane * 4 + 2] = pad ? 0 : (int32_t)(kw & 0xfffu) - 2048;
        out[lane * 4 + 3] = pad ? 0 : (int32_t)(kp & 0xffffffffu);
    }
    if (lane == 0) {
        out[k * 4 + 0] = -1;
        out[k * 4 + 1] = refused ? INT32_MIN : totals[q];
        out[k * 4 + 2] = 0;
        out[k * 4 + 3] = 0;
    }
}

// ---- the merge of the shards' blocks (tvz_align_topk_merge) ----------------------------------------------------
constexpr int kAlMergeBlock = 256;
constexpr int kAlMergeWaves = kAlMergeBlock / 64;      // queries per block: a wave each
constexpr int kAlMergeMaxLists = 16;                   // one n_hits per lane, far below a wave

// A list held one entry per lane whose padding may stand ANYWHERE (`live`: the lanes that hold a hit): the live
// entries are offered in lane order until one is refused.  As al_take, the early exit needs the live entries
// ascending - which every block of ts_align_topk_reduce_kernel is, by contract.
__device__ __forceinline__ void al_take_live(unsigned long long &kw, unsigned long long &kp, unsigned long long ew,
                                             unsigned long long ep, unsigned long long live, int k, int lane) {
    while (live) {                                                 // wave-uniform
        const int e = __ffsll((long long)live) - 1;
        live &= live - 1;
        if (!al_insert(kw, kp, __shfl(ew, e), __shfl(ep, e), k, lane)) break;
    }
}

// gathered int32[n_lists][Q][k+1][4], every [k+1][4] block as ts_align_topk_reduce_kernel writes it (k rows ascending
// in the contract's order, padding, then (-1, n_hits, 0, 0)) -> d_topk int32[Q][k][4], d_totals int32[Q].
// One wave per query, no LDS, no barrier.  A block row does not carry its order word - the score depends on nv, the
// query's count of non-NaN values, which no block holds - so the wave counts nv from the query itself and rebuilds
// (word, payload) with the sweep's expressions; a row with video_id < 0 is padding wherever it stands, and so is one
// whose u = nv + row_len - v would be 0 (nothing divides by zero).  The lists are SORTED BY CONTRACT: that is the
// precondition of the fold's early exit (al_take_live, as al_take).  Equal (word, payload) are identical rows and
// are all kept.  d_totals[q] = the lists' n_hits summed in 64 bits, clamped to INT32_MAX.  Refused - all k rows
// padding, d_totals[q] = INT32_MIN - when a list's n_hits is negative (INT32_MIN: a rank refused the query) or the
// query is longer than kAlMaxLen.  n_lists <= kAlMergeMaxLists, k <= kAlMaxK; gathered and d_topk 16-byte aligned.
__global__ __launch_bounds__(kAlMergeBlock) void ts_align_topk_merge_kernel(
    const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k, const double *__restrict__ queries,
    const int64_t *__restrict__ q_offsets, int32_t *__restrict__ d_topk, int32_t *__restrict__ d_totals) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kAlMergeWaves + (threadIdx.x >> 6);
    if (q >= Q) return;                                            // wave-uniform
    const int64_t k1 = (int64_t)k + 1;
    const int4 *blocks = reinterpret_cast<const int4 *>(gathered);            // [n_lists][Q][k+1] rows of 16 bytes
    // the lists' totals, one per lane; a negative one refuses the query
    const int32_t nh = lane < n_lists ? gathered[(((int64_t)lane * Q + q) * k1 + k) * 4 + 1] : 0;
    long long total = nh;
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    const int64_t qo = q_offsets[q];
    const int64_t len = q_offsets[q + 1] - qo;
    const bool refused = __ballot(nh < 0) != 0ull || len > kAlMaxLen;
    unsigned long long kw = kAlPad, kp = kAlPad;
    if (!refused) {
        int32_t nvl = 0;
        for (int64_t e = lane; e < len; e += 64) {
            const double x = queries[qo + e];
            nvl += x == x ? 1 : 0;
        }
        for (int off = 32; off > 0; off >>= 1) nvl += __shfl_xor(nvl, off);
        const uint32_t nv = (uint32_t)nvl;
        for (int l0 = 0; l0 < n_lists; l0 += kAlReduceLd) {        // wave-uniform
            int4 row[kAlReduceLd];
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {                // the loads of kAlReduceLd lists in flight together
                const int l = l0 + j;
                row[j] = l < n_lists && lane < k ? blocks[((int64_t)l * Q + q) * k1 + lane] : make_int4(-1, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {
                const uint32_t rl = (uint32_t)row[j].y, votes = (uint32_t)row[j].w;
                uint32_t v = votes < nv ? votes : nv;
                v = v < rl ? v : rl;
                const uint32_t u = nv + rl - v;
                const bool hit = row[j].x >= 0 && u != 0u;
                const uint32_t score = hit ? (v << 20) / u : 0u;   // v <= nv <= 4095: the shift fits 32 bits
                const unsigned long long ew = hit ? al_word(score, row[j].x, row[j].z) : kAlPad;
                const unsigned long long ep = hit ? ((unsigned long long)rl << 32) | votes : kAlPad;
                al_take_live(kw, kp, ew, ep, __ballot(hit), k, lane);
            }
        }
    }
    if (lane < k) {
        const bool pad = kw == kAlPad;
        int4 o;
        o.x = pad ? -1 : (int32_t)((kw >> 12) & 0x7fffffffu);
        o.y = pad ? 0 : (int32_t)(kp >> 32);
        o.z = pad ? 0 : (int32_t)(kw & 0xfffu) - 2048;
        o.w = pad ? 0 : (int32_t)(kp & 0xffffffffu);
        reinterpret_cast<int4 *>(d_topk)[(int64_t)q * k + lane] = o;
    }
    if (lane == 0) d_totals[q] = refused ? INT32_MIN : (int32_t)(total > INT32_MAX ? INT32_MAX : total);
}

}  // namespace
