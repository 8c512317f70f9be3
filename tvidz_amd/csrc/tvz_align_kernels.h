// tvz_align_kernels.h — batched alignment score with the k best rows kept inside the sweep, gfx950 wave64: the bounded
// call (tvz_align_topk, at most kAlignMaxBins bins), the call at any shift (tvz_align_wide_topk, up to kAwMaxB bins on
// either side of zero), that call with rates (tvz_align_rates_topk) and with the matched span (tvz_align_span_topk),
// and the merges of the shards' blocks, one per form.  Included by tvz_match.hip only, whose table kAlignForms says
// what each form is on the host.  From tvz_match_kernels.h: Row, load_row, al_bin (the vote's expression); from
// tvz_tol_kernels.h: ts_tol_sort_kernel (the batch's queries sorted numerically, NaNs dropped, qm = the non-NaN
// count) and the sweep's block count (tol_topk_max_blocks); from tvz_wave.h: wave_lds_fence.
//
// Contract (include/tvz.h): votes and bins are tvz_align's - the pair (row key c, query value x) votes into
//   d = floor((c - x) / eps + 0.5)      (one IEEE subtraction, one true division)
// when -B <= d <= B; the score is the tolerant Jaccard or, for the wide call with TVZ_ALIGN_CONTAIN, v / min(nv,
// row_len); a row's hit is ordered by the tuple (score descending, video_id, best_bin, row_len, votes).  The forms
// pack that tuple differently (AlHit, AwHit, ArHit, AsHit below) and share everything else.
//
// A key's run: for a fixed key c each of c - x, / eps, + 0.5 and floor never increases as x grows, so the query
// values that vote into a range of bins are ONE contiguous run of the sorted query.  Its start is found by a binary
// search with the vote's own expression (al_left below; never a rewrite such as x >= c - max_offset, which rounds
// differently); from there the run is walked, voting, until the expression itself says the run has ended.  A NaN
// (inf - inf, or inf / inf with an infinite eps) is outside the range on the side its x lies on.
//
// The sweep (al_sweep), grid = (row blocks, Q): a wave per row.  Per wave a histogram of `width` bins and a list of the
// bins it has touched.  A vote is a returning LDS add; every lane keeps the largest
//   count << 33 | (2^33 - 1 - order),   order = 2 |bin| + (bin > 0)
// it has seen - the lane that makes a bin's last increment sees its final count, so the wave's maximum is the best bin
// under the tie rule with no scan of the histogram - and the lane that finds a bin at zero notes it, so clearing costs
// the bins touched, not 2B + 1.  The wave's k best hits live in registers, one hit per lane, ascending: a hit below the
// k-th is inserted by one ballot and one lane shift (al_insert).  The selection (al_reduce), one block per query: the k
// smallest of the blocks' lists -> d_out[q].
//
// The window walk (al_sweep<.., true>, the wide call): the histogram holds aw_width(B) bins - all 2B + 1 of them while
// they fit kAwOneWindow, so a call with B <= 2047 is ONE window and does the bounded sweep's work; kAwWidth beyond.
// Window w of the global grid covers the bins [w * width - B, w * width - B + width - 1], clipped to B.  A row's pairs
// can only vote inside [bin(c_min, x_max), bin(c_max, x_min)] - every step of the vote's expression is monotone in c
// and in x - so only the windows that meet that range (clipped to [-B, B]) are visited, from the highest down.  Per
// window every key's run is found by al_lo with the WINDOW's upper bin as the bound, and walked until the expression
// falls below the window's lower bin: all votes of one bin fall into one window, so the lane that makes a bin's last
// increment sees its final count there, and the lane-wise best, whose order is taken on the GLOBAL bin, carries the
// tie rule across windows.  Between windows the histogram is cleared through the touched list.  The bounded sweep
// (al_sweep<.., false>) is the one window [-B, B] with none of this compiled in.
//
// The resume position: a key's runs move to larger x as the windows descend, and the position where a window's walk
// stops - the first value whose bin lies below the window - is al_lo's answer for the next window (whose upper bin is
// this one's lower bin - 1; a walk that stops at a NaN has met a key that never votes).  So only a row's highest
// window searches; the later ones read the position back, for the row's first kAwResume keys (a u16 per key and
// wave in LDS, written and read by the same lane); keys beyond them search in every window.
//
// The rates (al_sweep<.., true, true>, tvz_align_rates_topk): the copy played at another speed, c = rho x + t.  The
// wave walks its row once per rate rho_i of the call's list (a by-value kernel argument, read with scalar loads: no
// LDS) with every query value read as x' = x * rho_i - ONE IEEE multiplication that the compiler may not contract
// with the vote's subtraction (al_scaled) - and keeps the rate whose best bin has the most votes, the smaller index
// on a tie.  The product keeps the sorted query sorted: for rho > 0, fl(x * rho) never decreases as x grows, and an
// infinity stays the same infinity.  So al_lo, the runs and the row's window range [bin(c_min, x'_max), bin(c_max,
// x'_min)] hold per rate, with x'_min / x'_max the products of s[0] / s[m - 1].  The resume positions are one rate's:
// a rate's highest window searches.  The kept hit carries the rate's index behind the votes (ArHit) and the block
// has a fifth column; the selection and the merge carry it and never read it.
//
// The span (al_sweep<.., true, true, true>, tvz_align_span_topk): where the votes of the row's best bin
// lie.  When the rate loop ends the wave knows the row's best bin and rate; a row that can still be a hit is walked
// once more at that single bin (al_span) for the first and last voting index of the sorted query and the count of
// row keys between the smallest and the largest voting key.  The kept hit carries them behind the rate's index (AsHit),
// the block has eight columns, and with TVZ_ALIGN_LOCAL the score is the Jaccard of the two sides inside the span.
//
// Two bins (al_sweep<.., kTwoBins = true>, TVZ_ALIGN_TWO_BINS on the three calls above): the row's best
// WINDOW of two adjacent bins, J[b] = h[b] + h[b + 1], ordered by (J, h[b], the bin order) - for the copy whose shift
// lies near a bin's edge.  A window needs two bins' FINAL counts, so the lane-wise best of the vote loop is not
// taken; behind the fence that precedes the clearing every lane reads h[s] and h[s + 1] for its slots of the touched
// list - the candidates are exactly the touched bins, the second key rules a window with an empty lower bin out - and
// keeps the best.  The windows descend, so the bin above a window's last slot is the lowest bin of the window visited
// before: its count is carried in one word per wave, 0 for the first window of a rate.  The kept hit holds the
// window's lower bin and J; the span walks the two bins.  Kernels of their own (ts_align{w,r,s}2_sweep_kernel): the
// single-bin sweeps keep their machine code.
#pragma once
#include "tvz_match_kernels.h"
#include "tvz_tol_kernels.h"
#include "tvz_wave.h"
#include <type_traits>

namespace {

constexpr int kAlBlock = 256;
constexpr int kAlWaves = kAlBlock / 64;                // rows in flight per block
constexpr int kAlMaxK = 64;                            // one kept hit per lane
constexpr int kAlMaxLen = 4095;                        // v << 20 fits 32 bits; the sorted query fits LDS
constexpr int kAlScoreOne = 1 << 20;
constexpr int kAlReduceBlock = 1024;
constexpr int kAlReduceWaves = kAlReduceBlock / 64;
constexpr int kAlReduceLd = 4;                         // lists a wave loads per step (their loads in flight together)
constexpr unsigned long long kAlPad = ~0ull;           // no first word is all ones: its top field is at most 2^20
constexpr unsigned long long kAlOrderMask = (1ull << 33) - 1;

constexpr int kAwMaxB = 1 << 22;                       // TVZ_ALIGN_WIDE_MAX_B
constexpr int kAwOneWindow = 4096;                     // a call of at most this many bins is one window: the bounded sweep's shape
constexpr int kAwWidth = 1024;                         // bins of a window otherwise (measured against 256..4096)
constexpr int kAwResume = 512;                         // keys of a row whose resume position is kept (a multiple of 64)
constexpr uint32_t kAwContain = 1u;                    // TVZ_ALIGN_CONTAIN
constexpr int kArMaxRates = 8;                         // TVZ_ALIGN_MAX_RATES
constexpr uint32_t kAsLocal = 2u;                      // TVZ_ALIGN_LOCAL
constexpr uint32_t kAlTwoBins = 8u;                    // TVZ_ALIGN_TWO_BINS (4 is no flag, and stays refused)

// the rates of tvz_align_rates_topk, a kernel argument by value: r[0 .. n), each finite and > 0 (the host's check)
struct AlRates {
    double r[kArMaxRates];
    int32_t n;
};

// bins of a wave's histogram (even: the touched list behind the histograms stays 4-byte aligned).  The bounded call's
// is aw_width too: its B is at most 2047
__host__ __device__ inline int al_bins_padded(int32_t B) { return (2 * B + 1 + 1) & ~1; }
__host__ __device__ inline int aw_width(int32_t B) { return al_bins_padded(B) <= kAwOneWindow ? al_bins_padded(B) : kAwWidth; }
// the most windows a row can take: ceil((2B + 1) / width)
__host__ __device__ inline int aw_max_windows(int32_t B, int width) { return (2 * B + width) / width; }
// dynamic LDS of the sweep: the sorted query, then per wave a histogram (u32 per bin), the touched bins (u16 per
// bin), their count and the resume positions (u16 per key; none where the call has one window)
__host__ __device__ inline int aw_resume_keys(int32_t B, int width) { return aw_max_windows(B, width) > 1 ? kAwResume : 0; }
inline size_t aw_lds_bytes(int32_t lds_keys, int32_t B, int width) {
    return (size_t)lds_keys * 8 + (size_t)kAlWaves * ((size_t)width * 6 + 4 + (size_t)aw_resume_keys(B, width) * 2);
}
// ... and wave wv's part of it, with the call's window shape.  Without kWindowed: the one window, no resume positions
struct AlWave {
    uint32_t *hist;
    uint16_t *dirty;
    uint32_t *n_dirty;
    uint16_t *resume;
    int width, max_windows, resume_keys;
};
template <bool kWindowed>
__device__ __forceinline__ AlWave al_wave(unsigned char *smem, int32_t lds_keys, int32_t B, int32_t width, int wv) {
    unsigned char *waves = smem + (size_t)lds_keys * 8;
    uint32_t *counts = reinterpret_cast<uint32_t *>(waves + (size_t)kAlWaves * width * 6);      // behind the waves' bins
    AlWave w{reinterpret_cast<uint32_t *>(waves) + (size_t)wv * width,
             reinterpret_cast<uint16_t *>(waves + (size_t)kAlWaves * width * 4) + (size_t)wv * width, counts + wv, nullptr,
             width, 1, 0};
    if constexpr (kWindowed) {
        w.max_windows = aw_max_windows(B, width);
        w.resume_keys = aw_resume_keys(B, width);
        w.resume = reinterpret_cast<uint16_t *>(counts + kAlWaves) + (size_t)wv * w.resume_keys;
    }
    return w;
}
// a clean histogram and an empty touched list, which every row walk expects and leaves behind
__device__ __forceinline__ void al_wave_clear(const AlWave &w, int lane) {
    for (int b = lane; b < w.width; b += 64) w.hist[b] = 0;
    if (lane == 0) *w.n_dirty = 0;
}

// x' = x * rho of the contract: the product is rounded on its own, never fused with al_bin's subtraction
__device__ __forceinline__ double al_scaled(double x, double rho) {
#pragma clang fp contract(off)
    return x * rho;
}

// the sorted query's value t as the votes see it: scaled by the rate where the sweep has rates
template <bool kRates> __device__ __forceinline__ double al_x(const double *s, int t, double rho) {
    if constexpr (kRates) return al_scaled(s[t], rho);
    else return s[t];
}

// is x in front of key c's run?  d > Bd; a NaN d counts by the side x lies on (x == c only for two equal
// infinities: -inf is the smallest query value, +inf the largest)
__device__ __forceinline__ bool al_left(double c, double x, double eps, double Bd) {
    const double d = al_bin(c, x, eps);
    return d > Bd || (d != d && (x < c || (x == c && x < 0.0)));
}

// first t with s[t] not in front of the run: a prefix of the sorted query
template <bool kRates>
__device__ __forceinline__ int al_lo(const double *s, int m, double c, double eps, double Bd, double rho) {
    int lo = 0, len = m;
    while (len > 0) {
        const int half = len >> 1;
        if (al_left(c, al_x<kRates>(s, lo + half, rho), eps, Bd)) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// ---- a kept hit, in the forms' layouts ----------------------------------------------------------------------------
// Lists<N>: N hits as a structure of arrays, in static LDS; Parts / ConstParts: the same arrays in the workspace,
// [Q][n_lists][k] each.  load / store take any of them.  kCols: the int32 columns of the hit's block row; column 4 + i
// (ArHit's one, AsHit's four) is extra(i); make() takes the first, the rate's index, and with_more() those behind it.

// the bounded call's: 16 bytes, ordered as (w, p)
struct AlHit {
    unsigned long long w, p;       // (2^20 - score) << 43 | video_id << 12 | bin + 2048;  row_len << 32 | votes
    static constexpr int kCols = 4;
    template <int N> struct Lists { unsigned long long w[N], p[N]; };
    struct Parts { unsigned long long *w, *p; };
    struct ConstParts { const unsigned long long *w, *p; };
    static __device__ __forceinline__ AlHit make(uint32_t score, int32_t vid, int bin, uint32_t row_len, uint32_t votes,
                                                 uint32_t /* rate */) {
        return {((unsigned long long)(kAlScoreOne - score) << 43) | ((unsigned long long)((uint32_t)vid & 0x7fffffffu) << 12) |
                    (unsigned long long)(uint32_t)(bin + 2048),
                ((unsigned long long)row_len << 32) | votes};
    }
    static __device__ __forceinline__ AlHit pad() { return {kAlPad, kAlPad}; }
    __device__ __forceinline__ bool is_pad() const { return w == kAlPad; }
    static __device__ __forceinline__ bool le(const AlHit &a, const AlHit &b) { return a.w < b.w || (a.w == b.w && a.p <= b.p); }
    __device__ __forceinline__ int4 row() const {      // (video_id, row_len, best_bin, votes)
        const bool pad = is_pad();
        return make_int4(pad ? -1 : (int32_t)((w >> 12) & 0x7fffffffu), pad ? 0 : (int32_t)(p >> 32),
                         pad ? 0 : (int32_t)(w & 0xfffu) - 2048, pad ? 0 : (int32_t)(p & 0xffffffffu));
    }
    static __device__ __forceinline__ AlHit select(bool c, const AlHit &a, const AlHit &b) { return {c ? a.w : b.w, c ? a.p : b.p}; }
    __device__ __forceinline__ AlHit lane(int src) const { return {__shfl(w, src), __shfl(p, src)}; }
    __device__ __forceinline__ AlHit shift_up() const { return {__shfl_up(w, 1), __shfl_up(p, 1)}; }
    template <class L> static __device__ __forceinline__ AlHit load(const L &l, int64_t i) { return {l.w[i], l.p[i]}; }
    template <class L> __device__ __forceinline__ void store(L &l, int64_t i) const {
        l.w[i] = w;
        l.p[i] = p;
    }
};

// the wide call's: 20 bytes, ordered as (w, p, v)
struct AwHit {
    unsigned long long w, p;       // (2^20 - score) << 31 | video_id;  (bin + 2^22) << 32 | row_len
    uint32_t v;                    // the raw votes
    static constexpr int kCols = 4;
    template <int N> struct Lists { unsigned long long w[N], p[N]; uint32_t v[N]; };
    struct Parts { unsigned long long *w, *p; uint32_t *v; };
    struct ConstParts { const unsigned long long *w, *p; const uint32_t *v; };
    static __device__ __forceinline__ AwHit make(uint32_t score, int32_t vid, int bin, uint32_t row_len, uint32_t votes,
                                                 uint32_t /* rate */) {
        return {((unsigned long long)(kAlScoreOne - score) << 31) | (unsigned long long)((uint32_t)vid & 0x7fffffffu),
                ((unsigned long long)(uint32_t)(bin + kAwMaxB) << 32) | row_len, votes};
    }
    static __device__ __forceinline__ AwHit pad() { return {kAlPad, kAlPad, ~0u}; }
    __device__ __forceinline__ bool is_pad() const { return w == kAlPad; }
    static __device__ __forceinline__ bool le(const AwHit &a, const AwHit &b) {
        return a.w < b.w || (a.w == b.w && (a.p < b.p || (a.p == b.p && a.v <= b.v)));
    }
    __device__ __forceinline__ int4 row() const {      // (video_id, row_len, best_bin, votes)
        const bool pad = is_pad();
        return make_int4(pad ? -1 : (int32_t)(w & 0x7fffffffu), pad ? 0 : (int32_t)(p & 0xffffffffu),
                         pad ? 0 : (int32_t)(p >> 32) - kAwMaxB, pad ? 0 : (int32_t)v);
    }
    static __device__ __forceinline__ AwHit select(bool c, const AwHit &a, const AwHit &b) {
        return {c ? a.w : b.w, c ? a.p : b.p, c ? a.v : b.v};
    }
    __device__ __forceinline__ AwHit lane(int src) const { return {__shfl(w, src), __shfl(p, src), __shfl(v, src)}; }
    __device__ __forceinline__ AwHit shift_up() const { return {__shfl_up(w, 1), __shfl_up(p, 1), __shfl_up(v, 1)}; }
    template <class L> static __device__ __forceinline__ AwHit load(const L &l, int64_t i) { return {l.w[i], l.p[i], l.v[i]}; }
    template <class L> __device__ __forceinline__ void store(L &l, int64_t i) const {
        l.w[i] = w;
        l.p[i] = p;
        l.v[i] = v;
    }
};

// the call with rates' (DESIGN.md 4.12): AwHit and the index of the rate the votes were counted at, 24 bytes, ordered
// as (w, p, v, r)
struct ArHit {
    unsigned long long w, p;       // as AwHit's
    uint32_t v, r;                 // the raw votes; the rate's index
    static constexpr int kCols = 5;
    template <int N> struct Lists { unsigned long long w[N], p[N]; uint32_t v[N], r[N]; };
    struct Parts { unsigned long long *w, *p; uint32_t *v, *r; };
    struct ConstParts { const unsigned long long *w, *p; const uint32_t *v, *r; };
    static __device__ __forceinline__ ArHit make(uint32_t score, int32_t vid, int bin, uint32_t row_len, uint32_t votes,
                                                 uint32_t rate) {
        return {((unsigned long long)(kAlScoreOne - score) << 31) | (unsigned long long)((uint32_t)vid & 0x7fffffffu),
                ((unsigned long long)(uint32_t)(bin + kAwMaxB) << 32) | row_len, votes, rate};
    }
    static __device__ __forceinline__ ArHit pad() { return {kAlPad, kAlPad, ~0u, ~0u}; }
    __device__ __forceinline__ bool is_pad() const { return w == kAlPad; }
    static __device__ __forceinline__ bool le(const ArHit &a, const ArHit &b) {
        return a.w < b.w || (a.w == b.w && (a.p < b.p || (a.p == b.p && (a.v < b.v || (a.v == b.v && a.r <= b.r)))));
    }
    __device__ __forceinline__ int4 row() const {      // (video_id, row_len, best_bin, votes)
        const bool pad = is_pad();
        return make_int4(pad ? -1 : (int32_t)(w & 0x7fffffffu), pad ? 0 : (int32_t)(p & 0xffffffffu),
                         pad ? 0 : (int32_t)(p >> 32) - kAwMaxB, pad ? 0 : (int32_t)v);
    }
    __device__ __forceinline__ int32_t extra(int /* 0 */) const { return is_pad() ? 0 : (int32_t)r; }      // rate_index
    static __device__ __forceinline__ ArHit select(bool c, const ArHit &a, const ArHit &b) {
        return {c ? a.w : b.w, c ? a.p : b.p, c ? a.v : b.v, c ? a.r : b.r};
    }
    __device__ __forceinline__ ArHit lane(int src) const { return {__shfl(w, src), __shfl(p, src), __shfl(v, src), __shfl(r, src)}; }
    __device__ __forceinline__ ArHit shift_up() const {
        return {__shfl_up(w, 1), __shfl_up(p, 1), __shfl_up(v, 1), __shfl_up(r, 1)};
    }
    template <class L> static __device__ __forceinline__ ArHit load(const L &l, int64_t i) {
        return {l.w[i], l.p[i], l.v[i], l.r[i]};
    }
    template <class L> __device__ __forceinline__ void store(L &l, int64_t i) const {
        l.w[i] = w;
        l.p[i] = p;
        l.v[i] = v;
        l.r[i] = r;
    }
};

// the call with spans' (DESIGN.md 4.13): ArHit and where the best bin's votes lie - the first and the last voting
// index of the sorted query in ONE word (t_first << 16 | t_last, each at most 4094: the word orders as the pair) and
// the row keys inside the voting keys' range -, 32 bytes, ordered as (w, p, v, r, t, n)
struct AsHit {
    unsigned long long w, p;       // as AwHit's
    uint32_t v, r, t, n;           // the raw votes; the rate's index; t_first << 16 | t_last; nr
    static constexpr int kCols = 8;
    template <int N> struct Lists { unsigned long long w[N], p[N]; uint32_t v[N], r[N], t[N], n[N]; };
    struct Parts { unsigned long long *w, *p; uint32_t *v, *r, *t, *n; };
    struct ConstParts { const unsigned long long *w, *p; const uint32_t *v, *r, *t, *n; };
    static __device__ __forceinline__ AsHit make(uint32_t score, int32_t vid, int bin, uint32_t row_len, uint32_t votes,
                                                 uint32_t rate) {           // (the span: with_more)
        return {((unsigned long long)(kAlScoreOne - score) << 31) | (unsigned long long)((uint32_t)vid & 0x7fffffffu),
                ((unsigned long long)(uint32_t)(bin + kAwMaxB) << 32) | row_len, votes, rate, 0u, 0u};
    }
    // the columns behind the rate's: x = (t_first, t_last, nr), the first two below 2^16
    __device__ __forceinline__ AsHit with_more(const uint32_t *x) const { return {w, p, v, r, (x[0] << 16) | x[1], x[2]}; }
    static __device__ __forceinline__ AsHit pad() { return {kAlPad, kAlPad, ~0u, ~0u, ~0u, ~0u}; }
    __device__ __forceinline__ bool is_pad() const { return w == kAlPad; }
    static __device__ __forceinline__ bool le(const AsHit &a, const AsHit &b) {
        if (a.w != b.w) return a.w < b.w;
        if (a.p != b.p) return a.p < b.p;
        if (a.v != b.v) return a.v < b.v;
        if (a.r != b.r) return a.r < b.r;
        return a.t < b.t || (a.t == b.t && a.n <= b.n);
    }
    __device__ __forceinline__ int4 row() const {      // (video_id, row_len, best_bin, votes)
        const bool pad = is_pad();
        return make_int4(pad ? -1 : (int32_t)(w & 0x7fffffffu), pad ? 0 : (int32_t)(p & 0xffffffffu),
                         pad ? 0 : (int32_t)(p >> 32) - kAwMaxB, pad ? 0 : (int32_t)v);
    }
    __device__ __forceinline__ int32_t extra(int i) const {      // rate_index, t_first, t_last, nr
        const uint32_t x = i == 0 ? r : i == 1 ? t >> 16 : i == 2 ? t & 0xffffu : n;
        return is_pad() ? 0 : (int32_t)x;
    }
    static __device__ __forceinline__ AsHit select(bool c, const AsHit &a, const AsHit &b) {
        return {c ? a.w : b.w, c ? a.p : b.p, c ? a.v : b.v, c ? a.r : b.r, c ? a.t : b.t, c ? a.n : b.n};
    }
    __device__ __forceinline__ AsHit lane(int src) const {
        return {__shfl(w, src), __shfl(p, src), __shfl(v, src), __shfl(r, src), __shfl(t, src), __shfl(n, src)};
    }
    __device__ __forceinline__ AsHit shift_up() const {
        return {__shfl_up(w, 1), __shfl_up(p, 1), __shfl_up(v, 1), __shfl_up(r, 1), __shfl_up(t, 1), __shfl_up(n, 1)};
    }
    template <class L> static __device__ __forceinline__ AsHit load(const L &l, int64_t i) {
        return {l.w[i], l.p[i], l.v[i], l.r[i], l.t[i], l.n[i]};
    }
    template <class L> __device__ __forceinline__ void store(L &l, int64_t i) const {
        l.w[i] = w;
        l.p[i] = p;
        l.v[i] = v;
        l.r[i] = r;
        l.t[i] = t;
        l.n[i] = n;
    }
};

// static LDS of a sweep block: the waves' lists at the block's end + a few words
template <class Hit> constexpr int al_static_lds() { return (int)sizeof(typename Hit::template Lists<kAlWaves * 64>) + 64; }

// One wave's list: lane i holds its i-th best hit (ascending, padding behind them and from lane k on).  The wave
// takes one more hit (wave-uniform h): false when it does not come before the k-th.  Equal hits are all kept.
// (Member-wise selects: a conditional assignment of the whole struct compiles to branches and costs registers.)
template <class Hit> __device__ __forceinline__ bool al_insert(Hit &kept, Hit h, int k, int lane) {
    const int pos = __popcll(__ballot(Hit::le(kept, h)));          // the kept hits that stay in front: a prefix
    if (pos >= k) return false;
    const Hit up = kept.shift_up();
    kept = Hit::select(lane > pos, up, kept);
    kept = Hit::select(lane == pos, h, kept);
    kept = Hit::select(lane >= k, Hit::pad(), kept);
    return true;
}

// ... and a whole sorted list held one entry per lane (e): entry i is offered until one is refused
template <class Hit> __device__ __forceinline__ void al_take(Hit &kept, Hit e, int k, int lane) {
    for (int i = 0; i < k; ++i) {                                  // wave-uniform
        const Hit h = e.lane(i);
        if (h.is_pad() || !al_insert(kept, h, k, lane)) break;
    }
}

// A list held one entry per lane whose padding may stand ANYWHERE (`live`: the lanes that hold a hit; the other
// lanes' e is never read): the live entries are offered in lane order until one is refused.  As al_take, the early
// exit needs the live entries ascending - which every block of al_reduce is, by contract.
template <class Hit> __device__ __forceinline__ void al_take_live(Hit &kept, Hit e, unsigned long long live, int k, int lane) {
    while (live) {                                                 // wave-uniform
        const int i = __ffsll((long long)live) - 1;
        live &= live - 1;
        if (!al_insert(kept, e.lane(i), k, lane)) break;
    }
}

// The block-end merge: every wave leaves its list in LDS, wave 0 folds the others into its own.  Contains a block
// barrier: every thread of the block calls it.
template <class Hit, int N> __device__ __forceinline__ void al_merge_waves(Hit &kept, typename Hit::template Lists<N> &s, int wv,
                                                                           int lane, int k) {
    kept.store(s, wv * 64 + lane);
    __syncthreads();
    if (wv != 0) return;
#pragma unroll 1
    for (int j = 1; j < N / 64; ++j) al_take(kept, Hit::load(s, j * 64 + lane), k, lane);
}

// One wave writes a query's block int32[k+1][kCols]: k rows (video_id, row_len, best_bin, votes[, the hit's extra
// columns]), padding (-1, 0, 0, 0[, 0 ..]), then (-1, n_hits, 0, 0[, 0 ..]) with n_hits = INT32_MIN for a refused
// query.  Word stores: a row of five columns is not 16-byte aligned
template <class Hit> __device__ __forceinline__ void al_write_block(const Hit &kept, int32_t *out, int k, int lane, int32_t n_hits) {
    constexpr int kCols = Hit::kCols;
    if (lane < k) {
        const int4 o = kept.row();
        out[lane * kCols + 0] = o.x;
        out[lane * kCols + 1] = o.y;
        out[lane * kCols + 2] = o.z;
        out[lane * kCols + 3] = o.w;
        if constexpr (kCols > 4) {
#pragma unroll
            for (int i = 4; i < kCols; ++i) out[lane * kCols + i] = kept.extra(i - 4);
        }
    }
    if (lane == 0) {
        out[k * kCols + 0] = -1;
        out[k * kCols + 1] = n_hits;
        out[k * kCols + 2] = 0;
        out[k * kCols + 3] = 0;
        if constexpr (kCols > 4) {
#pragma unroll
            for (int i = 4; i < kCols; ++i) out[k * kCols + i] = 0;
        }
    }
}

// ---- what a wave does with one row, shared with tvz_align_parts_kernels.h ----------------------------------------------
// the bin of a best (count << 33 | 2^33 - 1 - order)
__device__ __forceinline__ int al_best_bin(unsigned long long best) {
    const uint32_t order = (uint32_t)(kAlOrderMask - (best & kAlOrderMask));
    const int mag = (int)(order >> 1);
    return (order & 1u) ? mag : -mag;
}

// Which pairs (row key c, index t of the sorted query) al_bin_extremes counts: key(c) is asked once per key, index(t)
// once per pair that votes into the bin.  The span allows every pair, and both tests fold away; the parts walk's is
// ApOutside.
struct AlAllPairs {
    __device__ __forceinline__ bool key(double) const { return true; }
    __device__ __forceinline__ bool index(int) const { return true; }
};

// a row's smallest and largest key, in every lane (+inf and -inf for an empty row)
struct AlKeyRange {
    double c_min, c_max;
};
__device__ __forceinline__ AlKeyRange al_key_range(const int64_t *__restrict__ rk, int len, int lane) {
    double c_min = __longlong_as_double(0x7ff0000000000000ll), c_max = -c_min;
    for (int j = lane; j < len; j += 64) {
        const double c = __longlong_as_double(rk[j]);
        c_min = c < c_min ? c : c_min;
        c_max = c > c_max ? c : c_max;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double lo = __shfl_xor(c_min, off), hi = __shfl_xor(c_max, off);
        c_min = lo < c_min ? lo : c_min;
        c_max = hi > c_max ? hi : c_max;
    }
    return {c_min, c_max};
}

// Where the votes of one bin lie: over the allowed pairs whose vote - the walk's own expression at the rate rho - is
// `bin`, the smallest and the largest index and key, the same in every lane.  The window loop's walk with the one bin
// as the window and nothing noted but the four extremes: no LDS beyond the sorted query, no barrier.  The bin has allowed
// votes (the caller's count of them is >= 1), so no range comes back empty.
struct AlExtremes {
    int t_first, t_last;
    double c_lo, c_hi;
};
template <class Allow, bool kTwoBins = false>
__device__ __forceinline__ AlExtremes al_bin_extremes(const int64_t *__restrict__ rk, int len, const double *s, int m, double eps,
                                                      int bin, double rho, const Allow &allow, int lane, int bin_hi = 0) {
    const double bd = (double)bin;
    double hd = bd;                                                           // kTwoBins: the bins [bin, bin_hi], bin_hi = bin
    if constexpr (kTwoBins) hd = (double)bin_hi;                              // or bin + 1; the one bin otherwise
    int t_first = m, t_last = -1;
    double c_lo = __longlong_as_double(0x7ff0000000000000ll), c_hi = -c_lo;
    for (int j = lane; j < len; j += 64) {
        const double c = __longlong_as_double(rk[j]);
        if (!allow.key(c)) continue;
        for (int t = al_lo<true>(s, m, c, eps, hd, rho); t < m; ++t) {
            const double d = al_bin(c, al_x<true>(s, t, rho), eps);
            if (!(d >= bd)) break;                                        // behind the bin (or NaN there)
            if (!(d <= hd) || !allow.index(t)) continue;                  // (the first: never, behind al_lo)
            t_first = t < t_first ? t : t_first;
            t_last = t > t_last ? t : t_last;
            c_lo = c < c_lo ? c : c_lo;
            c_hi = c > c_hi ? c : c_hi;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int tf = __shfl_xor(t_first, off), tl = __shfl_xor(t_last, off);
        const double lo = __shfl_xor(c_lo, off), hi = __shfl_xor(c_hi, off);
        t_first = tf < t_first ? tf : t_first;
        t_last = tl > t_last ? tl : t_last;
        c_lo = lo < c_lo ? lo : c_lo;
        c_hi = hi > c_hi ? hi : c_hi;
    }
    return {t_first, t_last, c_lo, c_hi};
}

// The span of a row's best bin (include/tvz.h, tvz_align_span_topk): the extremes of every pair that votes into it, and
// nr = the row's keys inside [smallest voting key, largest voting key], counted by a second lane-strided pass.
struct AlSpan {
    int t_first, t_last;
    uint32_t nr;
};
template <bool kTwoBins = false>
__device__ __forceinline__ AlSpan al_span(const int64_t *__restrict__ rk, int len, const double *s, int m, double eps, int bin,
                                          double rho, int lane, int bin_hi = 0) {
    const AlExtremes x = al_bin_extremes<AlAllPairs, kTwoBins>(rk, len, s, m, eps, bin, rho, AlAllPairs{}, lane, bin_hi);
    uint32_t nr = 0;
    for (int j = lane; j < len; j += 64) {
        const double c = __longlong_as_double(rk[j]);
        nr += c >= x.c_lo && c <= x.c_hi ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) nr += __shfl_xor(nr, off);
    return {x.t_first, x.t_last, nr};
}

// grid = (row blocks, Q).  Sorted query q: sv[at .. at + m) with at = q_offsets[q] - q_offsets[0], m = qm[q]
// (ts_tol_sort_kernel).  part: the kept lists, block bx writes list bx; totals[q] (zeroed by the preparation) += the
// block's hits, one atomic.  width = aw_width(B); dynamic LDS: aw_lds_bytes(lds_keys, B, width).  0 <= B <= kAwMaxB,
// and B <= 2047 where !kWindowed (the host refuses anything else before the launch).  kRates: the row is walked once
// per rate of `rates` (1 .. kArMaxRates of them) and its best rate kept; without, `rates` is never read.  kSpan (with
// kRates; Hit = AsHit): a row that can be a hit is walked once more at its best bin and rate for the span (al_span),
// and with `local` the score is the Jaccard inside the span.  kTwoBins (with kWindowed): the row's best window of two
// adjacent bins instead of its best bin (the header comment); nothing of it is compiled into the other sweeps.
template <class Hit, bool kWindowed, bool kRates = false, bool kSpan = false, bool kTwoBins = false>
__device__ __forceinline__ void al_sweep(const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys,
                                         const double *__restrict__ sv, const int64_t *__restrict__ q_offsets,
                                         const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B, int32_t width,
                                         int32_t min_votes, int32_t min_score, bool contain,
                                         const int32_t *__restrict__ exclude_ids, int32_t k, typename Hit::Parts part,
                                         int32_t n_lists, int32_t *__restrict__ totals, const AlRates &rates = AlRates{},
                                         bool local = false) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ typename Hit::template Lists<kAlWaves * 64> s_kept;
    __shared__ int32_t s_nhits;
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    const int32_t m = qm[q];
    if (m <= 0 || m > lds_keys) return;       // empty: no hit; refused by the preparation: the selection flags it
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    double *s = reinterpret_cast<double *>(smem);
    const AlWave w = al_wave<kWindowed>(smem, lds_keys, B, width, wv);
    for (int e = threadIdx.x; e < m; e += kAlBlock) s[e] = sv[at + e];
    al_wave_clear(w, lane);
    if (threadIdx.x == 0) s_nhits = 0;
    __syncthreads();

    const double Bd = (double)B;
    double x_min = 0.0, x_max = 0.0;
    if constexpr (kWindowed && !kRates) {
        x_min = s[0];                                                         // sorted numerically, no NaN
        x_max = s[m - 1];
    }
    const int n_rates = kRates ? rates.n : 1;                                 // >= 1 (the host's check)
    const int32_t excl = exclude_ids ? exclude_ids[q] : -1;
    const int64_t stride = (int64_t)gridDim.x * kAlWaves;
    const int64_t last_row = n_rows - 1;
    Hit kept = Hit::pad();
    int32_t n_hits = 0;
    int64_t r = (int64_t)bx * kAlWaves + wv;
    Row row = load_row(rows + (r < n_rows ? r : last_row));
    while (r < n_rows) {                      // wave-uniform: no block barrier inside
        const int64_t rn = r + stride;
        const Row nrow = load_row(rows + (rn < n_rows ? rn : last_row));      // lands while this row votes
        const int64_t *rk = keys + row.off;
        AlKeyRange kr{0.0, 0.0};
        if constexpr (kWindowed) kr = al_key_range(rk, row.len, lane);
        unsigned long long best = 0;                                          // of the row: the kept rate's
        uint32_t best_rate = 0;
        int ri = 0;
        do {                                                                  // wave-uniform; one round without rates
            double rho = 1.0;
            if constexpr (kRates) {
                rho = rates.r[ri];
                x_min = al_x<true>(s, 0, rho);                                // the products stay sorted (header comment)
                x_max = al_x<true>(s, m - 1, rho);
            }
            int w0 = 0, w1 = 0;                                               // the one window [-B, B]
            if constexpr (kWindowed) {
                // the row's offset range [bin(c_min, x_max), bin(c_max, x_min)], clipped to [-B, B]; a NaN end (inf -
                // inf) clips to the bound
                const double d_lo = al_bin(kr.c_min, x_max, eps), d_hi = al_bin(kr.c_max, x_min, eps);
                const double r_lo = d_lo >= -Bd ? d_lo : -Bd, r_hi = d_hi <= Bd ? d_hi : Bd;
                w1 = -1;                                                      // no window: an empty row, a range outside
                if (row.len > 0 && r_lo <= r_hi) {                            // -B <= r_lo <= r_hi <= B: both finite
                    w0 = ((int)r_lo + B) / w.width;
                    w1 = ((int)r_hi + B) / w.width;
                }
                w0 = __builtin_amdgcn_readfirstlane(w0);                      // (equal in every lane already)
                w1 = __builtin_amdgcn_readfirstlane(w1);
                w1 = w1 < w.max_windows - 1 ? w1 : w.max_windows - 1;         // (never: (2B) / w.width is the last window)
            }
            unsigned long long rbest = 0;                                     // of this rate
            // kTwoBins: the lane's best window (J, h << 33 | 2^33 - 1 - order), and the count of the bin above the
            // window's top slot - the lowest bin of the window visited before (the one above), 0 for the first
            [[maybe_unused]] uint32_t jbest = 0;
            [[maybe_unused]] uint32_t carry = 0;
            for (int wi = w1; wi >= w0; --wi) {                               // wave-uniform, at most w.max_windows rounds
                int w_lo = -B, w_hi = B;
                if constexpr (kWindowed) {
                    w_lo = wi * w.width - B;                                  // >= -B
                    w_hi = w_lo + w.width - 1 < B ? w_lo + w.width - 1 : B;
                }
                const double lo_d = (double)w_lo, hi_d = (double)w_hi;
                for (int j = lane; j < row.len; j += 64) {
                    const double c = __longlong_as_double(rk[j]);
                    const bool kept_pos = kWindowed && j < w.resume_keys;     // (the same in every lane of a round)
                    // (w1 is this rate's: the positions another rate left are never read)
                    int t = kept_pos && wi != w1 ? (int)w.resume[j] : al_lo<kRates>(s, m, c, eps, hi_d, rho);
                    for (; t < m; ++t) {
                        const double d = al_bin(c, al_x<kRates>(s, t, rho), eps);
                        if (!(d >= lo_d)) break;                              // behind the window (or NaN there)
                        if (!(d <= hi_d)) continue;                           // (never, behind al_lo: keeps the index in bounds)
                        const int bin = (int)d;                               // w_lo <= bin <= w_hi
                        const uint32_t slot = (uint32_t)(bin - w_lo);         // 0 .. w.width - 1
                        const uint32_t cnt = atomicAdd(&w.hist[slot], 1u) + 1u;
                        if (cnt == 1u) w.dirty[atomicAdd(w.n_dirty, 1u)] = (uint16_t)slot;  // at most once per slot: < w.width
                        if constexpr (!kTwoBins) {
                            const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                            const unsigned long long key = ((unsigned long long)cnt << 33) | (kAlOrderMask - order);
                            rbest = key > rbest ? key : rbest;
                        }
                    }
                    if constexpr (kWindowed) {
                        if (kept_pos) w.resume[j] = (uint16_t)t;              // t <= m <= 4095
                    }
                }
                // LDS ops of one wave complete in order: the notes above are visible to the clearing below
                wave_lds_fence();
                const int nd = (int)*w.n_dirty;
                if constexpr (kTwoBins) {
                    // every count is final: the window of two bins that starts at each touched bin, J = h[b] + h[b + 1].
                    // Slot + 1 inside the histogram is bin b + 1 or a slot no vote reaches (beyond B: 0); behind its
                    // last slot b + 1 is the lowest bin of the window above, whose count is the carry
                    for (int i = lane; i < nd; i += 64) {
                        const int slot = (int)w.dirty[i];                     // < w.width
                        const uint32_t h = w.hist[slot];
                        const uint32_t up = slot + 1 < w.width ? w.hist[slot + 1] : carry;
                        const int bin = w_lo + slot;
                        const uint32_t order = 2u * (uint32_t)(bin < 0 ? -bin : bin) + (bin > 0 ? 1u : 0u);
                        const uint32_t j = h + up;
                        const unsigned long long key = ((unsigned long long)h << 33) | (kAlOrderMask - order);
                        const bool better = j > jbest || (j == jbest && key > rbest);
                        jbest = better ? j : jbest;
                        rbest = better ? key : rbest;
                    }
                    carry = w.hist[0];                                        // (the same word in every lane)
                }
                for (int i = lane; i < nd; i += 64) w.hist[w.dirty[i]] = 0;
                wave_lds_fence();
                if (lane == 0) *w.n_dirty = 0;
            }
            if constexpr (kTwoBins) {
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t oj = __shfl_xor(jbest, off);
                    const unsigned long long o = __shfl_xor(rbest, off);
                    const bool better = oj > jbest || (oj == jbest && o > rbest);
                    jbest = better ? oj : jbest;
                    rbest = better ? o : rbest;
                }
                rbest = ((unsigned long long)jbest << 33) | (rbest & kAlOrderMask);   // the window's count and its lower bin
            } else {
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(rbest, off);
                    rbest = o > rbest ? o : rbest;
                }
            }
            if constexpr (kRates) {
                if ((rbest >> 33) > (best >> 33)) {                           // strictly more votes: a tie keeps the
                    best = rbest;                                             // smaller index (wave-uniform)
                    best_rate = (uint32_t)ri;
                }
            } else {
                best = rbest;
            }
        } while (kRates && ++ri < n_rates);
        const uint32_t votes = (uint32_t)(best >> 33);
        const uint32_t rl = (uint32_t)row.len;
        uint32_t v = votes < (uint32_t)m ? votes : (uint32_t)m;
        v = v < rl ? v : rl;
        if (v >= (uint32_t)min_votes && row.vid != excl) {                  // min_votes >= 1: v >= 1, so m, rl, u >= 1
            const uint32_t u = contain ? ((uint32_t)m < rl ? (uint32_t)m : rl) : (uint32_t)m + rl - v;
            uint32_t score = (v << 20) / u;                                 // v <= 4095: the shift fits 32 bits; v <= u
            if constexpr (kSpan) {
                // the span needs the row's best bin and rate, so it is one more walk of the row: only for a row that
                // can still be a hit - the local score is made from the span, every other score decides first
                if (local || score >= (uint32_t)min_score) {
                    const int bin = al_best_bin(best);
                    // kTwoBins: the pairs of the window's two bins, the upper one only inside the range
                    const AlSpan sp = al_span<kTwoBins>(rk, row.len, s, m, eps, bin, rates.r[best_rate], lane,
                                                        bin < B ? bin + 1 : bin);
                    if (local) {                                            // 1 <= nq <= m, 1 <= nr <= rl: v only shrinks
                        const uint32_t nq = (uint32_t)(sp.t_last - sp.t_first + 1);
                        v = votes < nq ? votes : nq;
                        v = v < sp.nr ? v : sp.nr;
                        score = (v << 20) / (nq + sp.nr - v);
                    }
                    if (v >= (uint32_t)min_votes && score >= (uint32_t)min_score) {
                        const uint32_t x[3] = {(uint32_t)sp.t_first, (uint32_t)sp.t_last, sp.nr};
                        ++n_hits;
                        al_insert(kept, Hit::make(score, row.vid, bin, rl, votes, best_rate).with_more(x), k, lane);
                    }
                }
            } else if (score >= (uint32_t)min_score) {
                ++n_hits;
                al_insert(kept, Hit::make(score, row.vid, al_best_bin(best), rl, votes, best_rate), k, lane);
            }
        }
        row = nrow;
        r = rn;
    }
    if (lane == 0 && n_hits) atomicAdd(&s_nhits, n_hits);                    // LDS
    al_merge_waves<Hit, kAlWaves * 64>(kept, s_kept, wv, lane, k);
    if (wv == 0 && lane < k) kept.store(part, ((int64_t)q * n_lists + bx) * k + lane);
    if (threadIdx.x == 0 && s_nhits) atomicAdd(&totals[q], s_nhits);
}

// One block per query: the k smallest hits of its n_lists sorted partial lists -> d_out[q] = int32[k+1][Hit::kCols]
// (al_write_block).  A query the preparation refused (qm < 0 or > lds_keys): all padding, n_hits = INT32_MIN.
template <class Hit>
__device__ __forceinline__ void al_reduce(typename Hit::ConstParts part, int32_t n_lists, int32_t k, const int32_t *__restrict__ qm,
                                          int32_t lds_keys, const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    __shared__ typename Hit::template Lists<kAlReduceWaves * 64> s_kept;
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int32_t m = qm[q];
    const bool refused = m < 0 || m > lds_keys;
    Hit kept = Hit::pad();
    if (!refused && m > 0) {                                                 // (an empty query's lists were never written)
        const int64_t base = (int64_t)q * n_lists;
        for (int l0 = wv; l0 < n_lists; l0 += kAlReduceLd * kAlReduceWaves) {   // wave-uniform
            Hit e[kAlReduceLd];
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {
                const int l = l0 + j * kAlReduceWaves;
                e[j] = l < n_lists && lane < k ? Hit::load(part, (base + l) * k + lane) : Hit::pad();
            }
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) al_take(kept, e[j], k, lane);
        }
    }
    al_merge_waves<Hit, kAlReduceWaves * 64>(kept, s_kept, wv, lane, k);
    if (wv == 0) al_write_block(kept, d_out + (int64_t)q * (k + 1) * Hit::kCols, k, lane, refused ? INT32_MIN : totals[q]);
}

// The eight entry points only forward (and the three of TVZ_ALIGN_TWO_BINS behind them).  part_w / part_p:
// uint64[Q][n_lists][k], part_v / part_r: uint32[Q][n_lists][k].
__global__ __launch_bounds__(kAlBlock) void ts_align_topk_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t min_votes, int32_t min_score, const int32_t *__restrict__ exclude_ids, int32_t k,
    unsigned long long *__restrict__ part_w, unsigned long long *__restrict__ part_p, int32_t n_lists,
    int32_t *__restrict__ totals) {
    al_sweep<AlHit, false>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, al_bins_padded(B), min_votes, min_score,
                           /* contain */ false, exclude_ids, k, AlHit::Parts{part_w, part_p}, n_lists, totals);
}

__global__ __launch_bounds__(kAlReduceBlock) void ts_align_topk_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p, int32_t n_lists,
    int32_t k, const int32_t *__restrict__ qm, int32_t lds_keys, const int32_t *__restrict__ totals,
    int32_t *__restrict__ d_out) {
    al_reduce<AlHit>(AlHit::ConstParts{part_w, part_p}, n_lists, k, qm, lds_keys, totals, d_out);
}

__global__ __launch_bounds__(kAlBlock) void ts_alignw_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, int32_t min_votes, int32_t min_score, uint32_t flags, const int32_t *__restrict__ exclude_ids,
    int32_t k, unsigned long long *__restrict__ part_w, unsigned long long *__restrict__ part_p,
    uint32_t *__restrict__ part_v, int32_t n_lists, int32_t *__restrict__ totals) {
    al_sweep<AwHit, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes, min_score,
                          (flags & kAwContain) != 0u, exclude_ids, k, AwHit::Parts{part_w, part_p, part_v}, n_lists, totals);
}

__global__ __launch_bounds__(kAlReduceBlock) void ts_alignw_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p,
    const uint32_t *__restrict__ part_v, int32_t n_lists, int32_t k, const int32_t *__restrict__ qm, int32_t lds_keys,
    const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    al_reduce<AwHit>(AwHit::ConstParts{part_w, part_p, part_v}, n_lists, k, qm, lds_keys, totals, d_out);
}

__global__ __launch_bounds__(kAlBlock) void ts_alignr_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, AlRates rates, int32_t min_votes, int32_t min_score, uint32_t flags,
    const int32_t *__restrict__ exclude_ids, int32_t k, unsigned long long *__restrict__ part_w,
    unsigned long long *__restrict__ part_p, uint32_t *__restrict__ part_v, uint32_t *__restrict__ part_r, int32_t n_lists,
    int32_t *__restrict__ totals) {
    al_sweep<ArHit, true, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes, min_score,
                                (flags & kAwContain) != 0u, exclude_ids, k, ArHit::Parts{part_w, part_p, part_v, part_r},
                                n_lists, totals, rates);
}

__global__ __launch_bounds__(kAlReduceBlock) void ts_alignr_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p,
    const uint32_t *__restrict__ part_v, const uint32_t *__restrict__ part_r, int32_t n_lists, int32_t k,
    const int32_t *__restrict__ qm, int32_t lds_keys, const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    al_reduce<ArHit>(ArHit::ConstParts{part_w, part_p, part_v, part_r}, n_lists, k, qm, lds_keys, totals, d_out);
}

// (part_t / part_n: uint32[Q][n_lists][k], the span's two index ends in one word and its count of row keys)
__global__ __launch_bounds__(kAlBlock) void ts_aligns_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, AlRates rates, int32_t min_votes, int32_t min_score, uint32_t flags,
    const int32_t *__restrict__ exclude_ids, int32_t k, unsigned long long *__restrict__ part_w,
    unsigned long long *__restrict__ part_p, uint32_t *__restrict__ part_v, uint32_t *__restrict__ part_r,
    uint32_t *__restrict__ part_t, uint32_t *__restrict__ part_n, int32_t n_lists, int32_t *__restrict__ totals) {
    al_sweep<AsHit, true, true, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes, min_score,
                                      (flags & kAwContain) != 0u, exclude_ids, k,
                                      AsHit::Parts{part_w, part_p, part_v, part_r, part_t, part_n}, n_lists, totals, rates,
                                      (flags & kAsLocal) != 0u);
}

__global__ __launch_bounds__(kAlReduceBlock) void ts_aligns_reduce_kernel(
    const unsigned long long *__restrict__ part_w, const unsigned long long *__restrict__ part_p,
    const uint32_t *__restrict__ part_v, const uint32_t *__restrict__ part_r, const uint32_t *__restrict__ part_t,
    const uint32_t *__restrict__ part_n, int32_t n_lists, int32_t k, const int32_t *__restrict__ qm, int32_t lds_keys,
    const int32_t *__restrict__ totals, int32_t *__restrict__ d_out) {
    al_reduce<AsHit>(AsHit::ConstParts{part_w, part_p, part_v, part_r, part_t, part_n}, n_lists, k, qm, lds_keys, totals,
                     d_out);
}

// The sweeps under TVZ_ALIGN_TWO_BINS: the three above with al_sweep's kTwoBins, kernels of their own so
// that the ones above keep their code.  Their lists go through the same selections and merges.
__global__ __launch_bounds__(kAlBlock) void ts_alignw2_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, int32_t min_votes, int32_t min_score, uint32_t flags, const int32_t *__restrict__ exclude_ids,
    int32_t k, unsigned long long *__restrict__ part_w, unsigned long long *__restrict__ part_p,
    uint32_t *__restrict__ part_v, int32_t n_lists, int32_t *__restrict__ totals) {
    al_sweep<AwHit, true, false, false, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes,
                                              min_score, (flags & kAwContain) != 0u, exclude_ids, k,
                                              AwHit::Parts{part_w, part_p, part_v}, n_lists, totals);
}

__global__ __launch_bounds__(kAlBlock) void ts_alignr2_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, AlRates rates, int32_t min_votes, int32_t min_score, uint32_t flags,
    const int32_t *__restrict__ exclude_ids, int32_t k, unsigned long long *__restrict__ part_w,
    unsigned long long *__restrict__ part_p, uint32_t *__restrict__ part_v, uint32_t *__restrict__ part_r, int32_t n_lists,
    int32_t *__restrict__ totals) {
    al_sweep<ArHit, true, true, false, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes,
                                             min_score, (flags & kAwContain) != 0u, exclude_ids, k,
                                             ArHit::Parts{part_w, part_p, part_v, part_r}, n_lists, totals, rates);
}

__global__ __launch_bounds__(kAlBlock) void ts_aligns2_sweep_kernel(
    const Row *__restrict__ rows, int64_t n_rows, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm, int32_t lds_keys, double eps, int32_t B,
    int32_t width, AlRates rates, int32_t min_votes, int32_t min_score, uint32_t flags,
    const int32_t *__restrict__ exclude_ids, int32_t k, unsigned long long *__restrict__ part_w,
    unsigned long long *__restrict__ part_p, uint32_t *__restrict__ part_v, uint32_t *__restrict__ part_r,
    uint32_t *__restrict__ part_t, uint32_t *__restrict__ part_n, int32_t n_lists, int32_t *__restrict__ totals) {
    al_sweep<AsHit, true, true, true, true>(rows, n_rows, keys, sv, q_offsets, qm, lds_keys, eps, B, width, min_votes,
                                            min_score, (flags & kAwContain) != 0u, exclude_ids, k,
                                            AsHit::Parts{part_w, part_p, part_v, part_r, part_t, part_n}, n_lists, totals,
                                            rates, (flags & kAsLocal) != 0u);
}

// ---- the merge of the shards' blocks (every form's tvz_align_*_topk_merge) -------------------------------------------
constexpr int kAlMergeBlock = 256;
constexpr int kAlMergeWaves = kAlMergeBlock / 64;      // queries per block: a wave each
constexpr int kAlMergeMaxLists = 16;                   // one n_hits per lane, far below a wave

// gathered int32[n_lists][Q][k+1][4], every [k+1][4] block as al_reduce<Hit> writes it (k rows ascending in Hit's
// order, padding, then (-1, n_hits, 0, 0)) -> d_topk int32[Q][k][4], d_totals int32[Q].  One wave per query, no LDS,
// no barrier.  A block row does not carry its order word - the score depends on nv, the query's count of non-NaN
// values, which no block holds - so the wave counts nv from the query itself and rebuilds the hit with the sweep's
// expressions (Hit::make; contain: the wide call's TVZ_ALIGN_CONTAIN, u = min(nv, row_len) instead of nv + row_len -
// v); a row with video_id < 0 is padding wherever it stands, and so is one whose u would be 0 (nothing divides by
// zero): neither is live.  The lists are SORTED BY CONTRACT, in the order of the SAME score kind: that is the
// precondition of the fold's early exit (al_take_live, as al_take).  Equal hits are identical rows and are all kept.
// d_totals[q] = the lists' n_hits summed in 64 bits, clamped to INT32_MAX.  Refused - all k rows padding, d_totals[q]
// = INT32_MIN - when a list's n_hits is negative (INT32_MIN: a rank refused the query) or the query is longer than
// kAlMaxLen.  n_lists <= kAlMergeMaxLists, k <= kAlMaxK; gathered and d_topk 16-byte aligned.  AlHit's word holds a
// bin of 12 bits: blocks with a bin outside +-2047 (the wide call's) are AwHit's alone.
// ArHit's blocks have rows of five columns, 20 bytes - read and written word by word, only the base pointers are
// aligned -, and the fifth, the rate's index, is carried into the hit's order and out again, never interpreted.
// AsHit's have eight, 32 bytes, read and written the same way; its three span columns are carried likewise, and under
// TVZ_ALIGN_LOCAL the score is rebuilt from them (al_row_score).

// A block row's score under the call's score kind, rebuilt from its columns (x: the columns
// behind the rate's; nv: the query's non-NaN count), and whether the row is live.  AsHit's with TVZ_ALIGN_LOCAL: v =
// min(votes, nq, nr), u = nq + nr - v with nq = t_last - t_first + 1, in 64 bits - a block is the caller's memory, and
// any columns must do no harm; nq <= 0 or nr <= 0 is padding.  An AsHit row whose t_first or t_last lies outside 0 ..
// kAlMaxLen - 1 - the call writes none - does not fit the hit's word and is padding under every flag.
struct AlRowScore {
    uint32_t score;
    bool hit;
};
template <class Hit>
__device__ __forceinline__ AlRowScore al_row_score(int32_t vid, uint32_t rl, uint32_t votes, const uint32_t *x, uint32_t nv,
                                                   bool contain, bool local) {
    if constexpr (std::is_same_v<Hit, AsHit>) {
        const bool fits = x[0] < (uint32_t)kAlMaxLen && x[1] < (uint32_t)kAlMaxLen;
        if (local || !fits) {
            const long long nq = (long long)x[1] - (long long)x[0] + 1, nr = (int32_t)x[2];
            long long v = (long long)votes < nq ? (long long)votes : nq;
            v = v < nr ? v : nr;
            const bool hit = vid >= 0 && fits && nq > 0 && nr > 0;         // then 0 <= v <= u = nq + nr - v, u >= 1
            return {hit ? (uint32_t)((v << 20) / (nq + nr - v)) : 0u, hit};
        }
    }
    uint32_t v = votes < nv ? votes : nv;
    v = v < rl ? v : rl;
    const uint32_t u = contain ? (nv < rl ? nv : rl) : nv + rl - v;
    const bool hit = vid >= 0 && u != 0u;
    const uint32_t score = hit ? (v << 20) / u : 0u;                       // v <= nv <= 4095: the shift fits 32 bits
    return {score, hit};
}

template <class Hit>
__device__ __forceinline__ void al_merge_blocks(const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k,
                                                const double *__restrict__ queries, const int64_t *__restrict__ q_offsets,
                                                bool contain, int32_t *__restrict__ d_topk, int32_t *__restrict__ d_totals,
                                                bool local = false) {
    constexpr int kExtra = Hit::kCols - 4;                         // the columns behind the first four: the rate's index,
    constexpr int kMore = kExtra > 1 ? kExtra - 1 : 0;             // ... and those behind it
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kAlMergeWaves + (threadIdx.x >> 6);
    if (q >= Q) return;                                            // wave-uniform
    const int64_t k1 = (int64_t)k + 1;
    const int4 *blocks = reinterpret_cast<const int4 *>(gathered);            // [n_lists][Q][k+1] rows of 16 bytes (kCols = 4)
    // the lists' totals, one per lane; a negative one refuses the query
    const int32_t nh = lane < n_lists ? gathered[(((int64_t)lane * Q + q) * k1 + k) * Hit::kCols + 1] : 0;
    long long total = nh;
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    const int64_t qo = q_offsets[q];
    const int64_t len = q_offsets[q + 1] - qo;
    const bool refused = __ballot(nh < 0) != 0ull || len > kAlMaxLen;
    Hit kept = Hit::pad();
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
            uint32_t rate[kAlReduceLd];
            uint32_t more[kAlReduceLd][kMore ? kMore : 1];
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {                // the loads of kAlReduceLd lists in flight together
                const int l = l0 + j;
                rate[j] = 0u;
#pragma unroll
                for (int i = 0; i < kMore; ++i) more[j][i] = 0u;
                if constexpr (kExtra == 0) {
                    row[j] = l < n_lists && lane < k ? blocks[((int64_t)l * Q + q) * k1 + lane] : make_int4(-1, 0, 0, 0);
                } else {
                    row[j] = make_int4(-1, 0, 0, 0);
                    if (l < n_lists && lane < k) {                 // rows of 20 bytes: word loads
                        const int32_t *p = gathered + (((int64_t)l * Q + q) * k1 + lane) * Hit::kCols;
                        row[j] = make_int4(p[0], p[1], p[2], p[3]);
                        rate[j] = (uint32_t)p[4];
#pragma unroll
                        for (int i = 0; i < kMore; ++i) more[j][i] = (uint32_t)p[5 + i];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kAlReduceLd; ++j) {
                const uint32_t rl = (uint32_t)row[j].y, votes = (uint32_t)row[j].w;
                const AlRowScore sc = al_row_score<Hit>(row[j].x, rl, votes, more[j], nv, contain, local);
                if constexpr (kMore == 0)
                    al_take_live(kept, Hit::make(sc.score, row[j].x, row[j].z, rl, votes, rate[j]), __ballot(sc.hit), k, lane);
                else
                    al_take_live(kept, Hit::make(sc.score, row[j].x, row[j].z, rl, votes, rate[j]).with_more(more[j]),
                                 __ballot(sc.hit), k, lane);
            }
        }
    }
    if constexpr (kExtra == 0) {
        if (lane < k) reinterpret_cast<int4 *>(d_topk)[(int64_t)q * k + lane] = kept.row();
    } else if (lane < k) {
        const int4 o = kept.row();
        int32_t *out = d_topk + ((int64_t)q * k + lane) * Hit::kCols;
        out[0] = o.x;
        out[1] = o.y;
        out[2] = o.z;
        out[3] = o.w;
#pragma unroll
        for (int i = 0; i < kExtra; ++i) out[4 + i] = kept.extra(i);
    }
    if (lane == 0) d_totals[q] = refused ? INT32_MIN : (int32_t)(total > INT32_MAX ? INT32_MAX : total);
}

// The four entry points only forward.
__global__ __launch_bounds__(kAlMergeBlock) void ts_align_topk_merge_kernel(
    const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k, const double *__restrict__ queries,
    const int64_t *__restrict__ q_offsets, int32_t *__restrict__ d_topk, int32_t *__restrict__ d_totals) {
    al_merge_blocks<AlHit>(gathered, n_lists, Q, k, queries, q_offsets, /* contain */ false, d_topk, d_totals);
}

__global__ __launch_bounds__(kAlMergeBlock) void ts_alignw_merge_kernel(
    const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
    const double *__restrict__ queries, const int64_t *__restrict__ q_offsets, int32_t *__restrict__ d_topk,
    int32_t *__restrict__ d_totals) {
    al_merge_blocks<AwHit>(gathered, n_lists, Q, k, queries, q_offsets, (flags & kAwContain) != 0u, d_topk, d_totals);
}

__global__ __launch_bounds__(kAlMergeBlock) void ts_alignr_merge_kernel(
    const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
    const double *__restrict__ queries, const int64_t *__restrict__ q_offsets, int32_t *__restrict__ d_topk,
    int32_t *__restrict__ d_totals) {
    al_merge_blocks<ArHit>(gathered, n_lists, Q, k, queries, q_offsets, (flags & kAwContain) != 0u, d_topk, d_totals);
}

__global__ __launch_bounds__(kAlMergeBlock) void ts_aligns_merge_kernel(
    const int32_t *__restrict__ gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
    const double *__restrict__ queries, const int64_t *__restrict__ q_offsets, int32_t *__restrict__ d_topk,
    int32_t *__restrict__ d_totals) {
    al_merge_blocks<AsHit>(gathered, n_lists, Q, k, queries, q_offsets, (flags & kAwContain) != 0u, d_topk, d_totals,
                           (flags & kAsLocal) != 0u);
}

}  // namespace
