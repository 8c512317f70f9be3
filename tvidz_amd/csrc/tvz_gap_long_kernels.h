// tvz_gap_long_kernels.h — the kernels of tvz_align_candidates_long (include/tvz_gap_long.h); gfx950, wave64.
//
//   ts_gapl_offsets_kernel  where every probe list goes: an exclusive scan of the probe slots of the Q S lists, S per
//                           query, list q S + s the slots of segment s of query q.
//   ts_gapl_probe_kernel    the probes: a thread per (query, position) writes its 8 slots into its segment's list.
//   (the internal match over the handle's code table: the probe lists are its queries)
//   ts_gapl_fold_kernel     per query its S hit lists SUMMED per id, the C best of the complete sums, the block, the total.
//
// The segment arithmetic is tvz_gap_codes.h's (long_segments, long_list_slots, long_list_of, long_place_of), the
// table's too (long_table_slots, long_table_home).  The kernels of tvz_gap_kernels.h are not touched: these are
// kernels of their own, not modes of those.  From tvz_topk_kernels.h: sort_and_keep, topk_total; from tvz_wave.h:
// wave_scan_incl, waves_sum; from tvz_align_kernels.h: al_scaled.  Included by tvz_match.hip behind tvz_gap_kernels.h.
#pragma once
#include "tvz_gap_kernels.h"

namespace {

// the probe slots of list s of a query of m sorted values; a refused query (m < 0) has none
__device__ __forceinline__ int32_t gapl_slots(int32_t m, int32_t s) { return tvz_gap::long_list_slots(m, s); }

// p_off[p] = the slots of the lists before p, p_off[Q S] = all of them; excl_out[p] = exclude_ids[p / S] where there is
// an array to copy (the lookup reads one id per probe list).  grid = 1; Q S <= 65,535: 64 per thread.
__global__ __launch_bounds__(kGapOffBlock) void ts_gapl_offsets_kernel(const int32_t *__restrict__ qm, int32_t Q, int32_t S,
                                                                        const int32_t *__restrict__ exclude_ids,
                                                                        int64_t *__restrict__ p_off,
                                                                        int32_t *__restrict__ excl_out) {
    __shared__ uint32_t s_w[kGapOffBlock / 64];
    const int n = Q * S;
    const int per = (n + kGapOffBlock - 1) / kGapOffBlock;
    const int p0 = (int)threadIdx.x * per;
    uint32_t mine = 0;
    for (int p = p0; p < p0 + per && p < n; ++p) mine += (uint32_t)gapl_slots(qm[p / S], p % S);
    const uint32_t incl = wave_scan_incl(mine);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before, all;
    waves_sum<kGapOffBlock / 64>(s_w, wave, before, all);
    uint32_t at = before + incl - mine;
    for (int p = p0; p < p0 + per && p < n; ++p) {
        p_off[p] = (int64_t)at;
        at += (uint32_t)gapl_slots(qm[p / S], p % S);
        if (excl_out) excl_out[p] = exclude_ids[p / S];
    }
    if (threadIdx.x == 0) p_off[n] = (int64_t)all;
}

// The query side of include/tvz_gap.h with ts_gapc_probe_kernel's expressions at the rate 1.0 (al_scaled(x, 1.0) == x;
// a choice with an invalid bin is the same NaN).  grid = (ceil(positions / kGapProbeBlock), Q); thread i of query q
// takes position i (i + 3 < m) and writes probes[p_off[q S + i / 511] + 8 (i % 511) ..+ 8): four 16-byte stores
// (p_off and the place are multiples of 8 slots).  A position's list has its slots by construction:
// i < m - 3 => 8 (i % 511) + 8 <= long_list_slots(m, i / 511).
__global__ __launch_bounds__(kGapProbeBlock) void ts_gapl_probe_kernel(const double *__restrict__ sv,
                                                                        const int64_t *__restrict__ q_offsets,
                                                                        const int32_t *__restrict__ qm, double gap_eps,
                                                                        int32_t S, const int64_t *__restrict__ p_off,
                                                                        double *__restrict__ probes) {
    const int q = blockIdx.y;
    const int32_t m = qm[q];
    if (m < 4) return;                                               // refused, or fewer than 4 values (block-uniform)
    const int i = (int)blockIdx.x * kGapProbeBlock + (int)threadIdx.x;
    if (i + 3 >= m) return;
    const double rho = 1.0;
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
    const int64_t p = (int64_t)q * S + tvz_gap::long_list_of(i);
    double2 *o = reinterpret_cast<double2 *>(probes + p_off[p] + tvz_gap::long_place_of(i));
#pragma unroll
    for (int v = 0; v < tvz_gap::kVariants; v += 2) {                // (NaN + x = NaN: an invalid choice poisons its slots)
        const double rest = ((v & 2) ? hi[1] : lo[1]) + ((v & 4) ? hi[2] : lo[2]);
        o[v >> 1] = make_double2(lo[0] + rest, hi[0] + rest);
    }
}

// ---- the fold ---------------------------------------------------------------------------------------------------------
constexpr int kGaplMaxLists = 9;                                     // S(4,095)
constexpr int kGaplScan = 4 * kBlock;                                // table slots looked at between two barriers

// Sums the n entries of a query into `tab` (slots: a power of two >= 2 n, zeroed here) and streams the occupied slots
// through key / cnt; -> the ids (block-uniform), `pos` the entries left in key / cnt.  An entry claims the first free
// slot from its id's home on (atomicCAS on the key word: 0 = empty, id + 1 otherwise) and adds its count there
// (atomicAdd); at most n <= slots / 2 keys are ever claimed, so the walk ends.  An id is ONE slot from then on, so
// keeping the C best of what was seen so far is exact.  Inlined once per address space of `tab` (LDS, global).
__device__ __forceinline__ int gapl_fold_table(int2 *tab, uint32_t slots, const int32_t *__restrict__ src,
                                               const int32_t *s_start, int n, int32_t cap, int32_t C, uint64_t *key,
                                               int32_t *cnt, int *s_fill, int &pos) {
    for (uint32_t i = threadIdx.x; i < slots; i += kBlock) tab[i] = make_int2(0, 0);
    __threadfence();                                                 // the zeros are where the atomics act (global: L2)
    __syncthreads();
    const uint32_t mask = slots - 1;
    for (int f = threadIdx.x; f < n; f += kBlock) {
        int i = 0;
        while (f >= s_start[i + 1]) ++i;                             // (f < n = s_start[S]: it ends)
        const int32_t *h = src + ((int64_t)i * cap + (f - s_start[i])) * 3;
        const int32_t vid = h[0], c = h[1];
        if (vid < 0) continue;
        const uint32_t k = (uint32_t)vid + 1u;
        uint32_t at = tvz_gap::long_table_home(k, slots);
        for (;;) {
            const uint32_t was = atomicCAS(reinterpret_cast<uint32_t *>(&tab[at].x), 0u, k);
            if (was == 0u || was == k) break;
            at = (at + 1) & mask;
        }
        atomicAdd(&tab[at].y, c);
    }
    __threadfence();
    __syncthreads();
    int ids = 0;
    for (uint32_t base = 0; base < slots; base += kGaplScan) {       // block-uniform
        if (threadIdx.x == 0) *s_fill = 0;
        __syncthreads();
        for (uint32_t i = base + threadIdx.x; i < base + kGaplScan && i < slots; i += kBlock) {
            // (read where the atomics acted, past this CU's vector cache: a relaxed load at device scope)
            const uint64_t word = __hip_atomic_load(reinterpret_cast<const uint64_t *>(&tab[i]), __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
            const int2 e = make_int2((int32_t)(uint32_t)word, (int32_t)(word >> 32));
            if (e.x == 0) continue;
            const int at = pos + atomicAdd(s_fill, 1);
            key[at] = ~(((uint64_t)(uint32_t)e.y << 32) | (uint32_t)(0x7fffffff - (e.x - 1)));
            cnt[at] = e.y;
        }
        __syncthreads();
        const int got = *s_fill;
        pos += got;
        ids += got;
        if (kSortCap - pos < kGaplScan) sort_and_keep(key, cnt, pos, C);     // (no room for another scan: keep the C best)
        __syncthreads();
    }
    return ids;
}

// grid = Q.  Query q's S hit lists hits[q S + s][min(hits_n[q S + s], cap)][3] = (video_id, count, kth), unordered, an
// id possibly in every one of them and in several rows of one -> out[q][C + 1][2] in ts_gapc_select_kernel's format:
// per id the SUM of its entries' counts, the C largest sums by the word sum << 32 | (2^31 - 1 - video_id), rows
// (video_id, sum), padding (-1, 0), and (-1, total): the distinct ids, or - when a list overflowed `cap` - the lists'
// true counts summed in 64 bits, negated (topk_total).  A sum fits 31 bits: the call refuses S x cap x 4,088 above
// INT32_MAX.  The table is in LDS where the query's n entries are at most kLongLdsEntries, in the query's
// `table_slots` slots of `table` otherwise (the host sizes them for S x cap entries).  A refused query folds nothing
// and goes through the same two store sites as every other.  One 8-byte store per row.
__global__ __launch_bounds__(kBlock) void ts_gapl_fold_kernel(const int32_t *__restrict__ hits,
                                                               const int32_t *__restrict__ hits_n,
                                                               const int32_t *__restrict__ qm, int32_t S, int32_t cap,
                                                               int32_t C, int2 *__restrict__ table, size_t table_slots,
                                                               int32_t *__restrict__ out) {
    __shared__ uint64_t key[kSortCap];
    __shared__ int32_t cnt[kSortCap];
    __shared__ int2 s_tab[tvz_gap::kLongLdsSlots];
    __shared__ int32_t s_start[kGaplMaxLists + 1];                   // where list s starts in the one sequence
    __shared__ int s_fill;
    const int q = blockIdx.x;
    int2 *o = reinterpret_cast<int2 *>(out) + (int64_t)q * (C + 1);
    const bool refused = qm[q] < 0;                                  // block-uniform, like everything up to the fold
    long long pairs = 0;
    bool over = false;
    int n = 0;
    for (int s = 0; s < S && !refused; ++s) {
        const int32_t t = hits_n[(int64_t)q * S + s];
        if (threadIdx.x == 0) s_start[s] = n;
        pairs += t < 0 ? 0 : t;
        over = over || t > cap;
        n += t > cap ? cap : (t < 0 ? 0 : t);                        // (at most S x cap: the host refuses what overflows)
    }
    if (threadIdx.x == 0) s_start[refused ? 0 : S] = n;
    __syncthreads();
    const int32_t *src = hits + (int64_t)q * S * cap * 3;            // list s starts at src + s * cap * 3
    int pos = 0, ids = 0;
    if (n > 0) {
        const uint32_t slots = tvz_gap::long_table_slots(n);
        if (n <= tvz_gap::kLongLdsEntries)
            ids = gapl_fold_table(s_tab, slots, src, s_start, n, cap, C, key, cnt, &s_fill, pos);
        else
            ids = gapl_fold_table(table + (size_t)q * table_slots, slots, src, s_start, n, cap, C, key, cnt, &s_fill, pos);
    }
    __syncthreads();
    sort_and_keep(key, cnt, pos, C);
    for (int i = threadIdx.x; i < C; i += kBlock) {
        const uint64_t w = i < pos ? ~key[i] : 0ULL;
        o[i] = w == 0ULL ? make_int2(-1, 0) : make_int2(0x7fffffff - (int32_t)(uint32_t)w, (int32_t)(w >> 32));
    }
    if (threadIdx.x == 0) o[C] = make_int2(-1, refused ? INT32_MIN : over ? topk_total(pairs, true) : topk_total(ids, false));
}

}  // namespace
