// tvz_wave.h — wave64 and 16-lane-group primitives shared by the matcher's kernel headers (gfx950).
// Every header that uses one of them includes this file itself.
//
// A "group" is one DPP row: 16 consecutive lanes, the unit that owns a corpus row in the sweeps.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

// LDS counters updated by other lanes of the SAME wave are read back by plain loads: make the
// compiler keep the order (the hardware completes a wave's LDS operations in order).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// set bits of a ballot below this lane: the lane's place among the lanes that voted
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- DPP moves, `old` = 0: a lane without a valid source, or in a row that ROW_MASK leaves out, reads 0
// whichever way BOUND_CTRL says.  The permutations inside a row have no invalid source.
template <int CTRL, bool BOUND_CTRL = true, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp16(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, BOUND_CTRL);
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp16_64(unsigned long long v) {
    return ((unsigned long long)dpp16<CTRL>((uint32_t)(v >> 32)) << 32) | dpp16<CTRL>((uint32_t)v);
}
// the value of the lane before this one in the group; lane 0 takes lane 15's
__device__ __forceinline__ uint32_t group16_prev(uint32_t v) { return dpp16<0x121, false>(v); }   // row_ror:1

// ---- wave64 inclusive prefix sum on the VALU (six DPP adds: row_shr 1/2/4/8 inside the 16-lane rows,
// then row_bcast 15 and 31 across them).  A __shfl_up ladder is six ds_bpermute round trips through
// the LDS crossbar (~100 cycles each, and LDS-pipe time): the index lookup runs five scans per
// sub-index and was paying ~3,000 cycles of pure latency for them.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add_u32(uint32_t v) {
    return v + dpp16<CTRL, false, ROW_MASK>(v);      // lanes whose source is invalid or masked add 0
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v = dpp_add_u32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add_u32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add_u32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add_u32<0x118, 0xf>(v);  // row_shr:8   -> inclusive scan inside each row
    v = dpp_add_u32<0x142, 0xa>(v);  // row_bcast:15 into rows 1,3
    v = dpp_add_u32<0x143, 0xc>(v);  // row_bcast:31 into rows 2,3
    return v;
}
__device__ __forceinline__ uint32_t wave_total(uint32_t incl) {       // of an inclusive scan
    return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
}

// ---- sums over the waves of a block, through one LDS word per wave: lane 63 of every wave posts the total of its
// inclusive scan; behind a block barrier every thread reads the sum of the waves before its own, and of all
template <int WAVES>
__device__ __forceinline__ void waves_sum(const uint32_t *s_w, int wave, uint32_t &before, uint32_t &all) {
    before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t a = s_w[w];
        if (w < wave) before += a;
        all += a;
    }
}

// ---- butterfly over a group: after the four steps every lane holds the reduction of all 16; each
// step combines two DISJOINT sets of lanes (needed for the second-smallest and top-5 merges)
#define TVZ_ROW16_BUTTERFLY(STEP) \
    STEP(0xB1)  /* quad_perm [1,0,3,2] */ \
    STEP(0x4E)  /* quad_perm [2,3,0,1] */ \
    STEP(0x141) /* row_half_mirror     */ \
    STEP(0x140) /* row_mirror          */

template <typename T>
__device__ __forceinline__ T group16_sum(T v) {
#define TVZ_SUM_STEP(C) v += (T)dpp16<C>((uint32_t)v);
    TVZ_ROW16_BUTTERFLY(TVZ_SUM_STEP)
#undef TVZ_SUM_STEP
    return v;
}

// (m1, m2) = every lane's smallest and second smallest value -> the group's
__device__ __forceinline__ void group16_min2(uint32_t &m1, uint32_t &m2) {
#define TVZ_M2_STEP(C) { const uint32_t p1 = dpp16<C>(m1), p2 = dpp16<C>(m2); \
    const uint32_t lo = m1 < p1 ? m1 : p1, hi = m1 < p1 ? p1 : m1, r2 = m2 < p2 ? m2 : p2; \
    m1 = lo; m2 = hi < r2 ? hi : r2; }
    TVZ_ROW16_BUTTERFLY(TVZ_M2_STEP)
#undef TVZ_M2_STEP
}

// ---- the FIVE smallest of a set of 12-bit values, packed as 5 x 12 bits in one 64-bit word (ascending
// from bit 0, 0xfff = none)
constexpr int kTop = 5;
constexpr unsigned long long kTopNone = 0x0fffffffffffffffULL;   // 5 fields of 0xfff

__device__ __forceinline__ unsigned long long top5_insert(unsigned long long p, uint32_t x) {
    uint32_t a[kTop];
#pragma unroll
    for (int i = 0; i < kTop; ++i) a[i] = (uint32_t)(p >> (12 * i)) & 0xfffu;
#pragma unroll
    for (int i = 0; i < kTop; ++i) {      // insertion network: keep the smaller, carry the larger
        const uint32_t lo = a[i] < x ? a[i] : x;
        x = a[i] < x ? x : a[i];
        a[i] = lo;
    }
    unsigned long long r = 0;
#pragma unroll
    for (int i = 0; i < kTop; ++i) r |= (unsigned long long)a[i] << (12 * i);
    return r;
}
// every lane's packed five -> the group's
__device__ __forceinline__ void group16_top5(unsigned long long &top) {
#define TVZ_T5_STEP(C) { const unsigned long long p = dpp16_64<C>(top); \
    _Pragma("unroll") for (int i = 0; i < kTop; ++i) top = top5_insert(top, (uint32_t)(p >> (12 * i)) & 0xfffu); }
    TVZ_ROW16_BUTTERFLY(TVZ_T5_STEP)
#undef TVZ_T5_STEP
}

}  // namespace
