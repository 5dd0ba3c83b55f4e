// sed_lane_dp.h - the cells of the short-sequence kernels, shared by the lane kernels (sed_lane.hip: one lane per pair)
// and the similarity join (sed_join.hip: one lane per column sequence, the wave walking the rows): one copy of the
// bit-parallel unit-cost step and of the scaled-integer row, from the per-column setup to the sink's decoding.  The
// comments on the recurrences are at the kernels in sed_lane.hip.
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

// ---- bit-parallel unit-cost distance (Myers 1999 / Hyyro; str2 = the bit dimension, m <= 32) ----
// One row of str1: tq = ~Eq, the complement of the row symbol's match mask over str2's bits.
__device__ __forceinline__ void sed_bitpar_step(uint32_t &Pv, uint32_t &Mv, uint32_t tq) {
    const uint32_t Xv = Mv | ~tq;
    const uint32_t Xh = (((Pv & ~tq) + Pv) ^ Pv) | ~tq;
    const uint32_t Ph = (Mv | ~(Xh | Pv)) << 1 | 1u;  // (the top border's +1)
    const uint32_t Mh = (Pv & Xh) << 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}
// ~Eq of a row symbol with 2-bit code u over the columns' two bit planes
__device__ __forceinline__ uint32_t sed_bitpar_tq(uint32_t E0, uint32_t E1, uint32_t u) {
    return (E0 ^ (0u - (u & 1u))) | (E1 ^ (0u - (u >> 1)));
}
// D[n][m] from the vertical deltas of row n (row 0 is D[j] = j: Pv all ones, Mv 0); m = 0 gives n
__device__ __forceinline__ uint32_t sed_bitpar_sink(int n, int m, uint32_t Pv, uint32_t Mv) {
    const uint32_t keep = m >= 32 ? ~0u : (1u << m) - 1u;
    return (uint32_t)n + (uint32_t)__builtin_popcount(Pv & keep) - (uint32_t)__builtin_popcount(Mv & keep);
}

// ---- scaled-integer DP over an 8-symbol table (offset keys, 3 VALU per cell) ----
// The perm selector of a column whose symbol is b: byte 3 <- 0xFF, byte 2 <- table byte b, bytes 1:0 <- 0xFF
__device__ __forceinline__ uint32_t sed_scaled_sel(uint32_t b) { return 0x0D000D0Du | ((b & 7u) << 16); }
// One row in place: cur = the row symbol's 8 cost bytes (sed_scaled_params::row), V[0] stays the offset key B.
// The addend of the update candidate is ((cost - ins - del) << 16) - 1; the candidates left (insert) and up (delete)
// carry none.
template <int MM>
__device__ __forceinline__ void sed_scaled_row(uint32_t (&V)[MM + 1], const uint32_t (&sel)[MM], uint2 cur) {
    uint32_t dg = V[0] + __builtin_amdgcn_perm(cur.y, cur.x, sel[0]);
    uint32_t left = V[0];  // stays B
#pragma unroll
    for (int j = 1; j <= MM; ++j) {
        const uint32_t up = V[j];
        const uint32_t dnext = j < MM ? up + __builtin_amdgcn_perm(cur.y, cur.x, sel[j]) : 0u;
        const uint32_t v = umin3(left, up, dg);
        dg = dnext;
        V[j] = v;
        left = v;
    }
}
// The scaled distance D * S from the sink's key (ins, del on the integer scale)
__device__ __forceinline__ uint32_t sed_scaled_decode(uint32_t cap, int n, int m, uint32_t ins, uint32_t del) {
    return (cap - SED_KB + (((uint32_t)n * del + (uint32_t)m * ins) << 16) + 0xFFFFu) >> 16;
}
