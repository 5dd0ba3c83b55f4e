// sed_lane_dp.h - the cells of the short-sequence kernels, shared by the lane kernels (sed_lane.hip: one lane per pair)
// and the similarity joins (sed_join.hip, sed_join_long.hip: one lane per column sequence, the wave walking the rows):
// one copy of the bit-parallel unit-cost step and of the scaled-integer row, from the per-column setup to the sink's
// decoding.  The comments on the recurrences are at the kernels in sed_lane.hip.
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

// ---- bit-parallel unit-cost distance (Myers 1999 / Hyyro; str2 = the bit dimension, 32 columns a word) ----
// One 32-bit word of one row of str1: tq = ~Eq, the complement of the row symbol's match mask over the word's bits of
// str2.  A column of more than 32 symbols is several words, run from the lowest up: cadd carries the step's one addition
// into the next word, cph and cmh carry the top bits the two left shifts push out.  Into word 0 go cadd = 0, cph = 1 (the
// top border's +1) and cmh = 0.
__device__ __forceinline__ void sed_bitpar_word(uint32_t &Pv, uint32_t &Mv, uint32_t tq, uint32_t &cadd, uint32_t &cph,
                                                uint32_t &cmh) {
    const uint32_t Xv = Mv | ~tq;
    const unsigned long long s = (unsigned long long)(Pv & ~tq) + Pv + cadd;
    cadd = (uint32_t)(s >> 32);
    const uint32_t Xh = ((uint32_t)s ^ Pv) | ~tq;
    const uint32_t ph = Mv | ~(Xh | Pv), mh = Pv & Xh;
    const uint32_t Ph = ph << 1 | cph;
    const uint32_t Mh = mh << 1 | cmh;
    cph = ph >> 31;
    cmh = mh >> 31;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}
// One row of str1 over a single word (m <= 32)
__device__ __forceinline__ void sed_bitpar_step(uint32_t &Pv, uint32_t &Mv, uint32_t tq) {
    uint32_t cadd = 0, cph = 1u, cmh = 0;
    sed_bitpar_word(Pv, Mv, tq, cadd, cph, cmh);
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
// Columns J0 + 1 .. J1 of one row in place.  addend(j) = the update addend of column j + 1, whose symbol is str2[j]:
// ((cost - ins - del) << 16) - 1; the candidates left (insert) and up (delete) carry none.  In: left = the row's V[J0],
// dg = the update candidate of column J0 + 1 (the previous row's V[J0] + addend(J0)); out: the same two for column J1.
template <int MM, int J0, int J1, class Addend>
__device__ __forceinline__ void sed_scaled_cols(uint32_t (&V)[MM + 1], uint32_t &left, uint32_t &dg, Addend addend) {
#pragma unroll
    for (int j = J0 + 1; j <= J1; ++j) {
        const uint32_t up = V[j];
        const uint32_t dnext = j < MM ? up + addend(j) : 0u;
        const uint32_t v = umin3(left, up, dg);
        dg = dnext;
        V[j] = v;
        left = v;
    }
}
// One row in place: cur = the row symbol's 8 cost bytes (sed_scaled_params::row), V[0] stays the offset key B.
template <int MM>
__device__ __forceinline__ void sed_scaled_row(uint32_t (&V)[MM + 1], const uint32_t (&sel)[MM], uint2 cur) {
    uint32_t dg = V[0] + __builtin_amdgcn_perm(cur.y, cur.x, sel[0]);
    uint32_t left = V[0];  // stays B
    sed_scaled_cols<MM, 0, MM>(V, left, dg, [&](int j) { return __builtin_amdgcn_perm(cur.y, cur.x, sel[j]); });
}
// The scaled distance D * S from the sink's key (ins, del on the integer scale)
__device__ __forceinline__ uint32_t sed_scaled_decode(uint32_t cap, int n, int m, uint32_t ins, uint32_t del) {
    return (cap - SED_KB + (((uint32_t)n * del + (uint32_t)m * ins) << 16) + 0xFFFFu) >> 16;
}
