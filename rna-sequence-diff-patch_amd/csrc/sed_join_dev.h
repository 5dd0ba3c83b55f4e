// sed_join_dev.h - what the integer join kernels share (sed_join.hip: columns of 0..32 symbols, sed_join_long.hip: 0..128):
// the append to the device hit list and the walk over a block's rows with the self rule, the length skip and the two
// counters.  One copy, so both kernels report the same pairs under the same rule (sed_internal.h: sed_join_args).
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

// One hit per lane, decided for the whole wave (sed_fit_dp.h: sed_fit_append): the first hitting lane takes popcount
// slots with one atomic add, every hitting lane stores at the first slot + its rank among them; slots >= cap only count.
__device__ __forceinline__ void sed_join_append(const sed_join_args &a, bool hit, int32_t row, int32_t col, uint32_t D) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(hit);
    if (b == 0) return;
    if (hit) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        unsigned long long base = 0;
        if (rank == 0) base = atomicAdd(a.count, (unsigned long long)__popcll(b));
        // (the first active lane here is the hitting lane of rank 0)
        const unsigned long long slot =
            (((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)base)) + rank;
        if (slot < a.cap) a.hits[slot] = make_uint4((uint32_t)row, (uint32_t)col, D, 0u);
    }
}

// The rows of this block's group against the lane's column (m symbols, original index orig; valid: the lane has one).
// Length skip: insert (m - n)+ + delete (n - m)+ bounds the distance from below, and a wave none of whose lanes can be
// within the cutoff for the current row leaves that row out.  count[1] counts the pairs whose bound passed: the pairs of
// the waves that ran.  pair(r, n) = the scaled distance D * S of row r (n symbols, uniform across the wave) and the
// lane's column; it runs with the whole wave active.
template <class Pair>
__device__ __forceinline__ void sed_join_rows(const int32_t *__restrict__ row_len, const sed_join_args &a, bool valid, int m,
                                              int orig, Pair pair) {
    const int rbeg = a.row0 + (int)blockIdx.y * SED_JOIN_G;
    const int rend = min(rbeg + SED_JOIN_G, a.row0 + a.nrows);
    uint32_t ran = 0;
    for (int r = rbeg; r < rend; ++r) {
        const int n = row_len[r];  // (uniform: a scalar load)
        const uint32_t lb = m > n ? (uint32_t)(m - n) * a.ins : (uint32_t)(n - m) * a.del;
        const bool go = valid && !(a.self && orig == r) && lb <= (uint32_t)a.cut;
        const unsigned long long gb = __builtin_amdgcn_ballot_w64(go);
        if (gb == 0) continue;  // no column of this wave can be within the cutoff of row r
        ran += (uint32_t)__popcll(gb);
        const uint32_t D = pair(r, n);
        sed_join_append(a, go && D <= (uint32_t)a.cut, r, orig, D);
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.count + 1, (unsigned long long)ran);
}
