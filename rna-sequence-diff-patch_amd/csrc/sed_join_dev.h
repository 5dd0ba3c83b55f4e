// sed_join_dev.h - what the join kernels share (sed_join.hip: columns of 0..32 symbols, sed_join_long.hip: 0..128,
// sed_join_f64.hip: the fp64 route): the append to the device hit list and the launch, for all three; the walk over a
// block's rows with the self rule, the length skip and the two counters, for the two integer units.  One copy, so the
// kernels report the same pairs under the same rule (sed_internal.h: sed_join_args, sed_join_f64_args).
// sed_join_f64_kernel keeps a row loop of its own: handed this walk with its skip, distance and hit test as parameters
// it compiled to another instruction schedule (profiles/kernel_shells/README.md).
#pragma once
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"

// One hit per lane, decided for the whole wave (sed_dev.h: wave_claim_slot); slots >= cap only count.  w2, w3 = the
// record's last two words: (D * S, 0) of the integer routes, D's low and high word of the fp64 route.
__device__ __forceinline__ void sed_join_append(const sed_join_list &out, bool hit, int32_t row, int32_t col, uint32_t w2,
                                                uint32_t w3) {
    unsigned long long slot;
    if (wave_claim_slot(out.count, hit, &slot) && slot < out.cap) out.hits[slot] = make_uint4((uint32_t)row, (uint32_t)col, w2, w3);
}

// The rows of this block's group against the lane's column (m symbols, original index orig; valid: the lane has one).
// Length skip: insert (m - n)+ + delete (n - m)+ bounds the distance from below, and a wave none of whose lanes can be
// within the cutoff for the current row leaves that row out.  count[1] counts the pairs whose bound passed: the pairs of
// the waves that ran.  pair(r, n) = the scaled distance D * S of row r (n symbols, uniform across the wave) and the
// lane's column; it runs with the whole wave active.
template <class Pair>
__device__ __forceinline__ void sed_join_rows(const int32_t *__restrict__ row_len, const sed_join_args &a, bool valid, int m,
                                              int orig, Pair pair) {
    const int rbeg = a.s.row0 + (int)blockIdx.y * SED_JOIN_G;
    const int rend = min(rbeg + SED_JOIN_G, a.s.row0 + a.s.nrows);
    uint32_t ran = 0;
    for (int r = rbeg; r < rend; ++r) {
        const int n = row_len[r];  // (uniform: a scalar load)
        const uint32_t lb = m > n ? (uint32_t)(m - n) * a.ins : (uint32_t)(n - m) * a.del;
        const bool go = valid && !(a.s.self && orig == r) && lb <= (uint32_t)a.cut;
        const unsigned long long gb = __builtin_amdgcn_ballot_w64(go);
        if (gb == 0) continue;  // no column of this wave can be within the cutoff of row r
        ran += (uint32_t)__popcll(gb);
        const uint32_t D = pair(r, n);
        sed_join_append(a.out, go && D <= (uint32_t)a.cut, r, orig, D, 0u);
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.out.count + 1, (unsigned long long)ran);
}

// A join kernel over a's rows and columns: grid = (column blocks) x (row groups); the kernel's parameters are the rows,
// their lengths, then `tables` (what the route reads through restrict pointers of its own), then a by value.
template <class Kernel, class Args, class... Tables>
hipError_t sed_join_launch(Kernel kernel, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const Args &a, Tables... tables) {
    if (a.s.nrows <= 0 || a.s.ncols <= 0) return hipSuccess;
    const dim3 grid((a.s.ncols + SED_JOIN_BLOCK - 1) / SED_JOIN_BLOCK, (a.s.nrows + SED_JOIN_G - 1) / SED_JOIN_G);
    if (grid.y > SED_JOIN_MAX_GROUPS) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(kernel, grid, dim3(SED_JOIN_BLOCK), 0, stream, ev0, ev1, 0, (const uint32_t *)a.s.rows, a.s.row_len,
                          tables..., a);
    return hipGetLastError();
}
