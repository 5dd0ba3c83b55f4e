// sed_join_dev.h - what the join kernels share (sed_join.hip: columns of 0..32 symbols, sed_join_long.hip: 0..128,
// sed_join_f64.hip: the fp64 route): the append to the device hit list and the launch, for all three; the walk over a
// block's rows with the self rule, the length skip and the two counters, for the two integer units, and beside it the two
// walks of the k-nearest calls, which the same kernel bodies are instantiated over.  One copy, so the
// kernels report the same pairs under the same rule (sed_internal.h: sed_join_args, sed_join_f64_args).
// sed_join_f64_kernel keeps a row loop of its own: handed this walk with its skip, distance and hit test as parameters
// it compiled to another instruction schedule (profiles/kernel_shells/README.md); its k-nearest passes live in that loop
// too (sed_join_f64.hip), on the bits of the fp64 distance as a 64-bit key.
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

// ---- the k nearest columns of every row: two more walks (sed_internal.h: sed_join_knn_args) ----
// Pass 1, the bound pass: sed_join_rows' loop with the row's bound b = bound[r] (a relaxed agent-scope atomic load:
// other waves lower it meanwhile, and a stale value only prunes less) in place of the cutoff, and no append.  A wave
// with at least k columns in scope at D <= b finds d_k, its k-th smallest such D, and one lane lowers bound[r] to it.
// Those k all lie <= b, so d_k is the wave's true k-th smallest whatever b was, and it is >= the row's; a wave with
// fewer than k has a true k-th smallest above b.  Hence bound[r] ends as min(cut, the smallest k-th smallest of any
// wave), in every schedule.  d_k by bisection on the value: 16 rounds of compare, ballot and popcount, since D <= b <=
// SED_JOIN_CUT_ALL < 2^16; no loop here depends on the data or waits for another wave.
template <class Pair>
__device__ __forceinline__ void sed_join_knn_bound_rows(const int32_t *__restrict__ row_len, const sed_join_knn_args &ka,
                                                        bool valid, int m, int orig, Pair pair) {
    const sed_join_args &a = ka.j;
    const int rbeg = a.s.row0 + (int)blockIdx.y * SED_JOIN_G;
    const int rend = min(rbeg + SED_JOIN_G, a.s.row0 + a.s.nrows);
    uint32_t ran = 0;
    for (int r = rbeg; r < rend; ++r) {
        const int n = row_len[r];  // (uniform: a scalar load)
        const uint32_t lb = m > n ? (uint32_t)(m - n) * a.ins : (uint32_t)(n - m) * a.del;
        const uint32_t b = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(ka.bound + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const bool go = valid && !(a.s.self && orig == r) && lb <= b;
        const unsigned long long gb = __builtin_amdgcn_ballot_w64(go);
        if (gb == 0) continue;  // no column of this wave can be within the bound of row r
        ran += (uint32_t)__popcll(gb);
        const uint32_t D = pair(r, n);
        const bool cand = go && D <= b;
        if (__popcll(__builtin_amdgcn_ballot_w64(cand)) < ka.k) continue;
        uint32_t x = 0;  // the largest x with fewer than k candidates at D < x: the k-th smallest D
#pragma unroll
        for (int bit = 15; bit >= 0; --bit) {
            const uint32_t c = x | (1u << bit);
            if (__popcll(__builtin_amdgcn_ballot_w64(cand && D < c)) < ka.k) x = c;
        }
        if (x < b && (threadIdx.x & 63) == 0) atomicMin(ka.bound + r, x);
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.out.count + 1, (unsigned long long)ran);
}

// Pass 2, the emit pass: sed_join_rows with bound[r] (final since pass 1 ended: one value for the whole wave) in place
// of the cutoff, in the length skip and the hit test alike.  It appends exactly {D <= bound[r]}: the k nearest and every
// tie at the k-th place.
template <class Pair>
__device__ __forceinline__ void sed_join_knn_emit_rows(const int32_t *__restrict__ row_len, const sed_join_knn_args &ka,
                                                       bool valid, int m, int orig, Pair pair) {
    const sed_join_args &a = ka.j;
    const int rbeg = a.s.row0 + (int)blockIdx.y * SED_JOIN_G;
    const int rend = min(rbeg + SED_JOIN_G, a.s.row0 + a.s.nrows);
    uint32_t ran = 0;
    for (int r = rbeg; r < rend; ++r) {
        const int n = row_len[r];  // (uniform: a scalar load)
        const uint32_t lb = m > n ? (uint32_t)(m - n) * a.ins : (uint32_t)(n - m) * a.del;
        const uint32_t b = __builtin_amdgcn_readfirstlane(ka.bound[r]);
        const bool go = valid && !(a.s.self && orig == r) && lb <= b;
        const unsigned long long gb = __builtin_amdgcn_ballot_w64(go);
        if (gb == 0) continue;
        ran += (uint32_t)__popcll(gb);
        const uint32_t D = pair(r, n);
        sed_join_append(a.out, go && D <= b, r, orig, D, 0u);
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.out.count + 1, (unsigned long long)ran);
}

// What a kernel body is instantiated over: the arguments it takes by value, the join's arguments within them, and the
// walk.  sed_join_walk_all is the join itself.
struct sed_join_walk_all {
    using args = sed_join_args;
    static __device__ __forceinline__ const sed_join_args &join(const args &a) { return a; }
    template <class Pair>
    static __device__ __forceinline__ void rows(const int32_t *__restrict__ row_len, const args &a, bool valid, int m, int orig,
                                                Pair pair) {
        sed_join_rows(row_len, a, valid, m, orig, pair);
    }
};
template <bool EMIT>
struct sed_join_walk_knn {
    using args = sed_join_knn_args;
    static __device__ __forceinline__ const sed_join_args &join(const args &a) { return a.j; }
    template <class Pair>
    static __device__ __forceinline__ void rows(const int32_t *__restrict__ row_len, const args &a, bool valid, int m, int orig,
                                                Pair pair) {
        if constexpr (EMIT)
            sed_join_knn_emit_rows(row_len, a, valid, m, orig, pair);
        else
            sed_join_knn_bound_rows(row_len, a, valid, m, orig, pair);
    }
};

template <class Args>
inline const sed_join_sides &sed_join_sides_of(const Args &a) { return a.s; }
inline const sed_join_sides &sed_join_sides_of(const sed_join_knn_args &a) { return a.j.s; }
inline const sed_join_sides &sed_join_sides_of(const sed_join_knn_f64_args &a) { return a.j.s; }

// A join kernel over a's rows and columns: grid = (column blocks) x (row groups); the kernel's parameters are the rows,
// their lengths, then `tables` (what the route reads through restrict pointers of its own), then a by value.
template <class Kernel, class Args, class... Tables>
hipError_t sed_join_launch(Kernel kernel, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const Args &a, Tables... tables) {
    const sed_join_sides &s = sed_join_sides_of(a);
    if (s.nrows <= 0 || s.ncols <= 0) return hipSuccess;
    const dim3 grid((s.ncols + SED_JOIN_BLOCK - 1) / SED_JOIN_BLOCK, (s.nrows + SED_JOIN_G - 1) / SED_JOIN_G);
    if (grid.y > SED_JOIN_MAX_GROUPS) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(kernel, grid, dim3(SED_JOIN_BLOCK), 0, stream, ev0, ev1, 0, (const uint32_t *)s.rows, s.row_len,
                          tables..., a);
    return hipGetLastError();
}
