// sed_fit_f64_dp.h - what the fp64 fit kernels of sed_fit_f64.hip (one lane per chunk) and sed_fit_long_f64.hip (one
// wave per chunk) share: the cost table in LDS, the lexicographic minimum of a cell, and the hit list's append.  One
// copy of each; the cell loops themselves differ (where the rows live) and stay in their units.
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

namespace {

constexpr int F64_K = SED_FIT_F64_MAXK;

// tab[a * F64_K + b] = cost(pattern symbol a -> text symbol b); every thread of the block
__device__ __forceinline__ void fit_f64_fill_tab(double *tab, const double *__restrict__ sub) {
    for (int e = threadIdx.x; e < F64_K * F64_K; e += blockDim.x) tab[e] = sub[e];
    __syncthreads();
}

struct fit_f64_hit_list {
    sed_fit_f64_hit *rec;
    unsigned long long *count;
    unsigned long long cap;
    double max_dist;
};

// One hit of the lane, decided for the whole wave (sed_fit_dp.h: sed_fit_append, with the wider record)
__device__ __forceinline__ void fit_f64_append(const fit_f64_hit_list &hl, bool hit, int32_t pair, int32_t end, int32_t start,
                                               double D) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(hit);
    if (b == 0) return;
    if (hit) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        unsigned long long base = 0;
        if (rank == 0) base = atomicAdd(hl.count, (unsigned long long)__popcll(b));
        const unsigned long long slot =
            (((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)base)) + rank;
        if (slot < hl.cap) hl.rec[slot] = sed_fit_f64_hit{(uint32_t)pair, (uint32_t)end, start, 0u, D};
    }
}

// (d, s) <- the lexicographic minimum of (d, -s) and (cd, -cs)
__device__ __forceinline__ void fit_f64_take(double &d, int32_t &s, double cd, int32_t cs) {
    const bool less = (cd < d) | ((cd == d) & (cs > s));  // (bitwise: three compares, no branch)
    d = less ? cd : d;
    s = less ? cs : s;
}

}  // namespace
