// sed_fit_f64_dp.h - what the fp64 fit kernels of sed_fit_f64.hip (one lane per chunk) and sed_fit_long_f64.hip (one
// wave per chunk) share: the cost table in LDS, the lexicographic minimum of a cell, the hit list's append and the
// best-hit reduce.  One copy of each; the cell loops themselves differ (where the rows live) and stay in their units.
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

// One hit of the lane, decided for the whole wave (sed_dev.h: wave_claim_slot)
__device__ __forceinline__ void fit_f64_append(const fit_f64_hit_list &hl, bool hit, int32_t pair, int32_t end, int32_t start,
                                               double D) {
    unsigned long long slot;
    if (wave_claim_slot(hl.count, hit, &slot) && slot < hl.cap)
        hl.rec[slot] = sed_fit_f64_hit{(uint32_t)pair, (uint32_t)end, start, 0u, D};
}

// Best hit over a run of records: the first strict minimum of rec[t], rec[t + 1], ... while k < n and same(k), the
// records that share rec[t]'s key (a pair's lanes, a text's chunk records) in chunk order.  The one copy for the three
// reduce kernels, which find their records, their key and their output slot.
template <class Same>
__device__ __forceinline__ sed_fit_f64_best fit_f64_first_min(const sed_fit_f64_best *__restrict__ rec, int t, int n, Same same) {
    sed_fit_f64_best b = rec[t];
    for (int k = t + 1; k < n && same(k); ++k)
        if (rec[k].D < b.D) b = rec[k];
    return b;
}

// (d, s) <- the lexicographic minimum of (d, -s) and (cd, -cs)
__device__ __forceinline__ void fit_f64_take(double &d, int32_t &s, double cd, int32_t cs) {
    const bool less = (cd < d) | ((cd == d) & (cs > s));  // (bitwise: three compares, no branch)
    d = less ? cd : d;
    s = less ? cs : s;
}

}  // namespace
