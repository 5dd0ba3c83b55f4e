// sed_windows.hip — the window kernels ahead of and after the integer forward (sed_kernels.hip): the band of diagonals
// of a checkpoint batch (sed_band_kernel), the cutoff's windows and its result filter, and their launchers.
#include <hip/hip_ext.h>
#include "sed_internal.h"

// The block's LDS copy of the 4 x 4 cost table, ready on return.  It holds the block's barrier, so a kernel calls it
// ahead of its early exits; that is why it is not part of diag_cost_sum.
__device__ __forceinline__ void diag_cost_table(uint32_t *tab, const sed_band_params &bp) {
    if (threadIdx.x < 16) tab[threadIdx.x] = bp.cost[threadIdx.x];
    __syncthreads();
}
// The cost of a wave pair's plain diagonal path over its first len = min(n, m) symbols, in every lane of the wave:
// each lane sums its share of the packed words through tab (diag_cost_table), then the wave adds the lanes up.  The
// host restates it as band_diag_bound (sed_runtime.cpp).
__device__ __forceinline__ uint32_t diag_cost_sum(const uint32_t *tab, const uint32_t *pa, const uint32_t *pb,
                                                  const int len, const int lane) {
    const int words = (len + 15) >> 4;
    uint32_t sum = 0;
    for (int w = lane; w < words; w += 64) {
        uint32_t x = pa[w], y = pb[w];
        const int cnt = min(16, len - 16 * w);
        for (int u = 0; u < cnt; ++u) {
            sum += tab[((x & 3u) << 2) | (y & 3u)];
            x >>= 2;
            y >>= 2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    return sum;
}

// ---------------------------------------------------------------------------
// Band pruning (sed_internal.h: sed_band_window): the cost UB of every wave pair's plain diagonal path and from it the
// window of diagonals an optimal path can touch, one wave per pair, launched before every forward of a checkpoint
// batch of the stripe kernel (a batch is run once in real use, so the run pays for its bound).  ~(n + m) / 4 bytes per pair
// (2 bits per symbol, 16 per word).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sed_band_kernel(const sed_pair_desc *__restrict__ pd, int npairs,
                                                       const uint32_t *__restrict__ seqa,
                                                       const uint32_t *__restrict__ seqb, sed_band *__restrict__ band,
                                                       sed_band_params bp, uint32_t *__restrict__ suf, int stride,
                                                       int ROWS) {
    __shared__ uint32_t tab[16];
    diag_cost_table(tab, bp);
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npairs) return;
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;
    if (d.lane || n == 0 || m == 0) {  // not a pair of the stripe kernel
        if (lane == 0) band[pair] = sed_band{SED_BAND_OPEN_LO, SED_BAND_OPEN_HI};
        return;
    }
    const uint32_t gap = m > n ? (uint32_t)(m - n) * bp.ins : (uint32_t)(n - m) * bp.del;
    uint32_t sum = 0;
    if (suf) {
        // refined windows: also suf(k ROWS), the diagonal's cost from every stripe boundary to the sink, one word per
        // stripe of the pair.  ROWS is a multiple of 16, so a packed word belongs to one stripe: from the last stripe
        // up, the lanes sum their words of the stripe and the wave adds them to the running suffix (each word is still
        // read once).  suf(0) is UB itself.
        const int len = min(n, m), words = (len + 15) >> 4, wps = ROWS >> 4;
        const uint32_t *pa = seqa + d.a_off, *pb = seqb + d.b_off;
        uint32_t *out = suf + (size_t)pair * stride;
        for (int k = (n + ROWS - 1) / ROWS - 1; k >= 0; --k) {
            uint32_t part = 0;
            for (int w = k * wps + lane; w < min(words, (k + 1) * wps); w += 64) {
                uint32_t x = pa[w], y = pb[w];
                const int cnt = min(16, len - 16 * w);
                for (int u = 0; u < cnt; ++u) {
                    part += tab[((x & 3u) << 2) | (y & 3u)];
                    x >>= 2;
                    y >>= 2;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
            sum += part;
            if (lane == 0) out[k] = k * ROWS <= len ? sum + gap : SED_REFINE_NO_SUF;
        }
    } else {
        sum = diag_cost_sum(tab, seqa + d.a_off, seqb + d.b_off, min(n, m), lane);
    }
    if (lane == 0) band[pair] = sed_band_window(n, m, bp.ins, bp.del, (uint64_t)sum + gap);
}

// ---------------------------------------------------------------------------
// Cutoff batches (sed_batch_set_cutoff).  sed_cut_band_kernel: the window of every pair of the cutoff's
// pair list, one wave per pair, before every windowed forward: ub = min(tkey, the diagonal bound) (tkey = the cutoff
// on the integer scale), or the empty window {1, 0} when the length difference alone costs more than tkey.  diag (if
// not null) receives every pair's diagonal bound, which the host reads once for its restatement of the windows.
// sed_cut_filter_kernel: every pair's result against the cutoff, after the run's last DP kernel: a distance above it
// becomes {+inf, len -1, not an int}; hits counts the pairs within.  Plain vector stores.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sed_cut_band_kernel(const sed_pair_desc *__restrict__ pd,
                                                           const int32_t *__restrict__ list, int nlist,
                                                           const uint32_t *__restrict__ seqa,
                                                           const uint32_t *__restrict__ seqb, sed_band *__restrict__ band,
                                                           uint32_t *__restrict__ diag, sed_band_params bp, uint32_t tkey) {
    __shared__ uint32_t tab[16];
    diag_cost_table(tab, bp);
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nlist) return;
    const int pair = list[w];
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;
    if (n == 0 || m == 0) {  // the stripe kernel writes these from the lengths alone
        if (lane == 0) {
            band[pair] = sed_band{SED_BAND_OPEN_LO, SED_BAND_OPEN_HI};
            if (diag) diag[pair] = 0xFFFFFFFFu;
        }
        return;
    }
    const uint32_t sum = diag_cost_sum(tab, seqa + d.a_off, seqb + d.b_off, min(n, m), lane);
    if (lane == 0) {
        const uint64_t gap = m > n ? (uint64_t)(m - n) * bp.ins : (uint64_t)(n - m) * bp.del;
        const uint64_t ub = (uint64_t)sum + gap;
        if (diag) diag[pair] = (uint32_t)(ub < 0xFFFFFFFFull ? ub : 0xFFFFFFFFull);
        band[pair] = gap > (uint64_t)tkey ? sed_band{1, 0}
                                          : sed_band_window(n, m, bp.ins, bp.del, ub < (uint64_t)tkey ? ub : (uint64_t)tkey);
    }
}

__global__ __launch_bounds__(256) void sed_cut_filter_kernel(sed_result *__restrict__ res, int npairs, double cutoff,
                                                             uint32_t *__restrict__ hits) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool within = false;
    if (p < npairs) {
        const sed_result r = res[p];
        within = r.err != 0 || r.dist <= cutoff;  // (a failed pair is reported as the failure it is)
        if (!within) {
            sed_result o = r;
            o.dist = __builtin_huge_val();
            o.len = -1;
            o.is_int = 0;
            res[p] = o;
        }
    }
    const uint64_t bal = __ballot(within);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(hits, (uint32_t)__popcll(bal));
}

// ---------------------------------------------------------------------------
// Launchers (host side, called from sed_runtime.cpp and from the forward's launchers in sed_kernels.hip)
// ---------------------------------------------------------------------------
hipError_t sed_launch_cut_band(const sed_launch &L, const int32_t *list, int nlist, uint32_t *diag,
                               const sed_band_params &bp, uint32_t tkey) {
    if (nlist <= 0) return hipSuccess;
    hipExtLaunchKernelGGL(sed_cut_band_kernel, dim3((nlist + 3) / 4), dim3(256), 0, L.stream, L.ev0, nullptr, 0, L.pd, list,
                          nlist, (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.band, diag, bp, tkey);
    return hipGetLastError();
}
hipError_t sed_launch_cut_filter(const sed_launch &L, double cutoff, uint32_t *hits) {
    if (L.npairs <= 0) return hipSuccess;
    SED_LAUNCH(sed_cut_filter_kernel, dim3((L.npairs + 255) / 256), dim3(256), 0, L, L.res, L.npairs, cutoff, hits);
    return hipGetLastError();
}
hipError_t sed_launch_band(const sed_launch &L, const sed_band_params &bp) {
    hipExtLaunchKernelGGL(sed_band_kernel, dim3((L.npairs + 3) / 4), dim3(256), 0, L.stream, L.ev0, nullptr, 0, L.pd,
                          L.npairs, (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.band, bp, L.bsuf, L.bstripes,
                          64 * L.R);
    return hipGetLastError();
}
