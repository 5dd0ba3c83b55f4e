// sed_fit.hip — fit search (include/sed.h: sed_fit_search, and sed_fit_index_search over a resident text index, whose
// kernel is at the end and runs the same DP, sed_fit_dp.h): the best approximate occurrence of a short pattern
// (1 <= P <= SED_LANE_MAXM) in a long text, one lane per (pair, chunk of text columns).  The last kernel,
// sed_fit_index_hits_kernel (sed_fit_index_hits), reports every end column within a cutoff instead of the best.
// The host side: sed_fit_plan.cpp decides what a search runs, sed_fit_runtime.cpp stages and launches it.
//
// The DP is the weighted Wagner-Fischer recurrence (StringEditDistance.py:92-128) with a free start: D[0][j] = 0,
// D[i][0] = i delete, and every cell carries (D, -s), s = the text column its path left row 0 at, as one
// lexicographic key.  The lane keeps the pattern dimension in VGPRs and streams the text, four byte codes per load:
//   - 33 key registers V[0..32].  The pattern sits at the bottom: its row i lives in V[32 - P + i], so the sink row
//     is V[32] whatever P is.  V[0] is set to row 0's key in every column, and the 32 - P rows in front of the pattern
//     have update addend 0 for every symbol, which makes them hand row 0's key down unchanged (see below).
//   - keys are offset keys K = (D + (P - i) delete - l' insert + B) << 16 | field: the delete candidate is the
//     register above and the insert candidate the register's own old value, both as they are; the update candidate is
//     the old register above minus kappa << 16, kappa = insert + delete - min(cost, insert + delete) in 0..255 (a
//     substitution dearer than delete + insert never wins: the pair of them from the same cell carries the same start).
//     A cell is v_perm_b32 (kappa of this row for the column's symbol) + v_sub_u32 + v_min3_u32.
//   - field = 0xFFFF - (s - the lane's first column): a smaller field is a larger start, so the unsigned minimum of
//     whole words is the minimum of (D, -s).
//   - l' counts columns since the last rebase: every 128 columns 128 insert << 16 is added to all 33 registers, so the
//     16-bit D field never wraps (D + (P - i) delete <= 32 * 255, 128 insert <= 128 * 255).
//   - row 0's key of column l is inj = (P delete + B - l' insert) << 16 | (0xFFFF - l), strictly decreasing in l; a
//     front row computes min3(own old = inj(l-1), above = inj(l), old above - 0 = inj(l-1)) = inj(l).
// A lane owns text columns [c0, c0 + cnt) and starts `lead` columns earlier (the planner's window W, sed_fit_plan.cpp)
// from the border column i delete: on its own columns it computes the full matrix's keys.  After each owned column it
// keeps the first strict minimum of the sink row: V[32] - inj = (D - P delete) << 16 | (end - start), compared as
// (that's high half, owned column index) signed.  The lanes of a pair meet in one 64-bit atomic minimum on
// D << 48 | end << 16 | (end - start): smallest distance, then smallest end; the start in the key is the largest one.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_fit_dp.h"
#include "sed_fit_index_dev.h"

namespace {

__global__ __launch_bounds__(SED_FIT_BLOCK, 4) void sed_fit_kernel(const sed_fit_lane *__restrict__ lanes, int nlanes,
                                                                    const uint4 *__restrict__ pats,
                                                                    const uint32_t *__restrict__ text,
                                                                    unsigned long long *__restrict__ out,
                                                                    sed_fit_params fp) {
    __shared__ uint2 tab[9];
    sed_fit_fill_tab(tab, fp);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes) return;
    const sed_fit_lane ln = lanes[t];
    sed_fit_dp(ln, pats[2 * (size_t)ln.pat], pats[2 * (size_t)ln.pat + 1], tab, text, out, fp);
}

// The same DP over a resident index (sed_internal.h: sed_fit_index_args): one lane per (query, chunk record)
// (sed_fit_index_dev.h: sed_fit_index_lane), which reports into out[query * ntexts + text].
__global__ __launch_bounds__(SED_FIT_BLOCK, 4) void sed_fit_index_kernel(const sed_fit_chunk *__restrict__ chunks,
                                                                          int nchunks,
                                                                          const sed_fit_text *__restrict__ texts,
                                                                          int ntexts, const uint4 *__restrict__ pats,
                                                                          const int32_t *__restrict__ plens, int q0,
                                                                          const uint32_t *__restrict__ text,
                                                                          unsigned long long *__restrict__ out,
                                                                          int32_t chunk, int32_t W, sed_fit_params fp) {
    __shared__ uint2 tab[9];
    sed_fit_fill_tab(tab, fp);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const int q = q0 + (int)blockIdx.y;
    const sed_fit_lane ln = sed_fit_index_lane(chunks, texts, ntexts, plens, q, chunk, W, t);
    sed_fit_dp(ln, pats[2 * (size_t)q], pats[2 * (size_t)q + 1], tab, text, out, fp);
}

// Every occurrence within a cutoff (include/sed.h: sed_fit_index_hits): sed_fit_index_kernel's grid, chunk table and
// lane derivation, so sed_fit_index_lanes describes these lanes too.  Instead of the sink row's minimum a lane reports
// every owned column e with E(e) <= the cutoff: hits[slot] = (query * ntexts + text, e, e - S(e), E(e) * S), slots from
// *count (sed_fit_dp.h: sed_fit_append), in no particular order; the host sorts them.
__global__ __launch_bounds__(SED_FIT_BLOCK, 4) void sed_fit_index_hits_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint4 *__restrict__ pats, const int32_t *__restrict__ plens, int q0, const uint32_t *__restrict__ text,
    uint4 *__restrict__ hits, unsigned long long *__restrict__ count, unsigned long long cap, int32_t cut, int32_t chunk,
    int32_t W, sed_fit_params fp) {
    __shared__ uint2 tab[9];
    sed_fit_fill_tab(tab, fp);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const int q = q0 + (int)blockIdx.y;
    const sed_fit_lane ln = sed_fit_index_lane(chunks, texts, ntexts, plens, q, chunk, W, t);
    sed_fit_dp_hits(ln, pats[2 * (size_t)q], pats[2 * (size_t)q + 1], tab, text, sed_fit_hit_list{hits, count, cap, cut}, fp);
}

}  // namespace

hipError_t sed_launch_fit(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_lane *lanes, int nlanes,
                          const void *pats, const void *text, unsigned long long *out, const sed_fit_params &fp) {
    if (nlanes <= 0) return hipSuccess;
    hipExtLaunchKernelGGL(sed_fit_kernel, dim3((nlanes + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK), dim3(SED_FIT_BLOCK), 0,
                          stream, ev0, ev1, 0, lanes, nlanes, (const uint4 *)pats, (const uint32_t *)text, out, fp);
    return hipGetLastError();
}

// An index kernel over all of a's queries (sed_internal.h: sed_fit_each_query_group): the arguments the index kernels
// share up to the text, then `tail`.
template <typename Kernel, typename... Tail>
static hipError_t fit_launch_queries(Kernel kernel, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                                     const sed_fit_index_args &a, Tail... tail) {
    const unsigned gx = (unsigned)((a.nchunks + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK);
    return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(kernel, dim3(gx, (unsigned)nq), dim3(SED_FIT_BLOCK), 0, stream, e0, e1, 0, a.chunks, a.nchunks,
                              a.texts, a.ntexts, (const uint4 *)a.pats, a.plens, q0, (const uint32_t *)a.text, tail...);
        return hipGetLastError();
    });
}

hipError_t sed_launch_fit_index(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                const sed_fit_params &fp) {
    return fit_launch_queries(sed_fit_index_kernel, stream, ev0, ev1, a, a.out, a.chunk, a.W, fp);
}

hipError_t sed_launch_fit_index_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                     void *hits, unsigned long long *count, unsigned long long cap, int32_t cut,
                                     const sed_fit_params &fp) {
    return fit_launch_queries(sed_fit_index_hits_kernel, stream, ev0, ev1, a, (uint4 *)hits, count, cap, cut, a.chunk, a.W, fp);
}
