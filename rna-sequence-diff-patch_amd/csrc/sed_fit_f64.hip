// sed_fit_f64.hip — fit search in fp64 (include/sed.h: sed_fit_search_f64, sed_fit_index_search_f64,
// sed_fit_index_hits_f64): the route for the cost tables and alphabets the integer keys of sed_fit.hip refuse.  The
// layout is the short kernels': one lane per (pair, chunk of text columns), the same sed_fit_lane records, the same
// chunk table and 32-byte pattern records of a resident index.  What differs is the cell.
//
// The DP is oracle/sed_oracle.c: sed_oracle_fit_pair, operation for operation.  A lane keeps column j's rows in
// registers: 33 fp64 values D[0..32] and 33 int32 starts S[0..32], the pattern right-aligned as in sed_fit.hip (its row
// i lives in register 32 - P + i, the sink row is register 32).  A cell is
//     insert  D[r] (column j - 1)     + insert           start of that cell
//     delete  D[r - 1] (column j)     + delete           start of that cell
//     update  D[r - 1] (column j - 1) + sub[p_r][t_j]    start of that cell
// each ONE v_add_f64 (the unit is compiled with contraction off and holds no multiply-add to contract), then the
// lexicographic minimum of (D, -start): smaller D, and on equal D the larger start.  Nothing is rebased, offset or
// reassociated: the value of a cell is the oracle's value of that cell, bit for bit.
//   - border row: D[0] = +0.0, S[0] = j in every column.
//   - border column (a lane's first, `lead` columns before its first owned one): D = (double)i * delete, a product as
//     the oracle writes it, S = that column.  DESIGN.md 3.6i shows that on the columns a lane owns this gives the full
//     matrix's cells although its border column is synthetic; the planner (sed_fit_plan.cpp) sizes the lead for it and
//     runs a text as one lane where the argument cannot be made.
//   - front rows (registers 1 .. 32 - P of a pattern shorter than 32): overwritten with row 0's (+0.0, j) after the
//     cell is computed, so the pattern's first row reads row 0 above it and no fp64 value is perturbed; the pattern
//     record's code in those rows (8) only has to index the table, whose SED_FIT_F64_MAXK rows are all present.
//   - the K x K substitution table lives in LDS as doubles, row = pattern symbol, SED_FIT_F64_MAXK columns a row.
// Best hit: a lane keeps the first strict minimum of the sink row over the columns it owns and writes (D, start, end)
// to its own record; sed_fit_f64_reduce_kernel / sed_fit_index_f64_reduce_kernel take per pair the first strict minimum
// over the pair's lanes in chunk order.  No atomic is involved: the result does not depend on any order of execution.
// Hits: every owned column with sink D <= max_dist (a plain fp64 compare) is appended through the wave's ballot, one
// atomic add per wave and column on the counter (sed_dev.h: wave_claim_slot), the record carrying D as 64 bits and the
// start as 32; the host sorts the list.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_fit_f64_dp.h"
#include "sed_fit_index_dev.h"

namespace {

constexpr int F64_ROWS = SED_LANE_MAXM;

// q0, q1 = the pattern record (sed_fit_runtime.cpp: fit_pack_pattern).  HITS = false: the lane's first strict minimum
// goes to *best; HITS = true: every owned column within hl.max_dist goes to the hit list.
template <bool HITS>
__device__ __forceinline__ void fit_f64_dp(const sed_fit_lane &ln, const uint4 q0, const uint4 q1, const double *tab,
                                           const uint32_t *__restrict__ text, sed_fit_f64_best *best,
                                           const fit_f64_hit_list &hl, double ins, double del) {
    static_assert(F64_ROWS == 32, "a pattern record is two 16-byte words");
    const uint32_t pw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    const int npad = F64_ROWS - ln.plen;  // registers 1 .. npad are front rows
    const int32_t jb = ln.c0 - ln.lead;   // the border column
    double D[F64_ROWS + 1];
    int32_t S[F64_ROWS + 1];
#pragma unroll
    for (int r = 0; r <= F64_ROWS; ++r) {
        D[r] = r > npad ? (double)(r - npad) * del : 0.0;
        S[r] = jb;
    }
    int32_t u = -ln.lead;  // the current column's index among the owned ones
    double bD = __builtin_inf();
    int32_t bS = 0, bE = 0;
    // an owned border column (lead = 0: column 0 of the text) is a column: D = P delete, start = end = 0
    if (HITS) {
        fit_f64_append(hl, ln.lead == 0 && D[F64_ROWS] <= hl.max_dist, ln.pair, ln.c0, jb, D[F64_ROWS]);
    } else if (ln.lead == 0) {
        bD = D[F64_ROWS];
        bS = jb;
        bE = ln.c0;
    }
    const uint32_t *tp = text + ln.tw;
    uint32_t wnext = ln.nsteps > 0 ? tp[0] : 0u;
    int32_t j = jb;
    for (int s = 0; s < ln.nsteps; s += 4) {
        const uint32_t w = wnext;
        wnext = tp[(s >> 2) + 1];  // (the text buffer ends with spare words)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t = (w >> (8 * k)) & (uint32_t)(F64_K - 1);
            ++j;
            double dgD = D[0];
            int32_t dgS = S[0];
            D[0] = 0.0;
            S[0] = j;
#pragma unroll
            for (int r = 1; r <= F64_ROWS; ++r) {
                const uint32_t a = (pw[(r - 1) >> 2] >> (8 * ((r - 1) & 3))) & (uint32_t)(F64_K - 1);
                const double cost = tab[a * F64_K + t];
                const double oldD = D[r];
                const int32_t oldS = S[r];
                double vD = oldD + ins;  // insert (left)
                int32_t vS = oldS;
                fit_f64_take(vD, vS, D[r - 1] + del, S[r - 1]);  // delete (up)
                fit_f64_take(vD, vS, dgD + cost, dgS);           // update (diagonal)
                const bool front = r <= npad;
                D[r] = front ? 0.0 : vD;
                S[r] = front ? j : vS;
                dgD = oldD;
                dgS = oldS;
            }
            ++u;
            const bool owned = (uint32_t)u < (uint32_t)ln.cnt;  // (false in the columns that round nsteps up to 4)
            if (HITS) {
                fit_f64_append(hl, owned && D[F64_ROWS] <= hl.max_dist, ln.pair, j, S[F64_ROWS], D[F64_ROWS]);
            } else {
                const bool take = owned && D[F64_ROWS] < bD;
                bD = take ? D[F64_ROWS] : bD;
                bS = take ? S[F64_ROWS] : bS;
                bE = take ? j : bE;
            }
        }
    }
    if (!HITS) *best = sed_fit_f64_best{bD, bS, bE};
}

__global__ __launch_bounds__(SED_FIT_BLOCK, 2) void sed_fit_f64_kernel(const sed_fit_lane *__restrict__ lanes, int nlanes,
                                                                        const uint4 *__restrict__ pats,
                                                                        const uint32_t *__restrict__ text,
                                                                        sed_fit_f64_best *__restrict__ rec,
                                                                        const double *__restrict__ sub, double ins, double del) {
    __shared__ double tab[F64_K * F64_K];
    fit_f64_fill_tab(tab, sub);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes) return;
    const sed_fit_lane ln = lanes[t];
    fit_f64_dp<false>(ln, pats[2 * (size_t)ln.pat], pats[2 * (size_t)ln.pat + 1], tab, text, rec + t, fit_f64_hit_list{}, ins, del);
}

// Per pair the first strict minimum over its lanes in chunk order: the thread of a pair's first lane (c0 = 0) walks
// the lanes that follow while they are the pair's.
__global__ __launch_bounds__(SED_FIT_BLOCK) void sed_fit_f64_reduce_kernel(const sed_fit_lane *__restrict__ lanes, int nlanes,
                                                                            const sed_fit_f64_best *__restrict__ rec,
                                                                            sed_fit_f64_best *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes || lanes[t].c0 != 0) return;
    const int32_t pair = lanes[t].pair;
    out[pair] = fit_f64_first_min(rec, t, nlanes, [&](int k) { return lanes[k].pair == pair; });
}

__global__ __launch_bounds__(SED_FIT_BLOCK, 2) void sed_fit_index_f64_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint4 *__restrict__ pats, const int32_t *__restrict__ plens, int q0, const uint32_t *__restrict__ text,
    sed_fit_f64_best *__restrict__ rec, int32_t chunk, int32_t W, const double *__restrict__ sub, double ins, double del) {
    __shared__ double tab[F64_K * F64_K];
    fit_f64_fill_tab(tab, sub);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const int q = q0 + (int)blockIdx.y;
    const sed_fit_lane ln = sed_fit_index_lane(chunks, texts, ntexts, plens, q, chunk, W, t);
    fit_f64_dp<false>(ln, pats[2 * (size_t)q], pats[2 * (size_t)q + 1], tab, text, rec + (size_t)q * nchunks + t,
                      fit_f64_hit_list{}, ins, del);
}

__global__ __launch_bounds__(SED_FIT_BLOCK) void sed_fit_index_f64_reduce_kernel(const sed_fit_chunk *__restrict__ chunks,
                                                                                  int nchunks, int ntexts, int q0,
                                                                                  const sed_fit_f64_best *__restrict__ rec,
                                                                                  sed_fit_f64_best *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks || chunks[t].c0 != 0) return;
    const int q = q0 + (int)blockIdx.y;
    const int32_t d = chunks[t].text;
    out[(size_t)q * ntexts + d] =
        fit_f64_first_min(rec + (size_t)q * nchunks, t, nchunks, [&](int k) { return chunks[k].text == d; });
}

__global__ __launch_bounds__(SED_FIT_BLOCK, 2) void sed_fit_index_f64_hits_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint4 *__restrict__ pats, const int32_t *__restrict__ plens, int q0, const uint32_t *__restrict__ text,
    sed_fit_f64_hit *__restrict__ hits, unsigned long long *__restrict__ count, unsigned long long cap, double max_dist,
    int32_t chunk, int32_t W, const double *__restrict__ sub, double ins, double del) {
    __shared__ double tab[F64_K * F64_K];
    fit_f64_fill_tab(tab, sub);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const int q = q0 + (int)blockIdx.y;
    const sed_fit_lane ln = sed_fit_index_lane(chunks, texts, ntexts, plens, q, chunk, W, t);
    fit_f64_dp<true>(ln, pats[2 * (size_t)q], pats[2 * (size_t)q + 1], tab, text, nullptr,
                     fit_f64_hit_list{hits, count, cap, max_dist}, ins, del);
}

}  // namespace

hipError_t sed_launch_fit_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_lane *lanes, int nlanes,
                              const void *pats, const void *text, sed_fit_f64_best *rec, sed_fit_f64_best *out,
                              const sed_fit_f64_costs &fc) {
    if (nlanes <= 0) return hipSuccess;
    const dim3 grid((nlanes + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK), block(SED_FIT_BLOCK);
    hipExtLaunchKernelGGL(sed_fit_f64_kernel, grid, block, 0, stream, ev0, nullptr, 0, lanes, nlanes, (const uint4 *)pats,
                          (const uint32_t *)text, rec, fc.sub, fc.ins, fc.del);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(sed_fit_f64_reduce_kernel, grid, block, 0, stream, nullptr, ev1, 0, lanes, nlanes,
                          (const sed_fit_f64_best *)rec, out);
    return hipGetLastError();
}

// nq queries of an index search (sed_internal.h: sed_fit_each_query_group): one lane per (query, chunk record)
static dim3 fit_f64_grid(const sed_fit_index_args &a, int nq) {
    return dim3((unsigned)((a.nchunks + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK), (unsigned)nq);
}

hipError_t sed_launch_fit_index_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                    sed_fit_f64_best *rec, sed_fit_f64_best *out, const sed_fit_f64_costs &fc) {
    return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
        const dim3 grid = fit_f64_grid(a, nq);
        hipExtLaunchKernelGGL(sed_fit_index_f64_kernel, grid, dim3(SED_FIT_BLOCK), 0, stream, e0, nullptr, 0, a.chunks, a.nchunks,
                              a.texts, a.ntexts, (const uint4 *)a.pats, a.plens, q0, (const uint32_t *)a.text, rec, a.chunk,
                              a.W, fc.sub, fc.ins, fc.del);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipExtLaunchKernelGGL(sed_fit_index_f64_reduce_kernel, grid, dim3(SED_FIT_BLOCK), 0, stream, nullptr, e1, 0, a.chunks,
                              a.nchunks, a.ntexts, q0, (const sed_fit_f64_best *)rec, out);
        return hipGetLastError();
    });
}

hipError_t sed_launch_fit_index_f64_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                         sed_fit_f64_hit *hits, unsigned long long *count, unsigned long long cap,
                                         double max_dist, const sed_fit_f64_costs &fc) {
    return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(sed_fit_index_f64_hits_kernel, fit_f64_grid(a, nq), dim3(SED_FIT_BLOCK), 0, stream, e0, e1, 0, a.chunks, a.nchunks,
                              a.texts, a.ntexts, (const uint4 *)a.pats, a.plens, q0, (const uint32_t *)a.text, hits, count, cap,
                              max_dist, a.chunk, a.W, fc.sub, fc.ins, fc.del);
        return hipGetLastError();
    });
}
