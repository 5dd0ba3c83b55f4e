// sed_fit_long_f64.hip — fit search in fp64 for patterns of up to 2048 symbols (include/sed.h:
// sed_fit_index_search_long_f64, sed_fit_index_hits_long_f64).  The wave layout and schedule are
// sed_fit_long.hip's, the cell is sed_fit_f64.hip's, operation for operation: oracle/sed_oracle.c: sed_oracle_fit_pair.
//   - Registers.  Rows G[0 .. 64 R]: G[0] is row 0, (+0.0, j) in every column; the pattern is right-aligned in
//     G[1 .. 64 R] behind 64 R - P front rows, and the sink row is G[64 R], the last register of lane 63, whatever P is.
//     Lane l holds G[l R + 1 .. l R + R] as (fp64 D[r], int32 S[r]), r = 0 .. R - 1.
//   - Skew.  At step t = 1, 2, ... lane l computes column jb + t - l of its rows, jb the wave's border column.  A lane
//     whose column is <= jb has not started: its registers hold the border column, D = (double)i * delete (0 in a front
//     row), start = jb, and the cell loop is skipped under the exec mask (every symbol indexes a real table row, so no
//     neutral input exists that would leave them there).  A wave runs nsteps + 63 steps, rounded up to the four
//     columns of a text word; the skew's tail runs on zero symbols into columns nobody owns.
//   - Hand-over.  Each step a lane takes through wave_shr:1 from lane l - 1: the (D, start) of G[l R] that lane
//     produced one step earlier, which is that row's cell of this lane's column (the delete candidate of the top row),
//     and the text symbol of that column, which lane 0 took from the text word.  They are plain values: there is no
//     offset to agree on.  The pair received the step before (tpD, tpS) is G[l R]'s cell of the column before, the top
//     row's diagonal.  Lane 0 keeps row 0's (+0.0, j) where the others receive.
//   - Front rows.  Overwritten with row 0's (+0.0, j) after the cell is computed, as in sed_fit_f64.hip: the pattern's
//     first row reads row 0 above it and on its diagonal, and no fp64 value passes through an extra operation.  A lane
//     holds min(max(64 R - P - l R, 0), R) of them at the top of its registers; they may fill whole lanes.  The pad
//     code of the record (8) only indexes the table, all of whose rows exist.
//   - Reporting.  Lane 63 owns the sink row.  Best hit: the first strict minimum (D, start, end) over the columns the
//     wave owns goes to the wave's record rec[query * nchunks + chunk record]; sed_fit_index_long_f64_reduce_kernel
//     takes per (query, text) the first strict minimum over the text's records in chunk order.  No atomic takes part.
//     Hits: every owned column with sink D <= max_dist goes through fit_f64_append (one hitting lane a wave and step).
//     The lane's record (sed_fit_index_dev.h), the reduce's walk and the append (sed_fit_f64_dp.h) are the one copies.
// The block is one wave (SED_FIT_BLOCK = 64): blockIdx.x = the chunk record, blockIdx.y = the query within its R group.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_fit_f64_dp.h"
#include "sed_fit_index_dev.h"

namespace {

static_assert(SED_FIT_BLOCK == 64, "a block is one wave");

// pw = the lane's R pattern codes, one byte each from bit 0 of pw[0] on
template <int R, bool HITS>
__device__ __forceinline__ void fit_long_f64_dp(const sed_fit_lane &ln, const uint32_t (&pw)[(R + 3) / 4], const double *tab,
                                                const uint32_t *__restrict__ text, sed_fit_f64_best *best,
                                                const fit_f64_hit_list &hl, double ins, double del) {
    // (a word's four columns of 32 rows unrolled spill, as in sed_fit_long.hip)
    constexpr int COLS_UNROLLED = R >= 32 ? 1 : 4;
    const int lane = (int)threadIdx.x;
    const int npad = 64 * R - ln.plen;    // G[1 .. npad] are front rows
    const int g0 = lane * R;              // G[g0] is the row above the lane's first
    const int nf = npad - g0;             // the lane's registers r < nf are front rows
    const int32_t jb = ln.c0 - ln.lead;   // the border column
    double D[R];
    int32_t S[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = g0 + r + 1 - npad;  // the pattern row of the register
        D[r] = i > 0 ? (double)i * del : 0.0;
        S[r] = jb;
    }
    // G[g0]'s cell of the column before the lane's: the top row's diagonal
    double tpD = g0 > npad ? (double)(g0 - npad) * del : 0.0;
    int32_t tpS = jb;
    uint32_t tsym = 0;
    int32_t jj = -lane;  // the lane's column, counted from the border column
    double bD = __builtin_inf();
    int32_t bS = 0, bE = 0;
    // an owned border column (lead = 0: column 0 of the text) is a column: D = P delete, start = end = 0
    if (HITS) {
        fit_f64_append(hl, lane == 63 && ln.lead == 0 && D[R - 1] <= hl.max_dist, ln.pair, ln.c0, jb, D[R - 1]);
    } else if (ln.lead == 0) {
        bD = D[R - 1];
        bS = jb;
        bE = ln.c0;
    }
    const uint32_t *tp = text + ln.tw;
    const int total = ln.nsteps + 63;
    uint32_t wnext = ln.nsteps > 0 ? tp[0] : 0u;
    for (int s = 0; s < total && ln.nsteps > 0; s += 4) {
        const uint32_t w = wnext;
        wnext = s + 4 < ln.nsteps ? tp[(s >> 2) + 1] : 0u;  // no word past the chunk's last: the skew's tail reads zeros
#pragma unroll COLS_UNROLLED
        for (int k = 0; k < 4; ++k) {
            const uint32_t sym0 = (w >> (8 * k)) & (uint32_t)(F64_K - 1);  // lane 0's column s + k + 1
            ++jj;
            const bool act = jj >= 1;
            const int32_t j = jb + jj;
            const double upD = dpp_shr1_f64(0.0, D[R - 1]);  // lane 0: row 0 of its column
            const int32_t upS = (int32_t)dpp_shr1((uint32_t)j, (uint32_t)S[R - 1]);
            tsym = dpp_shr1(sym0, tsym);
            if (act) {
                double dgD = tpD, aboveD = upD;
                int32_t dgS = tpS, aboveS = upS;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t a = (pw[r >> 2] >> (8 * (r & 3))) & (uint32_t)(F64_K - 1);
                    const double cost = tab[a * F64_K + tsym];
                    const double oldD = D[r];
                    const int32_t oldS = S[r];
                    double vD = oldD + ins;  // insert (left)
                    int32_t vS = oldS;
                    fit_f64_take(vD, vS, aboveD + del, aboveS);  // delete (up)
                    fit_f64_take(vD, vS, dgD + cost, dgS);       // update (diagonal)
                    const bool front = r < nf;
                    D[r] = front ? 0.0 : vD;
                    S[r] = front ? j : vS;
                    aboveD = D[r];
                    aboveS = S[r];
                    dgD = oldD;
                    dgS = oldS;
                }
            }
            tpD = upD;
            tpS = upS;
            const int32_t u = jj - ln.lead;  // the column's index among the owned ones
            const bool owned = act && lane == 63 && (uint32_t)u < (uint32_t)ln.cnt;
            if (HITS) {
                fit_f64_append(hl, owned && D[R - 1] <= hl.max_dist, ln.pair, j, S[R - 1], D[R - 1]);
            } else {
                const bool take = owned && D[R - 1] < bD;
                bD = take ? D[R - 1] : bD;
                bS = take ? S[R - 1] : bS;
                bE = take ? j : bE;
            }
        }
    }
    if (!HITS && lane == 63) *best = sed_fit_f64_best{bD, bS, bE};
}

template <int R> struct LongF64Waves { static constexpr int value = R <= 4 ? 8 : R == 8 ? 5 : R == 16 ? 3 : 2; };

template <int R>
__global__ __launch_bounds__(SED_FIT_BLOCK, LongF64Waves<R>::value) void sed_fit_index_long_f64_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint8_t *__restrict__ pats, const int32_t *__restrict__ plens, const int32_t *__restrict__ qlist, int q0,
    const uint32_t *__restrict__ text, sed_fit_f64_best *__restrict__ rec, int32_t chunk, int32_t W,
    const double *__restrict__ sub, double ins, double del) {
    __shared__ double tab[F64_K * F64_K];
    fit_f64_fill_tab(tab, sub);
    if ((int)blockIdx.x >= nchunks) return;
    uint32_t pw[(R + 3) / 4];
    int q;
    const sed_fit_lane ln = sed_fit_long_lane<R>(chunks, texts, ntexts, pats, plens, qlist, q0, chunk, W, pw, &q);
    fit_long_f64_dp<R, false>(ln, pw, tab, text, rec + (size_t)q * nchunks + blockIdx.x, fit_f64_hit_list{}, ins, del);
}

// sed_fit_f64.hip: sed_fit_index_f64_reduce_kernel, the query taken from the group's list
__global__ __launch_bounds__(SED_FIT_BLOCK) void sed_fit_index_long_f64_reduce_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, int ntexts, const int32_t *__restrict__ qlist, int q0,
    const sed_fit_f64_best *__restrict__ rec, sed_fit_f64_best *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks || chunks[t].c0 != 0) return;
    const int q = qlist[q0 + (int)blockIdx.y];
    const int32_t d = chunks[t].text;
    out[(size_t)q * ntexts + d] =
        fit_f64_first_min(rec + (size_t)q * nchunks, t, nchunks, [&](int k) { return chunks[k].text == d; });
}

template <int R>
__global__ __launch_bounds__(SED_FIT_BLOCK, LongF64Waves<R>::value) void sed_fit_index_long_f64_hits_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint8_t *__restrict__ pats, const int32_t *__restrict__ plens, const int32_t *__restrict__ qlist, int q0,
    const uint32_t *__restrict__ text, sed_fit_f64_hit *__restrict__ hits, unsigned long long *__restrict__ count,
    unsigned long long cap, double max_dist, int32_t chunk, int32_t W, const double *__restrict__ sub, double ins,
    double del) {
    __shared__ double tab[F64_K * F64_K];
    fit_f64_fill_tab(tab, sub);
    if ((int)blockIdx.x >= nchunks) return;
    uint32_t pw[(R + 3) / 4];
    int q;
    const sed_fit_lane ln = sed_fit_long_lane<R>(chunks, texts, ntexts, pats, plens, qlist, q0, chunk, W, pw, &q);
    fit_long_f64_dp<R, true>(ln, pw, tab, text, nullptr, fit_f64_hit_list{hits, count, cap, max_dist}, ins, del);
}

}  // namespace

hipError_t sed_launch_fit_index_long_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                         const int32_t *qlist, int rows, sed_fit_f64_best *rec, sed_fit_f64_best *out,
                                         const sed_fit_f64_costs &fc) {
    return sed_fit_long_with_rows(rows, [&](auto R) {
        return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(sed_fit_index_long_f64_kernel<decltype(R)::value>, dim3((unsigned)a.nchunks, (unsigned)nq),
                                  dim3(SED_FIT_BLOCK), 0, stream, e0, nullptr, 0, a.chunks, a.nchunks, a.texts, a.ntexts,
                                  (const uint8_t *)a.pats, a.plens, qlist, q0, (const uint32_t *)a.text, rec, a.chunk, a.W, fc.sub,
                                  fc.ins, fc.del);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            const dim3 grid((unsigned)((a.nchunks + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK), (unsigned)nq);
            hipExtLaunchKernelGGL(sed_fit_index_long_f64_reduce_kernel, grid, dim3(SED_FIT_BLOCK), 0, stream, nullptr, e1, 0,
                                  a.chunks, a.nchunks, a.ntexts, qlist, q0, (const sed_fit_f64_best *)rec, out);
            return hipGetLastError();
        });
    });
}

hipError_t sed_launch_fit_index_long_f64_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                              const int32_t *qlist, int rows, sed_fit_f64_hit *hits, unsigned long long *count,
                                              unsigned long long cap, double max_dist, const sed_fit_f64_costs &fc) {
    return sed_fit_long_with_rows(rows, [&](auto R) {
        return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(sed_fit_index_long_f64_hits_kernel<decltype(R)::value>, dim3((unsigned)a.nchunks, (unsigned)nq),
                                  dim3(SED_FIT_BLOCK), 0, stream, e0, e1, 0, a.chunks, a.nchunks, a.texts, a.ntexts,
                                  (const uint8_t *)a.pats, a.plens, qlist, q0, (const uint32_t *)a.text, hits, count, cap, max_dist,
                                  a.chunk, a.W, fc.sub, fc.ins, fc.del);
            return hipGetLastError();
        });
    });
}
