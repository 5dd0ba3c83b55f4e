// sed_fit_long.hip — fit search for patterns of up to 2048 symbols (include/sed.h: sed_fit_index_search_long,
// sed_fit_index_hits_long).  The definition, the keys and the cell are sed_fit.hip's; what changes is
// where the rows live: one wave runs one (query, chunk record), its 64 lanes hold the pattern's rows, R consecutive
// rows a lane (R = 2, 4, 8, 16, 32: P <= 64 R), and the wave runs as a skewed wavefront.
//   - Registers.  The key registers G[0 .. 64 R] of the short kernel's V[0 .. 32]: G[0] is row 0's key, the pattern is
//     right-aligned in G[1 .. 64 R] behind front rows of code 8 (kappa 0, they hand row 0's key down), and the sink row
//     is G[64 R], the last register of lane 63, whatever P is.  Lane l holds G[l R + 1 .. l R + R] as V[0 .. R - 1].
//   - Skew.  At step t = 1, 2, ... lane l computes column j = t - l of its rows; j <= 0: the lane has not started, and
//     its registers stay at the border column's key because everything it receives is still in its initial state (the
//     border key, and a perm selector that picks kappa 0).  A wave runs nsteps + 63 steps, rounded up to the four
//     columns of a text word.
//   - Hand-over.  Each step a lane takes two words from lane l - 1 through wave_shr:1: `bottom`, the key of G[l R]
//     lane l - 1 produced one step earlier, which is that register's key of this lane's column j: the delete candidate
//     of the lane's top row; and `selv`, column j's perm selector, which lane 0 made from the text j - 1 steps ago.
//     The top row's update candidate comes from G[l R]'s key of column j - 1: the word received the step before
//     (top_prev).  Lane 0 keeps its own row 0 key inj (strictly decreasing) in place of a received word.
//   - Frames.  A key carries - l' insert + B (sed_fit.hip), l' = columns since the last rebase.  Every lane counts its
//     own columns and rebases after its own columns 128, 256, ...: it adds 128 insert << 16 to V, top_prev and inj.
//     So the offset a key of column j is computed under is a function of j alone, the same in every lane, and `bottom`
//     is handed down as computed, before the rebase: the lane below computes the same column j one step later, before
//     its own rebase.  top_prev, computed as a key of column j - 1, is the one received word that crosses a rebase, and
//     the lane's own rebase after column j - 1 moves it with the registers.
//   - Reporting.  Lane 63 owns the sink row: per owned column V[R - 1] - inj = (D - P delete) << 16 | (end - start),
//     inj being row 0's key of the lane's own column.  D = that high half + P delete mod 2^16 (P delete may exceed
//     32767 here, so the high half is not read as signed).  The result words are the short kernels': the 64-bit atomic
//     minimum on D << 48 | end << 16 | (end - start), or a record of the hit list (sed_fit_dp.h).
// The block is one wave (SED_FIT_BLOCK = 64): blockIdx.x = the chunk record, blockIdx.y = the query within its R group.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_fit_dp.h"
#include "sed_fit_index_dev.h"

namespace {

static_assert(SED_FIT_BLOCK == 64, "a block is one wave");

// pw = the lane's R pattern codes, one byte each from bit 0 of pw[0] on
template <int R, bool HITS>
__device__ __forceinline__ void sed_fit_long_dp_t(const sed_fit_lane &ln, const uint32_t (&pw)[(R + 3) / 4],
                                                  const uint2 *tab, const uint32_t *__restrict__ text,
                                                  unsigned long long *__restrict__ out, const sed_fit_hit_list &hl,
                                                  const sed_fit_params &fp) {
    // (a word's four columns of 32 rows unrolled spill; rolled, the loop's own instructions are 1 in 30)
    constexpr int COLS_UNROLLED = R >= 32 ? 1 : 4;
    const int lane = (int)threadIdx.x;
    uint32_t clo[R], chi[R];  // register r's kappa bytes
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint2 e = tab[(pw[r >> 2] >> (8 * (r & 3))) & 15u];
        clo[r] = e.x;
        chi[r] = e.y;
    }
    const uint32_t pdel = (uint32_t)ln.plen * fp.del;
    const uint32_t rebase = ((uint32_t)FIT_REBASE * fp.ins) << 16;
    const uint32_t step = (fp.ins << 16) + 1u;  // row 0's key from one column to the next
    uint32_t inj = ((pdel << 16) + rebase) | 0xFFFFu;
    uint32_t V[R];
#pragma unroll
    for (int r = 0; r < R; ++r) V[r] = inj;  // the border column: D = i delete, start = this column
    uint32_t top_prev = inj, bottom = inj;   // G[l R] of the column before, and what lane l + 1 reads next step
    uint32_t selv = 0x0C0C0C0Cu;             // (kappa 0 until a column's selector arrives)
    int32_t j = -lane;                       // the lane's column
    // the sink row's first strict minimum over the owned columns (lane 63): D, the owned column index, V - inj
    int32_t bestd = ln.lead == 0 ? (int32_t)pdel : 0x10000, bestu = 0;
    uint32_t bestt = 0;                      // (an owned border column: D = P delete, start = end)
    // (sed_fit_append stores (tt & 0xFFFF, (tt >> 16) + its last argument): handed end - start and D, it stores them)
    if (HITS) sed_fit_append(hl, lane == 63 && ln.lead == 0 && (int32_t)pdel <= hl.cut, ln.pair, ln.c0, 0, pdel);
    const uint32_t *tp = text + ln.tw;
    const int total = ln.nsteps + 63;
    uint32_t wnext = ln.nsteps > 0 ? tp[0] : 0u;
    for (int s = 0; s < total && ln.nsteps > 0; s += 4) {
        const uint32_t w = wnext;
        wnext = s + 4 < ln.nsteps ? tp[(s >> 2) + 1] : 0u;  // no word past the chunk's last: the skew's tail reads zeros
#pragma unroll COLS_UNROLLED
        for (int k = 0; k < 4; ++k) {
            // lane 0's column s + k + 1: byte 2 of its selector <- the kappa byte of the text symbol, else 0
            const uint32_t sel0 = __builtin_amdgcn_perm(w, 0x0C0C0C0Cu, 0x00000000u | ((4u + k) << 16));
            ++j;
            const bool act = j >= 1;
            inj -= act ? step : 0u;
            const uint32_t up = dpp_shr1(inj, bottom);  // lane 0: row 0's key of its column
            selv = dpp_shr1(sel0, selv);
            uint32_t dg = top_prev - __builtin_amdgcn_perm(chi[0], clo[0], selv);
            uint32_t above = up;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t old = V[r];
                const int rn = r + 1 < R ? r + 1 : r;  // the register below, whose update candidate this one's old key makes
                const uint32_t dnext = r + 1 < R ? old - __builtin_amdgcn_perm(chi[rn], clo[rn], selv) : 0u;
                V[r] = umin3(old, above, dg);  // insert (left), delete (up), update (diagonal)
                above = V[r];
                dg = dnext;
            }
            top_prev = up;
            bottom = V[R - 1];
            const uint32_t tt = V[R - 1] - inj;
            const int32_t u = j - ln.lead;  // the column's index among the owned ones
            const int32_t d = (int32_t)(((tt >> 16) + pdel) & 0xFFFFu);
            const bool own = act && (uint32_t)u < (uint32_t)ln.cnt;
            if (HITS) {
                sed_fit_append(hl, own && lane == 63 && d <= hl.cut, ln.pair, ln.c0 + u, (int32_t)(tt & 0xFFFFu), (uint32_t)d);
            } else {
                const bool take = own && d < bestd;
                bestd = take ? d : bestd;
                bestu = take ? u : bestu;
                bestt = take ? tt : bestt;
            }
            if (act && (j & (FIT_REBASE - 1)) == 0) {  // the lane's own columns 128, 256, ...
                inj += rebase;
                top_prev += rebase;
#pragma unroll
                for (int r = 0; r < R; ++r) V[r] += rebase;
            }
        }
    }
    if (HITS || lane != 63) return;
    const uint32_t end = (uint32_t)ln.c0 + (uint32_t)bestu;
    atomicMin(out + ln.pair, ((unsigned long long)(uint32_t)bestd << 48) | ((unsigned long long)end << 16) | (bestt & 0xFFFFu));
}

template <int R> struct LongWaves { static constexpr int value = R <= 8 ? 8 : 4; };  // waves per SIMD the registers allow

template <int R>
__global__ __launch_bounds__(SED_FIT_BLOCK, LongWaves<R>::value) void sed_fit_index_long_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint8_t *__restrict__ pats, const int32_t *__restrict__ plens, const int32_t *__restrict__ qlist, int q0,
    const uint32_t *__restrict__ text, unsigned long long *__restrict__ out, int32_t chunk, int32_t W, sed_fit_params fp) {
    __shared__ uint2 tab[9];
    sed_fit_fill_tab(tab, fp);
    if ((int)blockIdx.x >= nchunks) return;
    uint32_t pw[(R + 3) / 4];
    int q;  // (not used: these kernels report by ln.pair)
    const sed_fit_lane ln = sed_fit_long_lane<R>(chunks, texts, ntexts, pats, plens, qlist, q0, chunk, W, pw, &q);
    sed_fit_long_dp_t<R, false>(ln, pw, tab, text, out, sed_fit_hit_list{}, fp);
}

template <int R>
__global__ __launch_bounds__(SED_FIT_BLOCK, LongWaves<R>::value) void sed_fit_index_long_hits_kernel(
    const sed_fit_chunk *__restrict__ chunks, int nchunks, const sed_fit_text *__restrict__ texts, int ntexts,
    const uint8_t *__restrict__ pats, const int32_t *__restrict__ plens, const int32_t *__restrict__ qlist, int q0,
    const uint32_t *__restrict__ text, uint4 *__restrict__ hits, unsigned long long *__restrict__ count,
    unsigned long long cap, int32_t cut, int32_t chunk, int32_t W, sed_fit_params fp) {
    __shared__ uint2 tab[9];
    sed_fit_fill_tab(tab, fp);
    if ((int)blockIdx.x >= nchunks) return;
    uint32_t pw[(R + 3) / 4];
    int q;  // (not used: these kernels report by ln.pair)
    const sed_fit_lane ln = sed_fit_long_lane<R>(chunks, texts, ntexts, pats, plens, qlist, q0, chunk, W, pw, &q);
    sed_fit_long_dp_t<R, true>(ln, pw, tab, text, nullptr, sed_fit_hit_list{hits, count, cap, cut}, fp);
}

}  // namespace

// One R group's launches (sed_internal.h: sed_fit_long_with_rows, sed_fit_each_query_group), as sed_fit_long_f64.hip's
hipError_t sed_launch_fit_index_long(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                     const int32_t *qlist, int rows, const sed_fit_params &fp) {
    return sed_fit_long_with_rows(rows, [&](auto R) {
        return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(sed_fit_index_long_kernel<decltype(R)::value>, dim3((unsigned)a.nchunks, (unsigned)nq),
                                  dim3(SED_FIT_BLOCK), 0, stream, e0, e1, 0, a.chunks, a.nchunks, a.texts, a.ntexts,
                                  (const uint8_t *)a.pats, a.plens, qlist, q0, (const uint32_t *)a.text, a.out, a.chunk, a.W, fp);
            return hipGetLastError();
        });
    });
}

hipError_t sed_launch_fit_index_long_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                          const int32_t *qlist, int rows, void *hits, unsigned long long *count,
                                          unsigned long long cap, int32_t cut, const sed_fit_params &fp) {
    return sed_fit_long_with_rows(rows, [&](auto R) {
        return sed_fit_each_query_group(a.nchunks, a.nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(sed_fit_index_long_hits_kernel<decltype(R)::value>, dim3((unsigned)a.nchunks, (unsigned)nq),
                                  dim3(SED_FIT_BLOCK), 0, stream, e0, e1, 0, a.chunks, a.nchunks, a.texts, a.ntexts,
                                  (const uint8_t *)a.pats, a.plens, qlist, q0, (const uint32_t *)a.text, (uint4 *)hits, count, cap,
                                  cut, a.chunk, a.W, fp);
            return hipGetLastError();
        });
    });
}
