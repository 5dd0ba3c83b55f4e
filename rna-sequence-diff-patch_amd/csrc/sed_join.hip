// sed_join.hip — similarity join over short sequences (include/sed.h: sed_join_self, sed_join_search): every (row,
// column) pair of 0..32 symbols whose distance is within a cutoff, appended to a hit list on the device.
//
// The lane kernels (sed_lane.hip) give every lane its own pair; here a lane owns a COLUMN sequence (str2) and the wave
// walks the rows (str1).  The lane builds what depends on its column once - the 32 perm selectors of the scaled DP, or
// the two bit planes E0 / E1 of the bit-parallel variant - and runs SED_JOIN_G rows against it.  A row is uniform across
// the wave: its length, its symbols and its 8-byte cost row come from scalar loads, and the row loop has one trip count
// for all 64 lanes.  The cells are sed_lane_dp.h's, shared with the lane kernels, so the scaled distance D * S is the
// lane kernels' number.
//
// The walk over the rows - the self rule, the length skip by ballot, the two counters - and the append are
// sed_join_dev.h's, shared with the kernel for longer sequences (sed_join_long.hip); the append and the launch also with
// the fp64 route (sed_join_f64.hip).  The columns are sorted by length,
// so the 64 columns of a wave have nearly one length, and the skip leaves out whole waves.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_lane_dp.h"
#include "sed_join_dev.h"

namespace {

// Walk = what is done with a row's distances (sed_join_dev.h): sed_join_walk_all is the join; the two sed_join_walk_knn
// are the passes of the k-nearest calls, with arguments of their own around the join's.
template <bool BITPAR, class Walk = sed_join_walk_all>
__global__ __launch_bounds__(SED_JOIN_BLOCK) void sed_join_kernel(const uint32_t *__restrict__ rows,
                                                                  const int32_t *__restrict__ row_len,
                                                                  const uint2 *__restrict__ tab,
                                                                  const typename Walk::args wa) {
    // (rows, row_len, tab = a's, as restrict parameters: the hit list's stores cannot alias them, so their uniform
    // loads are scalar loads)
    const sed_join_args &a = Walk::join(wa);
    constexpr int MM = SED_JOIN_MAXLEN;
    static_assert(MM == 32, "a record is two 16-byte words; the bit-parallel state is one 32-bit word");
    const int t = blockIdx.x * SED_JOIN_BLOCK + threadIdx.x;
    const bool valid = t < a.s.ncols;
    const int tc = valid ? t : a.s.ncols - 1;  // (lanes past the last column stay in the wave and report nothing)
    const uint4 *pc = reinterpret_cast<const uint4 *>(a.s.cols) + 2 * (size_t)tc;
    const uint4 q0 = pc[0], q1 = pc[1];
    const int m = a.s.col_len[tc];
    const int orig = a.s.col_orig[tc];
    const uint32_t bw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    // what the lane keeps of its column
    uint32_t sel[BITPAR ? 1 : MM];
    uint32_t E0 = 0, E1 = 0;
    if constexpr (BITPAR) {
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            const uint32_t u = __builtin_amdgcn_ubfe(a.umap, 2 * ((bw[j >> 2] >> (8 * (j & 3))) & 7u), 2);
            E0 |= (u & 1u) << j;
            E1 |= (u >> 1) << j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < MM; ++j) sel[j] = sed_scaled_sel(bw[j >> 2] >> (8 * (j & 3)));
    }
    Walk::rows(row_len, wa, valid, m, orig, [&](int r, int n) -> uint32_t {
        const uint32_t *pr = rows + 8 * (size_t)r;
        uint32_t w0 = pr[0], w1 = pr[1];  // rows 0..3 and 4..7 (the buffer ends with spare words)
        if constexpr (BITPAR) {
            uint32_t Pv = ~0u, Mv = 0u;
            for (int i = 0; i < n; ++i) {
                const uint32_t c = (w0 >> (8 * (i & 3))) & 7u;
                if ((i & 3) == 3) {
                    w0 = w1;
                    w1 = pr[(i >> 2) + 2];
                }
                sed_bitpar_step(Pv, Mv, sed_bitpar_tq(E0, E1, __builtin_amdgcn_ubfe(a.umap, 2 * c, 2)));
            }
            return sed_bitpar_sink(n, m, Pv, Mv) << a.shift;
        } else {
            uint32_t V[MM + 1];
#pragma unroll
            for (int j = 0; j <= MM; ++j) V[j] = SED_KB;  // row 0 and column 0: the offset key B
            uint2 rt = tab[w0 & 7u];
            for (int i = 0; i < n; ++i) {
                const uint2 cur = rt;  // row i's costs; row i + 1's are read during this row
                const int i1 = i + 1;
                if ((i1 & 3) == 0) {
                    w0 = w1;
                    w1 = pr[(i1 >> 2) + 1];
                }
                rt = tab[(w0 >> (8 * (i1 & 3))) & 7u];
                sed_scaled_row<MM>(V, sel, cur);
            }
            uint32_t cap = V[0];  // m = 0: the border column
#pragma unroll
            for (int j = 1; j <= MM; ++j) cap = (j == m) ? V[j] : cap;
            return sed_scaled_decode(cap, n, m, a.ins, a.del);
        }
    });
}

}  // namespace

hipError_t sed_launch_join(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_args &a, bool bitpar) {
    return bitpar ? sed_join_launch(sed_join_kernel<true>, stream, ev0, ev1, a, a.tab)
                  : sed_join_launch(sed_join_kernel<false>, stream, ev0, ev1, a, a.tab);
}

hipError_t sed_launch_join_knn(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_args &a, bool bitpar,
                               bool emit) {
    using Bound = sed_join_walk_knn<false>;
    using Emit = sed_join_walk_knn<true>;
    if (bitpar)
        return emit ? sed_join_launch(sed_join_kernel<true, Emit>, stream, ev0, ev1, a, a.j.tab)
                    : sed_join_launch(sed_join_kernel<true, Bound>, stream, ev0, ev1, a, a.j.tab);
    return emit ? sed_join_launch(sed_join_kernel<false, Emit>, stream, ev0, ev1, a, a.j.tab)
                : sed_join_launch(sed_join_kernel<false, Bound>, stream, ev0, ev1, a, a.j.tab);
}
