// sed_join_long.hip — similarity join over sequences of 0..128 symbols (include/sed.h: sed_join_long_self,
// sed_join_long_search): sed_join.hip's layout and semantics with a longer record.  A lane owns a COLUMN sequence (str2),
// the wave walks the rows (str1), a row's length, symbols and cost row are wave-uniform scalar loads, and the walk over
// the rows, the length skip and the append are the short kernel's own code (sed_join_dev.h).  The cells are
// sed_lane_dp.h's.
//
// Scaled DP: V[0 .. 128] as 32-bit offset keys in registers.  The column stays as its 32 words of byte codes: one perm
// with a code word as selector looks four cost bytes up in the row symbol's 8-byte cost row, and one perm per cell with
// a constant selector expands a byte into the update addend, so a cell costs perm, add, umin3 and a quarter of the
// look-up.  (SED_JOIN_LONG_SELREGS builds the other layout for comparison: one selector register per column, as the
// short kernel keeps them; DESIGN.md 3.6m has both resource reports.)  The unrolled row runs in blocks of
// SED_JOIN_LONG_BLOCK columns, each behind a wave-uniform test on the wave's longest column: the index stores the
// columns sorted by length, so a wave of 40-symbol columns runs 64 cells a row, not 128.  Every register index is static.
//
// Bit-parallel: sed_bitpar_word over four 32-bit words, the addition's carry and the shifts' top bits handed from word to
// word; words above the wave's longest column are not run, and the sink masks to m bits word by word.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_lane_dp.h"
#include "sed_join_dev.h"

namespace {

#ifdef SED_JOIN_LONG_SELREGS
constexpr bool kSelRegs = true;
#else
constexpr bool kSelRegs = false;
#endif

// Walk = what is done with a row's distances (sed_join_dev.h): the join, or a pass of the k-nearest calls.
template <bool BITPAR, bool SELREGS, class Walk = sed_join_walk_all>
__global__ __launch_bounds__(SED_JOIN_BLOCK) void sed_join_long_kernel(const uint32_t *__restrict__ rows,
                                                                       const int32_t *__restrict__ row_len,
                                                                       const uint2 *__restrict__ tab,
                                                                       const typename Walk::args wa) {
    // (rows, row_len, tab = a's, as restrict parameters: the hit list's stores cannot alias them, so their uniform
    // loads are scalar loads)
    const sed_join_args &a = Walk::join(wa);
    constexpr int MM = SED_JOIN_LONG_MAXLEN, BL = SED_JOIN_LONG_BLOCK, NW = MM / 4, NB = MM / BL;
    static_assert(BL == 32 && NB == 4, "a block of columns is one word of bit-parallel state; four of them a record");
    const int t = blockIdx.x * SED_JOIN_BLOCK + threadIdx.x;
    const bool valid = t < a.s.ncols;
    const int tc = valid ? t : a.s.ncols - 1;  // (lanes past the last column stay in the wave and report nothing)
    const uint4 *pc = reinterpret_cast<const uint4 *>(a.s.cols) + (NW / 4) * (size_t)tc;
    uint32_t cw[NW];  // the column's byte codes, four a word
#pragma unroll
    for (int k = 0; k < NW / 4; ++k) {
        const uint4 q = pc[k];
        cw[4 * k] = q.x & 0x07070707u, cw[4 * k + 1] = q.y & 0x07070707u;
        cw[4 * k + 2] = q.z & 0x07070707u, cw[4 * k + 3] = q.w & 0x07070707u;
    }
    const int m = a.s.col_len[tc];
    const int orig = a.s.col_orig[tc];
    // the blocks of columns (the words of state) the wave's longest column reaches: uniform, 0..4
    int nblk = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) nblk += __builtin_amdgcn_ballot_w64(m > BL * b) != 0 ? 1 : 0;
    if constexpr (BITPAR) {
        uint32_t E0[NB] = {}, E1[NB] = {};  // the column's two bit planes
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            const uint32_t u = __builtin_amdgcn_ubfe(a.umap, 2 * ((cw[j >> 2] >> (8 * (j & 3))) & 7u), 2);
            E0[j >> 5] |= (u & 1u) << (j & 31);
            E1[j >> 5] |= (u >> 1) << (j & 31);
        }
        Walk::rows(row_len, wa, valid, m, orig, [&](int r, int n) -> uint32_t {
            const uint32_t *pr = rows + NW * (size_t)r;
            uint32_t w0 = pr[0], w1 = pr[1];  // rows 0..3 and 4..7 (the buffer ends with spare words)
            uint32_t Pv[NB], Mv[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) Pv[k] = ~0u, Mv[k] = 0u;
            for (int i = 0; i < n; ++i) {
                const uint32_t c = (w0 >> (8 * (i & 3))) & 7u;
                if ((i & 3) == 3) {
                    w0 = w1;
                    w1 = pr[(i >> 2) + 2];
                }
                const uint32_t u = __builtin_amdgcn_ubfe(a.umap, 2 * c, 2);
                uint32_t cadd = 0, cph = 1u, cmh = 0;  // (the top border's +1 enters word 0 only)
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    if (k < nblk) sed_bitpar_word(Pv[k], Mv[k], sed_bitpar_tq(E0[k], E1[k], u), cadd, cph, cmh);
            }
            uint32_t D = (uint32_t)n;  // plus the vertical deltas of row n over the column's m bits
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if (k < nblk) D += sed_bitpar_sink(0, max(m - BL * k, 0), Pv[k], Mv[k]);
            return D << a.shift;
        });
    } else {
        uint32_t sel[SELREGS ? MM : 1];
        if constexpr (SELREGS) {
#pragma unroll
            for (int j = 0; j < MM; ++j) sel[j] = sed_scaled_sel(cw[j >> 2] >> (8 * (j & 3)));
        }
        Walk::rows(row_len, wa, valid, m, orig, [&](int r, int n) -> uint32_t {
            const uint32_t *pr = rows + NW * (size_t)r;
            uint32_t w0 = pr[0], w1 = pr[1];
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
                // the addend of column j + 1: the selector register's perm, or the code word's four cost bytes (one perm
                // a word: the four cells' calls are one value) and the byte's expansion to 0xFF, byte, 0xFF, 0xFF
                auto addend = [&](int j) -> uint32_t {
                    if constexpr (SELREGS) {
                        return __builtin_amdgcn_perm(cur.y, cur.x, sel[j]);
                    } else {
                        const uint32_t p = __builtin_amdgcn_perm(cur.y, cur.x, cw[j >> 2]);
                        return __builtin_amdgcn_perm(p, p, 0x0D000D0Du | ((uint32_t)(j & 3) << 16));
                    }
                };
                uint32_t left = V[0];  // stays B
                uint32_t dg = V[0] + addend(0);
                if (nblk > 0) {
                    sed_scaled_cols<MM, 0, BL>(V, left, dg, addend);
                    if (nblk > 1) {
                        sed_scaled_cols<MM, BL, 2 * BL>(V, left, dg, addend);
                        if (nblk > 2) {
                            sed_scaled_cols<MM, 2 * BL, 3 * BL>(V, left, dg, addend);
                            if (nblk > 3) sed_scaled_cols<MM, 3 * BL, 4 * BL>(V, left, dg, addend);
                        }
                    }
                }
            }
            uint32_t cap = V[0];  // m = 0: the border column
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nblk) {
#pragma unroll
                    for (int j = BL * b + 1; j <= BL * (b + 1); ++j) cap = (j == m) ? V[j] : cap;
                }
            return sed_scaled_decode(cap, n, m, a.ins, a.del);
        });
    }
}

}  // namespace

hipError_t sed_launch_join_long(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_args &a, bool bitpar) {
    return bitpar ? sed_join_launch(sed_join_long_kernel<true, false>, stream, ev0, ev1, a, a.tab)
                  : sed_join_launch(sed_join_long_kernel<false, kSelRegs>, stream, ev0, ev1, a, a.tab);
}

hipError_t sed_launch_join_long_knn(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_args &a,
                                    bool bitpar, bool emit) {
    using Bound = sed_join_walk_knn<false>;
    using Emit = sed_join_walk_knn<true>;
    if (bitpar)
        return emit ? sed_join_launch(sed_join_long_kernel<true, false, Emit>, stream, ev0, ev1, a, a.j.tab)
                    : sed_join_launch(sed_join_long_kernel<true, false, Bound>, stream, ev0, ev1, a, a.j.tab);
    return emit ? sed_join_launch(sed_join_long_kernel<false, kSelRegs, Emit>, stream, ev0, ev1, a, a.j.tab)
                : sed_join_launch(sed_join_long_kernel<false, kSelRegs, Bound>, stream, ev0, ev1, a, a.j.tab);
}
