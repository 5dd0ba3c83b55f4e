// sed_join_f64.hip — the similarity join in fp64 (include/sed.h: sed_join_self_f64, sed_join_search_f64): the route for
// the cost tables and alphabets the scaled-integer cells of sed_join.hip refuse.  The layout is sed_join.hip's: a lane
// owns a COLUMN sequence (str2), the block's waves walk SED_JOIN_G rows (str1), a row's length and symbols are uniform
// and come from scalar loads, grid = (column blocks of SED_JOIN_BLOCK lanes) x (row groups).  What differs is the cell.
//
// The DP is oracle/sed_oracle.c: sed_oracle_pair's D, operation for operation.  A lane keeps the current row of its
// column's matrix in registers, 33 fp64 values V[0..32] (V[j] = the cell of column prefix j), and its column's codes in
// the 8 words of its record.  A cell is
//     insert  V[j - 1] (this row)     + insert
//     delete  V[j] (the row above)    + delete
//     update  V[j - 1] (the row above) + sub[a][b_j]
// each ONE v_add_f64 (the unit is compiled with contraction off and holds no multiply beside the borders'), then two
// v_min_f64.  Every value is finite or +inf and >= +0 (the planner normalises -0.0), so the minimum of the three is the
// value of the oracle's first-minimum rule.  Nothing is scaled, offset or reassociated: the value of a cell is the
// oracle's value of that cell, bit for bit.
//   - row 0: V[j] = (double)j * insert, column 0 of row i: (double)i * delete; products, as the oracle writes them.
//   - columns past the lane's own length m run over the record's zero padding; nothing reads them: the sink is a select
//     over the registers at m, as in sed_join.hip's DP variant (here a tree over m's bits).
//   - the K x K table sits in LDS as SED_JOIN_F64_MAXK x SED_JOIN_F64_MAXK doubles, zeros past K; a cell reads
//     tab[16 a + b_j], a uniform.
// Length skip: keep[n] has bit m set when a pair of a row of n and a column of m symbols may be within max_dist; the
// planner (sed_join_plan.cpp: sed_join_f64_keep_rule) decides that on the host, conservatively under rounding
// (DESIGN.md 3.6l), and the kernel tests the bit: no floating point is involved in skipping.  A wave none of whose lanes
// has its bit set for the current row leaves that row out; count[1] counts the pairs whose bit was set.
// A hit is D <= max_dist, a plain fp64 compare; its record is (row, original column, D's low word, D's high word).
// The append and the launch are sed_join_dev.h's; the row loop is this kernel's own copy of sed_join_rows there (the
// shared walk, given the keep bit and the fp64 distance as parameters, compiled to another schedule).
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_join_dev.h"

namespace {

constexpr int JF_K = SED_JOIN_F64_MAXK;

__global__ __launch_bounds__(SED_JOIN_BLOCK) void sed_join_f64_kernel(const uint32_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ row_len,
                                                                      const double *__restrict__ sub,
                                                                      const unsigned long long *__restrict__ keep,
                                                                      const sed_join_f64_args a) {
    // (rows, row_len, keep = a's, as restrict parameters: the hit list's stores cannot alias them, so their uniform
    // loads are scalar loads)
    constexpr int MM = SED_JOIN_MAXLEN;
    static_assert(MM == 32 && JF_K == 16, "a record is two 16-byte words; a code indexes a table row of 16 doubles");
    __shared__ double tab[JF_K * JF_K];
    for (int e = threadIdx.x; e < JF_K * JF_K; e += SED_JOIN_BLOCK) tab[e] = sub[e];
    __syncthreads();
    const int t = blockIdx.x * SED_JOIN_BLOCK + threadIdx.x;
    const bool valid = t < a.s.ncols;
    const int tc = valid ? t : a.s.ncols - 1;  // (lanes past the last column stay in the wave and report nothing)
    const uint4 *pc = reinterpret_cast<const uint4 *>(a.s.cols) + 2 * (size_t)tc;
    const uint4 q0 = pc[0], q1 = pc[1];
    const int m = a.s.col_len[tc];
    const int orig = a.s.col_orig[tc];
    // the column's codes as byte offsets into a table row: 8 b_j, four to a word (b_j < 16: the planner's check)
    uint32_t bw[8] = {(q0.x & 0x0F0F0F0Fu) << 3, (q0.y & 0x0F0F0F0Fu) << 3, (q0.z & 0x0F0F0F0Fu) << 3,
                            (q0.w & 0x0F0F0F0Fu) << 3, (q1.x & 0x0F0F0F0Fu) << 3, (q1.y & 0x0F0F0F0Fu) << 3,
                            (q1.z & 0x0F0F0F0Fu) << 3, (q1.w & 0x0F0F0F0Fu) << 3};
    const char *tb = reinterpret_cast<const char *>(tab);
    const double ins = a.ins, del = a.del;
    const int rbeg = a.s.row0 + (int)blockIdx.y * SED_JOIN_G;
    const int rend = min(rbeg + SED_JOIN_G, a.s.row0 + a.s.nrows);
    uint32_t ran = 0;
    for (int r = rbeg; r < rend; ++r) {
        const int n = row_len[r];  // (uniform: a scalar load)
        const unsigned long long kn = keep[n];
        const bool go = valid && !(a.s.self && orig == r) && ((kn >> m) & 1ull) != 0;
        const unsigned long long gb = __builtin_amdgcn_ballot_w64(go);
        if (gb == 0) continue;  // no column of this wave can be within the cutoff of row r
        ran += (uint32_t)__popcll(gb);
        const uint32_t *pr = rows + 8 * (size_t)r;
        uint32_t w0 = pr[0], w1 = pr[1];  // rows 0..3 and 4..7 (the buffer ends with spare words)
        double V[MM + 1];
        double ins0 = ins;
        asm volatile("" : "+v"(ins0));  // (row 0 is rebuilt per row: 33 products hoisted out of the row loop cost 66 VGPRs)
#pragma unroll
        for (int j = 0; j <= MM; ++j) V[j] = (double)j * ins0;  // row 0
        for (int i = 0; i < n; ++i) {
            const uint32_t arow = ((w0 >> (8 * (i & 3))) & (uint32_t)(JF_K - 1)) * (uint32_t)(JF_K * sizeof(double));
            if ((i & 3) == 3) {
                w0 = w1;
                w1 = pr[(i >> 2) + 2];
            }
            // (the byte extracts stay in this loop: hoisted, the 32 offsets cost 32 VGPRs and an occupancy step)
#pragma unroll
            for (int w = 0; w < 8; ++w) asm volatile("" : "+v"(bw[w]));
            double dg = V[0];
            V[0] = (double)(i + 1) * del;  // column 0
#pragma unroll
            for (int j = 1; j <= MM; ++j) {
                const uint32_t bo = (bw[(j - 1) >> 2] >> (8 * ((j - 1) & 3))) & 0xFFu;
                const double cost = *reinterpret_cast<const double *>(tb + (arow + bo));
                const double up = V[j];
                // (the two candidates of the row above first: the chain from cell to cell is one add and one min; the
                // minimum of three values that are no NaN does not depend on the order)
                V[j] = __builtin_fmin(V[j - 1] + ins, __builtin_fmin(up + del, dg + cost));
                dg = up;
            }
        }
        // the sink V[m]: a select tree over m's bits (five masks for the whole kernel), then m = 32
#pragma unroll
        for (int s = 1; s < MM; s <<= 1)
#pragma unroll
            for (int j = 0; j < MM; j += 2 * s) V[j] = (m & s) ? V[j + s] : V[j];
        const double D = m == MM ? V[MM] : V[0];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(D);
        sed_join_append(a.out, go && D <= a.max_dist, r, orig, (uint32_t)bits, (uint32_t)(bits >> 32));
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.out.count + 1, (unsigned long long)ran);
}

}  // namespace

hipError_t sed_launch_join_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_f64_args &a) {
    return sed_join_launch(sed_join_f64_kernel, stream, ev0, ev1, a, a.sub, a.keep);
}
