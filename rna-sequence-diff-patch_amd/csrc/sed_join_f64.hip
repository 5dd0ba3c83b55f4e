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
// The same kernel body serves the k-nearest calls of this route (include/sed.h: sed_join_knn_self_f64,
// sed_join_knn_search_f64) as two further instantiations, chosen by `if constexpr`: the join's own instantiation
// compiles to the instructions it had as a plain kernel.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_join_dev.h"

namespace {

constexpr int JF_K = SED_JOIN_F64_MAXK;

// What the kernel is instantiated over (sed_join_dev.h's walks are the integer kernels'): the join itself, and the two
// passes of the k-nearest calls (sed_internal.h: sed_join_knn_f64_args).  skip = what the length skip reads: the join's
// keep words, or the passes' 33 x 33 table low[33 n + m] <= every D of a row of n and a column of m symbols.
struct sed_join_f64_all {
    using args = sed_join_f64_args;
    using skip = unsigned long long;
    static constexpr int pass = 0;
    static __device__ __forceinline__ const sed_join_f64_args &join(const args &a) { return a; }
};
template <int PASS>
struct sed_join_f64_knn {
    using args = sed_join_knn_f64_args;
    using skip = double;
    static constexpr int pass = PASS;  // 1: the bound pass, 2: the emit pass
    static __device__ __forceinline__ const sed_join_f64_args &join(const args &a) { return a.j; }
};

// The k nearest columns of every row (pass 1 and 2 below).  A distance is finite or +inf and >= +0, and the bit
// patterns of such doubles order as unsigned 64-bit integers exactly as the values do (sign bit 0: exponent, then
// fraction, most significant first; +inf = 0x7FF0..0 is above every finite one).  So bound[r] is a 64-bit word that
// holds a double's bits, it starts at max_dist's, and the integer passes of sed_join_dev.h carry over with the bits as
// the key: nothing is scaled or rounded.
// Pass 1, the bound pass: per row b = bound[r] (a relaxed agent-scope atomic load, made uniform: other waves lower it
// meanwhile, and a stale value is a larger one, which only prunes less).  A lane takes part when its column is in scope
// and low[33 n + m] <= b; low <= D (sed_join_plan.h: sed_join_f64_lower_rule), so a lane left out has D > b and the
// candidates {in scope, D <= b} are the same with or without the skip.  A wave with at least k candidates finds d_k,
// their k-th smallest D: those k all lie <= b, so d_k is the wave's true k-th smallest among its columns in scope,
// whatever b was, and it is >= the row's k-th smallest; one lane lowers bound[r] to it (64-bit unsigned atomicMin).  A
// wave with fewer than k candidates has no k-th smallest <= b and writes nothing.  Take any schedule and let w* be the
// wave of the smallest true k-th smallest d* among the waves that have k columns in scope within max_dist: every value
// ever written is some wave's true k-th smallest, so bound[r] >= min(max_dist, d*) throughout, hence w* reads b >= d*,
// counts its k columns <= d* as candidates, finds d* and writes it (or b = d* already).  So bound[r] ends as
// min(max_dist, the smallest k-th smallest of any wave that has k in-scope columns within max_dist), in every schedule.
// d_k by bisection on the key: bits 62..0 (bit 63, the sign, is 0), 63 rounds of compare, ballot and popcount; no loop
// depends on the data or waits for another wave.
// Pass 2, the emit pass: the join with b = bound[r] (final since pass 1 ended: one value for the whole wave) in place
// of max_dist, in the skip and the hit test alike.  It appends exactly {D <= bound[r]}.
template <class W>
__global__ __launch_bounds__(SED_JOIN_BLOCK) void sed_join_f64_kernel(const uint32_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ row_len,
                                                                      const double *__restrict__ sub,
                                                                      const typename W::skip *__restrict__ keep,
                                                                      const typename W::args wa) {
    // (rows, row_len, keep = a's, as restrict parameters: the hit list's stores cannot alias them, so their uniform
    // loads are scalar loads)
    const sed_join_f64_args &a = W::join(wa);
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
        bool go;
        double b = 0;  // (the passes: the row's bound, uniform)
        if constexpr (W::pass == 0) {
            const unsigned long long kn = keep[n];
            go = valid && !(a.s.self && orig == r) && ((kn >> m) & 1ull) != 0;
        } else {
            unsigned long long bb;
            if constexpr (W::pass == 1)
                bb = __hip_atomic_load(wa.bound + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                bb = wa.bound[r];
            // (the builtin returns an int: through uint32_t, or a low word with its top bit set would sign-extend)
            bb = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)bb) |
                 ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(bb >> 32)) << 32);
            b = __longlong_as_double((long long)bb);
            go = valid && !(a.s.self && orig == r) && keep[(SED_JOIN_MAXLEN + 1) * n + m] <= b;  // (a compare: no arithmetic)
        }
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
        if constexpr (W::pass == 0) {
            sed_join_append(a.out, go && D <= a.max_dist, r, orig, (uint32_t)bits, (uint32_t)(bits >> 32));
        } else if constexpr (W::pass == 2) {
            sed_join_append(a.out, go && D <= b, r, orig, (uint32_t)bits, (uint32_t)(bits >> 32));
        } else {
            const bool cand = go && D <= b;
            if (__popcll(__builtin_amdgcn_ballot_w64(cand)) < wa.k) continue;
            unsigned long long x = 0;  // the largest x with fewer than k candidates at key < x: the k-th smallest key
#pragma unroll 1
            for (int bit = 62; bit >= 0; --bit) {
                const unsigned long long c = x | (1ull << bit);
                if (__popcll(__builtin_amdgcn_ballot_w64(cand && bits < c)) < wa.k) x = c;
            }
            if (x < (unsigned long long)__double_as_longlong(b) && (threadIdx.x & 63) == 0) atomicMin(wa.bound + r, x);
        }
    }
    if (ran != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.out.count + 1, (unsigned long long)ran);
}

}  // namespace

hipError_t sed_launch_join_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_f64_args &a) {
    return sed_join_launch(sed_join_f64_kernel<sed_join_f64_all>, stream, ev0, ev1, a, a.sub, a.keep);
}

hipError_t sed_launch_join_knn_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_f64_args &a, bool emit) {
    return emit ? sed_join_launch(sed_join_f64_kernel<sed_join_f64_knn<2>>, stream, ev0, ev1, a, a.j.sub, a.low)
                : sed_join_launch(sed_join_f64_kernel<sed_join_f64_knn<1>>, stream, ev0, ev1, a, a.j.sub, a.low);
}
