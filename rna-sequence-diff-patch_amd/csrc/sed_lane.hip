// sed_lane.hip — lane-per-pair kernels for short str2 (m <= SED_LANE_MAXM): integer keys
// (distance, length, canonical script) and fp64 distance-only.
//
// Config 5 (all-vs-all over ~24-32 nt piRNAs, IRMethods.py:435-440 / 443-477) and the GUI's
// short pairs: a 64-lane wave per pair (sed_kernels.hip) would leave most lanes idle and spend
// ~m+63 systolic steps on a 32-column matrix.  Here one lane owns one pair and walks its matrix
// row by row (StringEditDistance.py:185-222 order) with the whole DP row in VGPRs: no DPP, no
// LDS, no inter-lane traffic; 64 pairs per wave, >= 4 waves per SIMD for 250k pairs.
//
// Cell keys are the offset keys of sed_i32_keys.h (W = V - i*(kdel - 1) - j*kins + B over
// V = D << 16 | L << 2 | op), so results (distance, L = script length, canonical op) are
// identical to the wave kernel's:
//   LEN:  candidates left, up + 1, diag + perm(costrow, -2, sel) -> v_min3 -> & ~3   (5 VALU)
//   !LEN: distance only, no L/op field: left, up, diag + perm(costrow, -1, sel)      (3 VALU)
// TB (implies LEN): the op of every cell (2 bits, 32 per row = one uint2) is stored per pair,
// row-major, and the same lane walks it back from (n, m) to write the canonical script.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"
#include "sed_lane_dp.h"

namespace {

template <bool LEN, bool TB>
__global__ __launch_bounds__(256) void sed_lane_i32_kernel(const sed_pair_desc *__restrict__ pd,
                                                           const int32_t *__restrict__ idx, int nidx,
                                                           const uint32_t *__restrict__ seqa,
                                                           const uint32_t *__restrict__ seqb,
                                                           uint32_t *__restrict__ tb, uint32_t *__restrict__ ops,
                                                           sed_result *__restrict__ res, sed_i32_params prm) {
    static_assert(LEN || !TB, "the traceback needs the op-count field");
    constexpr int MM = SED_LANE_MAXM;
    static_assert(MM == 32, "str2 codes are read as two 16-symbol words");
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nidx) return;
    const int pair = idx[t];
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;  // host guarantees 1 <= n <= SED_LANE_MAXN, 1 <= m <= MM
    const uint32_t s1 = LEN ? 0xFFFFFFFEu : 0xFFFFFFFFu;  // perm bytes 1:0 of the update constant
    // Transposed lookup: the lane keeps, per column j, the 4 costs cost(a -> b_j) as bytes of colw[j];
    // a row's symbol a_i becomes the perm selector, so a row costs 2 ops of setup instead of a
    // per-lane select of its cost row.  (Columns beyond m read the next pair's codes or padding:
    // don't-care, nothing flows from column j > m into columns <= m.)
    uint32_t colrow[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t w = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) w |= ((prm.costrow[a] >> (8 * b)) & 0xFFu) << (8 * a);
        colrow[b] = w;
    }
    const uint32_t *pb = seqb + d.b_off;
    const uint32_t wb0 = pb[0], wb1 = pb[1];
    uint32_t colw[MM], V[MM + 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        const uint32_t b = ((j < 16 ? wb0 : wb1) >> (2 * (j & 15))) & 3u;
        const uint32_t lo = (b & 1u) ? colrow[1] : colrow[0], hi = (b & 1u) ? colrow[3] : colrow[2];
        colw[j] = (b & 2u) ? hi : lo;
    }
#pragma unroll
    for (int j = 0; j <= MM; ++j) V[j] = SED_KB;  // row 0: j inserts (offset key B)
    const uint32_t *pa = seqa + d.a_off;
    uint32_t wa = 0;  // column 0 (i deletes) is the offset key B in every row
    uint2 *tbp = reinterpret_cast<uint2 *>(tb) + (TB ? d.tb_off / 2 : 0);
    for (int i = 0; i < n; ++i) {
        if ((i & 15) == 0) wa = pa[i >> 4];
        const uint32_t a = (wa >> (2 * (i & 15))) & 3u;
        const uint32_t sel = 0x0D000100u | ((4u + a) << 16);  // perm: byte3 <- 0xFF, byte2 <- cost byte a, 1:0 <- s1
        // update candidate of column j+1 is formed from the old V[j] before V[j] is overwritten,
        // so every V[j] is updated in place (no register rotation across the row loop)
        uint32_t dg = V[0] + __builtin_amdgcn_perm(colw[0], s1, sel);
        uint32_t left = V[0];  // stays B
        uint32_t W0 = 0, W1 = 0;
#pragma unroll
        for (int j = 1; j <= MM; ++j) {
            const uint32_t up = V[j];
            const uint32_t dnext = j < MM ? up + __builtin_amdgcn_perm(colw[j], s1, sel) : 0u;
            const uint32_t mm = umin3(left, LEN ? up + 1u : up, dg);  // insert (op 0), delete (op 1), update (op 2)
            dg = dnext;
            if constexpr (TB) {
                if (j <= 16) W0 = __builtin_amdgcn_alignbit(mm, W0, 2);
                else W1 = __builtin_amdgcn_alignbit(mm, W1, 2);
            }
            const uint32_t v = LEN ? (mm & ~3u) : mm;
            V[j] = v;
            left = v;
        }
        if constexpr (TB) tbp[i] = make_uint2(W0, W1);  // column j's op at bits 2(j-1) of the row's 64 bits
    }
    uint32_t cap = V[1];
#pragma unroll
    for (int j = 2; j <= MM; ++j) cap = (j == m) ? V[j] : cap;
    uint32_t D;
    int32_t L = -1;
    if constexpr (LEN) {  // back to V space: V = W - B + n*(kdel - 1) + m*kins
        const uint32_t v = cap - SED_KB + (uint32_t)n * (prm.kdel - 1u) + (uint32_t)m * prm.kins;
        D = v >> 16;
        L = (int32_t)((v >> 2) & 0x3FFFu);
    } else {
        D = (cap - SED_KB + (((uint32_t)n * prm.del + (uint32_t)m * prm.ins) << 16) + 0xFFFFu) >> 16;
    }
    sed_result r;
    r.dist = (double)D;
    r.len = L;
    r.is_int = (D == 0);
    r.err = 0;
    r.seq = 0;
    res[pair] = r;
    if constexpr (TB) {
        // canonical path, sink -> origin; op k of the script (origin -> sink) at bits 2(k&15) of word k>>4
        zero_script_tails_wave(ops, d.ops_off, L, n, m);  // (before the walk, as sed_traceback_kernel)
        uint32_t *po = ops + d.ops_off;
        int i = n, j = m, k = L - 1;
        uint32_t w = 0;
        while (k >= 0) {
            uint32_t op;
            if (i == 0) op = 0;
            else if (j == 0) op = 1;
            else {
                const uint2 rw = tbp[i - 1];
                op = ((j <= 16 ? rw.x : rw.y) >> (2 * ((j - 1) & 15))) & 3u;
            }
            w |= op << (2 * (k & 15));
            if ((k & 15) == 0) {
                po[k >> 4] = w;
                w = 0;
            }
            i -= (op != 0);
            j -= (op != 1);
            --k;
        }
    }
}

// Distance only, two pairs per lane (SED_NO_LEN batches: config 5, wfsearch).  Pair P lives in
// the low 16 bits of every cell word and pair Q in the high 16 bits; both have the same n, so one
// row loop serves both.  Each half is the 16-bit offset key of sed_kernels.hip's i32x2 kernel
// (W = D - i*delete - j*insert + 0xFFFF; the host checks n*delete + 32*insert <= 0xFFFF and that
// every substitution is cheaper than delete + insert), so packed 16-bit ops do two cells at once:
//   perm (P's and Q's update constants in one word) + v_pk_add_u16 + 2 v_pk_min_u16 = 4 VALU / 2 cells.

__global__ __launch_bounds__(256) void sed_lane_i32x2_kernel(const sed_pair_desc *__restrict__ pd,
                                                             const int32_t *__restrict__ idx, int nlanes,
                                                             const uint32_t *__restrict__ seqa,
                                                             const uint32_t *__restrict__ seqb,
                                                             sed_result *__restrict__ res, sed_i32_params prm) {
    constexpr int MM = SED_LANE_MAXM;
    static_assert(MM == 32, "str2 codes are read as two 16-symbol words");
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes) return;
    const int P = idx[2 * t], Q = idx[2 * t + 1];
    const sed_pair_desc dP = pd[P], dQ = pd[Q];
    const int n = dP.n, mP = dP.m, mQ = dQ.m;  // host guarantees dQ.n == n, 1 <= n <= MAXN, 1 <= m <= MM
    uint32_t colrow[4];  // transposed cost table, as in sed_lane_i32_kernel
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t w = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) w |= ((prm.costrow16[a] >> (8 * b)) & 0xFFu) << (8 * a);
        colrow[b] = w;
    }
    const uint32_t *pbP = seqb + dP.b_off, *pbQ = seqb + dQ.b_off;
    const uint32_t wP0 = pbP[0], wP1 = pbP[1], wQ0 = pbQ[0], wQ1 = pbQ[1];
    uint32_t colP[MM], colQ[MM], V[MM + 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        const uint32_t bp = ((j < 16 ? wP0 : wP1) >> (2 * (j & 15))) & 3u;
        const uint32_t bq = ((j < 16 ? wQ0 : wQ1) >> (2 * (j & 15))) & 3u;
        colP[j] = (bp & 2u) ? ((bp & 1u) ? colrow[3] : colrow[2]) : ((bp & 1u) ? colrow[1] : colrow[0]);
        colQ[j] = (bq & 2u) ? ((bq & 1u) ? colrow[3] : colrow[2]) : ((bq & 1u) ? colrow[1] : colrow[0]);
    }
#pragma unroll
    for (int j = 0; j <= MM; ++j) V[j] = 0xFFFFFFFFu;  // row 0 and column 0: offset key 0xFFFF, both halves
    const uint32_t *paP = seqa + dP.a_off, *paQ = seqa + dQ.a_off;
    uint32_t waP = 0, waQ = 0;
    for (int i = 0; i < n; ++i) {
        if ((i & 15) == 0) {
            waP = paP[i >> 4];
            waQ = paQ[i >> 4];
        }
        const uint32_t aP = (waP >> (2 * (i & 15))) & 3u, aQ = (waQ >> (2 * (i & 15))) & 3u;
        // perm: byte0 <- colP byte aP (S1), byte2 <- colQ byte aQ (S0), bytes 1, 3 <- 0xFF
        const uint32_t sel = 0x0D000D00u | aP | ((4u + aQ) << 16);
        uint32_t dg = pk_add(V[0], __builtin_amdgcn_perm(colQ[0], colP[0], sel));
        uint32_t left = V[0];  // column 0 stays 0xFFFF
#pragma unroll
        for (int j = 1; j <= MM; ++j) {
            const uint32_t up = V[j];
            const uint32_t dnext = j < MM ? pk_add(up, __builtin_amdgcn_perm(colQ[j], colP[j], sel)) : 0u;
            const uint32_t v = pk_min(pk_min(up, dg), left);  // left (this row's chain) enters last
            dg = dnext;
            V[j] = v;
            left = v;
        }
    }
    uint32_t capP = V[1], capQ = V[1];
#pragma unroll
    for (int j = 2; j <= MM; ++j) {
        capP = (j == mP) ? V[j] : capP;
        capQ = (j == mQ) ? V[j] : capQ;
    }
    sed_result r;
    r.len = -1;
    r.err = 0;
    r.seq = 0;
    // 16-bit offset keys back to D: D = W - 0xFFFF + n*delete + m*insert (mod 2^16)
    const uint32_t DP = ((capP & 0xFFFFu) + 1u + (uint32_t)n * prm.del + (uint32_t)mP * prm.ins) & 0xFFFFu;
    const uint32_t DQ = ((capQ >> 16) + 1u + (uint32_t)n * prm.del + (uint32_t)mQ * prm.ins) & 0xFFFFu;
    r.dist = (double)DP;
    r.is_int = (DP == 0);
    res[P] = r;
    r.dist = (double)DQ;
    r.is_int = (DQ == 0);
    res[Q] = r;
}

// Distance only under unit costs (insert = delete = 1, every mismatch 1: costs.json's ACGU block, config 5 and
// the IRMethods wf_score searches), one pair per lane, bit-parallel (Myers 1999, in Hyyrö's formulation for the
// global distance).  str2 (m <= 32) is the bit dimension: bit j-1 holds the vertical delta D[j] - D[j-1] of the
// current row as the pair (Pv, Mv) = (+1, -1) masks; every row of str1 updates all of them with ~18 word ops,
// and the top border's +1 per row enters as the carry-in of the shifted Ph.  Row 0 is D[j] = j (Pv all ones), so
// the sink is D[n][m] = n + popcount(Pv) - popcount(Mv) over bits 0..m-1 (StringEditDistance.py:146-182 borders,
// :92-128 recurrence; the values are integers, a Python int exactly when 0).  Bits at and above m hold don't-care
// values: additions carry and shifts move only upward, so they never reach bits below m.  The match masks come
// from two bit planes of str2's 2-bit codes: Eq = ~t with t = (E0 ^ c0) | (E1 ^ c1), c0/c1 = the row symbol's
// bits sign-extended; Eq itself is never formed (bfi folds the complement into its uses).
__device__ __forceinline__ uint32_t even_bits(uint32_t x) {  // bits 0, 2, .., 30 of x -> bits 0..15
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    return (x | (x >> 8)) & 0x0000FFFFu;
}
__global__ __launch_bounds__(256) void sed_lane_bitpar_kernel(const sed_pair_desc *__restrict__ pd,
                                                              const int32_t *__restrict__ idx, int nidx,
                                                              const uint32_t *__restrict__ seqa,
                                                              const uint32_t *__restrict__ seqb,
                                                              sed_result *__restrict__ res) {
    static_assert(SED_LANE_MAXM == 32, "str2 fits one 32-bit word of bit-parallel state");
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nidx) return;
    const int pair = idx[t];
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;  // host guarantees 1 <= n <= SED_LANE_MAXN, 1 <= m <= 32
    const uint32_t *pb = seqb + d.b_off, *pa = seqa + d.a_off;
    const uint32_t wb0 = pb[0], wb1 = pb[1];  // (the upload pads every sequence buffer)
    const uint32_t E0 = even_bits(wb0) | (even_bits(wb1) << 16);            // bit j: symbol j's low bit
    const uint32_t E1 = even_bits(wb0 >> 1) | (even_bits(wb1 >> 1) << 16);  // and its high bit
    uint32_t Pv = ~0u, Mv = 0u;
    uint32_t wa = pa[0];
    for (int i0 = 0; i0 < n; i0 += 16) {
        const uint32_t w = wa;
        if (i0 + 16 < n) wa = pa[(i0 >> 4) + 1];  // next word in flight during these 16 rows
        const int cnt = min(16, n - i0);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (u >= cnt) break;
            const uint32_t c0 = (uint32_t)__builtin_amdgcn_sbfe((int)w, 2 * u, 1);  // 0 or ~0
            const uint32_t c1 = (uint32_t)__builtin_amdgcn_sbfe((int)w, 2 * u + 1, 1);
            sed_bitpar_step(Pv, Mv, (E0 ^ c0) | (E1 ^ c1));  // ~Eq
        }
    }
    const uint32_t D = sed_bitpar_sink(n, m, Pv, Mv);
    sed_result r;
    r.dist = (double)D;
    r.len = -1;
    r.is_int = (D == 0);
    r.err = 0;
    r.seq = 0;
    res[pair] = r;
}

// fp64 distance-only variant (SED_MODE_F64 = "simple typing", SED_NO_LEN): short pairs whose
// alphabet or costs rule out the integer keys (IUPAC codes, N in piRNA data; config 5 with N).
// Cells follow the reference exactly: borders j*insert and i*delete are products
// (StringEditDistance.py:146-182), each candidate is one fp64 add, the value is the minimum
// (ties have equal values; in this mode a value is a Python int exactly when it is 0).
// The K x K cost table sits in LDS; a lane keeps per-column byte offsets into it.
// Pairs flagged by the host (d.pad[0]: every symbol in the unit-cost set `umask`, see sed_runtime.cpp:
// unit_subset) take the bit-parallel recurrence of sed_lane_bitpar_kernel instead: their distance does not depend
// on the other symbols' costs, and it is an integer, a Python int exactly when 0 (config 5 with N: the pairs
// without N).  The host puts them first in idx, so waves are uniform but for one.
__device__ __forceinline__ uint32_t unit_code(uint32_t c, uint32_t umask) {  // 2-bit index of code c in umask
    return (uint32_t)__builtin_popcount(umask & ((1u << c) - 1u));
}

// The unit-cost distance of a byte-coded pair whose symbols all lie in umask (sed_lane_bitpar_kernel's recurrence)
__device__ __forceinline__ uint32_t bitpar_bytes(const uint8_t *pa, const uint8_t *pb, int n, int m, uint32_t umask) {
    uint32_t E0 = 0, E1 = 0;
    for (int j = 0; j < m; ++j) {
        const uint32_t b = unit_code(pb[j], umask);
        E0 |= (b & 1u) << j;
        E1 |= (b >> 1) << j;
    }
    uint32_t Pv = ~0u, Mv = 0u;
    for (int i = 0; i < n; ++i) {
        const uint32_t a = unit_code(pa[i], umask);
        sed_bitpar_step(Pv, Mv, sed_bitpar_tq(E0, E1, a));
    }
    return sed_bitpar_sink(n, m, Pv, Mv);
}

template <int MM>
__global__ __launch_bounds__(256) void sed_lane_f64_kernel(const sed_pair_desc *__restrict__ pd,
                                                           const int32_t *__restrict__ idx, int nidx,
                                                           const uint8_t *__restrict__ seqa,
                                                           const uint8_t *__restrict__ seqb,
                                                           sed_result *__restrict__ res,
                                                           const double *__restrict__ gtab, double ins, double del,
                                                           int K, uint32_t umask) {
    __shared__ double tab[SED_MAX_K * SED_MAX_K];
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) tab[e] = gtab[2 * e];
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nidx) return;
    const int pair = idx[t];
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;  // host guarantees 1 <= n <= SED_LANE_MAXN, 1 <= m <= MM
    const uint8_t *pa = seqa + d.a_off, *pb = seqb + d.b_off;
    if (d.pad[0]) {  // unit costs over this pair's symbols: bit-parallel (sed_lane_bitpar_kernel)
        const uint32_t Dv = bitpar_bytes(pa, pb, n, m, umask);
        sed_result r;
        r.dist = (double)Dv;
        r.len = -1;
        r.is_int = (Dv == 0);
        r.err = 0;
        r.seq = 0;
        res[pair] = r;
        return;
    }
    uint32_t col[MM];  // byte offset of cost(., b_j) within a table row
    double V[MM + 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) col[j] = (j < m ? (uint32_t)pb[j] : 0u) * 8u;
#pragma unroll
    for (int j = 0; j <= MM; ++j) V[j] = (double)j * ins;
    const char *tb8 = reinterpret_cast<const char *>(tab);
    uint32_t a_next = pa[0];
    for (int i = 0; i < n; ++i) {
        const char *row = tb8 + a_next * (uint32_t)K * 8u;
        if (i + 1 < n) a_next = pa[i + 1];  // in flight during this row
        double dg = V[0] + *reinterpret_cast<const double *>(row + col[0]);
        V[0] = (double)(i + 1) * del;
        double left = V[0];
#pragma unroll
        for (int j = 1; j <= MM; ++j) {
            const double up = V[j];
            const double cdel = up + del;
            const double dnext = j < MM ? up + *reinterpret_cast<const double *>(row + col[j]) : 0.0;
            const double v = fmin(fmin(left + ins, cdel), dg);
            dg = dnext;
            V[j] = v;
            left = v;
        }
    }
    double D = V[1];
#pragma unroll
    for (int j = 2; j <= MM; ++j) D = (j == m) ? V[j] : D;
    sed_result r;
    r.dist = D;
    r.len = -1;
    r.is_int = (D == 0.0);
    r.err = 0;
    r.seq = 0;
    res[pair] = r;
}

// fp64 distance-only batches whose costs are dyadic over <= 8 symbols (costs.json with N: insert = delete = 1,
// updates 1 and 0.75; the reference maps X -> N on ingest, fa_import.py:61-62, so config 5 on real data meets N).
// Every cost times S = 2^k is an integer and the reference's fp64 sums of such values are exact (far below 2^53),
// so D * S is the integer DP of the scaled costs: the sed_lane_i32_kernel distance keys (offset keys, 3 VALU per
// cell: v_perm, v_add, v_min3), with an 8-symbol cost table.  The row symbol a_i picks its table row (8 bytes
// cost(a_i -> b), two registers, one LDS read per row, in flight during the row before), and each column keeps a
// perm selector whose byte 2 is its symbol b_j (0..3 select S1's bytes, 4..7 S0's): one v_perm per cell reads
// cost(a_i -> b_j).  The distance is D / S, a Python int exactly when it is 0, as in the fp64 path ("simple
// typing").  Pairs flagged by the host (d.pad[0]) run bit-parallel, as in sed_lane_f64_kernel.  Sequences are byte
// codes, each starting 16-byte aligned: str2 is two 16-byte loads, str1 one word per 4 rows.
template <int MM>
__global__ __launch_bounds__(256) void sed_lane_scaled_kernel(const sed_pair_desc *__restrict__ pd,
                                                              const int32_t *__restrict__ idx, int nidx,
                                                              const uint8_t *__restrict__ seqa,
                                                              const uint8_t *__restrict__ seqb,
                                                              sed_result *__restrict__ res, sed_scaled_params sp) {
    static_assert(MM == 32, "str2 is read as two 16-byte words");
    __shared__ uint2 tab[8];
    if (threadIdx.x < 8) tab[threadIdx.x] = make_uint2(sp.row[threadIdx.x][0], sp.row[threadIdx.x][1]);
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nidx) return;
    const int pair = idx[t];
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;  // host guarantees 1 <= n <= SED_LANE_MAXN, 1 <= m <= MM, codes < 8
    const uint4 *pb4 = reinterpret_cast<const uint4 *>(seqb + d.b_off);
    const uint4 q0 = pb4[0], q1 = pb4[1];  // (bytes past m: padding or the next sequence's codes, all < 8)
    const uint32_t bw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    const uint32_t *pa4 = reinterpret_cast<const uint32_t *>(seqa + d.a_off);
    uint32_t w0 = pa4[0], w1 = pa4[1];  // rows 0..3 and 4..7 (the upload pads the buffer)
    sed_result r;
    r.len = -1;
    r.err = 0;
    r.seq = 0;
    if (d.pad[0]) {  // unit costs over this pair's symbols: sed_lane_bitpar_kernel's recurrence
        uint32_t E0 = 0, E1 = 0;
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            const uint32_t u = __builtin_amdgcn_ubfe(sp.umap, 2 * ((bw[j >> 2] >> (8 * (j & 3))) & 7u), 2);
            E0 |= (u & 1u) << j;
            E1 |= (u >> 1) << j;
        }
        uint32_t Pv = ~0u, Mv = 0u;
        for (int i = 0; i < n; ++i) {
            const uint32_t a = (w0 >> (8 * (i & 3))) & 7u;
            if ((i & 3) == 3) {
                w0 = w1;
                w1 = pa4[(i >> 2) + 2];
            }
            const uint32_t u = __builtin_amdgcn_ubfe(sp.umap, 2 * a, 2);
            sed_bitpar_step(Pv, Mv, sed_bitpar_tq(E0, E1, u));
        }
        const uint32_t Dv = sed_bitpar_sink(n, m, Pv, Mv);
        r.dist = (double)Dv;
        r.is_int = (Dv == 0);
        res[pair] = r;
        return;
    }
    uint32_t sel[MM], V[MM + 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) sel[j] = sed_scaled_sel(bw[j >> 2] >> (8 * (j & 3)));
#pragma unroll
    for (int j = 0; j <= MM; ++j) V[j] = SED_KB;  // row 0 and column 0: the offset key B
    uint2 rt = tab[w0 & 7u];
    for (int i = 0; i < n; ++i) {
        const uint2 cur = rt;  // row i's costs; row i + 1's are read during this row
        const int i1 = i + 1;
        if ((i1 & 3) == 0) {
            w0 = w1;
            w1 = pa4[(i1 >> 2) + 1];
        }
        rt = tab[(w0 >> (8 * (i1 & 3))) & 7u];
        sed_scaled_row<MM>(V, sel, cur);
    }
    uint32_t cap = V[1];
#pragma unroll
    for (int j = 2; j <= MM; ++j) cap = (j == m) ? V[j] : cap;
    const uint32_t D = sed_scaled_decode(cap, n, m, sp.ins, sp.del);
    r.dist = (double)D * sp.inv_scale;  // exact: a power of two
    r.is_int = (D == 0);
    res[pair] = r;
}

}  // namespace

hipError_t sed_launch_lane_scaled(const sed_launch &L, const int32_t *idx, int nidx, const sed_scaled_params &sp) {
    if (nidx <= 0) return hipSuccess;
    SED_LAUNCH((sed_lane_scaled_kernel<SED_LANE_MAXM>), dim3((nidx + 255) / 256), dim3(256), 0, L, L.pd, idx, nidx,
               (const uint8_t *)L.seqa, (const uint8_t *)L.seqb, L.res, sp);
    return hipGetLastError();
}

hipError_t sed_launch_lane_f64(const sed_launch &L, const int32_t *idx, int nidx, const double *gtab, double ins,
                               double del, int K, uint32_t umask) {
    if (nidx <= 0) return hipSuccess;
    SED_LAUNCH((sed_lane_f64_kernel<SED_LANE_MAXM>), dim3((nidx + 255) / 256), dim3(256), 0, L, L.pd,
                       idx, nidx, (const uint8_t *)L.seqa, (const uint8_t *)L.seqb, L.res, gtab, ins, del, K, umask);
    return hipGetLastError();
}

hipError_t sed_launch_lane_bitpar(const sed_launch &L, const int32_t *idx, int nidx) {
    if (nidx <= 0) return hipSuccess;
    SED_LAUNCH(sed_lane_bitpar_kernel, dim3((nidx + 255) / 256), dim3(256), 0, L, L.pd, idx, nidx,
               (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.res);
    return hipGetLastError();
}

hipError_t sed_launch_lane_i32x2(const sed_launch &L, const int32_t *idx, int nlanes, const sed_i32_params &prm) {
    if (nlanes <= 0) return hipSuccess;
    SED_LAUNCH(sed_lane_i32x2_kernel, dim3((nlanes + 255) / 256), dim3(256), 0, L, L.pd, idx, nlanes,
                       (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.res, prm);
    return hipGetLastError();
}

hipError_t sed_launch_lane_i32(const sed_launch &L, const int32_t *idx, int nidx, const sed_i32_params &prm,
                               bool len) {
    if (nidx <= 0) return hipSuccess;
    const dim3 grid((nidx + 255) / 256), block(256);
    const uint32_t *a = (const uint32_t *)L.seqa, *b = (const uint32_t *)L.seqb;
    if (L.tb)
        SED_LAUNCH((sed_lane_i32_kernel<true, true>), grid, block, 0, L, L.pd, idx, nidx, a, b, L.tb,
                           L.ops, L.res, prm);
    else if (len)
        SED_LAUNCH((sed_lane_i32_kernel<true, false>), grid, block, 0, L, L.pd, idx, nidx, a, b,
                           nullptr, nullptr, L.res, prm);
    else
        SED_LAUNCH((sed_lane_i32_kernel<false, false>), grid, block, 0, L, L.pd, idx, nidx, a, b,
                           nullptr, nullptr, L.res, prm);
    return hipGetLastError();
}
