// sed_fit.hip — fit search (include/sed.h: sed_fit_search): the best approximate occurrence of a short pattern
// (1 <= P <= SED_LANE_MAXM) in a long text, one lane per (pair, chunk of text columns).
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
// A lane owns text columns [c0, c0 + cnt) and starts `lead` columns earlier (the planner's window W, sed_plan.cpp)
// from the border column i delete: on its own columns it computes the full matrix's keys.  After each owned column it
// keeps the first strict minimum of the sink row: V[32] - inj = (D - P delete) << 16 | (end - start), compared as
// (that's high half, owned column index) signed.  The lanes of a pair meet in one 64-bit atomic minimum on
// D << 48 | end << 16 | (end - start): smallest distance, then smallest end; the start in the key is the largest one.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"

namespace {

constexpr int FIT_ROWS = SED_LANE_MAXM;
constexpr int FIT_REBASE = 128;  // columns between rebases of the insert offset

__global__ __launch_bounds__(SED_FIT_BLOCK, 4) void sed_fit_kernel(const sed_fit_lane *__restrict__ lanes, int nlanes,
                                                                    const uint4 *__restrict__ pats,
                                                                    const uint32_t *__restrict__ text,
                                                                    unsigned long long *__restrict__ out,
                                                                    sed_fit_params fp) {
    static_assert(FIT_ROWS == 32, "a pattern record is two 16-byte words");
    __shared__ uint2 tab[9];  // kappa bytes of pattern symbol a for text symbols 0..7; row 8 (front rows): zeros
    if (threadIdx.x < 9)
        tab[threadIdx.x] = threadIdx.x < 8 ? make_uint2(fp.row[threadIdx.x][0], fp.row[threadIdx.x][1]) : make_uint2(0u, 0u);
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes) return;
    const sed_fit_lane ln = lanes[t];
    // the pattern, right-aligned in 32 byte codes, code 8 in front of it (sed_runtime.cpp packs the records)
    const uint4 q0 = pats[2 * (size_t)ln.pat], q1 = pats[2 * (size_t)ln.pat + 1];
    const uint32_t pw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t clo[FIT_ROWS], chi[FIT_ROWS];  // register r + 1's kappa bytes
#pragma unroll
    for (int r = 0; r < FIT_ROWS; ++r) {
        const uint2 e = tab[(pw[r >> 2] >> (8 * (r & 3))) & 15u];
        clo[r] = e.x;
        chi[r] = e.y;
    }
    const uint32_t pdel = (uint32_t)ln.plen * fp.del;
    const uint32_t rebase = ((uint32_t)FIT_REBASE * fp.ins) << 16;
    const uint32_t step = (fp.ins << 16) + 1u;  // row 0's key from one column to the next
    uint32_t inj = ((pdel << 16) + rebase) | 0xFFFFu;
    uint32_t V[FIT_ROWS + 1];
#pragma unroll
    for (int r = 0; r <= FIT_ROWS; ++r) V[r] = inj;  // the border column: D = i delete, start = this column
    // the sink row's first strict minimum over the owned columns: bestc = (D - P delete) << 16 | owned column index
    // (signed order), bestt = the same with end - start in the low half
    int32_t u = -ln.lead;  // the current column's index among the owned ones
    int32_t bestc = ln.lead == 0 ? 0 : 0x7FFFFFFF, bestt = 0;  // (an owned border column: D = P delete, start = end)
    const uint32_t *tp = text + ln.tw;
    uint32_t wnext = ln.nsteps > 0 ? tp[0] : 0u;
    for (int s = 0; s < ln.nsteps; s += 4) {
        const uint32_t w = wnext;
        wnext = tp[(s >> 2) + 1];  // in flight during these four columns (the text buffer ends with spare words)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // perm selector of this column: byte 2 <- kappa byte of the text symbol (0..3: clo, 4..7: chi), else 0
            const uint32_t sel = __builtin_amdgcn_perm(w, 0x0C0C0C0Cu, 0x00000000u | ((4u + k) << 16));
            inj -= step;
            uint32_t dg = V[0] - __builtin_amdgcn_perm(chi[0], clo[0], sel);
            V[0] = inj;
#pragma unroll
            for (int r = 1; r <= FIT_ROWS; ++r) {
                const uint32_t old = V[r];
                const uint32_t dnext = r < FIT_ROWS ? old - __builtin_amdgcn_perm(chi[r], clo[r], sel) : 0u;
                V[r] = umin3(old, V[r - 1], dg);  // insert (left), delete (up), update (diagonal)
                dg = dnext;
            }
            ++u;
            const int32_t tt = (int32_t)(V[FIT_ROWS] - inj);
            const int32_t c = (int32_t)((uint32_t)tt & 0xFFFF0000u) | (u & 0xFFFF);
            const bool take = (uint32_t)u < (uint32_t)ln.cnt && c < (int32_t)((uint32_t)bestc & 0xFFFF0000u);
            bestc = take ? c : bestc;
            bestt = take ? tt : bestt;
        }
        if ((s & (FIT_REBASE - 1)) == FIT_REBASE - 4) {
            inj += rebase;
#pragma unroll
            for (int r = 0; r <= FIT_ROWS; ++r) V[r] += rebase;
        }
    }
    const uint32_t D = (uint32_t)((bestt >> 16) + (int32_t)pdel);
    const uint32_t len = (uint32_t)bestt & 0xFFFFu;
    const uint32_t end = (uint32_t)ln.c0 + ((uint32_t)bestc & 0xFFFFu);
    atomicMin(out + ln.pair, ((unsigned long long)D << 48) | ((unsigned long long)end << 16) | len);
}

}  // namespace

hipError_t sed_launch_fit(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_lane *lanes, int nlanes,
                          const void *pats, const void *text, unsigned long long *out, const sed_fit_params &fp) {
    if (nlanes <= 0) return hipSuccess;
    hipExtLaunchKernelGGL(sed_fit_kernel, dim3((nlanes + SED_FIT_BLOCK - 1) / SED_FIT_BLOCK), dim3(SED_FIT_BLOCK), 0,
                          stream, ev0, ev1, 0, lanes, nlanes, (const uint4 *)pats, (const uint32_t *)text, out, fp);
    return hipGetLastError();
}
