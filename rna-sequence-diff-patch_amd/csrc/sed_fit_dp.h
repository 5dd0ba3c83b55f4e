// sed_fit_dp.h - the DP of fit search, shared by sed_fit_kernel, sed_fit_index_kernel and sed_fit_index_hits_kernel
// (sed_fit.hip, whose header comment describes the keys): from the block's kappa table to what the lane reports, one
// copy of the arithmetic.  A kernel fills the table (sed_fit_fill_tab, every thread of the block), finds its lane
// record and the pattern's two 16-byte words its own way, and calls sed_fit_dp (the lane's 64-bit atomic minimum of
// the sink row) or sed_fit_dp_hits (every owned column whose sink key is within a cutoff, appended to a hit list).
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

constexpr int FIT_ROWS = SED_LANE_MAXM;
constexpr int FIT_REBASE = 128;  // columns between rebases of the insert offset

// tab[9]: kappa bytes of pattern symbol a for text symbols 0..7; row 8 (front rows): zeros
__device__ __forceinline__ void sed_fit_fill_tab(uint2 *tab, const sed_fit_params &fp) {
    if (threadIdx.x < 9)
        tab[threadIdx.x] = threadIdx.x < 8 ? make_uint2(fp.row[threadIdx.x][0], fp.row[threadIdx.x][1]) : make_uint2(0u, 0u);
    __syncthreads();
}

// The hit list of sed_fit_index_hits_kernel: rec[slot] = (pair, end, end - start, scaled D), slots handed out by one
// atomic add per wave and column step on *count, which counts every hit; a hit whose slot is >= cap is not stored.
// cut = the scaled cutoff (sed_fit_plan.cpp: sed_fit_cutoff_rule), from which the lane takes its own P delete.
struct sed_fit_hit_list {
    uint4 *rec;
    unsigned long long *count;
    unsigned long long cap;
    int32_t cut;
};

// One hit of the lane, decided for the whole wave (sed_dev.h: wave_claim_slot).  tt = (D - P delete) << 16 | (end - start).
__device__ __forceinline__ void sed_fit_append(const sed_fit_hit_list &hl, bool hit, int32_t pair, int32_t end, int32_t tt,
                                               uint32_t pdel) {
    unsigned long long slot;
    if (wave_claim_slot(hl.count, hit, &slot) && slot < hl.cap)
        hl.rec[slot] = make_uint4((uint32_t)pair, (uint32_t)end, (uint32_t)tt & 0xFFFFu, (uint32_t)((tt >> 16) + (int32_t)pdel));
}

// q0, q1 = the pattern, right-aligned in 32 byte codes, code 8 in front of it (sed_fit_runtime.cpp: fit_pack_pattern).
// HITS = false: the sink row's first strict minimum goes to out[ln.pair]; HITS = true: every owned column within
// hl.cut goes to the hit list, and out is not touched.
template <bool HITS>
__device__ __forceinline__ void sed_fit_dp_t(const sed_fit_lane &ln, const uint4 q0, const uint4 q1, const uint2 *tab,
                                             const uint32_t *__restrict__ text, unsigned long long *__restrict__ out,
                                             const sed_fit_hit_list &hl, const sed_fit_params &fp) {
    static_assert(FIT_ROWS == 32, "a pattern record is two 16-byte words");
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
    const int32_t thr = HITS ? hl.cut - (int32_t)pdel : 0;     // a column is a hit when D - P delete <= thr
    if (HITS) sed_fit_append(hl, ln.lead == 0 && 0 <= thr, ln.pair, ln.c0, 0, pdel);  // (the same border column)
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
            if (HITS) {
                sed_fit_append(hl, (uint32_t)u < (uint32_t)ln.cnt && (tt >> 16) <= thr, ln.pair, ln.c0 + u, tt, pdel);
            } else {
                const int32_t c = (int32_t)((uint32_t)tt & 0xFFFF0000u) | (u & 0xFFFF);
                const bool take = (uint32_t)u < (uint32_t)ln.cnt && c < (int32_t)((uint32_t)bestc & 0xFFFF0000u);
                bestc = take ? c : bestc;
                bestt = take ? tt : bestt;
            }
        }
        if ((s & (FIT_REBASE - 1)) == FIT_REBASE - 4) {
            inj += rebase;
#pragma unroll
            for (int r = 0; r <= FIT_ROWS; ++r) V[r] += rebase;
        }
    }
    if (HITS) return;
    const uint32_t D = (uint32_t)((bestt >> 16) + (int32_t)pdel);
    const uint32_t len = (uint32_t)bestt & 0xFFFFu;
    const uint32_t end = (uint32_t)ln.c0 + ((uint32_t)bestc & 0xFFFFu);
    atomicMin(out + ln.pair, ((unsigned long long)D << 48) | ((unsigned long long)end << 16) | len);
}

__device__ __forceinline__ void sed_fit_dp(const sed_fit_lane &ln, const uint4 q0, const uint4 q1, const uint2 *tab,
                                           const uint32_t *__restrict__ text, unsigned long long *__restrict__ out,
                                           const sed_fit_params &fp) {
    sed_fit_dp_t<false>(ln, q0, q1, tab, text, out, sed_fit_hit_list{}, fp);
}
__device__ __forceinline__ void sed_fit_dp_hits(const sed_fit_lane &ln, const uint4 q0, const uint4 q1, const uint2 *tab,
                                                const uint32_t *__restrict__ text, const sed_fit_hit_list &hl,
                                                const sed_fit_params &fp) {
    sed_fit_dp_t<true>(ln, q0, q1, tab, text, nullptr, hl, fp);
}
