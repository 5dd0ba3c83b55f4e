// sed_cktb.hip — the checkpoint traceback (sed_traceback_ck_kernel, config 4's script route) and its launcher, in a
// translation unit of its own so that it can be compiled with its own code-generation options (Makefile: CKTB_FLAGS).
// The tile sweep and walk it shares with sed_ck_codes_kernel are in sed_ck_tile.h.  A tile visit keeps its lane's code
// words in a uint32_t[NW] and the entry word's LDS inputs in two uint32_t[16]; by default the compiler promotes such
// arrays to single vector values of 12 / 16 registers (AMDGPUPromoteAlloca) and copies them whole at the joins between
// a visit's words (6 v_mov_b64 per word and per entry-word exit, ~60 VALU a visit against ~1320).  Built with promotion
// limited to 16-byte arrays, SROA splits them into separate registers after unrolling: no copies, same registers, no
// scratch.  The other kernels keep the default (several use more registers or scratch without the promotion).
#include <hip/hip_ext.h>
#include "sed_ck_tile.h"

template <int R, bool WAVE, int NW>
__device__ __forceinline__ void ck_traceback_pair(const sed_pair_desc &d, const int pair, const uint32_t q0,
                                                  const int lane, const uint32_t *__restrict__ seqa,
                                                  const uint32_t *__restrict__ seqb, const uint32_t *__restrict__ ck,
                                                  sed_result *__restrict__ res, uint32_t *__restrict__ ops,
                                                  const sed_i32_params &prm, uint32_t *__restrict__ topb,
                                                  uint32_t *__restrict__ selb,
                                                  const sed_band bw = sed_band{SED_BAND_OPEN_LO, SED_BAND_OPEN_HI},
                                                  const int2 *__restrict__ win = nullptr) {
    constexpr int ROWS = 64 * R, G = Grp<R>::G;  // a tile: G forward lanes (bands) of R rows
    static_assert(R == 4 || R == 8 || R == 16, "R in {4, 8, 16}");
    const int n = d.n, m = d.m;
#ifdef SED_TB_DEBUG
    int visit = 0;  // debug dumps: 136 words per tile visit (entry keys, initial keys, coordinates)
#endif
    uint32_t *out = ops + d.ops_off;
#ifndef SED_TB_DEBUG
    zero_script_tail(out, (int)q0, n, m, lane, 64);  // (before the walk, as sed_traceback_kernel)
#endif
    uint32_t q = q0, err = 0;
    uint64_t acc = 0;  // the last 32 ops, the latest (position q) in bits 1:0
    auto emit = [&](uint32_t op) {  // sink -> origin (trailing border runs)
        if (q == 0) {
            err = SED_ERR_TB_LENGTH;
            return;
        }
        acc = (acc << 2) | op;
        if ((--q & 15u) == 0) out[q >> 4] = (uint32_t)acc;
    };
    const uint32_t Kd = (prm.del << 16) + 4u, Ki = (prm.ins << 16) + 4u;
    int i = n, j = m;
    if (i > 0 && j > 0) {
        const CkPairCtx px = ck_pair_ctx<R>(d, lane, seqa, seqb, ck, 0);
        // band pruning: the forward computed stripe k from column 64 clo + 1 on, and the stripe above it stored no
        // bottom row past step tophi; both change only when the walk enters another stripe
        int kband = -1, clo = 0, clo_prev = 0, tophi = 0x7FFFFFFF;
        uint32_t one = 1u;  // the delete candidate's +1, a VGPR operand of v_add_u32_dpp
        asm volatile("" : "+v"(one));
        int guard = 2 * (n + m) + 8;       // tiles visited; every visit makes progress
        while (i > 0 && j > 0) {
            if (--guard <= 0) {
                err = SED_ERR_TB_GUARD;
                break;
            }
            const int k = (i - 1) / ROWS, t = ((i - 1) % ROWS) / R, Q = t / G;
            const int ce = (j - 1 + t) >> 6;            // the entry cell's chunk
            if (k != kband) {  // (uniform; once per stripe)
                int hi_;
                tophi = 0x7FFFFFFF;
                clo_prev = 0;
                if (win) {  // refined windows: the ranges the forward of this run stored, stripe by stripe
                    if (k >= 1) {
                        const int2 wp = win[k - 1];
                        clo_prev = __builtin_amdgcn_readfirstlane(wp.x);
                        tophi = 64 * __builtin_amdgcn_readfirstlane(wp.y) + 63;
                    }
                    clo = __builtin_amdgcn_readfirstlane(win[k].x);
                } else {
                    if (k >= 1) {
                        sed_band_chunks(n, m, ROWS, px.nchunks, bw, k - 1, &clo_prev, &hi_);
                        tophi = 64 * hi_ + 63;
                    }
                    sed_band_chunks(n, m, ROWS, px.nchunks, bw, k, &clo, &hi_);
                }
                kband = k;
            }
            // every optimal path stays inside the window, so a walk that arrives left of it followed keys the forward
            // never wrote
            if (j <= 64 * clo) {
                err = SED_ERR_TB_BAND;
                break;
            }
            const int rowbase = k * ROWS + 64 * Q;
            const int re = i - rowbase - 1;             // the entry cell's tile row
            // NW = 12: a window of two chunks (ce - 1, ce) when the entry step x inside its chunk is below re, i.e. when
            // a diagonal path would leave chunk ce through its left edge before the tile's top: the path then crosses
            // the row group in one visit instead of two, 151 against 93 sweep steps per visit but half the visits
            // (22.3 -> 17.1 VALU per emitted op on config 4's pairs, tools/tb_window_model.py)
            const int c = (NW > 8 && ce > clo && ((j - 1 + t) & 63) < re) ? ce - 1 : ce;
            const int J0 = 64 * c - G * Q + 1;
            const int sig_end = (j - J0 + G - 1) + re;  // the entry cell's sweep step (<= 16 NW - 2)
            uint32_t W[NW], vinit = 0;
            const uint32_t ent = ck_tile_sweep<R, WAVE, false, NW>(px, lane, prm, topb, selb, k, Q, c, sig_end, one, W, vinit,
                                                                   clo, clo_prev, tophi);
            (void)vinit;
#ifdef SED_TB_DEBUG
            if (visit < 32) {  // debug builds only (pair 0; its script words, 64 spare, then 136 words per visit v)
                uint32_t *dv = out + ((n + m + 15) >> 4) + 64 + 136 * visit;
                dv[lane] = ent;
                dv[64 + lane] = vinit;
                if (lane == 0) {
                    dv[128] = (uint32_t)i; dv[129] = (uint32_t)j; dv[130] = (uint32_t)c; dv[131] = (uint32_t)Q;
                    dv[132] = (uint32_t)k; dv[133] = (uint32_t)sig_end; dv[134] = (uint32_t)re; dv[135] = q;
                }
            }
            ++visit;
#endif
            // ---- the entry cell's key must carry the ops still to emit (L of a canonical-path cell) ----
            {
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)ent, re) - SED_KB + (uint32_t)i * Kd +
                                   (uint32_t)j * Ki;
                if (((v >> 2) & 0x3FFFu) != q) {
                    err = SED_ERR_TB_CHECK;
                    break;
                }
            }
            // ---- walk inside the tile ----
            const uint32_t qin = q;
            const uint32_t S0 = (uint32_t)re | ((uint32_t)sig_end << 7);
            const uint32_t S = c == 0 ? ck_walk<true, NW>(W, S0, q, acc, err, out, j)
                                      : ck_walk<false, NW>(W, S0, q, acc, err, out, j);
            if (err) break;
            if (q == qin) {  // no progress: give up rather than spin
                err = SED_ERR_TB_STALL;
                break;
            }
            const int sg = (int)((S + 64u) >> 7), r = (int)((S + 64u) & 127u) - 64;
            i = rowbase + r + 1;
            j = J0 - (G - 1) + sg - r;
            ck_sync<WAVE>();  // topb / selb are rewritten for the next tile
        }
    }
    if (!err) {
        while (j > 0) { emit(0u); --j; }
        while (i > 0) { emit(1u); --i; }
        if (q != 0) err = SED_ERR_TB_LENGTH;
    }
#ifdef SED_TB_DEBUG
    if (lane == 0) out[((n + m + 15) >> 4) + 63] = err | ((uint32_t)visit << 8);  // (debug: no error, the dumps stay)
#else
    if (err && lane == 0) res[pair].err = (uint8_t)err;
#endif
}

// waves per SIMD the checkpoint traceback is compiled for (A/B: SED_CKTB_WAVES; 1 = the compiler's choice: 128 VGPRs and
// 4 waves with the two-chunk windows, whose c4 traceback span was 3.2-3.3 against 2.06 ms at 5 waves / 96 VGPRs, no
// spills; profiles/r06/ck_wide), and its
// waves' issue priority against the other part's forward waves on the same SIMD (SED_CKTB_PRIO, s_setprio).  At
// priority 1 the traceback's waves issue ahead of the forward's when both are ready, so a part's traceback ends
// sooner beside the other part's forward and the step's tracebacks-only tail shrinks from ~0.5 to ~0.13 ms: c4
// 9.74-9.79 against 9.91-9.98 ms at 0, 3 interleaved rounds (profiles/r05/s15; 3 is no different from 1).  With the
// two-chunk windows: 0 9.70-9.74 against 9.55-9.60 ms; 2 and 3 within noise of 1 over 4 rounds (profiles/r06/ckprio)
#ifndef SED_CKTB_WAVES
#define SED_CKTB_WAVES 5
#endif
#ifndef SED_CKTB_PRIO
#define SED_CKTB_PRIO 1
#endif
// code words per lane of the checkpoint traceback's sweep: 12 = two-chunk windows where they pay (ck_traceback_pair), 8 =
// one chunk per visit
#ifndef SED_CKTB_NW
#define SED_CKTB_NW 12
#endif
template <int R>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SED_CKTB_WAVES))) void sed_traceback_ck_kernel(const sed_pair_desc *__restrict__ pd, int npairs,
                                                              const uint32_t *__restrict__ seqa,
                                                              const uint32_t *__restrict__ seqb,
                                                              const uint32_t *__restrict__ ck,
                                                              sed_result *__restrict__ res,
                                                              uint32_t *__restrict__ ops, sed_i32_params prm,
                                                              const sed_band *__restrict__ band,
                                                              const int2 *__restrict__ win, int wstride) {
    if constexpr (SED_CKTB_PRIO > 0) __builtin_amdgcn_s_setprio(SED_CKTB_PRIO);
    const int lane = threadIdx.x;
    const int pair = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (pair >= npairs) return;
    const sed_pair_desc d = pd[pair];
    if (d.lane) return;  // scripted by sed_lane.hip
#ifdef SED_TB_DEBUG
    if (pair != 0) return;
#endif
    constexpr int NSEL = CkVHold<R>::value ? Grp<R>::G : 1, NW = SED_CKTB_NW;
    __shared__ uint32_t topb[SED_CK_NX(NW)], selb[NSEL * SED_CK_SELB(NW)];
    if constexpr (NSEL > 1) {
        for (int x = lane; x < NSEL * SED_CK_SELB(NW); x += 64) selb[x] = SED_SEL_SENT;  // (entries below 64: before column 1)
        __syncthreads();
    }
    const uint32_t q0 = (uint32_t)__builtin_amdgcn_readfirstlane(res[pair].len);
    sed_band bw{SED_BAND_OPEN_LO, SED_BAND_OPEN_HI};
    if (band) {
        bw.elo = __builtin_amdgcn_readfirstlane(band[pair].elo);
        bw.ehi = __builtin_amdgcn_readfirstlane(band[pair].ehi);
    }
    ck_traceback_pair<R, false, NW>(d, pair, q0, lane, seqa, seqb, ck, res, ops, prm, topb, selb, bw,
                                    win ? win + (size_t)pair * wstride : nullptr);
}

hipError_t sed_launch_traceback_ck(const sed_launch &L, uint32_t *ops, const sed_i32_params &prm) {
    const dim3 grid(L.npairs), block(64);
    const uint32_t *a = (const uint32_t *)L.seqa, *b = (const uint32_t *)L.seqb;
    const sed_band *bd = L.band;
    const int2 *win = L.band && L.bsuf ? L.bwin : nullptr;  // (refined windows only: the static ones are restated)
    const int ws = L.bstripes;
    return sed_for_R<4, 8, 16>(L.R, [&](auto r) {
        SED_LAUNCH(sed_traceback_ck_kernel<decltype(r)::value>, grid, block, 0, L, L.pd, L.npairs, a, b, L.tb, L.res, ops, prm,
                   bd, win, ws);
        return hipGetLastError();
    });
}
