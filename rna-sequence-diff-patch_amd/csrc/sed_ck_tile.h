// sed_ck_tile.h — recomputing one 64 x 64 tile from the forward kernels' checkpoints, and walking its codes: what the
// checkpoint traceback (sed_cktb.hip: sed_traceback_ck_kernel) and the SPLIT route's code tiles (sed_tb.hip:
// sed_ck_codes_kernel) share.
#pragma once
#include "sed_i32_keys.h"

// ---------------------------------------------------------------------------
// Traceback from checkpoints (CK: script batches of the stripe and CHAIN kernels with R = 4, 8 or 16 rows
// per lane, G = 64/R).  One wave per pair walks the canonical path back from (n, m) tile by tile.  A tile
// is 64 rows (forward lanes GQ .. GQ+G-1 of a stripe, the tile's G bands of R rows) x the 64 columns those
// lanes processed in one chunk c, a staircase: band t = GQ + b covers columns 64c - t + 1 .. 64c - t + 64.
// Entering a tile, the wave recomputes it from
//   - the column checkpoints of chunk c-1 (each band's R row values at column 64c - t, and the value
//     above the band at that column), or the column-0 borders for c = 0;
//   - the row above the tile: the row checkpoints of lane GQ-1 (or lane 63 of the stripe above, or
//     row 0), read through LDS by lane 0;
// with one lane per row (row r at sweep step sigma is at column J0 - (G-1) + sigma - r, J0 = 64c - GQ + 1;
// the cell above arrives through the DPP chain from lane r - 1, the str2 selector from LDS).  The forward kernel
// stores distance keys (D, L without the op); every checkpoint value is converted on load to the
// traceback key of the same (D, L) (i32_dist_to_tb), whose min carries the canonical op in its low two
// bits: 6 VALU per cell (v_add_u32_dpp for the cell above + 1, perm, add, min3, and, alignbit).  Lanes of
// band b hold their checkpoint until their first column (step r - b + G - 1: one v_cndmask on a scalar
// mask) and read code 3 there (outside the band's window, OR-ed in per word); the first row of bands
// 1..G-1 takes its first diagonal from the checkpoint; columns < 1 get the sentinel selector, so they keep
// the column-0 border.  The sweep stops after the 16-step word holding the entry cell's step (the path only
// goes up and left), and the entry cell's key must carry the path length still to emit: a mismatch (a
// corrupted checkpoint, SED_OPT_DEBUG_CORRUPT) sets res.err instead of writing a wrong script.  Codes stay
// in registers, 16 steps per word.  The walk is scalar: one v_readlane per step and the state packed as
// S = row + (step << 7), 10 SALU per step (a step moves S by 128 / 129 / 257 for insert / delete /
// update; one masked compare catches leaving the word, the tile (bit 6 = above it) and the window (code
// 3)), one unrolled copy per code word since the step only decreases.
// ---------------------------------------------------------------------------
// S decrement per code: insert 128, delete 129, update 257 (S = row | step << 7); the marker 3 (left of the
// band's window) moves S by 0x8000, out of every word, and is taken back at the exit.  Only the low 16 bits of S
// are kept: a move subtracts the next code's field << 16 as well.
#define SED_TB_MOVES (128ull | (129ull << 16) | (257ull << 32) | (0x8000ull << 48))
#define SED_TB_WORD 0xF840u  // S bits that change when the walk leaves a 16-step word or the tile (bit 6: above it)
// The walk of one tile from state S; returns the state of the first cell it did not take (outside the
// tile: above it, left of its band's window, or at column 0 for C0), low 16 bits.  One loop per code word with a
// single exit test: the next state's word bits (S & SED_TB_WORD) must still be the word's tag.
template <bool C0, int NW>  // C0: chunk-0 tile, whose window reaches the column-0 border: stop at j = 0
__device__ __forceinline__ uint32_t ck_walk(const uint32_t (&W)[NW], uint32_t S, uint32_t &q, uint64_t &acc,
                                            uint32_t &err, uint32_t *__restrict__ out, int jcol) {
    static_assert(NW <= 15, "the step field (S bits 7..14) and the word tags need a free bit 15");
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {
        const uint32_t tag = (uint32_t)w << 11;
        if ((S & SED_TB_WORD) == tag) {
            // Every op moves the walk at least one step left, so one word yields at most 16 ops.  Inside the loop
            // the state is carried as T = S - tag (same low 11 bits: lane and shift), so leaving the word, the tile or
            // the window is (T & SED_TB_WORD) != 0, one s_and that sets SCC; the codes collect in a 32-bit lo
            // (s_lshl2_add_u32), which holds all of them, and go onto the 64-bit acc (the last 32 ops) after the
            // loop, where the script word completed in it, if any, is stored.  A step is one v_readlane and 10 SALU.
            const uint32_t qs = q;
            uint32_t T = S - tag, lo = 0, code;
            do {
                // s_lshr takes the low 5 bits of T >> 6: 2 * (step & 15), bit 6 being clear inside the tile
                code = ((uint32_t)__builtin_amdgcn_readlane((int)W[w], (int)T) >> ((T >> 6) & 31u)) & 3u;
                if (C0 && jcol == 0) code = 3u;
                // the marker too: taken back below (asm: the compiler emits s_lshl + s_or; the op writes SCC)
                asm("s_lshl2_add_u32 %0, %1, %2" : "=s"(lo) : "s"(lo), "s"(code) : "scc");
                if constexpr (C0) jcol -= (int)((5u >> code) & 1u);
                T -= (uint32_t)(SED_TB_MOVES >> (code << 4));
                --q;
            } while ((T & SED_TB_WORD) == 0u);
            S = T + tag;
            const bool marker = code == 3u;
            // opaque: otherwise the compiler keeps the previous lo and q alive through the loop for the undo
            asm volatile("" : "+s"(lo), "+s"(q));
            if (marker) {  // not an op: the walk stays at the cell before it
                lo >>= 2;
                ++q;
            }
            // lo started at 0 and holds exactly this word's ops (at most 16)
            const uint32_t nw = qs - q;
            acc = (acc << (2u * nw)) | lo;
            // the script word [p, p + 16) completed in this word, if any: [q, qs) holds at most 16 positions, so at most
            // one p = 16k with q <= p < qs
            const uint32_t p = (q + 15u) & ~15u;
            if ((int32_t)nw < 0) err = SED_ERR_TB_LENGTH;  // ran past the sink's L (q wrapped; the tile bounds the walk)
            else if (p < qs) out[p >> 4] = (uint32_t)(acc >> (2u * (p - q)));
            if (marker) return (S + 0x8000u) & 0xFFFFu;
        }
    }
    return S & 0xFFFFu;
}

// SED_CK_VHOLD (default on; -DSED_CK_VHOLD=0 restores the select): at R = 16 lanes left of their window hold
// their key without a select (per-band selector copies carry the sentinel, and each band's first row takes a
// compensated delete addend until its band starts).  6 VALU per swept cell instead of 7; profiles/r03/vhold:
// traceback 3.78 against 3.91 ms beside the forward parts, step within noise
#ifndef SED_CK_VHOLD
#define SED_CK_VHOLD 1
#endif
// NW code words per lane cover sweep steps 0 .. 16 NW - 1: 8 for one chunk's tile (127 steps), 12 for a wide window
// of two chunks (191 steps); topb holds 16 NW + 4 words, each band's selector copy 64 more
#define SED_CK_NX(NW) (16 * (NW) + 4)
#define SED_CK_SELB(NW) (64 + SED_CK_NX(NW))
template <int R> struct CkVHold { static constexpr bool value = SED_CK_VHOLD && R == 16; };
// lanes 0 .. n-1 have reached their window at sweep step sig (sig0(r) = r - r/R + G - 1 is nondecreasing)
template <int R> constexpr int ck_active_lanes(int sig) {
    constexpr int G = 64 / R;
    int n = 0;
    for (int r = 0; r < 64; ++r)
        if (r - r / R + G - 1 <= sig) n = r + 1;
    return n;
}
// lanes >= act keep v, the others take vn: the mask is built on the scalar unit inside the asm, so the
// compiler can neither hoist the 60-odd constant masks (they spill) nor turn them into a VALU compare
__device__ __forceinline__ uint32_t ck_hold(uint32_t vn, uint32_t v, const int act) {
    uint32_t r;
    uint64_t m;
    // (s_lshl_b64 writes SCC: without the clobber a compare's SCC could be read across the asm)
    asm("s_lshl_b64 %1, -1, %4\n\tv_cndmask_b32 %0, %2, %3, %1" : "=v"(r), "=&s"(m) : "v"(vn), "v"(v), "i"(act) : "scc");
    return r;
}

// band b >= 1 of a tile starts (its first row takes the checkpoint's top_prev as diagonal) at sweep step
// (R - 1) b + G - 1; returns b, or 0 when `sig` starts no band
template <int R> constexpr int ck_band_start(int sig) {
    constexpr int G = 64 / R;
    for (int b = 1; b < G; ++b)
        if (sig == (R - 1) * b + G - 1) return b;
    return 0;
}

// a word at a 32-bit byte offset from a uniform base: the scalar-base (saddr) load form, no 64-bit lane address
__device__ __forceinline__ uint32_t ld_byte_off(const uint32_t *__restrict__ base, const uint32_t off) {
    return *(const uint32_t *)((const char *)base + off);
}

// LDS ordering inside the traceback: a workgroup barrier for the one-wave traceback kernel; WAVE: a wave-local
// wait, for a traceback run by a wave of a larger workgroup (LDS accesses of one wave execute in order; the
// clobber keeps the compiler from moving them across).  Fusing the traceback into the CK forward kernel this way
// (each wave walks its pair after its forward pass) measured 13.9-14.0 ms per config-4 step against 13.87 ms
// for the separate kernel (profiles/r02/abfuse), so the traceback stays a kernel of its own.
template <bool WAVE> __device__ __forceinline__ void ck_sync() {
    if constexpr (WAVE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else __syncthreads();
}

// topb[x] (132 words): the row above the tile at lane 0's column of step x, plus 1 (lane 0's delete candidate);
// selb[64 + x] (196 words): str2 selector of lane 0's column at step x; lane r reads selb[64 + sigma - r] itself
// (its column at step sigma), so no selector travels through the DPP chain.  q0: the sink's L.
// Per-pair constants of the checkpoint tiles.  ckoff: word offset of the checkpoints past d.tb_off (SPLIT batches keep
// them after the pair's per-cell code region, sed_ck_codes_kernel).
struct CkPairCtx {
    int n, m, SG, nchunks, ngroups, band;
    const uint32_t *ccp, *rcp, *pa, *pb;
    uint32_t cko0, cko1, hm[4];
};
template <int R>
__device__ __forceinline__ CkPairCtx ck_pair_ctx(const sed_pair_desc &d, const int lane, const uint32_t *__restrict__ seqa,
                                                 const uint32_t *__restrict__ seqb, const uint32_t *__restrict__ ck,
                                                 const uint64_t ckoff) {
    constexpr int ROWS = 64 * R, G = Grp<R>::G;
    constexpr int LR = R == 4 ? 2 : R == 8 ? 3 : 4;
    CkPairCtx px;
    px.n = d.n;
    px.m = d.m;
    const int nstripes = (d.n + ROWS - 1) / ROWS;
    px.SG = (d.m + 63 + G - 1) / G * G;
    px.nchunks = (px.SG + 63) >> 6;
    px.ngroups = px.SG / G;
    px.ccp = ck + d.tb_off + ckoff;
    px.rcp = px.ccp + sed_ck_col_words(R, nstripes, px.nchunks);
    px.pa = seqa + d.a_off;
    px.pb = seqb + d.b_off;
    px.band = lane >> LR;
    px.cko0 = ((uint32_t)(lane & (R - 1)) * 64u + (uint32_t)px.band) * 4u;
    px.cko1 = (uint32_t)(R * 64 + px.band) * 4u;
    const int sig0 = lane - px.band + G - 1;  // first real sweep step of this lane (<= 63)
    // code 3 (outside the window) for the steps before sig0, OR-ed into words 0..3 once they are complete
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int h = min(max(sig0 - 16 * w, 0), 16);
        px.hm[w] = h >= 16 ? ~0u : (1u << (2 * h)) - 1u;
    }
    return px;
}

// One tile visit: tile (stripe k, band group Q, chunk c) recomputed from its checkpoints up to sweep step sig_end (FULL:
// all 128 steps), the codes in W (lane r's code of step sigma in W[sigma >> 4], bits 2 (sigma & 15)); returns the lanes'
// keys after the last step (the entry keys).
template <int R, bool WAVE, bool FULL, int NW>
__device__ __forceinline__ uint32_t ck_tile_sweep(const CkPairCtx &px, const int lane, const sed_i32_params &prm,
                                                  uint32_t *__restrict__ topb, uint32_t *__restrict__ selb, const int k,
                                                  const int Q, const int c, const int sig_end, uint32_t &one,
                                                  uint32_t (&W)[NW], uint32_t &vinit, const int bclo = 0,
                                                  const int bclo_prev = 0, const int btophi = 0x7FFFFFFF) {
    constexpr int NX = SED_CK_NX(NW), SELB = SED_CK_SELB(NW), NH = (NX + 63) / 64;
    constexpr int ROWS = 64 * R, G = Grp<R>::G;  // a tile: G forward lanes (bands) of R rows
    constexpr int LR = R == 4 ? 2 : R == 8 ? 3 : 4;
    constexpr bool VHOLD = CkVHold<R>::value;
    const int n = px.n, m = px.m, SG = px.SG, nchunks = px.nchunks, ngroups = px.ngroups, band = px.band;
    const int J0 = 64 * c - G * Q + 1, rowbase = k * ROWS + 64 * Q;
    // band pruning: the forward ran stripe k from the border state at column jb = 64 bclo (bclo = 0: column 0 itself),
    // and the stripe above stored no bottom row past step btophi (both uniform, computed by the caller once per stripe;
    // the defaults are an open window's)
    const int jb = 64 * bclo, tophi = Q == 0 ? btophi : 0x7FFFFFFF;
    // ---- boundaries (distance keys -> traceback keys) ----
    // Every load of the tile is issued before the first use (one memory round trip per tile visit): addresses
    // are clamped to valid words and the border cases are selects afterwards.
    const int ir = min(rowbase + lane, n - 1);  // 0-based str1 index of this lane's row (clamped)
    const uint32_t wa = px.pa[ir >> 4];
    // (uniform 64-bit bases + 32-bit lane offsets: the loads take the scalar-base form and the address
    // arithmetic stays on the scalar unit)
    uint32_t ck0 = 0, ck1 = 0;
    if (c > bclo) {  // (uniform)
        const uint32_t *cp = px.ccp + sed_ck_col_word(R, k, nchunks, c - 1, 0, G * Q);
        uint32_t o0 = px.cko0, o1 = px.cko1;
        asm volatile("" : "+v"(o0), "+v"(o1));  // (else the zero-extended offsets are hoisted as 64-bit pairs)
        ck0 = ld_byte_off(cp, o0);
        ck1 = ld_byte_off(cp, o1);
    }
    // the row above the tile at column J0 - G + x (x = lane, lane + 64, lane + 128 < 132): row checkpoints of
    // forward lane G*Q - 1 (or lane 63 of the stripe above); steps clamped: past SG the columns are beyond m and
    // never read by the walk; columns < 1 are the column-0 border (a CHAIN wave's lanes still hold the
    // previous pair there)
    const bool above = Q >= 1 || k >= 1;  // (uniform) else row 0: the border
    const int kr = Q >= 1 ? k : k - 1, tr = Q >= 1 ? G * Q - 1 : 63, s0r = Q >= 1 ? 64 * c - G - 1 : 64 * c + 63 - G;
    uint32_t rk[NH], wb[NH];
    const uint32_t *rbase = px.rcp + sed_ck_row_word(R, max(kr, 0), ngroups, 0, tr);  // (uniform; read when above)
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int x = lane + 64 * h;
        rk[h] = 0u;
        // (a visit reads the top row and selectors of steps <= sig_end + 1 only: the blocks past it are skipped, a
        // uniform branch; the entry word's reads past sig_end see unused words)
        if ((FULL || 64 * h <= sig_end + 1) && (64 * (h + 1) <= NX || x < NX)) {
            if (above) {
                const uint32_t s = (uint32_t)min(max(s0r + x, 0), SG - 1);
                rk[h] = ld_byte_off(rbase, ((s >> (6 - LR)) * (uint32_t)SED_CK_RW + (s & (uint32_t)(G - 1))) * 4u);
            }
            const int ci = min(max(J0 - (G - 1) + x - 1, 0), m - 1);
            wb[h] = px.pb[ci >> 4];
        }
    }
    const uint32_t a = (wa >> ((ir & 15) * 2)) & 3u;
    const uint32_t clo = (a & 1u) ? prm.costrow[1] : prm.costrow[0];
    const uint32_t chi = (a & 1u) ? prm.costrow[3] : prm.costrow[2];
    const uint32_t cv = (a & 2u) ? chi : clo;
    uint32_t V = SED_KB, tp = SED_KB;  // c = clo: the borders of column 64 clo
    if (c > bclo) {
        V = ck_to_tb(ck0, prm);
        tp = ck_to_tb(ck1, prm);
        if (VHOLD && J0 - band - 1 > m) V = 0u;  // (forward garbage past m: key 0 holds under the recurrence)
    }
    tp += 1u;  // diagonals carry the +1 of the delete candidate they were taken from
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int x = lane + 64 * h;
        if ((FULL || 64 * h <= sig_end + 1) && (64 * (h + 1) <= NX || x < NX)) {
            // (the stripe above's cell at column jb is real where that stripe started left of it: the diagonal of the
            // stripe's first cell, as the forward took it)
            const int tcol = J0 - G + x;
            const bool tin = tcol > jb || (Q == 0 && bclo > bclo_prev && tcol == jb);
            const uint32_t v = (above && tin && s0r + x <= tophi) ? ck_to_tb(rk[h], prm) : SED_KB;
            topb[x] = v + 1u;
            const int col = J0 - (G - 1) + x;  // column of lane 0 at step x
            const int ci = min(max(col - 1, 0), m - 1);
            const uint32_t sv = col <= jb ? SED_SEL_SENT : i32_sel((wb[h] >> ((ci & 15) * 2)) & 3u);
            if constexpr (VHOLD) {  // band b's copy: the sentinel left of its window (x < G - 1 - b)
#pragma unroll
                for (int b = 0; b < G; ++b) selb[b * SELB + 64 + x] = x < G - 1 - b ? SED_SEL_SENT : sv;
            } else {
                selb[64 + x] = sv;
            }
        }
    }
    ck_sync<WAVE>();
    // ---- sweep: lane r at step sigma computes (row rowbase + r + 1, column J0 - (G-1) + sigma - r) ----
    // Whole 16-step words (a branch per step would keep the LDS reads from running ahead), except the
    // word holding the entry step, which stops at it: the lanes' keys are then the entry keys.  The cell above and the diagonal
    // carry the delete candidate's +1 (one v_add_u32_dpp: lane r - 1's key + 1, or topb for lane 0), so
    // the update constant is one less.  Lanes still left of their window (sigma < sig0: lanes
    // ck_active_lanes(sigma) .. 63, a compile-time count) keep their checkpoint through one v_cndmask on a
    // scalar mask; their codes become 3 through hm.  Steps 0 .. G-2 hold every lane and are skipped.
    W[0] = 0u;  // steps 0 .. G-2 are skipped: their bits are OR-ed to 3 from a defined word
    if constexpr (VHOLD) {  // a band's first row: V - V_above + 1 until the band starts
        // (through the asm DPP add: with the builtin, the compiler folded V - dpp(V) into one
        // v_subrev_u32_dpp ... bound_ctrl:1, which returned V_above - V on the device)
        uint32_t zero = 0u;
        asm volatile("" : "+v"(zero));
        const uint32_t vabove = dpp_shr1_add(0u, V, zero);
        one = ((lane & (R - 1)) == 0 && lane > 0) ? V - vabove + 1u : 1u;
    }
#ifdef SED_TB_DEBUG
    vinit = V;
#endif
    uint32_t tprev = dpp_shr1_add(topb[G - 1], V, one);  // diagonal of step G-1 (+1)
    // the top row's reads through one opaque base register and immediate offsets (else every constant address became a
    // VGPR of its own: 28 preloaded at the kernel's start, one more v_mov per two steps of an entry word)
    const uint32_t *topr = topb;
    {
        uint32_t z = 0u;
        asm volatile("" : "+v"(z));
        topr += z;
    }
    const uint32_t *selp = selb + (VHOLD ? band * SELB : 0) + 64 - lane;  // lane r's selector at step sigma
    const int w_end = FULL ? NW - 1 : sig_end >> 4;  // FULL: every word, whole
    auto step = [&](const int sig, uint32_t &wv, const uint32_t topin, const uint32_t selv) {
        if (sig < G - 1) return;  // every lane holds
        const int bs = ck_band_start<R>(sig);  // folds to a constant in the unrolled sweep
        if (VHOLD && bs > 0) one = lane == R * bs ? 1u : one;  // the band starts: its first row's real delete
        const uint32_t topv = dpp_shr1_add(topin, V, one);
        // (selv: steps before the lane's first column read don't-care)
        uint32_t diag = tprev;
        if (bs > 0) diag = lane == R * bs ? tp : diag;
        const uint32_t mm = umin3(V, topv, diag + __builtin_amdgcn_perm(cv, 0xFFFFFFFDu, selv));
        const uint32_t vn = mm & ~3u;
        if constexpr (VHOLD) {
            V = vn;
        } else {
            const int act = ck_active_lanes<R>(sig);  // lanes 0 .. act-1 are inside their window
            V = act >= 64 ? vn : ck_hold(vn, V, act);
        }
        wv = __builtin_amdgcn_alignbit(mm, wv, 2);
        tprev = topv;
    };
    // (the words expand through static_for: a #pragma unroll over 12 words gives up, and the steps' constants with it)
    static_for<0, NW>([&](auto wc) {
        constexpr int w = decltype(wc)::value;
        if (w > w_end) return;  // the path never needs later steps
        if (!FULL && w == w_end) {  // up to the entry step exactly: the lanes then hold the entry keys
            // the word's LDS inputs first (the compiler sinks them into the steps anyway; pinning them ahead of the exits
            // with an asm use measured the same, profiles/r06/ck_wide)
            uint32_t tw[16], sw[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                tw[u] = topr[16 * w + u + 1];
                sw[u] = selp[16 * w + u];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (16 * w + u > sig_end) break;
                step(16 * w + u, W[w], tw[u], sw[u]);
            }
            W[w] >>= 2u * (15u - ((uint32_t)sig_end & 15u));  // step u's code to bits 2u, 2u+1
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) step(16 * w + u, W[w], topr[16 * w + u + 1], selp[16 * w + u]);
        }
        if (w < 4) W[w] |= px.hm[w];
    });
    return V;
}

