// sed_kernels.hip — gfx950 (MI355X / CDNA4) kernels for the weighted
// Wagner–Fischer DP and its canonical traceback.
//
// Reference semantics (plsakr/rna-sequence-diff-patch, StringEditDistance.py):
//   border cells :146-182, recurrence min_cost :92-128 (candidates insert,
//   delete, update; one fp64 add each; first minimal value), canonical path =
//   create_paths(dp)[0] :228-271 (shortest co-optimal path, ties
//   insert < delete < update read from the sink), script ops :274-334.
//
// Work decomposition: one wave64 per sequence pair.  A pair's
// rows are cut into stripes of 64*R rows; lane t of the wave owns R
// consecutive rows and sweeps the columns one step behind lane t-1
// (a systolic anti-diagonal wavefront).  Per step a lane receives the cell
// above its band from lane t-1 through a DPP wave_shr:1 move, so there is no
// barrier in the inner loop.  Lane 0 takes its "above" value (the stripe's top
// row) and every lane its str2 selector from small per-wave LDS rings, read as
// broadcasts; lane 63's bottom row is collected by DPP wave_shl:1 and stored as
// the next stripe's top row (per 64-step chunk in one wave, per 16-step group
// through tagged words between SPLIT workgroups, sed_dev.h).
//
// Integer kernels (the exact fast path).  When every cost is
// an integral positive Python float (or the int 0 of a match), the reference's
// fp64 values are exact integers and the per-cell decision
//    (distance, path length, op)   lexicographically minimal
// is one unsigned v_min3_u32 over packed keys.  Three key formats, all kept in
// an offset space where the insert candidate needs no add and every border is a
// constant (details in sed_i32_keys.h):
//  - ladder keys V = D << 16 + L << 3 + op (per-cell traceback codes): v_perm,
//    v_add, v_min3, v_and_or (clears the op), v_alignbit (packs the 2-bit op)
//    = 5 VALU per cell, plus a delete add on 3 of 16 rows;
//  - distance keys D << 16 - U (U = updates on the path, so at a fixed cell the
//    low half orders by the path length L = i + j - U): v_perm, v_add, v_min3
//    = 3 VALU.  Distance-only batches and the checkpoint forward kernel (CK),
//    whose traceback recomputes tiles in traceback keys (D << 16 | L << 2 | op
//    in offset space) converted from them;
//  - 16-bit packed distance keys, two pairs per word (distance only).
//
// fp64 kernel (the general path): fp64 candidates added exactly as the
// reference does, equality ties, L tie-break on an integer key, and an
// optional int/float typing bit.
//
// Where things live:
//   sed_dev.h       cross-lane moves, min / packed helpers, code-group stores, the SPLIT hand-off's tagged words
//   sed_i32_keys.h  the integer key machinery (i32_step, i32_group, ladders, decode, forward -> traceback keys)
//   sed_ck_tile.h   the checkpoint tile sweep and walk (shared by sed_cktb.hip and sed_ck_codes_kernel)
//   sed_internal.h  the launch structures, SED_LAUNCH and sed_for_R (the runtime's R as a template argument, every launcher)
//   sed_kernels.hip (this file) the integer wave-per-pair forward kernels, in this order: integer stripe / SPLIT /
//                   cutoff, two pairs per wave, CHAIN, self-test; then their launchers
//   sed_tb.hip      the tracebacks over per-cell codes (lane, window, stripe-parallel), sed_ck_codes_kernel, their launchers
//   sed_windows.hip the band and cutoff window kernels, the cutoff filter and their launchers
//   sed_f64.hip     the fp64 wave kernel (whole wave and 16-lane segments), fp64 SPLIT and their launchers
//   sed_cktb.hip    the checkpoint traceback and its launcher, built with its own code-generation options
//   sed_lane.hip    lane-per-pair kernels for short str2
#include <hip/hip_ext.h>
#include <stdlib.h>
#include "sed_i32_keys.h"

// Minimum waves per SIMD the register allocator must leave room for, per R: the budget at which
// the hot loop does not spill (R=16: 96 VGPRs / 5 waves; the 80-VGPR budget of 6 waves spills the
// cost rows and ran 2.5x slower; R=4/8: 72 / 7; R=32: 128 / 4, which still spills: never chosen).
template <int R> struct I32Waves { static constexpr int value = R >= 32 ? 4 : (R == 16 ? 5 : 7); };
#ifndef SED_SPLIT_BWORDS
#define SED_SPLIT_BWORDS 1024  // SPLIT: str2 words staged in LDS (m <= 16384)
#endif
#ifndef SED_CK_WAVES
#define SED_CK_WAVES 5
#endif
#ifndef SED_CK_GUNROLL
#define SED_CK_GUNROLL 2  // groups per iteration of the CK chunk loop
#endif
#ifdef SED_I32_WAVES_PER_EU
#define SED_I32_WAVES(R) SED_I32_WAVES_PER_EU
#else
#define SED_I32_WAVES(R) I32Waves<R>::value
#endif

// SPLIT: the ring of lane 0's top values (one per step) and the hand-off feeder.  Each stripe below the first runs
// as two waves: the compute wave, which never waits on a global load (any such wait with its own stores in flight is
// an s_waitcnt vmcnt(0): the compiler counts mixed reads and writes as out of order, and the store round trip then
// sat in every group), and this feeder.  The feeder polls the stripe above's tagged words 64 columns at a time (sc1,
// past its L1), moves the longest valid prefix into the LDS ring and publishes how many steps are ready (flag[0]);
// the compute wave publishes how many it has consumed (flag[1]), which bounds how far the feeder may run ahead.
// A poisoned word upstream, or no progress for ~2^22 polls, poisons flag[0] (bit 31) with every step ready, so the
// compute wave never waits again and the last stripe reports err.
#define SED_SPLIT_RING 256
template <int G>
__device__ __forceinline__ void split_feed(const uint64_t *__restrict__ bin64, const int m, const int SG,
                                           const uint32_t epoch, uint32_t *ring, uint32_t *flag,
                                           const int lane) {
    uint32_t poison = 0, idle = 0;
    int have = 0;  // steps whose top values are in the ring
    while (have < SG) {
        if (have + 64 > (int)lds_flag_get(flag + 1) + SED_SPLIT_RING) {  // ring full: the compute wave is behind
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        const int t = have + lane, col = t + 1;
        const bool need = t < SG && col <= m;  // columns past m are never stored nor waited for
        const uint64_t w = need ? load_sc1_u64(bin64 + (uint32_t)(col + 64)) : 0ull;
        const bool good = !need || (((uint32_t)(w >> 32) & ~SED_PROG_POISON) == epoch);
        const uint64_t bad = __ballot(!good);
        const int nv = min(bad ? (int)__builtin_ctzll(bad) : 64, SG - have);  // the valid prefix
        if (__any(lane < nv && need && (w >> 63))) poison = SED_PROG_POISON;  // poisoned upstream
        if (nv > 0) {
            if (lane < nv) ring[t & (SED_SPLIT_RING - 1)] = (uint32_t)w;
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the values before the count
            have += nv;
            idle = 0;
        } else if (++idle > (1u << 22)) {  // the stripe above stopped: give up, let the compute wave drain
            poison = SED_PROG_POISON;
            have = SG;
        } else {
            __builtin_amdgcn_s_sleep(1);
        }
        if (lane == 0 && (nv > 0 || poison)) lds_flag_set(flag, (uint32_t)have | poison);
    }
}

// SPLIT = false: one wave per pair walks all of its stripes (batches).
// SPLIT = true : one 128-thread workgroup per stripe (the compute wave and its
//                feeder, split_feed), all stripes of a pair run concurrently,
//                each a few groups behind the stripe above it (single long
//                pairs: config 2, the GUI; hand-off: sed_dev.h).
// CK (not SPLIT): instead of per-cell codes, tb receives checkpoints for the recompute traceback
// (sed_traceback_ck_kernel; layout in sed_internal.h): per stripe, at every chunk end each lane's R row values
// and its top_prev ("column checkpoints", [chunk][R+1][64 lanes]), and every step the bottom row of the lanes
// t = G-1 (mod G) ("row checkpoints", [group][64/G][G steps]) -- ~0.13 B per cell instead of 0.25.  The CK
// kernel runs distance keys (LEN = false, 3 VALU per cell instead of the ladder keys' 5.19): they carry
// (D, L), which is all the checkpoints need; the traceback recomputes the op tie-break.
// The CK kernel (distance keys, no codes) would fit 80 VGPRs (6 waves per SIMD, spills per chunk only) but
// ran slower: 12.45 against 12.11 ms at 5 waves (profiles/r02/ab_ck_waves.txt).
// CUT (distance-only batches under a cutoff, sed_batch_set_cutoff; not TB, LEN, CK or SPLIT): wave w runs pair
// list[w] of the cutoff's pair list (passed in `tasks`, npairs = its length) inside the pair's window band[pair]
// (sed_cut_band_kernel: ub = min(cutoff, diagonal bound)), with the chunk ranges and border rules of the CK forward
// on this kernel's own bottom-row layout (column j at word j + 64); a pair whose window is empty (elo > ehi: the
// length difference alone costs more than the cutoff) runs no stripe and reports +inf.
template <int R, bool TB, bool SPLIT, bool LEN = true, bool CK = false, bool DOT = false, bool CUT = false>
__global__ __launch_bounds__(SPLIT ? 128 : 256) __attribute__((amdgpu_waves_per_eu(CK ? SED_CK_WAVES : SED_I32_WAVES(R))))
void sed_wf_i32_kernel(const sed_pair_desc *__restrict__ pd, int npairs, const int2 *__restrict__ tasks,
                  const uint32_t *__restrict__ seqa, const uint32_t *__restrict__ seqb,
                  uint32_t *__restrict__ tb, uint32_t *__restrict__ bnd, sed_result *__restrict__ res,
                  sed_i32_params prm, const sed_band *__restrict__ band, sed_stripe_wins sw) {
    constexpr int ROWS = 64 * R;
    constexpr int G = Grp<R>::G;
    static_assert(!CK || (R <= 16 && !TB && !LEN), "checkpoints: R <= 16, distance keys");
    static_assert(!(CK && SPLIT) || R == 4, "SPLIT checkpoints (sed_ck_codes_kernel): R = 4");
    static_assert(!DOT || CK, "dot keys: checkpoint batches only");
    static_assert(!CUT || (R <= 16 && !TB && !LEN && !CK && !SPLIT), "cutoff window: distance keys, one wave per pair");
    constexpr bool WIN = (CK && !SPLIT) || CUT;  // the forward runs a window of chunks per stripe
    if constexpr (SPLIT && SED_SPLIT_PRIO > 0) __builtin_amdgcn_s_setprio(SED_SPLIT_PRIO);
    const int lane = threadIdx.x & 63;
    int pair, kfirst = 0;
    if constexpr (SPLIT) {
        const int2 t = tasks[blockIdx.x];
        pair = __builtin_amdgcn_readfirstlane(t.x);
        kfirst = __builtin_amdgcn_readfirstlane(t.y);
    } else {
        pair = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
        if (pair >= npairs) return;
        if constexpr (CUT) pair = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t *>(tasks)[pair]);
    }
    const sed_pair_desc d = pd[pair];
    if (!CUT && d.lane) return;  // short str2: sed_lane.hip (CUT: the list holds wave pairs only)
    const int n = d.n, m = d.m;
    if (n == 0 || m == 0) {
        if (lane == 0) {
            const uint32_t D = (n == 0) ? (uint32_t)m * prm.ins : (uint32_t)n * prm.del;
            res[pair].dist = (double)D;
            res[pair].len = (LEN || CK) ? n + m : -1;  // (as i32_decode: no length without LEN or checkpoints)
            res[pair].is_int = (D == 0);
            res[pair].err = 0;
        }
        return;
    }
    const int nstripes = (n + ROWS - 1) / ROWS;
    const int klast = SPLIT ? kfirst : nstripes - 1;
    const int SG = (m + 63 + G - 1) / G * G;  // steps per stripe, rounded to whole groups
    const int nchunks = (SG + 63) >> 6;
    const uint32_t bstride = (uint32_t)(nchunks + 2) * 64u;  // bottom-row buffer of one stripe (SPLIT: 64-bit words)
    const uint32_t *pa = seqa + d.a_off;
    const uint32_t *pb = seqb + d.b_off;
    // the sink cell (n, m): last stripe, lane (n-1)%ROWS / R, row (n-1)%R, computed at step m-1+lane
    const int wsink = (n - 1) % ROWS;
    const int cap_lane = wsink / R, cap_row = wsink % R;
    uint32_t cap = 0;
    bool ok = true;
    // band pruning (CK, one wave per pair; sed_internal.h: sed_band_chunks): stripe k runs chunks clo .. chi of its
    // schedule, from the border state at column 64 clo, and takes the border constant for the top values the stripe
    // above did not compute (steps past top_hi of the in-place bottom-row buffer, which holds stale words there).
    // Wave-uniform, in scalar registers; an open window (no band) gives 0 .. nchunks - 1 and every top value.
    sed_band bw{SED_BAND_OPEN_LO, SED_BAND_OPEN_HI};
    if constexpr (WIN) {
        if (band) {
            bw.elo = __builtin_amdgcn_readfirstlane(band[pair].elo);
            bw.ehi = __builtin_amdgcn_readfirstlane(band[pair].ehi);
        }
    }
    if constexpr (CUT) {
        if (bw.elo > bw.ehi) {  // no path within the cutoff (uniform)
            if (lane == 0) {
                res[pair].dist = __builtin_huge_val();
                res[pair].len = -1;
                res[pair].is_int = 0;
                res[pair].err = 0;
            }
            return;
        }
    }
    int top_hi = 0x7FFFFFFF, clo_prev = 0;  // (of the stripe above)
    // refined windows: the running upper bound (UB_0 = suf(0), the whole diagonal) and the forward's own error
    uint32_t ub_run = 0, rerr = 0;
    if constexpr (CK && !SPLIT) {
        if (sw.suf) ub_run = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw.suf[(size_t)pair * sw.stride]);
    }
    // per wave: lane 0's top values of the current 64-step chunk, and a ring of str2 selectors by column
    // (column ci at slots ci & 127 and (ci & 127) + 128; the 64 columns before 0 hold the virtual-column
    // sentinel), from which lane t reads column s - t at step s
    __shared__ uint32_t lds_top[SPLIT ? SED_SPLIT_RING / 64 : 4][64];
    __shared__ uint32_t lds_sel[SPLIT ? 1 : 4][256];
    __shared__ uint32_t split_flag[2];
    uint32_t *lch = lds_top[SPLIT ? 0 : (threadIdx.x >> 6)];  // SPLIT: the whole array is the feeder's ring
    uint32_t *ring = lds_sel[SPLIT ? 0 : (threadIdx.x >> 6)];
    // SPLIT: str2's packed words in LDS (m <= 16 * SED_SPLIT_BWORDS), so the chunk loop issues no global load of its
    // own: a wait for one with the group's stores in flight is a vmcnt(0), i.e. a store round trip per chunk.  (The
    // same per wave in the one-wave-per-pair kernels made the checkpoint kernel spill.)
    constexpr int BW = SPLIT ? SED_SPLIT_BWORDS : 1;
    __shared__ uint32_t lds_b[BW];
    const int bwords = (m + 15) >> 4;
    const bool bl = SPLIT && bwords <= BW;  // (uniform)
    if (bl && threadIdx.x < 64) {
        for (int x = lane; x < bwords; x += 64) lds_b[x] = pb[x];
    }
    if constexpr (SPLIT) {
        if (threadIdx.x < 2) split_flag[threadIdx.x] = 0u;
        __syncthreads();
    }

    for (int k = kfirst; k <= klast; ++k) {
        // in-place single buffer per pair when one wave does all stripes; one buffer per stripe otherwise
        const uint32_t *bnd_in = bnd + d.bnd_off;
        uint32_t *bnd_out = bnd + d.bnd_off;
        const uint64_t *bin64 = reinterpret_cast<const uint64_t *>(bnd + d.bnd_off) + (uint32_t)(k - 1) * bstride;
        uint64_t *bout64 = reinterpret_cast<uint64_t *>(bnd + d.bnd_off) + (uint32_t)k * bstride;
        if constexpr (SPLIT) {
            if (threadIdx.x >= 64) {  // the feeder wave
                if (k > 0) split_feed<G>(bin64, m, SG, prm.epoch, lch, split_flag, lane);
                return;
            }
        }
        const int row0 = k * ROWS + lane * R;  // 0-based str1 index of this lane's first row
        int clo = 0, chi = nchunks - 1;
        if constexpr (WIN) sed_band_chunks(n, m, ROWS, nchunks, bw, k, &clo, &chi);
        if constexpr (CK && !SPLIT) {
            // refined windows (sed_internal.h: sed_refine_cell): the stripe above left row r0 = k ROWS complete in the
            // bottom-row buffer (column j at word j + 62, columns 64 clo_prev + 1 .. its last, its stores waited for at
            // its end), every value a real path's cost.  The wave scans it 64 columns at a time, takes the extremes
            // across its lanes and keeps the chunk range uniform; the chunk loops below do not change.
            if (sw.suf && k > 0) {
                const int r0 = k * ROWS, chi_prev = top_hi >> 6;
                const int j0 = 64 * clo_prev + 1, j1 = min(m, 64 * chi_prev + 1);
                const uint32_t *row = bnd + d.bnd_off + 62;
                const uint32_t suf = sw.suf[(size_t)pair * sw.stride + k];
                if (suf != SED_REFINE_NO_SUF && r0 >= j0 && r0 <= j1) {  // (uniform) the diagonal cell and the rest of its path
                    const uint32_t dd = ck_key_dist<DOT>(load_sc1(row + r0), r0, r0, prm) + suf;
                    ub_run = min(ub_run, (uint32_t)__builtin_amdgcn_readfirstlane((int)dd));
                }
                int32_t lo = SED_REFINE_LO_INIT, hi = SED_REFINE_HI_INIT;
                for (int jb = j0; jb <= j1; jb += 64) {
                    const int j = jb + lane;
                    if (j <= j1)
                        sed_refine_cell(n, m, prm.ins, prm.del, r0, j, ck_key_dist<DOT>(load_sc1(row + j), r0, j, prm), ub_run,
                                        &lo, &hi);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    lo = min(lo, __shfl_xor(lo, o));
                    hi = max(hi, __shfl_xor(hi, o));
                }
                lo = __builtin_amdgcn_readfirstlane(lo);
                hi = __builtin_amdgcn_readfirstlane(hi);
                if (!sed_refine_chunks(n, m, ROWS, nchunks, prm.ins, prm.del, ub_run, lo, hi, k, clo_prev, chi_prev, &clo, &chi))
                    rerr = SED_ERR_FWD_BAND;
                clo = __builtin_amdgcn_readfirstlane(clo);
                chi = __builtin_amdgcn_readfirstlane(chi);
            }
            if (sw.win && lane == 0) sw.win[(size_t)pair * sw.stride + k] = make_int2(clo, chi);
        }
        uint32_t cv[R], V[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ri = row0 + r;
            const uint32_t a = (pa[ri >> 4] >> ((ri & 15) * 2)) & 3u;
            if constexpr (DOT) cv[r] = a == 0 ? prm.dotrow[0] : a == 1 ? prm.dotrow[1] : a == 2 ? prm.dotrow[2] : prm.dotrow[3];
            else cv[r] = a == 0 ? prm.costrow[0] : a == 1 ? prm.costrow[1] : a == 2 ? prm.costrow[2] : prm.costrow[3];
        }
        uint32_t top_prev;
        i32_reset<R, LEN, DOT>(V, top_prev);
        if constexpr (WIN) {
            // a stripe that starts at column 64 clo + 1 > 1: the diagonal of lane 0's first cell is the cell (r0, 64 clo)
            // of the stripe above, which lies on the window's edge when 64 clo = r0 + elo, so it is the real value
            // (its step's word of the bottom-row buffer; every other lane's first diagonal is left of the window).
            // Only where the stripe above computed that column (clo > its own clo): where both start at the same
            // chunk the cell is left of the window (e < elo) and the reset's border constant stands.  (The word
            // there is a virtual-step store of the stripe above, which holds the same constant: a lane's state
            // stays at the border through its virtual columns, i32_sent.  The guard keeps this load off that.)
            if (k > 0 && clo > clo_prev) {
                const int idx = 64 * clo + 62;  // (its word: the step, or column + 64 in the CUT layout)
                const uint32_t v = load_sc1(bnd + d.bnd_off + (uint32_t)(idx + (CK ? 0 : 2)));
                top_prev = (lane == 0 && idx <= top_hi) ? v : top_prev;
            }
        }
        // column-0 state for every lane; virtual columns until the lane's first real one (sed_i32_keys.h: ramp for free)
        uint32_t bottom = V[R - 1], selv = i32_sent<LEN, DOT>(), outc = 0;
        uint32_t W[4] = {0, 0, 0, 0};

        // CK: the previous stripe's lane 63 stored its bottom row contiguously by step into the pair's
        // bottom-row buffer (column j at step j + 62, in place: this stripe writes step s while it reads
        // steps >= s + 64; past SG the columns are beyond m and never read)
        auto load_top = [&](int c) -> uint32_t {
            const int j = 64 * c + lane + 1;
            if (k == 0) return i32_row0<LEN, DOT>();
            if constexpr (CK) {  // (past the stripe above's last chunk: the border, as the columns it never computed)
                const uint32_t v = load_sc1(bnd + d.bnd_off + (uint32_t)(j + 62));
                return (SPLIT || j + 62 <= top_hi) ? v : i32_row0<LEN, DOT>();
            }
            if constexpr (CUT) {  // (as above, in this layout)
                const uint32_t v = load_sc1(bnd_in + j + 64);
                return j + 62 <= top_hi ? v : i32_row0<LEN, DOT>();
            }
            return load_sc1(bnd_in + j + 64);
        };
        auto load_sel = [&](int c) -> uint32_t {
            const int ci = 64 * c + lane;
            const uint32_t wb = bl ? lds_b[min(ci >> 4, bwords - 1)] : pb[ci >> 4];  // (past m: never read)
            const uint32_t b = (wb >> ((ci & 15) * 2)) & 3u;
            if constexpr (DOT) return b == 0 ? prm.dotcol[0] : b == 1 ? prm.dotcol[1] : b == 2 ? prm.dotcol[2] : prm.dotcol[3];
            return i32_sel(b);
        };
        uint32_t tch = (SPLIT && k > 0) ? 0u : load_top(clo), sch = load_sel(clo);
        if constexpr (SPLIT) {  // stripe 0's constant row in the whole ring; the feeder fills the others'
            if (k == 0) {
#pragma unroll
                for (int x = 0; x < SED_SPLIT_RING; x += 64) lch[x + lane] = tch;
            }
        } else {
            lch[lane] = tch;
        }
        {  // columns 64 clo .. 64 clo + 63 at their slots, the 64 columns before them the sentinel
            const int h0 = (64 * clo) & 64;
            ring[h0 + lane] = ring[h0 + lane + 128] = sch;
            ring[(h0 ^ 64) + lane] = ring[(h0 ^ 64) + lane + 128] = i32_sent<LEN, DOT>();
        }
        uint32_t *tbk = tb + d.tb_off + (uint64_t)k * (uint64_t)(SG / G) * 256u;
        // CK: column checkpoints of stripe k at ccb[(chunk * (R+1) + v) * 64 + lane], row checkpoints at
        // rcb[group * 64 + (lane / G) * G + step % G] (sed_ck_*_word, the layout sed_traceback_ck_kernel reads)
        // (SPLIT: the checkpoints follow the pair's per-cell code region, which sed_ck_codes_kernel fills from them)
        const uint64_t ckoff = (SPLIT && CK) ? (uint64_t)nstripes * (uint64_t)(SG / G) * 256u : 0u;
        uint32_t *ccb = tb + d.tb_off + ckoff + sed_ck_col_word(R, k, nchunks, 0, 0, 0);
        uint32_t *rcb = tb + d.tb_off + ckoff + sed_ck_col_words(R, nstripes, nchunks) + (uint64_t)k * (uint64_t)(SG / G) * SED_CK_RW;
        uint32_t rcv[G];
        const bool last = (k == nstripes - 1);
        const int cap_step = last ? m - 1 + cap_lane : -1;
        // CK: a chunk is 64/G groups (unrolled by 2) and always whole: the last chunk's steps past SG compute
        // columns beyond m that nothing reads, and only their stores are skipped.  The chunk holding the sink
        // runs the rolled loop below, so the others have no merge point: a CAP/plain choice per group made the
        // register allocator move the whole row state every group (3.30 -> 3.11 VALU per cell).  The per-cell-code
        // kernels keep the rolled loop for every chunk: split the same way, their hot loop spills.  (Fully
        // unrolled chunks take the compiler > 15 min.)
        const int c_cap = last ? cap_step >> 6 : -1;
        int s = 64 * clo;
        int ready = 0;  // SPLIT: steps the feeder has published as ready (last read)
        // CK (not SPLIT): the chunks before the sink's run the unrolled group loop, the sink's chunk and any after it the
        // rolled one, as two loops: one loop choosing per chunk merged the paths, and the register allocator moved the
        // row state in and out of the unrolled loop's registers every chunk (24 VALU per 2112)
        auto chunk = [&](auto fast_tag, const int c) {
            constexpr bool FASTC = decltype(fast_tag)::value;
            uint32_t tnx = 0, snx = 0;
            if (c < chi) {
                if (!SPLIT) tnx = load_top(c + 1);
                snx = load_sel(c + 1);
            }
            const uint32_t *lsel = ring + ((64 * c - lane) & 127);  // this lane's column at the chunk's first step
            auto stores = [&](const int s0) {
                if constexpr (TB) {
                    uint32_t *gp = tbk + (uint64_t)(s0 / G) * 256u;  // wave-uniform base, per-lane 16-byte offset
                    store_tb(gp + lane * 4, W);
                }
                if constexpr (CK) {
                    constexpr int GH = SED_CK_TILE / R;  // forward lanes per traceback tile
                    if ((lane & (GH - 1)) == GH - 1)
                        store_words<G>(rcb + (uint64_t)(s0 / G) * SED_CK_RW + (uint32_t)(lane / GH) * G, rcv);
                    if (!SPLIT && lane == 63 && !last) store_words<G>(bnd + d.bnd_off + (uint32_t)s0, rcv);  // next stripe's top row
                }
            };
            if constexpr (FASTC) {
                // (lch is the first capture this lambda names: the closure's members follow the order of first use, and
                // with another order every variant of the kernel, the rolled ones too, allocates its registers differently)
                const uint32_t *ltop = lch;
#pragma unroll SED_CK_GUNROLL
                for (int g = 0; g < 64 / G; ++g) {
                    const int s0 = 64 * c + g * G;  // (s0 & 63 folds to g * G)
                    i32_group<R, TB, LEN, false, CK, DOT, !CK>(V, cv, top_prev, bottom, selv, ltop, lsel + g * G, outc, W, s0,
                                                               lane, cap_step, cap_lane, cap_row, cap, rcv);
                    if (s0 < SG) stores(s0);
                }
                s = 64 * (c + 1);  // lane 63's bottom cells of the whole chunk are in outc (!CK)
            } else {
                for (int g = 0; g < 64 / G && s < SG; ++g, s += G, lsel += G) {
                    const uint32_t *ltop = lch;
                    if constexpr (SPLIT) {
                        ltop = lch + (s & (SED_SPLIT_RING - 64));
                        // the feeder has this group's top values in the ring (LDS only: no vmcnt).  The ready count
                        // is re-read only when the groups it covered are used up (the feeder publishes up to 64 steps
                        // at a time), so most groups start without an LDS round trip.
                        if (k > 0 && ready < s + G) {
                            uint32_t f = lds_flag_get(split_flag), spins = 0;
                            while (ok && (int)(f & ~SED_PROG_POISON) < s + G) {
                                if (++spins > (1u << 24)) ok = false;
                                __builtin_amdgcn_s_sleep(1);
                                f = lds_flag_get(split_flag);
                            }
                            if (f & SED_PROG_POISON) ok = false;
                            ready = (int)(f & ~SED_PROG_POISON);
                            asm volatile("" ::: "memory");
                        }
                    }
                    const bool capg = cap_step >= s && cap_step < s + G;
                    if (capg)
                        i32_group<R, TB, LEN, true, CK, DOT, !CK || SPLIT>(V, cv, top_prev, bottom, selv, ltop, lsel, outc, W,
                                                                          s, lane, cap_step, cap_lane, cap_row, cap, rcv);
                    else
                        i32_group<R, TB, LEN, false, CK, DOT, !CK || SPLIT>(V, cv, top_prev, bottom, selv, ltop, lsel, outc, W,
                                                                           s, lane, cap_step, cap_lane, cap_row, cap, rcv);
                    stores(s);
                    if constexpr (SPLIT) {
                        // lanes 64-G+u hold lane 63's bottom cell of step s+u, column s+u-62 (word col + 64)
                        if (!last && lane >= 64 - G)
                            store_tagged(bout64 + (uint32_t)(s + lane - (64 - G) - 62 + 64),
                                         prm.epoch | (ok ? 0u : SED_PROG_POISON), outc);
                        if (k > 0) {  // this group's ring slots are free again
                            asm volatile("" ::: "memory");
                            if (lane == 0) lds_flag_set(split_flag + 1, (uint32_t)(s + G));
                        }
                    }
                }
            }
            if constexpr (CK) {  // column checkpoint: state after the chunk's last step
                uint32_t *cp = ccb + (uint64_t)c * (uint64_t)(R + 1) * 64u + lane;
#pragma unroll
                for (int r = 0; r < R; ++r) cp[r * 64] = V[r];
                cp[R * 64] = top_prev;
            }
            // lane i holds lane 63's bottom cell of step s-64+i, i.e. column s-126+i at bnd index col+64
            if (!CK && !SPLIT && !last) bnd_out[s - 62 + lane] = outc;
            tch = tnx;
            sch = snx;
            if (!SPLIT) lch[lane] = tch;  // after the chunk's last LDS read (in order)
            const uint32_t slot = (uint32_t)(64 * (c + 1) + lane) & 127u;  // replaces column 64(c-1) + lane
            ring[slot] = ring[slot + 128] = sch;
        };
        int cfast = 0;
        if constexpr (CK && !SPLIT) {
            cfast = c_cap >= 0 ? c_cap : chi + 1;  // (clo <= c_cap <= chi on the last stripe)
            for (int c = clo; c < cfast; ++c) chunk(BoolTag<true>{}, c);
        }
        for (int c = cfast > clo ? cfast : clo; c <= chi; ++c) chunk(BoolTag<false>{}, c);
        if (!last) __builtin_amdgcn_s_waitcnt(0);  // own bottom-row stores done before the next stripe reads them
        top_hi = 64 * chi + 63;  // the last step whose bottom row this stripe stored
        clo_prev = clo;
    }
    if (klast == nstripes - 1 && lane == cap_lane) {
        const int2 dl = i32_decode<R, LEN, CK, DOT>(cap, n, m, prm);
        res[pair].dist = (double)dl.x;
        res[pair].len = dl.y;
        res[pair].is_int = (dl.x == 0);
        res[pair].err = ok ? rerr : SED_ERR_SPLIT_TIMEOUT;  // SPLIT: a timed-out wait anywhere up the stripe chain poisons the pair
    }
}

// ---------------------------------------------------------------------------
// Distance only, two pairs per wave (SED_NO_LEN batches, pairs of equal n): pair P in the low
// 16 bits of every cell word, pair Q in the high 16 bits.  Each half is a 16-bit offset key
// W = D - i*delete - j*insert + 0xFFFF (the host checks i*delete + j*insert <= 0xFFFF over the
// computed block, so no half wraps), with insert candidate W_left, delete candidate W_up and
// update candidate W_diag + (cost - delete - insert), a 16-bit constant 0xFFxx since the host
// packs only when every substitution is cheaper than delete + insert.  Packed 16-bit ops do two
// cells at once: perm + v_pk_add_u16 + 2 v_pk_min_u16 = 4 VALU / 2 cells.  The rest is the stripe
// kernel's schedule (virtual-column ramp, lane-0 LDS chunk, in-place bottom rows in P's buffer,
// which the host makes the pair with the larger m); both pairs have the same n, so they share
// stripes and rows, and the wave runs max(m) columns, the shorter pair's extra columns being
// don't-care.  Each pair's sink is captured at its own step.
// ---------------------------------------------------------------------------
// 16-bit offset key of the sink back to D: D = W - 0xFFFF + n*delete + m*insert (mod 2^16)
__device__ __forceinline__ uint32_t x2_decode(uint32_t half, int n, int m, const sed_i32_params &prm) {
    return (half + 1u + (uint32_t)n * prm.del + (uint32_t)m * prm.ins) & 0xFFFFu;
}

template <int R, bool CAP>
__device__ __forceinline__ void x2_group(uint32_t (&V)[R], const uint32_t (&cP)[R], const uint32_t (&cQ)[R],
                                         uint32_t &top_prev, uint32_t &bottom, uint32_t &selv,
                                         const uint2 *__restrict__ lch, uint32_t &outc, const int s0, const int lane,
                                         const int capP_step, const int capQ_step, const int cap_lane,
                                         const int cap_row, uint32_t &capP, uint32_t &capQ) {
    constexpr int G = Grp<R>::G;
    uint2 tv[G];
    const uint2 *lp = lch + (s0 & 63);
#pragma unroll
    for (int u = 0; u < G; ++u) tv[u] = lp[u];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int s = s0 + u;
        const uint32_t topv = dpp_shr1(tv[u].x, bottom);
        selv = dpp_shr1(tv[u].y, selv);
        uint32_t up = topv, diag = top_prev;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t left = V[r];
            // the row above (up) enters last: one dependent op per row on the column's chain
            const uint32_t mm = pk_min(pk_min(left, pk_add(diag, __builtin_amdgcn_perm(cQ[r], cP[r], selv))), up);
            diag = left;
            up = mm;
            V[r] = mm;
        }
        top_prev = topv;
        bottom = V[R - 1];
        outc = dpp_shl1(bottom, outc);
        if constexpr (CAP) {
            const bool hP = (s == capP_step) && (lane == cap_lane), hQ = (s == capQ_step) && (lane == cap_lane);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                capP = (hP && r == cap_row) ? V[r] : capP;
                capQ = (hQ && r == cap_row) ? V[r] : capQ;
            }
        }
    }
}

// occupancy targets with room for both pairs' cost rows (2R) next to the packed row values (R)
template <int R> struct X2Waves { static constexpr int value = R >= 32 ? 3 : (R == 16 ? 5 : (R == 8 ? 7 : 8)); };
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(X2Waves<R>::value))) void
sed_wf_i32x2_kernel(const sed_pair_desc *__restrict__ pd, const int32_t *__restrict__ list, int nwaves,
                    const uint32_t *__restrict__ seqa, const uint32_t *__restrict__ seqb,
                    uint32_t *__restrict__ bnd, sed_result *__restrict__ res, sed_i32_params prm) {
    constexpr int ROWS = 64 * R;
    constexpr int G = Grp<R>::G;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nwaves) return;
    const int P = __builtin_amdgcn_readfirstlane(list[2 * w]), Q = __builtin_amdgcn_readfirstlane(list[2 * w + 1]);
    const sed_pair_desc dP = pd[P], dQ = pd[Q];
    const int n = dP.n, m = dP.m, mQ = dQ.m;  // host: dQ.n == n, 1 <= mQ <= m
    const int nstripes = (n + ROWS - 1) / ROWS;
    const int SG = (m + 63 + G - 1) / G * G;
    const int nchunks = (SG + 63) >> 6;
    const uint32_t *paP = seqa + dP.a_off, *paQ = seqa + dQ.a_off;
    const uint32_t *pbP = seqb + dP.b_off, *pbQ = seqb + dQ.b_off;
    const int wsink = (n - 1) % ROWS;
    const int cap_lane = wsink / R, cap_row = wsink % R;
    uint32_t capP = 0, capQ = 0;
    __shared__ uint2 lds_chunk[4][64];
    uint2 *lch = lds_chunk[threadIdx.x >> 6];
    uint32_t *bnd_io = bnd + dP.bnd_off;  // in place, as in the stripe kernel

    for (int k = 0; k < nstripes; ++k) {
        const int row0 = k * ROWS + lane * R;
        uint32_t cP[R], cQ[R], V[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ri = row0 + r;
            const uint32_t aP = (paP[ri >> 4] >> ((ri & 15) * 2)) & 3u, aQ = (paQ[ri >> 4] >> ((ri & 15) * 2)) & 3u;
            cP[r] = aP == 0 ? prm.costrow16[0] : aP == 1 ? prm.costrow16[1] : aP == 2 ? prm.costrow16[2] : prm.costrow16[3];
            cQ[r] = aQ == 0 ? prm.costrow16[0] : aQ == 1 ? prm.costrow16[1] : aQ == 2 ? prm.costrow16[2] : prm.costrow16[3];
        }
        uint32_t top_prev = 0xFFFFFFFFu;  // column 0 and row 0 are the offset key 0xFFFF in both halves
#pragma unroll
        for (int r = 0; r < R; ++r) V[r] = 0xFFFFFFFFu;
        uint32_t bottom = V[R - 1], selv = SED_SEL_SENT, outc = 0;
        auto load_top = [&](int c) -> uint32_t {
            const int j = 64 * c + lane + 1;
            if (k == 0) return 0xFFFFFFFFu;
            return load_sc1(bnd_io + j + 64);
        };
        auto load_sel = [&](int c) -> uint32_t {
            const int ci = 64 * c + lane;
            const uint32_t bp = (pbP[ci >> 4] >> ((ci & 15) * 2)) & 3u;
            const uint32_t bq = ci < mQ ? (pbQ[ci >> 4] >> ((ci & 15) * 2)) & 3u : 0u;  // Q may be far shorter
            return 0x0D000D00u | bp | ((4u + bq) << 16);  // byte0 <- cP byte bP, byte2 <- cQ byte bQ, 1 and 3 <- 0xFF
        };
        uint32_t tch = load_top(0), sch = load_sel(0);
        lch[lane] = make_uint2(tch, sch);
        const bool last = (k == nstripes - 1);
        const int capP_step = last ? m - 1 + cap_lane : -1, capQ_step = last ? mQ - 1 + cap_lane : -1;
        int s = 0;
        for (int c = 0; c < nchunks; ++c) {
            uint32_t tnx = 0, snx = 0;
            if (c + 1 < nchunks) { tnx = load_top(c + 1); snx = load_sel(c + 1); }
            for (int g = 0; g < 64 / G && s < SG; ++g, s += G) {
                const bool capg = (capP_step >= s && capP_step < s + G) || (capQ_step >= s && capQ_step < s + G);
                if (capg)
                    x2_group<R, true>(V, cP, cQ, top_prev, bottom, selv, lch, outc, s, lane, capP_step, capQ_step,
                                      cap_lane, cap_row, capP, capQ);
                else
                    x2_group<R, false>(V, cP, cQ, top_prev, bottom, selv, lch, outc, s, lane, capP_step, capQ_step,
                                       cap_lane, cap_row, capP, capQ);
            }
            if (!last) bnd_io[s - 62 + lane] = outc;
            lch[lane] = make_uint2(tnx, snx);
        }
        if (!last) __builtin_amdgcn_s_waitcnt(0);
    }
    if (lane == cap_lane) {
        sed_result r;
        r.len = -1;
        r.err = 0;
        r.seq = 0;
        const uint32_t DP = x2_decode(capP & 0xFFFFu, n, m, prm), DQ = x2_decode(capQ >> 16, n, mQ, prm);
        r.dist = (double)DP;
        r.is_int = (DP == 0);
        res[P] = r;
        r.dist = (double)DQ;
        r.is_int = (DQ == 0);
        res[Q] = r;
    }
}

// ---------------------------------------------------------------------------
// CHAIN mode (integer keys, single-stripe pairs: n <= 64R).  One wave runs a chain of pairs
// back to back so that a pair's 63-step wavefront ramp overlaps the previous pair's drain.
// Pair q of the chain owns global steps [T_q, T_q + S_q) for lane 0, S_q = m_q rounded up to
// 64 (whole LDS chunks); lane t runs it at [T_q + t, T_q + S_q + t).  Lane t therefore
// switches pairs right after global step T_q + t - 1: its V / cost rows / diagonal are set
// to the new pair's column-0 state with per-lane selects (rows are the same for every pair
// of the chain: row0 = 64R * 0 + t*R, so the column-0 borders are per-lane constants).
// The cell above a lane's band keeps arriving by DPP from lane t-1, which switched one step
// earlier, and the str2 selectors flow from lane 0 as in the stripe kernel.  The first pair
// starts with the virtual-column ramp.  Per-pair traceback layout, results and captures are
// exactly the stripe kernel's (one stripe), so the traceback kernel is shared.
// ---------------------------------------------------------------------------
struct chain_pair_state {
    int pair, n, m, T, S, end;         // end: first global step after its last real column (T + m + 63)
    int cap_step, cap_lane, cap_row;   // the sink cell (n, m)
    uint64_t tb_off;
    int sg;                            // traceback groups allocated per stripe
    int nchunks;                       // CK: 64-step chunks of the pair's stripe (column checkpoints)
    const uint32_t *pb;                // str2 codes
};

template <int R>
__device__ __forceinline__ chain_pair_state chain_load(const sed_pair_desc *__restrict__ pd,
                                                       const uint32_t *__restrict__ seqb, int pair, int T) {
    constexpr int G = Grp<R>::G;
    const sed_pair_desc d = pd[pair];
    chain_pair_state c;
    c.pair = pair;
    c.n = d.n;
    c.m = d.m;
    c.T = T;
    c.S = (d.m + 63) & ~63;
    c.end = T + d.m + 63;
    const int wsink = d.n - 1;
    c.cap_lane = wsink / R;
    c.cap_row = wsink % R;
    c.cap_step = T + d.m - 1 + c.cap_lane;
    c.tb_off = d.tb_off;
    c.sg = (d.m + 63 + G - 1) / G;
    c.nchunks = (c.sg * G + 63) >> 6;
    c.pb = seqb + d.b_off;
    return c;
}

// One group of G steps.  SW: lanes switch from the previous pair to the pair starting at
// `Tcur` after the step at which lane == s + 1 - Tcur.  GEN (rare groups: sink captures of the
// previous (A) and current (B) pair, and any switch in those groups) additionally captures.
// Lane 0's top value is row 0 (single-stripe pairs); every lane reads its str2 selector from the wave's
// selector ring by global column s - t (lsel: this lane's column at the group's first step), which always
// belongs to the pair the lane is working on: lane t is on the pair starting at T exactly when s - t >= T.
template <int R, bool TB, bool LEN, bool SW, bool GEN, bool CK, int LDOT = 0>
__device__ __forceinline__ void i32_chain_group(uint32_t (&V)[R], uint32_t (&cv)[R], const uint32_t (&cvn)[R],
                                                const uint32_t (&Vb)[R], const uint32_t tpb, uint32_t &top_prev,
                                                uint32_t &bottom, uint32_t &selv, const uint32_t *__restrict__ lsel,
                                                uint32_t &outc, uint32_t (&W)[4], const int s0, const int lane,
                                                const int Tcur, const int csA, const int clA, const int crA,
                                                uint32_t &capA, const int csB, const int clB, const int crB,
                                                uint32_t &capB, uint32_t (&rcv)[Grp<R>::G], const uint32_t jv) {
    constexpr int G = Grp<R>::G;
    uint2 tv[G];
#pragma unroll
    for (int u = 0; u < G; ++u) tv[u] = make_uint2(i32_row0<LEN>(), lsel[u]);
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int s = s0 + u;
        i32_step<R, TB, LEN, false, true, true, false, LDOT>(V, cv, top_prev, bottom, selv, tv[u], outc, W, u, jv);
        if constexpr (CK) rcv[u] = V[R - 1];  // the band's bottom row (row checkpoints), before any switch
        if constexpr (GEN) {
            const bool hA = (s == csA) && (lane == clA), hB = (s == csB) && (lane == clB);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                capA = (hA && r == crA) ? V[r] : capA;
                capB = (hB && r == crB) ? V[r] : capB;
            }
        }
        if constexpr (SW || GEN) {
            const bool sw = (lane == s + 1 - Tcur);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                V[r] = sw ? Vb[r] : V[r];
                cv[r] = sw ? cvn[r] : cv[r];
            }
            top_prev = sw ? tpb : top_prev;
        }
    }
}

template <int R, bool TB, bool LEN, bool CK, int LDOT = 0>
__device__ __forceinline__ void chain_store_result(sed_result *__restrict__ res, int pair, uint32_t cap, int n,
                                                   int m, int seq, const sed_i32_params &prm) {
    const int2 dl = i32_decode<R, LEN, CK, false, LDOT>(cap, n, m, prm);
    res[pair].dist = (double)dl.x;
    res[pair].len = dl.y;
    res[pair].is_int = (dl.x == 0);
    res[pair].err = 0;
    res[pair].seq = (uint16_t)min(seq, 65535);  // the pair's ordinal in its wave (dynamic-CHAIN diagnostics)
}

// the chain kernel also holds the next pair's cost rows and the column-0 constants
#ifndef SED_CHAIN_WAVES
#define SED_CHAIN_WAVES 5
#endif
template <int R> struct ChainWaves { static constexpr int value = R >= 16 ? 4 : SED_CHAIN_WAVES; };

// CK: distance keys, and checkpoints instead of codes (the stripe kernel's layout, one stripe per pair).  At every
// chunk end all lanes are on the pair lane 0 is on (a lane switches at most 63 steps after lane 0), so the column
// checkpoints go to that pair; a row-checkpoint group of a switch window goes to both pairs, like the codes.
template <int R, bool TB, bool LEN, bool CK = false, int LDOT = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ChainWaves<R>::value))) void
sed_wf_i32_chain_kernel(const sed_pair_desc *__restrict__ pd, const int32_t *__restrict__ chain_pairs,
                        const int32_t *__restrict__ chain_off, int nchains, uint32_t *__restrict__ counter,
                        uint32_t cbase, int nlist, const uint32_t *__restrict__ seqa, const uint32_t *__restrict__ seqb,
                        uint32_t *__restrict__ tb, sed_result *__restrict__ res, sed_i32_params prm) {
    constexpr int G = Grp<R>::G;
    static_assert(!CK || (!TB && !LEN), "checkpoints: distance keys, no codes");
    const int lane = threadIdx.x & 63;
    const int chain = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (chain >= nchains) return;
    // Static chains: list entries [chain_off[c], chain_off[c+1]).  Dynamic (counter != null):
    // persistent waves take the next list entry from a device counter whenever lane 0 reaches
    // the end of a pair, so every wave stays busy until the list is exhausted.  A run takes exactly
    // nlist + nchains values (every wave ends with one failed grab), so the counter is never reset:
    // this run's values start at cbase (no fill kernel per run).
    auto grab = [&]() -> int {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(counter, 1u) - cbase;
        return (int)__builtin_amdgcn_readfirstlane(v);
    };
    int c0, c1;
    if (counter) {
        c0 = grab();
        c1 = nlist;
        if (c0 >= nlist) return;
    } else {
        c0 = chain_off[chain];
        c1 = chain_off[chain + 1];
    }
    // per wave: str2 selectors by global column (column g at slots g & 127 and (g & 127) + 128; the 64 columns
    // before the chain's first pair hold the virtual-column sentinel)
    __shared__ uint32_t lds_sel[4][256];
    uint32_t *ring = lds_sel[threadIdx.x >> 6];
    const int row0 = lane * R;

    // per-lane constants: column-0 state of this lane's rows (the same for every pair)
    uint32_t Vb[R], tpb;
    i32_reset<R, LEN, false, LDOT == 2>(Vb, tpb);
    uint32_t jv = (uint32_t)(LadderW<R>::rung(1) - LadderW<R>::rung(0) + 1);  // (LDOT = 2: the DPP move's add, a VGPR)
    asm volatile("" : "+v"(jv));
    auto rows_of = [&](int pair, uint32_t (&out)[R]) {
        const uint32_t *pa = seqa + pd[pair].a_off;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ri = row0 + r;
            const uint32_t a = (pa[ri >> 4] >> ((ri & 15) * 2)) & 3u;
            if constexpr (LDOT) out[r] = a == 0 ? prm.ladrow[0] : a == 1 ? prm.ladrow[1] : a == 2 ? prm.ladrow[2] : prm.ladrow[3];
            else out[r] = a == 0 ? prm.costrow[0] : a == 1 ? prm.costrow[1] : a == 2 ? prm.costrow[2] : prm.costrow[3];
        }
    };
    auto chunk_of = [&](const chain_pair_state &c, int cl) -> uint2 {  // lane 0's inputs, local chunk cl
        const int j = 64 * cl + lane;
        const uint32_t b = (c.pb[j >> 4] >> ((j & 15) * 2)) & 3u;
        if constexpr (LDOT)
            return make_uint2(i32_row0<LEN>(), b == 0 ? prm.ladcol[0] : b == 1 ? prm.ladcol[1] : b == 2 ? prm.ladcol[2] : prm.ladcol[3]);
        return make_uint2(i32_row0<LEN>(), i32_sel(b));  // row 0, str2 selector
    };
    // ladder dot keys: the host's column vector {s, 0, 0, 0} adds s*x in [8, 490] (above any jump, and the border
    // SED_KB3 + c(i) plus it stays below 2^32)
    const uint32_t sent = LDOT ? prm.ladsent : i32_sent<LEN>();

    chain_pair_state cur = chain_load<R>(pd, seqb, chain_pairs[c0], 0), prv = cur;
    bool have_cur = true, have_prv = false;
    int q = c0;
    int ord = 0, ord_prv = 0;  // ordinals of cur and prv among this wave's pairs
    uint32_t cv[R], cvn[R], V[R];
    rows_of(cur.pair, cv);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        V[r] = Vb[r];
        cvn[r] = cv[r];
    }
    uint32_t top_prev = tpb, bottom = V[R - 1], selv = sent, outc = 0, capA = 0, capB = 0;
    uint32_t W[4] = {0, 0, 0, 0};
    uint32_t rcv[G];
    ring[lane] = ring[lane + 128] = chunk_of(cur, 0).y;
    ring[lane + 64] = ring[lane + 192] = sent;

    for (int s0 = 0;; s0 += 64) {
        // prefetch the next chunk's lane-0 inputs (this pair's next chunk, or the next pair's first)
        uint2 nx = make_uint2(0, 0);
        chain_pair_state nxt = cur;
        bool have_nxt = false;
        if (have_cur && s0 + 64 < cur.T + cur.S) {
            nx = chunk_of(cur, (s0 + 64 - cur.T) >> 6);
        } else if (have_cur) {
            const int qn = counter ? grab() : q + 1;
            if (qn < c1) {
                nxt = chain_load<R>(pd, seqb, chain_pairs[qn], cur.T + cur.S);
                have_nxt = true;
                nx = chunk_of(nxt, 0);
                q = qn - 1;  // advanced below when nxt becomes cur
            }
        }
        const uint32_t *lsel0 = ring + ((s0 - lane) & 127);  // this lane's global column at the chunk's first step
        // A chunk with every lane on cur, no switch window and no sink capture runs its own loop of plain groups:
        // with the three group variants in one loop, the register allocator copied the row state (18 v_mov) after
        // every plain group at the merge point (5.6 % of its VALU).  Pairs start on chunk boundaries (T is a
        // multiple of 64), so a window is always a whole chunk.
        const bool plain = have_cur && s0 >= cur.T && !(have_prv && s0 < cur.T + 64) &&
                           !(have_prv && prv.cap_step >= s0 && prv.cap_step < s0 + 64) &&
                           !(cur.cap_step >= s0 && cur.cap_step < s0 + 64);
        if (plain) {
            for (int g = 0; g < 64 / G; ++g) {
                const int s = s0 + g * G;
                i32_chain_group<R, TB, LEN, false, false, CK, LDOT>(
                    V, cv, cvn, Vb, tpb, top_prev, bottom, selv, lsel0 + g * G, outc, W, s, lane, -(1 << 30), prv.cap_step,
                    prv.cap_lane, prv.cap_row, capA, cur.cap_step, cur.cap_lane, cur.cap_row, capB, rcv, jv);
                if constexpr (TB) {
                    uint32_t lo = (uint32_t)lane * 16u;
                    asm volatile("" : "+v"(lo));
                    char *gp = reinterpret_cast<char *>(tb + cur.tb_off + (uint64_t)((s - cur.T) / G) * 256u);
                    *reinterpret_cast<uint4 *>(gp + lo) = make_uint4(W[0], W[1], W[2], W[3]);
                }
                if constexpr (CK) {
                    constexpr int GH = SED_CK_TILE / R;
                    if ((lane & (GH - 1)) == GH - 1)
                        store_words<G>(tb + cur.tb_off + sed_ck_col_words(R, 1, cur.nchunks) +
                                           (uint64_t)((s - cur.T) / G) * SED_CK_RW + (uint32_t)(lane / GH) * G, rcv);
                }
            }
        } else
        for (int g = 0; g < 64 / G; ++g) {
            const int s = s0 + g * G;
            const uint32_t *lsel = lsel0 + g * G;
            const bool win = have_cur && have_prv && s < cur.T + 64;  // lanes switch from prv to cur
            const bool capg = (have_prv && prv.cap_step >= s && prv.cap_step < s + G) ||
                              (have_cur && cur.cap_step >= s && cur.cap_step < s + G);
            // wave-uniform: which body; Tsw never matches a lane outside a switch window
            const int Tsw = win ? cur.T : -(1 << 30);
#define SED_CGROUP(SW, GEN)                                                                               \
    i32_chain_group<R, TB, LEN, SW, GEN, CK, LDOT>(V, cv, cvn, Vb, tpb, top_prev, bottom, selv, lsel, outc, W, s, lane, \
                                             Tsw, prv.cap_step, prv.cap_lane, prv.cap_row, capA, cur.cap_step,    \
                                             cur.cap_lane, cur.cap_row, capB, rcv, jv)
            if (capg) SED_CGROUP(false, true);
            else if (win) SED_CGROUP(true, false);
            else SED_CGROUP(false, false);
#undef SED_CGROUP
            if constexpr (TB) {
                // a lane's 16 bytes go to the pair it worked on; in the switch window a group holds
                // steps of both pairs, so it is stored to both (each slot's unused part is never read).
                // Uniform base + 32-bit lane offset: saddr stores, no per-lane 64-bit address kept live.
                uint32_t lo = (uint32_t)lane * 16u;
                asm volatile("" : "+v"(lo));
                if (have_cur && s >= cur.T) {
                    char *gp = reinterpret_cast<char *>(tb + cur.tb_off + (uint64_t)((s - cur.T) / G) * 256u);
                    *reinterpret_cast<uint4 *>(gp + lo) = make_uint4(W[0], W[1], W[2], W[3]);
                }
                // lanes still on prv: the switch window, or the final drain after the chain's last pair
                if (have_prv && s < (have_cur ? cur.T + 64 : prv.end) && (s - prv.T) / G < prv.sg) {
                    char *gp = reinterpret_cast<char *>(tb + prv.tb_off + (uint64_t)((s - prv.T) / G) * 256u);
                    *reinterpret_cast<uint4 *>(gp + lo) = make_uint4(W[0], W[1], W[2], W[3]);
                }
            }
            if constexpr (CK) {  // row checkpoints of lanes t = G-1 (mod G), to the pair(s) the group's steps belong to
                constexpr int GH = SED_CK_TILE / R;
                if ((lane & (GH - 1)) == GH - 1) {
                    const uint32_t lo = (uint32_t)(lane / GH) * G;
                    if (have_cur && s >= cur.T)
                        store_words<G>(tb + cur.tb_off + sed_ck_col_words(R, 1, cur.nchunks) +
                                           (uint64_t)((s - cur.T) / G) * SED_CK_RW + lo, rcv);
                    if (have_prv && s < (have_cur ? cur.T + 64 : prv.end) && (s - prv.T) / G < prv.sg)
                        store_words<G>(tb + prv.tb_off + sed_ck_col_words(R, 1, prv.nchunks) +
                                           (uint64_t)((s - prv.T) / G) * SED_CK_RW + lo, rcv);
                }
            }
            if (capg) {
                if (have_prv && prv.cap_step >= s && prv.cap_step < s + G && lane == prv.cap_lane)
                    chain_store_result<R, TB, LEN, CK, LDOT>(res, prv.pair, capA, prv.n, prv.m, ord_prv, prm);
                if (have_cur && cur.cap_step >= s && cur.cap_step < s + G && lane == cur.cap_lane)
                    chain_store_result<R, TB, LEN, CK, LDOT>(res, cur.pair, capB, cur.n, cur.m, ord, prm);
            }
        }
        if constexpr (CK) {  // column checkpoint of cur's local chunk: every lane is on cur at a chunk end
            if (have_cur) {
                const int lc = (s0 - cur.T) >> 6;
                if (lc < cur.nchunks) {
                    uint32_t *cp = tb + cur.tb_off + sed_ck_col_word(R, 0, cur.nchunks, lc, 0, lane);
#pragma unroll
                    for (int r = 0; r < R; ++r) cp[r * 64] = V[r];
                    cp[R * 64] = top_prev;
                }
            }
        }
        {  // global columns s0 + 64 .. s0 + 127, after the chunk's last LDS read (in order)
            const uint32_t slot = (uint32_t)(s0 + 64 + lane) & 127u;
            ring[slot] = ring[slot + 128] = nx.y;
        }
        const int s1 = s0 + 64;
        if (have_cur && s1 == cur.T + cur.S) {  // lane 0 is done with cur: it becomes the draining pair
            prv = cur;
            ord_prv = ord;
            have_prv = true;
            capA = capB;
            if (have_nxt) {
                cur = nxt;
                ++q;
                ++ord;
                rows_of(cur.pair, cvn);
                // lane 0 switches before the next pair's first step
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    V[r] = lane == 0 ? Vb[r] : V[r];
                    cv[r] = lane == 0 ? cvn[r] : cv[r];
                }
                top_prev = lane == 0 ? tpb : top_prev;
            } else {
                have_cur = false;
            }
        }
        if (have_prv && s1 >= prv.end && (!have_cur || s1 >= cur.T + 64)) have_prv = false;  // drained
        if (!have_cur && !have_prv) break;
    }
}

// ---------------------------------------------------------------------------
// Self-test of the cross-lane primitives the kernels rely on.
// ---------------------------------------------------------------------------
__global__ void sed_selftest_kernel(uint32_t *out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t v = 1000u + lane;
    uint32_t fail = 0;
    const uint32_t shr = dpp_shr1(7u, v);
    if (shr != (lane == 0 ? 7u : 999u + lane)) fail |= 1;
    const uint32_t shl = dpp_shl1(9u, v);
    if (shl != (lane == 63 ? 9u : 1001u + lane)) fail |= 2;
    const uint32_t rol = dpp_rol1(v);
    if (rol != 1000u + ((lane + 1) & 63)) fail |= 4;
    const uint32_t p = __builtin_amdgcn_perm(0x44332211u, 0xFFFFFFFEu, i32_sel(lane & 3));
    if (p != (0xFF00FFFEu | (((0x44332211u >> (8 * (lane & 3))) & 0xFFu) << 16))) fail |= 8;
    const uint32_t ab = __builtin_amdgcn_alignbit(0x3u + (lane << 2), 0x80000000u, 2);
    if (ab != (0xE0000000u | 0x20000000u)) fail |= 16;
    // the 16-lane segment moves of the fp64 kernel's short-pair route (row_shr:1, row_shl:1, row_ror:15)
    const uint32_t sl = lane & 15u;
    if (seg_shr1<16>(7u, v) != (sl == 0 ? 7u : 999u + lane)) fail |= 32;
    if (seg_shl1<16>(9u, v) != (sl == 15 ? 9u : 1001u + lane)) fail |= 64;
    if (seg_rol1<16>(v) != 1000u + (lane & ~15u) + ((sl + 1) & 15u)) fail |= 128;
    atomicOr(out, fail);
}

// ---------------------------------------------------------------------------
// Launchers (host side, called from sed_runtime.cpp)
// ---------------------------------------------------------------------------
hipError_t sed_launch_i32_cut(const sed_launch &L, const int32_t *list, int nlist, const sed_i32_params &prm,
                              uint32_t tkey) {
    if (nlist <= 0 || !L.band || !L.bandp) return hipErrorInvalidValue;
    const hipError_t e = sed_launch_cut_band(L, list, nlist, nullptr, *L.bandp, tkey);  // (the phase's start event)
    if (e != hipSuccess) return e;
    sed_launch Lf = L;
    Lf.ev0 = nullptr;
    const dim3 grid((nlist + 3) / 4), block(256);
    const int2 *lp = reinterpret_cast<const int2 *>(list);  // (the kernel's `tasks` argument: CUT reads it as the list)
    const uint32_t *a = (const uint32_t *)L.seqa, *b = (const uint32_t *)L.seqb;
    return sed_for_R<4, 8, 16>(L.R, [&](auto r) {
        SED_LAUNCH((sed_wf_i32_kernel<decltype(r)::value, false, false, false, false, false, true>), grid, block, 0, Lf, L.pd,
                   nlist, lp, a, b, (uint32_t *)nullptr, L.bnd, L.res, prm, (const sed_band *)L.band, sed_stripe_wins{});
        return hipGetLastError();
    });
}
template <int R, bool TB, bool LEN = true, bool CK = false, bool DOT = false>
static hipError_t launch_i32_R(const sed_launch &L, const sed_i32_params &prm) {
    if (L.ntasks > 0) {  // SPLIT: one workgroup per (pair, stripe): the compute wave and its feeder
        if constexpr (CK && R != 4) {  // (SPLIT checkpoints: R = 4 only)
            return hipErrorInvalidValue;
        } else {
            SED_LAUNCH((sed_wf_i32_kernel<R, TB, true, LEN, CK, DOT>), dim3(L.ntasks), dim3(128), 0, L, L.pd, L.npairs,
                       L.tasks, (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.tb, L.bnd, L.res, prm,
                       (const sed_band *)nullptr, sed_stripe_wins{});
        }
    } else {
        const int grid = (L.npairs + 3) / 4;
        // SED_OCC_LDS (tuning/A-B only): dynamic LDS bytes per workgroup, which caps the resident waves
        static const int occ_lds = [] { const char *e = getenv("SED_OCC_LDS"); return e ? atoi(e) : 0; }();
        sed_launch Lf = L;
        if (CK && L.band && L.bandp) {  // band pruning: this run's windows first (the phase's start event rides on it)
            const hipError_t e = sed_launch_band(L, *L.bandp);
            if (e != hipSuccess) return e;
            Lf.ev0 = nullptr;
        }
        SED_LAUNCH((sed_wf_i32_kernel<R, TB, false, LEN, CK, DOT>), dim3(grid), dim3(256), occ_lds, Lf, L.pd, L.npairs,
                           L.tasks, (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.tb, L.bnd, L.res,
                           prm, CK ? (const sed_band *)L.band : nullptr,
                           CK && L.band ? sed_stripe_wins{L.bwin, L.bsuf, L.bstripes} : sed_stripe_wins{});
    }
    return hipGetLastError();
}

template <int R, bool TB, bool LEN, bool CK = false, int LDOT = 0>
static hipError_t launch_chain_R(const sed_launch &L, const sed_i32_params &prm) {
    SED_LAUNCH((sed_wf_i32_chain_kernel<R, TB, LEN, CK, LDOT>), dim3((L.nchains + 3) / 4), dim3(256), 0, L, L.pd,
                       L.chain_pairs, L.chain_off, L.nchains, L.chain_counter, L.chain_base, L.chain_list,
                       (const uint32_t *)L.seqa, (const uint32_t *)L.seqb, L.tb, L.res, prm);
    return hipGetLastError();
}

hipError_t sed_launch_i32_chain(const sed_launch &L, const sed_i32_params &prm, bool len) {
    const bool tb = L.tb != nullptr;
    return sed_for_R<4, 8, 16>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (tb && L.ck) return launch_chain_R<R, false, false, true>(L, prm);  // distance keys + checkpoints
        if (prm.lad == 2 && len)
            return tb ? launch_chain_R<R, true, true, false, 2>(L, prm) : launch_chain_R<R, false, true, false, 2>(L, prm);
        if (prm.lad && len)
            return tb ? launch_chain_R<R, true, true, false, 1>(L, prm) : launch_chain_R<R, false, true, false, 1>(L, prm);
        return tb ? launch_chain_R<R, true, true>(L, prm)
                  : (len ? launch_chain_R<R, false, true>(L, prm) : launch_chain_R<R, false, false>(L, prm));
    });
}

hipError_t sed_launch_i32x2(const sed_launch &L, const int32_t *list, int nwaves, const sed_i32_params &prm) {
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((nwaves + 3) / 4), block(256);
    const uint32_t *a = (const uint32_t *)L.seqa, *b = (const uint32_t *)L.seqb;
    return sed_for_R<4, 8, 16, 32>(L.R, [&](auto r) {
        SED_LAUNCH((sed_wf_i32x2_kernel<decltype(r)::value>), grid, block, 0, L, L.pd, list, nwaves, a, b, L.bnd, L.res, prm);
        return hipGetLastError();
    });
}

hipError_t sed_launch_i32(const sed_launch &L, const sed_i32_params &prm, bool len) {
    const bool tb = L.tb != nullptr;
    if (tb && L.ck)  // distance keys + checkpoints (SPLIT has them at R = 4 only, sed_ck_codes_kernel: launch_i32_R refuses the rest)
        return sed_for_R<4, 8, 16>(L.R, [&](auto r) {
            constexpr int R = decltype(r)::value;
            // dot keys: the host found a byte factorisation of the update addends
            return prm.dot ? launch_i32_R<R, false, false, true, true>(L, prm) : launch_i32_R<R, false, false, true>(L, prm);
        });
    return sed_for_R<4, 8, 16, 32>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        return tb ? launch_i32_R<R, true>(L, prm)
                  : (len ? launch_i32_R<R, false>(L, prm) : launch_i32_R<R, false, false>(L, prm));
    });
}

hipError_t sed_launch_selftest(uint32_t *d_out, hipStream_t stream) {
    hipLaunchKernelGGL(sed_selftest_kernel, dim3(1), dim3(64), 0, stream, d_out);
    return hipGetLastError();
}

