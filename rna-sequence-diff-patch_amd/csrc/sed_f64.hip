// sed_f64.hip — the fp64 kernels (general costs): one wave per pair or per 16-lane segment (sed_wf_f64_kernel), one
// workgroup per stripe (SPLIT, sed_wf_f64_split_kernel; the hand-off's tagged words: sed_dev.h), and their launchers.
#include <hip/hip_ext.h>
#include "sed_internal.h"
#include "sed_dev.h"

// ---------------------------------------------------------------------------
// fp64 kernel (general costs).  State per row: D (fp64), Lk = L << 2,
// optional int-typing bit T (TYPED).  Cost table in LDS:
//   tab[a*K + b] = {cost value, is-int flag}
// ---------------------------------------------------------------------------
// Path-length keys of the fp64 kernel in U-space: LK = SED_F64_LB - 4U (U = updates on the canonical path to the
// cell, so L = i + j - U) with the op in the low 2 bits of a candidate.  At a cell every candidate's L is the cell's
// i + j - U, so comparing B - 4U orders candidates exactly as L does, and the borders are all B: the insert
// candidate is LK_left (op 0), the delete candidate LK_up + 1, the update candidate LK_diag - 4 + 2.  (L << 2 keys
// took an add per candidate, +4, +5, +6: 21.25 against 20.25 VALU per cell on the R = 8 group loop's unmasked path.)
#define SED_F64_LB 0x80000000u
struct f64_cell_in {
    double d;
    uint32_t lk;
    uint32_t t;
};

// PF: the caller has moved this step's column symbol (bsel) and read its table entries (epf) a step ahead (the
// SPLIT kernel's lone waves, whose LDS reads would otherwise stall every step)
template <int R, bool TB, bool TYPED, bool MASKED, bool FULL, int SW = 64, bool PF = false>
__device__ __forceinline__ void f64_step(double (&D)[R], uint32_t (&LK)[R], uint32_t (&T)[R],
                                         const uint32_t (&rowbase)[R], const double2 *__restrict__ tab,
                                         double &dtop_prev, uint32_t &ltop_prev, uint32_t &ttop_prev,
                                         double &dbot, uint32_t &lbot, uint32_t &tbot, uint32_t &bsel,
                                         const double dtin, const uint32_t ltin, const uint32_t ttin,
                                         const uint32_t stin, uint32_t (&W)[4], const int u,
                                         const double cins, const double cdel, const uint32_t tins,
                                         const uint32_t tdel, const bool active, const sed_full_out &fo,
                                         const int i0, const int j, const double2 *epf = nullptr) {
    // the segment's first lane takes this step's top-row cell and column symbol (dtin .. stin, broadcast LDS reads of
    // the chunk), the others the lane above's bottom cell and previous symbol
    const double dtop = seg_shr1_f64<SW>(dtin, dbot);
    const uint32_t ltop = seg_shr1<SW>(ltin, lbot);
    uint32_t ttop = 0;
    if constexpr (TYPED) ttop = seg_shr1<SW>(ttin, tbot);
    if constexpr (!PF) bsel = seg_shr1<SW>(stin, bsel);
    double dup = dtop, ddiag = dtop_prev;
    uint32_t lup = ltop, ldiag = ltop_prev, tup = ttop, tdiag = ttop_prev;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double2 e = PF ? epf[r] : tab[rowbase[r] + bsel];  // x = cost, y = int flag (as double bits)
        const double dl = D[r];
        const double ca = dl + cins;
        const double cb = dup + cdel;
        const double cc = ddiag + e.x;
        const double mn = fmin(ca, fmin(cb, cc));
        const bool ea = (ca == mn), eb = (cb == mn), ec = (cc == mn);
        const uint32_t ka = ea ? LK[r] : 0xFFFFFFFFu;  // (U-space keys: the insert candidate needs no add)
        const uint32_t kb = eb ? lup + 1u : 0xFFFFFFFFu;
        const uint32_t kc = ec ? ldiag - 2u : 0xFFFFFFFFu;
        const uint32_t km = umin3_op(ka, kb, kc);
        const uint32_t ln = km & ~3u;
        uint32_t tn = 0;
        if constexpr (TYPED) {
            const uint32_t tc = (uint32_t)__double_as_longlong(e.y);
            tn = ea ? (T[r] & tins) : (eb ? (tup & tdel) : (tdiag & tc));
        }
        if constexpr (TB) {
            const int c = u * R + r;
            W[c >> 4] = __builtin_amdgcn_alignbit(km, W[c >> 4], 2);
        }
        if constexpr (FULL) {  // full-matrix materialisation (dp proxy, GUI path): value, edge mask, typing
            if (active && i0 + r <= fo.n) {
                const uint64_t o = (uint64_t)(i0 + r) * (uint64_t)(fo.m + 1) + (uint64_t)j;
                const uint32_t t = TYPED ? tn : (uint32_t)(mn == 0.0);
                fo.D[o] = mn;
                fo.M[o] = (uint8_t)((ea ? 1u : 0u) | (eb ? 2u : 0u) | (ec ? 4u : 0u) | (t << 3));
            }
        }
        ddiag = dl;
        ldiag = LK[r];
        if constexpr (TYPED) tdiag = T[r];
        dup = mn;
        lup = ln;
        if constexpr (TYPED) tup = tn;
        if constexpr (MASKED) {
            D[r] = active ? mn : dl;
            LK[r] = active ? ln : LK[r];
            if constexpr (TYPED) T[r] = active ? tn : T[r];
        } else {
            D[r] = mn;
            LK[r] = ln;
            if constexpr (TYPED) T[r] = tn;
        }
    }
    if constexpr (MASKED) {
        dtop_prev = active ? dtop : dtop_prev;
        ltop_prev = active ? ltop : ltop_prev;
        if constexpr (TYPED) ttop_prev = active ? ttop : ttop_prev;
    } else {
        dtop_prev = dtop;
        ltop_prev = ltop;
        if constexpr (TYPED) ttop_prev = ttop;
    }
    dbot = D[R - 1];
    lbot = LK[R - 1];
    if constexpr (TYPED) tbot = T[R - 1];
}

// Per wave: the current chunk's top row (cell values, L keys, typing) and str2 symbols, which the segment's first lane
// reads one per step, and the segment's last lane's bottom cells of the chunk, which it writes one per step (the
// next stripe's top row, stored to global memory at the chunk's end).  These replace DPP rotations of the chunk
// values and a DPP collection of the bottom cells: 8-11 VALU per step.
struct f64_chunk_lds {
    double d[64], od[64];
    uint32_t l[64], t[64], s[64], ol[64], ot[64];
};

// SW = 64: one wave per pair (pairs with d.seg set are skipped: they run in segments).  SW = 16 (short pairs of
// large batches): each DPP row of 16 lanes runs its own pair (items idx[0 .. nidx), four per wave, the
// host sorts them so a wave's four pairs have similar shapes): stripes of 16 R rows, 16-step chunks, a 15-step ramp
// instead of 63, and every lane move a row DPP (seg_*), so the four segments never exchange data.  The loop bounds
// are then per lane (uniform within a segment), and a segment whose pair is done sits out with its lanes masked.
// issue priority of the fp64 DP's waves (SED_F64_PRIO): pipelined fp64 script batches run the traceback of run k
// beside the DP of run k+1, which now issues first.  iupac 4.83-4.85 against 4.87-4.89 ms per step at 0, timing within
// noise, 3 interleaved rounds (profiles/r05/s17)
#ifndef SED_F64_PRIO
#define SED_F64_PRIO 1
#endif
template <int R, bool TB, bool TYPED, bool FULL, int SW = 64>
__global__ __launch_bounds__(256) void sed_wf_f64_kernel(const sed_pair_desc *__restrict__ pd, int npairs,
                                                         const uint8_t *__restrict__ seqa,
                                                         const uint8_t *__restrict__ seqb,
                                                         uint32_t *__restrict__ tb, uint32_t *__restrict__ bnd,
                                                         sed_result *__restrict__ res,
                                                         const double *__restrict__ gtab, sed_f64_params prm,
                                                         sed_full_out fo, const int32_t *__restrict__ idx) {
    if constexpr (SED_F64_PRIO > 0) __builtin_amdgcn_s_setprio(SED_F64_PRIO);
    static_assert(SW == 64 || (SW == 16 && !FULL), "segments of 16 lanes: no full-matrix output");
    constexpr int ROWS = SW * R;
    constexpr int G = Grp<R>::G;
    static_assert(SW % G == 0, "a group of G steps never crosses a chunk");
    __shared__ double2 tab[SED_MAX_K * SED_MAX_K];
    __shared__ f64_chunk_lds chx[4];
    const int K = prm.K;
    for (int e = threadIdx.x; e < K * K; e += blockDim.x)
        tab[e] = make_double2(gtab[2 * e], gtab[2 * e + 1]);
    __syncthreads();

    const int lane = SW == 64 ? (threadIdx.x & 63) : (threadIdx.x & (SW - 1));  // lane within the segment
    int pair;
    if constexpr (SW == 64) {
        pair = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
        if (pair >= npairs) return;
    } else {
        const int item = (blockIdx.x * 256 + threadIdx.x) / SW;
        if (item >= npairs) return;  // (npairs = the item count)
        pair = idx[item];
    }
    const sed_pair_desc d = pd[pair];
    if (d.lane || (SW == 64 && d.pad[1])) return;  // short str2, distance only: sed_lane.hip; segments: the SW = 16 launch
    const int n = d.n, m = d.m;
    if constexpr (FULL) {  // border cells: row 0 (insert edges) and column 0 (delete edges)
        for (int j = lane; j <= m; j += 64) {
            const double v = (double)j * prm.ins;
            const uint32_t t = (j == 0) ? 1u : (TYPED ? (uint32_t)prm.ins_int : (uint32_t)(v == 0.0));
            fo.D[j] = v;
            fo.M[j] = (uint8_t)((j == 0 ? 0u : 1u) | (t << 3));
        }
        for (int i = 1 + lane; i <= n; i += 64) {
            const double v = (double)i * prm.del;
            const uint32_t t = TYPED ? (uint32_t)prm.del_int : (uint32_t)(v == 0.0);
            fo.D[(uint64_t)i * (m + 1)] = v;
            fo.M[(uint64_t)i * (m + 1)] = (uint8_t)(2u | (t << 3));
        }
    }
    if (n == 0 || m == 0) {
        if (lane == 0) {
            res[pair].dist = (n == 0) ? (double)m * prm.ins : (double)n * prm.del;
            res[pair].len = n + m;
            res[pair].is_int = (n == 0 && m == 0) ? 1 : (n == 0 ? prm.ins_int : prm.del_int);
            res[pair].err = 0;
        }
        return;
    }
    const int nstripes = (n + ROWS - 1) / ROWS;
    const int SG = (m + SW - 1 + G - 1) / G * G;
    const int nchunks = (SG + SW - 1) / SW;
    // bottom-row buffer of a pair: [D as u64 | L as u32 | T as u32] planes; column j at index j + SW
    const uint64_t bwords = (uint64_t)(nchunks + 2) * SW;
    uint64_t *bndD = reinterpret_cast<uint64_t *>(bnd + d.bnd_off);
    uint32_t *bndL = bnd + d.bnd_off + 2 * bwords;
    uint32_t *bndT = bndL + bwords;
    const uint8_t *pa = seqa + d.a_off;
    const uint8_t *pb = seqb + d.b_off;
    const uint32_t tins = (uint32_t)prm.ins_int, tdel = (uint32_t)prm.del_int;

    for (int k = 0; k < nstripes; ++k) {
        const int row0 = k * ROWS + lane * R;
        double D[R];
        uint32_t LK[R], T[R], rowbase[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ri = row0 + r;
            const uint32_t a = (ri < n) ? pa[ri] : 0u;
            rowbase[r] = a * (uint32_t)K;
            D[r] = (double)(ri + 1) * prm.del;
            LK[r] = SED_F64_LB;
            T[r] = tdel;
        }
        double dtop_prev = (double)row0 * prm.del;
        uint32_t ltop_prev = SED_F64_LB;
        uint32_t ttop_prev = (row0 == 0) ? 1u : tdel;
        double dbot = 0.0;
        uint32_t lbot = 0, tbot = 0, bsel = 0;
        uint32_t W[4] = {0, 0, 0, 0};

        auto load_d = [&](int c) -> double {
            const int j = SW * c + lane + 1;
            if (k == 0) return (double)j * prm.ins;
            return __longlong_as_double((long long)load_sc1_u64(bndD + j + SW));
        };
        auto load_l = [&](int c) -> uint32_t {
            const int j = SW * c + lane + 1;
            if (k == 0) return SED_F64_LB;
            return load_sc1(bndL + j + SW);
        };
        auto load_t = [&](int c) -> uint32_t {
            if (k == 0) return tins;
            return load_sc1(bndT + SW * c + lane + SW + 1);
        };
        auto load_sel = [&](int c) -> uint32_t {
            const int ci = SW * c + lane;
            return (ci < m) ? (uint32_t)pb[ci] : 0u;
        };
        double dch = load_d(0);
        uint32_t lch = load_l(0), tch = TYPED ? load_t(0) : 0u, sch = load_sel(0);
        f64_chunk_lds &cx = chx[threadIdx.x >> 6];
        const int sb = (threadIdx.x & 63) - lane;  // the segment's first slot
        const bool lastlane = lane == SW - 1;
        uint32_t *tbk = tb + d.tb_off + (uint64_t)k * (uint64_t)(SG / G) * (SW * 4u);
        const bool last = (k == nstripes - 1);
        int s = 0;
        for (int c = 0; c < nchunks; ++c) {
            double dnx = 0.0;
            uint32_t lnx = 0, tnx = 0, snx = 0;
            if (c + 1 < nchunks) {
                dnx = load_d(c + 1);
                lnx = load_l(c + 1);
                if (TYPED) tnx = load_t(c + 1);
                snx = load_sel(c + 1);
            }
            // this chunk's top row and symbols (after the previous chunk's last reads: a wave's LDS accesses run in
            // order)
            cx.d[sb + lane] = dch;
            cx.l[sb + lane] = lch;
            if (TYPED) cx.t[sb + lane] = tch;
            cx.s[sb + lane] = sch;
            // (A separate loop for chunks of unmasked steps, as in the integer kernels, measured slower: iupac DP
            // 4.89 against 4.81 ms, timing 4.60 against 4.47 ms; profiles/r03/f64_plain_dropped.)
            for (int g = 0; g < SW / G && s < SG; ++g, s += G) {
                const bool full = (s >= SW - 1) && (s + G - 1 < m);
                const int cu0 = sb + g * G;
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const int j = s + u - lane + 1;
                    const bool active = (j >= 1) && (j <= m);
                    const double dtin = cx.d[cu0 + u];
                    const uint32_t ltin = cx.l[cu0 + u], ttin = TYPED ? cx.t[cu0 + u] : 0u, stin = cx.s[cu0 + u];
                    if (full)
                        f64_step<R, TB, TYPED, false, FULL, SW>(D, LK, T, rowbase, tab, dtop_prev, ltop_prev, ttop_prev,
                                                                dbot, lbot, tbot, bsel, dtin, ltin, ttin, stin, W, u,
                                                                prm.ins, prm.del, tins, tdel, active, fo, row0 + 1, j);
                    else
                        f64_step<R, TB, TYPED, true, FULL, SW>(D, LK, T, rowbase, tab, dtop_prev, ltop_prev, ttop_prev,
                                                               dbot, lbot, tbot, bsel, dtin, ltin, ttin, stin, W, u,
                                                               prm.ins, prm.del, tins, tdel, active, fo, row0 + 1, j);
                    if (!last && lastlane) {  // the next stripe's top row
                        cx.od[cu0 + u] = dbot;
                        cx.ol[cu0 + u] = lbot;
                        if (TYPED) cx.ot[cu0 + u] = tbot;
                    }
                }
                if constexpr (TB) store_tb(tbk + ((uint64_t)(s / G) * SW + lane) * 4u, W);
            }
            // slot i holds the segment's last lane's bottom cell of the chunk's step SW c + i, i.e. column
            // SW (c - 1) + 2 + i at index SW c + 2 + i (a short last chunk: only its steps' slots)
            if (!last && lane < s - SW * c) {
                bndD[SW * c + 2 + lane] = (uint64_t)__double_as_longlong(cx.od[sb + lane]);
                bndL[SW * c + 2 + lane] = cx.ol[sb + lane];
                if (TYPED) bndT[SW * c + 2 + lane] = cx.ot[sb + lane];
            }
            dch = dnx;
            lch = lnx;
            tch = tnx;
            sch = snx;
        }
        if (!last) __builtin_amdgcn_s_waitcnt(0);
        else {
            const int w = (n - 1) % ROWS;
            if (lane == w / R) {
                const int rf = w % R;
                double dv = 0.0;
                uint32_t lv = 0, tv = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    dv = (r == rf) ? D[r] : dv;
                    lv = (r == rf) ? LK[r] : lv;
                    tv = (r == rf) ? T[r] : tv;
                }
                res[pair].dist = dv;
                res[pair].len = n + m - (int32_t)((SED_F64_LB - lv) >> 2);
                res[pair].is_int = TYPED ? (uint8_t)tv : (uint8_t)(dv == 0.0);
                res[pair].err = 0;
            }
        }
    }
}

// SPLIT fp64 (few long pairs: timing.py's one-call loop, GUI calls over IUPAC symbols).  A lone fp64 wave issues
// ~20 dependent VALU per cell on one SIMD (a 2000^2 pair took 3.5 ms), so, as in the integer SPLIT kernel, each
// stripe of 64 R rows (R = 2 by default, 4 on request) is a 128-thread workgroup of its own: all stripes of a pair
// run at once, each ~63 steps (its lanes' systolic depth) plus a 16-step block and the hand-off's latency behind the
// stripe above.  The hand-off is the integer kernel's tagged words: lane 63's bottom cell of column j
// travels as three relaxed agent-scope 64-bit stores {tag, D low}, {tag, D high}, {tag, L key | T} (the L key is a
// multiple of 4, so its bit 0 carries the typing bit), each single-copy atomic and validated on its own, tag = the
// run's epoch | poison << 31.  The feeder wave (f64_split_feed) polls the stripe above's words, writes the steps'
// top-row cells and str2 symbols into an LDS ring and publishes how many steps are ready; stripe 0's feeder writes
// the row-0 border.  The compute wave is sed_wf_f64_kernel's stripe loop (SW = 64) reading the ring, with each step's
// column symbol and table entries read a step ahead (f64_step PF).  Codes, their layout and the result are the
// one-wave kernel's, so the tracebacks read them unchanged.
#define SED_F64_RING 256
template <int G> struct f64_split_lds {
    double d[SED_F64_RING];
    uint32_t l[SED_F64_RING], t[SED_F64_RING], s[SED_F64_RING];
    double od[G][64];  // every lane's bottom cell of the group's steps (lane 63's are handed off)
    uint32_t ol[G][64], ot[G][64];
};
// the three hand-off planes of stripe k: words [plane][column + 64], (nchunks + 2) * 64 per plane
__device__ __forceinline__ uint64_t *f64_split_words(uint32_t *bnd, const sed_pair_desc &d, int k, uint32_t plane_words) {
    return reinterpret_cast<uint64_t *>(bnd + d.bnd_off) + (uint64_t)k * 3u * plane_words;
}
template <int G>
__device__ void f64_split_feed(const uint64_t *__restrict__ hin, const uint32_t plane_words, const bool top, const int m,
                               const int SG, const uint32_t epoch, const uint8_t *__restrict__ pb, const double ins,
                               const uint32_t tins, f64_split_lds<G> &rg, uint32_t *flag, const int lane) {
    uint32_t poison = 0, idle = 0;
    int have = 0;  // steps whose top-row cells are in the ring
    while (have < SG) {
        if (have + 64 > (int)lds_flag_get(flag + 1) + SED_F64_RING) {  // ring full: the compute wave is behind
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        const int t = have + lane, col = t + 1;
        const bool need = !top && t < SG && col <= m;  // columns past m are never stored nor waited for
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (need) {
            w0 = load_sc1_u64(hin + (uint32_t)(col + 64));
            w1 = load_sc1_u64(hin + plane_words + (uint32_t)(col + 64));
            w2 = load_sc1_u64(hin + 2u * plane_words + (uint32_t)(col + 64));
        }
        const uint32_t g0 = (uint32_t)(w0 >> 32), g1 = (uint32_t)(w1 >> 32), g2 = (uint32_t)(w2 >> 32);
        const bool good = !need || (((g0 & ~SED_PROG_POISON) == epoch) && ((g1 & ~SED_PROG_POISON) == epoch) &&
                                    ((g2 & ~SED_PROG_POISON) == epoch));
        const uint64_t bad = __ballot(!good);
        const int nv = min(bad ? (int)__builtin_ctzll(bad) : 64, SG - have);  // the valid prefix
        if (__any(lane < nv && need && ((g0 | g1 | g2) & SED_PROG_POISON))) poison = SED_PROG_POISON;
        if (nv > 0) {
            if (lane < nv) {
                const int slot = t & (SED_F64_RING - 1);
                if (top) {  // row 0: D = j * insert, L key B, typing of insert
                    rg.d[slot] = (double)col * ins;
                    rg.l[slot] = SED_F64_LB;
                    rg.t[slot] = tins;
                } else {
                    rg.d[slot] = __longlong_as_double((long long)(((w1 & 0xFFFFFFFFull) << 32) | (w0 & 0xFFFFFFFFull)));
                    rg.l[slot] = (uint32_t)w2 & ~3u;
                    rg.t[slot] = (uint32_t)w2 & 1u;
                }
                rg.s[slot] = t < m ? (uint32_t)pb[t] : 0u;
            }
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

template <int R, bool TB, bool TYPED, bool FULL>
__global__ __launch_bounds__(128) void sed_wf_f64_split_kernel(const sed_pair_desc *__restrict__ pd,
                                                               const int2 *__restrict__ tasks,
                                                               const uint8_t *__restrict__ seqa,
                                                               const uint8_t *__restrict__ seqb,
                                                               uint32_t *__restrict__ tb, uint32_t *__restrict__ bnd,
                                                               sed_result *__restrict__ res,
                                                               const double *__restrict__ gtab, sed_f64_params prm,
                                                               sed_full_out fo) {
    if constexpr (SED_SPLIT_PRIO > 0) __builtin_amdgcn_s_setprio(SED_SPLIT_PRIO);
    static_assert(!(FULL && TB), "full-matrix output: distance kernel");
    constexpr int ROWS = 64 * R;
    constexpr int G = Grp<R>::G;
    __shared__ double2 tab[SED_MAX_K * SED_MAX_K];
    __shared__ f64_split_lds<Grp<R>::G> rg;
    __shared__ uint32_t split_flag[2];
    const int K = prm.K;
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) tab[e] = make_double2(gtab[2 * e], gtab[2 * e + 1]);
    if (threadIdx.x < 2) split_flag[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int2 task = tasks[blockIdx.x];
    const int pair = __builtin_amdgcn_readfirstlane(task.x), k = __builtin_amdgcn_readfirstlane(task.y);
    const sed_pair_desc d = pd[pair];
    const int n = d.n, m = d.m;
    if constexpr (FULL) {  // border cells (stripe 0's compute wave): row 0 (insert edges) and column 0 (delete edges)
        if (k == 0 && threadIdx.x < 64) {
            for (int j = lane; j <= m; j += 64) {
                const double v = (double)j * prm.ins;
                const uint32_t t = (j == 0) ? 1u : (TYPED ? (uint32_t)prm.ins_int : (uint32_t)(v == 0.0));
                fo.D[j] = v;
                fo.M[j] = (uint8_t)((j == 0 ? 0u : 1u) | (t << 3));
            }
            for (int i = 1 + lane; i <= n; i += 64) {
                const double v = (double)i * prm.del;
                const uint32_t t = TYPED ? (uint32_t)prm.del_int : (uint32_t)(v == 0.0);
                fo.D[(uint64_t)i * (m + 1)] = v;
                fo.M[(uint64_t)i * (m + 1)] = (uint8_t)(2u | (t << 3));
            }
        }
    }
    if (n == 0 || m == 0) {
        if (threadIdx.x == 0) {
            res[pair].dist = (n == 0) ? (double)m * prm.ins : (double)n * prm.del;
            res[pair].len = n + m;
            res[pair].is_int = (n == 0 && m == 0) ? 1 : (n == 0 ? prm.ins_int : prm.del_int);
            res[pair].err = 0;
        }
        return;
    }
    const int nstripes = (n + ROWS - 1) / ROWS;
    const int SG = (m + 63 + G - 1) / G * G;
    const int nchunks = (SG + 63) >> 6;
    const uint32_t plane_words = (uint32_t)(nchunks + 2) * 64u;
    const uint8_t *pa = seqa + d.a_off;
    const uint8_t *pb = seqb + d.b_off;
    const uint32_t tins = (uint32_t)prm.ins_int, tdel = (uint32_t)prm.del_int;
    if (threadIdx.x >= 64) {  // the feeder wave
        f64_split_feed<G>(k > 0 ? f64_split_words(bnd, d, k - 1, plane_words) : nullptr, plane_words, k == 0, m, SG,
                       prm.epoch, pb, prm.ins, tins, rg, split_flag, lane);
        return;
    }
    uint64_t *hout = f64_split_words(bnd, d, k, plane_words);
    const int row0 = k * ROWS + lane * R;
    double D[R];
    uint32_t LK[R], T[R], rowbase[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ri = row0 + r;
        const uint32_t a = (ri < n) ? pa[ri] : 0u;
        rowbase[r] = a * (uint32_t)K;
        D[r] = (double)(ri + 1) * prm.del;
        LK[r] = SED_F64_LB;
        T[r] = tdel;
    }
    double dtop_prev = (double)row0 * prm.del;
    uint32_t ltop_prev = SED_F64_LB;
    uint32_t ttop_prev = (row0 == 0) ? 1u : tdel;
    double dbot = 0.0;
    uint32_t lbot = 0, tbot = 0, bsel = 0;
    uint32_t W[4] = {0, 0, 0, 0};
    uint32_t *tbk = TB ? tb + d.tb_off + (uint64_t)k * (uint64_t)(SG / G) * 256u : nullptr;
    const bool last = (k == nstripes - 1);
    const uint32_t tag = prm.epoch;
    bool ok = true;
    int ready = 0;  // steps the feeder has published as ready (last read)
    constexpr int HB = G < 16 ? G : 16;  // steps per block of ring reads, waits and hand-offs
    // until the ring holds the top-row cells of steps < upto (LDS only)
    auto wait_ready = [&](int upto) {
        upto = min(upto, SG);  // (the feeder publishes SG steps in all)
        if (ready < upto) {
            uint32_t f = lds_flag_get(split_flag), spins = 0;
            while (ok && (int)(f & ~SED_PROG_POISON) < upto) {
                if (++spins > (1u << 24)) ok = false;
                __builtin_amdgcn_s_sleep(1);
                f = lds_flag_get(split_flag);
            }
            if (f & SED_PROG_POISON) ok = false;
            ready = (int)(f & ~SED_PROG_POISON);
            asm volatile("" ::: "memory");
        }
    };
    // lane u < HB hands off column s0 + u - 62 (lane 63's cell of step s0 + u, staged at rg.od[u0 + u]), then the
    // block's ring slots are free again
    auto handoff = [&](const int s0, const int u0) {
        if (!last && lane < HB) {
            const int col = s0 + lane - 62;
            if (col >= 1 && col <= m) {
                const uint32_t tg = tag | (ok ? 0u : SED_PROG_POISON);
                const uint64_t bits = (uint64_t)__double_as_longlong(rg.od[u0 + lane][63]);
                const uint32_t lt = rg.ol[u0 + lane][63] | (TYPED ? rg.ot[u0 + lane][63] : 0u);
                store_tagged(hout + (uint32_t)(col + 64), tg, (uint32_t)bits);
                store_tagged(hout + plane_words + (uint32_t)(col + 64), tg, (uint32_t)(bits >> 32));
                store_tagged(hout + 2u * plane_words + (uint32_t)(col + 64), tg, lt);
            }
        }
        asm volatile("" ::: "memory");
        if (lane == 0) lds_flag_set(split_flag + 1, (uint32_t)(s0 + HB));
    };
    for (int s = 0; s < SG; s += G) {
        // a block needs its own steps and the next block's first symbol (the table reads a step ahead)
        wait_ready(s + (HB < G ? HB + 1 : HB));
        // the group's steps as one straight-line block per variant (a lone wave is latency-bound: a branch per step
        // kept the compiler from overlapping one step's table reads with the previous step's arithmetic)
        // The group's top-row cells and symbols are read from the ring at its start, and each step's column symbol
        // and table entries are fetched one step ahead (PF).
        // (ring entries in blocks of 16 steps: the R = 2 group's 32 would take ~160 VGPRs at once; each block waits
        // for its own steps and hands its bottom cells off, so the stripe below trails by 16 steps, not 32)
        auto group = [&](auto masked_tag) {
            constexpr bool MASKED = decltype(masked_tag)::value;
            double2 en[R];
            uint32_t bn = dpp_shr1(rg.s[s & (SED_F64_RING - 1)], bsel);
#pragma unroll
            for (int r = 0; r < R; ++r) en[r] = tab[rowbase[r] + bn];
#pragma unroll
            for (int h = 0; h < G; h += HB) {
                if (h > 0) wait_ready(s + h + (h + HB < G ? HB + 1 : HB));
                double dg[HB];
                uint32_t lg[HB], tg[HB], sg[HB + 1];
#pragma unroll
                for (int v = 0; v <= HB; ++v) {
                    const int slot = (s + h + v) & (SED_F64_RING - 1);
                    if (v < HB) {
                        dg[v] = rg.d[slot];
                        lg[v] = rg.l[slot];
                        tg[v] = TYPED ? rg.t[slot] : 0u;
                    }
                    if (v > 0) sg[v] = rg.s[slot];  // (sg[0]: in bn already)
                }
#pragma unroll
                for (int v = 0; v < HB; ++v) {
                    const int u = h + v;
                    const int j = s + u - lane + 1;
                    const bool active = (j >= 1) && (j <= m);
                    double2 e[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) e[r] = en[r];
                    bsel = bn;
                    if (u + 1 < G) {
                        bn = dpp_shr1(sg[v + 1], bsel);
#pragma unroll
                        for (int r = 0; r < R; ++r) en[r] = tab[rowbase[r] + bn];
                    }
                    f64_step<R, TB, TYPED, MASKED, FULL, 64, true>(D, LK, T, rowbase, tab, dtop_prev, ltop_prev,
                                                                   ttop_prev, dbot, lbot, tbot, bsel, dg[v], lg[v],
                                                                   tg[v], 0u, W, u, prm.ins, prm.del, tins, tdel,
                                                                   active, fo, row0 + 1, j, e);
                    // every lane's bottom cell, lane 63's read back below: a write under lane == 63 put a branch
                    // (exec skip) between every two steps
                    rg.od[u][lane] = dbot;
                    rg.ol[u][lane] = lbot;
                    if (TYPED) rg.ot[u][lane] = tbot;
                    __builtin_amdgcn_sched_barrier(0);  // (the next step's table reads stay a step ahead of their use)
                }
                handoff(s + h, h);
            }
        };
        if ((s >= 63) && (s + G - 1 < m))
            group(BoolTag<false>{});
        else
            group(BoolTag<true>{});
        if constexpr (TB) store_tb(tbk + ((uint64_t)(s / G) * 64u + lane) * 4u, W);
    }
    if (last) {
        const int w = (n - 1) % ROWS;
        if (lane == w / R) {
            const int rf = w % R;
            double dv = 0.0;
            uint32_t lv = 0, tv = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                dv = (r == rf) ? D[r] : dv;
                lv = (r == rf) ? LK[r] : lv;
                tv = (r == rf) ? T[r] : tv;
            }
            res[pair].dist = dv;
            res[pair].len = n + m - (int32_t)((SED_F64_LB - lv) >> 2);
            res[pair].is_int = TYPED ? (uint8_t)tv : (uint8_t)(dv == 0.0);
            res[pair].err = ok ? 0 : SED_ERR_SPLIT_TIMEOUT;  // a timed-out wait anywhere up the chain poisons the pair
        }
    }
}

template <int R, bool TB, bool TYPED, bool FULL = false, int SW = 64>
static hipError_t launch_f64_R(const sed_launch &L, const double *gtab, const sed_f64_params &prm,
                               const sed_full_out &fo = sed_full_out{}, const int32_t *idx = nullptr, int nidx = 0) {
    const int items = SW == 64 ? L.npairs : nidx;
    const int grid = (items * SW + 255) / 256;
    if (items <= 0) return hipSuccess;
    SED_LAUNCH((sed_wf_f64_kernel<R, TB, TYPED, FULL, SW>), dim3(grid), dim3(256), 0, L, L.pd, items,
                       (const uint8_t *)L.seqa, (const uint8_t *)L.seqb, L.tb, L.bnd, L.res, gtab, prm, fo, idx);
    return hipGetLastError();
}

// SPLIT (L.ntasks > 0): one 128-thread workgroup per (pair, stripe) task, R = 2 (the default) or 4
template <bool TB, bool TYPED, bool FULL = false>
static hipError_t launch_f64_split(const sed_launch &L, const double *gtab, const sed_f64_params &prm,
                                   const sed_full_out &fo = sed_full_out{}) {
    return sed_for_R<2, 4>(L.R, [&](auto r) {
        SED_LAUNCH((sed_wf_f64_split_kernel<decltype(r)::value, TB, TYPED, FULL>), dim3(L.ntasks), dim3(128), 0, L, L.pd,
                   L.tasks, (const uint8_t *)L.seqa, (const uint8_t *)L.seqb, L.tb, L.bnd, L.res, gtab, prm, fo);
        return hipGetLastError();
    });
}

hipError_t sed_launch_f64_full(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed,
                               const sed_full_out &fo) {
    if (L.tb || (L.ntasks > 0 ? (L.R != 2 && L.R != 4) : L.R != 4)) return hipErrorInvalidValue;
    if (L.ntasks > 0)
        return typed ? launch_f64_split<false, true, true>(L, gtab, prm, fo)
                     : launch_f64_split<false, false, true>(L, gtab, prm, fo);
    return typed ? launch_f64_R<4, false, true, true>(L, gtab, prm, fo)
                 : launch_f64_R<4, false, false, true>(L, gtab, prm, fo);
}

hipError_t sed_launch_f64(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed) {
    const bool tb = L.tb != nullptr;
    if (L.ntasks > 0) {
        if (typed) return tb ? launch_f64_split<true, true>(L, gtab, prm) : launch_f64_split<false, true>(L, gtab, prm);
        return tb ? launch_f64_split<true, false>(L, gtab, prm) : launch_f64_split<false, false>(L, gtab, prm);
    }
    // (R = 16: 206 VGPRs, 2 waves per SIMD, iupac 5.22-5.25 against 5.04-5.06 ms at R = 8)
    return sed_for_R<4, 8>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (typed) return tb ? launch_f64_R<R, true, true>(L, gtab, prm) : launch_f64_R<R, false, true>(L, gtab, prm);
        return tb ? launch_f64_R<R, true, false>(L, gtab, prm) : launch_f64_R<R, false, false>(L, gtab, prm);
    });
}

hipError_t sed_launch_f64_seg(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed,
                              const int32_t *idx, int nidx) {
    const bool tb = L.tb != nullptr;
    const sed_full_out none{};
    return sed_for_R<4, 8>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (typed) return tb ? launch_f64_R<R, true, true, false, 16>(L, gtab, prm, none, idx, nidx)
                             : launch_f64_R<R, false, true, false, 16>(L, gtab, prm, none, idx, nidx);
        return tb ? launch_f64_R<R, true, false, false, 16>(L, gtab, prm, none, idx, nidx)
                  : launch_f64_R<R, false, false, false, 16>(L, gtab, prm, none, idx, nidx);
    });
}
