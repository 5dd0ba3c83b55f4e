// sed_tb.hip — the tracebacks over per-cell codes (the codes of the integer TB kernels in sed_kernels.hip and of the
// fp64 kernels in sed_f64.hip): one lane per pair, the wave-uniform window walk, the stripe-parallel band map / compose /
// emit kernels, and sed_ck_codes_kernel, which fills the code layout from a SPLIT forward's checkpoints; then their
// launchers.  (The checkpoint traceback itself is sed_cktb.hip.)
#include <hip/hip_ext.h>
#include "sed_ck_tile.h"

// ---------------------------------------------------------------------------
// Traceback: one lane per pair walks the 2-bit choices from (n, m) to (0, 0)
// and writes the op codes origin->sink, 16 per word.  Position bookkeeping is
// incremental (stripe k, lane t, row r, step s) with power-of-two R, and the
// 16-byte aligned block of codes last read is kept in registers: a diagonal
// run stays in it for up to four steps.
// ---------------------------------------------------------------------------
// SW = 16: the fp64 kernel's segment pairs (idx[0 .. npairs)), whose codes have the stripe layout of 16 lanes; SW = 64
// skips them (d.pad[1]).
// issue priority of the per-cell-code traceback's waves on integer (ladder-code) batches (SED_TB_PRIO, s_setprio):
// pipelined batches run the traceback of run k beside the DP of run k+1, and at priority 1 it no longer trails it.
// Config 3 (CHAIN): 2.50-2.51 against 2.62-2.72 ms per step at 10 steps (traceback span 0.71 against 1.85-1.95 ms),
// the last run's unoverlapped traceback; 2.38 ms at 20 steps either way.  The fp64 workloads (pat = 0) stay at
// priority 0: iupac 4.89-4.90 against 4.83-4.89 ms (profiles/r05/s16)
#ifndef SED_TB_PRIO
#define SED_TB_PRIO 1
#endif
template <int R, int SW = 64>
__global__ __launch_bounds__(64) void sed_traceback_kernel(const sed_pair_desc *__restrict__ pd, int npairs,
                                                           const uint32_t *__restrict__ tb,
                                                           sed_result *__restrict__ res,
                                                           uint32_t *__restrict__ ops, const uint64_t pat,
                                                           const int32_t *__restrict__ idx) {
    constexpr int G = Grp<R>::G, P = Ladder<R>::P;
    if (SED_TB_PRIO > 0 && pat != 0) __builtin_amdgcn_s_setprio(SED_TB_PRIO);
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= npairs) return;
    const int pair = SW == 64 ? item : idx[item];
    const sed_pair_desc d = pd[pair];
    if (d.lane || (SW == 64 && d.pad[1])) return;  // scripted by sed_lane.hip / by the SW = 16 launch
    const int n = d.n, m = d.m;
    const int SG = (m + SW - 1 + G - 1) / G * G;
    const uint64_t stripe_words = (uint64_t)(SG / G) * (SW * 4u);
    uint32_t *out = ops + d.ops_off;
    const int L0 = res[pair].len;
    int q = L0;  // ops in the script; written from position q-1 down to 0
    int i = n, j = m;
    // the padding past the script first: zeroed after the walk instead, config 3's traceback span is 1.65-1.90 against
    // 0.70-0.76 ms (step 2.60-2.76 against 2.57-2.58 ms; none at all: 2.56-2.57 ms, profiles/r06/pad_ab)
    zero_script_tails_wave(ops, d.ops_off, L0, n, m);
    uint32_t acc = 0, bad = 0;
    auto emit = [&](uint32_t op) {
        if (q <= 0) {  // the walk is longer than the sink's L: never write below the pair's script
            bad = 1;
            return;
        }
        --q;
        acc |= op << (2 * (q & 15));
        if ((q & 15) == 0) {
            out[q >> 4] = acc;
            acc = 0;
        }
    };
    if (i > 0 && j > 0) {
        const int rr = i - 1;
        int k = rr / (SW * R);
        int t = (rr >> __builtin_ctz(R)) & (SW - 1);
        int r = rr & (R - 1);
        const uint32_t *base = tb + d.tb_off + (uint64_t)k * stripe_words;
        uint64_t cached = ~0ull;
        uint4 cw = make_uint4(0, 0, 0, 0);
        while (true) {
            const int s = j - 1 + t;
            const int c = (s % G) * R + r;  // code index inside the lane's 16-byte group block
            const uint64_t blk = ((uint64_t)(s / G) * SW + t) * 4u;
            if (blk != cached) {
                cached = blk;
                cw = *reinterpret_cast<const uint4 *>(base + blk);
            }
            const int wsel = c >> 4;
            const uint32_t wv = (wsel & 2) ? ((wsel & 1) ? cw.w : cw.z) : ((wsel & 1) ? cw.y : cw.x);
            // integer codes are (rung(i) + op) & 3 (pat = the ladder), fp64 codes op (pat = 0)
            const uint32_t op = ((wv >> (2 * (c & 15))) - (uint32_t)(pat >> (4 * (i & (P - 1))))) & 3u;
            emit(op);
            if (op != 1) --j;
            if (op != 0) {  // move up one row
                --i;
                if (--r < 0) {
                    r = R - 1;
                    if (--t < 0) {
                        t = SW - 1;
                        --k;
                        base -= stripe_words;
                        cached = ~0ull;
                    }
                }
            }
            if (i == 0 || j == 0) break;
        }
    }
    while (j > 0) { emit(0u); --j; }
    while (i > 0) { emit(1u); --i; }
    if (bad || q != 0) res[pair].err = SED_ERR_TB_LENGTH;
}


// Few pairs (config 2, the GUI): one pair per wave, the walk itself wave-uniform (scalar unit),
// and the wave's 64 lanes fetch a window of 64 code blocks at once.  A lone walk is bound by the
// latency of its dependent block loads (a new 16-byte block every ~R steps of a diagonal path);
// the window covers NT = G lanes x NS = R step-groups, i.e. the next ~50-64 steps of any path
// direction, so one load latency serves them all.  Blocks move from the window's VGPRs to SGPRs
// with v_readlane when the walk enters them.
// The window walk of one pair from cell (i, j), emitting script positions q-1 down, until it reaches row istop
// (0: the origin, with the trailing border runs).  SEG: one segment of the stripe-parallel traceback, whose
// script words go through atomicOr (the buffer is zeroed; the first and last words are shared with the
// neighbouring segments), the last partial word included.  Returns the final q.
template <int R, bool SEG>
__device__ __forceinline__ uint32_t window_walk(const sed_pair_desc &d, int i, int j, const int istop, uint32_t q,
                                                const int lane, const uint32_t *__restrict__ tb,
                                                uint32_t *__restrict__ out, const uint64_t pat, uint32_t &bad) {
    constexpr int G = Grp<R>::G, NT = G, NS = R;  // NT * NS = 64 blocks
    constexpr int P = Ladder<R>::P;
    constexpr int LR = R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : R == 16 ? 4 : 5, LG = 6 - LR;
    static_assert((1 << LR) == R, "R must be a power of two in 2..32");
    const int m = d.m;
    const int SG = (m + 63 + G - 1) / G * G;
    const uint64_t stripe_words = (uint64_t)(SG / G) * 256u;
    // ops are emitted sink -> origin, i.e. from position q-1 down; acc = acc<<2 | op leaves the op of
    // position q in bits 1:0 and position q+p in bits 2p+1:2p when a word [q, q+16) completes
    uint32_t acc = 0;
    auto emit = [&](uint32_t op) {
        if (q == 0) {  // longer than the sink's L (integer flag: a wave-uniform walk)
            bad = 1;
            return;
        }
        acc = (acc << 2) | op;
        if ((--q & 15u) == 0) {
            if constexpr (SEG) {
                if (lane == 0) atomicOr(out + (q >> 4), acc);
            } else {
                out[q >> 4] = acc;  // every lane stores the same word (no exec switching)
            }
        }
    };
    if (i > istop && j > 0) {
        const int rr = i - 1;
        int k = rr >> (6 + LR);
        int t = (rr >> LR) & 63;
        uint32_t r = (uint32_t)rr & (R - 1);
        int s = j - 1 + t;  // the step at which lane t computed column j
        const uint32_t *base = tb + d.tb_off + (uint64_t)k * stripe_words;
        int wt = -1, wsg = -1;  // window corner (highest lane, highest step-group); -1: none loaded
        uint4 wv = make_uint4(0, 0, 0, 0);
        uint64_t lo = 0, hi = 0;  // codes 0..31 and 32..63 of the block being walked
        uint32_t fresh = 1;  // integer flags throughout: bools of uniform values round-trip through VALU masks
        while (true) {
            if (fresh) {  // entered another block: from the window, reloading it first if needed
                const int sg = s >> LG;
                if (!(t <= wt && t > wt - NT && sg <= wsg && sg > wsg - NS)) {
                    wt = t;
                    wsg = sg;
                    const int lt = t - lane / NS, ls = sg - lane % NS;
                    wv = (lt >= 0 && ls >= 0) ? *reinterpret_cast<const uint4 *>(base + ((uint64_t)ls * 64u + lt) * 4u)
                                              : make_uint4(0, 0, 0, 0);
                }
                const int L = (wt - t) * NS + (wsg - sg);
                lo = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(wv.x, L) |
                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(wv.y, L) << 32);
                hi = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(wv.z, L) |
                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(wv.w, L) << 32);
            }
            const uint32_t c = ((uint32_t)(s & (G - 1)) << LR) | r;  // code index inside the block
            const uint32_t op =  // minus the ladder rung of row i (sed_traceback_kernel)
                ((uint32_t)(((c & 32u) ? hi : lo) >> (2u * c & 63u)) - (uint32_t)(pat >> (4 * (i & (P - 1))))) & 3u;
            emit(op);
            const uint32_t di = (op + 1u) >> 1, dj = (5u >> op) & 1u;  // row move (del, upd), column move (ins, upd)
            i -= (int)di;
            j -= (int)dj;
            if (i == istop || j == 0) break;
            const uint32_t wrap = di & ((r - 1u) >> 31);  // moved up out of the lane's rows (r was 0)
            r = (r - di) & (R - 1);
            const int s_old = s;
            s -= (int)(dj + wrap);
            fresh = wrap | ((uint32_t)(s ^ s_old) >> LG);
            if (wrap) {
                if (--t < 0) {  // the stripe above
                    t = 63;
                    --k;
                    base -= stripe_words;
                    s = j - 1 + t;
                    wt = -1;
                }
            }
        }
    }
    if (istop == 0) {
        while (j > 0) { emit(0u); --j; }
        while (i > 0) { emit(1u); --i; }
    } else {
        while (i > istop) { emit(1u); --i; }  // the column-0 border inside the segment
    }
    if constexpr (SEG) {
        if ((q & 15u) != 0 && lane == 0) atomicOr(out + (q >> 4), acc << (2u * (q & 15u)));  // last partial word
    }
    return q;
}

template <int R>
__global__ __launch_bounds__(64) void sed_traceback_window_kernel(const sed_pair_desc *__restrict__ pd,
                                                                  int npairs, const uint32_t *__restrict__ tb,
                                                                  sed_result *__restrict__ res,
                                                                  uint32_t *__restrict__ ops, const uint64_t pat) {
    const int lane = threadIdx.x;
    const int pair = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (pair >= npairs) return;
    const sed_pair_desc d = pd[pair];
    if (d.lane) return;  // scripted by sed_lane.hip
    const uint32_t q0 = (uint32_t)__builtin_amdgcn_readfirstlane(res[pair].len);
    uint32_t bad = 0;
    zero_script_tail(ops + d.ops_off, (int)q0, d.n, d.m, lane, 64);  // (before the walk, as sed_traceback_kernel)
    const uint32_t q = window_walk<R, false>(d, d.n, d.m, 0, q0, lane, tb, ops + d.ops_off, pat, bad);
    if ((bad | q) && lane == 0) res[pair].err = SED_ERR_TB_LENGTH;
}


// ---------------------------------------------------------------------------
// Stripe-parallel traceback for few pairs (per-cell codes; config 2, the GUI: one 4096^2 pair, SPLIT at
// R = 4, 16 stripes).  The window walk above is one dependent chain of ~4200 steps.  Instead:
//   band map kernel: one lane per (64-row band g, column x): walk the codes from cell (last row of band g, x)
//     until the path steps into band g-1; record that column and the ops taken.  A path through a cell continues
//     the same way whatever led to it (each code is the cell's canonical op), so these maps compose;
//   compose kernel: one thread per (stripe k in 1 .. K-2, column x) chains the stripe's R bands into a stripe
//     map entry, and one more thread the sink's stripe from the sink;
//   band emit kernel: one wave per (pair, band): compose the stripe maps from the sink down to its stripe and
//     that stripe's band maps down to its band (its entry column and the script positions of its segment), then
//     walk that segment with the window walk, storing script words with atomicOr (the two words a segment shares
//     with its neighbours; the buffer is zeroed).
// ---------------------------------------------------------------------------
template <int R> struct CodeCursor {  // per-lane reader of one pair's per-cell codes, one 16-byte block cached
    static constexpr int G = Grp<R>::G, LR = R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : R == 16 ? 4 : 5, LG = 6 - LR;
    static constexpr int P = Ladder<R>::P;
    const uint32_t *base;
    uint64_t stripe_words;
    uint4 blk;
    uint64_t key;
    __device__ CodeCursor(const uint32_t *b, uint64_t sw) : base(b), stripe_words(sw), blk(make_uint4(0, 0, 0, 0)), key(~0ull) {}
    // canonical op (0 insert, 1 delete, 2 update) of cell (i, j), 1 <= i, 1 <= j
    __device__ __forceinline__ uint32_t op(int i, int j, uint64_t pat) {
        const int rr = i - 1, k = rr >> (6 + LR), t = (rr >> LR) & 63, r = rr & (R - 1);
        const int s = j - 1 + t;  // the step at which lane t computed column j
        const uint64_t kk = ((uint64_t)k << 40) | ((uint64_t)(s >> LG) << 6) | (uint64_t)t;
        if (kk != key) {
            key = kk;
            blk = *reinterpret_cast<const uint4 *>(base + (uint64_t)k * stripe_words + ((uint64_t)(s >> LG) * 64u + t) * 4u);
        }
        const uint32_t c = ((uint32_t)(s & (G - 1)) << LR) | (uint32_t)r;
        const uint32_t w = (c & 32u) ? ((c & 16u) ? blk.w : blk.z) : ((c & 16u) ? blk.y : blk.x);
        return ((w >> (2u * (c & 15u))) - (uint32_t)(pat >> (4 * (i & (P - 1))))) & 3u;
    }
};

// The map of a pair, at pd.map_off, in {exit column, ops} entries of two words: the stripe map, entry k * (m + 1) + x
// for stripes 1 .. K-2 and the sink's stripe at x = 0 (K (m + 1) entries), then the band maps, entry
// (g - 1) * (m + 1) + x for bands 1 .. nbt-1 (band g: rows 64g + 1 .. 64g + 64; stripe 0's upper bands too, for the
// band emit): the exit column at row 64g, walked from the band's last row, or from row n in the last band.
// A band map workgroup takes 256 consecutive columns x0 .. x0+255 of one band.  Paths near the diagonal stay within
// SED_TBMAP_LEFT (R = 2: SED_TBMAP_LEFT_R2) columns left of x0: the band's 64/R forward lanes of the code groups of
// those steps (layout [group][64 lanes][16 B]) are copied to LDS once, so a step reads LDS instead of waiting on a
// global load (a wave's lanes need new blocks at different steps: with global loads nearly every step waited on
// one).  A path that leaves the staged steps (cells far from the diagonal insert first, since ties prefer insert,
// and can run along the row for thousands of columns) stops: its entry is marked unknown (exit 0xFFFFFFFF) and the
// emit kernel walks that band itself if the real path needs it.  Every workgroup also zeroes its share of the
// pair's script words, which the emit kernel's segments OR into (lane-kernel pairs wrote theirs already).
// One lane per band, not per stripe: a whole stripe is a chain of up to ~700 dependent LDS steps at about one wave
// per SIMD (config 2: 104 us); the bands are R times the lanes at 1/R the chain and 1/R the LDS per workgroup, so
// many workgroups share a CU.
#ifndef SED_TBMAP_LEFT
#define SED_TBMAP_LEFT 512
#endif
// R = 2 (the fp64 SPLIT route's 128-row stripes): a path crosses its stripe within fewer columns, and the map's time is
// its longest walks (lanes far from the path, running left through the staged columns): 1000^2 per call 400 -> 360 us,
// 2000^2 629 -> 587 us at 192 (tools/script_calls.py, profiles/r05/s47); the 256-row stripes of config 2 keep 512
// (at 192 its path needed columns past the staged ones, and the emit kernel's fallback walks took 187 against 53 us)
// With the band maps (64-row walks) 128 staged columns serve R = 2 better still: 1000^2 343 -> 335 us, 2000^2 572 -> 563 us
// per call (96: 335 / 562; profiles/r05/s57)
#ifndef SED_TBMAP_LEFT_R2
#define SED_TBMAP_LEFT_R2 128
#endif
#ifndef SED_TBMAP_RUN
#define SED_TBMAP_RUN 96
#endif
// Band-map walks stop (entry unknown, left to the emit kernel's fallback walk) after 64 + 64 ceil(m / n) steps: the
// canonical path crosses a 64-row band in 64 steps plus its inserts, while a wave's time is its longest lane, and the
// lanes far from the path run left for 200-340 steps (config 2's pair: median walk 65 steps, 99th percentile 283,
// tools/tbmap_walks.py).  SED_TBMAP_CAP: the base (96: map 36.3 against 33.9 us at R = 4, 32.7 against 26.8 at R = 2,
// profiles/r06/tbmap_cap/step23); 0: no step limit (A/B)
#ifndef SED_TBMAP_CAP
#define SED_TBMAP_CAP 64
#endif
template <int R>
__global__ __launch_bounds__(256) void sed_tb_bandmap_kernel(const sed_pair_desc *__restrict__ pd,
                                                             const uint32_t *__restrict__ tb,
                                                             uint32_t *__restrict__ map,
                                                             uint32_t *__restrict__ ops, const uint64_t pat) {
    constexpr int ROWS = 64 * R, NB = R, NL = 64 / R, G = Grp<R>::G, LG = CodeCursor<R>::LG, LR = CodeCursor<R>::LR;
    constexpr int P = Ladder<R>::P;
    constexpr int LEFT = R == 2 ? SED_TBMAP_LEFT_R2 : SED_TBMAP_LEFT;
    constexpr int NSG = (LEFT + 256 + 64 + 2 * G) / G + 1;  // staged step groups
    constexpr int NIT = (NSG * NL + 255) / 256;  // staging trips of the 256 threads
    __shared__ uint4 stage[NIT * 256];
    const __attribute__((address_space(3))) uint32_t *stage32 =
        (const __attribute__((address_space(3))) uint32_t *)(stage);
    const int p = blockIdx.y;
    const sed_pair_desc d = pd[p];
    const int n = d.n, m = d.m;
    if (d.lane) return;
    const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid;
    if (idx < (n + m + 15) / 16) ops[d.ops_off + idx] = 0u;
    if (n == 0 || m == 0) return;
    const int K = (n + ROWS - 1) / ROWS;
    if (K < 3) return;  // walked whole by the emit kernel
    const int nx = m + 1, nxc = (nx + 255) / 256, nbt = (n + 63) / 64;  // bands 1 .. nbt-1 are mapped
    const int blk = blockIdx.x;
    if (blk >= (nbt - 1) * nxc) return;
    const int g = 1 + blk / nxc, x0 = (blk % nxc) * 256;
    const int k = g / NB, t0 = (g % NB) * NL;  // the band's stripe and first forward lane
    const int SG = (m + 63 + G - 1) / G * G;
    const uint64_t stripe_words = (uint64_t)(SG / G) * 256u;
    int j = x0 + tid, i = min(64 * (g + 1), n);
    const bool live = j <= m;
    // stage the band's lanes of the groups of steps s = j' - 1 + t, j' in [x0 - LEFT, x0 + 255], t in [0, 63]
    const uint32_t *tbk = tb + d.tb_off + (uint64_t)k * stripe_words;
    const int s_lo = max(0, x0 - LEFT - 1), s_hi = min(SG - 1, x0 + 255 + 63);
    const int sg_lo = s_lo >> LG, nsg = min(NSG, (s_hi >> LG) - sg_lo + 1);
    const uint4 *src = reinterpret_cast<const uint4 *>(tbk) + (uint64_t)sg_lo * 64u + t0;
    {  // fixed trip count, unguarded stores (clamped loads fill the tail): every load is in flight before the first
       // wait (guarded stores split the blocks, and the copy ran load, wait, store per trip)
        uint4 v[NIT];
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int e = tid + 256 * u;
            v[u] = src[e < nsg * NL ? (e / NL) * 64 + (e % NL) : 0];
        }
#pragma unroll
        for (int u = 0; u < NIT; ++u) stage[tid + 256 * u] = v[u];
    }
    __syncthreads();
    if (!live) return;
    const int top = 64 * g;  // row top belongs to band g - 1
    uint32_t cnt = 0, run = 0;  // run: consecutive inserts
    const uint32_t cap = SED_TBMAP_CAP ? (uint32_t)SED_TBMAP_CAP + 64u * (uint32_t)((m + n - 1) / n) : 0xFFFFFFFFu;
    for (;;) {  // one exit per step (separate exits became nested exec-mask regions); reason decided after
        const int rr = i - 1, t = (rr >> LR) & 63, r = rr & (R - 1);
        const int s = j - 1 + t;
        const uint32_t c = ((uint32_t)(s & (G - 1)) << LR) | (uint32_t)r;
        // one unconditional ds_read_b32 per step (an LDS-qualified pointer: a generic one became a flat load, and
        // a uint4 read was split into two branch-guarded halves)
        const uint32_t rel = (uint32_t)((s >> LG) - sg_lo);
        const bool inside = rel < (uint32_t)nsg;
        // (t - t0) & (NL - 1): the read after the exit row (t outside the band) stays inside the staged lanes
        const uint32_t word = stage32[(inside ? rel : 0u) * (NL * 4u) + ((uint32_t)(t - t0) & (NL - 1u)) * 4u + (c >> 4)];
        if (!((i > top) & (j > 0) & inside & (run <= SED_TBMAP_RUN) & (cnt < cap))) break;
        const uint32_t op = ((word >> (2u * (c & 15u))) - (uint32_t)(pat >> (4 * (i & (P - 1))))) & 3u;
        ++cnt;
        run = op == 0u ? run + 1u : 0u;
        i -= (int)(op != 0u);
        j -= (int)(op != 1u);
    }
    if (i > top) {
        if (j == 0) {  // the column-0 border: deletes up to the band above
            cnt += (uint32_t)(i - top);
        } else {  // left of the staged steps, a long run of inserts (a cell far from the diagonal) or past the step
            j = -1;  // limit: unknown, walked by the emit kernel if the real path needs it
            cnt = 0;
        }
    }
    uint32_t *mp = map + (uint32_t)d.map_off + 2u * ((uint32_t)K * (uint32_t)nx + (uint32_t)(g - 1) * (uint32_t)nx + (uint32_t)(x0 + tid));
    mp[0] = (uint32_t)j;
    mp[1] = cnt;
}

// The stripe map from the band maps: one thread per (stripe k in 1 .. K-2, column x), chaining the stripe's NB
// bands from its last row, and one for the sink's stripe, from the sink (stored at x = 0).  Unknown if any band on
// the chain is.
template <int R>
__global__ __launch_bounds__(256) void sed_tb_bandcompose_kernel(const sed_pair_desc *__restrict__ pd,
                                                                 uint32_t *__restrict__ map) {
    constexpr int ROWS = 64 * R, NB = R;
    const int p = blockIdx.y;
    const sed_pair_desc d = pd[p];
    const int n = d.n, m = d.m;
    if (d.lane || n == 0 || m == 0) return;
    const int K = (n + ROWS - 1) / ROWS;
    if (K < 3) return;
    const int nx = m + 1, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx > (K - 2) * nx) return;
    int k, g, x;
    uint32_t slot;
    if (idx == (K - 2) * nx) {  // the sink: from (n, m) in the band holding row n
        k = K - 1;
        g = (n - 1) / 64;
        x = m;
        slot = (uint32_t)k * nx;
    } else {
        k = 1 + idx / nx;
        x = idx % nx;
        g = (k + 1) * NB - 1;
        slot = (uint32_t)k * nx + x;
    }
    uint32_t *mp = map + (uint32_t)d.map_off;
    const uint32_t *bm = mp + 2u * (uint32_t)K * nx;
    uint32_t cnt = 0;
    for (; g >= k * NB; --g) {
        const uint32_t e = 2u * ((uint32_t)(g - 1) * nx + (uint32_t)x);
        const uint32_t xn = bm[e];
        if (xn == 0xFFFFFFFFu) {
            x = -1;
            cnt = 0;
            break;
        }
        cnt += bm[e + 1u];
        x = (int)xn;
    }
    mp[2u * slot] = (uint32_t)x;
    mp[2u * slot + 1u] = cnt;
}

// The exit column and op count of stripe k's segment from cell (i, j), walked here (entries the maps left
// unknown); wave-uniform, codes read one word per step
template <int R>
__device__ __forceinline__ uint2 ck_count_walk(const sed_pair_desc &d, const uint32_t *__restrict__ tb, const uint64_t pat,
                                               const int k, int i, int j, int top = -1) {
    constexpr int ROWS = 64 * R, G = Grp<R>::G, LG = CodeCursor<R>::LG, LR = CodeCursor<R>::LR, P = Ladder<R>::P;
    const int SG = (d.m + 63 + G - 1) / G * G;
    const uint32_t *tbk = tb + d.tb_off + (uint64_t)k * (uint64_t)(SG / G) * 256u;
    if (top < 0) top = k * ROWS;  // (else a band's top row inside stripe k)
    uint32_t cnt = 0;
    while (i > top) {
        if (j == 0) {
            cnt += (uint32_t)(i - top);
            break;
        }
        const int rr = i - 1, t = (rr >> LR) & 63, r = rr & (R - 1);
        const int s = j - 1 + t;
        const uint32_t c = ((uint32_t)(s & (G - 1)) << LR) | (uint32_t)r;
        const uint32_t word = tbk[((uint64_t)(s >> LG) * 64u + t) * 4u + (c >> 4)];
        const uint32_t op = ((word >> (2u * (c & 15u))) - (uint32_t)(pat >> (4 * (i & (P - 1))))) & 3u;
        ++cnt;
        i -= (int)(op != 0u);
        j -= (int)(op != 1u);
    }
    return make_uint2((uint32_t)j, cnt);
}

// The emit: one wave per (pair, 64-row band) walks its band's segment of the canonical path (a wave per stripe
// walked R times as far).  The wave composes the stripe maps from the sink down to its band's stripe, then that
// stripe's band maps down to its band (entries the maps left unknown are walked here, ck_count_walk), and walks its
// segment to the band's top row (band 0: to the origin) with the window walk, ORing its script words into the zeroed
// buffer.
template <int R>
__global__ __launch_bounds__(64) void sed_tb_bandemit_kernel(const sed_pair_desc *__restrict__ pd,
                                                             const uint32_t *__restrict__ tb,
                                                             sed_result *__restrict__ res,
                                                             uint32_t *__restrict__ ops,
                                                             const uint32_t *__restrict__ map, const uint64_t pat) {
    constexpr int ROWS = 64 * R, NB = R;
    const int lane = threadIdx.x;
    const int pair = __builtin_amdgcn_readfirstlane(blockIdx.x), gme = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const sed_pair_desc d = pd[pair];
    if (d.lane) return;
    const int n = d.n, m = d.m;
    const int K = n > 0 ? (n + ROWS - 1) / ROWS : 1;
    const bool multi = K >= 3 && m > 0;  // pairs of one or two stripes: one segment, the whole walk (band 0's wave)
    const int nbt = multi ? (n + 63) / 64 : 1;
    if (gme >= nbt) return;
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane(res[pair].len);
    int i0 = n, j0 = m;
    uint32_t qhi = L, cnt = L;  // cnt: the ops of this segment
    if (multi) {
        const uint32_t nx = (uint32_t)m + 1u;
        const uint32_t *mp = map + (uint32_t)d.map_off;
        const uint32_t *bm = mp + 2u * (uint32_t)K * nx;
        const int kme = gme / NB;
        uint32_t x = (uint32_t)m;
        for (int kk = K - 1; kk > kme; --kk) {  // whole stripes above this band's: from the sink's
            const uint32_t e = kk == K - 1 ? 2u * ((uint32_t)(K - 1) * nx) : 2u * ((uint32_t)kk * nx + x);
            uint32_t xn = mp[e], c = mp[e + 1u];
            if (xn == 0xFFFFFFFFu) {
                const uint2 w = ck_count_walk<R>(d, tb, pat, kk, i0, (int)x);
                xn = w.x;
                c = w.y;
            }
            qhi -= c;
            x = xn;
            i0 = kk * ROWS;
        }
        for (int g = (i0 - 1) / 64; g >= gme; --g) {  // bands of this stripe from its entry: the last one is this band's
            uint32_t xn, c;
            if (g == 0) {  // band 0: to the origin, whatever is left
                xn = 0u;
                c = qhi;
            } else {
                const uint32_t e = 2u * ((uint32_t)(g - 1) * nx + x);
                xn = bm[e];
                c = bm[e + 1u];
                if (xn == 0xFFFFFFFFu) {
                    const uint2 w = ck_count_walk<R>(d, tb, pat, kme, i0, (int)x, 64 * g);
                    xn = w.x;
                    c = w.y;
                }
            }
            if (g == gme) {
                cnt = c;
                break;
            }
            qhi -= c;
            x = xn;
            i0 = 64 * g;
        }
        j0 = (int)x;
    }
    const int istop = multi ? 64 * gme : 0;
    uint32_t bad = 0;
    const uint32_t q = window_walk<R, true>(d, i0, j0, istop, qhi, lane, tb, ops + d.ops_off, pat, bad);
    if ((bad || q != qhi - cnt) && lane == 0) res[pair].err = SED_ERR_TB_LENGTH;
}

// ---------------------------------------------------------------------------
// SPLIT batches with checkpoints (config 2, GUI pairs; sed_runtime.cpp: split_ck).  The SPLIT forward kernel runs the
// distance (or dot) keys, 2-3 VALU per cell instead of the ladder keys' 5.2, and stores checkpoints after the pair's
// per-cell code region; this kernel then recomputes every 64 x 64 tile from them at once (one wave per tile, the
// traceback's whole-tile sweep) and writes the tile's canonical op codes in the per-cell code layout of the TB kernels
// (store_tb: per stripe and G-step group, 4 words per forward lane, code (step u, row rr) at bits 2 (u R + rr)), which
// the stripe-parallel traceback walks (as plain ops: the ladder keys' per-row code offsets are not applied, L.tb_ladder).
// Every tile is written, those below row n too, so the walks only ever read codes of a DP.  R = 4 (G = 16): tile lane r = 4 b + rr is forward lane G Q + b's row rr; its
// codes of the chunk's forward steps 64 c .. 64 c + 63 sit at sweep steps G - 1 + 3 b + rr onwards.
__device__ __forceinline__ uint32_t ck_codes_transpose(uint32_t y) {
    // 4 x 4 transpose of 2-bit elements, byte = row: (row rr, element u) -> (row u, element rr)
    uint32_t t = ((y >> 6) ^ y) & 0x00CC00CCu;
    y ^= t ^ (t << 6);
    t = ((y >> 12) ^ y) & 0x0000F0F0u;
    return y ^ t ^ (t << 12);
}
template <int R>
__global__ __launch_bounds__(64) void sed_ck_codes_kernel(const sed_pair_desc *__restrict__ pd,
                                                          const uint32_t *__restrict__ seqa,
                                                          const uint32_t *__restrict__ seqb, uint32_t *__restrict__ tb,
                                                          sed_i32_params prm) {
    static_assert(R == 4, "the code layout transposition is written for R = 4");
    constexpr int ROWS = 64 * R, G = Grp<R>::G;
    const int lane = threadIdx.x;
    const sed_pair_desc d = pd[blockIdx.y];
    if (d.lane || d.n == 0 || d.m == 0) return;
    const int n = d.n, m = d.m;
    const int nstripes = (n + ROWS - 1) / ROWS, SG = (m + 63 + G - 1) / G * G, nchunks = (SG + 63) >> 6;
    const int tile = (int)blockIdx.x;  // (k R + Q) nchunks + c
    if (tile >= nstripes * R * nchunks) return;
    const int c = tile % nchunks, kq = tile / nchunks, Q = kq % R, k = kq / R;
    const uint64_t codew = (uint64_t)nstripes * (uint64_t)(SG / G) * 256u;  // the pair's per-cell code words
    __shared__ uint32_t topb[SED_CK_NX(8)], selb[SED_CK_SELB(8)], wl[64 * 9], win[64 * 5];
    const CkPairCtx px = ck_pair_ctx<R>(d, lane, seqa, seqb, tb, codew);
    uint32_t one = 1u;
    asm volatile("" : "+v"(one));
    uint32_t W[8], vinit = 0;
    (void)ck_tile_sweep<R, false, true, 8>(px, lane, prm, topb, selb, k, Q, c, 127, one, W, vinit);
    // this lane's window: 64 codes from sweep step s0 (bit 2 s0 of W[0..7])
    const int b = lane >> 2, rr = lane & 3;
    const uint32_t s0 = (uint32_t)(G - 1 + (R - 1) * b + rr);
#pragma unroll
    for (int w = 0; w < 8; ++w) wl[lane * 9 + w] = W[w];
    __syncthreads();
    uint32_t x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = wl[lane * 9 + (int)(s0 >> 4) + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) win[lane * 5 + i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], (2u * s0) & 31u);
    __syncthreads();
    // lane = 4 b' + g writes forward lane G Q + b''s group 4 c + g: rows 4 b' .. 4 b' + 3, window word g
    const int bo = lane >> 2, g = lane & 3;
    const int gg = 4 * c + g;
    if (gg >= SG / G) return;  // past the stripe's last group
    uint32_t y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) y[q] = win[(4 * bo + q) * 5 + g];
    uint32_t o[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // word w: steps 4w .. 4w+3 of the group, byte w of each row's window word
        const uint32_t sel = (uint32_t)w * 0x0101u + 0x0400u;  // bytes w of y[0], w of y[1]
        const uint32_t y01 = __builtin_amdgcn_perm(y[1], y[0], sel | 0x0C0C0000u);
        const uint32_t y23 = __builtin_amdgcn_perm(y[3], y[2], sel | 0x0C0C0000u);
        o[w] = ck_codes_transpose(__builtin_amdgcn_perm(y23, y01, 0x05040100u));
    }
    uint32_t *gp = tb + d.tb_off + (uint64_t)k * (uint64_t)(SG / G) * 256u + (uint64_t)gg * 256u + (uint32_t)(G * Q + bo) * 4u;
    *reinterpret_cast<uint4 *>(gp) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------
// Launchers (host side, called from sed_runtime.cpp)
// ---------------------------------------------------------------------------
hipError_t sed_launch_traceback_seg(const sed_launch &L, uint32_t *ops, const int32_t *idx, int nidx) {
    if (nidx <= 0) return hipSuccess;
    const int grid = (nidx + 63) / 64;
    return sed_for_R<4, 8>(L.R, [&](auto r) {
        SED_LAUNCH((sed_traceback_kernel<decltype(r)::value, 16>), dim3(grid), dim3(64), 0, L, L.pd, nidx, L.tb, L.res, ops,
                   0ull, idx);
        return hipGetLastError();
    });
}

hipError_t sed_launch_ck_codes(const sed_launch &L, int max_tiles, const sed_i32_params &prm) {
    if (L.R != 4 || max_tiles <= 0 || L.npairs <= 0) return hipErrorInvalidValue;
    SED_LAUNCH(sed_ck_codes_kernel<4>, dim3(max_tiles, L.npairs), dim3(64), 0, L, L.pd, (const uint32_t *)L.seqa,
               (const uint32_t *)L.seqb, L.tb, prm);
    return hipGetLastError();
}

hipError_t sed_launch_traceback(const sed_launch &L, uint32_t *ops) {
    // up to one pair per CU: a wave-uniform walk per pair over windows of blocks; beyond: one lane per pair
    const bool uni = L.npairs <= 256;
    const int grid = uni ? L.npairs : (L.npairs + 63) / 64;
    return sed_for_R<2, 4, 8, 16, 32>(L.R, [&](auto r) {  // (R = 2: the fp64 SPLIT route's codes)
        constexpr int R = decltype(r)::value;
        const uint64_t pat = L.tb_ladder ? (L.tb_wide ? LadderW<R>::pat : Ladder<R>::pat) : 0ull;
        if (uni)
            SED_LAUNCH((sed_traceback_window_kernel<R>), dim3(grid), dim3(64), 0, L, L.pd, L.npairs, L.tb, L.res, ops, pat);
        else
            SED_LAUNCH((sed_traceback_kernel<R>), dim3(grid), dim3(64), 0, L, L.pd, L.npairs, L.tb, L.res, ops, pat, nullptr);
        return hipGetLastError();
    });
}

// stripe-parallel traceback (few pairs with >= 3 stripes): ops zeroed by the caller; items = the most map lanes
// of a pair ((K-2)(m+1)+1), kmax = the most stripes of a pair
hipError_t sed_launch_traceback_stripes(const sed_launch &L, uint32_t *ops, uint32_t *map, int items, int kmax) {
    // items: map workgroups x 256 of the largest pair, and at least every pair's script words; >= one block
    // (the compose grid: (K-2)(m+1)+1 threads per pair, at most items / 256 / R + 1 blocks, sed_runtime.cpp)
    const dim3 gmap((max(items, 1) + 255) / 256, L.npairs), gemit(L.npairs, max(kmax, 1) * L.R),
        gcomp((max(items, 1) + 255) / 256 / max(L.R, 1) + 1, L.npairs);
    // the runtime takes this route at R = 2 (fp64 SPLIT) and 4 only
    return sed_for_R<2, 4>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        const uint64_t pat = L.tb_ladder ? (L.tb_wide ? LadderW<R>::pat : Ladder<R>::pat) : 0ull;
        hipExtLaunchKernelGGL((sed_tb_bandmap_kernel<R>), gmap, dim3(256), 0, L.stream, L.ev0, nullptr, 0, L.pd, L.tb, map, ops, pat);
        hipLaunchKernelGGL((sed_tb_bandcompose_kernel<R>), gcomp, dim3(256), 0, L.stream, L.pd, map);
        hipExtLaunchKernelGGL((sed_tb_bandemit_kernel<R>), gemit, dim3(64), 0, L.stream, nullptr, L.ev1, 0, L.pd, L.tb, L.res, ops,
                              map, pat);
        return hipGetLastError();
    });
}
