// sed_internal.h — structures shared by the kernels, the planners and the runtime (not part of the C-ABI).  Fit search's
// are in one section ("Fit search" below), read by sed_fit.hip, sed_fit_dp.h, sed_fit_plan.h and sed_fit_runtime.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#define SED_MAX_K 32

// Per-pair descriptor in device memory (64 bytes).
struct sed_pair_desc {
    uint64_t a_off;    // str1: word offset (integer kernel, 2-bit packed) or byte offset (fp64 kernel)
    uint64_t b_off;    // str2: same
    uint64_t tb_off;   // traceback codes: uint32 word offset
    uint64_t bnd_off;  // stripe bottom-row buffer: uint32 word offset
    uint64_t ops_off;  // packed script: uint32 word offset
    int32_t n, m;
    int32_t lane;      // 1: computed by the lane-per-pair kernel (short str2), the wave kernels skip it
    int32_t map_off;   // stripe-parallel traceback: word offset of the pair's stripe exit map
    int32_t pad[2];
};

// Per-pair result (16 bytes).
struct sed_result {
    double dist;     // dp[n][m].value
    int32_t len;     // ops in the canonical script (L at the sink)
    uint8_t is_int;  // 1 when the reference's value is a Python int
    uint8_t err;     // SED_ERR_* (0 = ok); nonzero: the pair's results are invalid
    uint16_t seq;    // CHAIN mode: ordinal of the pair within the wave that computed it (diagnostics)
};

// sed_result.err codes (sed_runtime.cpp: fetch_results maps them to SED_E_DEVICE with the pair index)
#define SED_ERR_SPLIT_TIMEOUT 1  // SPLIT: an inter-workgroup hand-off wait timed out
#define SED_ERR_TB_CHECK 2       // CK traceback: a recomputed tile disagrees with the path length (bad checkpoint)
#define SED_ERR_TB_STALL 3       // traceback: a tile visit made no progress
#define SED_ERR_TB_GUARD 4       // traceback: more tile visits than any path can need
#define SED_ERR_TB_LENGTH 5      // traceback: the walk's op count differs from the sink's L
#define SED_ERR_TB_BAND 6        // CK traceback: the walk left the band the forward computed (band pruning)
#define SED_ERR_FWD_BAND 7       // CK forward: no cell of a stripe's boundary row passed the refinement's slack test

#ifdef __HIPCC__  // (device helpers: the runtime, compiled by g++, does not see them)
// Script padding.  A pair's script region holds ceil((n+m)/16) words; its ops fill ceil(len/16) of them.  Every walk
// starts its op accumulator at 0, so the bits past the last op inside the last op word are 0 already; this zeroes the
// spare words after it (lanes lane, lane + stride, ...), so the packed buffer is a function of the scripts alone,
// whatever the buffer held before (sed.h).  Every script-writing kernel calls it once per pair.
#ifndef SED_PAD_ZERO
#define SED_PAD_ZERO 1  // (0: A/B builds only; the padding is then whatever the buffer held)
#endif
__device__ __forceinline__ void zero_script_tail(uint32_t *__restrict__ out, int len, int n, int m, int lane,
                                                 int stride) {
    if (!SED_PAD_ZERO) return;
    const int end = (n + m + 15) >> 4;
    for (int w = ((len > 0 ? len : 0) + 15) / 16 + lane; w < end; w += stride) out[w] = 0u;
}

// The same for the lane-per-pair walks, where each lane owns a pair: the wave stores every active lane's spare words
// [ceil(len/16), ceil((n+m)/16)) pair by pair as one coalesced run, its active lanes side by side.  (Each lane storing
// its own pair's words one after another scattered every store instruction over 64 pairs: config 3's per-cell-code
// traceback took 1.68-1.91 instead of 0.75 ms, profiles/r06/pad_ab.)  Lanes that left the kernel own no pair here.
__device__ __forceinline__ void zero_script_tails_wave(uint32_t *__restrict__ ops, uint64_t off, int len, int n, int m) {
    if (!SED_PAD_ZERO) return;
    const uint64_t act = __ballot(1);
    const int rank = __popcll(act & ((1ull << (threadIdx.x & 63)) - 1ull)), nact = __popcll(act);
    const int w0 = ((len > 0 ? len : 0) + 15) >> 4, w1 = (n + m + 15) >> 4;
    uint64_t todo = __ballot(w0 < w1);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int a = __builtin_amdgcn_readlane(w0, l), b = __builtin_amdgcn_readlane(w1, l);
        const uint64_t o = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, l) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(off >> 32), l) << 32);
        for (int w = a + rank; w < b; w += nact) ops[o + (uint64_t)w] = 0u;
    }
}
#endif  // __HIPCC__

// Integer kernel constants (offset-key space, see sed_i32_keys.h):
//   costrow[a]   byte b = (cost(a -> b) - insert - delete - 1) & 0xFF  (32-bit keys)
//   costrow16[a] byte b = (cost(a -> b) - insert - delete) & 0xFF      (16-bit packed distance keys)
//   kins = (insert << 16) + 4, kdel = (delete << 16) + 5: the lane kernels' key increments (op included;
//   their offsets per column / row are kins and kdel - 1).  The wave kernels derive their own from ins/del.
#define SED_KB 0xFFFFFFFCu  // bias of the 32-bit distance-only offset keys (sed_i32_keys.h)
#define SED_KB_DOT 0u       // border of the dot keys (every border cell is X = U = 0)
struct sed_i32_params {
    uint32_t costrow[4];
    uint32_t costrow16[4];
    uint32_t kins, kdel;
    uint32_t ins, del;
    uint32_t epoch;  // SPLIT hand-off words' tag: 1..32767 per run (sed_dev.h: store_tagged)
    // Dot keys (checkpoint batches of the stripe kernel, sed_i32_keys.h: i32_step DOT): the update addend
    // A*kappa(a, b) + 1, kappa = insert + delete - cost(a -> b), as a signed byte dot product
    // dot4(dotrow[a], dotcol[b]); keys W = A*X + U (X = sum of kappa on the path, U = its updates), maximised.
    // Decode: X = (k * dotM) >> dotS (= floor(k*kmax / (A*kmax + 1)); dotM includes kmax, dotS >= 32, so the
    // kernels take one v_mul_hi_u32), U = k - A*X.
    uint32_t dot;  // 1: the CK forward kernel runs dot keys, the CK traceback converts them
    uint32_t dotA, dotkmax, dotM, dotS;
    uint32_t dotrow[4], dotcol[4];
    // Ladder dot keys (CHAIN kernel with the L field): V = D*ladA + 8L over the ladder (lad = 1) or D*ladA + 16L over
    // the wide ladder (lad = 2), the update addend of a d = -1 row -(ladA*kappa + 7) (+ 15) = dot4(ladrow[a],
    // ladcol[b]) (sed_i32_keys.h: i32_step LDOT)
    uint32_t lad, ladA, ladsent;
    uint32_t ladrow[4], ladcol[4];
};

struct sed_f64_params {
    double ins, del;
    int32_t ins_int, del_int;
    int32_t K;
    uint32_t epoch;  // SPLIT hand-off words' tag, as sed_i32_params::epoch (sed_f64.hip: sed_wf_f64_split_kernel)
};

// Full-matrix output (dp proxy materialisation): D[i*(m+1)+j], M = edge mask (1 ins, 2 del, 4 upd) | int << 3.
struct sed_full_out {
    double *D;
    uint8_t *M;
    int32_t n, m;
};

// a kernel launch of a sed_launch phase, carrying its events (see sed_launch::ev0 / ev1); the .hip files that
// use it include <hip/hip_ext.h> (the host-compiled runtime does not)
#define SED_LAUNCH(kernel, grid, block, shmem, L, ...) \
    hipExtLaunchKernelGGL(kernel, grid, block, shmem, (L).stream, (L).ev0, (L).ev1, 0, __VA_ARGS__)
// The runtime's rows per lane as a template argument, for every launcher: f(std::integral_constant<int, R>{}) for the R
// of Rs... that equals rows, hipErrorInvalidValue for any other.  A generic f is instantiated for every R of the list and
// no other, so a site's list is the set of kernels it builds.
template <int... Rs, class F> inline hipError_t sed_for_R(int rows, F f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((rows == Rs && ((e = f(std::integral_constant<int, Rs>{})), true)) || ...);
    return e;
}

struct sed_launch {
    const sed_pair_desc *pd;
    int npairs;
    const void *seqa, *seqb;
    uint32_t *tb;   // nullptr -> distance only
    uint32_t *ops;  // packed scripts (lane kernel writes them itself)
    uint32_t *bnd;
    sed_result *res;
    int R;
    hipStream_t stream;
    bool tb_ladder;     // traceback codes of the integer kernels carry the row's ladder rung (sed_i32_keys.h)
    bool tb_wide;       // ... of the wide ladder (ladder dot keys, LadderW: the CHAIN kernel's LDOT batches)
    bool ck;            // integer R = 16 wave kernel: tb holds checkpoints, the traceback recomputes tiles
    // band pruning (checkpoint batches of the stripe kernel): band[pair] = the window of diagonals the forward computes
    // and the traceback assumes, written by sed_band_kernel before every forward with bandp's costs; nullptr = off
    struct sed_band *band;
    const struct sed_band_params *bandp;
    // the windows per stripe: bwin[pair * bstripes + k] = {clo, chi}, the chunks the forward ran of stripe k (it writes
    // them whenever bwin is set; sed_batch_band_chunks_run sums them).  Refined windows (bsuf set): sed_band_kernel
    // writes bsuf[pair * bstripes + k] = suf(k ROWS), the forward narrows every stripe below the first from the row
    // above it (sed_refine_cell) and the traceback reads bwin instead of restating the static range.
    int2 *bwin;
    uint32_t *bsuf;
    int bstripes;
    // timing events carried by the launches themselves (hipExtLaunchKernelGGL: timestamps on the dispatch
    // packet, no marker packet between kernels): the launcher's first kernel records ev0 at its start, its last
    // kernel ev1 at its end; nullptr = none
    hipEvent_t ev0, ev1;
    const int2 *tasks;  // SPLIT mode: (pair, stripe) per workgroup, else nullptr
    int ntasks;         // 0 -> one wave per pair
    // CHAIN mode: chain c runs pairs chain_pairs[chain_off[c] .. chain_off[c+1]) back to back;
    // with chain_counter set, nchains persistent waves take list entries [0, chain_list) from it
    const int32_t *chain_pairs, *chain_off;
    int nchains;
    uint32_t *chain_counter;
    uint32_t chain_base;  // the counter's value when this run starts (it is never reset between runs)
    int chain_list;
};

// len = false (distance only, SED_NO_LEN): keys without the op-count field, out len = -1.
hipError_t sed_launch_i32(const sed_launch &L, const sed_i32_params &prm, bool len);
// CHAIN mode (single-stripe pairs, R in {4, 8, 16}): one wave per chain of pairs.
hipError_t sed_launch_i32_chain(const sed_launch &L, const sed_i32_params &prm, bool len);
hipError_t sed_launch_f64(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed);
// fp64 wave kernel in 16-lane segments, four pairs per wave (pairs idx[0 .. nidx), pd.pad[1] = 1; the SW = 64 kernel and
// traceback skip them), and their per-cell-code traceback
hipError_t sed_launch_f64_seg(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed,
                              const int32_t *idx, int nidx);
hipError_t sed_launch_traceback_seg(const sed_launch &L, uint32_t *ops, const int32_t *idx, int nidx);
hipError_t sed_launch_f64_full(const sed_launch &L, const double *gtab, const sed_f64_params &prm, bool typed,
                               const sed_full_out &fo);
// Lane-per-pair integer kernel (sed_lane.hip): pairs idx[0..nidx) with 1 <= m <= SED_LANE_MAXM.
// len = false: distance only, no op-count field (3 VALU per cell).
#define SED_LANE_MAXM 32
#define SED_LANE_MAXN 512
hipError_t sed_launch_lane_i32(const sed_launch &L, const int32_t *idx, int nidx, const sed_i32_params &prm, bool len);
// distance only, two pairs of equal shape per wave (packed 16-bit cells); list holds 2 * nwaves pair indices
hipError_t sed_launch_i32x2(const sed_launch &L, const int32_t *list, int nwaves, const sed_i32_params &prm);
// distance only, two pairs of equal n per lane (packed 16-bit cells); idx holds 2 * nlanes pair indices
hipError_t sed_launch_lane_i32x2(const sed_launch &L, const int32_t *idx, int nlanes, const sed_i32_params &prm);
// distance only under unit costs, one pair per lane, bit-parallel (str2 as the bit dimension, m <= 32)
hipError_t sed_launch_lane_bitpar(const sed_launch &L, const int32_t *idx, int nidx);
// fp64 distance-only lane kernel (SED_MODE_F64 with SED_NO_LEN): gtab = the {value, flag} table.  Pairs with
// pd.pad[0] = 1 (every symbol in the unit-cost code set umask, at most 4 codes) run bit-parallel.
hipError_t sed_launch_lane_f64(const sed_launch &L, const int32_t *idx, int nidx, const double *gtab, double ins,
                               double del, int K, uint32_t umask);
// Scaled-integer lane kernel for fp64 distance-only batches whose costs are dyadic over at most 8 symbols (costs.json
// with N: multiples of 1/4): every cost times S = 2^shift is an integer, and the reference's fp64 sums of such values
// are exact, so an integer DP of the scaled costs gives D * S exactly (sed_lane.hip: sed_lane_scaled_kernel).
// row[a] = the 8 bytes (cost(a -> b) * S - ins - del - 1) & 0xFF for b = 0..7 (b = 0..3 in row[a][0]); ins / del
// scaled; pairs with pd.pad[0] run bit-parallel as in sed_lane_f64_kernel (umap: the 2-bit unit-subset code of every
// code < 8 at bits 2c).  Byte-coded sequences start 16-byte aligned (sed_plan.cpp: plan_layout).
struct sed_scaled_params {
    uint32_t row[8][2];
    uint32_t ins, del;
    double inv_scale;  // 2^-shift
    uint32_t umask, umap;
};
hipError_t sed_launch_lane_scaled(const sed_launch &L, const int32_t *idx, int nidx, const sed_scaled_params &sp);
// Fit search (sed_fit.hip: sed_fit_kernel; include/sed.h: sed_fit_search).  One lane per (pair, chunk): it owns the
// text columns [c0, c0 + cnt) of its pair and starts `lead` columns before c0 at the border column, which is symbol
// 4 tw of the packed text buffer (every text starts 4-byte aligned and lead is rounded up so the lane does too); it
// runs nsteps columns after the border column.  pat = the pair's pattern record (32 byte codes, the pattern
// right-aligned, code 8 in front).  row[a] = the 8 bytes kappa(a -> b) = insert + delete - min(cost(a -> b), insert +
// delete) on the integer scale, b = 0..3 in row[a][0].  out[pair] = min over the pair's lanes of
// D << 48 | end << 16 | (end - start), preset to all ones.
struct sed_fit_lane {
    uint32_t tw;
    int32_t pair, pat, plen;
    int32_t nsteps, lead, cnt, c0;
};
struct sed_fit_params {
    uint32_t row[8][2];
    uint32_t ins, del;
};
#define SED_FIT_BLOCK 64
hipError_t sed_launch_fit(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_lane *lanes, int nlanes,
                          const void *pats, const void *text, unsigned long long *out, const sed_fit_params &fp);
// columns a lane that owns [c0, ...) starts before c0: min(c0, W) rounded up so that c0 - lead is a multiple of 4
__host__ __device__ inline int32_t sed_fit_lead(int64_t W, int64_t c0) {
    const int64_t jb = c0 <= W ? 0 : (c0 - W) & ~(int64_t)3;
    return (int32_t)(c0 - jb);
}
// Fit search over a resident index (sed_fit.hip: sed_fit_index_kernel; include/sed.h: sed_fit_index_search).  The index
// keeps one record per text (the word its copy starts at, its length) and, per chunk length, one record per (text,
// chunk): neither depends on a query.  A lane is a (query, chunk record): it derives the sed_fit_lane sed_fit_kernel
// would be handed for pair query * ntexts + text from the two records, the chunk length, the query's P and the
// search's W (sed_fit_derive_lane: pair = the text, pat = 0, for the caller to set), and runs the same DP.
struct sed_fit_chunk {
    int32_t text, c0;  // the text and the chunk's first owned column
};
struct sed_fit_text {
    uint32_t base;  // the 4-symbol word at which the text's copy starts
    int32_t len;
};
__host__ __device__ inline sed_fit_lane sed_fit_derive_lane(sed_fit_chunk ck, sed_fit_text tx, int32_t chunk, int32_t plen,
                                                            int64_t W) {
    const int64_t ncol = (int64_t)tx.len + 1, c0 = ck.c0;
    const int64_t c1 = chunk > 0 && c0 + chunk < ncol ? c0 + chunk : ncol;
    const int32_t lead = sed_fit_lead(W, c0);
    sed_fit_lane ln;
    ln.tw = tx.base + (uint32_t)((c0 - lead) / 4);
    ln.pair = ck.text;
    ln.pat = 0;
    ln.plen = plen;
    ln.nsteps = (int32_t)(c1 - 1 - (c0 - lead));
    ln.lead = lead;
    ln.cnt = (int32_t)(c1 - c0);
    ln.c0 = (int32_t)c0;
    return ln;
}
// One search: queries q0 .. q0 + nq) of the grid's y run against every chunk record; pats = 32-byte pattern records,
// plens = their lengths, by query; out[query * ntexts + text], preset to all ones.
struct sed_fit_index_args {
    const sed_fit_chunk *chunks;
    int nchunks;
    const sed_fit_text *texts;
    int ntexts;
    const void *pats;
    const int32_t *plens;
    int nqueries;
    const void *text;
    unsigned long long *out;
    int32_t chunk;
    int32_t W;
};
// A search's launches (every index launcher of the four fit units): the queries are a grid's y, so they run in groups of
// at most SED_FIT_MAX_QUERIES.  launch(q0, nq, e0, e1) runs queries [q0, q0 + nq) and returns its error, the first of
// which ends the search; it starts e0 with its first kernel and stops e1 with its last.  The events bracket the whole
// search: ev0 goes to the first group, ev1 to the last, the others get null.  Host code without a kernel in it:
// tools/fit_groups_check.cpp runs it with a recording callback.
#define SED_FIT_MAX_QUERIES 65535  // a grid's y extent
template <class Launch>
inline hipError_t sed_fit_each_query_group(int nchunks, int nqueries, hipEvent_t ev0, hipEvent_t ev1, Launch launch) {
    if (nchunks <= 0 || nqueries <= 0) return hipSuccess;
    for (int q0 = 0; q0 < nqueries; q0 += SED_FIT_MAX_QUERIES) {
        const int nq = nqueries - q0 < SED_FIT_MAX_QUERIES ? nqueries - q0 : SED_FIT_MAX_QUERIES;
        const hipError_t e = launch(q0, nq, q0 == 0 ? ev0 : nullptr, q0 + nq == nqueries ? ev1 : nullptr);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t sed_launch_fit_index(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                const sed_fit_params &fp);
// The same lanes, reporting every owned column whose sink distance * S is <= cut (sed_fit.hip:
// sed_fit_index_hits_kernel; a.out is not used): hits = 16-byte records (pair, end, end - start, D * S), room for cap;
// *count, zeroed by the caller, counts every hit, stored or not.
hipError_t sed_launch_fit_index_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                     void *hits, unsigned long long *count, unsigned long long cap, int32_t cut,
                                     const sed_fit_params &fp);
// Long patterns (sed_fit_long.hip; include/sed.h: sed_fit_index_search_long): one wave per (query, chunk record), the
// pattern's rows over the wave's 64 lanes, `rows` = R in {2, 4, 8, 16, 32} consecutive rows a lane, P <= 64 R.  One
// launch serves the a.nqueries queries of one R: a.pats = their records of 64 R bytes (the pattern right-aligned, code
// 8 in front), qlist[k] = the query whose record is the k-th, a.plens by query.  The wave derives the chunk's
// sed_fit_lane as the short kernels do and reports in their words, into out[query * ntexts + text] or the hit list.
// ev0 / ev1 may be null (a search of several R starts the first group's and stops the last's).
#define SED_FIT_LONG_MAXP 2048
__host__ __device__ inline int sed_fit_long_rows(int P) {  // the smallest R with 64 R >= P
    int R = 2;
    while (64 * R < P) R *= 2;
    return R;
}
// `rows` as a compile-time R for the long launchers (sed_for_R over the R of sed_fit_long_rows)
template <class F> inline hipError_t sed_fit_long_with_rows(int rows, F f) { return sed_for_R<2, 4, 8, 16, 32>(rows, f); }
hipError_t sed_launch_fit_index_long(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                     const int32_t *qlist, int rows, const sed_fit_params &fp);
hipError_t sed_launch_fit_index_long_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                          const int32_t *qlist, int rows, void *hits, unsigned long long *count,
                                          unsigned long long cap, int32_t cut, const sed_fit_params &fp);
// The fp64 route (sed_fit_f64.hip; include/sed.h: sed_fit_search_f64): the short kernels' lanes, chunk table and
// pattern records, the DP in fp64 as the oracle states it, for the tables and alphabets the integer keys refuse.
// sub = SED_FIT_F64_MAXK x SED_FIT_F64_MAXK doubles on the device, row a = pattern symbol a, zeros past K.  A lane
// writes rec[its lane index] = its first strict minimum over the columns it owns; sed_launch_fit_f64_reduce then takes,
// per pair, the first strict minimum over the pair's lanes in chunk order into out[pair] (D = all ones: no result).
#define SED_FIT_F64_MAXK 16
struct sed_fit_f64_best {
    double D;
    int32_t start, end;
};
struct sed_fit_f64_hit {  // one record of the fp64 hit list
    uint32_t pair, end;
    int32_t start;
    uint32_t zero;
    double D;
};
struct sed_fit_f64_costs {
    const double *sub;
    double ins, del;
};
hipError_t sed_launch_fit_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_lane *lanes, int nlanes,
                              const void *pats, const void *text, sed_fit_f64_best *rec, sed_fit_f64_best *out,
                              const sed_fit_f64_costs &fc);
// a.out is not used: rec = a.nqueries x a.nchunks records (query-major), out = a.nqueries x a.ntexts
hipError_t sed_launch_fit_index_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                    sed_fit_f64_best *rec, sed_fit_f64_best *out, const sed_fit_f64_costs &fc);
// every owned column whose sink value is <= max_dist (a plain fp64 compare), appended as sed_fit_index_hits' kernel does
hipError_t sed_launch_fit_index_f64_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                         sed_fit_f64_hit *hits, unsigned long long *count, unsigned long long cap,
                                         double max_dist, const sed_fit_f64_costs &fc);
// The fp64 route for long patterns (sed_fit_long_f64.hip; include/sed.h: sed_fit_index_search_long_f64): the long
// kernels' waves, R groups, pattern records and qlist, the fp64 kernels' cell, cost table, records and hit list.  One
// call serves one R group: its waves write rec[query * a.nchunks + chunk record], then its reduce kernel writes
// out[query * a.ntexts + text]; a.out is not used.
hipError_t sed_launch_fit_index_long_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                         const int32_t *qlist, int rows, sed_fit_f64_best *rec, sed_fit_f64_best *out,
                                         const sed_fit_f64_costs &fc);
hipError_t sed_launch_fit_index_long_f64_hits(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_fit_index_args &a,
                                              const int32_t *qlist, int rows, sed_fit_f64_hit *hits, unsigned long long *count,
                                              unsigned long long cap, double max_dist, const sed_fit_f64_costs &fc);
// Similarity join (sed_join.hip; include/sed.h: sed_join_self, sed_join_search).  Every sequence is a record of
// SED_JOIN_MAXLEN byte codes, zero padded.  A lane owns one column record (the index's sequences sorted by length,
// col_orig[t] = the original index of sorted column t) and the block's waves walk the rows row0 + SED_JOIN_G blockIdx.y
// .. of the row records (the index's sequences in their own order, or a search's queries): grid = (column blocks of
// SED_JOIN_BLOCK lanes) x (row groups of SED_JOIN_G rows).  The row loads are wave-uniform and read up to two words past
// a record, so both record buffers end with 16 spare bytes.
//   tab[a] = the 8 bytes (cost(a -> b) * S - ins - del - 1) & 0xFF (sed_scaled_params::row) on the device;
//   umap   = the 2-bit code of every symbol < 8 at bits 2c, for the bit-parallel variant;
//   cut    = floor(max_dist * S); a pair is a hit when D * S <= cut, and is not computed when its length bound
//            insert (m - n)+ + delete (n - m)+ on the integer scale exceeds cut (a wave whose lanes all fail it skips
//            the row);
//   hits   = 16-byte records (row, original column, D * S, 0), room for cap; count[0] counts every hit, stored or not,
//            count[1] the pairs in scope whose bound passed (the pairs the waves ran); both zeroed by the caller.
// self: the pair (r, column of original index r) is out of scope.
#define SED_JOIN_G 4
#define SED_JOIN_BLOCK 256
#define SED_JOIN_MAXLEN 32
#define SED_JOIN_MAX_GROUPS 65535  // a grid's y extent
struct sed_join_sides {  // the two sides of a launch, the same for every route: s of sed_join_args and sed_join_f64_args
    const void *rows;
    const int32_t *row_len;
    int32_t row0, nrows;
    const void *cols;
    const int32_t *col_len, *col_orig;
    int32_t ncols;
    int32_t self;
};
struct sed_join_list {  // the hit list and the two counters, the same for every route: out of both
    uint4 *hits;
    unsigned long long *count;
    unsigned long long cap;
};
struct sed_join_args {
    sed_join_sides s;
    const uint2 *tab;
    uint32_t ins, del, umap;
    int32_t shift;  // log2 S: the bit-parallel variant's D << shift is the scaled distance
    int32_t cut;
    sed_join_list out;
};
hipError_t sed_launch_join(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_args &a, bool bitpar);
// The integer join over sequences of 0..SED_JOIN_LONG_MAXLEN symbols (sed_join_long.hip; include/sed.h: sed_join_long_self,
// sed_join_long_search): sed_join_args, the grid, the counters, the self rule and the hit records of the kernel above.
// What differs is the record: SED_JOIN_LONG_MAXLEN byte codes, zero padded, 32 words.  The row loads are wave-uniform and
// read up to two words past a record (word 33 of a row of 128 symbols), so both record buffers end with 16 spare bytes.
// The scaled DP keeps V[0 .. 128] and the column's 32 code words in registers and runs a row in blocks of
// SED_JOIN_LONG_BLOCK columns, the bit-parallel variant keeps four 32-bit words of state; a block or word above the
// wave's longest column is not run.
#define SED_JOIN_LONG_MAXLEN 128
#define SED_JOIN_LONG_BLOCK 32
hipError_t sed_launch_join_long(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_args &a, bool bitpar);
// The fp64 route of the join (sed_join_f64.hip; include/sed.h: sed_join_self_f64, sed_join_search_f64): the same records,
// grid, counters and self rule.
//   sub      = SED_JOIN_F64_MAXK x SED_JOIN_F64_MAXK doubles on the device, row a = row symbol a, zeros past K;
//   keep[n]  = 33 words on the device, bit m set when a row of n and a column of m symbols are computed (the planner's
//              length skip, sed_join_plan.h: sed_join_f64_keep_rule); the kernel tests the bit and nothing else;
//   max_dist = the cutoff: a pair is a hit when its fp64 distance D <= max_dist;
//   hits     = 16-byte records (row, original column, D's low word, D's high word).
#define SED_JOIN_F64_MAXK 16
struct sed_join_f64_args {
    sed_join_sides s;
    const double *sub;
    const unsigned long long *keep;
    double ins, del, max_dist;
    sed_join_list out;
};
// The kernels take both structs by value, so their layout is part of the code objects: every field where it was when
// each struct spelled its own copy of s and out.
#define SED_JOIN_AT(T, field, at) static_assert(offsetof(T, field) == at, #T "." #field " moved")
#define SED_JOIN_SIDES_AT(T)                                                                                         \
    SED_JOIN_AT(T, s.rows, 0); SED_JOIN_AT(T, s.row_len, 8); SED_JOIN_AT(T, s.row0, 16); SED_JOIN_AT(T, s.nrows, 20); \
    SED_JOIN_AT(T, s.cols, 24); SED_JOIN_AT(T, s.col_len, 32); SED_JOIN_AT(T, s.col_orig, 40);                       \
    SED_JOIN_AT(T, s.ncols, 48); SED_JOIN_AT(T, s.self, 52)
SED_JOIN_SIDES_AT(sed_join_args);
SED_JOIN_AT(sed_join_args, tab, 56); SED_JOIN_AT(sed_join_args, ins, 64); SED_JOIN_AT(sed_join_args, del, 68);
SED_JOIN_AT(sed_join_args, umap, 72); SED_JOIN_AT(sed_join_args, shift, 76); SED_JOIN_AT(sed_join_args, cut, 80);
SED_JOIN_AT(sed_join_args, out.hits, 88); SED_JOIN_AT(sed_join_args, out.count, 96); SED_JOIN_AT(sed_join_args, out.cap, 104);
static_assert(sizeof(sed_join_args) == 112, "sed_join_args");
SED_JOIN_SIDES_AT(sed_join_f64_args);
SED_JOIN_AT(sed_join_f64_args, sub, 56); SED_JOIN_AT(sed_join_f64_args, keep, 64); SED_JOIN_AT(sed_join_f64_args, ins, 72);
SED_JOIN_AT(sed_join_f64_args, del, 80); SED_JOIN_AT(sed_join_f64_args, max_dist, 88);
SED_JOIN_AT(sed_join_f64_args, out.hits, 96); SED_JOIN_AT(sed_join_f64_args, out.count, 104);
SED_JOIN_AT(sed_join_f64_args, out.cap, 112);
static_assert(sizeof(sed_join_f64_args) == 120, "sed_join_f64_args");
#undef SED_JOIN_SIDES_AT
#undef SED_JOIN_AT
// The k nearest columns of every row (include/sed.h: sed_join_knn_self, sed_join_knn_search and their _long_ twins): the
// integer join's kernels under two other walks over the rows (sed_join_dev.h).  j = the join's arguments as they are,
// j.cut = the cap floor(max_dist S); bound[r], r = the row's index as the join counts it (j.s.row0 ..), starts at j.cut.
// Pass 1 (emit = false) lowers bound[r] to the smallest k-th smallest in-scope distance any wave finds and appends
// nothing; pass 2 (emit = true) is the join with bound[r] in place of j.cut.  Both add to count[1]; 1 <= k <= 64.
#define SED_JOIN_KNN_MAXK 64
struct sed_join_knn_args {
    sed_join_args j;
    uint32_t *bound;
    int32_t k;
};
hipError_t sed_launch_join_knn(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_args &a, bool bitpar,
                               bool emit);
hipError_t sed_launch_join_long_knn(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_args &a,
                                    bool bitpar, bool emit);
hipError_t sed_launch_join_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_f64_args &a);
// The k nearest columns of every row on the fp64 route (include/sed.h: sed_join_knn_self_f64, sed_join_knn_search_f64):
// the fp64 join's kernel under two other passes (sed_join_f64.hip).  j = the join's arguments, j.keep unused, j.max_dist
// = the cap; bound[r], r indexed as for sed_join_knn_args, is a 64-bit word holding the bits of a double (finite or
// +inf, >= +0: such bits order as the values do) and starts at j.max_dist's; low = 33 x 33 doubles on the device,
// low[33 n + m] <= every distance of a row of n and a column of m symbols (sed_join_plan.h: sed_join_f64_lower_rule):
// the length skip is low[33 n + m] <= bound[r], a compare.  Pass 1 (emit = false) lowers bound[r] to the smallest k-th
// smallest in-scope distance any wave finds and appends nothing; pass 2 (emit = true) is the join with bound[r] in
// place of j.max_dist.  Both add to count[1]; 1 <= k <= 64.
struct sed_join_knn_f64_args {
    sed_join_f64_args j;
    unsigned long long *bound;
    const double *low;
    int32_t k;
};
hipError_t sed_launch_join_knn_f64(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const sed_join_knn_f64_args &a,
                                   bool emit);
hipError_t sed_launch_traceback(const sed_launch &L, uint32_t *ops);
// stripe-parallel traceback of few long pairs (per-cell codes): map[pd.map_off ...] per pair, ops zeroed first
hipError_t sed_launch_traceback_stripes(const sed_launch &L, uint32_t *ops, uint32_t *map, int items, int kmax);
// A pair's schedule on the wave kernels (SW = 64 lanes a pair, or 16 in the fp64 segments), R rows per lane: nstripes
// stripes of SW R rows, each SG steps (m + SW - 1 rounded up to whole traceback groups of G = 64/R steps) in nchunks
// chunks of SW steps.
struct sed_geom {
    int nstripes, SG, nchunks;
};
__host__ __device__ inline sed_geom sed_stripe_geom(int n, int m, int R, int SW) {
    const int64_t G = 64 / R, rows = (int64_t)SW * R;
    sed_geom g;
    g.nstripes = (int)((n + rows - 1) / rows);
    g.SG = (int)((m + SW - 1 + G - 1) / G * G);
    g.nchunks = (g.SG + SW - 1) / SW;
    return g;
}
// Checkpoint layout of the CK forward kernels (R = 4, 8 or 16 rows per lane, G = 64/R steps per group):
//   column checkpoints, per stripe [nchunks][R + 1][64 lanes]: each lane's R row values and its top_prev
//   at every 64-step chunk end;
//   then row checkpoints, per stripe [SG/G groups][64/G lanes t = G-1 (mod G)][G steps]: the bottom row of
//   every G-th lane at every step (the row above each 64-row traceback tile).
__host__ __device__ inline uint64_t sed_ck_col_word(int R, int stripe, int nchunks, int c, int r, int t) {
    return (((uint64_t)stripe * (uint64_t)nchunks + (uint64_t)c) * (uint64_t)(R + 1) + (uint64_t)r) * 64u +
           (uint64_t)t;
}
__host__ __device__ inline uint64_t sed_ck_col_words(int R, int nstripes, int nchunks) {
    return (uint64_t)nstripes * (uint64_t)nchunks * (uint64_t)(R + 1) * 64u;
}
// Row checkpoints: every step, the bottom row of the forward lanes t = GH-1 (mod GH), GH = SED_CK_TILE / R, i.e.
// of every SED_CK_TILE-th matrix row (the traceback's tile height, 64).  Per stripe and G-step group (G = 64/R):
// SED_CK_RW = 64 * 64 / SED_CK_TILE words, [group][t / GH][step % G].  SED_CK_TILE = 32 (twice the row checkpoints)
// served a two-pairs-per-wave traceback of 32-row tiles, measured and dropped in round 3: the forward kernel took
// 9.87 instead of 9.18-9.32 ms and that traceback 2.43 instead of 2.20 ms (profiles/r03/ab_tb_tiles.jsonl).
#ifndef SED_CK_HALVES_DEFAULT
#define SED_CK_HALVES_DEFAULT 2  // checkpoint batches: parts on as many streams, >= 1024 wave pairs each (sed_plan.cpp)
#endif
#ifndef SED_CK_TILE
#define SED_CK_TILE 64
#endif
#define SED_CK_RW (64 * 64 / SED_CK_TILE)
// row checkpoint of forward lane t (t = GH-1 mod GH) at step s of stripe k
__host__ __device__ inline uint64_t sed_ck_row_word(int R, int k, int ngroups, int s, int t) {
    const int G = 64 / R, GH = SED_CK_TILE / R;
    return ((uint64_t)k * (uint64_t)ngroups + (uint64_t)(s / G)) * (uint64_t)SED_CK_RW + (uint64_t)(t / GH) * (uint64_t)G +
           (uint64_t)(s % G);
}
// Band pruning of checkpoint script batches of the stripe kernel.  With substitution costs >= 0, any
// path through cell (i, j), e = j - i, costs at least insert (e+ + (D - e)+) + delete ((-e)+ + (e - D)+), D = m - n.
// UB = the cost of the plain diagonal path (sum of sub(a_i, b_i) over i < min(n, m), plus |D| inserts or deletes) bounds
// the distance from above, so only cells with elo <= e <= ehi can lie on an optimal path:
//   e <= (UB + delete D) / (insert + delete),   -e <= (UB - insert D) / (insert + delete)     (integer floor).
// Both numerators are >= 0 (UB >= insert D+ + delete (-D)+), and elo <= min(0, D), ehi >= max(0, D).
struct sed_band {
    int32_t elo, ehi;
};
#define SED_BAND_OPEN_LO (-0x20000000)
#define SED_BAND_OPEN_HI 0x20000000
__host__ __device__ inline sed_band sed_band_window(int n, int m, uint32_t ins, uint32_t del, uint64_t ub) {
    const int64_t D = (int64_t)m - n, s = (int64_t)ins + del;
    int64_t hi = ((int64_t)ub + (int64_t)del * D) / s, lo = ((int64_t)ub - (int64_t)ins * D) / s;
    hi = hi > m ? m : hi;
    lo = lo > n ? n : lo;
    sed_band w;
    w.elo = (int32_t)-lo;
    w.ehi = (int32_t)hi;
    return w;
}
// Stripe k (rows k ROWS + 1 .. min(n, (k + 1) ROWS)) needs columns [r0 + 1 + elo, r1 + ehi] clipped to [1, m]; its
// schedule runs whole 64-step chunks clo .. chi (x = clo, y = chi): every lane starts at column 64 clo + 1 from the
// border state (lane 0's first diagonal, the stripe above's cell at column 64 clo, is the real value where that stripe
// computed it: it is inside the window when 64 clo = r0 + elo), and lane 63 reaches column 64 chi + 1 (lane t: 64 chi +
// 64 - t).  Both are nondecreasing in k, clo <= chi <= nchunks - 1, and the last stripe's range holds the sink's chunk.
// An open window gives 0 .. nchunks - 1.
__host__ __device__ inline void sed_band_chunks(int n, int m, int ROWS, int nchunks, sed_band w, int k, int *clo,
                                                int *chi) {
    const int64_t r0 = (int64_t)k * ROWS, r1 = r0 + ROWS < n ? r0 + ROWS : n;
    int64_t jlo = r0 + 1 + w.elo, jhi = r1 + w.ehi;
    jlo = jlo < 1 ? 1 : (jlo > m ? m : jlo);
    jhi = jhi > m ? m : (jhi < 1 ? 1 : jhi);
    const int lo = (int)((jlo - 1) >> 6), hi = (int)((jhi + 62) >> 6);
    *chi = hi < nchunks - 1 ? hi : nchunks - 1;
    *clo = lo < *chi ? lo : *chi;
}
// Refined windows ("Refinement"): before stripe k >= 1 the forward holds row r0 = k ROWS of the stripe
// above, every value a real path's cost.  With UB_k = min(UB_{k-1}, D(r0, r0) + suf(r0)) (suf = the plain diagonal's
// cost from (r0, r0) to the sink), a cell (r0, j), e0 = j - r0, with
//   slack = UB_k - D(r0, j) - rem,   rem = insert (Dl - e0)+ + delete (e0 - Dl)+,   Dl = m - n
// below 0 lies on no optimal path.  A path through a surviving cell that later touches diagonal e costs at least
// D + insert ((e - e0)+ + (Dl - e)+) + delete ((e0 - e)+ + (e - Dl)+): moving towards Dl is paid for by rem already,
// every step beyond [min(e0, Dl), max(e0, Dl)] costs insert + delete more.  So it stays within
//   min(e0, Dl) - slack / (insert + delete)  <=  e  <=  max(e0, Dl) + slack / (insert + delete)      (integer floor).
// sed_refine_cell folds one cell into the running extremes, kept times s = insert + delete so that no cell divides:
// lo = min(s min(e0, Dl) - slack), hi = max(s max(e0, Dl) + slack); lo > hi = no cell survived.  The planner keeps
// s (n + m) below 2^30 for every pair of a refined batch, so everything fits 32 bits.
#define SED_REFINE_LO_INIT 0x7FFFFFFF
#define SED_REFINE_HI_INIT (-0x7FFFFFFF - 1)
#define SED_REFINE_NO_SUF 0xFFFFFFFFu  // suf(r0) of a stripe boundary below the diagonal's end (r0 > min(n, m))
__host__ __device__ inline void sed_refine_cell(int n, int m, uint32_t ins, uint32_t del, int r0, int j, uint32_t D,
                                                uint32_t ub, int32_t *lo, int32_t *hi) {
    const int32_t dl = m - n, e0 = j - r0, s = (int32_t)(ins + del);
    const int32_t rem = e0 < dl ? (int32_t)ins * (dl - e0) : (int32_t)del * (e0 - dl);
    const int32_t slack = (int32_t)ub - (int32_t)D - rem;
    if (slack < 0) return;
    const int32_t a = s * (e0 < dl ? e0 : dl) - slack, b = s * (e0 < dl ? dl : e0) + slack;
    *lo = a < *lo ? a : *lo;
    *hi = b > *hi ? b : *hi;
}
// Stripe k's chunk range from the extremes over row r0's computed cells: the offsets [ceil(lo / s), floor(hi / s)]
// inside the static window of UB_k, mapped to chunks as sed_band_chunks does, then raised to the range of the stripe
// above (the kernels rely on both ends being nondecreasing: top_hi, the clo > clo_prev diagonal load, the in-place
// bottom-row buffer; a path is monotone, so neither clamp drops a cell an optimal path reaches).  False when no cell
// survived: the stripe then keeps the static range of UB_k (a correct forward always has a survivor, the cell of
// row r0 on an optimal path).  The refined offsets hold Dl, so the last stripe's range holds the sink's chunk.
__host__ __device__ inline bool sed_refine_chunks(int n, int m, int ROWS, int nchunks, uint32_t ins, uint32_t del,
                                                  uint32_t ub, int32_t lo, int32_t hi, int k, int clo_prev, int chi_prev,
                                                  int *clo, int *chi) {
    // (sed_band_window in 32 bits: ub and delete |Dl| stay below 2^30 under the planner's bound, both numerators >= 0)
    const int32_t s = (int32_t)(ins + del), dl = m - n;
    const uint32_t whi = (uint32_t)((int32_t)ub + (int32_t)del * dl) / (uint32_t)s;
    const uint32_t wlo = (uint32_t)((int32_t)ub - (int32_t)ins * dl) / (uint32_t)s;
    sed_band w;
    w.ehi = (int32_t)(whi > (uint32_t)m ? (uint32_t)m : whi);
    w.elo = -(int32_t)(wlo > (uint32_t)n ? (uint32_t)n : wlo);
    const bool any = lo <= hi;
    if (any) {
        const uint32_t us = (uint32_t)s;
        const int32_t elo = lo >= 0 ? (int32_t)(((uint32_t)lo + us - 1u) / us) : -(int32_t)((uint32_t)(-lo) / us);  // ceil
        const int32_t ehi = hi >= 0 ? (int32_t)((uint32_t)hi / us) : -(int32_t)(((uint32_t)(-hi) + us - 1u) / us);  // floor
        w.elo = elo > w.elo ? elo : w.elo;
        w.ehi = ehi < w.ehi ? ehi : w.ehi;
    }
    sed_band_chunks(n, m, ROWS, nchunks, w, k, clo, chi);
    *clo = *clo > clo_prev ? *clo : clo_prev;
    *chi = *chi > chi_prev ? *chi : chi_prev;
    return any;
}
// the per-stripe windows as the kernels take them (sed_launch: bwin, bsuf, bstripes); all null = none
struct sed_stripe_wins {
    int2 *win;
    const uint32_t *suf;
    int stride;
};
// cells of the pair inside its stripes' chunk ranges: rows x (64 (chi - clo)) columns per stripe (the columns every
// lane computes, as n m counts them for an unpruned pair; a stripe that runs to its last chunk counts up to m)
__host__ __device__ inline double sed_band_pair_cells(int n, int m, int R, sed_band w) {
    const int ROWS = 64 * R, nstripes = sed_stripe_geom(n, m, R, 64).nstripes, nchunks = sed_stripe_geom(n, m, R, 64).nchunks;
    double cells = 0;
    for (int k = 0; k < nstripes; ++k) {
        int clo, chi;
        sed_band_chunks(n, m, ROWS, nchunks, w, k, &clo, &chi);
        const int rows = (k + 1) * ROWS < n ? ROWS : n - k * ROWS;
        const int jend = (chi >= nchunks - 1 || 64 * chi > m) ? m : 64 * chi;
        cells += (double)rows * (double)(jend - 64 * clo);
    }
    return cells;
}
// the diagonal bound's inputs, for sed_band_kernel: cost[a * 4 + b] = sub(a -> b) as an integer
struct sed_band_params {
    uint32_t cost[16];
    uint32_t ins, del;
};
// UB and the window of every wave pair of the launch, into band[pair] (one wave per pair; the forward's first kernel);
// with L.bsuf also the diagonal's suffix cost at every stripe boundary
hipError_t sed_launch_band(const sed_launch &L, const sed_band_params &bp);
// Cutoff batches (sed_batch_set_cutoff).  tkey = the cutoff on the integer scale.
// sed_launch_i32_cut: the windowed distance-only stripe kernel (R = 4, 8, 16) over the wave pairs list[0 .. nlist), after
// their windows of this run (L.band, L.bandp: ub = min(tkey, diagonal bound); an empty window {1, 0} = the pair runs no
// stripe and reports +inf).  sed_launch_cut_band alone also stores every listed pair's diagonal bound into diag.
// sed_launch_cut_filter: every result of L.res above `cutoff` becomes {+inf, len -1, not an int}; *hits += pairs within.
hipError_t sed_launch_cut_band(const sed_launch &L, const int32_t *list, int nlist, uint32_t *diag,
                               const sed_band_params &bp, uint32_t tkey);
hipError_t sed_launch_i32_cut(const sed_launch &L, const int32_t *list, int nlist, const sed_i32_params &prm,
                              uint32_t tkey);
hipError_t sed_launch_cut_filter(const sed_launch &L, double cutoff, uint32_t *hits);
// CK batches (L.ck): the traceback that recomputes tiles from the forward kernel's checkpoints
hipError_t sed_launch_traceback_ck(const sed_launch &L, uint32_t *ops, const sed_i32_params &prm);
// SPLIT batches with checkpoints: every tile's op codes from the checkpoints, into the per-cell code layout (one wave
// per tile of each pair: grid max_tiles x npairs)
hipError_t sed_launch_ck_codes(const sed_launch &L, int max_tiles, const sed_i32_params &prm);
hipError_t sed_launch_selftest(uint32_t *d_out, hipStream_t stream);
