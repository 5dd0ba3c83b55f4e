/*
 * sed.h — C-ABI of libsed.so, the MI355X (gfx950) engine for the weighted
 * Wagner–Fischer edit distance and its canonical edit script.
 *
 * It replaces the compute inside the reference's Python module
 * StringEditDistance (plsakr/rna-sequence-diff-patch):
 *   wagnerFisher(str1, str2, userCosts)   StringEditDistance.py:133-224  -> sed_run_batch / sed_batch_*
 *   min_cost / cost (per-cell recurrence) StringEditDistance.py:76-128   -> the DP kernels
 *   create_paths(dp)[0] (canonical path)  StringEditDistance.py:228-271  -> SED_WANT_SCRIPT traceback
 *   generate_es op sequence               StringEditDistance.py:274-334  -> packed op codes
 *   wf_score distance                     IRMethods.py:435-440           -> out_dist
 * The reference has no FFI; its boundary is the Python module itself.  The
 * Python shim (rna-sequence-diff-patch_amd/StringEditDistance.py) keeps that
 * module's names and calls this ABI through ctypes (binding shown in
 * INTEGRATION.md).
 *
 * Conventions
 *   - Sequences are passed as per-call alphabet codes (uint8, 0..K-1); the
 *     caller resolves characters -> codes and the reference's cost() into a
 *     K x K matrix (value + "is a Python int" flag) and raises the
 *     reference's KeyError itself before calling.
 *   - Every host buffer is caller-allocated.  The context owns device memory
 *     and its HIP stream.  No C++ exception crosses this ABI; functions return
 *     SED_OK or a negative SED_E_* code, with text in sed_last_error().
 *   - Threading: one context per thread and device; calls on one context are
 *     serialised by the caller; distinct contexts are independent.
 *   - Op codes of a script, origin -> sink order, 2 bits each, 16 per uint32
 *     (op p at bits 2*(p%16) of word p/16): 0 insert, 1 delete, 2 update.
 */
#ifndef SED_H
#define SED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SED_OK = 0,
    SED_E_ARG = -1,       /* bad argument (NULL, negative length, non-finite cost ...) */
    SED_E_DEVICE = -2,    /* HIP error */
    SED_E_OOM = -3,       /* device allocation failed */
    SED_E_RANGE = -4,     /* forced integer mode but the packed key would overflow */
    SED_E_ALPHABET = -5,  /* alphabet larger than the kernel supports (K > 32) */
    SED_E_STATE = -6      /* call order (no costs set, batch not run ...) */
};

/* flags for sed_run_batch / sed_batch_create */
#define SED_WANT_SCRIPT 1u
/* sed_batch only, a hint:
 *  - batches with per-cell traceback codes get three traceback/result buffers and a traceback stream, so the
 *    traceback of run k overlaps the DP kernel of run k+1 (device memory for the traceback triples); dynamic-CHAIN
 *    script batches also put odd runs' DP on a second DP stream (one device counter per buffer);
 *  - distance-only batches of lane pairs alternate their runs over two streams with one result slot each;
 *  - checkpoint batches (sed_batch_traceback_mode 2, the default for script batches of > 256 pairs) ignore it.
 *    Instead, one of >= 2048 wave pairs always runs in parts: part i (a contiguous range of pairs, >= 1024 wave
 *    pairs) runs forward then traceback on its own stream, 2 parts by default (environment SED_CK_HALVES = parts,
 *    1..4: up to 4 streams, the hardware queues a process gets), and nothing joins the streams at a run's end, so
 *    one part's traceback overlaps another part's forward (see sed_batch_dp_launches).
 * sed_batch_sync / _results / _export / _times wait for every stream a batch uses, and a refill waits first. */
#define SED_PIPELINE 2u
/* distance only (no SED_WANT_SCRIPT): out_len is not computed (-1), which lets the integer
 * kernels drop the op-count field of their keys (3 instead of ~4.2 VALU ops per cell). */
#define SED_NO_LEN 4u

/* sed_set_option keys */
#define SED_OPT_MODE 1          /* 0 auto, 1 packed-integer kernel, 2 fp64 kernel, 3 fp64 + int-typing */
#define SED_OPT_ROWS_PER_LANE 2 /* 0 auto, else 4,8,16,32 (integer) / 4,8 (fp64) */
#define SED_OPT_SPLIT 3         /* integer kernel, one wave per stripe: 0 auto (small batches of long
                                   pairs), 1 always, 2 never */
#define SED_OPT_LANE 4          /* one lane per pair for short str2 (m <= 32, n <= 512): 0 auto (on), 2 never */
#define SED_OPT_CHAIN 5         /* integer kernel, single-stripe pairs run back to back in one wave (no
                                   per-pair ramp): 0 auto (large batches), 1 whenever eligible, 2 never,
                                   L >= 3 whenever eligible with chains of L pairs */
#define SED_OPT_TB 7            /* integer script batches at R = 4/8/16 (stripe and CHAIN kernels, not SPLIT): 0 auto
                                   (checkpoints + recompute for > 256 pairs averaging >= 512 cells per path op,
                                   i.e. sum n*m >= 512 * sum (n+m)), 1 per-cell traceback codes, 2 checkpoints
                                   whenever eligible */
#define SED_OPT_PACK 6          /* distance-only integer batches (SED_NO_LEN): two pairs per lane (equal n) or per
                                   wave (equal n and m) in packed 16-bit cells: 0 auto (on), 2 never */
#define SED_OPT_CHAIN_WAVES 8   /* dynamic CHAIN mode: persistent waves, 0 auto (every SIMD's resident waves), else a
                                   cap (tests: several counter-fetched pairs per wave) */
#define SED_OPT_DOT 10          /* checkpoint batches of the stripe kernel and CHAIN batches: 0 auto (dot keys when
                                   the cost table's update addends factor over signed bytes and the pairs fit the
                                   bound), 2 never, 3 (tests) CHAIN ladder dot keys on the 3-bit ladder only */
#define SED_OPT_BITPAR 11       /* distance-only batches under unit costs (insert = delete = 1, every mismatch 1): lane
                                   pairs (m <= 32) run one per lane bit-parallel; in fp64 batches (e.g. costs.json with N)
                                   the lane pairs whose symbols all have unit costs among themselves: 0 auto (on),
                                   2 never */
#define SED_OPT_SCALED 12       /* distance-only fp64 batches whose costs are dyadic over <= 8 symbols (costs.json with N:
                                   multiples of 1/4): lane pairs run an exact integer DP of the costs scaled by 2^k
                                   (3 VALU per cell instead of the fp64 cell): 0 auto (on), 2 never */
#define SED_OPT_SEG 13          /* fp64 batches of > 256 wave pairs: pairs whose cost model favours it run in 16-lane
                                   segments, four per wave (stripes of 16 R rows, a 15-step ramp instead of 63: the
                                   timing.py sweep's short pairs): 0 auto, 1 every such pair, 2 never */
#define SED_OPT_SPLITCK 14      /* SPLIT script batches (<= 256 long pairs: config 2, GUI calls): the forward runs distance
                                   or dot keys with checkpoints and every 64 x 64 tile's codes are then recomputed at once
                                   for the stripe-parallel traceback (sed_batch_traceback_mode 4): 0 auto (on), 2 never
                                   (per-cell codes from the ladder-key forward) */
#define SED_OPT_ZEROCOPY 15     /* small batches (the per-call path) whose kernels write results and scripts with plain
                                   stores: the kernels write them into the batch's pinned host block, so no download
                                   follows the run: 0 auto (on), 2 never */
#define SED_OPT_BAND 16         /* checkpoint script batches of the stripe kernel (sed_batch_traceback_mode 2, not CHAIN):
                                   the forward skips the 64-step chunks of every stripe that no optimal path can reach,
                                   by the cost of the plain diagonal path as an upper bound on the distance (computed on
                                   the device in every run; substitution costs must be >= 0, else off): 0 auto (on),
                                   2 never, 3 the static windows only.  By default every stripe below a pair's first
                                   narrows its range further from the row the stripe above left behind (refined windows:
                                   a smaller upper bound from the diagonal cell, and each computed cell's slack under it).
                                   Environment SED_BAND=0 turns pruning off for the process, SED_BAND=static selects the
                                   static windows.  Results are the same bit for bit. */
#define SED_OPT_CUT 17          /* distance-only integer batches under a cutoff (sed_batch_set_cutoff), SED_NO_LEN, R = 4/8/16, not
                                   SPLIT: the wave pairs leave the two-pairs-per-wave and CHAIN routes for the windowed
                                   stripe kernel: 0 auto (when the window keeps < 2/3 of their cells; pairs already on the
                                   stripe kernel whenever it skips any), 1 whenever eligible, 2 never (filter only) */
#define SED_OPT_FIT_CHUNK 18    /* fit search (sed_fit_search): owned text columns per lane: 0 auto, else the chunk length
                                   (tests and A/Bs; a value >= every text's length + 1 is one lane per text).  An
                                   option of sed_fit_search / sed_fit_plan only: sed_plan_routes, which plans batches,
                                   refuses it */
#define SED_OPT_FIT_ROWS 19     /* the long fit calls (sed_fit_index_search_long, sed_fit_index_hits_long and their plan
                                   calls) only: pattern rows per lane, 0 auto (each query the smallest R of 2, 4, 8, 16,
                                   32 with 64 R >= P), else that R for every query (tests and A/Bs; a query of P > 64 R:
                                   SED_E_RANGE).  sed_plan_routes refuses it */
#define SED_OPT_JOIN_DP 20      /* the similarity join (sed_join_self, sed_join_search, sed_join_plan, sed_join_long_*) only: 0 auto (the
                                   bit-parallel kernel when the codes present have unit costs), 2 the scaled DP kernel always
                                   (tests and A/Bs).  sed_plan_routes refuses it */
#define SED_OPT_JOIN_ROWS 21    /* the similarity join only, for tests: the rows one launch takes, 0 auto (the grid's limit,
                                   65535 row groups); a call with more rows runs further launches.  sed_plan_routes
                                   refuses it */
#define SED_OPT_DEBUG_CORRUPT 9 /* testing only: p + 1 overwrites one checkpoint word of pair p before its traceback,
                                   which must then fail with SED_E_DEVICE naming the pair; 0 off */

/* modes reported by sed_batch_mode */
#define SED_MODE_I32 1
#define SED_MODE_F64 2
#define SED_MODE_F64_TYPED 3

typedef struct sed_ctx sed_ctx;
typedef struct sed_batch sed_batch;

const char *sed_version(void);

/* Create a context on HIP device `device` (NULL on failure). */
sed_ctx *sed_create(int device);
void sed_destroy(sed_ctx *ctx);
const char *sed_last_error(const sed_ctx *ctx);
int sed_set_option(sed_ctx *ctx, int key, int value);

/* Cost model (replaces default_costs / user_costs lookups, StringEditDistance.py:6-18,76-99).
 * sub[a*K+b] = cost(symbol a -> symbol b) as the reference's cost() returns it
 * (0 for case-insensitive matches), sub_int[a*K+b] = 1 when that value is a Python int. */
int sed_set_costs(sed_ctx *ctx, int K, const double *sub, const uint8_t *sub_int,
                  double ins, int ins_is_int, double del, int del_is_int);

/* One-shot batch: host inputs, host outputs (blocking).
 * Pair p: str1 = codes_a[off_a[p] .. +len_a[p]), str2 = codes_b[off_b[p] .. +len_b[p]).
 * out_dist[p]  = dp[n][m].value as fp64; out_is_int[p] = 1 when it is a Python int.
 * out_len[p]   = number of ops in the canonical script.
 * With SED_WANT_SCRIPT: out_ops + ops_off[p] receives ceil((n+m)/16) words for pair p: the out_len[p] ops, then
 * zeros (the bits past the last op in its word and every spare word after it, on every route, so a pair's words
 * are a function of its script alone; the device buffers of sed_batch_device_results / _export hold the same).
 * Script batches whose traceback workspace (~n*m/4 bytes per pair) exceeds SED_TB_BUDGET_GB
 * (environment, default 48) run as several consecutive launches. */
int sed_run_batch(sed_ctx *ctx,
                  const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                  const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                  int32_t npairs, uint32_t flags,
                  double *out_dist, uint8_t *out_is_int, int32_t *out_len,
                  uint32_t *out_ops, const int64_t *ops_off);

/* One pair, blocking: sed_run_batch with npairs = 1 and plain pointers (the drop-in module's per-call path:
 * wagnerFisher of one (str1, str2), StringEditDistance.py:133-224, as IRMethods.wf_score calls it per document,
 * IRMethods.py:435-440,469-470).  out_len may be NULL; with SED_WANT_SCRIPT, out_ops receives ceil((n+m)/16) words.
 * Small batches like this one go to the device as one blob from pinned staging and come back in one download, and
 * one-shot runs carry no timing events. */
int sed_run_pair(sed_ctx *ctx, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m, uint32_t flags,
                 double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops);

/* sed_run_pair in two halves (round 6): sed_pair_submit uploads the pair and enqueues its kernels, then returns; the
 * caller may do host work while the device computes (the drop-in module builds the edit-script records of
 * generate_es, StringEditDistance.py:274-334, for the GUI's wagnerFisher -> create_paths -> generate_es call,
 * gui.py:360,385-391); sed_pair_wait then waits and writes the results exactly as sed_run_pair would.  The inputs may
 * be freed once submit returns.  One pair in flight per context: until sed_pair_wait, sed_set_costs, sed_run_batch,
 * sed_run_pair, sed_full_matrix and another submit fail with SED_E_STATE. */
int sed_pair_submit(sed_ctx *ctx, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m, uint32_t flags);
int sed_pair_wait(sed_ctx *ctx, double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops);

/* Device-resident batch: upload once, run many times (bench), fetch results. */
sed_batch *sed_batch_create(sed_ctx *ctx,
                            const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                            const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                            int32_t npairs, uint32_t flags);
void sed_batch_destroy(sed_batch *b);
int sed_batch_mode(const sed_batch *b);               /* SED_MODE_* chosen for this batch */
int sed_batch_rows_per_lane(const sed_batch *b);
int sed_batch_lane_pairs(const sed_batch *b);         /* pairs on the lane-per-pair kernel (short str2) */
int sed_batch_chains(const sed_batch *b);             /* CHAIN mode: number of chains (0 = not used) */
int sed_batch_packed_pairs(const sed_batch *b);       /* pairs computed two per lane / wave (SED_OPT_PACK) */
int sed_batch_bitpar_pairs(const sed_batch *b);       /* lane pairs computed bit-parallel (SED_OPT_BITPAR) */
int sed_batch_scaled_pairs(const sed_batch *b);       /* fp64 lane pairs on the scaled-integer DP (SED_OPT_SCALED) */
int sed_batch_segment_pairs(const sed_batch *b);      /* fp64 wave pairs run in 16-lane segments (SED_OPT_SEG) */
int sed_batch_split_tasks(const sed_batch *b);        /* SPLIT: workgroups (pair, stripe) per run, 0 = not SPLIT */
/* The byte factorisation behind SED_OPT_DOT, without a device (tests): for the 4 x 4 table sub (a -> b, row-major)
 * and insert/delete costs, the dot keys for pairs with min(n, m) <= maxmin (ladder_maxsum = 0) or the ladder dot
 * keys for n + m <= ladder_maxsum (the wide ladder's, L unit 16, for min(n, m) <= maxmin (or ladder_maxsum when
 * maxmin is 0) where it exists, else the 3-bit ladder's, unit 8).
 * out[0..3] = row vectors, out[4..7] = column vectors (4 signed bytes each), out[8] = decode shift / ladder sentinel
 * byte, out[9] = decode multiplier / ladder L unit.  Returns A (> 0), 0 when the table has no such factorisation,
 * or SED_E_ARG. */
int sed_dot_factor(const double *sub, double ins, double del, int maxmin, int ladder_maxsum, uint32_t *out);
/* The planner, without a device (tests, diagnostics): what sed_batch_create would decide for these costs (as
 * sed_set_costs takes them), options and pairs (as sed_batch_create takes them), with no context and no HIP call.
 * options = noptions (key, value) pairs: the SED_OPT_* keys with the values sed_set_option takes, and the
 * SED_PLAN_ENV_* keys below, which stand for the process environment the runtime reads once (any value).
 * out[0 .. nout) receives, in this order, what the getters of the created batch would return:
 *   0 sed_batch_mode, 1 _rows_per_lane, 2 _lane_pairs, 3 _chains, 4 _traceback_mode, 5 _dot_keys, 6 _bitpar_pairs,
 *   7 _segment_pairs, 8 _split_tasks, 9 _scaled_pairs, 10 _packed_pairs, 11 _dp_launches, 12 _band_cells,
 *   13 and 14 sed_batch_work's cells and algo_bytes.
 * Returns SED_OK or the SED_E_* code batch creation would fail with (SED_E_ARG also for a bad option). */
#define SED_PLAN_ENV_TBPAR 101     /* SED_TBPAR: 0 / 1 overrides the stripe-parallel traceback's rule; unset = -1 */
#define SED_PLAN_ENV_BAND 102      /* SED_BAND: 0 turns band pruning off, 3 (SED_BAND=static) keeps the static windows;
                                      unset = 1 */
#define SED_PLAN_ENV_ALT_DP 103    /* SED_ALT_DP: 0 keeps every DP on the context's stream; unset = 1 */
#define SED_PLAN_ENV_CK_HALVES 104 /* SED_CK_HALVES: parts of a checkpoint batch, 1..4; unset = -1 (2 parts) */
int sed_plan_routes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                    int del_is_int, const int32_t *options, int noptions,
                    const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                    const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                    int32_t npairs, uint32_t flags, double *out, int nout);
/* The launches of one run of that batch, without a device: the planner's schedule, which sed_batch_run executes step by
 * step.  cut_on / cut_win = the cutoff state sed_batch_set_cutoff left the batch in (a cutoff is set; its wave pairs run
 * the windowed stripe kernel); a state no batch of this plan can be in is SED_E_ARG.  out receives up to max_steps rows
 * of 6: launcher (0 windowed cutoff forward, 1 packed forward, 2 CHAIN, 3 integer stripe forward, 4 checkpoint codes,
 * 5 fp64, 6 fp64 segments, 7 lane, 8 cutoff filter, 9 checkpoint traceback, 10 per-cell-code traceback,
 * 11 stripe-parallel traceback, 12 segment traceback), phase (0 DP, 1 traceback), stream (0 the run's DP stream, 1 the
 * traceback stream, 2 the part's stream), part, and whether the launch carries its part's start / end event of the
 * phase.  info (or null) receives: whether untimed runs record events too, the event of a buffer slot's previous run
 * the next one waits for (0 none, 1 DP end, 3 traceback end), the parts, and the most steps a schedule holds.
 * Returns the number of steps or the SED_E_* code sed_plan_routes would return. */
int sed_plan_schedule(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                      int del_is_int, const int32_t *options, int noptions,
                      const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                      const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                      int32_t npairs, uint32_t flags, int cut_on, int cut_win, int32_t *out, int max_steps,
                      int32_t *info);
int sed_batch_dot_keys(const sed_batch *b);           /* bit 0: the checkpoint forward kernel runs dot keys, bit 1: the
                                                         CHAIN kernel runs ladder dot keys (SED_OPT_DOT), bit 2: over
                                                         the wide ladder (L unit 16) */
/* Band pruning (SED_OPT_BAND).  The three functions below are for tests and diagnostics only: they restate the shared
 * bound without a device, and no caller of the engine needs them.
 * sed_band_bounds: out[0..1] = the lowest and highest diagonal e = j - i an optimal path of an n x m pair can touch when
 *   some path costs ub: e <= (ub + delete (m - n)) / (insert + delete), -e <= (ub - insert (m - n)) / (insert + delete).
 * sed_band_chunk_range: out[0..1] = the first and last 64-step chunk stripe `stripe` (64 rows_per_lane rows) runs for
 *   that window, out[2] = the chunks of an unpruned stripe.  A stripe starts at column 64 out[0] + 1.
 * sed_band_cells: the cells the forward computes for one pair of codes 0..3 under the 4 x 4 table sub (a -> b,
 *   row-major), with ub = the cost of the plain diagonal path; negative on bad arguments.
 * sed_batch_band_cells: the same summed over the batch's pairs (= sum n*m when the batch is not pruned).  It restates the
 *   static windows on the host, so for a batch with refined windows it is an upper estimate.
 * sed_band_refine_row: the refinement of one stripe, as the forward kernel does it.  drow[j] = the cost of some path to
 *   cell (stripe * 64 rows_per_lane, j) for j = 0..m (only the columns the stripe above computed, 64 clo_prev + 1 ..
 *   min(m, 64 chi_prev + 1), are read); ub_prev = the bound so far, suf = the plain diagonal's cost from (r0, r0) to the
 *   sink, negative where r0 > min(n, m).  out[0..1] = the stripe's chunk range, out[2] = the new bound, out[3] = 1 when a
 *   cell survived (else the static range of the new bound).
 * sed_batch_band_chunks_run: after a finished run of a band-pruned batch, the 64-step chunks its forward ran, summed
 *   over the stripes of its wave pairs from the ranges the kernel stored; *total (if not null) = the chunks of the same
 *   stripes unpruned.  Negative when the batch is not band-pruned or has not run. */
int sed_band_refine_row(int32_t n, int32_t m, int32_t rows_per_lane, double ins, double del, int32_t stripe,
                        double ub_prev, double suf, const int32_t *drow, int32_t clo_prev, int32_t chi_prev,
                        int32_t *out);
double sed_batch_band_chunks_run(sed_batch *b, double *total);
int sed_band_bounds(int32_t n, int32_t m, double ins, double del, double ub, int32_t *out);
int sed_band_chunk_range(int32_t n, int32_t m, int32_t rows_per_lane, int32_t elo, int32_t ehi, int32_t stripe,
                         int32_t *out);
double sed_band_cells(const double *sub, double ins, double del, const uint8_t *codes_a, int32_t n,
                      const uint8_t *codes_b, int32_t m, int32_t rows_per_lane);
double sed_batch_band_cells(const sed_batch *b);
/* Bounded search: a cutoff on the distances of a distance-only batch (no SED_WANT_SCRIPT: SED_E_ARG), for the runs that
 * follow.  Valid on a created batch before any run or between runs (a run in flight is waited for, as a refill does);
 * calling it again changes the cutoff of later runs on the same resident batch, with no upload of the inputs.
 * max_dist = +inf turns the cutoff off: every kernel choice and result is then what the batch gives without one.  NaN
 * or a negative value: SED_E_ARG.  With cutoff T, on every route and in every mode:
 *   - a pair whose distance D <= T reports exactly what it reports without a cutoff (out_dist, out_is_int, and out_len
 *     where the batch computes it);
 *   - a pair with D > T reports out_dist = +inf, out_is_int = 0, out_len = -1;
 *   - "<=" is exact: in integer mode (sed_batch_mode = SED_MODE_I32, every distance an integer) T is floored and
 *     clamped to the key range (65535), in the fp64 modes the fp64 values are compared.
 * Integer SED_NO_LEN batches of wave pairs (R = 4, 8, 16, not SPLIT, substitution costs >= 0, insert + delete > 0) may
 * then run only the cells a path of cost <= T can reach (the window of SED_OPT_BAND under ub = min(T, diagonal bound),
 * from the device in every run; a pair whose length difference alone costs more than T runs nothing), see
 * SED_OPT_CUT; every other route computes as before and only compares.  sed_batch_band_cells reports the cells the
 * forward computes under the current cutoff (sed_batch_work keeps the nominal sum n*m), sed_batch_chains and
 * sed_batch_packed_pairs the routes the wave pairs run under it. */
int sed_batch_set_cutoff(sed_batch *b, double max_dist);
/* The number of pairs within the cutoff in the last run (waits for it; every pair when that run had no cutoff), without
 * a download of the distances. */
int sed_batch_cutoff_hits(sed_batch *b, int32_t *within);
int sed_batch_traceback_mode(const sed_batch *b);     /* 0 no script, 1 per-cell codes, 2 checkpoints (SED_OPT_TB),
                                                         3 per-cell codes walked stripe-parallel (<= 64 pairs, R = 4),
                                                         4 SPLIT checkpoints recomputed into per-cell codes
                                                         (SED_OPT_SPLITCK), walked as 3 or 1 */
/* CHAIN diagnostics of the last run (waits for it): pairs handed out by the dynamic-CHAIN device counter, and
 * the most pairs one wave computed back to back (0 when CHAIN mode is off). */
int sed_batch_chain_stats(sed_batch *b, int32_t *fetched, int32_t *max_per_wave);
int sed_batch_run(sed_batch *b);                      /* enqueue on the batch's streams (SED_PIPELINE), returns at once */
int sed_batch_sync(sed_batch *b);                     /* wait for the last run (every stream the batch uses) */
/* Forward launches per run: a checkpoint batch of >= 2048 wave pairs runs in parts on as many streams
 * (SED_CK_HALVES = parts, default 2, >= 1024 wave pairs each), else 1.  With parts, the run times below are the mean
 * launch over the parts (the launches overlap each other's kernels); part 0's DP window includes the lane kernel
 * of the batch's short pairs, if any. */
int sed_batch_dp_launches(const sed_batch *b);
/* device time of the last run, from HIP events on the launching stream(s) (ms; with parts the mean over them) */
int sed_batch_last_times(const sed_batch *b, float *dp_ms, float *traceback_ms);
/* Device times of every run since the last sed_batch_reset_times (waits for them):
 * dp_ms[i] / traceback_ms[i] for run i; returns the number of runs reported (<= max_runs). */
int sed_batch_times(sed_batch *b, float *dp_ms, float *traceback_ms, int max_runs);
/* The same runs as intervals (waits for them): out[(i * parts + p) * 4 + k] for run i, part p
 * (parts = sed_batch_dp_launches), k = {DP start, DP end, traceback start, traceback end} in ms from the DP start of
 * the first run since sed_batch_reset_times (traceback fields 0 without SED_WANT_SCRIPT).  The union of the DP
 * intervals is the time some forward kernel ran, which overlapping parts do not double-count.  Returns the number
 * of runs reported (<= max_runs). */
int sed_batch_spans(sed_batch *b, float *out, int max_runs);
int sed_batch_reset_times(sed_batch *b);
/* Timing events on the batch's kernels: every = 1 on every run (default), k > 1 on every k-th run, 0 never.  Untimed
 * runs are left out of sed_batch_times / _spans / _last_times (SED_E_STATE when the last run was untimed).  Pipelined
 * batches that order buffer reuse through their events keep them on every run. */
int sed_batch_set_timing(sed_batch *b, int every);
int sed_batch_results(sed_batch *b, double *out_dist, uint8_t *out_is_int, int32_t *out_len,
                      uint32_t *out_ops, const int64_t *ops_off);
/* Device pointers of the result arrays (for an RCCL gather); any may be NULL.  Call sed_batch_sync first: the
 * pointers are not ordered after the batch's streams. */
int sed_batch_device_results(const sed_batch *b, uint64_t *d_dist, uint64_t *d_is_int,
                             uint64_t *d_len, uint64_t *d_ops, uint64_t *ops_words);
/* Copy dist (f64[npairs]), len (i32[npairs]) and the packed scripts (u32[ops_words]) of the last
 * run into caller device memory (e.g. tensors an RCCL gather sends); any pointer may be 0. Blocking. */
int sed_batch_export(sed_batch *b, uint64_t d_dist, uint64_t d_len, uint64_t d_ops);
/* Algorithmic counts of one run: DP cells (sum n*m, nominal: pruned cells count too) and HBM bytes (inputs +
 * traceback + outputs; with band pruning the checkpoints of the chunks that run). */
int sed_batch_work(const sed_batch *b, double *cells, double *algo_bytes);

/* Fit search (an extension; the reference has no such function): the best approximate occurrence of a short pattern
 * in each text, blocking, under the costs of sed_set_costs.
 * Pair q: pattern p = codes_p[off_p[q] .. +len_p[q]) of length P, 1 <= P <= 32, text t = codes_t[off_t[q] .. +len_t[q])
 * of length n >= 0; pairs may share patterns and texts through the offsets (Q queries x D documents with one copy of
 * each).  G(s, e) = the distance wagnerFisher(p, t[s:e]) gives (str1 = the pattern, str2 = the substring, the direction
 * of wf_score(query, doc)).  The hit of a pair is (dist, start, end):
 *   dist  = min over 0 <= s <= e <= n of G(s, e)  (the empty substring is allowed, so dist <= P * delete);
 *   end   = the smallest e for which some s gives dist;
 *   start = the largest s with G(s, end) = dist   (the tightest window ending earliest).
 * It is the sink scan of the DP with borders D[0][j] = 0, D[i][0] = i * delete and the reference's recurrence, every
 * cell carrying (D, -s) as one lexicographic key: the first strict minimum of row P over j.
 * Cost models served (anything else: SED_E_RANGE, the text says which condition failed; this call has no fallback of
 * its own: sed_fit_search_f64 below serves what it refuses, and sed_fit_route says which of the two serves a search):
 *   at most 8 symbols (K <= 8); some S = 2^k, k <= 8, makes insert, delete and every substitution cost an integer in
 *   0..255 with (insert + delete) * S <= 255 and P * delete * S <= 65535; a lane's text columns fit 16 bits (a text runs
 *   in chunks of at most 65535 - W columns, W = P + floor(P * delete / insert); with insert = 0 a text runs as one
 *   chunk, n <= 65534).  For such tables every fp64 sum of the reference is exact, so out_dist = D / S equals the sink
 *   value of wagnerFisher(p, t[start:end]) as a number.  No is_int is reported: callers who need the typed value or
 *   the script run the window through sed_run_batch.
 * Errors: SED_E_ARG (NULL, negative length, a code >= K), SED_E_STATE (no costs set, or a pair in flight after
 * sed_pair_submit), SED_E_RANGE as above.  SED_OPT_FIT_CHUNK sets the chunk length. */
int sed_fit_search(sed_ctx *ctx,
                   const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                   const uint8_t *codes_t, const int64_t *off_t, const int32_t *len_t,
                   int32_t npairs, double *out_dist, int32_t *out_start, int32_t *out_end);
/* What sed_fit_search would decide, without a device: the code it would return for these costs (as sed_set_costs takes
 * them), options (as sed_plan_routes takes them) and lengths, and out[0 .. nout) = 0 the scale S, 1 W (-1 when
 * insert = 0), 2 the chunk length (0 = one lane per text), 3 lanes, 4 cells computed (P x columns, warm-up included),
 * 5 nominal cells (sum P * n). */
int sed_fit_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                 double del, int del_is_int, const int32_t *options, int noptions,
                 const int32_t *len_p, const int32_t *len_t, int32_t npairs, double *out, int nout);
/* The lane records sed_fit_search would run for the same arguments, without a device (for tests and tools): one lane
 * per (pair, chunk of text columns), pair by pair in chunk order, lanes as sed_fit_plan counts them.
 * out_lanes = eight 32-bit words per lane, room for max_lanes lanes (SED_E_ARG when there are more):
 *   0 tw      the lane's border column, in 4-symbol words from the start of the pair's own text (the search adds the
 *             word at which its copy of the text starts)
 *   1 pair    2 pat  0 here (the search sets the pattern's record)    3 plen  the pattern's length P
 *   4 nsteps  text columns the lane runs after its border column (the kernel rounds it up to a multiple of 4)
 *   5 lead    columns before c0 that only warm the lane up          6 cnt   columns it owns, [c0, c0 + cnt)
 *   7 c0      its first owned column (column j = the DP column after j text symbols; column 0 is the border)
 * out_params = 18 words: the update addends insert + delete - min(cost(a -> b), insert + delete) on the integer scale,
 * one byte each, b = 0..3 in word 2a and b = 4..7 in word 2a + 1 for a = 0..7, then insert * S and delete * S. */
int sed_fit_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                  double del, int del_is_int, const int32_t *options, int noptions,
                  const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                  int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params);
/* Device time of the last sed_fit_search's kernel, from HIP events (ms); SED_E_STATE before the first search. */
int sed_fit_last_time(const sed_ctx *ctx, float *kernel_ms);

/* Fit search over a resident index: the texts of a collection are packed and uploaded once, and every search sends
 * only its queries.  A sed_fit_index belongs to the context it was created on (several may live on one context, beside
 * its batches; each owns its device buffers and its pinned result buffer) and must be destroyed before the context.
 * sed_fit_index_create: text d = codes_t[off_t[d] .. +len_t[d]), every text copied (4-byte aligned, as sed_fit_search
 * lays them out).  It needs no cost model: the index keeps the texts' lengths and the largest code it saw, and every
 * search runs under the context's costs of that moment, so costs and options may change between searches.  ntexts = 0
 * is valid.  NULL on failure, with the reason in sed_last_error(ctx): SED_E_ARG conditions (NULL, a negative length or
 * offset), more than 16 GB of text, an allocation or a copy that failed. */
typedef struct sed_fit_index sed_fit_index;
sed_fit_index *sed_fit_index_create(sed_ctx *ctx, const uint8_t *codes_t, const int64_t *off_t, const int32_t *len_t,
                                    int32_t ntexts);
void sed_fit_index_destroy(sed_fit_index *ix);
int32_t sed_fit_index_texts(const sed_fit_index *ix);    /* the number of texts */
int64_t sed_fit_index_symbols(const sed_fit_index *ix);  /* the sum of their lengths */
/* Every query against every text, blocking, in one launch (65535 queries per launch; more run as further launches of
 * the same call): query q = codes_p[off_p[q] .. +len_p[q]), and out_*[q * ntexts + d] = the hit (dist, start, end) of
 * (query q, text d) as sed_fit_search defines it.  The hits equal, bit for bit, what sed_fit_search returns for the
 * nqueries x ntexts pairs listed query-major under the same costs and the same chunk length: the plan is that batch's
 * plan (sed_fit_index_plan), and every lane runs the same DP on the same columns.  The cost models served and the
 * refusals are sed_fit_search's, decided per search before anything is launched: SED_E_RANGE with the failed condition
 * in the text, SED_E_ARG (NULL, a negative length or offset, a query code >= K, or an index that holds a text code >= K
 * under the current costs), SED_E_STATE (no costs set, or a pair in flight after sed_pair_submit).  A refused search
 * leaves the index usable.  SED_OPT_FIT_CHUNK sets the chunk length as for sed_fit_search.  The host work of a search
 * grows with the queries and the results, never with the texts' bytes; the per-(text, chunk) table on the device is
 * rebuilt only when the chunk length differs from the last search's. */
int sed_fit_index_search(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                         int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end);
/* Device time of the last sed_fit_index_search's kernel(s), from HIP events (ms); SED_E_STATE before the first search
 * that launched one. */
int sed_fit_index_last_time(const sed_fit_index *ix, float *kernel_ms);
/* What sed_fit_index_search would decide, without a device: sed_fit_plan's code and out[] for the nqueries x ntexts
 * cross product (pair q * ntexts + d = query q, text d), computed from the queries' lengths and sums over the texts. */
int sed_fit_index_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                       double del, int del_is_int, const int32_t *options, int noptions,
                       const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts, double *out, int nout);
/* The lane records sed_fit_index_search would run, without a device (for tests and tools): each from the index's
 * (text, chunk) table and the function the kernel derives its lane with, query-major, then in the table's order (text
 * by text, chunk by chunk).  out_lanes and out_params as sed_fit_lanes lays them out, pair = q * ntexts + d. */
int sed_fit_index_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                        double del, int del_is_int, const int32_t *options, int noptions,
                        const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts,
                        int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params);

/* Every occurrence within a distance, not only the best one.  Pattern p, text t of length n and G(s, e) as for
 * sed_fit_search.  For each end column 0 <= e <= n:
 *   E(e) = min over 0 <= s <= e of G(s, e);
 *   S(e) = the largest s that reaches it: the (D, -start) key of row P at column e, exactly as sed_fit_search defines it.
 * The hits of (p, t) within T are all (e, S(e), E(e)) with E(e) <= T.  Column 0 is a column: E(0) = P * delete, S(0) = 0.
 * A hit is decided per column and depends on nothing but that column's key, so the chunk length cannot change the set
 * (on the columns a lane owns its keys are the full matrix's).  sed_fit_search's hit of the pair is the hit of smallest
 * (dist, end) whenever its distance is <= T.
 * sed_fit_index_hits: every query against every text of the index, blocking, under sed_fit_index_search's plan, lanes,
 * cost models, refusals and state errors (and its 65535 queries per launch); max_dist = T >= 0, +inf meaning every
 * column, NaN or negative: SED_E_ARG.  dist = D / S as the search decodes it; a distance is within T exactly when
 * D <= floor(T * S).
 *   *found = the total number of hits, always (when the call returns SED_OK or SED_E_RANGE for lack of room).
 *   found <= cap: out[0 .. found) = all hits sorted by (query, text, end), which are unique keys; SED_OK.
 *   found > cap:  nothing in out is promised; SED_E_RANGE, the text names found and cap.  The index stays usable: call
 *                 again with room.  cap = 0 with out = NULL is a count query.
 * The device hit list belongs to the index, grows to the largest cap seen and is apart from the search's result buffer:
 * searches and hits searches on one index may alternate. */
typedef struct { int32_t query, text, start, end; double dist; } sed_fit_hit;
int sed_fit_index_hits(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                       int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found);
/* Device time of the last sed_fit_index_hits' kernel(s), from HIP events (ms); SED_E_STATE before the first that
 * launched one. */
int sed_fit_index_hits_last_time(const sed_fit_index *ix, float *kernel_ms);
/* The cutoff on the integer scale, without a device: the code sed_fit_plan returns for these arguments, else SED_E_ARG
 * for a NaN or negative max_dist, else *out = min(floor(max_dist * S), 65535) under the plan's scale S (no scaled
 * distance exceeds P * delete * S <= 65535, so 65535 admits every column; the kernel takes each query's own
 * P * delete * S from it). */
int sed_fit_cutoff_scaled(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                          double del, int del_is_int, const int32_t *options, int noptions,
                          const int32_t *len_p, const int32_t *len_t, int32_t npairs, double max_dist, int64_t *out);

/* Long patterns: sed_fit_index_search and sed_fit_index_hits for 1 <= P <= 2048 (pre-miRNA hairpins, tRNAs, riboswitches,
 * short transcripts).  The definition, arguments, results, errors, cap protocol and the index are those of the two calls
 * above; the hits of a query of P <= 32 equal theirs bit for bit.  What differs is the kernel: one wave runs one (query,
 * chunk of a text), the pattern's rows spread over its 64 lanes, R = 2, 4, 8, 16 or 32 rows a lane (the smallest with
 * 64 R >= P; SED_OPT_FIT_ROWS forces one R for every query of a call), and the queries of a call run grouped by R, one
 * launch per group and 65535 queries.  The cost models served (anything else: SED_E_RANGE, the text says which condition
 * failed; the _long_f64 calls below serve what these refuse, and sed_fit_long_route says which of the two serves a search):
 *   at most 8 symbols; some S = 2^k, k <= 8, makes every cost an integer in 0..255 with (insert + delete) * S <= 255;
 *   P * delete * S + 128 * insert * S <= 65535 over the call's longest pattern (distance and the 128 columns of insert a
 *   key carries between rebases share one 16-bit field);
 *   a wave's text columns fit 16 bits: a text runs in chunks of at most 65535 - W - 3 columns, W = P + floor(P * delete /
 *   insert) over the call's longest pattern (so chunk + W + 3 <= 65535; the 3 is the alignment of a wave's first column
 *   to a 4-symbol word); with insert = 0 a text runs as one chunk, n <= 65534.
 * The automatic chunk length follows sed_fit_search's rule with waves in place of lanes.  SED_OPT_FIT_CHUNK forces it.
 * sed_fit_search, sed_fit_index_search and sed_fit_index_hits keep refusing P > 32.
 * sed_fit_index_last_time / sed_fit_index_hits_last_time report the last search / hits search of either kind. */
int sed_fit_index_search_long(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                              int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end);
int sed_fit_index_hits_long(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                            int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found);
/* What the long calls would decide, without a device: out[] as sed_fit_index_plan lays it out (3 lanes = the waves, one
 * per (query, chunk record); 4 cells = P x the columns a wave's chunk spans, the 63 steps of its skew not counted), and
 * out_rows[q] (may be NULL) = the rows per lane query q runs with. */
int sed_fit_index_long_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                            double del, int del_is_int, const int32_t *options, int noptions,
                            const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts, double *out, int nout,
                            int32_t *out_rows);
/* The wave records of that plan, without a device: what sed_fit_index_lanes gives for the plan's chunk length (each
 * wave derives its record as a lane of the short kernels does), in query order whatever the grouping. */
int sed_fit_index_long_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                             double del, int del_is_int, const int32_t *options, int noptions,
                             const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts,
                             int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params);

/* The fp64 route: sed_fit_search, sed_fit_index_search and sed_fit_index_hits for the cost tables and alphabets their
 * integer keys refuse.  Arguments, results, state errors, the cap protocol and the index are those of the three calls
 * above; the index is used as it stands, so integer and fp64 searches may alternate on one index.  What differs:
 *   cost models served: at most 16 symbols (K <= 16; more: SED_E_RANGE, the text names the bound); insert, delete and
 *   every substitution cost finite and >= 0 (a negative cost: SED_E_RANGE, the text names it; -0.0 counts as +0.0);
 *   1 <= P <= 32 (the _long_f64 calls below: 1 <= P <= 2048).  No scale, no byte ranges, and no limit on a text's columns (starts are 32 bits): any int32 length.
 *   The definition met is sed_fit_search's, evaluated as oracle/sed_oracle.c: sed_oracle_fit_pair states it: every
 *   candidate of a cell is ONE fp64 add (left + insert, up + delete, diagonal + cost), borders D[0][j] = 0 and
 *   D[i][0] = (double)i * delete, every cell the lexicographic minimum of (D, -start), the hit the first strict
 *   minimum of row P.  out_dist / sed_fit_hit.dist is that fp64 value itself, bit for bit, whatever the chunk length:
 *   for tables whose sums are not exact in fp64 this is the value of that one fixed order of additions.
 *   A hit of sed_fit_index_hits_f64 is a column with E(e) <= max_dist as fp64 numbers; there is no scaled cutoff.
 *   On tables the integer calls serve, the results of the two routes are equal bit for bit (every sum is exact).
 *   A text runs in chunks as in sed_fit_search, the lanes warming up over W = P + floor(P * delete / insert) + 2
 *   columns (DESIGN.md 3.6i proves the owned columns exact under rounding); with insert = 0, costs outside
 *   2^-900 .. 2^900 or P * delete / insert above 2^20 every text runs as one lane.  SED_OPT_FIT_CHUNK as before.
 * sed_fit_last_time, sed_fit_index_last_time and sed_fit_index_hits_last_time report the last search of either kind
 * (the fp64 times include the small kernel that reduces the lanes' records per pair).  A refused call leaves the
 * context and the index usable. */
int sed_fit_search_f64(sed_ctx *ctx,
                       const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                       const uint8_t *codes_t, const int64_t *off_t, const int32_t *len_t,
                       int32_t npairs, double *out_dist, int32_t *out_start, int32_t *out_end);
int sed_fit_index_search_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                             int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end);
int sed_fit_index_hits_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                           int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found);
/* What the fp64 calls would decide, without a device: out[] as sed_fit_plan / sed_fit_index_plan lay it out, with
 * 0 = 0 (no scale: fp64), 1 W (-1: one lane per text), and 6 = why every text runs as one lane: 0 it does not have to,
 * 1 insert = 0, 2 the window argument's conditions on the costs fail.  The lanes are the eight-word records of
 * sed_fit_lanes / sed_fit_index_lanes (there are no parameter words). */
int sed_fit_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                     double del, int del_is_int, const int32_t *options, int noptions,
                     const int32_t *len_p, const int32_t *len_t, int32_t npairs, double *out, int nout);
int sed_fit_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                      double del, int del_is_int, const int32_t *options, int noptions,
                      const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                      int32_t *out_lanes, int64_t max_lanes);
int sed_fit_index_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                           double del, int del_is_int, const int32_t *options, int noptions,
                           const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts, double *out, int nout);
int sed_fit_index_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                            double del, int del_is_int, const int32_t *options, int noptions,
                            const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts,
                            int32_t *out_lanes, int64_t max_lanes);
/* Which route serves the search sed_fit_plan's arguments describe, without a device: SED_FIT_ROUTE_INT (sed_fit_search
 * serves it; it is preferred whenever it does), SED_FIT_ROUTE_F64 (only sed_fit_search_f64 does; why = the integer
 * route's refusal text), or the negative code both fail with (why = both texts, "; " between them).  why (room for
 * why_len bytes, may be NULL with 0) is always terminated. */
#define SED_FIT_ROUTE_INT 0
#define SED_FIT_ROUTE_F64 1
int sed_fit_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                  double del, int del_is_int, const int32_t *options, int noptions,
                  const int32_t *len_p, const int32_t *len_t, int32_t npairs, char *why, int why_len);

/* The fp64 route for long patterns: sed_fit_index_search_long and sed_fit_index_hits_long for the cost tables and
 * alphabets their integer keys refuse, i.e. the _f64 calls above for 1 <= P <= 2048.  Arguments, results, state errors,
 * the cap protocol and the index are those of the _long calls; integer, fp64, long and long-fp64 searches may alternate
 * on one index.  The kernel is the long calls' wave (one per (query, chunk of a text), R = 2 .. 32 rows a lane, the
 * smallest with 64 R >= P, SED_OPT_FIT_ROWS forcing one; one launch per R group and 65535 queries) running the fp64
 * calls' cell: every candidate ONE fp64 add, the (D, -start) minimum, no scale, 32-bit starts.  So the results are the
 * oracle's values bit for bit; a query of P <= 32 gives what sed_fit_index_search_f64 / sed_fit_index_hits_f64 give, and
 * on a table the _long calls serve the results equal theirs, bit for bit.  Envelope: K <= 16, every cost finite and >= 0,
 * 1 <= P <= 2048 over the call; anything else is SED_E_RANGE and the text names the bound or the cost.  Chunks: the
 * _long calls' rule (waves for lanes), never below W = P + floor(P * delete / insert) + 2 over the call's longest
 * pattern; with insert = 0, costs outside 2^-900 .. 2^900 or P * delete / insert above 2^20 every text runs as one wave
 * (DESIGN.md 3.6j).  SED_OPT_FIT_CHUNK forces the chunk.  sed_fit_index_last_time / sed_fit_index_hits_last_time report
 * these calls too (the search's time includes the reduce kernels).  A refused call leaves the context and the index
 * usable. */
int sed_fit_index_search_long_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                                  int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end);
int sed_fit_index_hits_long_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                                int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found);
/* What the long fp64 calls would decide, without a device: out[] as sed_fit_index_f64_plan lays it out (3 lanes = the
 * waves; 6 = why every text runs as one wave), out_rows[q] (may be NULL) as sed_fit_index_long_plan; and the wave
 * records, as sed_fit_index_f64_lanes lays them out (for P <= 32 and the same chunk length they are its records). */
int sed_fit_index_long_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                                double del, int del_is_int, const int32_t *options, int noptions,
                                const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts, double *out,
                                int nout, int32_t *out_rows);
int sed_fit_index_long_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                                 double del, int del_is_int, const int32_t *options, int noptions,
                                 const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts,
                                 int32_t *out_lanes, int64_t max_lanes);
/* sed_fit_route for the long calls, over sed_fit_index_long_plan's arguments: SED_FIT_ROUTE_INT whenever
 * sed_fit_index_search_long serves the search, SED_FIT_ROUTE_F64 when only sed_fit_index_search_long_f64 does (why = the
 * integer route's refusal), else the negative code both fail with (why = both texts, "; " between them). */
int sed_fit_long_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                       double del, int del_is_int, const int32_t *options, int noptions,
                       const int32_t *len_p, int32_t nqueries, const int32_t *len_t, int32_t ntexts, char *why, int why_len);

/* Similarity join (an extension; it batches what the reference does pair by pair: wf_score(query, doc) over a whole
 * collection, IRMethods.py:435-440 inside search_collection's loop, IRMethods.py:443-477, each a full
 * wagnerFisher(str1, str2), StringEditDistance.py:133-224): every (row, column) pair of short sequences with
 * wagnerFisher(row, column).value <= max_dist, as a compact sorted hit list; the pairs are enumerated on the device.
 * Rows are str1 and columns str2 (the direction of wf_score(query, doc)); cost tables may be asymmetric, so (i, j) and
 * (j, i) are different pairs.
 * A sed_join_index holds nseqs sequences of 0..32 symbols each, resident on the device: sequence i = codes[off[i] ..
 * +len[i]).  It needs no cost model (it keeps the sequences, their lengths and a 32-bit mask of the codes it holds; its
 * columns are stored sorted by length, and hits carry the original indices); every call runs under the context's costs
 * and options of that moment.  It belongs to its context and is destroyed before it.  nseqs = 0 is valid.  NULL on
 * failure, the reason in sed_last_error(ctx): SED_E_ARG conditions (NULL, a length above 32, a negative length or
 * offset), an allocation or a copy that failed.
 *   sed_join_self:   rows = the index's own sequences row_lo <= i < row_hi, columns = every sequence j != i.  (i, i) is
 *                    never reported; duplicates (i != j, equal sequences) are, in both directions.
 *   sed_join_search: rows = nqueries host sequences of 0..32 symbols, columns = every sequence of the index; nothing is
 *                    excluded.
 * Hits: dist = D / S, the scaled-integer lane kernel's number (no is_int, as for fit search); a pair is within max_dist
 * exactly when D <= floor(max_dist * S); +inf admits every pair (the dense matrix as a hit list); NaN or a negative
 * max_dist: SED_E_ARG.  Empty sequences are ordinary: their distances are n * delete and m * insert.
 * The cap protocol is sed_fit_index_hits': *found = the total, always; found <= cap: out[0 .. found) sorted by (row, col),
 * SED_OK; found > cap: SED_E_RANGE, the text names both numbers, the index stays usable; cap = 0 with out = NULL is a count
 * query.  The device hit list belongs to the index and grows to the largest cap seen.
 * Cost models served (anything else: SED_E_RANGE before any launch, the text names the failed condition, the index stays
 * usable): at most 8 symbols; some S = 2^k, k <= 8, makes insert, delete and every substitution cost an integer;
 * insert * S and delete * S >= 1; every cost <= insert + delete; (insert + delete) * S <= 255.  For such tables every fp64
 * sum of the reference is exact, so D / S is the reference's value bit for bit.  A row or column code >= K: SED_E_ARG.
 * State errors: sed_fit_index_search's.
 * One kernel variant per launch (sed_join_plan's out[1]): bit-parallel when insert = delete = 1 and the codes present
 * (the index's, OR'd with the queries' for a search) are at most four symbols with unit costs among themselves, else the
 * scaled DP; SED_OPT_JOIN_DP forces the DP.  A pair whose length bound insert * (m - n)+ + delete * (n - m)+ exceeds
 * max_dist is never computed, and a wave whose 64 columns all fail it skips the row.  More rows than one launch takes
 * (65535 groups of sed_join_rows_per_group rows; SED_OPT_JOIN_ROWS) run as further launches of the same call.
 * Not served: tables the conditions refuse (IUPAC: the _f64 calls below serve them), sequences over 32 symbols (the
 * sed_join_long_ calls below serve up to 128), edit scripts of the hits, the i < j half alone for symmetric tables, a
 * per-tile mix of the two variants; of the k-nearest calls below: k > 64. */
typedef struct sed_join_index sed_join_index;
typedef struct { int32_t row, col; double dist; } sed_join_hit;
sed_join_index *sed_join_index_create(sed_ctx *ctx, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                      int32_t nseqs);
void sed_join_index_destroy(sed_join_index *ix);
int32_t sed_join_index_seqs(const sed_join_index *ix);
int sed_join_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                  int64_t *found);
int sed_join_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                    int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
/* Device time of the last join's kernel(s), from HIP events (ms); SED_E_STATE before the first that launched one. */
int sed_join_last_time(const sed_join_index *ix, float *kernel_ms);
/* The pairs the last join's waves ran (those in scope whose length bound passed), counted on the device: equal to
 * sed_join_plan's out[4] for the same call.  SED_E_STATE before the first join that got past its plan. */
int sed_join_pairs_run(const sed_join_index *ix, int64_t *pairs);
/* The rows a block's waves run against their columns (the row side of the launch geometry). */
int32_t sed_join_rows_per_group(void);
/* What a join would decide, without a device: the code it would return for these costs (as sed_set_costs takes them),
 * options (as sed_plan_routes takes them), lengths, codes seen (bit c set when code c occurs; bit 31: any code >= 31) and
 * cutoff; self != 0: the rows are nrows of the ncols columns and each row's own column is out of scope.
 * out[0 .. nout) = 0 the scale S, 1 the kernel (1 DP, 2 bit-parallel), 2 waves launched, 3 pairs in scope, 4 pairs the
 * waves run (after the length skip), 5 the cells n * m of those pairs. */
int sed_join_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                  double del, int del_is_int, const int32_t *options, int noptions,
                  const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                  uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout);

/* The k nearest columns of every row (an extension; it batches the same reference lines as the join: wf_score(query,
 * doc) over a whole collection, IRMethods.py:435-440 inside search_collection's loop, IRMethods.py:443-477, each a full
 * wagnerFisher(str1, str2), StringEditDistance.py:133-224, followed by the sort that shows the best few): for every row
 * in the scope of sed_join_self / sed_join_search, the k columns of smallest distance, exact and deterministic, through
 * the integer route's kernels (both variants).
 *   Scope: sed_join_self's or sed_join_search's; a self join never reports (i, i); duplicates are ordinary columns.
 *   Order within a row: by (scaled distance D, original column index); the result is the first min(k, the in-scope
 *   columns with D <= floor(max_dist * S)) of them.  max_dist = +inf: no cap; NaN or negative: SED_E_ARG.
 *   k = 1..64 (a wave selects among its 64 lanes); anything else: SED_E_ARG, the text names k.
 *   out: sed_join_hit records sorted by (row, dist, col): each row's neighbours together, nearest first; dist = D / S as
 *   for the join, the reference's wagnerFisher(...).value bit for bit for the tables served.
 * Everything else is the integer join's: the cap protocol (*found = the records of the result, always set; SED_E_RANGE
 * names both numbers; cap = 0 with out = NULL counts; the index stays usable), the state errors, the cost models served
 * and the order of refusals (k is checked with the arguments), a code >= K: SED_E_ARG, SED_OPT_JOIN_DP,
 * SED_OPT_JOIN_ROWS and the 65535-group limit handled by further launches.
 * Two passes over the rows, no wave waits for another: pass 1 keeps a bound for every row, starting at floor(max_dist * S)
 * and lowered to the k-th smallest distance any wave of 64 columns finds among its own; pass 2 is the join with the row's
 * bound as the cutoff, so it appends the k nearest and every tie at the k-th place, at most what sed_join_self appends at
 * max_dist; the host keeps each row's first k (sed_join_knn_trim).  The device list is sized for the untrimmed candidates
 * and grows when pass 2 overflows it (pass 2 then runs once more).
 * sed_join_last_time and sed_join_pairs_run report these calls too: the device time from the first pass 1 to the last
 * pass 2 (a second pass 2 and the wait before it included), and the pairs both passes ran (a second pass 2 not counted). */
int sed_join_knn_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist, sed_join_hit *out,
                      int64_t cap, int64_t *found);
int sed_join_knn_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
/* The last k-nearest call's per-row bounds after pass 1, on the integer scale (D * S): bounds[i] belongs to row row_lo + i
 * (query i), n = the call's rows exactly (else SED_E_ARG).  A call that launched nothing (no rows, or no columns) reports
 * floor(max_dist * S), clamped to 65535, for every row.  SED_E_STATE before the first k-nearest call that got past its
 * plan, and when the last such call was an fp64 one (sed_join_knn_bounds_f64 reports those). */
int sed_join_knn_bounds(const sed_join_index *ix, int32_t *bounds, int32_t n);
/* The hits its pass 2 appended, before the trim.  SED_E_STATE as above. */
int sed_join_knn_candidates(const sed_join_index *ix, int64_t *n);
/* Device time of pass 1 of its first launch (ms); with one launch, the usual case, sed_join_last_time less this is pass 2.
 * SED_E_STATE unless the last call that launched a kernel was a k-nearest one. */
int sed_join_knn_bound_time(const sed_join_index *ix, float *kernel_ms);
/* The trim and the sort alone, in place, without a device: hits[0 .. n) in any order -> sorted by (row, dist, col), each
 * row's first k; *kept = the records left.  k outside 1..64, n < 0, a NULL or a NaN dist: SED_E_ARG. */
int sed_join_knn_trim(sed_join_hit *hits, int64_t n, int32_t k, int64_t *kept);
/* What every join call does with the records it downloads, alone and without a device: validate, convert, order.
 * records = n device records of four 32-bit words (row, col, w0, w1).  route = SED_JOIN_ROUTE_INT: dist = w0 *
 * 2^-scale_log2 (scale_log2 0..8) and cap = the cutoff on the integer scale; SED_JOIN_ROUTE_F64: (w0, w1) are the low and
 * high words of dist, copied, and cap = max_dist.  The call's rows are first_row .. first_row + nrows - 1, the columns
 * 0 .. ncols - 1; self != 0: (i, i) is out of scope.  k = 0: a join, bounds unread, out sorted by (row, col); k = 1..64:
 * a k-nearest call, bounds = its rows' bounds after pass 1 (nrows of them: uint32_t each on the integer route, double on
 * fp64), out = sed_join_knn_trim's.  out has room for n hits; *kept = the hits left.
 * SED_E_ARG: bad arguments.  SED_E_DEVICE: a record no kernel emits - a row outside the call, a column outside the
 * index, (i, i) of a self join, a distance that is NaN, negative, above cap or above its row's bound, or a (row, col)
 * reported twice among the hits left; why (why_len bytes, may be 0) names the record. */
int sed_join_decode(const uint32_t *records, int64_t n, int route, int32_t scale_log2, double cap, int32_t first_row,
                    int32_t nrows, int32_t ncols, int self, int32_t k, const void *bounds, sed_join_hit *out, int64_t *kept,
                    char *why, int why_len);
/* What a k-nearest call would decide, without a device: k, then sed_join_plan's arguments (long_index != 0: those of
 * sed_join_long_plan, with its out[6]).  k outside 1..64: SED_E_ARG before anything else is looked at; then
 * sed_join_plan's refusals in their order.  out[]: the plan of the join at max_dist, which bounds each pass from above.
 * sed_join_knn_plan_error: the text of this thread's last refusal (of this call or of sed_join_knn_f64_plan), "" after a
 * plan that passed. */
int sed_join_knn_plan(int long_index, int32_t k, int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                      double del, int del_is_int, const int32_t *options, int noptions,
                      const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                      uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout);
const char *sed_join_knn_plan_error(void);

/* The fp64 route of the similarity join: sed_join_self / sed_join_search for the cost tables and alphabets their scaled
 * integer cells refuse (the 15-symbol IUPAC table of costs.json among them).  Arguments, hit records, sort order, cap
 * protocol, state errors and error order are those of the integer calls; the index is the same (it stores one code per
 * byte), and calls of either kind may alternate on it.
 * A pair (row, column) is a hit exactly when wagnerFisher(row, column).value (StringEditDistance.py:133-224; the
 * recurrence of lines 143-224 in fp64: row 0 = j * insert, column 0 = i * delete, a cell = min(left + insert, up +
 * delete, diagonal + cost), each one fp64 add) is <= max_dist as a plain fp64 compare, and dist is that double bit for
 * bit: there is no scale, no floor and no offset key.  +inf admits every pair; NaN or a negative max_dist: SED_E_ARG.
 * Cost models served: at most 16 symbols, every cost finite and >= 0 (-0.0 counts as 0; subnormal
 * costs are served and come out as the reference's); anything else is SED_E_RANGE before any launch, and the text names
 * the bound or the cost.  A row or column code >= K: SED_E_ARG.
 * Length skip: the reference's value is a sequentially rounded sum and can lie below the product |m - n| * cost, so a
 * pair of lengths (n, m) is left out only when fl(|m - n| * cost) * (1 - 2^-40) > max_dist (with n, m >= 1, max_dist
 * finite, the product finite and >= 2^-900), or, with n = 0 or m = 0, when the border product itself exceeds max_dist
 * (DESIGN.md 3.6l).  It never drops a pair the reference keeps; it may run pairs the integer route's bound would skip.
 * SED_OPT_JOIN_ROWS splits the rows into launches as for the integer calls; SED_OPT_JOIN_DP does not concern this
 * route.  sed_join_last_time and sed_join_pairs_run report the last call of either kind. */
int sed_join_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                      int64_t *found);
int sed_join_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
/* The k nearest columns of every row on the fp64 route (an extension; it batches the same reference lines as
 * sed_join_knn_self: wf_score(query, doc) over a whole collection, IRMethods.py:435-440 inside search_collection's loop,
 * IRMethods.py:443-477, each a full wagnerFisher(str1, str2), StringEditDistance.py:133-224, followed by the sort that
 * shows the best few): sed_join_knn_self / sed_join_knn_search for the cost tables and alphabets of sed_join_self_f64,
 * on the same sed_join_index; calls of every kind may alternate on one index.
 *   Order within a row: by (D, original column index), D = wagnerFisher(row, column).value in fp64, bit for bit, as
 *   sed_join_self_f64 defines it; the result is the first min(k, the in-scope columns with D <= max_dist as a plain fp64
 *   compare) of them, as records sorted by (row, dist, col).  max_dist = +inf: no cap; NaN or negative: SED_E_ARG; -0.0
 *   counts as 0.  A distance that overflowed to +inf is an ordinary value: reported under max_dist = +inf, ordered last.
 *   k = 1..64, checked with the arguments; then the fp64 join's refusals in the fp64 join's order.
 * The cap protocol, the state errors, SED_OPT_JOIN_ROWS, the 65535-group limit and the device list that grows (pass 2
 * then runs once more) are the integer k-nearest calls'; sed_join_knn_candidates, sed_join_knn_bound_time,
 * sed_join_last_time and sed_join_pairs_run report these calls as they report those.
 * The two passes are the integer calls' on a 64-bit key: every distance of this route is finite or +inf and >= +0, and
 * the bit patterns of such doubles order, as unsigned 64-bit integers, exactly as the values do.  A row's bound is such
 * a pattern (8 bytes a row), starts at max_dist's and is lowered by a 64-bit atomic minimum; nothing is scaled or
 * rounded.  The length skip compares a table entry with the row's bound: low[33 n + m] <= bound (sed_join_f64_lower),
 * the value sed_join_f64_keep compares with max_dist. */
int sed_join_knn_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist, sed_join_hit *out,
                          int64_t cap, int64_t *found);
int sed_join_knn_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                            int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
/* The last fp64 k-nearest call's per-row bounds after pass 1, as doubles: bounds[i] belongs to row row_lo + i (query i),
 * n = the call's rows exactly (else SED_E_ARG).  A call that launched nothing reports max_dist for every row.
 * No bound is negative: a max_dist of -0.0 is reported as +0.0.  SED_E_STATE before the first k-nearest call that got past its plan, and when the last such call was an integer one. */
int sed_join_knn_bounds_f64(const sed_join_index *ix, double *bounds, int32_t n);
/* What an fp64 k-nearest call would decide, without a device: k, then sed_join_f64_plan's arguments.  k outside 1..64:
 * SED_E_ARG before anything else is looked at; then sed_join_f64_plan's refusals in their order.  out[]: the fp64 join's
 * plan at max_dist, which bounds each pass from above.  The refusal's text: sed_join_knn_plan_error. */
int sed_join_knn_f64_plan(int32_t k, int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                          double del, int del_is_int, const int32_t *options, int noptions,
                          const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                          uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout);
/* The table behind the fp64 length skip: low[33 n + m], n, m = 0..32, a value <= every distance of a row of n and a
 * column of m symbols under these costs (finite, >= 0; anything else: SED_E_ARG): the border product when n = 0 or m = 0,
 * fl(p - p 2^-40) for p = fl(|m - n| * cost) when n != m and p is finite and >= 2^-900, else 0.  sed_join_f64_keep's bit
 * (n, m) is low[33 n + m] <= max_dist. */
int sed_join_f64_lower(double ins, double del, double *low);
/* What the fp64 calls would decide, without a device: sed_join_plan's arguments and out[] slots, with 0 = 0 (no scale)
 * and 1 = 3 (the fp64 kernel). */
int sed_join_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                      double del, int del_is_int, const int32_t *options, int noptions,
                      const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                      uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout);
/* The fp64 length skip alone: keep[n], n = 0..32, bit m set when a row of n and a column of m symbols are computed under
 * these costs (finite, >= 0) and cutoff (>= 0 or +inf); anything else: SED_E_ARG. */
int sed_join_f64_keep(double ins, double del, double max_dist, uint64_t *keep);
/* Which route serves the join sed_join_plan's arguments describe, without a device, with sed_fit_route's conventions:
 * SED_JOIN_ROUTE_INT (sed_join_self / sed_join_search serve it; preferred whenever they do), SED_JOIN_ROUTE_F64 (only
 * the _f64 calls do; why = the integer route's refusal text), or the negative code both fail with (why = both texts,
 * "; " between them).  why (room for why_len bytes, may be NULL with 0) is always terminated. */
#define SED_JOIN_ROUTE_INT 0
#define SED_JOIN_ROUTE_F64 1
int sed_join_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                   double del, int del_is_int, const int32_t *options, int noptions,
                   const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                   uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, char *why, int why_len);

/* The similarity join over sequences of 0..128 symbols (tRNA, pre-miRNA hairpins, snoRNA, 5S rRNA): sed_join_self /
 * sed_join_search with a longer record, through the integer route.  It batches the same reference lines:
 * wf_score(query, doc) over a whole collection, IRMethods.py:435-440 inside search_collection's loop,
 * IRMethods.py:443-477, each a full wagnerFisher(str1, str2), StringEditDistance.py:133-224.
 * A sed_join_long_index is a type of its own, because its device records differ (128 byte codes a sequence); it is
 * created, used and destroyed as a sed_join_index is, holds nseqs sequences of 0..sed_join_long_max_len() = 128 symbols
 * each (129, a negative length or offset, NULL: SED_E_ARG, the text names the number of symbols), and belongs to its
 * context.  Unchanged from sed_join_self / sed_join_search: rows are str1 and columns str2; the hit record, dist = D / S
 * and the rule D <= floor(max_dist * S); the (row, col) sort; the cap protocol (*found always set, SED_E_RANGE naming
 * both numbers, the index stays usable, the count query with cap = 0 and out = NULL); the state errors; +inf admits
 * every pair (no scaled distance of two sequences of <= 128 symbols exceeds 128 * 255 < 65535); NaN or a negative
 * max_dist: SED_E_ARG; the cost models served and their refusals, condition for condition (for such tables D / S is the
 * reference's value bit for bit); a row or column code >= K: SED_E_ARG; bit-parallel under the same conditions, else
 * the scaled DP, and SED_OPT_JOIN_DP forces the DP; the length skip by wave; SED_OPT_JOIN_ROWS and the limit of 65535
 * groups of sed_join_rows_per_group rows a launch.
 * A wave runs a row over the columns 1 .. 32 * ceil(longest / 32) of its 64 columns (stored sorted by length), so a
 * collection of 40-symbol sequences pays for 64 cells a row, not 128; sequences of at most 32 symbols are served, and
 * faster by sed_join_index.  sed_join_long_plan's out[6] counts the cells executed.
 * Not served: tables the conditions refuse (there is no fp64 route for this index yet), sequences over 128 symbols, edit
 * scripts of the hits, the i < j half alone for symmetric tables, a per-tile mix of the two variants; of the k-nearest
 * calls below: an fp64 route (sed_join_knn_self_f64 / sed_join_knn_search_f64 serve the short index only) and k > 64. */
typedef struct sed_join_long_index sed_join_long_index;
sed_join_long_index *sed_join_long_index_create(sed_ctx *ctx, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                                int32_t nseqs);
void sed_join_long_index_destroy(sed_join_long_index *ix);
int32_t sed_join_long_index_seqs(const sed_join_long_index *ix);
int sed_join_long_self(sed_join_long_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out,
                       int64_t cap, int64_t *found);
int sed_join_long_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                         int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
/* sed_join_last_time and sed_join_pairs_run for this index type. */
int sed_join_long_last_time(const sed_join_long_index *ix, float *kernel_ms);
int sed_join_long_pairs_run(const sed_join_long_index *ix, int64_t *pairs);
/* sed_join_knn_self, sed_join_knn_search, sed_join_knn_bounds, sed_join_knn_candidates and sed_join_knn_bound_time for
 * this index type (the same reference lines: IRMethods.py:435-440, 443-477; StringEditDistance.py:133-224): rows, columns
 * and queries of 0..128 symbols, everything else as stated there. */
int sed_join_long_knn_self(sed_join_long_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist,
                           sed_join_hit *out, int64_t cap, int64_t *found);
int sed_join_long_knn_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                             int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found);
int sed_join_long_knn_bounds(const sed_join_long_index *ix, int32_t *bounds, int32_t n);
int sed_join_long_knn_candidates(const sed_join_long_index *ix, int64_t *n);
int sed_join_long_knn_bound_time(const sed_join_long_index *ix, float *kernel_ms);
/* The longest sequence a sed_join_long_index holds: 128. */
int32_t sed_join_long_max_len(void);
/* What the long calls would decide, without a device: sed_join_plan's arguments, order of refusals and out[] slots 0..5,
 * with lengths 0..128 accepted (129 or a negative length: SED_E_ARG); for lengths all <= 32 slots 0..5 are
 * sed_join_plan's.  out[6] = the cells the waves execute: for every wave (64 columns in sorted order; the last wave's
 * spare lanes run too) and every row it runs (one of its columns passes the length bound; a self join's own pairs are
 * not taken out here), 64 * n * 32 * ceil(the wave's longest column / 32).  Beside out[5] it shows what the padding of a
 * collection costs: the bit-parallel variant skips words by the same rule. */
int sed_join_long_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                       double del, int del_is_int, const int32_t *options, int noptions,
                       const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, int self,
                       uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout);
/* The text of this thread's last sed_join_long_plan refusal (the one the long calls leave in sed_last_error for the same
 * inputs: it names the failed condition, or the row or column and its number of symbols); "" after a plan that passed. */
const char *sed_join_long_plan_error(void);

/* Full DP matrix of one pair (the dp object the GUI renders, StringEditDistance.py:143-224):
 * D[i*(m+1)+j] = dp[i][j].value, M[...] = optimal incoming edges (1 insert, 2 delete,
 * 4 update) | (1 << 3 when the value is a Python int).  Always runs the fp64 kernel. */
int sed_full_matrix(sed_ctx *ctx, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m,
                    double *D, uint8_t *M);

/* Kernel self-test on the device (DPP lane shifts, byte permute); 0 = pass, else a failure bitmask. */
int sed_selftest(sed_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SED_H */
