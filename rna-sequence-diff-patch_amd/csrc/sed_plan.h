// sed_plan.h — the device-free half of a batch fill: everything the runtime decides about a batch (mode, rows per lane,
// every route, the layout of every buffer, the kernels' parameters) as a function of the cost model, the options and
// the pairs.  sed_plan.cpp calls no HIP API, so the planner runs, and is tested, without a device
// (include/sed.h: sed_plan_routes; tests/test_plan_routes.py), and so does the launch sequence of a run under a plan
// (sed_plan_run below; sed_plan_schedule; tests/test_plan_schedule.py).  Fit search plans in a unit of its own, sed_fit_plan.h,
// which takes sed_costs, sed_opts and sed_plan_fail from here.
#pragma once
#include "../../include/sed.h"
#include "sed_internal.h"

#include <string>
#include <vector>

// the cost model of sed_set_costs
struct sed_costs {
    int K = 0;
    std::vector<double> sub;
    std::vector<uint8_t> sub_int;
    double ins = 1, del = 1;
    int ins_int = 0, del_int = 0;
};

// sed_set_option's values, and the process's environment knobs as the runtime read them (sed_runtime.cpp: env_opts)
struct sed_opts {
    int mode = 0, R = 0, split = 0, lane = 0, chain = 0, pack = 0, tb = 0;
    int chain_waves = 0;    // SED_OPT_CHAIN_WAVES: cap on the persistent waves of dynamic CHAIN mode
    int bitpar = 0;         // SED_OPT_BITPAR: 0 auto (unit-cost distance-only lane pairs), 2 never
    int scaled = 0;         // SED_OPT_SCALED: 0 auto (fp64 lane pairs under dyadic costs), 2 never
    int seg = 0;            // SED_OPT_SEG: 0 auto (fp64 pairs the cost model prefers in 16-lane segments), 1 every
                            // eligible pair, 2 never
    int splitck = 0;        // SED_OPT_SPLITCK: 0 auto (on), 2 never (SPLIT script batches keep the per-cell-code forward)
    int zc = 0;             // SED_OPT_ZEROCOPY: 0 auto (small batches write results into pinned host memory), 2 never
    int dot = 0;            // SED_OPT_DOT: 0 auto, 2 never (checkpoint batches keep the perm-based distance keys), 3 no wide ladder
    int debug_corrupt = 0;  // SED_OPT_DEBUG_CORRUPT: pair + 1 whose sink-tile checkpoint is overwritten
    int band = 0;           // SED_OPT_BAND: 0 auto (checkpoint batches of the stripe kernel skip the cells no
                            // optimal path reaches, every stripe's range refined from the row above it), 2 never,
                            // 3 the static windows only
    int cut = 0;            // SED_OPT_CUT: cutoff batches' wave pairs: 0 auto (the windowed stripe kernel when it
                            // should pay), 1 whenever eligible, 2 never (filter only)
    int fit_chunk = 0;      // SED_OPT_FIT_CHUNK: fit search (sed_fit_plan.h), owned text columns per lane: 0 auto, else
                            // the chunk length
    int fit_rows = 0;       // SED_OPT_FIT_ROWS: the long fit calls (sed_fit_plan.h), pattern rows per lane: 0 auto, else R
    int join_dp = 0;        // SED_OPT_JOIN_DP: the similarity join (sed_join_plan.h): 0 auto (bit-parallel under unit costs),
                            // 2 the scaled DP kernel always
    int join_rows = 0;      // SED_OPT_JOIN_ROWS: the join's rows per launch: 0 auto (the grid's limit), else that many (tests)
    int env_tbpar = -1;     // SED_TBPAR: 0/1 overrides the stripe-parallel traceback's rule (A/B), -1 unset
    int env_band = 1;       // SED_BAND: 0 turns band pruning off, 3 ("static") keeps the static windows (A/B through bench.py)
    int env_alt_dp = 1;     // SED_ALT_DP: 0 keeps every DP on the context's stream (A/B)
    int env_ck_halves = -1; // SED_CK_HALVES: parts per checkpoint batch, -1 unset (SED_CK_HALVES_DEFAULT)
};
// one (key, value) of sed_set_option, or of sed_plan_routes (which also takes the SED_PLAN_ENV_* keys): false when the
// key is unknown or the value is not one it takes
bool sed_opts_set(sed_opts &o, int key, int value, bool env_keys);

// A planner's refusal (the batch planner's and the fit planner's, sed_fit_plan.cpp): the formatted text into *err when
// it is not null; returns code
int sed_plan_fail(std::string *err, int code, const char *fmt, ...);

// Batches whose input arrays and results fit this many bytes go up as one blob from pinned staging (sed_plan::small)
#define SED_SMALL_BATCH_BYTES (4u << 20)

// the input arrays of a batch on the device, in upload order
enum { SED_UP_PD, SED_UP_SEQA, SED_UP_SEQB, SED_UP_TASKS, SED_UP_CHAIN, SED_UP_LANE, SED_UP_X2, SED_UP_SEG, SED_UP_COUNT };

// Everything a fill decides.  A refilled plan (the context's scratch batch, every per-call request) keeps its vectors'
// storage.
struct sed_plan {
    int npairs = 0;
    uint32_t flags = 0;
    int mode = 0, R = 0;
    bool split = false;
    bool ck = false;           // traceback from checkpoints + recompute (sed_kernels.hip: CK) instead of codes
    // SPLIT script batches at R = 4 (config 2, GUI pairs): the forward runs distance / dot keys and stores checkpoints
    // after each pair's per-cell code region; sed_ck_codes_kernel (ck_tiles waves per pair) recomputes every tile's
    // codes into that region, which the stripe-parallel traceback walks
    bool split_ck = false;
    int ck_tiles = 0;
    bool tbpar = false;        // stripe-parallel traceback (few long pairs, per-cell codes; sed_tb_stripe*_kernel)
    int tbpar_items = 0, tbpar_kmax = 0;
    // band pruning (sed_internal.h: sed_band_window): the forward runs only the chunks an optimal path can reach;
    // band_cells = the cells the forward computes (from the host's own diagonal bounds; = cells when off)
    bool band = false;
    // refined windows (sed_internal.h: sed_refine_cell): band_stripes = the most stripes of any wave pair, the stride of
    // the per-stripe regions [suffix costs (npairs x band_stripes words) | windows (npairs x band_stripes x 2)]
    bool band_refine = false;
    int band_stripes = 0;
    sed_band_params bandp{};
    double band_cells = 0;
    // a cutoff's windows (sed_batch_set_cutoff): their costs and whether they allow pruning, taken at the fill with the
    // kernels' own parameters (ip), so a later sed_set_costs on the context cannot part the windows from the DP
    bool cut_costs_ok = false;
    sed_band_params cut_bp{};
    bool dot = false;          // CK forward kernel on dot keys
    bool lad = false;          // CHAIN kernel with the L field on ladder dot keys
    int nlane = 0, nwave = 0;  // pairs on the lane-per-pair kernel / on the wave kernels
    int nlane_x2 = 0;          // > 0: lane pairs run two per lane (distance only), in this many lanes
    bool lane_bitpar = false;  // lane pairs run the bit-parallel unit-cost kernel (distance only)
    uint32_t umask = 0;        // fp64 lane kernel: codes of the unit-cost subset; its pairs run bit-parallel
    int nbitpar_f64 = 0;       // fp64 lane pairs flagged for it (pd.pad[0])
    bool scaled = false;       // fp64 lane pairs on the scaled-integer kernel (dyadic costs)
    sed_scaled_params sp{};
    int nwave_x2 = 0;          // distance-only wave pairs of equal shape run two per wave, in this many waves
    int nseg = 0;              // fp64 wave pairs in 16-lane segments (pd.pad[1]), listed in seg
    int nchains = 0;           // CHAIN mode: wave pairs run as nchains back-to-back chains (0 = off)
    bool chain_dyn = false;    // persistent waves + device counter instead of static chains
    size_t chain_npairs = 0;   // chain = [chain pairs (chain_npairs) | chain offsets (nchains + 1)]; the device array
                               // ends with the dynamic mode's counters
    int ntasks = 0;
    // SED_PIPELINE: run k uses traceback/result buffer k % nbuf (sed_runtime.cpp: sed_batch)
    int nbuf = 1;
    int nparts = 1;            // checkpoint batches in parts (SED_CK_HALVES)
    bool alt_dp = false;       // odd runs' DP on a second stream
    // small batches keep every input array and the results in one blob; zc: their kernels write results and scripts
    // straight into pinned host memory
    bool small = false, zc = false;
    uint64_t tb_words = 0, bnd_words = 0, ops_words = 0, map_words = 0;
    double cells = 0, algo_bytes = 0;
    std::vector<sed_pair_desc> pd;
    std::vector<int2> tasks;                // SPLIT: (pair, stripe) per workgroup
    std::vector<int32_t> lane, seg, x2, chain;
    std::vector<int32_t> tmp;               // scratch of the pair lists' sorts
    // the device arrays: bytes reserved for each, the bytes of host data that go up, and the aligned offsets of the
    // small path's blob [arrays | results | scripts] (results and scripts adjacent: one download)
    size_t up_size[SED_UP_COUNT] = {}, up_copy[SED_UP_COUNT] = {}, up_off[SED_UP_COUNT] = {};
    size_t res_size = 0, o_res = 0, o_ops = 0, blob_bytes = 0;
    sed_i32_params ip{};
    sed_f64_params fp{};
};

// Plans the batch.  Returns SED_OK or the SED_E_* code of the first failed check, with its text in *err.
int sed_plan_batch(const sed_costs &c, const sed_opts &o, const uint8_t *codes_a, const int64_t *off_a,
                   const int32_t *len_a, const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                   int32_t npairs, uint32_t flags, sed_plan *plan, std::string *err);
// The sequences as the kernels read them (2-bit packed words in integer mode, else bytes), zero padded:
// plan.up_copy[SED_UP_SEQA / SED_UP_SEQB] bytes at ha / hb.
void sed_pack_sequences(const sed_plan &plan, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                        const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, std::vector<uint32_t> &ha,
                        std::vector<uint32_t> &hb);

// ---- what a run launches ----
// One step = one launcher call of the runtime's loop (sed_runtime.cpp: run_batch).  A launcher keeps its helper kernels
// inside: the stripe forward its band kernel, the windowed forward its window kernel, the stripe-parallel walk its three.
enum sed_step_kind : uint8_t {
    SED_STEP_WIN,         // windowed cutoff forward (sed_launch_i32_cut)
    SED_STEP_X2,          // packed forward, two pairs per wave
    SED_STEP_CHAIN,
    SED_STEP_I32,         // integer stripe forward (with checkpoints in a ck or split_ck batch)
    SED_STEP_CODES,       // split_ck: every tile's codes from the forward's checkpoints
    SED_STEP_F64,
    SED_STEP_F64_SEG,
    SED_STEP_LANE,        // the lane kernel the plan's lane route names (the runtime picks among the five launchers)
    SED_STEP_FILTER,      // cutoff filter
    SED_STEP_TB_CK,       // traceback from checkpoints
    SED_STEP_TB_CODES,    // traceback over per-cell codes
    SED_STEP_TB_STRIPES,  // stripe-parallel traceback
    SED_STEP_TB_SEG,      // traceback of the fp64 segment pairs
};
enum : uint8_t { SED_PHASE_DP, SED_PHASE_TB };
// the stream a step runs on: this run's DP stream (the context's, or the second DP stream on odd runs of an alt_dp
// batch), the traceback stream (the DP stream's when buffers do not rotate), or the stream of the step's part
enum : uint8_t { SED_ON_DP, SED_ON_TB, SED_ON_PART };
// a rotating buffer's next user waits for this event of the slot's previous run (the value = its place in an event-log
// entry {DP start, DP end, traceback start, traceback end})
enum : uint8_t { SED_REUSE_NONE = 0, SED_REUSE_DP_END = 1, SED_REUSE_TB_END = 3 };
#define SED_MAX_PARTS 4
// (the longest schedules: four forwards, the lane kernel and four tracebacks of a batch in parts; packed, forward,
// segments, lane, filter and three traceback steps of one in a single part)
#define SED_MAX_STEPS 12

struct sed_step {
    uint8_t kind, phase, on;
    // part's pairs are [npairs * part / nparts, npairs * (part + 1) / nparts); the lane step addresses the whole batch's
    // lane pairs by index and belongs to part 0 for its stream and events only
    uint8_t part;
    // the timing events ride on the kernels' own dispatch packets: the first step of a (phase, part) carries that
    // part's start event of the phase and the last one its end event
    bool first, last;
};
// Fixed capacity, no heap: the per-call path refills a batch, and so rebuilds this, on every call.
struct sed_run_plan {
    int n = 0, nparts = 1;
    bool tb = false;       // the run has a traceback phase (a phase without steps records its two events directly)
    bool cut = false;      // the DP phase ends with the cutoff filter
    bool need_ev = false;  // the run's events order the reuse of rotating buffers: recorded on untimed runs too
    uint8_t reuse = SED_REUSE_NONE;
    sed_step step[SED_MAX_STEPS] = {};
};
// The launches of one run of the planned batch, in order; cut_on / cut_win: the batch's cutoff state
// (sed_batch_set_cutoff).  A batch without pairs launches nothing.
sed_run_plan sed_plan_run(const sed_plan &p, bool cut_on, bool cut_win);
// whether a cutoff may move the batch's wave pairs to the windowed stripe kernel (cut_win)
bool sed_plan_cut_window_ok(const sed_plan &p);

bool sed_simple_typing(const sed_costs &c);  // a cell's value is an int exactly when it equals 0
sed_band_params sed_band_params_from(const sed_costs &c);
// the cost of the plain diagonal path (band pruning's upper bound on the distance): the host's restatement of
// sed_band_kernel over unpacked codes
uint64_t sed_band_diag_bound(const sed_band_params &bp, const uint8_t *a, int n, const uint8_t *b, int m);

// What the sed_batch_* getters report, as functions of the plan (cut_win: a cutoff moved the wave pairs to the
// windowed stripe kernel, sed_batch_set_cutoff)
inline int sed_plan_chains(const sed_plan &p, bool cut_win) { return cut_win ? 0 : p.nchains; }
inline int sed_plan_traceback_mode(const sed_plan &p) {
    if (!(p.flags & SED_WANT_SCRIPT)) return 0;
    return p.ck ? 2 : p.split_ck ? 4 : (p.tbpar ? 3 : 1);
}
inline int sed_plan_dot_keys(const sed_plan &p) {
    return (p.dot ? 1 : 0) | (p.lad ? 2 : 0) | (p.lad && p.ip.lad == 2 ? 4 : 0);
}
inline int sed_plan_bitpar_pairs(const sed_plan &p) { return p.lane_bitpar ? p.nlane : p.nbitpar_f64; }
inline int sed_plan_split_tasks(const sed_plan &p) { return p.split ? p.ntasks : 0; }
inline int sed_plan_scaled_pairs(const sed_plan &p) { return p.scaled ? p.nlane - p.nbitpar_f64 : 0; }
inline int sed_plan_packed_pairs(const sed_plan &p, bool cut_win) {
    return (p.nlane_x2 > 0 ? p.nlane : 0) + (cut_win ? 0 : 2 * p.nwave_x2);
}
