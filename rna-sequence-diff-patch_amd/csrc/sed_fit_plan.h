// sed_fit_plan.h — the device-free half of fit search (include/sed.h: sed_fit_search, sed_fit_index_search,
// sed_fit_index_hits): what a search decides from the cost model, the options and the lengths.  sed_fit_plan.cpp calls
// no HIP API, as the batch planner (sed_plan.h, whose sed_costs, sed_opts and sed_plan_fail it shares and nothing else);
// its exports sed_fit_plan, sed_fit_lanes, sed_fit_index_plan, sed_fit_index_lanes, sed_fit_cutoff_scaled, their
// _long and _f64 siblings and sed_fit_route run, and are tested, without a device.  The four numeric routes (FitKind)
// are a parameter of one pair planner and one index planner; what differs between them is in FitRoute and in the
// route's cost envelope, nothing else.
#pragma once
#include "sed_plan.h"

// Pair p's lanes are first[p] .. first[p + 1); lane k of a pair owns text columns [k chunk, min((k + 1) chunk, n + 1))
// (chunk = 0: the pair's one lane owns them all) and starts sed_fit_lead(W, c0) columns before its first.
struct sed_fit_plan_t {
    int scale_log2 = 0;      // S = 2^scale_log2
    int64_t W = 0;           // P + floor(P delete / insert) over the batch's longest pattern; -1 when insert = 0
    int32_t chunk = 0;       // owned columns per lane; 0 = one lane per text
    int64_t lanes = 0;
    double cells = 0, nominal = 0;  // P x columns computed (warm-up included), and sum P n
    std::vector<int64_t> first;
    sed_fit_params fp{};
    // the fp64 routes alone; scale_log2 and fp are not used there
    int one_lane = 0;             // SED_FIT_F64_* below: why every text runs as one lane whatever the chunk option says
    double f64_ins = 0, f64_del = 0;
    std::vector<double> f64_sub;  // SED_FIT_F64_MAXK x SED_FIT_F64_MAXK, zeros past K, -0.0 normalised to +0.0
};

// The numeric route of a search: which kernel family runs it and in which layout.
//   FIT_SHORT_KEYS  sed_fit.hip           16-bit integer keys, one (pair, chunk) per lane, 1 <= P <= SED_LANE_MAXM
//   FIT_LONG_KEYS   sed_fit_long.hip      the same keys, one (query, chunk record) per wave, P <= SED_FIT_LONG_MAXP
//   FIT_F64         sed_fit_f64.hip       fp64 values, the lane layout
//   FIT_LONG_F64    sed_fit_long_f64.hip  fp64 values, the wave layout
enum FitKind { FIT_SHORT_KEYS, FIT_LONG_KEYS, FIT_F64, FIT_LONG_F64 };
// What the planner reads of a route.  The lane layout runs one pair's chunk in a lane, 64 to a wave, and its P <= 32
// keeps the D field's rebase room out of the envelope; the wave layout runs it in a whole wave, so its chunk rule counts
// waves where the lane layout counts lanes, and on the integer keys P delete S shares the 16-bit D field with the
// FIT_REBASE insert S a key carries at most between rebases.
struct FitRoute {
    int pmax;            // patterns of 1..pmax symbols
    int units_per_wave;  // (pair, chunk) units a wave runs: 64 (lanes) or 1 (the wave layout)
    int rebase_cols;     // columns of insert the D-field condition adds to P delete; 0: none
    bool f64;            // the fp64 envelope and window, no scale, no span limit; else the integer keys'
    bool waves() const { return units_per_wave == 1; }
};
const FitRoute &sed_fit_route_of(FitKind kind);

// The integer routes (FIT_SHORT_KEYS, FIT_LONG_KEYS): at most 8 symbols - refused before any length is looked at -,
// the smallest scale S = 2^k, k <= 8, that makes every cost a byte, P delete S (plus rebase_cols insert S) <= 65535,
// (insert + delete) S <= 255, W = P + floor(P delete / insert), and no lane spanning more than 65535 text columns.
//
// The fp64 routes (FIT_F64, FIT_LONG_F64): any table of finite costs >= 0 over at most SED_FIT_F64_MAXK symbols -
// refused after the lengths.  There is no scale and no span limit (starts are 32 bits).  W = P + floor(P delete /
// insert) + 2, the integer window plus the slack the rounding argument needs (it does not depend on
// P <= 32: 3.6j); where that argument cannot be made every text runs as one lane, W = -1, and plan->one_lane says why.
#define SED_FIT_F64_CHUNKED 0
#define SED_FIT_F64_INSERT_ZERO 1   // insert = 0: no window is finite (the integer route's rule)
#define SED_FIT_F64_NO_WINDOW 2     // the window argument's hypotheses fail: a cost outside 2^-900 .. 2^900, P delete /
                                    // insert above 2^20, or its checked inequality

// Every route shares the chunk rule and the order of the refusals.  The plan of npairs listed pairs (the lane layouts:
// sed_fit_search, sed_fit_search_f64); first / lanes / cells / nominal are filled.
int sed_fit_plan_batch(FitKind kind, const sed_costs &c, const sed_opts &o, const int32_t *len_p, const int32_t *len_t,
                       int32_t npairs, sed_fit_plan_t *plan, std::string *err);
// The same plan for an index search (include/sed.h: sed_fit_index_search and its siblings): nqueries patterns against
// every text of an index, i.e. sed_fit_plan_batch's plan of the nqueries x ntexts cross product, query-major, from the
// patterns' lengths and the texts' sums alone (both go through one rule).  It leaves lanes and cells 0 and `first`
// empty: they follow from the chunk table, sed_fit_build_chunks (lanes = nqueries x its records).  Under the wave layout
// rows[q] = the pattern rows per lane query q runs with: o.fit_rows when set (a query it cannot hold: SED_E_RANGE), else
// sed_fit_long_rows(P); the lane layout leaves rows empty.  The chunk table, W, the parameter words and the lane records
// do not depend on the layout: for P <= 32 and the same chunk the wave layout's records are the lane layout's.
struct sed_fit_index_sums {
    int32_t ntexts = 0;
    double cols = 0;             // sum (n + 1)
    int64_t nmax = -1;           // the longest text
    int32_t first_negative = -1; // the first text of negative length (the device-free exports; an index holds none)
};
int sed_fit_plan_index(FitKind kind, const sed_costs &c, const sed_opts &o, const int32_t *len_p, int32_t nqueries,
                       const sed_fit_index_sums &tx, sed_fit_plan_t *plan, std::vector<int32_t> *rows, std::string *err);
// The chunk table of the texts under plan.chunk, text by text in chunk order (chunks may be null), independent of the
// queries; returns the number of records.  *computed (if not null) += the columns the records' lanes run under plan.W,
// warm-up included.
int64_t sed_fit_build_chunks(const sed_fit_plan_t &plan, const int32_t *len_t, int32_t ntexts,
                             std::vector<sed_fit_chunk> *chunks, double *computed);
// (sed_fit_lead, the columns a lane starts before its first owned one: sed_internal.h, shared with the kernels)
// The cutoff of a hits search (include/sed.h: sed_fit_index_hits) on the plan's integer scale: *cut =
// min(floor(max_dist S), SED_FIT_CUT_ALL).  A distance D / S is within max_dist exactly when D <= floor(max_dist S)
// (S is a power of two, so max_dist S is exact); no D exceeds P delete S <= 65535, so SED_FIT_CUT_ALL admits every
// column of every query, which is what +inf means.  NaN or a negative max_dist: SED_E_ARG.
#define SED_FIT_CUT_ALL 65535
int sed_fit_cutoff_rule(const sed_fit_plan_t &plan, double max_dist, int32_t *cut, std::string *err);

// The lane records of a planned batch (sed_internal.h: sed_fit_lane), lanes[plan.first[p] + k] = lane k of pair p, from
// the plan and the lengths alone: tw counts 4-symbol words from the pair's own text start and pat is 0.  The runtime
// adds the base word of each text's copy and sets the pattern record (sed_fit_runtime.cpp: sed_fit_search).
void sed_fit_build_lanes(const sed_fit_plan_t &plan, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                         std::vector<sed_fit_lane> &lanes);
