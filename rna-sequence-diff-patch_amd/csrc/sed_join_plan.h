// sed_join_plan.h — the device-free half of the similarity join (include/sed.h: sed_join_self, sed_join_search): what a
// join decides from the cost model, the options, the lengths, the codes seen and the cutoff.  sed_join_plan.cpp calls no
// HIP API (it shares sed_costs, sed_opts and sed_plan_fail with the batch planner, sed_plan.h, and nothing else); its
// exports sed_join_plan, sed_join_long_plan, sed_join_knn_plan, sed_join_knn_trim, sed_join_decode, sed_join_f64_plan,
// sed_join_f64_keep, sed_join_knn_f64_plan, sed_join_f64_lower and sed_join_route run, and are tested, without a device.
// The integer rule takes its longest sequence as a parameter: SED_JOIN_MAXLEN for sed_join_self / sed_join_search,
// SED_JOIN_LONG_MAXLEN for sed_join_long_self / sed_join_long_search (kernel: sed_join_long.hip).
#pragma once
#include "sed_plan.h"

#define SED_JOIN_KERNEL_DP 1
#define SED_JOIN_KERNEL_BITPAR 2
// No scaled distance of two sequences of <= 128 symbols exceeds 128 * 255 = 32640 (every cost <= insert + delete, so
// max(n, m) updates and |n - m| indels bound it), so this cutoff admits every pair.  The same product is what a key's
// high half-word sinks by at most, and its low half-word sinks by at most 128 below 0xFFFC (sed_lane_dp.h).
#define SED_JOIN_CUT_ALL 65535

// What a plan of either route counts, from the lengths and the route's rule of which (n, m) are computed
struct sed_join_counts {
    int64_t launch_rows = 0;     // rows one launch takes: SED_JOIN_MAX_GROUPS groups, or SED_OPT_JOIN_ROWS
    double waves = 0;            // the 64-lane waves of every launch: 4 per block
    double scope = 0;            // the pairs the call is about: rows x columns, less the (i, i) of a self join
    double run = 0, cells = 0;   // those the route's length rule computes, and their n m
    int block = 0;               // the columns of a block the kernel runs or skips as one (0: lane_cells is not counted)
    double lane_cells = 0;       // the cells the waves execute: per wave and row it runs, 64 lanes x n x the blocks of
                                 // columns up to the wave's longest column (padding and spare lanes included)
};
struct sed_join_plan_t : sed_join_counts {  // run: the pairs whose length bound is within the cutoff
    int scale_log2 = 0;          // S = 2^scale_log2
    int kernel = SED_JOIN_KERNEL_DP;
    sed_scaled_params sp{};      // the cost rows, insert and delete on the integer scale, umap (bit-parallel variant)
    int32_t cut = 0;             // min(floor(max_dist S), SED_JOIN_CUT_ALL)
};

// The table alone: the smallest S = 2^k, k <= 8, that makes insert, delete and every substitution cost integral, with
// insert S, delete S >= 1, every cost <= insert + delete and (insert + delete) S <= 255 over at most 8 symbols
// (sed_plan.cpp: scaled_costs' conditions without the lane block's n <= 512 and without its typing); fills scale_log2 and
// sp's rows, ins, del and inv_scale.  Anything else: SED_E_RANGE, *err names the failed condition.  maxlen = the longest
// sequence the keys must hold: maxlen (insert + delete) S <= 65535, which the conditions give for every maxlen <= 128.
int sed_join_costs_rule(const sed_costs &c, int maxlen, sed_join_plan_t *plan, std::string *err);
// The whole plan.  len_rows / len_cols = the lengths (0..maxlen each, else SED_E_ARG; maxlen = SED_JOIN_MAXLEN or
// SED_JOIN_LONG_MAXLEN, and with the latter lane_cells counts SED_JOIN_LONG_BLOCK columns a block); self: the rows are nrows of the ncols
// columns, and each row's own column is out of scope; row_codes / col_codes = bit c set when code c occurs (bit 31: any
// code >= 31).  A code >= K: SED_E_ARG; NaN or negative max_dist: SED_E_ARG.  Both routes' plans refuse in one order:
// the arguments, max_dist, the route's costs rule, the code set, the rows, the columns.
int sed_join_plan_of(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows, const int32_t *len_cols,
                     int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes, double max_dist, int maxlen,
                     sed_join_plan_t *plan, std::string *err);
// The k-nearest calls (include/sed.h: sed_join_knn_self, sed_join_knn_search and their _long_ twins): k = 1 ..
// SED_JOIN_KNN_MAXK, checked with the arguments by this one rule (anything else: SED_E_ARG, the text names k); their plan
// is sed_join_plan_of as it is: plan->cut is the cap floor(max_dist S) every row's bound starts from, and run / cells /
// lane_cells count what one pass runs at most (the bounds only take pairs away).
int sed_join_knn_k_rule(int32_t k, std::string *err);

// The decode of a call's device records, for every route and form: validate, convert, order.  The one place a wrong
// record is refused before the caller sees it (DESIGN.md 3.6q lists the checks).
struct sed_join_rec {  // one 16-byte record of the device list (sed_internal.h: sed_join_list)
    uint32_t row, col, w0, w1;  // integer route: w0 = D on the scale, w1 unread; fp64: the distance's low and high words
};
struct sed_join_decode_call {
    int route;           // SED_JOIN_ROUTE_INT or SED_JOIN_ROUTE_F64
    int scale_log2;      // integer route: dist = D * 2^-scale_log2 (0..8); fp64: unread, the words are the double's bits
    double cap;          // the plan's cut (integer route) or max_dist (fp64): no distance is above it
    int32_t first, nrows, ncols;  // the call's rows are first .. first + nrows - 1, the index's columns 0 .. ncols - 1
    bool self;           // a self join: (i, i) is out of scope
    int32_t k;           // 0: a join; else k of a k-nearest call
    const void *bound;   // k-nearest: the rows' bounds after pass 1, nrows of them: uint32_t each on the integer route,
                         // a double each on fp64 (any alignment); a record is within its row's bound
};
// rec[0 .. n) -> out[0 .. n) (room for n hits), *kept = the hits left.  A join: sorted by (row, col).  A k-nearest
// call: through sed_join_knn_trim, so sorted by (row, dist, col) and each row's first k.  Then no (row, col) occurs twice
// among the hits left.  Bad arguments: SED_E_ARG; a record that fails a check: SED_E_DEVICE, *err names it.  Nothing in
// out is promised after a refusal.
int sed_join_decode_of(const sed_join_decode_call &d, const sed_join_rec *rec, int64_t n, sed_join_hit *out, int64_t *kept,
                       std::string *err);

// The fp64 route (include/sed.h: sed_join_self_f64, sed_join_search_f64; kernel: sed_join_f64.hip): any table of finite
// costs >= 0 over at most SED_JOIN_F64_MAXK symbols.  There is no scale: a cell's value is the oracle's.
#define SED_JOIN_KERNEL_F64 3
struct sed_join_f64_plan_t : sed_join_counts {
    double ins = 0, del = 0;     // -0.0 normalised to +0.0, as sub
    double sub[SED_JOIN_F64_MAXK * SED_JOIN_F64_MAXK] = {};  // row a = row symbol a, zeros past K
    double max_dist = 0;
    uint64_t keep[SED_JOIN_MAXLEN + 1] = {};  // keep[n] bit m: a row of n and a column of m symbols are computed
    double low[(SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1)] = {};  // low[33 n + m]: what keep compares with max_dist
};
// The table alone: K <= SED_JOIN_F64_MAXK, every cost finite and >= 0; fills ins, del, sub.  Anything else: SED_E_RANGE,
// *err names the bound or the cost.
int sed_join_f64_costs_rule(const sed_costs &c, sed_join_f64_plan_t *plan, std::string *err);
// The length skip under rounding.  The oracle's D of a row of n and a column of m symbols is a
// sequentially rounded sum; with k = |m - n| and c = insert (m > n) or delete (n > m),
//     D >= k c (1 - 2^-53)^(n + m) > fl(k c) (1 - 2^-46),
// so the pair is left out exactly when n, m, k >= 1, max_dist is finite, p = fl(k c) is finite and >= 2^-900, and
// fl(p - p 2^-40) > max_dist.  With n = 0 or m = 0, D is the product fl(m insert) or fl(n delete) itself and the exact
// compare decides.  keep[n] bit m = the pair is computed.  ins, del >= +0, max_dist >= 0 or +inf.
// The value the rule compares is a table of its own, low[33 n + m] for n, m = 0..32: the border product when n = 0 or
// m = 0; fl(p - p 2^-40) when n != m and p is finite and >= 2^-900; else 0.  low <= D for every pair of those lengths,
// every entry is >= +0 and no NaN (a border product may be +inf), and keep[n] bit m = low[33 n + m] <= max_dist.  The
// k-nearest calls of this route compare it with a row's moving bound on the device.
void sed_join_f64_lower_rule(double ins, double del, double low[(SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1)]);
void sed_join_f64_keep_rule(double ins, double del, double max_dist, uint64_t keep[SED_JOIN_MAXLEN + 1]);
// The whole plan: sed_join_plan_of's arguments, checks and counts, under the rule above.  It is the plan of this route's
// k-nearest calls as it is (sed_join_knn_k_rule first): max_dist is the cap every row's bound starts from, low the table
// the passes skip by, and run / cells count what one pass runs at most.
int sed_join_f64_plan_of(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows,
                         const int32_t *len_cols, int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes,
                         double max_dist, sed_join_f64_plan_t *plan, std::string *err);
