// sed_join_plan.h — the device-free half of the similarity join (include/sed.h: sed_join_self, sed_join_search): what a
// join decides from the cost model, the options, the lengths, the codes seen and the cutoff.  sed_join_plan.cpp calls no
// HIP API (it shares sed_costs, sed_opts and sed_plan_fail with the batch planner, sed_plan.h, and nothing else); its
// export sed_join_plan runs, and is tested, without a device.
#pragma once
#include "sed_plan.h"

#define SED_JOIN_KERNEL_DP 1
#define SED_JOIN_KERNEL_BITPAR 2
#define SED_JOIN_CUT_ALL 65535  // no scaled distance of two sequences of <= 32 symbols exceeds 64 * 255

struct sed_join_plan_t {
    int scale_log2 = 0;          // S = 2^scale_log2
    int kernel = SED_JOIN_KERNEL_DP;
    sed_scaled_params sp{};      // the cost rows, insert and delete on the integer scale, umap (bit-parallel variant)
    int32_t cut = 0;             // min(floor(max_dist S), SED_JOIN_CUT_ALL)
    int64_t launch_rows = 0;     // rows one launch takes: SED_JOIN_MAX_GROUPS groups, or SED_OPT_JOIN_ROWS
    double waves = 0;            // the 64-lane waves of every launch: 4 per block
    double scope = 0;            // the pairs the call is about: rows x columns, less the (i, i) of a self join
    double run = 0, cells = 0;   // those whose length bound is within the cutoff, and their n m
};

// The table alone: the smallest S = 2^k, k <= 8, that makes insert, delete and every substitution cost integral, with
// insert S, delete S >= 1, every cost <= insert + delete and (insert + delete) S <= 255 over at most 8 symbols
// (sed_plan.cpp: scaled_costs' conditions without the lane block's n <= 512 and without its typing); fills scale_log2 and
// sp's rows, ins, del and inv_scale.  Anything else: SED_E_RANGE, *err names the failed condition.
int sed_join_costs_rule(const sed_costs &c, sed_join_plan_t *plan, std::string *err);
// The whole plan.  len_rows / len_cols = the lengths (0..32 each, else SED_E_ARG); self: the rows are nrows of the ncols
// columns, and each row's own column is out of scope; row_codes / col_codes = bit c set when code c occurs (bit 31: any
// code >= 31).  A code >= K: SED_E_ARG; NaN or negative max_dist: SED_E_ARG.
int sed_join_plan_of(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows, const int32_t *len_cols,
                     int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes, double max_dist,
                     sed_join_plan_t *plan, std::string *err);
