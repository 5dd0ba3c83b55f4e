// sed_join_plan.cpp — the join planner (sed_join_plan.h): scale and cost rows, the kernel variant, the cutoff on the
// integer scale, the launches and the pair counts of a similarity join, and the decode of its device records.  No HIP
// call.  Also the device-free entry points of include/sed.h: the five plan exports (one body, join_plan_export),
// sed_join_knn_trim, sed_join_decode, sed_join_f64_keep, sed_join_f64_lower and sed_join_route.
#include "sed_join_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

int sed_join_costs_rule(const sed_costs &c, int maxlen, sed_join_plan_t *plan, std::string *err) {
    if (c.K > 8) return sed_plan_fail(err, SED_E_RANGE, "join: %d symbols (the scaled cost rows hold at most 8)", c.K);
    auto finite = [](double v) { return std::isfinite(v) && v >= 0; };
    bool ok = finite(c.ins) && finite(c.del);
    for (int e = 0; e < c.K * c.K && ok; ++e) ok = finite(c.sub[e]);
    if (!ok) return sed_plan_fail(err, SED_E_RANGE, "join: a cost is negative or not finite");
    int k = 0;
    for (;; ++k) {
        if (k > 8)
            return sed_plan_fail(err, SED_E_RANGE, "join: the costs are not all multiples of 2^-k for any k <= 8 (no scale makes them integers)");
        const double S = std::ldexp(1.0, k);
        auto integral = [&](double v) { const double x = v * S; return x == std::floor(x); };
        ok = integral(c.ins) && integral(c.del);
        for (int e = 0; e < c.K * c.K && ok; ++e) ok = integral(c.sub[e]);
        if (ok) break;
    }
    const double S = std::ldexp(1.0, k);
    if (c.ins * S < 1 || c.del * S < 1)
        return sed_plan_fail(err, SED_E_RANGE, "join: insert * S = %g, delete * S = %g: both must be at least 1", c.ins * S, c.del * S);
    for (int e = 0; e < c.K * c.K; ++e)
        if (c.sub[e] > c.ins + c.del)
            return sed_plan_fail(err, SED_E_RANGE, "join: cost(%d -> %d) = %g exceeds insert + delete = %g", e / c.K, e % c.K,
                                 c.sub[e], c.ins + c.del);
    if ((c.ins + c.del) * S > 255)
        return sed_plan_fail(err, SED_E_RANGE, "join: (insert + delete) * S = %g exceeds 255 (the update addend's byte)",
                             (c.ins + c.del) * S);
    // the keys' room (sed_join_plan.h): a key's high half-word sinks by at most maxlen (insert + delete) S
    if ((c.ins + c.del) * S * maxlen > SED_JOIN_CUT_ALL)
        return sed_plan_fail(err, SED_E_RANGE, "join: (insert + delete) * S * %d = %g exceeds %d (the key's half-word)", maxlen,
                             (c.ins + c.del) * S * maxlen, SED_JOIN_CUT_ALL);
    plan->scale_log2 = k;
    sed_scaled_params &sp = plan->sp;
    sp = sed_scaled_params{};
    sp.ins = (uint32_t)(c.ins * S);
    sp.del = (uint32_t)(c.del * S);
    sp.inv_scale = std::ldexp(1.0, -k);
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) {
            const uint32_t v = (a < c.K && b < c.K) ? (uint32_t)(c.sub[a * c.K + b] * S) : 0u;
            sp.row[a][b >> 2] |= ((v - sp.ins - sp.del - 1u) & 0xFFu) << (8 * (b & 3));
        }
    return SED_OK;
}

// unit_costs' conditions (sed_plan.cpp) on the numbers, restricted to the cells a join can meet: insert = delete = 1, at
// most four codes in all, and cost(a -> b) = 1 (0 when a = b) for every row code a and column code b.  *umap = the
// codes' 2-bit codes, in code order.
static bool join_unit_costs(const sed_costs &c, uint32_t row_codes, uint32_t col_codes, uint32_t *umap) {
    const uint32_t seen = row_codes | col_codes;
    if (c.ins != 1.0 || c.del != 1.0 || __builtin_popcount(seen) > 4) return false;
    uint32_t map = 0, next = 0;
    for (int a = 0; a < c.K; ++a) {
        if (!((seen >> a) & 1u)) continue;
        for (int b = 0; b < c.K && ((row_codes >> a) & 1u); ++b)
            if (((col_codes >> b) & 1u) && c.sub[a * c.K + b] != (a == b ? 0.0 : 1.0)) return false;
        map |= next++ << (2 * a);
    }
    *umap = map;
    return true;
}

// What the plans of both routes share: the checks in their one order - the arguments, max_dist, the route's costs rule
// (rule(): it also derives whatever keep reads), the code set, the rows, the columns - then the launches and the counts
// under keep(n, m) = a row of n and a column of m symbols are computed.  maxlen = the route's longest sequence.
template <class Rule, class Keep>
static int join_plan_shared(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows, const int32_t *len_cols,
                            int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes, double max_dist, int maxlen,
                            sed_join_counts *plan, std::string *err, Rule rule, Keep keep) {
    if (nrows < 0 || ncols < 0 || (nrows && !len_rows) || (ncols && !len_cols) || (self && nrows > ncols))
        return sed_plan_fail(err, SED_E_ARG, "bad join arguments");
    if (std::isnan(max_dist) || max_dist < 0) return sed_plan_fail(err, SED_E_ARG, "join: max_dist is NaN or negative");
    const int rc = rule();
    if (rc != SED_OK) return rc;
    const uint32_t seen = row_codes | col_codes;
    if (c.K < 32 && (seen >> c.K) != 0) {
        const bool in_cols = (col_codes >> c.K) != 0;
        return sed_plan_fail(err, SED_E_ARG, "join: a %s code is outside the alphabet (K=%d)", in_cols ? "column" : "row", c.K);
    }
    double hr[SED_JOIN_LONG_MAXLEN + 1] = {}, hc[SED_JOIN_LONG_MAXLEN + 1] = {};
    double own_cells = 0;  // sum n n over the rows: the (i, i) pairs a self join leaves out
    for (int i = 0; i < nrows; ++i) {
        if (len_rows[i] < 0 || len_rows[i] > maxlen)
            return sed_plan_fail(err, SED_E_ARG, "join: row %d has %d symbols (0..%d)", i, len_rows[i], maxlen);
        hr[len_rows[i]] += 1;
        own_cells += (double)len_rows[i] * len_rows[i];
    }
    for (int j = 0; j < ncols; ++j) {
        if (len_cols[j] < 0 || len_cols[j] > maxlen)
            return sed_plan_fail(err, SED_E_ARG, "join: column %d has %d symbols (0..%d)", j, len_cols[j], maxlen);
        hc[len_cols[j]] += 1;
    }
    plan->launch_rows = o.join_rows > 0 ? o.join_rows : (int64_t)SED_JOIN_MAX_GROUPS * SED_JOIN_G;
    const double blocks = (ncols + SED_JOIN_BLOCK - 1) / SED_JOIN_BLOCK;
    double groups = 0;
    for (int64_t r = 0; r < nrows; r += plan->launch_rows)
        groups += (double)((std::min<int64_t>(plan->launch_rows, nrows - r) + SED_JOIN_G - 1) / SED_JOIN_G);
    plan->waves = ncols > 0 ? blocks * groups * (SED_JOIN_BLOCK / 64) : 0;
    plan->scope = (double)nrows * ncols - (self ? nrows : 0);
    plan->run = plan->cells = 0;
    for (int n = 0; n <= maxlen; ++n)
        for (int m = 0; m <= maxlen; ++m) {
            if (!keep(n, m)) continue;
            plan->run += hr[n] * hc[m];
            plan->cells += hr[n] * hc[m] * n * m;
        }
    if (self) {  // every (i, i) has n = m, which both routes' rules compute, and was counted
        plan->run -= nrows;
        plan->cells -= own_cells;
    }
    // What the waves execute: the columns sorted by length, 64 to a wave (the last wave's spare lanes take the longest
    // column); a wave runs a row when keep() holds for one of its columns, over every block of `block` columns up to
    // its longest.  (block = 0: the route does not count them.)
    plan->lane_cells = 0;
    if (plan->block > 0 && ncols > 0) {
        std::vector<int32_t> sorted(len_cols, len_cols + ncols);
        std::sort(sorted.begin(), sorted.end());
        for (int32_t w = 0; w < ncols; w += 64) {
            const int32_t end = std::min(w + 64, ncols);
            const int longest = end - w < 64 ? sorted[ncols - 1] : sorted[end - 1];
            const double width = (double)((longest + plan->block - 1) / plan->block) * plan->block;
            for (int n = 0; n <= maxlen; ++n) {
                if (hr[n] == 0) continue;
                bool runs = false;
                for (int32_t t = w; t < end && !runs; ++t) runs = (t == w || sorted[t] != sorted[t - 1]) && keep(n, sorted[t]);
                if (runs) plan->lane_cells += hr[n] * 64.0 * n * width;
            }
        }
    }
    return SED_OK;
}

int sed_join_plan_of(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows, const int32_t *len_cols,
                     int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes, double max_dist, int maxlen,
                     sed_join_plan_t *plan, std::string *err) {
    if (maxlen != SED_JOIN_MAXLEN && maxlen != SED_JOIN_LONG_MAXLEN) return sed_plan_fail(err, SED_E_ARG, "bad join arguments");
    plan->block = maxlen == SED_JOIN_LONG_MAXLEN ? SED_JOIN_LONG_BLOCK : 0;
    auto rule = [&]() -> int {
        const int rc = sed_join_costs_rule(c, maxlen, plan, err);
        if (rc != SED_OK) return rc;
        uint32_t umap = 0;
        plan->kernel = o.join_dp != 2 && join_unit_costs(c, row_codes, col_codes, &umap) ? SED_JOIN_KERNEL_BITPAR : SED_JOIN_KERNEL_DP;
        plan->sp.umap = umap;
        // floor(max_dist S): S is a power of two, so the product is exact (or overflows to +inf, which the clamp takes)
        const double cs = std::floor(std::ldexp(max_dist, plan->scale_log2));
        plan->cut = cs >= SED_JOIN_CUT_ALL ? SED_JOIN_CUT_ALL : (int32_t)cs;
        return SED_OK;
    };
    auto keep = [&](int n, int m) {  // the length bound within the cutoff
        const uint32_t lb = m > n ? (uint32_t)(m - n) * plan->sp.ins : (uint32_t)(n - m) * plan->sp.del;
        return lb <= (uint32_t)plan->cut;
    };
    return join_plan_shared(c, o, len_rows, nrows, len_cols, ncols, self, row_codes, col_codes, max_dist, maxlen, plan, err, rule,
                            keep);
}

int sed_join_knn_k_rule(int32_t k, std::string *err) {
    if (k < 1 || k > SED_JOIN_KNN_MAXK)
        return sed_plan_fail(err, SED_E_ARG, "join: k = %d neighbours a row (1..%d: a wave selects among its 64 lanes)", k,
                             SED_JOIN_KNN_MAXK);
    return SED_OK;
}

// The trim of the k-nearest calls, in place: hits in any order -> sorted by (row, dist, col), the first k of each row.
// The order of (dist, col) is the kernels' (D, original column): dist = D / S with S a power of two.
extern "C" int sed_join_knn_trim(sed_join_hit *hits, int64_t n, int32_t k, int64_t *kept) {
    if (n < 0 || (n && !hits) || k < 1 || k > SED_JOIN_KNN_MAXK || !kept) return SED_E_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (std::isnan(hits[i].dist)) return SED_E_ARG;  // (no order)
    std::sort(hits, hits + n, [](const sed_join_hit &x, const sed_join_hit &y) {
        return x.row != y.row ? x.row < y.row : x.dist != y.dist ? x.dist < y.dist : x.col < y.col;
    });
    int64_t w = 0, in_row = 0;
    for (int64_t i = 0; i < n; ++i) {
        in_row = i > 0 && hits[i - 1].row == hits[i].row ? in_row + 1 : 0;
        if (in_row < k) hits[w++] = hits[i];
    }
    *kept = w;
    return SED_OK;
}

int sed_join_decode_of(const sed_join_decode_call &d, const sed_join_rec *rec, int64_t n, sed_join_hit *out, int64_t *kept,
                       std::string *err) {
    const bool f64 = d.route == SED_JOIN_ROUTE_F64, knn = d.k != 0;
    if ((!f64 && d.route != SED_JOIN_ROUTE_INT) || n < 0 || (n && (!rec || !out)) || !kept || d.first < 0 || d.nrows < 0 ||
        d.ncols < 0 || std::isnan(d.cap) || d.cap < 0 || (!f64 && (d.scale_log2 < 0 || d.scale_log2 > 8)) ||
        (knn && (d.k < 1 || d.k > SED_JOIN_KNN_MAXK || (d.nrows && !d.bound))))
        return sed_plan_fail(err, SED_E_ARG, "bad join arguments");
    const char *const form = knn ? "k-nearest join" : "join", *const what = knn ? "candidate" : "hit";
    const uint32_t first = (uint32_t)d.first, end = first + (uint32_t)d.nrows;
    const double inv = std::ldexp(1.0, -d.scale_log2);
    for (int64_t i = 0; i < n; ++i) {
        const sed_join_rec &r = rec[i];
        bool ok = r.row >= first && r.row < end && r.col < (uint32_t)d.ncols && !(d.self && r.row == r.col);
        double dist = 0;
        if (ok && f64) {  // the two words are the double's low and high ones, copied, not scaled; NaN fails the compares
            const uint64_t bits = (uint64_t)r.w0 | ((uint64_t)r.w1 << 32);
            memcpy(&dist, &bits, sizeof dist);
            double bound = d.cap;
            if (knn) memcpy(&bound, (const uint8_t *)d.bound + sizeof bound * (r.row - first), sizeof bound);
            ok = dist >= 0 && dist <= d.cap && dist <= bound;
        } else if (ok) {
            dist = (double)r.w0 * inv;
            uint32_t bound = r.w0;
            if (knn) memcpy(&bound, (const uint8_t *)d.bound + sizeof bound * (r.row - first), sizeof bound);
            ok = (double)r.w0 <= d.cap && r.w0 <= bound;
        }
        if (!ok)
            return sed_plan_fail(err, SED_E_DEVICE, "%s: record %lld from the device is no %s (row %u, column %u)", form,
                                 (long long)i, what, r.row, r.col);
        out[i] = sed_join_hit{(int32_t)r.row, (int32_t)r.col, dist};
    }
    *kept = n;
    if (knn) {
        if (sed_join_knn_trim(out, n, d.k, kept) != SED_OK)
            return sed_plan_fail(err, SED_E_DEVICE, "k-nearest join: the trim refused the device's records");
    } else {
        std::sort(out, out + n, [](const sed_join_hit &x, const sed_join_hit &y) { return x.row != y.row ? x.row < y.row : x.col < y.col; });
    }
    for (int64_t i = 1; i < *kept; ++i)
        if (out[i - 1].row == out[i].row && out[i - 1].col == out[i].col)
            return knn ? sed_plan_fail(err, SED_E_DEVICE, "k-nearest join: row %d reports column %d twice", out[i].row, out[i].col)
                       : sed_plan_fail(err, SED_E_DEVICE, "join: record %lld from the device is no hit (row %d, column %d)",
                                       (long long)i, out[i].row, out[i].col);
    return SED_OK;
}

extern "C" int sed_join_decode(const uint32_t *records, int64_t n, int route, int32_t scale_log2, double cap, int32_t first_row,
                               int32_t nrows, int32_t ncols, int self, int32_t k, const void *bounds, sed_join_hit *out,
                               int64_t *kept, char *why, int why_len) {
    if (why_len < 0 || (why_len && !why)) return SED_E_ARG;
    std::string text;
    const sed_join_decode_call d{route, scale_log2, cap, first_row, nrows, ncols, self != 0, k, bounds};
    const int rc = sed_join_decode_of(d, (const sed_join_rec *)records, n, out, kept, &text);
    if (why_len) std::snprintf(why, (size_t)why_len, "%s", text.c_str());
    return rc;
}

// ---- the fp64 route ----
int sed_join_f64_costs_rule(const sed_costs &c, sed_join_f64_plan_t *plan, std::string *err) {
    if (c.K > SED_JOIN_F64_MAXK)
        return sed_plan_fail(err, SED_E_RANGE, "join (fp64): %d symbols (at most %d)", c.K, SED_JOIN_F64_MAXK);
    auto cost_ok = [](double v) { return std::isfinite(v) && v >= 0; };  // (-0.0 >= 0)
    if (!cost_ok(c.ins)) return sed_plan_fail(err, SED_E_RANGE, "join (fp64): insert = %g is not a finite cost >= 0", c.ins);
    if (!cost_ok(c.del)) return sed_plan_fail(err, SED_E_RANGE, "join (fp64): delete = %g is not a finite cost >= 0", c.del);
    for (int e = 0; e < c.K * c.K; ++e)
        if (!cost_ok(c.sub[e]))
            return sed_plan_fail(err, SED_E_RANGE, "join (fp64): cost(%d -> %d) = %g is not a finite cost >= 0", e / c.K, e % c.K,
                                 c.sub[e]);
    plan->ins = c.ins + 0.0;  // (-0.0 + 0.0 = +0.0)
    plan->del = c.del + 0.0;
    std::fill(plan->sub, plan->sub + SED_JOIN_F64_MAXK * SED_JOIN_F64_MAXK, 0.0);
    for (int a = 0; a < c.K; ++a)
        for (int b = 0; b < c.K; ++b) plan->sub[a * SED_JOIN_F64_MAXK + b] = c.sub[a * c.K + b] + 0.0;
    return SED_OK;
}

void sed_join_f64_lower_rule(double ins, double del, double low[(SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1)]) {
    const double tiny = std::ldexp(1.0, -900), shrink = std::ldexp(1.0, -40);
    for (int n = 0; n <= SED_JOIN_MAXLEN; ++n)
        for (int m = 0; m <= SED_JOIN_MAXLEN; ++m) {
            double v = 0.0;
            if (n == 0 || m == 0) {  // D is this product itself (0.0 when n = m = 0)
                v = n == 0 ? (double)m * ins : (double)n * del;
            } else if (n != m) {
                const double p = m > n ? (double)(m - n) * ins : (double)(n - m) * del;
                // D > p (1 - 2^-46) >= fl(p - p 2^-40) for a finite p >= 2^-900 (p 2^-40 is exact there)
                if (std::isfinite(p) && p >= tiny) v = p - p * shrink;
            }
            low[(SED_JOIN_MAXLEN + 1) * n + m] = v;
        }
}

void sed_join_f64_keep_rule(double ins, double del, double max_dist, uint64_t keep[SED_JOIN_MAXLEN + 1]) {
    double low[(SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1)];
    sed_join_f64_lower_rule(ins, del, low);
    for (int n = 0; n <= SED_JOIN_MAXLEN; ++n) {
        keep[n] = 0;
        for (int m = 0; m <= SED_JOIN_MAXLEN; ++m)
            if (low[(SED_JOIN_MAXLEN + 1) * n + m] <= max_dist) keep[n] |= (uint64_t)1 << m;
    }
}

int sed_join_f64_plan_of(const sed_costs &c, const sed_opts &o, const int32_t *len_rows, int32_t nrows,
                         const int32_t *len_cols, int32_t ncols, bool self, uint32_t row_codes, uint32_t col_codes,
                         double max_dist, sed_join_f64_plan_t *plan, std::string *err) {
    auto rule = [&]() -> int {
        const int rc = sed_join_f64_costs_rule(c, plan, err);
        if (rc != SED_OK) return rc;
        // (-0.0 + 0.0 = +0.0: the k-nearest passes start every row's bound from these bits and order bounds as unsigned
        // keys, whose sign bit is 0; as -0.0 the starting bound lay above every key and was reported as -0.0)
        plan->max_dist = max_dist + 0.0;
        sed_join_f64_lower_rule(plan->ins, plan->del, plan->low);
        sed_join_f64_keep_rule(plan->ins, plan->del, max_dist, plan->keep);
        return SED_OK;
    };
    auto keep = [&](int n, int m) { return ((plan->keep[n] >> m) & 1u) != 0; };
    return join_plan_shared(c, o, len_rows, nrows, len_cols, ncols, self, row_codes, col_codes, max_dist, SED_JOIN_MAXLEN, plan,
                            err, rule, keep);
}

// sed_join_plan's, sed_join_f64_plan's and sed_join_route's arguments as the planner's costs and options
static int join_costs_of(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                         int del_is_int, const int32_t *options, int noptions, sed_costs *c, sed_opts *o) {
    if (K < 1 || K > 255 || !sub || noptions < 0 || (noptions && !options)) return SED_E_ARG;
    c->K = K;
    c->sub.assign(sub, sub + K * K);
    if (sub_int) c->sub_int.assign(sub_int, sub_int + K * K);
    c->ins = ins;
    c->del = del;
    c->ins_int = ins_is_int ? 1 : 0;
    c->del_int = del_is_int ? 1 : 0;
    for (int i = 0; i < noptions; ++i)
        if (!sed_opts_set(*o, options[2 * i], options[2 * i + 1], true)) return SED_E_ARG;
    return SED_OK;
}

// what sed_join_plan and sed_join_f64_plan report: JOIN_PLAN_FIELDS of sedgpu.py
static int join_plan_out(double scale, int kernel, const sed_join_counts &p, double *out, int nout) {
    const double v[] = {scale, (double)kernel, p.waves, p.scope, p.run, p.cells, p.lane_cells};
    for (int i = 0; i < nout && i < (int)(sizeof v / sizeof *v); ++i) out[i] = v[i];
    return SED_OK;
}

// The five plan exports' one body.  What an export is: its route (SED_JOIN_ROUTE_*), its longest sequence, k of a
// k-nearest plan (NULL: a join's), the slots of out[] it fills (6, or 7 with lane_cells) and where a refusal's text goes
// (NULL: nowhere).  The order: k, the out[] slots, the costs and options, then the route's whole plan.
struct JoinPlanExport {
    int route, maxlen;
    const int32_t *k;
    int nslots;
    std::string *err;
};
// sed_join_plan's arguments after the export's own, in its order
#define JOIN_PLAN_PARAMS                                                                                                       \
    int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,                \
        const int32_t *options, int noptions, const int32_t *len_rows, int32_t nrows, const int32_t *len_cols, int32_t ncols, \
        int self, uint32_t row_codes_seen, uint32_t col_codes_seen, double max_dist, double *out, int nout
#define JOIN_PLAN_ARGS                                                                                                  \
    K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions, len_rows, nrows, len_cols, ncols, self, \
        row_codes_seen, col_codes_seen, max_dist, out, nout

static int join_plan_export(const JoinPlanExport &x, JOIN_PLAN_PARAMS) {
    if (x.err) x.err->clear();
    int rc = x.k ? sed_join_knn_k_rule(*x.k, x.err) : SED_OK;
    if (rc != SED_OK) return rc;
    if (nout < 0 || (nout && !out)) return sed_plan_fail(x.err, SED_E_ARG, "bad join arguments");
    sed_costs c;
    sed_opts o;
    rc = join_costs_of(K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions, &c, &o);
    if (rc != SED_OK) return sed_plan_fail(x.err, rc, "bad join arguments");
    if (x.route == SED_JOIN_ROUTE_F64) {
        sed_join_f64_plan_t p;
        rc = sed_join_f64_plan_of(c, o, len_rows, nrows, len_cols, ncols, self != 0, row_codes_seen, col_codes_seen, max_dist, &p,
                                  x.err);
        return rc != SED_OK ? rc : join_plan_out(0.0, SED_JOIN_KERNEL_F64, p, out, std::min(nout, x.nslots));
    }
    sed_join_plan_t p;
    rc = sed_join_plan_of(c, o, len_rows, nrows, len_cols, ncols, self != 0, row_codes_seen, col_codes_seen, max_dist, x.maxlen,
                          &p, x.err);
    return rc != SED_OK ? rc : join_plan_out(std::ldexp(1.0, p.scale_log2), p.kernel, p, out, std::min(nout, x.nslots));
}

static thread_local std::string long_plan_error;  // sed_join_long_plan_error's text
static thread_local std::string knn_plan_error;   // sed_join_knn_plan_error's text

extern "C" int sed_join_plan(JOIN_PLAN_PARAMS) {
    return join_plan_export({SED_JOIN_ROUTE_INT, SED_JOIN_MAXLEN, nullptr, 6, nullptr}, JOIN_PLAN_ARGS);
}

extern "C" int sed_join_long_plan(JOIN_PLAN_PARAMS) {
    return join_plan_export({SED_JOIN_ROUTE_INT, SED_JOIN_LONG_MAXLEN, nullptr, 7, &long_plan_error}, JOIN_PLAN_ARGS);
}

extern "C" int sed_join_knn_plan(int long_index, int32_t k, JOIN_PLAN_PARAMS) {
    const JoinPlanExport x{SED_JOIN_ROUTE_INT, long_index ? SED_JOIN_LONG_MAXLEN : SED_JOIN_MAXLEN, &k, long_index ? 7 : 6,
                           &knn_plan_error};
    return join_plan_export(x, JOIN_PLAN_ARGS);
}

extern "C" int sed_join_f64_plan(JOIN_PLAN_PARAMS) {
    return join_plan_export({SED_JOIN_ROUTE_F64, SED_JOIN_MAXLEN, nullptr, 6, nullptr}, JOIN_PLAN_ARGS);
}

extern "C" int sed_join_knn_f64_plan(int32_t k, JOIN_PLAN_PARAMS) {
    return join_plan_export({SED_JOIN_ROUTE_F64, SED_JOIN_MAXLEN, &k, 6, &knn_plan_error}, JOIN_PLAN_ARGS);
}
#undef JOIN_PLAN_PARAMS
#undef JOIN_PLAN_ARGS

extern "C" const char *sed_join_long_plan_error(void) { return long_plan_error.c_str(); }

extern "C" const char *sed_join_knn_plan_error(void) { return knn_plan_error.c_str(); }

extern "C" int sed_join_f64_lower(double ins, double del, double *low) {
    if (!low || !(std::isfinite(ins) && ins >= 0) || !(std::isfinite(del) && del >= 0)) return SED_E_ARG;
    sed_join_f64_lower_rule(ins + 0.0, del + 0.0, low);
    return SED_OK;
}

extern "C" int sed_join_f64_keep(double ins, double del, double max_dist, uint64_t *keep) {
    if (!keep || !(std::isfinite(ins) && ins >= 0) || !(std::isfinite(del) && del >= 0) || std::isnan(max_dist) || max_dist < 0)
        return SED_E_ARG;
    sed_join_f64_keep_rule(ins + 0.0, del + 0.0, max_dist, keep);
    return SED_OK;
}

extern "C" int sed_join_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                              int del_is_int, const int32_t *options, int noptions, const int32_t *len_rows, int32_t nrows,
                              const int32_t *len_cols, int32_t ncols, int self, uint32_t row_codes_seen,
                              uint32_t col_codes_seen, double max_dist, char *why, int why_len) {
    if (why_len < 0 || (why_len && !why)) return SED_E_ARG;
    if (why_len) why[0] = 0;
    sed_costs c;
    sed_opts o;
    int rc = join_costs_of(K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions, &c, &o);
    if (rc != SED_OK) return rc;
    sed_join_plan_t p;
    std::string e_int, e_f64;
    if ((rc = sed_join_plan_of(c, o, len_rows, nrows, len_cols, ncols, self != 0, row_codes_seen, col_codes_seen, max_dist,
                               SED_JOIN_MAXLEN, &p, &e_int)) == SED_OK)
        return SED_JOIN_ROUTE_INT;
    if (rc != SED_E_RANGE) return rc;  // (bad arguments are bad for both)
    sed_join_f64_plan_t pf;
    rc = sed_join_f64_plan_of(c, o, len_rows, nrows, len_cols, ncols, self != 0, row_codes_seen, col_codes_seen, max_dist, &pf,
                              &e_f64);
    const std::string text = rc == SED_OK ? e_int : e_int + "; " + e_f64;
    if (why_len) std::snprintf(why, (size_t)why_len, "%s", text.c_str());
    return rc == SED_OK ? SED_JOIN_ROUTE_F64 : rc;
}
