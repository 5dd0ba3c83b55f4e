// sed_fit_plan.cpp — the fit planner (sed_fit_plan.h): scale, update addends, window, chunk length, lanes and the
// cutoff of a fit search, from the route, the cost model, the options and the lengths.  No HIP call.  Also the
// device-free fit entry points of include/sed.h (sed_fit_plan, sed_fit_lanes, sed_fit_index_plan, sed_fit_index_lanes,
// sed_fit_index_long_plan, sed_fit_index_long_lanes, sed_fit_cutoff_scaled, sed_fit_f64_plan, sed_fit_f64_lanes,
// sed_fit_index_f64_plan, sed_fit_index_f64_lanes, sed_fit_route, sed_fit_index_long_f64_plan,
// sed_fit_index_long_f64_lanes, sed_fit_long_route): each is its route handed to one of a few shared bodies.
#include "sed_fit_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>

// The device the auto chunk rule sizes for: 256 CUs x 4 SIMDs, 64 lanes a wave.  One lane per text is kept when that
// alone gives every SIMD SED_FIT_ENOUGH_WAVES waves; else the chunk is the length that gives SED_FIT_TARGET_WAVES, but
// never below W (a lane's warm-up is W columns, so warm-up stays at most half of its work).
#define SED_FIT_SIMDS 1024
#define SED_FIT_ENOUGH_WAVES 2
#define SED_FIT_TARGET_WAVES 4
#define SED_FIT_MAX_SPAN 65535  // columns of one lane, border column included: the 16-bit start field

static const FitRoute FIT_ROUTES[] = {
    {SED_LANE_MAXM, 64, 0, false},       // FIT_SHORT_KEYS
    {SED_FIT_LONG_MAXP, 1, 128, false},  // FIT_LONG_KEYS (128 = sed_fit_dp.h: FIT_REBASE)
    {SED_LANE_MAXM, 64, 0, true},        // FIT_F64
    {SED_FIT_LONG_MAXP, 1, 0, true},     // FIT_LONG_F64: the waves, no key field to share
};
const FitRoute &sed_fit_route_of(FitKind kind) { return FIT_ROUTES[kind]; }

// What the plan takes from the pairs through sums alone (a batch of listed pairs and an index search's cross product
// fill it their own ways): the pairs, the longest pattern, sum (n + 1) and the longest text.
struct FitSums {
    int64_t npairs = 0;
    int pmax = 0;
    double cols = 0;
    int64_t nmax = -1;
};

// The integer routes' cost envelope: scale, update addends and W from the costs and the longest pattern.
static int fit_keys_envelope(const sed_costs &c, int pmax, const FitRoute &r, sed_fit_plan_t *plan, std::string *err) {
    // the smallest S = 2^k, k <= 8, that makes every cost an integer in 0..255
    int k = 0;
    for (;; ++k) {
        if (k > 8)
            return sed_plan_fail(err, SED_E_RANGE,
                                 "fit search: the costs are not all multiples of 2^-k in 0..255 * 2^-k for any k <= 8");
        const double S = std::ldexp(1.0, k);
        auto integral = [&](double v) { const double x = v * S; return x == std::floor(x) && x >= 0 && x < 1e9; };
        auto byte = [&](double v) { return integral(v) && v * S <= 255; };
        bool ok = byte(c.ins) && integral(c.del);  // (delete's range is reported below, with P)
        for (int e = 0; e < c.K * c.K && ok; ++e) ok = byte(c.sub[e]);
        if (ok) break;
    }
    const double S = std::ldexp(1.0, k);
    const double insS = c.ins * S, delS = c.del * S;
    if ((double)pmax * delS > 65535.0)
        return sed_plan_fail(err, SED_E_RANGE, "fit search: P * delete * S = %d * %g exceeds 65535", pmax, delS);
    if (r.rebase_cols && (double)pmax * delS + (double)r.rebase_cols * insS > 65535.0)
        return sed_plan_fail(err, SED_E_RANGE, "fit search: P * delete * S + %d * insert * S = %d * %g + %d * %g exceeds 65535",
                             r.rebase_cols, pmax, delS, r.rebase_cols, insS);
    if (delS > 255.0) return sed_plan_fail(err, SED_E_RANGE, "fit search: delete * S = %g exceeds 255", delS);
    if (insS + delS > 255.0)
        return sed_plan_fail(err, SED_E_RANGE, "fit search: (insert + delete) * S = %g exceeds 255 (the update addend's byte)",
                             insS + delS);
    const uint32_t ins = (uint32_t)insS, del = (uint32_t)delS;
    plan->scale_log2 = k;
    plan->fp = sed_fit_params{};
    plan->fp.ins = ins;
    plan->fp.del = del;
    for (int a = 0; a < c.K; ++a)
        for (int b = 0; b < c.K; ++b) {
            const uint32_t v = std::min((uint32_t)(c.sub[a * c.K + b] * S), ins + del);
            plan->fp.row[a][b >> 2] |= (ins + del - v) << (8 * (b & 3));
        }
    plan->W = ins ? pmax + (int64_t)pmax * del / ins : -1;
    return SED_OK;
}

// The fp64 routes' cost envelope: the symbols, the table the kernels read, W and why there is none.
static int fit_f64_envelope(const sed_costs &c, int pmax, sed_fit_plan_t *plan, std::string *err) {
    if (c.K > SED_FIT_F64_MAXK)
        return sed_plan_fail(err, SED_E_RANGE, "fit search (fp64): the batch has %d symbols (at most %d)", c.K, SED_FIT_F64_MAXK);
    auto cost_ok = [](double v) { return std::isfinite(v) && v >= 0; };  // (-0.0 >= 0)
    if (!cost_ok(c.ins)) return sed_plan_fail(err, SED_E_RANGE, "fit search (fp64): insert = %g is not a finite cost >= 0", c.ins);
    if (!cost_ok(c.del)) return sed_plan_fail(err, SED_E_RANGE, "fit search (fp64): delete = %g is not a finite cost >= 0", c.del);
    for (int e = 0; e < c.K * c.K; ++e)
        if (!cost_ok(c.sub[e]))
            return sed_plan_fail(err, SED_E_RANGE, "fit search (fp64): cost(%d -> %d) = %g is not a finite cost >= 0", e / c.K,
                                 e % c.K, c.sub[e]);
    plan->scale_log2 = 0;
    plan->fp = sed_fit_params{};
    plan->f64_ins = c.ins + 0.0;  // (-0.0 + 0.0 = +0.0)
    plan->f64_del = c.del + 0.0;
    plan->f64_sub.assign((size_t)SED_FIT_F64_MAXK * SED_FIT_F64_MAXK, 0.0);
    for (int a = 0; a < c.K; ++a)
        for (int b = 0; b < c.K; ++b) plan->f64_sub[(size_t)a * SED_FIT_F64_MAXK + b] = c.sub[a * c.K + b] + 0.0;
    // W = P + Y, Y = floor(P delete / insert) + 2, under the hypotheses of DESIGN.md 3.6i: insert, and delete unless 0,
    // within 2^-900 .. 2^900 (no product here under- or overflows), P delete / insert <= 2^20, and, checked as
    // computed, (Y - 1) insert >= P delete (1 + 2^-30).  Anything else: one lane per text.  The argument holds for the
    // wave layout's P <= 2048 as it stands (the straight-down path's (1 + u)^2047 is below 1 + 2^-42).
    const double ins = plan->f64_ins, del = plan->f64_del, lo = std::ldexp(1.0, -900), hi = std::ldexp(1.0, 900);
    plan->W = -1;
    plan->one_lane = ins == 0 ? SED_FIT_F64_INSERT_ZERO : SED_FIT_F64_NO_WINDOW;
    if (ins >= lo && ins <= hi && (del == 0 || (del >= lo && del <= hi))) {
        const double pd = (double)pmax * del, x = pd / ins;
        if (x <= 1048576.0) {
            const double Y = std::floor(x) + 2;
            if ((Y - 1) * ins >= pd * (1 + std::ldexp(1.0, -30))) {
                plan->W = pmax + (int64_t)Y;
                plan->one_lane = SED_FIT_F64_CHUNKED;
            }
        }
    }
    return SED_OK;
}

// The one rule every caller shares: the route's envelope (scale or table, and W: a finite window exists when W >= 0),
// then the chunk length under the route's layout (its two wave constants were measured for the integer lane layout and
// are carried over to the others) and, on the integer routes, the span check.  *chunk_out = the chunk every text is
// cut by (0: one lane per text); plan->chunk = the chunk the plan reports, which cuts them the same way (it is 0 only
// where no text has more columns than the chunk, or no window exists).  *span_fail_cols > 0 (a span refusal) = the
// columns n + 1 from which a text fails, for the caller to name one.
static int fit_plan_rule(const FitRoute &r, const sed_costs &c, const sed_opts &o, const FitSums &sm, sed_fit_plan_t *plan,
                         std::string *err, int64_t *chunk_out, int64_t *span_fail_cols) {
    const int rc = r.f64 ? fit_f64_envelope(c, sm.pmax, plan, err) : fit_keys_envelope(c, sm.pmax, r, plan, err);
    if (rc != SED_OK) return rc;
    const bool window = plan->W >= 0, span_limit = !r.f64;
    int64_t chunk = 0;
    if (window && o.fit_chunk > 0)
        chunk = o.fit_chunk;
    else if (window && sm.npairs > 0 && sm.npairs < SED_FIT_ENOUGH_WAVES * SED_FIT_SIMDS * r.units_per_wave) {
        chunk = (int64_t)std::ceil(sm.cols / (double)(SED_FIT_TARGET_WAVES * SED_FIT_SIMDS * r.units_per_wave));
        chunk = std::max<int64_t>((chunk + 3) & ~(int64_t)3, plan->W);
    }
    // texts too long for one lane's start field are always split
    if (span_limit && window && o.fit_chunk == 0 && sm.nmax + 1 > SED_FIT_MAX_SPAN &&
        (chunk == 0 || chunk + plan->W + 3 > SED_FIT_MAX_SPAN))
        chunk = SED_FIT_MAX_SPAN - plan->W - 3;
    // a text of ncol columns runs in more than one lane when ncol > chunk > 0, each spanning chunk + W + 3 at most;
    // else in one lane of ncol
    const bool split = chunk > 0 && sm.nmax + 1 > chunk;
    *span_fail_cols = 0;
    if (span_limit && split && chunk + plan->W + 3 > SED_FIT_MAX_SPAN)
        *span_fail_cols = std::min<int64_t>(chunk, SED_FIT_MAX_SPAN) + 1;
    else if (span_limit && !split && sm.nmax + 1 > SED_FIT_MAX_SPAN)
        *span_fail_cols = SED_FIT_MAX_SPAN + 1;
    plan->chunk = split || (window && o.fit_chunk > 0) ? (int32_t)std::min<int64_t>(chunk, INT_MAX) : 0;
    *chunk_out = chunk;
    return SED_OK;
}
static int fit_span_fail(std::string *err, const char *what, int64_t idx, bool ins) {
    return sed_plan_fail(err, SED_E_RANGE, "fit search: %s %lld: a lane would span more than %d text columns%s", what,
                         (long long)idx, SED_FIT_MAX_SPAN, ins ? "" : " (insert = 0: a text runs as one chunk)");
}
// the integer routes' refusal of a table over more than 8 symbols, which comes before any look at the lengths (the fp64
// routes' own, fit_f64_envelope's, comes after them)
static int fit_keys_symbols_fail(const sed_costs &c, std::string *err) {
    return sed_plan_fail(err, SED_E_RANGE, "fit search: the batch has %d symbols (at most 8)", c.K);
}
// the lanes of one text under the rule's chunk, and the columns they compute (warm-up included)
static inline int64_t fit_text_lanes(int64_t chunk, int64_t W, int64_t n, double *computed) {
    const int64_t ncol = n + 1;
    const int64_t nl = chunk > 0 ? (ncol + chunk - 1) / chunk : 1;
    if (computed)
        for (int64_t l = 0; l < nl; ++l) {
            const int64_t c0 = l * chunk, c1 = nl > 1 ? std::min(ncol, c0 + chunk) : ncol;
            *computed += (double)(c1 - 1 - (c0 - sed_fit_lead(W, c0)));
        }
    return nl;
}

int sed_fit_plan_batch(FitKind kind, const sed_costs &c, const sed_opts &o, const int32_t *len_p, const int32_t *len_t,
                       int32_t npairs, sed_fit_plan_t *plan, std::string *err) {
    const FitRoute &r = sed_fit_route_of(kind);
    if (npairs < 0 || (npairs > 0 && (!len_p || !len_t))) return sed_plan_fail(err, SED_E_ARG, "bad fit arguments");
    if (!r.f64 && c.K > 8) return fit_keys_symbols_fail(c, err);
    FitSums sm;
    sm.npairs = npairs;
    for (int p = 0; p < npairs; ++p) {
        if (len_t[p] < 0) return sed_plan_fail(err, SED_E_ARG, "pair %d: negative text length", p);
        if (len_p[p] < 1 || len_p[p] > r.pmax)
            return sed_plan_fail(err, SED_E_RANGE, "fit search: pair %d: pattern length %d outside 1..%d", p, len_p[p], r.pmax);
        sm.pmax = std::max(sm.pmax, len_p[p]);
        sm.cols += (double)len_t[p] + 1;
        sm.nmax = std::max<int64_t>(sm.nmax, len_t[p]);
    }
    int64_t chunk = 0, span_cols = 0;
    const int rc = fit_plan_rule(r, c, o, sm, plan, err, &chunk, &span_cols);
    if (rc != SED_OK) return rc;
    plan->first.assign((size_t)npairs + 1, 0);
    plan->cells = plan->nominal = 0;
    for (int p = 0; p < npairs; ++p) {
        if (span_cols && (int64_t)len_t[p] + 1 >= span_cols) return fit_span_fail(err, "pair", p, plan->fp.ins != 0);
        double computed = 0;
        plan->first[p + 1] = plan->first[p] + fit_text_lanes(chunk, plan->W, len_t[p], &computed);
        plan->cells += (double)len_p[p] * computed;
        plan->nominal += (double)len_p[p] * (double)len_t[p];
    }
    plan->lanes = plan->first[npairs];
    if (plan->lanes > INT_MAX) return sed_plan_fail(err, SED_E_RANGE, "fit search: %lld lanes", (long long)plan->lanes);
    return SED_OK;
}

int sed_fit_plan_index(FitKind kind, const sed_costs &c, const sed_opts &o, const int32_t *len_p, int32_t nqueries,
                       const sed_fit_index_sums &tx, sed_fit_plan_t *plan, std::vector<int32_t> *rows, std::string *err) {
    const FitRoute &r = sed_fit_route_of(kind);
    if (nqueries < 0 || (nqueries > 0 && !len_p) || tx.ntexts < 0) return sed_plan_fail(err, SED_E_ARG, "bad fit arguments");
    if (!r.f64 && c.K > 8) return fit_keys_symbols_fail(c, err);
    FitSums sm;
    double psum = 0;
    // the refusals of the cross product's pairs, query-major, in sed_fit_plan_batch's order: pair (0, 0)'s text, then its
    // pattern, then the other texts (pairs (0, d)), then the other patterns; an empty cross product has no pair to refuse
    for (int q = 0; q < nqueries && tx.ntexts > 0; ++q) {
        if (tx.first_negative >= 0 && (q == 0 ? tx.first_negative == 0 : q == 1))
            return sed_plan_fail(err, SED_E_ARG, "text %d: negative text length", tx.first_negative);
        if (len_p[q] < 1 || len_p[q] > r.pmax)
            return sed_plan_fail(err, SED_E_RANGE, "fit search: query %d: pattern length %d outside 1..%d", q, len_p[q], r.pmax);
        if (r.waves() && o.fit_rows && len_p[q] > 64 * o.fit_rows)  // (the wave layout reads the option)
            return sed_plan_fail(err, SED_E_RANGE, "fit search: query %d: pattern length %d exceeds the 64 * %d rows of SED_OPT_FIT_ROWS",
                                 q, len_p[q], o.fit_rows);
        sm.pmax = std::max(sm.pmax, len_p[q]);
        psum += (double)len_p[q];
    }
    if (nqueries == 1 && tx.ntexts > 0 && tx.first_negative >= 0)
        return sed_plan_fail(err, SED_E_ARG, "text %d: negative text length", tx.first_negative);
    if (nqueries > 0 && tx.ntexts > 0) {
        sm.npairs = (int64_t)nqueries * tx.ntexts;
        sm.cols = (double)nqueries * tx.cols;
        sm.nmax = tx.nmax;
    }
    int64_t chunk = 0, span_cols = 0;
    const int rc = fit_plan_rule(r, c, o, sm, plan, err, &chunk, &span_cols);
    if (rc != SED_OK) return rc;
    if (span_cols) return fit_span_fail(err, "a text of length", tx.nmax, plan->fp.ins != 0);
    plan->first.clear();
    plan->lanes = 0;
    plan->cells = 0;
    plan->nominal = psum * (tx.cols - (double)tx.ntexts);
    if (rows) {
        rows->resize(r.waves() ? (size_t)nqueries : 0);
        for (size_t q = 0; q < rows->size(); ++q) (*rows)[q] = o.fit_rows ? o.fit_rows : sed_fit_long_rows(len_p[q]);
    }
    return SED_OK;
}

int64_t sed_fit_build_chunks(const sed_fit_plan_t &plan, const int32_t *len_t, int32_t ntexts,
                             std::vector<sed_fit_chunk> *chunks, double *computed) {
    int64_t total = 0;
    if (chunks) chunks->clear();
    for (int d = 0; d < ntexts; ++d) {
        const int64_t nl = fit_text_lanes(plan.chunk, plan.W, len_t[d], computed);
        total += nl;
        if (chunks)
            for (int64_t l = 0; l < nl; ++l) chunks->push_back(sed_fit_chunk{d, (int32_t)(l * plan.chunk)});
    }
    return total;
}

int sed_fit_cutoff_rule(const sed_fit_plan_t &plan, double max_dist, int32_t *cut, std::string *err) {
    if (!(max_dist >= 0))
        return sed_plan_fail(err, SED_E_ARG, "fit hits: max_dist = %g is not a distance (NaN or negative)", max_dist);
    const double scaled = std::floor(std::ldexp(max_dist, plan.scale_log2));
    *cut = scaled >= (double)SED_FIT_CUT_ALL ? SED_FIT_CUT_ALL : (int32_t)scaled;
    return SED_OK;
}

void sed_fit_build_lanes(const sed_fit_plan_t &plan, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                         std::vector<sed_fit_lane> &lanes) {
    lanes.assign((size_t)plan.lanes, sed_fit_lane{});
    for (int p = 0; p < npairs; ++p) {
        const int64_t ncol = (int64_t)len_t[p] + 1, nl = plan.first[p + 1] - plan.first[p];
        for (int64_t l = 0; l < nl; ++l) {
            const int64_t c0 = l * plan.chunk, c1 = nl > 1 ? std::min(ncol, c0 + plan.chunk) : ncol;
            const int32_t lead = sed_fit_lead(plan.W, c0);
            sed_fit_lane &ln = lanes[(size_t)(plan.first[p] + l)];
            ln.tw = (uint32_t)((c0 - lead) / 4);
            ln.pair = p;
            ln.pat = 0;
            ln.plen = len_p[p];
            ln.nsteps = (int32_t)(c1 - 1 - (c0 - lead));
            ln.lead = lead;
            ln.cnt = (int32_t)(c1 - c0);
            ln.c0 = (int32_t)c0;
        }
    }
}

// ---- the device-free exports: a few bodies, each taking the route ----
// The cost model and options as every export takes them, gathered where the C function is entered.
struct FitCArgs {
    int K;
    const double *sub;
    const uint8_t *sub_int;
    double ins;
    int ins_is_int;
    double del;
    int del_is_int;
    const int32_t *options;
    int noptions;
};
#define FIT_C_ARGS (FitCArgs{K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions})

static int fit_costs_of(const FitCArgs &a, sed_costs *c, sed_opts *o) {
    const int K = a.K;
    if (K < 1 || K > 255 || !a.sub || a.noptions < 0 || (a.noptions && !a.options)) return SED_E_ARG;
    if (!std::isfinite(a.ins) || !std::isfinite(a.del)) return SED_E_ARG;
    for (int e = 0; e < K * K; ++e)
        if (!std::isfinite(a.sub[e])) return SED_E_ARG;
    c->K = K;
    c->sub.assign(a.sub, a.sub + K * K);
    if (a.sub_int) c->sub_int.assign(a.sub_int, a.sub_int + K * K);
    c->ins = a.ins;
    c->del = a.del;
    c->ins_int = a.ins_is_int ? 1 : 0;
    c->del_int = a.del_is_int ? 1 : 0;
    for (int i = 0; i < a.noptions; ++i)
        if (!sed_opts_set(*o, a.options[2 * i], a.options[2 * i + 1], true)) return SED_E_ARG;
    return SED_OK;
}
// the texts' sums as an index keeps them, from their lengths
static sed_fit_index_sums fit_text_sums(const int32_t *len_t, int32_t ntexts) {
    sed_fit_index_sums tx;
    tx.ntexts = ntexts;
    for (int d = 0; d < ntexts; ++d) {
        if (len_t[d] < 0 && tx.first_negative < 0) tx.first_negative = d;
        tx.cols += (double)len_t[d] + 1;
        tx.nmax = std::max<int64_t>(tx.nmax, len_t[d]);
    }
    return tx;
}
static bool fit_index_lengths_ok(int32_t nqueries, const int32_t *len_t, int32_t ntexts) {
    return nqueries >= 0 && ntexts >= 0 && (ntexts == 0 || len_t);
}

// the plan of listed pairs from the C arguments
static int fit_pairs_plan_of(FitKind kind, const FitCArgs &a, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                             sed_fit_plan_t *p) {
    sed_costs c;
    sed_opts o;
    const int rc = fit_costs_of(a, &c, &o);
    return rc != SED_OK ? rc : sed_fit_plan_batch(kind, c, o, len_p, len_t, npairs, p, nullptr);
}
// the plan of a cross product from the C arguments, the chunk table (may be null) and the sums the plan reports
static int fit_index_plan_of(FitKind kind, const FitCArgs &a, const int32_t *len_p, int32_t nqueries, const int32_t *len_t,
                             int32_t ntexts, sed_fit_plan_t *p, std::vector<sed_fit_chunk> *chunks, std::vector<int32_t> *rows) {
    if (!fit_index_lengths_ok(nqueries, len_t, ntexts)) return SED_E_ARG;
    sed_costs c;
    sed_opts o;
    const int rc0 = fit_costs_of(a, &c, &o);
    if (rc0 != SED_OK) return rc0;
    const int rc = sed_fit_plan_index(kind, c, o, len_p, nqueries, fit_text_sums(len_t, ntexts), p, rows, nullptr);
    if (rc != SED_OK) return rc;
    double computed = 0, psum = 0;
    const int64_t nchunks = nqueries > 0 ? sed_fit_build_chunks(*p, len_t, ntexts, chunks, &computed) : 0;
    for (int q = 0; q < nqueries && ntexts > 0; ++q) psum += (double)len_p[q];
    p->lanes = nqueries * nchunks;
    p->cells = psum * computed;
    return p->lanes > INT_MAX ? SED_E_RANGE : SED_OK;
}

// What the _plan exports report of a plan that stands (rc = its planning's result, handed through): FIT_PLAN_FIELDS of
// sedgpu.py; the fp64 routes have no scale (0.0) and add one_lane.
static int fit_plan_out(FitKind kind, int rc, const sed_fit_plan_t &p, double *out, int nout) {
    if (rc != SED_OK) return rc;
    const bool f64 = sed_fit_route_of(kind).f64;
    const double v[] = {f64 ? 0.0 : std::ldexp(1.0, p.scale_log2), (double)p.W, (double)p.chunk, (double)p.lanes, p.cells,
                        p.nominal, (double)p.one_lane};
    for (int i = 0; i < nout && i < (f64 ? 7 : 6); ++i) out[i] = v[i];
    return SED_OK;
}
static int fit_pairs_plan_export(FitKind kind, const FitCArgs &a, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                                 double *out, int nout) {
    if (nout < 0 || (nout && !out)) return SED_E_ARG;
    sed_fit_plan_t p;
    return fit_plan_out(kind, fit_pairs_plan_of(kind, a, len_p, len_t, npairs, &p), p, out, nout);
}
static int fit_index_plan_export(FitKind kind, const FitCArgs &a, const int32_t *len_p, int32_t nqueries, const int32_t *len_t,
                                 int32_t ntexts, double *out, int nout, int32_t *out_rows) {
    if (nout < 0 || (nout && !out)) return SED_E_ARG;
    sed_fit_plan_t p;
    std::vector<int32_t> rows;
    const int rc = fit_plan_out(kind, fit_index_plan_of(kind, a, len_p, nqueries, len_t, ntexts, &p, nullptr, &rows), p, out, nout);
    if (rc == SED_OK && out_rows && !rows.empty()) std::memcpy(out_rows, rows.data(), rows.size() * sizeof(int32_t));
    return rc;
}

// The _lanes exports: the records, and on the integer routes the kernel's parameter words (out_params; the fp64
// exports have none and pass null).
static_assert(sizeof(sed_fit_lane) == 8 * sizeof(int32_t), "a lane record is eight 32-bit words");
static bool fit_lanes_args_ok(FitKind kind, const int32_t *out_lanes, int64_t max_lanes, const uint32_t *out_params) {
    return max_lanes >= 0 && (max_lanes == 0 || out_lanes) && (sed_fit_route_of(kind).f64 || out_params);
}
static void fit_params_out(const sed_fit_params &fp, uint32_t *out_params) {
    if (!out_params) return;
    for (int a = 0; a < 8; ++a) {
        out_params[2 * a] = fp.row[a][0];
        out_params[2 * a + 1] = fp.row[a][1];
    }
    out_params[16] = fp.ins;
    out_params[17] = fp.del;
}
static int fit_pairs_lanes_export(FitKind kind, const FitCArgs &a, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                                  int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params) {
    if (!fit_lanes_args_ok(kind, out_lanes, max_lanes, out_params)) return SED_E_ARG;
    sed_fit_plan_t p;
    const int rc = fit_pairs_plan_of(kind, a, len_p, len_t, npairs, &p);
    if (rc != SED_OK) return rc;
    if (p.lanes > max_lanes) return SED_E_ARG;
    std::vector<sed_fit_lane> lanes;
    sed_fit_build_lanes(p, len_p, len_t, npairs, lanes);
    if (!lanes.empty()) std::memcpy(out_lanes, lanes.data(), lanes.size() * sizeof(sed_fit_lane));
    fit_params_out(p.fp, out_params);
    return SED_OK;
}
static int fit_index_lanes_export(FitKind kind, const FitCArgs &a, const int32_t *len_p, int32_t nqueries, const int32_t *len_t,
                                  int32_t ntexts, int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params) {
    if (!fit_lanes_args_ok(kind, out_lanes, max_lanes, out_params)) return SED_E_ARG;
    sed_fit_plan_t p;
    std::vector<sed_fit_chunk> chunks;
    std::vector<int32_t> rows;
    const int rc = fit_index_plan_of(kind, a, len_p, nqueries, len_t, ntexts, &p, &chunks, &rows);
    if (rc != SED_OK) return rc;
    if (p.lanes > max_lanes) return SED_E_ARG;
    sed_fit_lane *out = (sed_fit_lane *)out_lanes;
    for (int q = 0; q < nqueries; ++q)  // the kernel's own derivation, with each text at word 0
        for (const sed_fit_chunk &ck : chunks) {
            sed_fit_lane ln = sed_fit_derive_lane(ck, sed_fit_text{0u, len_t[ck.text]}, p.chunk, len_p[q], p.W);
            ln.pair = q * ntexts + ck.text;
            *out++ = ln;
        }
    fit_params_out(p.fp, out_params);
    return SED_OK;
}

// The route exports: plan(kind, costs, options, err) = the planner's answer for the call's lengths.  The integer route
// when it serves; else, when its refusal is one of range (bad arguments are bad for both), the fp64 route or both
// refusals, the integer one's first.
template <class Plan>
static int fit_route_export(const FitCArgs &a, bool lengths_ok, FitKind keys, FitKind f64, char *why, int why_len, Plan plan) {
    if (why_len < 0 || (why_len && !why)) return SED_E_ARG;
    if (why_len) why[0] = 0;
    if (!lengths_ok) return SED_E_ARG;
    sed_costs c;
    sed_opts o;
    int rc = fit_costs_of(a, &c, &o);
    if (rc != SED_OK) return rc;
    std::string e_int, e_f64;
    if ((rc = plan(keys, c, o, &e_int)) == SED_OK) return SED_FIT_ROUTE_INT;
    if (rc != SED_E_RANGE) return rc;
    rc = plan(f64, c, o, &e_f64);
    const std::string text = rc == SED_OK ? e_int : e_int + "; " + e_f64;
    if (why_len) std::snprintf(why, (size_t)why_len, "%s", text.c_str());
    return rc == SED_OK ? SED_FIT_ROUTE_F64 : rc;
}

extern "C" {

int sed_fit_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
                 const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                 double *out, int nout) {
    return fit_pairs_plan_export(FIT_SHORT_KEYS, FIT_C_ARGS, len_p, len_t, npairs, out, nout);
}
int sed_fit_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
                     const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                     double *out, int nout) {
    return fit_pairs_plan_export(FIT_F64, FIT_C_ARGS, len_p, len_t, npairs, out, nout);
}

int sed_fit_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
                  const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                  int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params) {
    return fit_pairs_lanes_export(FIT_SHORT_KEYS, FIT_C_ARGS, len_p, len_t, npairs, out_lanes, max_lanes, out_params);
}
int sed_fit_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
                      const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t, int32_t npairs,
                      int32_t *out_lanes, int64_t max_lanes) {
    return fit_pairs_lanes_export(FIT_F64, FIT_C_ARGS, len_p, len_t, npairs, out_lanes, max_lanes, nullptr);
}

int sed_fit_cutoff_scaled(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                          int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t,
                          int32_t npairs, double max_dist, int64_t *out) {
    if (!out) return SED_E_ARG;
    sed_fit_plan_t p;
    const int rc = fit_pairs_plan_of(FIT_SHORT_KEYS, FIT_C_ARGS, len_p, len_t, npairs, &p);
    if (rc != SED_OK) return rc;
    int32_t cut = 0;
    const int rc2 = sed_fit_cutoff_rule(p, max_dist, &cut, nullptr);
    if (rc2 == SED_OK) *out = cut;
    return rc2;
}

int sed_fit_index_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                       int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                       const int32_t *len_t, int32_t ntexts, double *out, int nout) {
    return fit_index_plan_export(FIT_SHORT_KEYS, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out, nout, nullptr);
}
int sed_fit_index_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                           int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                           const int32_t *len_t, int32_t ntexts, double *out, int nout) {
    return fit_index_plan_export(FIT_F64, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out, nout, nullptr);
}
int sed_fit_index_long_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                            int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                            const int32_t *len_t, int32_t ntexts, double *out, int nout, int32_t *out_rows) {
    return fit_index_plan_export(FIT_LONG_KEYS, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out, nout, out_rows);
}
int sed_fit_index_long_f64_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                                int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                                const int32_t *len_t, int32_t ntexts, double *out, int nout, int32_t *out_rows) {
    return fit_index_plan_export(FIT_LONG_F64, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out, nout, out_rows);
}

int sed_fit_index_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                        int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                        const int32_t *len_t, int32_t ntexts, int32_t *out_lanes, int64_t max_lanes, uint32_t *out_params) {
    return fit_index_lanes_export(FIT_SHORT_KEYS, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out_lanes, max_lanes, out_params);
}
int sed_fit_index_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                            int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                            const int32_t *len_t, int32_t ntexts, int32_t *out_lanes, int64_t max_lanes) {
    return fit_index_lanes_export(FIT_F64, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out_lanes, max_lanes, nullptr);
}
int sed_fit_index_long_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                             int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                             const int32_t *len_t, int32_t ntexts, int32_t *out_lanes, int64_t max_lanes,
                             uint32_t *out_params) {
    return fit_index_lanes_export(FIT_LONG_KEYS, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out_lanes, max_lanes, out_params);
}
int sed_fit_index_long_f64_lanes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                                 int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                                 const int32_t *len_t, int32_t ntexts, int32_t *out_lanes, int64_t max_lanes) {
    return fit_index_lanes_export(FIT_LONG_F64, FIT_C_ARGS, len_p, nqueries, len_t, ntexts, out_lanes, max_lanes, nullptr);
}

int sed_fit_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
                  const int32_t *options, int noptions, const int32_t *len_p, const int32_t *len_t, int32_t npairs, char *why,
                  int why_len) {
    return fit_route_export(FIT_C_ARGS, true, FIT_SHORT_KEYS, FIT_F64, why, why_len,
                            [&](FitKind kind, const sed_costs &c, const sed_opts &o, std::string *err) {
                                sed_fit_plan_t p;
                                return sed_fit_plan_batch(kind, c, o, len_p, len_t, npairs, &p, err);
                            });
}
int sed_fit_long_route(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                       int del_is_int, const int32_t *options, int noptions, const int32_t *len_p, int32_t nqueries,
                       const int32_t *len_t, int32_t ntexts, char *why, int why_len) {
    const bool ok = fit_index_lengths_ok(nqueries, len_t, ntexts);
    const sed_fit_index_sums tx = ok ? fit_text_sums(len_t, ntexts) : sed_fit_index_sums{};
    return fit_route_export(FIT_C_ARGS, ok, FIT_LONG_KEYS, FIT_LONG_F64, why, why_len,
                            [&](FitKind kind, const sed_costs &c, const sed_opts &o, std::string *err) {
                                sed_fit_plan_t p;
                                return sed_fit_plan_index(kind, c, o, len_p, nqueries, tx, &p, nullptr, err);
                            });
}

}  // extern "C"
