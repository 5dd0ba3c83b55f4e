// sed_fit_runtime.cpp — fit search's entry points of the C-ABI (include/sed.h): sed_fit_search over listed pairs, and
// sed_fit_index_* over a resident text index (best hit per (query, text), or every hit within a distance), each also as
// its _f64 sibling, the index calls also as _long and _long_f64.  What a search runs is the fit planner's decision
// (sed_fit_plan.cpp), the kernels are sed_fit.hip, sed_fit_long.hip, sed_fit_f64.hip and sed_fit_long_f64.hip; here: pack, reserve, upload, launch, download, decode, on the context's stream
// (sed_runtime.h).  The routes of a call differ in the plan, the launch and the decoding, and share the staging.
#include "sed_fit_plan.h"
#include "sed_runtime.h"

#include <climits>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

// The events around a search's kernels (carried by the launches, sed_fit.hip), created on first use.
struct FitTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;  // the last search ran to its end: the events hold its time
    ~FitTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // before a launch: nothing is timed until the caller sets `timed` after its wait
    hipError_t begin() {
        hipError_t e = hipSuccess;
        for (hipEvent_t &x : ev)
            if (!x && (e = hipEventCreate(&x)) != hipSuccess) return e;
        timed = false;
        return hipSuccess;
    }
    int elapsed(float *ms) const {
        if (!timed) return SED_E_STATE;
        return hipEventElapsedTime(ms, ev[0], ev[1]) == hipSuccess ? SED_OK : SED_E_DEVICE;
    }
};

// sed_fit_search's device arrays and the timer of its kernel, kept across calls
struct sed_fit_state {
    DevBuf text, pat, lanes, out;
    DevBuf rec, tab;  // the fp64 route's per-lane records and its cost table
    FitTimer timer;
    ~sed_fit_state() { text.release(); pat.release(); lanes.release(); out.release(); rec.release(); tab.release(); }
};
void sed_fit_state_destroy(sed_fit_state *s) { delete s; }

// What every search refuses first, in this order, then the context's device.  args_ok = the entry point's own check
// of its arguments.
static int fit_enter(sed_ctx *c, bool args_ok) {
    if (!c) return SED_E_ARG;
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (!args_ok) return c->fail(SED_E_ARG, "bad fit arguments");
    if (!c->have_costs) return c->fail(SED_E_STATE, "sed_set_costs() was not called");
    (void)hipSetDevice(c->device);
    return SED_OK;
}

// A pattern record as the kernels read it (sed_fit_dp.h): `rows` byte codes (SED_LANE_MAXM; the long kernels' 64 R,
// sed_fit_long.hip), the pattern right-aligned, code 8 in front.  Returns the first code outside the alphabet, or -1.
static int fit_pack_pattern(uint8_t *rec, const uint8_t *codes, int P, int K, int rows = SED_LANE_MAXM) {
    memset(rec, 8, (size_t)(rows - P));
    for (int i = 0; i < P; ++i)
        if ((rec[rows - P + i] = codes[i]) >= K) return codes[i];
    return -1;
}

// A result key D << 48 | end << 16 | (end - start) of a text of text_len symbols; false = no result (the preset key, or
// one no lane of that text can have written).  inv = 1 / S.
static bool fit_decode_key(uint64_t k, int32_t text_len, double inv, double *dist, int32_t *start, int32_t *end) {
    const int64_t e = (int64_t)((k >> 16) & 0xFFFFFFFFu), len = (int64_t)(k & 0xFFFFu);
    if (k == ~0ull || e > text_len || len > e) return false;
    *dist = (double)(k >> 48) * inv;
    *end = (int32_t)e;
    *start = (int32_t)(e - len);
    return true;
}

// A result record of the fp64 kernels (sed_fit_f64.hip) for a text of text_len symbols; false = no result (the preset
// bytes, or one no lane of that text can have written).
static bool fit_decode_f64(const sed_fit_f64_best &b, int32_t text_len, double *dist, int32_t *start, int32_t *end) {
    if (!(b.D >= 0) || b.end < 0 || b.end > text_len || b.start < 0 || b.start > b.end) return false;
    *dist = b.D;
    *start = b.start;
    *end = b.end;
    return true;
}
// The fp64 plan's cost table on the device, and the kernels' cost arguments
static hipError_t fit_f64_costs_upload(sed_ctx *c, const sed_fit_plan_t &plan, DevBuf &tab, sed_fit_f64_costs *fc) {
    if (!tab.reserve(plan.f64_sub.size() * sizeof(double))) return hipErrorOutOfMemory;
    *fc = sed_fit_f64_costs{(const double *)tab.p, plan.f64_ins, plan.f64_del};
    return hipMemcpyAsync(tab.p, plan.f64_sub.data(), plan.f64_sub.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
}

// The planner decides scale, window and lanes from the lengths and builds the lane records (sed_fit_plan.cpp:
// sed_fit_plan_batch, sed_fit_build_lanes); here the distinct patterns become records and the distinct texts one buffer
// in which each starts 4-byte aligned, so pairs that share a pattern or a text through their offsets share its copy.
// sed_fit_search and sed_fit_search_f64: the plan, the launch and the decoding differ, nothing else.
static int fit_search_of(sed_ctx *c, bool f64, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                         const uint8_t *codes_t, const int64_t *off_t, const int32_t *len_t, int32_t npairs, double *out_dist,
                         int32_t *out_start, int32_t *out_end) {
    int rc = fit_enter(c, npairs == 0 || (npairs > 0 && codes_p && off_p && len_p && codes_t && off_t && len_t && out_dist &&
                                          out_start && out_end));
    if (rc != SED_OK) return rc;
    sed_fit_plan_t plan;
    rc = sed_fit_plan_batch(f64 ? FIT_F64 : FIT_SHORT_KEYS, c->costs, c->opt, len_p, len_t, npairs, &plan, &c->err);
    if (rc != SED_OK || npairs == 0) return rc;
    const int K = c->costs.K;
    struct Span {
        int64_t off;
        int32_t len;
        bool operator==(const Span &o) const { return off == o.off && len == o.len; }
    };
    struct SpanHash {
        size_t operator()(const Span &s) const { return std::hash<int64_t>()(s.off * 0x9E3779B97F4A7C15ll + s.len); }
    };
    std::unordered_map<Span, int64_t, SpanHash> pat_of, text_of;
    std::vector<uint8_t> pats, text;
    std::vector<sed_fit_lane> lanes;
    sed_fit_build_lanes(plan, len_p, len_t, npairs, lanes);
    for (int p = 0; p < npairs; ++p) {
        if (off_p[p] < 0 || off_t[p] < 0) return c->fail(SED_E_ARG, "pair %d: negative offset", p);
        const int P = len_p[p], n = len_t[p];
        auto pi = pat_of.find(Span{off_p[p], P});
        if (pi == pat_of.end()) {
            pi = pat_of.emplace(Span{off_p[p], P}, (int64_t)(pats.size() / SED_LANE_MAXM)).first;
            pats.resize(pats.size() + SED_LANE_MAXM);
            const int bad = fit_pack_pattern(pats.data() + pats.size() - SED_LANE_MAXM, codes_p + off_p[p], P, K);
            if (bad >= 0) return c->fail(SED_E_ARG, "pair %d: pattern code %d outside the alphabet (K=%d)", p, bad, K);
        }
        auto ti = text_of.find(Span{off_t[p], n});
        if (ti == text_of.end()) {
            ti = text_of.emplace(Span{off_t[p], n}, (int64_t)(text.size() / 4)).first;
            const size_t at = text.size();
            text.resize(at + (((size_t)n + 3) & ~(size_t)3), 0);
            uint8_t top = 0;
            for (int j = 0; j < n; ++j) top |= (text[at + j] = codes_t[off_t[p] + j]) >= K ? 0x80 : 0;
            if (top) return c->fail(SED_E_ARG, "pair %d: a text code is outside the alphabet (K=%d)", p, K);
            if (text.size() / 4 > 0xFFFFFFF0u) return c->fail(SED_E_RANGE, "fit search: more than 16 GB of text");
        }
        for (int64_t l = plan.first[p]; l < plan.first[p + 1]; ++l) {  // the planner's records, at this text's copy
            lanes[(size_t)l].tw += (uint32_t)ti->second;
            lanes[(size_t)l].pat = (int32_t)pi->second;
        }
    }
    text.resize(text.size() + 16, 0);  // (a lane reads one word past its last)
    if (!c->fit) c->fit = new sed_fit_state;
    sed_fit_state &f = *c->fit;
    const size_t outbytes = (f64 ? sizeof(sed_fit_f64_best) : 8) * (size_t)npairs;
    if (!f.text.reserve(text.size()) || !f.pat.reserve(pats.size()) || !f.lanes.reserve(lanes.size() * sizeof(sed_fit_lane)) ||
        !f.out.reserve(outbytes) || (f64 && !f.rec.reserve(lanes.size() * sizeof(sed_fit_f64_best))))
        return c->fail(SED_E_OOM, "device allocation failed (fit search, %zu text bytes)", text.size());
    hipError_t e = hipSuccess;
    if ((e = f.timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    std::vector<uint64_t> keys(outbytes / 8);
    sed_fit_f64_costs fc{};
    if (f64 && (e = fit_f64_costs_upload(c, plan, f.tab, &fc)) != hipSuccess) return c->hipfail(e, "upload (fit search costs)");
    if ((e = hipMemcpyAsync(f.text.p, text.data(), text.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(f.pat.p, pats.data(), pats.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(f.lanes.p, lanes.data(), lanes.size() * sizeof(sed_fit_lane), hipMemcpyHostToDevice,
                            c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(f.out.p, 0xFF, outbytes, c->stream)) != hipSuccess)
        return c->hipfail(e, "upload (fit search)");
    if (f64) {
        if ((e = sed_launch_fit_f64(c->stream, f.timer.ev[0], f.timer.ev[1], (const sed_fit_lane *)f.lanes.p, (int)lanes.size(),
                                    f.pat.p, f.text.p, (sed_fit_f64_best *)f.rec.p, (sed_fit_f64_best *)f.out.p, fc)) != hipSuccess)
            return c->hipfail(e, "fit fp64 kernel launch");
    } else if ((e = sed_launch_fit(c->stream, f.timer.ev[0], f.timer.ev[1], (const sed_fit_lane *)f.lanes.p, (int)lanes.size(),
                            f.pat.p, f.text.p, (unsigned long long *)f.out.p, plan.fp)) != hipSuccess)
        return c->hipfail(e, "fit kernel launch");
    if ((e = hipMemcpyAsync(keys.data(), f.out.p, outbytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "download (fit search)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "fit kernel execution");
    f.timer.timed = true;
    const double inv = std::ldexp(1.0, -plan.scale_log2);
    const sed_fit_f64_best *best = (const sed_fit_f64_best *)keys.data();
    for (int p = 0; p < npairs; ++p)
        if (f64 ? !fit_decode_f64(best[p], len_t[p], &out_dist[p], &out_start[p], &out_end[p])
                : !fit_decode_key(keys[p], len_t[p], inv, &out_dist[p], &out_start[p], &out_end[p]))
            return c->fail(SED_E_DEVICE, "pair %d: no fit result from the device", p);
    return SED_OK;
}

extern "C" {

int sed_fit_search(sed_ctx *c, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p, const uint8_t *codes_t,
                   const int64_t *off_t, const int32_t *len_t, int32_t npairs, double *out_dist, int32_t *out_start,
                   int32_t *out_end) {
    return fit_search_of(c, false, codes_p, off_p, len_p, codes_t, off_t, len_t, npairs, out_dist, out_start, out_end);
}
int sed_fit_search_f64(sed_ctx *c, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p, const uint8_t *codes_t,
                       const int64_t *off_t, const int32_t *len_t, int32_t npairs, double *out_dist, int32_t *out_start,
                       int32_t *out_end) {
    return fit_search_of(c, true, codes_p, off_p, len_p, codes_t, off_t, len_t, npairs, out_dist, out_start, out_end);
}

int sed_fit_last_time(const sed_ctx *c, float *kernel_ms) {
    return !c || !kernel_ms ? SED_E_ARG : c->fit ? c->fit->timer.elapsed(kernel_ms) : SED_E_STATE;
}

}  // extern "C"

// Fit search over a resident index (include/sed.h).  The index holds what no query changes: the packed texts, one
// record per text, and for the chunk length of the last search one record per (text, chunk).  A search plans the
// queries x texts cross product from the index's sums (sed_fit_plan.cpp: sed_fit_plan_index), uploads the queries'
// pattern records and lengths from pinned memory, and launches one lane per (query, chunk record); the kernel derives
// each lane (sed_internal.h: sed_fit_derive_lane).  Per search the host touches the queries and the results only.
struct sed_fit_hit_rec {  // one record of the device hit list (sed_fit_dp.h: sed_fit_append)
    uint32_t pair, end, len, D;
};
struct sed_fit_index {
    sed_ctx *ctx = nullptr;
    sed_fit_index_sums sums;
    int64_t symbols = 0;
    int maxcode = -1;              // the largest text code (a search under K symbols needs maxcode < K)
    std::vector<int32_t> len_t;    // the texts' lengths: the chunk table's input, and the bound of every reported end
    DevBuf d_text, d_trec, d_chunks, d_query, d_out;
    bool have_chunks = false;      // d_chunks holds the table of chunk length `chunk`, nchunks records
    int32_t chunk = 0;
    int64_t nchunks = 0;
    std::vector<sed_fit_chunk> h_chunks;
    // pinned host memory: [result keys (queries x texts) | pattern records | pattern lengths] of the search under way
    PinBuf pin;
    FitTimer timer;
    // hits searches (sed_fit_index_hits): the device hit list, grown to the largest cap seen, its 64-bit counter, the
    // host copy the records are sorted in, and the timer of the hits kernel; none shared with a search's
    DevBuf d_hits, d_count;
    std::vector<sed_fit_hit_rec> h_hits;
    // the fp64 route (sed_fit_f64.hip): the lanes' records of a search, the cost table, and a hits search's host copy
    // (its device list is d_hits, sized in its own records)
    DevBuf d_rec, d_tab;
    std::vector<sed_fit_f64_hit> h_hits64;
    FitTimer hits_timer;
    ~sed_fit_index() {
        pin.release();
        d_text.release(); d_trec.release(); d_chunks.release(); d_query.release(); d_out.release();
        d_hits.release(); d_count.release();
        d_rec.release(); d_tab.release();
    }
};

// The queries of a long call in launch order: grouped by their rows per lane R, ascending, each group in query order.
// Group g = places first .. first + count) of qlist, its records 64 R bytes each from byte `at` of the pattern area.
struct FitLongGroups {
    struct Group {
        int rows, first, count;
        size_t at;
    };
    std::vector<Group> groups;
    const int32_t *d_qlist = nullptr;  // the device copy of qlist (place -> query)
};

// What a search and a hits search share once their plan stands (nqueries, ntexts > 0): the chunk table of the plan's
// chunk length, the pinned buffer [front bytes of the caller's | pattern records | pattern lengths], the queries packed
// into it and sent to the device, and the kernel's arguments but for its output.  A long call (rows = each query's R,
// lg = its groups, out) lays the pattern records out group by group, 64 R bytes a query, and appends qlist.
static int fit_index_stage(sed_fit_index *ix, const sed_fit_plan_t &plan, const uint8_t *codes_p, const int64_t *off_p,
                           const int32_t *len_p, int32_t nqueries, size_t front, sed_fit_index_args *args,
                           const std::vector<int32_t> *rows = nullptr, FitLongGroups *lg = nullptr) {
    sed_ctx *c = ix->ctx;
    const int ntexts = ix->sums.ntexts;
    const int K = c->costs.K;
    if (ix->maxcode >= K)
        return c->fail(SED_E_ARG, "fit index: it holds text code %d, outside the alphabet (K=%d)", ix->maxcode, K);
    hipError_t e = hipSuccess;
    // the chunk table: the last search's when the chunk length is the same
    if (!ix->have_chunks || ix->chunk != plan.chunk) {
        ix->have_chunks = false;
        ix->nchunks = sed_fit_build_chunks(plan, ix->len_t.data(), ntexts, &ix->h_chunks, nullptr);
        if (!ix->d_chunks.reserve(ix->h_chunks.size() * sizeof(sed_fit_chunk)))
            return c->fail(SED_E_OOM, "device allocation failed (fit index, %lld chunk records)", (long long)ix->nchunks);
        if ((e = hipMemcpyAsync(ix->d_chunks.p, ix->h_chunks.data(), ix->h_chunks.size() * sizeof(sed_fit_chunk),
                                hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return c->hipfail(e, "upload (fit index chunk table)");
        ix->chunk = plan.chunk;
        ix->have_chunks = true;
    }
    if ((int64_t)nqueries * ix->nchunks > INT_MAX)
        return c->fail(SED_E_RANGE, "fit search: %lld lanes", (long long)nqueries * ix->nchunks);
    // where each query's record goes: by query, or (long) by group
    std::vector<size_t> rec_at((size_t)nqueries);
    std::vector<int32_t> place_q;
    size_t patbytes = 0;
    if (rows) {
        lg->groups.clear();
        for (int R = 2; R <= 32; R *= 2) {
            FitLongGroups::Group g{R, (int)place_q.size(), 0, patbytes};
            for (int q = 0; q < nqueries; ++q)
                if ((*rows)[q] == R) {
                    rec_at[q] = patbytes;
                    patbytes += (size_t)64 * R;
                    place_q.push_back(q);
                }
            if ((g.count = (int)place_q.size() - g.first) > 0) lg->groups.push_back(g);
        }
    } else {
        for (int q = 0; q < nqueries; ++q) rec_at[q] = (size_t)SED_LANE_MAXM * q;
        patbytes = (size_t)SED_LANE_MAXM * nqueries;
    }
    const size_t o_pat = front, o_len = o_pat + patbytes, qbytes = patbytes + (rows ? 8 : 4) * (size_t)nqueries;
    if (!ix->pin.reserve(o_pat + qbytes, 1u << 16))
        return c->fail(SED_E_OOM, "pinned allocation failed (fit index, %zu bytes)", std::max<size_t>(o_pat + qbytes, 1u << 16));
    // the queries: their pattern records, then their lengths (then, long, the groups' query list)
    uint8_t *pats = (uint8_t *)ix->pin.p + o_pat;
    int32_t *plens = (int32_t *)((uint8_t *)ix->pin.p + o_len);
    for (int q = 0; q < nqueries; ++q) {
        if (off_p[q] < 0) return c->fail(SED_E_ARG, "query %d: negative offset", q);
        const int bad = fit_pack_pattern(pats + rec_at[q], codes_p + off_p[q], len_p[q], K, rows ? 64 * (*rows)[q] : SED_LANE_MAXM);
        if (bad >= 0) return c->fail(SED_E_ARG, "query %d: pattern code %d outside the alphabet (K=%d)", q, bad, K);
        plens[q] = len_p[q];
    }
    if (rows) memcpy(plens + nqueries, place_q.data(), sizeof(int32_t) * (size_t)nqueries);
    if (!ix->d_query.reserve(qbytes))
        return c->fail(SED_E_OOM, "device allocation failed (fit index, %d queries)", nqueries);
    sed_fit_index_args a{};
    a.chunks = (const sed_fit_chunk *)ix->d_chunks.p;
    a.nchunks = (int)ix->nchunks;
    a.texts = (const sed_fit_text *)ix->d_trec.p;
    a.ntexts = ntexts;
    a.pats = ix->d_query.p;
    a.plens = (const int32_t *)((const uint8_t *)ix->d_query.p + patbytes);
    if (rows) lg->d_qlist = a.plens + nqueries;
    a.nqueries = nqueries;
    a.text = ix->d_text.p;
    a.out = nullptr;
    a.chunk = plan.chunk;
    a.W = (int32_t)plan.W;
    if ((e = hipMemcpyAsync(ix->d_query.p, pats, qbytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return c->hipfail(e, "upload (fit index queries)");
    *args = a;
    return SED_OK;
}

// One R group's share of a long call's arguments
static sed_fit_index_args fit_long_group_args(const sed_fit_index_args &a, const FitLongGroups::Group &g) {
    sed_fit_index_args ga = a;
    ga.pats = (const uint8_t *)a.pats + g.at;
    ga.nqueries = g.count;
    return ga;
}

// What the kernels of one index call take besides the staged arguments: the plan's parameter words or the fp64 cost
// table, a search's per-lane records (fp64) and, for a hits call, the list, its counter and room, and the cutoff on the
// route's own scale.
struct FitIndexCall {
    FitKind kind;
    bool hits;
    const sed_fit_plan_t *plan;
    sed_fit_f64_costs fc;
    unsigned long long cap;
    int32_t cut;
    double max_dist;
};
static const char *const FIT_INDEX_LAUNCH_FAILS[2][4] = {  // [hits][kind]
    {"fit index kernel launch", "fit index long kernel launch", "fit index fp64 kernel launch",
     "fit index long fp64 kernel launch"},
    {"fit index hits kernel launch", "fit index long hits kernel launch", "fit index fp64 hits kernel launch",
     "fit index long fp64 hits kernel launch"}};
// The launches of an index call, best-hit or hits, on any route: the lane layouts' one launch, or the wave layouts' R
// groups (each group: its waves, then, best-hit, its reduce), the timer's events bracketing them.
static hipError_t fit_index_launch(sed_fit_index *ix, const FitIndexCall &k, FitTimer &timer, const sed_fit_index_args &a,
                                   const FitLongGroups &lg) {
    hipStream_t s = ix->ctx->stream;
    unsigned long long *count = (unsigned long long *)ix->d_count.p;
    sed_fit_f64_best *rec = (sed_fit_f64_best *)ix->d_rec.p, *best = (sed_fit_f64_best *)ix->d_out.p;
    sed_fit_f64_hit *hits64 = (sed_fit_f64_hit *)ix->d_hits.p;
    const sed_fit_params &fp = k.plan->fp;
    auto one = [&](hipEvent_t e0, hipEvent_t e1, const sed_fit_index_args &ga, const int32_t *qlist, int rows) {
        switch (k.kind) {
        case FIT_SHORT_KEYS:
            return k.hits ? sed_launch_fit_index_hits(s, e0, e1, ga, ix->d_hits.p, count, k.cap, k.cut, fp)
                          : sed_launch_fit_index(s, e0, e1, ga, fp);
        case FIT_F64:
            return k.hits ? sed_launch_fit_index_f64_hits(s, e0, e1, ga, hits64, count, k.cap, k.max_dist, k.fc)
                          : sed_launch_fit_index_f64(s, e0, e1, ga, rec, best, k.fc);
        case FIT_LONG_KEYS:
            return k.hits ? sed_launch_fit_index_long_hits(s, e0, e1, ga, qlist, rows, ix->d_hits.p, count, k.cap, k.cut, fp)
                          : sed_launch_fit_index_long(s, e0, e1, ga, qlist, rows, fp);
        default:
            return k.hits ? sed_launch_fit_index_long_f64_hits(s, e0, e1, ga, qlist, rows, hits64, count, k.cap, k.max_dist, k.fc)
                          : sed_launch_fit_index_long_f64(s, e0, e1, ga, qlist, rows, rec, best, k.fc);
        }
    };
    if (!sed_fit_route_of(k.kind).waves()) return one(timer.ev[0], timer.ev[1], a, nullptr, 0);
    hipError_t e = hipSuccess;
    for (size_t g = 0; g < lg.groups.size() && e == hipSuccess; ++g)
        e = one(g == 0 ? timer.ev[0] : nullptr, g + 1 == lg.groups.size() ? timer.ev[1] : nullptr,
                fit_long_group_args(a, lg.groups[g]), lg.d_qlist + lg.groups[g].first, lg.groups[g].rows);
    return e;
}

// The tail of a hits search over either record type: download the n records the kernels appended, sort them by
// (pair, end) - unique keys -, check each and decode it.  read(record, &start, &dist) = whether the record's own fields
// are those of a hit within the cutoff, and its start and distance.
template <class Rec, class Read>
static int fit_hits_decode(sed_fit_index *ix, std::vector<Rec> &recs, size_t n, int32_t nqueries, sed_fit_hit *out, Read read) {
    sed_ctx *c = ix->ctx;
    const uint32_t ntexts = (uint32_t)ix->sums.ntexts;
    recs.resize(n);
    hipError_t e = hipSuccess;
    if ((e = hipMemcpyAsync(recs.data(), ix->d_hits.p, n * sizeof(Rec), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return c->hipfail(e, "download (fit index hits)");
    std::sort(recs.begin(), recs.end(), [](const Rec &x, const Rec &y) { return x.pair != y.pair ? x.pair < y.pair : x.end < y.end; });
    for (size_t i = 0; i < n; ++i) {
        const Rec &r = recs[i];
        const uint32_t q = r.pair / ntexts, d = r.pair % ntexts;
        int32_t start = 0;
        double dist = 0;
        if (q >= (uint32_t)nqueries || r.end > (uint32_t)ix->len_t[d] || !read(r, &start, &dist) ||
            (i > 0 && recs[i - 1].pair == r.pair && recs[i - 1].end == r.end))
            return c->fail(SED_E_DEVICE, "fit hits: record %zu from the device is no hit (query %u, text %u, end %u)", i, q, d,
                           r.end);
        out[i] = sed_fit_hit{(int32_t)q, (int32_t)d, start, (int32_t)r.end, dist};
    }
    return SED_OK;
}

extern "C" {

sed_fit_index *sed_fit_index_create(sed_ctx *c, const uint8_t *codes_t, const int64_t *off_t, const int32_t *len_t,
                                    int32_t ntexts) {
    if (!c) return nullptr;
    if (ntexts < 0 || (ntexts > 0 && (!codes_t || !off_t || !len_t))) {
        c->fail(SED_E_ARG, "bad fit index arguments");
        return nullptr;
    }
    (void)hipSetDevice(c->device);
    size_t words = 0;
    for (int d = 0; d < ntexts; ++d) {
        if (len_t[d] < 0 || off_t[d] < 0) {
            c->fail(SED_E_ARG, "text %d: negative %s", d, len_t[d] < 0 ? "length" : "offset");
            return nullptr;
        }
        words += ((size_t)len_t[d] + 3) / 4;
        if (words > 0xFFFFFFF0u) {
            c->fail(SED_E_RANGE, "fit search: more than 16 GB of text");
            return nullptr;
        }
    }
    sed_fit_index *ix = new sed_fit_index;
    ix->ctx = c;
    ix->sums.ntexts = ntexts;
    ix->len_t.assign(len_t, len_t + ntexts);
    // every text 4-byte aligned, zero padded, and spare words at the end: a lane reads one word past its last
    std::vector<uint8_t> text(4 * words + 16, 0);
    std::vector<sed_fit_text> trec((size_t)ntexts);
    size_t at = 0;
    uint8_t top = 0;
    for (int d = 0; d < ntexts; ++d) {
        const int n = len_t[d];
        trec[d] = sed_fit_text{(uint32_t)(at / 4), n};
        const uint8_t *src = codes_t + off_t[d];
        for (int j = 0; j < n; ++j) top = std::max(top, text[at + j] = src[j]);
        if (n > 0) ix->maxcode = std::max<int>(ix->maxcode, top);
        at += ((size_t)n + 3) & ~(size_t)3;
        ix->symbols += n;
        ix->sums.cols += (double)n + 1;
        ix->sums.nmax = std::max<int64_t>(ix->sums.nmax, n);
    }
    hipError_t e = hipSuccess;
    if (!ix->d_text.reserve(text.size()) || !ix->d_trec.reserve(trec.size() * sizeof(sed_fit_text))) {
        c->fail(SED_E_OOM, "device allocation failed (fit index, %zu text bytes)", text.size());
    } else if ((e = hipMemcpyAsync(ix->d_text.p, text.data(), text.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
               (ntexts > 0 && (e = hipMemcpyAsync(ix->d_trec.p, trec.data(), trec.size() * sizeof(sed_fit_text),
                                                  hipMemcpyHostToDevice, c->stream)) != hipSuccess) ||
               (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->hipfail(e, "upload (fit index)");
    } else {
        return ix;
    }
    delete ix;
    return nullptr;
}

void sed_fit_index_destroy(sed_fit_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    delete ix;
}

int32_t sed_fit_index_texts(const sed_fit_index *ix) { return ix ? ix->sums.ntexts : SED_E_ARG; }
int64_t sed_fit_index_symbols(const sed_fit_index *ix) { return ix ? ix->symbols : SED_E_ARG; }

// sed_fit_index_search, sed_fit_index_search_long, sed_fit_index_search_f64 and sed_fit_index_search_long_f64: the plan,
// the launches and the result records differ with the route (sed_fit_plan.h: FitKind), nothing else
static int fit_index_search_of(sed_fit_index *ix, FitKind kind, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                               int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    const int ntexts = ix->sums.ntexts;
    int rc = fit_enter(c, nqueries == 0 || (nqueries > 0 && codes_p && off_p && len_p &&
                                            (ntexts == 0 || (out_dist && out_start && out_end))));
    if (rc != SED_OK) return rc;
    sed_fit_plan_t plan;
    std::vector<int32_t> rows;
    FitLongGroups lg;
    const bool lng = sed_fit_route_of(kind).waves(), f64 = sed_fit_route_of(kind).f64;
    rc = sed_fit_plan_index(kind, c->costs, c->opt, len_p, nqueries, ix->sums, &plan, &rows, &c->err);
    if (rc != SED_OK || nqueries == 0 || ntexts == 0) return rc;
    const size_t nres = (size_t)nqueries * (size_t)ntexts, resbytes = (f64 ? sizeof(sed_fit_f64_best) : 8) * nres;
    sed_fit_index_args a{};
    if ((rc = fit_index_stage(ix, plan, codes_p, off_p, len_p, nqueries, resbytes, &a, lng ? &rows : nullptr, &lg)) != SED_OK)
        return rc;
    if (!ix->d_out.reserve(resbytes) ||
        (f64 && !ix->d_rec.reserve((size_t)nqueries * (size_t)ix->nchunks * sizeof(sed_fit_f64_best))))
        return c->fail(SED_E_OOM, "device allocation failed (fit index, %zu results)", nres);
    hipError_t e = hipSuccess;
    if ((e = ix->timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    a.out = (unsigned long long *)ix->d_out.p;
    if ((e = hipMemsetAsync(ix->d_out.p, 0xFF, resbytes, c->stream)) != hipSuccess)
        return c->hipfail(e, "upload (fit index search)");
    sed_fit_f64_costs fc{};
    if (f64 && (e = fit_f64_costs_upload(c, plan, ix->d_tab, &fc)) != hipSuccess) return c->hipfail(e, "upload (fit index costs)");
    if ((e = fit_index_launch(ix, FitIndexCall{kind, false, &plan, fc, 0, 0, 0.0}, ix->timer, a, lg)) != hipSuccess)
        return c->hipfail(e, FIT_INDEX_LAUNCH_FAILS[0][kind]);
    const uint64_t *keys = (const uint64_t *)ix->pin.p;
    if ((e = hipMemcpyAsync(ix->pin.p, ix->d_out.p, resbytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "download (fit index search)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "fit index kernel execution");
    ix->timer.timed = true;
    const double inv = std::ldexp(1.0, -plan.scale_log2);
    size_t r = 0;
    for (int q = 0; q < nqueries; ++q)
        for (int d = 0; d < ntexts; ++d, ++r)
            if (f64 ? !fit_decode_f64(((const sed_fit_f64_best *)ix->pin.p)[r], ix->len_t[d], &out_dist[r], &out_start[r], &out_end[r])
                    : !fit_decode_key(keys[r], ix->len_t[d], inv, &out_dist[r], &out_start[r], &out_end[r]))
                return c->fail(SED_E_DEVICE, "query %d, text %d: no fit result from the device", q, d);
    return SED_OK;
}

int sed_fit_index_search(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                         int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end) {
    return fit_index_search_of(ix, FIT_SHORT_KEYS, codes_p, off_p, len_p, nqueries, out_dist, out_start, out_end);
}
int sed_fit_index_search_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                             int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end) {
    return fit_index_search_of(ix, FIT_F64, codes_p, off_p, len_p, nqueries, out_dist, out_start, out_end);
}
int sed_fit_index_search_long(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                              int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end) {
    return fit_index_search_of(ix, FIT_LONG_KEYS, codes_p, off_p, len_p, nqueries, out_dist, out_start, out_end);
}

int sed_fit_index_search_long_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                                  int32_t nqueries, double *out_dist, int32_t *out_start, int32_t *out_end) {
    return fit_index_search_of(ix, FIT_LONG_F64, codes_p, off_p, len_p, nqueries, out_dist, out_start, out_end);
}

int sed_fit_index_last_time(const sed_fit_index *ix, float *kernel_ms) {
    return ix && kernel_ms ? ix->timer.elapsed(kernel_ms) : SED_E_ARG;
}

// Every hit within max_dist (include/sed.h).  The search's plan, chunk table and queries (fit_index_stage); the kernel
// appends its records in whatever order the waves' atomic adds land, and counts on past `cap`.  The host reads the
// count, then the records when they all fit (fit_hits_decode).
static int fit_index_hits_of(sed_fit_index *ix, FitKind kind, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                             int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    const int ntexts = ix->sums.ntexts;
    int rc = fit_enter(c, (nqueries == 0 || (nqueries > 0 && codes_p && off_p && len_p)) && cap >= 0 && (cap == 0 || out) && found);
    if (rc != SED_OK) return rc;
    sed_fit_plan_t plan;
    std::vector<int32_t> rows;
    FitLongGroups lg;
    const bool lng = sed_fit_route_of(kind).waves(), f64 = sed_fit_route_of(kind).f64;
    rc = sed_fit_plan_index(kind, c->costs, c->opt, len_p, nqueries, ix->sums, &plan, &rows, &c->err);
    int32_t cut = 0;
    if (rc == SED_OK) rc = sed_fit_cutoff_rule(plan, max_dist, &cut, &c->err);  // (fp64: its check of max_dist alone)
    if (rc != SED_OK) return rc;
    *found = 0;
    if (nqueries == 0 || ntexts == 0) return SED_OK;
    sed_fit_index_args a{};
    if ((rc = fit_index_stage(ix, plan, codes_p, off_p, len_p, nqueries, 8, &a, lng ? &rows : nullptr, &lg)) != SED_OK) return rc;
    const size_t recbytes = f64 ? sizeof(sed_fit_f64_hit) : sizeof(sed_fit_hit_rec);
    if ((uint64_t)cap > SIZE_MAX / recbytes || !ix->d_count.reserve(8) ||
        !ix->d_hits.reserve(std::max<size_t>((size_t)cap * recbytes, recbytes)))
        return c->fail(SED_E_OOM, "device allocation failed (fit index, room for %lld hits)", (long long)cap);
    hipError_t e = hipSuccess;
    if ((e = ix->hits_timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    if ((e = hipMemsetAsync(ix->d_count.p, 0, 8, c->stream)) != hipSuccess) return c->hipfail(e, "upload (fit index hits)");
    sed_fit_f64_costs fc{};
    if (f64 && (e = fit_f64_costs_upload(c, plan, ix->d_tab, &fc)) != hipSuccess) return c->hipfail(e, "upload (fit index costs)");
    const FitIndexCall call{kind, true, &plan, fc, (unsigned long long)cap, cut, max_dist};
    if ((e = fit_index_launch(ix, call, ix->hits_timer, a, lg)) != hipSuccess) return c->hipfail(e, FIT_INDEX_LAUNCH_FAILS[1][kind]);
    if ((e = hipMemcpyAsync(ix->pin.p, ix->d_count.p, 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "download (fit index hits)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "fit index hits kernel execution");
    ix->hits_timer.timed = true;
    const uint64_t n = *(const uint64_t *)ix->pin.p;
    *found = (int64_t)n;
    if (n > (uint64_t)cap)
        return c->fail(SED_E_RANGE, "fit hits: found %lld hits, cap %lld: call again with room for them", (long long)n,
                       (long long)cap);
    if (n == 0) return SED_OK;
    if (f64)
        return fit_hits_decode(ix, ix->h_hits64, (size_t)n, nqueries, out, [&](const sed_fit_f64_hit &r, int32_t *start, double *dist) {
            *start = r.start;
            *dist = r.D;
            return r.start >= 0 && (uint32_t)r.start <= r.end && r.D >= 0 && r.D <= max_dist;
        });
    const double inv = std::ldexp(1.0, -plan.scale_log2);
    return fit_hits_decode(ix, ix->h_hits, (size_t)n, nqueries, out, [&](const sed_fit_hit_rec &r, int32_t *start, double *dist) {
        *start = (int32_t)(r.end - r.len);
        *dist = (double)r.D * inv;
        return r.len <= r.end && r.D <= (uint32_t)cut;
    });
}

int sed_fit_index_hits(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                       int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found) {
    return fit_index_hits_of(ix, FIT_SHORT_KEYS, codes_p, off_p, len_p, nqueries, max_dist, out, cap, found);
}
int sed_fit_index_hits_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                           int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found) {
    return fit_index_hits_of(ix, FIT_F64, codes_p, off_p, len_p, nqueries, max_dist, out, cap, found);
}
int sed_fit_index_hits_long(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                            int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found) {
    return fit_index_hits_of(ix, FIT_LONG_KEYS, codes_p, off_p, len_p, nqueries, max_dist, out, cap, found);
}

int sed_fit_index_hits_long_f64(sed_fit_index *ix, const uint8_t *codes_p, const int64_t *off_p, const int32_t *len_p,
                                int32_t nqueries, double max_dist, sed_fit_hit *out, int64_t cap, int64_t *found) {
    return fit_index_hits_of(ix, FIT_LONG_F64, codes_p, off_p, len_p, nqueries, max_dist, out, cap, found);
}

int sed_fit_index_hits_last_time(const sed_fit_index *ix, float *kernel_ms) {
    return ix && kernel_ms ? ix->hits_timer.elapsed(kernel_ms) : SED_E_ARG;
}

}  // extern "C"
