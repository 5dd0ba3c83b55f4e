// sed_join_runtime.cpp — the similarity join's entry points of the C-ABI (include/sed.h): sed_join_index_*,
// sed_join_self / sed_join_search, their _f64 siblings and the k-nearest forms of both (sed_join_knn_*) over a resident
// index of short sequences, and sed_join_long_* over one of sequences of up to 128 symbols.  What a join runs is the
// join planner's decision and what its records mean is the planner's decode (sed_join_plan.cpp); the kernels are
// sed_join.hip, sed_join_f64.hip and sed_join_long.hip.  Here: pack, reserve, upload, launch, download, on the context's
// stream (sed_runtime.h).  A call is three values - the index type (one number, the record's length), the numeric route
// (JoinRoute) and the form (k = 0: a join, else the k nearest) - and one loop, join_run, runs every combination.
#include "sed_join_plan.h"
#include "sed_runtime.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {
struct JoinTimer {  // the events around a call's launches, created on first use ([2]: a k-nearest call's first bound pass ends)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = false;
    bool knn = false;  // the timed call was a k-nearest one: ev[2] was recorded
    ~JoinTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t begin() {
        hipError_t e = hipSuccess;
        for (hipEvent_t &x : ev)
            if (!x && (e = hipEventCreate(&x)) != hipSuccess) return e;
        timed = false;
        return hipSuccess;
    }
};
const size_t REC_BYTES = sizeof(sed_join_rec);  // one record of the device hit list (sed_internal.h: sed_join_list)
static_assert(REC_BYTES == sizeof(uint4), "a record of the device list");
const size_t SPARE = 16;  // the spare bytes that end a record buffer (the kernels' row loads reach two words past a record)

const size_t F64_TAB = SED_JOIN_F64_MAXK * SED_JOIN_F64_MAXK;  // the fp64 table's doubles
const size_t F64_LOW = (SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1);  // its k-nearest calls' lower-bound table's

uint32_t code_bit(uint8_t c) { return 1u << (c < 31 ? c : 31); }

struct JoinRoute;
}  // namespace

struct sed_join_index {
    sed_ctx *ctx = nullptr;
    int32_t maxlen = SED_JOIN_MAXLEN;  // the longest sequence = the bytes of a record: SED_JOIN_MAXLEN or SED_JOIN_LONG_MAXLEN
    int32_t nseqs = 0;
    uint32_t codes = 0;            // bit c: code c occurs (bit 31: any code >= 31)
    std::vector<int32_t> len;      // in the caller's order: the rows of a self join
    std::vector<int32_t> col_len;  // sorted by length: the columns
    // the records in the caller's order and their lengths (rows of a self join); the records sorted by length (stable),
    // their lengths and original indices (columns of every join); a search's query records and lengths
    DevBuf d_rows, d_row_len, d_cols, d_col_len, d_col_orig, d_query;
    DevBuf d_hits, d_count;
    DevBuf d_block;                // the route's upload block (JoinRoute::fill) and its source
    uint64_t h_block[F64_TAB + F64_LOW] = {};
    DevBuf d_bound;                // the k-nearest calls' bound of every row, indexed as the rows are, JoinRoute::bound_bytes each
    std::vector<uint64_t> h_bound; // the last k-nearest call's bounds after pass 1, packed as on the device: bound_rows of
    int32_t bound_rows = 0;        // knn_route->bound_bytes each (a call that ran nothing: the bound every row starts from)
    const JoinRoute *knn_route = nullptr;  // the route of the last k-nearest call that got past its plan
    std::vector<sed_join_hit> h_knn;  // its candidates, decoded and trimmed
    int64_t knn_candidates = -1;   // the hits its emit pass appended; -1 before the first k-nearest call
    std::vector<uint8_t> h_query;
    std::vector<sed_join_rec> h_hits;
    PinBuf pin;                    // the two counters' download
    JoinTimer timer;
    int64_t pairs_run = -1;
    ~sed_join_index() {
        pin.release();
        d_rows.release(); d_row_len.release(); d_cols.release(); d_col_len.release(); d_col_orig.release();
        d_query.release(); d_block.release(); d_hits.release(); d_count.release(); d_bound.release();
    }
};

struct sed_join_long_index : sed_join_index {};  // (a type of its own in the C-ABI: its records are 128 bytes)

namespace {
// What a call runs: its route, that route's plan, and the form
struct JoinCall {
    const JoinRoute *route = nullptr;
    sed_join_plan_t pi;      // route->id == SED_JOIN_ROUTE_INT
    sed_join_f64_plan_t pf;  // route->id == SED_JOIN_ROUTE_F64
    const sed_join_counts *counts = nullptr;  // what both plans share, of the one that is filled
    int32_t knn = 0;         // k of a k-nearest call, 0: a join
    int maxlen = SED_JOIN_MAXLEN;  // the index type
};

// The launch arguments of either route in their k-nearest form; a join launches the .j of its route's
union JoinArgs {
    sed_join_knn_args i;
    sed_join_knn_f64_args f;
};

// Everything join_run does that depends on the numeric route.  A new route is a new row of this table.
struct JoinRoute {
    int id;                 // SED_JOIN_ROUTE_*
    size_t bound_bytes;     // a row's bound on the device (the kernels read it at this width)
    size_t block_bytes[2];  // the upload block of a join [0] and of a k-nearest call [1]
    // the route's plan of the call into k, the refusal's text in the context
    int (*plan)(sed_ctx *c, const sed_join_index *ix, const int32_t *len_rows, int32_t nrows, bool self, uint32_t row_codes,
                double max_dist, JoinCall *k);
    // the upload block's content (h_block) and the arguments but for the sides, from the plan
    void (*fill)(const JoinCall &k, uint64_t *h_block, const void *d_block, void *d_bound, const sed_join_list &list, JoinArgs *a);
    // one launch over the rows of s: a join's one pass, or a k-nearest call's bound (emit = false) or emit pass
    hipError_t (*launch)(const JoinCall &k, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, JoinArgs *a, const sed_join_sides &s,
                         bool emit);
    uint64_t (*bound0)(const JoinCall &k);  // the bound every row starts from, as a 64-bit fill word
    void (*decode)(const JoinCall &k, sed_join_decode_call *d);  // how a record's trailing words become a distance
};

// ---- the integer route: the block is the 64 bytes of cost rows; a bound is D on the scale, 4 bytes ----
int int_plan(sed_ctx *c, const sed_join_index *ix, const int32_t *len_rows, int32_t nrows, bool self, uint32_t row_codes,
             double max_dist, JoinCall *k) {
    k->counts = &k->pi;
    return sed_join_plan_of(c->costs, c->opt, len_rows, nrows, ix->len.data(), ix->nseqs, self, row_codes, ix->codes, max_dist,
                            ix->maxlen, &k->pi, &c->err);
}
void int_fill(const JoinCall &k, uint64_t *h_block, const void *d_block, void *d_bound, const sed_join_list &list, JoinArgs *a) {
    const sed_join_plan_t &p = k.pi;
    static_assert(sizeof p.sp.row == 64, "the upload's layout");
    memcpy(h_block, p.sp.row, sizeof p.sp.row);
    sed_join_args &j = a->i.j;
    j.tab = (const uint2 *)d_block;
    j.ins = p.sp.ins;
    j.del = p.sp.del;
    j.umap = p.sp.umap;
    j.shift = p.scale_log2;
    j.cut = p.cut;
    j.out = list;
    a->i.bound = (uint32_t *)d_bound;
    a->i.k = k.knn;
}
hipError_t int_launch(const JoinCall &k, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, JoinArgs *a, const sed_join_sides &s,
                      bool emit) {
    a->i.j.s = s;
    const bool bitpar = k.pi.kernel == SED_JOIN_KERNEL_BITPAR, lng = k.maxlen == SED_JOIN_LONG_MAXLEN;
    if (!k.knn) return lng ? sed_launch_join_long(stream, ev0, ev1, a->i.j, bitpar) : sed_launch_join(stream, ev0, ev1, a->i.j, bitpar);
    return lng ? sed_launch_join_long_knn(stream, ev0, ev1, a->i, bitpar, emit)
               : sed_launch_join_knn(stream, ev0, ev1, a->i, bitpar, emit);
}
uint64_t int_bound0(const JoinCall &k) { return (uint64_t)(uint32_t)k.pi.cut * 0x100000001ull; }
void int_decode(const JoinCall &k, sed_join_decode_call *d) {
    d->scale_log2 = k.pi.scale_log2;
    d->cap = k.pi.cut;
}

// ---- the fp64 route: the block is [sub | keep] for a join, [sub | low] for a k-nearest call; a bound is a double's bits ----
int f64_plan(sed_ctx *c, const sed_join_index *ix, const int32_t *len_rows, int32_t nrows, bool self, uint32_t row_codes,
             double max_dist, JoinCall *k) {
    k->counts = &k->pf;
    return sed_join_f64_plan_of(c->costs, c->opt, len_rows, nrows, ix->len.data(), ix->nseqs, self, row_codes, ix->codes, max_dist,
                                &k->pf, &c->err);
}
void f64_fill(const JoinCall &k, uint64_t *h_block, const void *d_block, void *d_bound, const sed_join_list &list, JoinArgs *a) {
    const sed_join_f64_plan_t &p = k.pf;
    static_assert(sizeof p.sub == F64_TAB * 8 && sizeof p.low == F64_LOW * 8 && sizeof p.keep <= sizeof p.low, "the upload's layout");
    memcpy(h_block, p.sub, sizeof p.sub);
    sed_join_f64_args &j = a->f.j;
    j.sub = (const double *)d_block;
    if (k.knn) {
        memcpy(h_block + F64_TAB, p.low, sizeof p.low);
        a->f.low = (const double *)d_block + F64_TAB;
    } else {
        memcpy(h_block + F64_TAB, p.keep, sizeof p.keep);
        j.keep = (const unsigned long long *)d_block + F64_TAB;
    }
    j.ins = p.ins;
    j.del = p.del;
    j.max_dist = p.max_dist;
    j.out = list;
    a->f.bound = (unsigned long long *)d_bound;
    a->f.k = k.knn;
}
hipError_t f64_launch(const JoinCall &k, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, JoinArgs *a, const sed_join_sides &s,
                      bool emit) {
    a->f.j.s = s;
    return k.knn ? sed_launch_join_knn_f64(stream, ev0, ev1, a->f, emit) : sed_launch_join_f64(stream, ev0, ev1, a->f.j);
}
uint64_t f64_bound0(const JoinCall &k) {
    uint64_t b;
    memcpy(&b, &k.pf.max_dist, sizeof b);
    return b;
}
void f64_decode(const JoinCall &k, sed_join_decode_call *d) { d->cap = k.pf.max_dist; }

const JoinRoute ROUTE_INT = {SED_JOIN_ROUTE_INT, sizeof(uint32_t), {64, 64}, int_plan, int_fill, int_launch, int_bound0, int_decode};
const JoinRoute ROUTE_F64 = {SED_JOIN_ROUTE_F64, sizeof(uint64_t), {8 * (F64_TAB + SED_JOIN_MAXLEN + 1), 8 * (F64_TAB + F64_LOW)},
                             f64_plan, f64_fill, f64_launch, f64_bound0, f64_decode};

// What a HIP failure's text calls the steps of either form
struct JoinSteps {
    const char *upload, *launch, *download, *execution, *records;
};
const JoinSteps STEPS[2] = {
    {"upload (join)", "join kernel launch", "download (join)", "join kernel execution", "download (join hits)"},
    {"upload (k-nearest join)", "k-nearest join kernel launch", "download (k-nearest join)", "k-nearest join kernel execution",
     "download (k-nearest candidates)"}};
}  // namespace

// What every call runs once its rows are on the device.  s holds the rows (rows, row_len, row0, self); nrows rows from
// s.row0 on.  A k-nearest call (k.knn = k): every row's bound starts at the route's cap; per row step, the bound pass
// then the emit pass (the candidates within bound[r]) on the one stream; the counters and the bounds come down.  Its
// device list is sized for the candidates: when the emit pass overflows it, it grows to the count the device reports and
// the emit pass alone runs once more (the bounds are final), which the pairs counted leave out and the time spans.  A
// join is the same with the emit pass alone, the cap as every row's bound, the list the caller's cap long and no second
// attempt: an overflow goes back as SED_E_RANGE before any record is downloaded.
static int join_run(sed_join_index *ix, const JoinCall &k, sed_join_sides s, int32_t nrows, sed_join_hit *out, int64_t cap,
                    int64_t *found) {
    sed_ctx *c = ix->ctx;
    const JoinRoute &rt = *k.route;
    const bool knn = k.knn != 0;
    const JoinSteps &step_of = STEPS[knn];
    const int32_t first = s.row0;
    const size_t block = rt.block_bytes[knn], bbytes = knn ? (size_t)nrows * rt.bound_bytes : 0;
    // the list's records: twice a k-nearest call's answer and a little; a join's: what the caller has room for
    const size_t room = knn ? 2 * (size_t)nrows * (size_t)k.knn + 1024 : std::max<size_t>((size_t)cap, 1);
    if ((!knn && (uint64_t)cap > SIZE_MAX / REC_BYTES) || !ix->d_count.reserve(16) || !ix->d_block.reserve(block) ||
        !ix->d_bound.reserve(knn ? ((size_t)first + (size_t)nrows) * rt.bound_bytes : 0) || !ix->d_hits.reserve(room * REC_BYTES) ||
        !ix->pin.reserve(16, 64))
        return knn ? c->fail(SED_E_OOM, "device allocation failed (k-nearest join, %d rows)", nrows)
                   : c->fail(SED_E_OOM, "device allocation failed (join, room for %lld hits)", (long long)cap);
    hipError_t e = hipSuccess;
    if ((e = ix->timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    s.cols = ix->d_cols.p;  // the columns' side of every launch
    s.col_len = (const int32_t *)ix->d_col_len.p;
    s.col_orig = (const int32_t *)ix->d_col_orig.p;
    s.ncols = ix->nseqs;
    JoinArgs a;
    memset(&a, 0, sizeof a);
    void *const d_first = (uint8_t *)ix->d_bound.p + (size_t)first * rt.bound_bytes;
    const int64_t step = k.counts->launch_rows;
    if (knn) ix->knn_candidates = -1;  // (a call that fails from here on leaves nothing to report)
    uint64_t n = 0;
    for (int attempt = 0;; ++attempt) {  // (attempt 1, k-nearest alone: the emit pass again with room for what attempt 0 counted)
        const sed_join_list list{(uint4 *)ix->d_hits.p, (unsigned long long *)ix->d_count.p,
                                 knn ? (unsigned long long)(ix->d_hits.cap / REC_BYTES) : (unsigned long long)cap};
        const int pass0 = knn && attempt == 0 ? 0 : 1;  // this attempt's passes: pass0 .. 1 (0: the bounds, 1: emit)
        rt.fill(k, ix->h_block, ix->d_block.p, ix->d_bound.p, list, &a);
        if ((e = hipMemsetAsync(ix->d_count.p, 0, 16, c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(ix->d_block.p, ix->h_block, block, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
            (pass0 == 0 && (e = hipMemcpyAsync(d_first, ix->h_bound.data(), bbytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess))
            return c->hipfail(e, step_of.upload);  // (h_bound: every row's starting bound, join_knn_planned)
        for (int64_t r = 0; r < nrows; r += step) {  // the events bracket the launches
            s.row0 = first + (int32_t)r;
            s.nrows = (int32_t)std::min<int64_t>(step, nrows - r);
            const bool head = attempt == 0 && r == 0, tail = r + step >= nrows;
            for (int pass = pass0; pass < 2; ++pass) {
                hipEvent_t e0 = head && pass == pass0 ? ix->timer.ev[0] : nullptr;
                hipEvent_t e1 = pass ? (tail ? ix->timer.ev[1] : nullptr) : (head ? ix->timer.ev[2] : nullptr);
                if ((e = rt.launch(k, c->stream, e0, e1, &a, s, pass != 0)) != hipSuccess) return c->hipfail(e, step_of.launch);
            }
        }
        if ((e = hipMemcpyAsync(ix->pin.p, ix->d_count.p, 16, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (pass0 == 0 && (e = hipMemcpyAsync(ix->h_bound.data(), d_first, bbytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess))
            return c->hipfail(e, step_of.download);
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, step_of.execution);
        ix->timer.timed = true;
        ix->timer.knn = knn;
        n = ((const uint64_t *)ix->pin.p)[0];
        if (attempt == 0) ix->pairs_run = (int64_t)((const uint64_t *)ix->pin.p)[1];
        if (n <= list.cap) break;
        if (!knn) {
            *found = (int64_t)n;
            return c->fail(SED_E_RANGE, "join: found %lld hits, cap %lld: call again with room for them", (long long)n, (long long)cap);
        }
        if (attempt == 1) return c->fail(SED_E_DEVICE, "k-nearest join: %llu candidates after room was made for them", (unsigned long long)n);
        if (n > SIZE_MAX / REC_BYTES || !ix->d_hits.reserve((size_t)n * REC_BYTES))
            return c->fail(SED_E_OOM, "device allocation failed (k-nearest join, room for %llu candidates)", (unsigned long long)n);
    }
    if (knn)
        ix->knn_candidates = (int64_t)n;
    else
        *found = (int64_t)n;
    if (n == 0) return SED_OK;
    ix->h_hits.resize((size_t)n);
    if ((e = hipMemcpyAsync(ix->h_hits.data(), ix->d_hits.p, (size_t)n * REC_BYTES, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return c->hipfail(e, step_of.records);
    sed_join_hit *hits = out;  // a join's n hits fit the caller's room; a k-nearest call's candidates are trimmed first
    if (knn) {
        ix->h_knn.resize((size_t)n);
        hits = ix->h_knn.data();
    }
    sed_join_decode_call d{rt.id, 0, 0.0, first, nrows, ix->nseqs, s.self != 0, k.knn, ix->h_bound.data()};
    rt.decode(k, &d);
    int64_t kept = 0;
    const int rc = sed_join_decode_of(d, ix->h_hits.data(), (int64_t)n, hits, &kept, &c->err);
    if (rc != SED_OK) return rc;
    *found = kept;
    if (kept > cap)
        return c->fail(SED_E_RANGE, "join: found %lld hits, cap %lld: call again with room for them", (long long)kept, (long long)cap);
    if (knn && kept) memcpy(out, hits, (size_t)kept * sizeof(sed_join_hit));
    return SED_OK;
}

// What every join refuses first, in sed_fit_index_search's order
// (knn: NULL for a join, else k of the k-nearest call, checked with the arguments by the planner's rule)
static int join_enter(sed_ctx *c, bool args_ok, const int32_t *knn) {
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (knn && sed_join_knn_k_rule(*knn, &c->err) != SED_OK) return SED_E_ARG;
    if (!args_ok) return c->fail(SED_E_ARG, "bad join arguments");
    if (!c->have_costs) return c->fail(SED_E_STATE, "sed_set_costs() was not called");
    (void)hipSetDevice(c->device);
    return SED_OK;
}

// sed_join_index_create and sed_join_long_index_create: Index = the type made, of sequences of up to maxlen symbols
template <class Index>
static Index *join_index_create(sed_ctx *c, int32_t maxlen, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                int32_t nseqs) {
    if (!c) return nullptr;
    const size_t REC = (size_t)maxlen;
    if (nseqs < 0 || (nseqs > 0 && (!codes || !off || !len))) {
        c->fail(SED_E_ARG, "bad join index arguments");
        return nullptr;
    }
    for (int i = 0; i < nseqs; ++i)
        if (len[i] < 0 || len[i] > maxlen || off[i] < 0) {
            if (off[i] < 0 || len[i] < 0)
                c->fail(SED_E_ARG, "join index: sequence %d: negative %s", i, len[i] < 0 ? "length" : "offset");
            else
                c->fail(SED_E_ARG, "join index: sequence %d has %d symbols (at most %d)", i, len[i], maxlen);
            return nullptr;
        }
    (void)hipSetDevice(c->device);
    Index *ix = new Index;
    ix->ctx = c;
    ix->maxlen = maxlen;
    ix->nseqs = nseqs;
    ix->len.assign(len, len + nseqs);
    std::vector<int32_t> order((size_t)nseqs);
    for (int i = 0; i < nseqs; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return len[x] < len[y]; });
    std::vector<uint8_t> rows(REC * (size_t)nseqs + SPARE, 0), cols(REC * (size_t)nseqs + SPARE, 0);
    ix->col_len.resize((size_t)nseqs);
    for (int i = 0; i < nseqs; ++i) {
        for (int j = 0; j < len[i]; ++j) ix->codes |= code_bit(rows[REC * (size_t)i + j] = codes[off[i] + j]);
    }
    for (int t = 0; t < nseqs; ++t) {
        memcpy(&cols[REC * (size_t)t], &rows[REC * (size_t)order[t]], REC);
        ix->col_len[t] = len[order[t]];
    }
    const size_t ibytes = sizeof(int32_t) * (size_t)nseqs;
    hipError_t e = hipSuccess;
    if (!ix->d_rows.reserve(rows.size()) || !ix->d_cols.reserve(cols.size()) || !ix->d_row_len.reserve(ibytes) ||
        !ix->d_col_len.reserve(ibytes) || !ix->d_col_orig.reserve(ibytes)) {
        c->fail(SED_E_OOM, "device allocation failed (join index, %d sequences)", nseqs);
    } else if ((e = hipMemcpyAsync(ix->d_rows.p, rows.data(), rows.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
               (e = hipMemcpyAsync(ix->d_cols.p, cols.data(), cols.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
               (nseqs > 0 &&
                ((e = hipMemcpyAsync(ix->d_row_len.p, ix->len.data(), ibytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
                 (e = hipMemcpyAsync(ix->d_col_len.p, ix->col_len.data(), ibytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
                 (e = hipMemcpyAsync(ix->d_col_orig.p, order.data(), ibytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)) ||
               (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->hipfail(e, "upload (join index)");
    } else {
        return ix;
    }
    delete ix;
    return nullptr;
}

template <class Index>
static void join_index_destroy(Index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    delete ix;
}

extern "C" {

sed_join_index *sed_join_index_create(sed_ctx *c, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                      int32_t nseqs) {
    return join_index_create<sed_join_index>(c, SED_JOIN_MAXLEN, codes, off, len, nseqs);
}

sed_join_long_index *sed_join_long_index_create(sed_ctx *c, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                                int32_t nseqs) {
    return join_index_create<sed_join_long_index>(c, SED_JOIN_LONG_MAXLEN, codes, off, len, nseqs);
}

void sed_join_index_destroy(sed_join_index *ix) { join_index_destroy(ix); }

void sed_join_long_index_destroy(sed_join_long_index *ix) { join_index_destroy(ix); }

int32_t sed_join_index_seqs(const sed_join_index *ix) { return ix ? ix->nseqs : SED_E_ARG; }

int32_t sed_join_long_index_seqs(const sed_join_long_index *ix) { return ix ? ix->nseqs : SED_E_ARG; }

}  // extern "C"

// A call got past its plan: nothing found, nothing run yet; and what sed_join_knn_bounds and sed_join_knn_candidates
// report of a k-nearest call until it has run: every row's bound where it starts, no candidate
static void join_planned(sed_join_index *ix, const JoinCall &k, int32_t nrows, int64_t *found) {
    *found = 0;
    ix->pairs_run = 0;
    if (!k.knn) return;
    ix->knn_route = k.route;
    ix->bound_rows = nrows;
    ix->h_bound.assign(((size_t)nrows * k.route->bound_bytes + 7) / 8, k.route->bound0(k));
    ix->knn_candidates = 0;
}

// (knn: NULL for a join, else k of the k-nearest call)
static int join_self(sed_join_index *ix, const JoinRoute &rt, const int32_t *knn, int32_t row_lo, int32_t row_hi, double max_dist,
                     sed_join_hit *out, int64_t cap, int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    int rc = join_enter(c, 0 <= row_lo && row_lo <= row_hi && row_hi <= ix->nseqs && cap >= 0 && (cap == 0 || out) && found,
                        knn);
    if (rc != SED_OK) return rc;
    JoinCall k;
    k.route = &rt;
    k.knn = knn ? *knn : 0;
    k.maxlen = ix->maxlen;
    const int32_t nrows = row_hi - row_lo;
    rc = rt.plan(c, ix, ix->len.data() + row_lo, nrows, true, ix->codes, max_dist, &k);
    if (rc != SED_OK) return rc;
    join_planned(ix, k, nrows, found);
    if (nrows == 0) return SED_OK;
    sed_join_sides s{};
    s.rows = ix->d_rows.p;
    s.row_len = (const int32_t *)ix->d_row_len.p;
    s.row0 = row_lo;
    s.self = 1;
    return join_run(ix, k, s, nrows, out, cap, found);
}

static int join_search(sed_join_index *ix, const JoinRoute &rt, const int32_t *knn, const uint8_t *codes_q, const int64_t *off_q,
                       const int32_t *len_q, int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap,
                       int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    int rc = join_enter(c, (nqueries == 0 || (nqueries > 0 && codes_q && off_q && len_q)) && cap >= 0 && (cap == 0 || out) &&
                               found, knn);
    if (rc != SED_OK) return rc;
    // the queries' records and lengths, one block: [records | spare | lengths]
    const size_t REC = (size_t)ix->maxlen;
    const size_t o_len = REC * (size_t)nqueries + SPARE, qbytes = o_len + sizeof(int32_t) * (size_t)nqueries;
    ix->h_query.assign(qbytes, 0);
    uint32_t qcodes = 0;
    for (int q = 0; q < nqueries; ++q) {
        if (off_q[q] < 0) return c->fail(SED_E_ARG, "query %d: negative offset", q);
        if (len_q[q] < 0 || len_q[q] > ix->maxlen)
            return c->fail(SED_E_ARG, "query %d has %d symbols (0..%d)", q, len_q[q], ix->maxlen);
        for (int j = 0; j < len_q[q]; ++j) qcodes |= code_bit(ix->h_query[REC * (size_t)q + j] = codes_q[off_q[q] + j]);
    }
    if (nqueries) memcpy(&ix->h_query[o_len], len_q, sizeof(int32_t) * (size_t)nqueries);
    JoinCall k;
    k.route = &rt;
    k.knn = knn ? *knn : 0;
    k.maxlen = ix->maxlen;
    rc = rt.plan(c, ix, len_q, nqueries, false, qcodes, max_dist, &k);
    if (rc != SED_OK) return rc;
    join_planned(ix, k, nqueries, found);
    if (nqueries == 0 || ix->nseqs == 0) return SED_OK;
    if (!ix->d_query.reserve(qbytes)) return c->fail(SED_E_OOM, "device allocation failed (join, %d queries)", nqueries);
    hipError_t e = hipMemcpyAsync(ix->d_query.p, ix->h_query.data(), qbytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->hipfail(e, "upload (join queries)");
    sed_join_sides s{};
    s.rows = ix->d_query.p;
    s.row_len = (const int32_t *)((const uint8_t *)ix->d_query.p + o_len);
    s.row0 = 0;
    s.self = 0;
    return join_run(ix, k, s, nqueries, out, cap, found);
}

// sed_join_knn_bounds and its siblings: the last k-nearest call's bounds, when that call took route rt
static int join_knn_bounds(const sed_join_index *ix, const JoinRoute &rt, void *bounds, int32_t n) {
    if (!ix || n < 0 || (n && !bounds)) return SED_E_ARG;
    if (ix->knn_candidates < 0 || ix->knn_route != &rt) return SED_E_STATE;
    if (n != ix->bound_rows) return SED_E_ARG;
    if (n) memcpy(bounds, ix->h_bound.data(), (size_t)n * rt.bound_bytes);
    return SED_OK;
}

extern "C" {

int sed_join_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                  int64_t *found) {
    return join_self(ix, ROUTE_INT, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                      int64_t *found) {
    return join_self(ix, ROUTE_F64, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                    int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_INT, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_F64, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_last_time(const sed_join_index *ix, float *kernel_ms) {
    if (!ix || !kernel_ms) return SED_E_ARG;
    if (!ix->timer.timed) return SED_E_STATE;
    return hipEventElapsedTime(kernel_ms, ix->timer.ev[0], ix->timer.ev[1]) == hipSuccess ? SED_OK : SED_E_DEVICE;
}

int sed_join_pairs_run(const sed_join_index *ix, int64_t *pairs) {
    if (!ix || !pairs) return SED_E_ARG;
    if (ix->pairs_run < 0) return SED_E_STATE;
    *pairs = ix->pairs_run;
    return SED_OK;
}

int32_t sed_join_rows_per_group(void) { return SED_JOIN_G; }

// ---- the k nearest columns of every row (the integer route of either index type) ----
int sed_join_knn_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist, sed_join_hit *out,
                      int64_t cap, int64_t *found) {
    return join_self(ix, ROUTE_INT, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_knn_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_INT, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_knn_bounds(const sed_join_index *ix, int32_t *bounds, int32_t n) { return join_knn_bounds(ix, ROUTE_INT, bounds, n); }

// ---- the same on the fp64 route (the short index) ----
int sed_join_knn_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist, sed_join_hit *out,
                          int64_t cap, int64_t *found) {
    return join_self(ix, ROUTE_F64, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_knn_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                            int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_F64, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_knn_bounds_f64(const sed_join_index *ix, double *bounds, int32_t n) { return join_knn_bounds(ix, ROUTE_F64, bounds, n); }

int sed_join_knn_candidates(const sed_join_index *ix, int64_t *n) {
    if (!ix || !n) return SED_E_ARG;
    if (ix->knn_candidates < 0) return SED_E_STATE;
    *n = ix->knn_candidates;
    return SED_OK;
}

int sed_join_knn_bound_time(const sed_join_index *ix, float *kernel_ms) {
    if (!ix || !kernel_ms) return SED_E_ARG;
    if (!ix->timer.timed || !ix->timer.knn) return SED_E_STATE;
    return hipEventElapsedTime(kernel_ms, ix->timer.ev[0], ix->timer.ev[2]) == hipSuccess ? SED_OK : SED_E_DEVICE;
}

int sed_join_long_knn_self(sed_join_long_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist,
                           sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_self(ix, ROUTE_INT, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_long_knn_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                             int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_INT, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_long_knn_bounds(const sed_join_long_index *ix, int32_t *bounds, int32_t n) { return sed_join_knn_bounds(ix, bounds, n); }

int sed_join_long_knn_candidates(const sed_join_long_index *ix, int64_t *n) { return sed_join_knn_candidates(ix, n); }

int sed_join_long_knn_bound_time(const sed_join_long_index *ix, float *kernel_ms) { return sed_join_knn_bound_time(ix, kernel_ms); }

// ---- sequences of up to 128 symbols: the calls above over the other index type (the integer route only) ----
int sed_join_long_self(sed_join_long_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out,
                       int64_t cap, int64_t *found) {
    return join_self(ix, ROUTE_INT, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_long_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                         int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, ROUTE_INT, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_long_last_time(const sed_join_long_index *ix, float *kernel_ms) { return sed_join_last_time(ix, kernel_ms); }

int sed_join_long_pairs_run(const sed_join_long_index *ix, int64_t *pairs) { return sed_join_pairs_run(ix, pairs); }

int32_t sed_join_long_max_len(void) { return SED_JOIN_LONG_MAXLEN; }

}  // extern "C"
