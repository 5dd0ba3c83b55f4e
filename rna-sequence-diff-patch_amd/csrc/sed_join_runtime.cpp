// sed_join_runtime.cpp — the similarity join's entry points of the C-ABI (include/sed.h): sed_join_index_* and
// sed_join_self / sed_join_search, their _f64 siblings and the k-nearest forms of both, sed_join_knn_*, over a resident
// index of short sequences, and sed_join_long_* over one of sequences of up to 128 symbols.  What a join runs is the join planner's decision (sed_join_plan.cpp), the
// kernels are sed_join.hip, sed_join_f64.hip and sed_join_long.hip; here: pack, reserve, upload, launch, download, sort,
// decode, on the context's stream (sed_runtime.h).  The two index types differ in one number, the record's length.
#include "sed_join_plan.h"
#include "sed_runtime.h"

#include <cmath>
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
struct JoinRec {  // one record of the device hit list (sed_internal.h: sed_join_args)
    uint32_t row, col, D, zero;  // (the fp64 route: D, zero = the distance's low and high words)
};
const size_t SPARE = 16;  // the spare bytes that end a record buffer (the kernels' row loads reach two words past a record)

const size_t F64_TAB = SED_JOIN_F64_MAXK * SED_JOIN_F64_MAXK;  // the fp64 table's doubles
const size_t F64_LOW = (SED_JOIN_MAXLEN + 1) * (SED_JOIN_MAXLEN + 1);  // its k-nearest calls' lower-bound table's

uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}
double double_of(uint64_t b) {
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

uint32_t code_bit(uint8_t c) { return 1u << (c < 31 ? c : 31); }
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
    DevBuf d_tab, d_hits, d_count;
    DevBuf d_bound;                // the k-nearest calls' bound of every row, indexed as the rows are (fp64 route: 8 bytes a row)
    std::vector<uint32_t> h_bound; // the last k-nearest call's bounds after pass 1, one a row of the call
    std::vector<uint64_t> h_bound64;  // the same when that call took the fp64 route (knn_f64): the bits of a double each
    bool knn_f64 = false;          // the last k-nearest call that got past its plan took the fp64 route
    std::vector<sed_join_hit> h_knn;  // its candidates, decoded, for the trim
    int64_t knn_candidates = -1;   // the hits its pass 2 appended; -1 before the first k-nearest call
    uint32_t h_tab[16] = {};       // the cost rows of the call under way (the upload's source)
    DevBuf d_f64;                  // the fp64 route's table and keep words, and their upload's source
    uint64_t h_f64[F64_TAB + SED_JOIN_MAXLEN + 1] = {};
    DevBuf d_f64k;                 // its k-nearest calls': [the table | the lower-bound table], and their upload's source
    double h_f64k[F64_TAB + F64_LOW] = {};
    std::vector<uint8_t> h_query;
    std::vector<JoinRec> h_hits;
    PinBuf pin;                    // the two counters' download
    JoinTimer timer;
    int64_t pairs_run = -1;
    ~sed_join_index() {
        pin.release();
        d_rows.release(); d_row_len.release(); d_cols.release(); d_col_len.release(); d_col_orig.release();
        d_query.release(); d_tab.release(); d_f64.release(); d_f64k.release(); d_hits.release(); d_count.release(); d_bound.release();
    }
};

struct sed_join_long_index : sed_join_index {};  // (a type of its own in the C-ABI: its records are 128 bytes)

// What a call runs: the integer plan or the fp64 plan (exactly one is set)
struct JoinCall {
    const sed_join_plan_t *pi = nullptr;
    const sed_join_f64_plan_t *pf = nullptr;
    int32_t knn = 0;  // k of a k-nearest call (of either route), 0: a join
    int64_t launch_rows() const { return pi ? pi->launch_rows : pf->launch_rows; }
};

// The integer route's arguments but for the sides: the cost rows' upload, the plan's numbers, the list
static hipError_t join_int_args(sed_join_index *ix, const sed_join_plan_t &plan, const sed_join_list &list, sed_join_args *a) {
    memcpy(ix->h_tab, plan.sp.row, sizeof ix->h_tab);
    a->tab = (const uint2 *)ix->d_tab.p;
    a->ins = plan.sp.ins;
    a->del = plan.sp.del;
    a->umap = plan.sp.umap;
    a->shift = plan.scale_log2;
    a->cut = plan.cut;
    a->out = list;
    return hipMemcpyAsync(ix->d_tab.p, ix->h_tab, sizeof ix->h_tab, hipMemcpyHostToDevice, ix->ctx->stream);
}

// The columns' side of every launch
static void join_cols(const sed_join_index *ix, sed_join_sides *s) {
    s->cols = ix->d_cols.p;
    s->col_len = (const int32_t *)ix->d_col_len.p;
    s->col_orig = (const int32_t *)ix->d_col_orig.p;
    s->ncols = ix->nseqs;
}

// A k-nearest call once its rows are on the device (k.knn = k, k.pi or k.pf the plan; s, nrows as join_run takes them):
// every row's bound set to the plan's cut (the fp64 route: to max_dist's bits, a 64-bit word a row); per row launch pass 1 (the bounds) then pass 2 (the candidates {D <= bound[r]}) on
// the one stream; the counters, the bounds and the candidates come down; the trim keeps each row's first k by (D, col).
// The device list is sized for the candidates: when pass 2 overflows it, it grows to the count the device reports and
// pass 2 alone runs once more (the bounds are final), which the pairs counted leave out and the time spans.
static int join_knn_run(sed_join_index *ix, const JoinCall &k, sed_join_sides s, int32_t nrows, sed_join_hit *out, int64_t cap,
                        int64_t *found) {
    sed_ctx *c = ix->ctx;
    const bool f64 = k.pf != nullptr;
    const int32_t first = s.row0;
    const size_t nbound = (size_t)first + (size_t)nrows;
    const size_t guess = 2 * (size_t)nrows * (size_t)k.knn + 1024;  // records: twice the answer and a little
    if (!ix->d_count.reserve(16) || !(f64 ? ix->d_f64k.reserve(sizeof ix->h_f64k) : ix->d_tab.reserve(sizeof ix->h_tab)) ||
        !ix->d_bound.reserve(nbound * (f64 ? sizeof(uint64_t) : sizeof(uint32_t))) ||
        !ix->d_hits.reserve(guess * sizeof(JoinRec)) || !ix->pin.reserve(16, 64))
        return c->fail(SED_E_OOM, "device allocation failed (k-nearest join, %d rows)", nrows);
    hipError_t e = hipSuccess;
    if ((e = ix->timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    join_cols(ix, &s);
    sed_join_knn_args ka{};  // (one of ka and kf is filled and launched: the call's route)
    sed_join_knn_f64_args kf{};
    ka.bound = (uint32_t *)ix->d_bound.p;
    kf.bound = (unsigned long long *)ix->d_bound.p;
    ka.k = kf.k = k.knn;
    const bool bitpar = !f64 && k.pi->kernel == SED_JOIN_KERNEL_BITPAR;
    const int64_t step = k.launch_rows();
    ix->knn_candidates = -1;  // (a call that fails from here on leaves nothing to report)
    if (f64)
        ix->h_bound64.assign((size_t)nrows, 0u);
    else
        ix->h_bound.assign((size_t)nrows, 0u);
    const size_t bsize = f64 ? sizeof(uint64_t) : sizeof(uint32_t);
    void *const d_first = (uint8_t *)ix->d_bound.p + (size_t)first * bsize;
    void *const h_first = f64 ? (void *)ix->h_bound64.data() : (void *)ix->h_bound.data();
    uint64_t n = 0;
    for (int run = 0; run < 2; ++run) {  // (run 1: pass 2 again with room for what run 0 counted)
        const sed_join_list list{(uint4 *)ix->d_hits.p, (unsigned long long *)ix->d_count.p,
                                 (unsigned long long)(ix->d_hits.cap / sizeof(JoinRec))};
        if ((e = hipMemsetAsync(ix->d_count.p, 0, 16, c->stream)) != hipSuccess) return c->hipfail(e, "upload (k-nearest join)");
        if (f64) {  // one block: [the table | the lower-bound table]; the bounds start as max_dist's bits
            const sed_join_f64_plan_t &plan = *k.pf;
            static_assert(sizeof ix->h_f64k == sizeof plan.sub + sizeof plan.low, "the upload's layout");
            memcpy(ix->h_f64k, plan.sub, sizeof plan.sub);
            memcpy(ix->h_f64k + F64_TAB, plan.low, sizeof plan.low);
            kf.j.sub = (const double *)ix->d_f64k.p;
            kf.low = (const double *)ix->d_f64k.p + F64_TAB;
            kf.j.ins = plan.ins;
            kf.j.del = plan.del;
            kf.j.max_dist = plan.max_dist;
            kf.j.out = list;
            e = hipMemcpyAsync(ix->d_f64k.p, ix->h_f64k, sizeof ix->h_f64k, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess && run == 0) {
                std::fill(ix->h_bound64.begin(), ix->h_bound64.end(), bits_of(plan.max_dist));
                e = hipMemcpyAsync(d_first, h_first, (size_t)nrows * bsize, hipMemcpyHostToDevice, c->stream);
            }
        } else if ((e = join_int_args(ix, *k.pi, list, &ka.j)) == hipSuccess && run == 0) {
            e = hipMemsetD32Async((hipDeviceptr_t)d_first, k.pi->cut, (size_t)nrows, c->stream);
        }
        if (e != hipSuccess) return c->hipfail(e, "upload (k-nearest join)");
        for (int64_t r = 0; r < nrows; r += step) {
            s.row0 = first + (int32_t)r;
            s.nrows = (int32_t)std::min<int64_t>(step, nrows - r);
            ka.j.s = kf.j.s = s;
            const bool head = r == 0, tail = r + step >= nrows;
            for (int emit = run; emit < 2; ++emit) {
                hipEvent_t e0 = run == 0 && head && !emit ? ix->timer.ev[0] : nullptr;
                hipEvent_t e1 = emit ? (tail ? ix->timer.ev[1] : nullptr) : (run == 0 && head ? ix->timer.ev[2] : nullptr);
                e = f64 ? sed_launch_join_knn_f64(c->stream, e0, e1, kf, emit != 0)
                    : ix->maxlen == SED_JOIN_LONG_MAXLEN ? sed_launch_join_long_knn(c->stream, e0, e1, ka, bitpar, emit != 0)
                                                         : sed_launch_join_knn(c->stream, e0, e1, ka, bitpar, emit != 0);
                if (e != hipSuccess) return c->hipfail(e, "k-nearest join kernel launch");
            }
        }
        if ((e = hipMemcpyAsync(ix->pin.p, ix->d_count.p, 16, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (run == 0 && (e = hipMemcpyAsync(h_first, d_first, (size_t)nrows * bsize, hipMemcpyDeviceToHost, c->stream)) !=
                             hipSuccess))
            return c->hipfail(e, "download (k-nearest join)");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "k-nearest join kernel execution");
        ix->timer.timed = ix->timer.knn = true;
        n = ((const uint64_t *)ix->pin.p)[0];
        if (run == 0) ix->pairs_run = (int64_t)((const uint64_t *)ix->pin.p)[1];
        if (n <= list.cap) break;
        if (run == 1) return c->fail(SED_E_DEVICE, "k-nearest join: %llu candidates after room was made for them", (unsigned long long)n);
        if (n > SIZE_MAX / sizeof(JoinRec) || !ix->d_hits.reserve((size_t)n * sizeof(JoinRec)))
            return c->fail(SED_E_OOM, "device allocation failed (k-nearest join, room for %llu candidates)", (unsigned long long)n);
    }
    ix->knn_candidates = (int64_t)n;
    ix->h_hits.resize((size_t)n);
    if (n != 0 && ((e = hipMemcpyAsync(ix->h_hits.data(), ix->d_hits.p, (size_t)n * sizeof(JoinRec), hipMemcpyDeviceToHost,
                                       c->stream)) != hipSuccess ||
                   (e = hipStreamSynchronize(c->stream)) != hipSuccess))
        return c->hipfail(e, "download (k-nearest candidates)");
    const double inv = f64 ? 0.0 : std::ldexp(1.0, -k.pi->scale_log2);
    ix->h_knn.resize((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) {
        const JoinRec &r = ix->h_hits[i];
        bool ok = r.row >= (uint32_t)first && r.row < (uint32_t)first + (uint32_t)nrows && r.col < (uint32_t)ix->nseqs &&
                  !(s.self && r.row == r.col);
        double dist = 0;
        if (ok && f64) {  // (D, zero) = the double's low and high words, copied, not scaled; NaN fails the compares
            dist = double_of((uint64_t)r.D | ((uint64_t)r.zero << 32));
            ok = dist >= 0 && dist <= double_of(ix->h_bound64[r.row - (uint32_t)first]) && dist <= k.pf->max_dist;
        } else if (ok) {
            dist = (double)r.D * inv;
            ok = r.D <= ix->h_bound[r.row - (uint32_t)first] && r.D <= (uint32_t)k.pi->cut;
        }
        if (!ok)
            return c->fail(SED_E_DEVICE, "k-nearest join: record %zu from the device is no candidate (row %u, column %u)", i,
                           r.row, r.col);
        ix->h_knn[i] = sed_join_hit{(int32_t)r.row, (int32_t)r.col, dist};
    }
    int64_t kept = 0;
    if (sed_join_knn_trim(ix->h_knn.data(), (int64_t)n, k.knn, &kept) != SED_OK)
        return c->fail(SED_E_DEVICE, "k-nearest join: the trim refused the device's records");
    for (int64_t i = 1; i < kept; ++i)
        if (ix->h_knn[i - 1].row == ix->h_knn[i].row && ix->h_knn[i - 1].col == ix->h_knn[i].col)
            return c->fail(SED_E_DEVICE, "k-nearest join: row %d reports column %d twice", ix->h_knn[i].row, ix->h_knn[i].col);
    *found = kept;
    if (kept > cap)
        return c->fail(SED_E_RANGE, "join: found %lld hits, cap %lld: call again with room for them", (long long)kept,
                       (long long)cap);
    if (kept) memcpy(out, ix->h_knn.data(), (size_t)kept * sizeof(sed_join_hit));
    return SED_OK;
}

// What all joins share once their rows are on the device: the plan's launches, the counters, the hit list.
// s holds the rows (rows, row_len, row0, self); nrows rows from s.row0 on.
static int join_run(sed_join_index *ix, const JoinCall &k, sed_join_sides s, int32_t nrows, sed_join_hit *out, int64_t cap,
                    int64_t *found) {
    if (k.knn) return join_knn_run(ix, k, s, nrows, out, cap, found);
    sed_ctx *c = ix->ctx;
    if ((uint64_t)cap > SIZE_MAX / sizeof(JoinRec) || !ix->d_count.reserve(16) ||
        !(k.pi ? ix->d_tab.reserve(sizeof ix->h_tab) : ix->d_f64.reserve(sizeof ix->h_f64)) ||
        !ix->d_hits.reserve(std::max<size_t>((size_t)cap * sizeof(JoinRec), sizeof(JoinRec))) || !ix->pin.reserve(16, 64))
        return c->fail(SED_E_OOM, "device allocation failed (join, room for %lld hits)", (long long)cap);
    hipError_t e = hipSuccess;
    if ((e = ix->timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    if ((e = hipMemsetAsync(ix->d_count.p, 0, 16, c->stream)) != hipSuccess) return c->hipfail(e, "upload (join)");
    join_cols(ix, &s);
    const sed_join_list list{(uint4 *)ix->d_hits.p, (unsigned long long *)ix->d_count.p, (unsigned long long)cap};
    sed_join_args a{};  // (one of a and f is filled and launched: the call's route)
    sed_join_f64_args f{};
    if (k.pi) {
        e = join_int_args(ix, *k.pi, list, &a);
    } else {  // one block: [the table | the keep words]
        const sed_join_f64_plan_t &plan = *k.pf;
        static_assert(sizeof ix->h_f64 == sizeof plan.sub + sizeof plan.keep, "the upload's layout");
        memcpy(ix->h_f64, plan.sub, sizeof plan.sub);
        memcpy(ix->h_f64 + F64_TAB, plan.keep, sizeof plan.keep);
        e = hipMemcpyAsync(ix->d_f64.p, ix->h_f64, sizeof ix->h_f64, hipMemcpyHostToDevice, c->stream);
        f.sub = (const double *)ix->d_f64.p;
        f.keep = (const unsigned long long *)ix->d_f64.p + F64_TAB;
        f.ins = plan.ins;
        f.del = plan.del;
        f.max_dist = plan.max_dist;
        f.out = list;
    }
    if (e != hipSuccess) return c->hipfail(e, "upload (join)");
    const int32_t first = s.row0;
    const int64_t step = k.launch_rows();
    for (int64_t r = 0; r < nrows; r += step) {  // the events bracket the launches
        s.row0 = first + (int32_t)r;
        s.nrows = (int32_t)std::min<int64_t>(step, nrows - r);
        hipEvent_t e0 = r == 0 ? ix->timer.ev[0] : nullptr, e1 = r + step >= nrows ? ix->timer.ev[1] : nullptr;
        if (!k.pi) {
            f.s = s;
            e = sed_launch_join_f64(c->stream, e0, e1, f);
        } else {
            a.s = s;
            const bool bitpar = k.pi->kernel == SED_JOIN_KERNEL_BITPAR;
            e = ix->maxlen == SED_JOIN_LONG_MAXLEN ? sed_launch_join_long(c->stream, e0, e1, a, bitpar)
                                                   : sed_launch_join(c->stream, e0, e1, a, bitpar);
        }
        if (e != hipSuccess) return c->hipfail(e, "join kernel launch");
    }
    if ((e = hipMemcpyAsync(ix->pin.p, ix->d_count.p, 16, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "download (join)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "join kernel execution");
    ix->timer.timed = true;
    ix->timer.knn = false;
    const uint64_t n = ((const uint64_t *)ix->pin.p)[0];
    ix->pairs_run = (int64_t)((const uint64_t *)ix->pin.p)[1];
    *found = (int64_t)n;
    if (n > (uint64_t)cap)
        return c->fail(SED_E_RANGE, "join: found %lld hits, cap %lld: call again with room for them", (long long)n,
                       (long long)cap);
    if (n == 0) return SED_OK;
    ix->h_hits.resize((size_t)n);
    if ((e = hipMemcpyAsync(ix->h_hits.data(), ix->d_hits.p, (size_t)n * sizeof(JoinRec), hipMemcpyDeviceToHost, c->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return c->hipfail(e, "download (join hits)");
    std::sort(ix->h_hits.begin(), ix->h_hits.end(),
              [](const JoinRec &x, const JoinRec &y) { return x.row != y.row ? x.row < y.row : x.col < y.col; });
    const double inv = k.pi ? std::ldexp(1.0, -k.pi->scale_log2) : 0.0;
    for (size_t i = 0; i < (size_t)n; ++i) {
        const JoinRec &r = ix->h_hits[i];
        double dist;
        bool within;
        if (k.pi) {
            within = r.D <= (uint32_t)k.pi->cut;
            dist = (double)r.D * inv;
        } else {  // (D, zero) = the double's low and high words, copied, not scaled; NaN fails the compare
            const uint64_t bits = (uint64_t)r.D | ((uint64_t)r.zero << 32);
            memcpy(&dist, &bits, sizeof dist);
            within = dist <= k.pf->max_dist;
        }
        if (r.row < (uint32_t)first || r.row >= (uint32_t)first + (uint32_t)nrows || r.col >= (uint32_t)ix->nseqs || !within ||
            (i > 0 && ix->h_hits[i - 1].row == r.row && ix->h_hits[i - 1].col == r.col))
            return c->fail(SED_E_DEVICE, "join: record %zu from the device is no hit (row %u, column %u)", i, r.row, r.col);
        out[i] = sed_join_hit{(int32_t)r.row, (int32_t)r.col, dist};
    }
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

// The plan of a call under either route (f64: the fp64 planner), the refusal's text in the context
static int join_plan_call(sed_ctx *c, bool f64, const int32_t *len_rows, int32_t nrows, const sed_join_index *ix, bool self,
                          uint32_t row_codes, double max_dist, sed_join_plan_t *pi, sed_join_f64_plan_t *pf, JoinCall *k) {
    if (f64) {
        k->pf = pf;
        return sed_join_f64_plan_of(c->costs, c->opt, len_rows, nrows, ix->len.data(), ix->nseqs, self, row_codes, ix->codes,
                                    max_dist, pf, &c->err);
    }
    k->pi = pi;
    return sed_join_plan_of(c->costs, c->opt, len_rows, nrows, ix->len.data(), ix->nseqs, self, row_codes, ix->codes, max_dist,
                            ix->maxlen, pi, &c->err);
}

// A k-nearest call got past its plan: what sed_join_knn_bounds and sed_join_knn_candidates report until it has run
static void join_knn_planned(sed_join_index *ix, const JoinCall &k, int32_t nrows) {
    if (!k.knn) return;
    ix->knn_f64 = k.pf != nullptr;
    if (k.pf)
        ix->h_bound64.assign((size_t)nrows, bits_of(k.pf->max_dist));
    else
        ix->h_bound.assign((size_t)nrows, (uint32_t)k.pi->cut);
    ix->knn_candidates = 0;
}

// (knn: NULL for a join, else k of the k-nearest call)
static int join_self(sed_join_index *ix, bool f64, const int32_t *knn, int32_t row_lo, int32_t row_hi, double max_dist,
                     sed_join_hit *out, int64_t cap, int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    int rc = join_enter(c, 0 <= row_lo && row_lo <= row_hi && row_hi <= ix->nseqs && cap >= 0 && (cap == 0 || out) && found,
                        knn);
    if (rc != SED_OK) return rc;
    sed_join_plan_t pi;
    sed_join_f64_plan_t pf;
    JoinCall k;
    k.knn = knn ? *knn : 0;
    const int32_t nrows = row_hi - row_lo;
    rc = join_plan_call(c, f64, ix->len.data() + row_lo, nrows, ix, true, ix->codes, max_dist, &pi, &pf, &k);
    if (rc != SED_OK) return rc;
    *found = 0;
    ix->pairs_run = 0;
    join_knn_planned(ix, k, nrows);
    if (nrows == 0) return SED_OK;
    sed_join_sides s{};
    s.rows = ix->d_rows.p;
    s.row_len = (const int32_t *)ix->d_row_len.p;
    s.row0 = row_lo;
    s.self = 1;
    return join_run(ix, k, s, nrows, out, cap, found);
}

static int join_search(sed_join_index *ix, bool f64, const int32_t *knn, const uint8_t *codes_q, const int64_t *off_q,
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
    sed_join_plan_t pi;
    sed_join_f64_plan_t pf;
    JoinCall k;
    k.knn = knn ? *knn : 0;
    rc = join_plan_call(c, f64, len_q, nqueries, ix, false, qcodes, max_dist, &pi, &pf, &k);
    if (rc != SED_OK) return rc;
    *found = 0;
    ix->pairs_run = 0;
    join_knn_planned(ix, k, nqueries);
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

extern "C" {

int sed_join_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                  int64_t *found) {
    return join_self(ix, false, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                      int64_t *found) {
    return join_self(ix, true, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                    int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, false, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, true, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
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
    return join_self(ix, false, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_knn_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                        int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, false, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_knn_bounds(const sed_join_index *ix, int32_t *bounds, int32_t n) {
    if (!ix || n < 0 || (n && !bounds)) return SED_E_ARG;
    if (ix->knn_candidates < 0 || ix->knn_f64) return SED_E_STATE;
    if ((size_t)n != ix->h_bound.size()) return SED_E_ARG;
    for (int32_t i = 0; i < n; ++i) bounds[i] = (int32_t)ix->h_bound[(size_t)i];
    return SED_OK;
}

// ---- the same on the fp64 route (the short index) ----
int sed_join_knn_self_f64(sed_join_index *ix, int32_t row_lo, int32_t row_hi, int32_t k, double max_dist, sed_join_hit *out,
                          int64_t cap, int64_t *found) {
    return join_self(ix, true, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_knn_search_f64(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                            int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, true, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_knn_bounds_f64(const sed_join_index *ix, double *bounds, int32_t n) {
    if (!ix || n < 0 || (n && !bounds)) return SED_E_ARG;
    if (ix->knn_candidates < 0 || !ix->knn_f64) return SED_E_STATE;
    if ((size_t)n != ix->h_bound64.size()) return SED_E_ARG;
    for (int32_t i = 0; i < n; ++i) bounds[i] = double_of(ix->h_bound64[(size_t)i]);
    return SED_OK;
}

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
    return join_self(ix, false, &k, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_long_knn_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                             int32_t nqueries, int32_t k, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, false, &k, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_long_knn_bounds(const sed_join_long_index *ix, int32_t *bounds, int32_t n) { return sed_join_knn_bounds(ix, bounds, n); }

int sed_join_long_knn_candidates(const sed_join_long_index *ix, int64_t *n) { return sed_join_knn_candidates(ix, n); }

int sed_join_long_knn_bound_time(const sed_join_long_index *ix, float *kernel_ms) { return sed_join_knn_bound_time(ix, kernel_ms); }

// ---- sequences of up to 128 symbols: the calls above over the other index type (the integer route only) ----
int sed_join_long_self(sed_join_long_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out,
                       int64_t cap, int64_t *found) {
    return join_self(ix, false, nullptr, row_lo, row_hi, max_dist, out, cap, found);
}

int sed_join_long_search(sed_join_long_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                         int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    return join_search(ix, false, nullptr, codes_q, off_q, len_q, nqueries, max_dist, out, cap, found);
}

int sed_join_long_last_time(const sed_join_long_index *ix, float *kernel_ms) { return sed_join_last_time(ix, kernel_ms); }

int sed_join_long_pairs_run(const sed_join_long_index *ix, int64_t *pairs) { return sed_join_pairs_run(ix, pairs); }

int32_t sed_join_long_max_len(void) { return SED_JOIN_LONG_MAXLEN; }

}  // extern "C"
