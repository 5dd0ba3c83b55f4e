// sed_join_runtime.cpp — the similarity join's entry points of the C-ABI (include/sed.h): sed_join_index_* and
// sed_join_self / sed_join_search over a resident index of short sequences.  What a join runs is the join planner's
// decision (sed_join_plan.cpp), the kernels are sed_join.hip; here: pack, reserve, upload, launch, download, sort,
// decode, on the context's stream (sed_runtime.h).
#include "sed_join_plan.h"
#include "sed_runtime.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {
struct JoinTimer {  // the events around a call's launches, created on first use
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
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
    uint32_t row, col, D, zero;
};
const size_t REC = SED_JOIN_MAXLEN, SPARE = 16;  // a sequence record, and the spare bytes that end a record buffer

uint32_t code_bit(uint8_t c) { return 1u << (c < 31 ? c : 31); }
}  // namespace

struct sed_join_index {
    sed_ctx *ctx = nullptr;
    int32_t nseqs = 0;
    uint32_t codes = 0;            // bit c: code c occurs (bit 31: any code >= 31)
    std::vector<int32_t> len;      // in the caller's order: the rows of a self join
    std::vector<int32_t> col_len;  // sorted by length: the columns
    // the records in the caller's order and their lengths (rows of a self join); the records sorted by length (stable),
    // their lengths and original indices (columns of every join); a search's query records and lengths
    DevBuf d_rows, d_row_len, d_cols, d_col_len, d_col_orig, d_query;
    DevBuf d_tab, d_hits, d_count;
    uint32_t h_tab[16] = {};       // the cost rows of the call under way (the upload's source)
    std::vector<uint8_t> h_query;
    std::vector<JoinRec> h_hits;
    PinBuf pin;                    // the two counters' download
    JoinTimer timer;
    int64_t pairs_run = -1;
    ~sed_join_index() {
        pin.release();
        d_rows.release(); d_row_len.release(); d_cols.release(); d_col_len.release(); d_col_orig.release();
        d_query.release(); d_tab.release(); d_hits.release(); d_count.release();
    }
};

// What both joins share once their rows are on the device: the plan's launches, the counters, the hit list.
// a holds the rows and columns; nrows rows from a.row0 on.
static int join_run(sed_join_index *ix, const sed_join_plan_t &plan, sed_join_args a, int32_t nrows, sed_join_hit *out,
                    int64_t cap, int64_t *found) {
    sed_ctx *c = ix->ctx;
    if ((uint64_t)cap > SIZE_MAX / sizeof(JoinRec) || !ix->d_count.reserve(16) || !ix->d_tab.reserve(sizeof ix->h_tab) ||
        !ix->d_hits.reserve(std::max<size_t>((size_t)cap * sizeof(JoinRec), sizeof(JoinRec))) || !ix->pin.reserve(16, 64))
        return c->fail(SED_E_OOM, "device allocation failed (join, room for %lld hits)", (long long)cap);
    hipError_t e = hipSuccess;
    if ((e = ix->timer.begin()) != hipSuccess) return c->hipfail(e, "event create");
    memcpy(ix->h_tab, plan.sp.row, sizeof ix->h_tab);
    if ((e = hipMemsetAsync(ix->d_count.p, 0, 16, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(ix->d_tab.p, ix->h_tab, sizeof ix->h_tab, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return c->hipfail(e, "upload (join)");
    a.cols = ix->d_cols.p;
    a.col_len = (const int32_t *)ix->d_col_len.p;
    a.col_orig = (const int32_t *)ix->d_col_orig.p;
    a.ncols = ix->nseqs;
    a.tab = (const uint2 *)ix->d_tab.p;
    a.ins = plan.sp.ins;
    a.del = plan.sp.del;
    a.umap = plan.sp.umap;
    a.shift = plan.scale_log2;
    a.cut = plan.cut;
    a.hits = (uint4 *)ix->d_hits.p;
    a.count = (unsigned long long *)ix->d_count.p;
    a.cap = (unsigned long long)cap;
    const int32_t first = a.row0;
    for (int64_t r = 0; r < nrows; r += plan.launch_rows) {  // the events bracket the launches
        a.row0 = first + (int32_t)r;
        a.nrows = (int32_t)std::min<int64_t>(plan.launch_rows, nrows - r);
        if ((e = sed_launch_join(c->stream, r == 0 ? ix->timer.ev[0] : nullptr,
                                 r + plan.launch_rows >= nrows ? ix->timer.ev[1] : nullptr, a,
                                 plan.kernel == SED_JOIN_KERNEL_BITPAR)) != hipSuccess)
            return c->hipfail(e, "join kernel launch");
    }
    if ((e = hipMemcpyAsync(ix->pin.p, ix->d_count.p, 16, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "download (join)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "join kernel execution");
    ix->timer.timed = true;
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
    const double inv = std::ldexp(1.0, -plan.scale_log2);
    for (size_t i = 0; i < (size_t)n; ++i) {
        const JoinRec &r = ix->h_hits[i];
        if (r.row < (uint32_t)first || r.row >= (uint32_t)first + (uint32_t)nrows || r.col >= (uint32_t)ix->nseqs ||
            r.D > (uint32_t)plan.cut || (i > 0 && ix->h_hits[i - 1].row == r.row && ix->h_hits[i - 1].col == r.col))
            return c->fail(SED_E_DEVICE, "join: record %zu from the device is no hit (row %u, column %u)", i, r.row, r.col);
        out[i] = sed_join_hit{(int32_t)r.row, (int32_t)r.col, (double)r.D * inv};
    }
    return SED_OK;
}

// What every join refuses first, in sed_fit_index_search's order
static int join_enter(sed_ctx *c, bool args_ok) {
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (!args_ok) return c->fail(SED_E_ARG, "bad join arguments");
    if (!c->have_costs) return c->fail(SED_E_STATE, "sed_set_costs() was not called");
    (void)hipSetDevice(c->device);
    return SED_OK;
}

extern "C" {

sed_join_index *sed_join_index_create(sed_ctx *c, const uint8_t *codes, const int64_t *off, const int32_t *len,
                                      int32_t nseqs) {
    if (!c) return nullptr;
    if (nseqs < 0 || (nseqs > 0 && (!codes || !off || !len))) {
        c->fail(SED_E_ARG, "bad join index arguments");
        return nullptr;
    }
    for (int i = 0; i < nseqs; ++i)
        if (len[i] < 0 || len[i] > SED_JOIN_MAXLEN || off[i] < 0) {
            if (off[i] < 0 || len[i] < 0)
                c->fail(SED_E_ARG, "join index: sequence %d: negative %s", i, len[i] < 0 ? "length" : "offset");
            else
                c->fail(SED_E_ARG, "join index: sequence %d has %d symbols (at most %d)", i, len[i], SED_JOIN_MAXLEN);
            return nullptr;
        }
    (void)hipSetDevice(c->device);
    sed_join_index *ix = new sed_join_index;
    ix->ctx = c;
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

void sed_join_index_destroy(sed_join_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    delete ix;
}

int32_t sed_join_index_seqs(const sed_join_index *ix) { return ix ? ix->nseqs : SED_E_ARG; }

int sed_join_self(sed_join_index *ix, int32_t row_lo, int32_t row_hi, double max_dist, sed_join_hit *out, int64_t cap,
                  int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    int rc = join_enter(c, 0 <= row_lo && row_lo <= row_hi && row_hi <= ix->nseqs && cap >= 0 && (cap == 0 || out) && found);
    if (rc != SED_OK) return rc;
    sed_join_plan_t plan;
    const int32_t nrows = row_hi - row_lo;
    rc = sed_join_plan_of(c->costs, c->opt, ix->len.data() + row_lo, nrows, ix->len.data(), ix->nseqs, true, ix->codes,
                          ix->codes, max_dist, &plan, &c->err);
    if (rc != SED_OK) return rc;
    *found = 0;
    ix->pairs_run = 0;
    if (nrows == 0) return SED_OK;
    sed_join_args a{};
    a.rows = ix->d_rows.p;
    a.row_len = (const int32_t *)ix->d_row_len.p;
    a.row0 = row_lo;
    a.self = 1;
    return join_run(ix, plan, a, nrows, out, cap, found);
}

int sed_join_search(sed_join_index *ix, const uint8_t *codes_q, const int64_t *off_q, const int32_t *len_q,
                    int32_t nqueries, double max_dist, sed_join_hit *out, int64_t cap, int64_t *found) {
    if (!ix) return SED_E_ARG;
    sed_ctx *c = ix->ctx;
    int rc = join_enter(c, (nqueries == 0 || (nqueries > 0 && codes_q && off_q && len_q)) && cap >= 0 && (cap == 0 || out) &&
                               found);
    if (rc != SED_OK) return rc;
    // the queries' records and lengths, one block: [records | spare | lengths]
    const size_t o_len = REC * (size_t)nqueries + SPARE, qbytes = o_len + sizeof(int32_t) * (size_t)nqueries;
    ix->h_query.assign(qbytes, 0);
    uint32_t qcodes = 0;
    for (int q = 0; q < nqueries; ++q) {
        if (off_q[q] < 0) return c->fail(SED_E_ARG, "query %d: negative offset", q);
        if (len_q[q] < 0 || len_q[q] > SED_JOIN_MAXLEN)
            return c->fail(SED_E_ARG, "query %d has %d symbols (0..%d)", q, len_q[q], SED_JOIN_MAXLEN);
        for (int j = 0; j < len_q[q]; ++j) qcodes |= code_bit(ix->h_query[REC * (size_t)q + j] = codes_q[off_q[q] + j]);
    }
    if (nqueries) memcpy(&ix->h_query[o_len], len_q, sizeof(int32_t) * (size_t)nqueries);
    sed_join_plan_t plan;
    rc = sed_join_plan_of(c->costs, c->opt, len_q, nqueries, ix->len.data(), ix->nseqs, false, qcodes, ix->codes, max_dist,
                          &plan, &c->err);
    if (rc != SED_OK) return rc;
    *found = 0;
    ix->pairs_run = 0;
    if (nqueries == 0 || ix->nseqs == 0) return SED_OK;
    if (!ix->d_query.reserve(qbytes)) return c->fail(SED_E_OOM, "device allocation failed (join, %d queries)", nqueries);
    hipError_t e = hipMemcpyAsync(ix->d_query.p, ix->h_query.data(), qbytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->hipfail(e, "upload (join queries)");
    sed_join_args a{};
    a.rows = ix->d_query.p;
    a.row_len = (const int32_t *)((const uint8_t *)ix->d_query.p + o_len);
    a.row0 = 0;
    a.self = 0;
    return join_run(ix, plan, a, nqueries, out, cap, found);
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

}  // extern "C"
