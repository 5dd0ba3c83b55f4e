// sed_runtime.cpp — the C-ABI of libsed.so (include/sed.h): contexts, the
// cost model, device-resident batches and the launch sequence
//   DP kernel (integer or fp64)  ->  traceback kernel
// on one HIP stream, timed with HIP events recorded on that stream.  What a batch runs (mode, routes, layout,
// kernel parameters) and what a run launches (sed_plan_run: the launcher calls in order, their streams and who carries
// which event) is the planner's decision (sed_plan.cpp); a fill here is: wait, plan, reserve, upload, streams, and a
// run is one loop over the planned steps (run_batch).
// Fit search's entry points are sed_fit_runtime.cpp; the context and the buffers both units use are sed_runtime.h.
#include "../../include/sed.h"
#include "sed_internal.h"
#include "sed_plan.h"
#include "sed_runtime.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

const sed_opts &sed_env_opts() {
    static const sed_opts env = [] {
        sed_opts o;
        auto knob = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        o.env_tbpar = knob("SED_TBPAR", -1);
        o.env_band = knob("SED_BAND", 1);
        if (const char *e = getenv("SED_BAND"))
            if (!strcmp(e, "static")) o.env_band = 3;  // band pruning with the static windows only
        o.env_alt_dp = knob("SED_ALT_DP", 1);
        o.env_ck_halves = knob("SED_CK_HALVES", -1);
        return o;
    }();
    return env;
}

// Cutoff batches: the wave pairs of a batch with x2 or CHAIN pairs move to the windowed stripe kernel when the window
// keeps less than this share of their cells (sed_batch_set_cutoff)
#ifndef SED_CUT_SHARE
#define SED_CUT_SHARE (2.0 / 3.0)
#endif

namespace {
// grow the context's pinned staging to `bytes` (first waiting for a copy still in flight from it)
hipError_t pin_reserve(sed_ctx *c, size_t bytes) {
    hipError_t e = hipSuccess;
    if (c->pin_busy && (e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    c->pin_busy = false;
    return c->pin.reserve(bytes, 1u << 20) ? hipSuccess : hipErrorOutOfMemory;
}
}  // namespace

struct sed_batch {
    sed_ctx *ctx = nullptr;
    sed_plan plan;                // what the last fill decided (sed_plan.h)
    sed_run_plan sched;           // what a run launches under the plan and the cutoff state (set_cut_state)
    std::vector<uint32_t> ha, hb;  // the packed sequences on their way up (kept across refills)
    DevBuf d_pd, d_seqa, d_seqb, d_bnd, d_ops, d_tasks, d_lane, d_chain, d_x2, d_tbmap, d_seg;
    // small batches (plan.small) keep every input array and the results in one blob, d_small; the kernels' pointers
    // (p_*) point into it or at the per-array buffers above
    DevBuf d_small;
    // small batches whose kernels write their results and scripts with plain stores (not the stripe-parallel walk's
    // atomicOr; plan.zc): the kernels write them straight into this pinned host block, so no download follows the run
    // (sed_run_pair on a 30-nt pair: one copy kernel fewer per call)
    void *h_out = nullptr;
    size_t h_out_cap = 0;
    // a zero-copy run was enqueued on the context's stream and not yet waited for (set before its first launch, so a
    // run that failed halfway counts too): the kernels may still store into h_out
    bool zc_busy = false;
    void *p_pd = nullptr, *p_seqa = nullptr, *p_seqb = nullptr, *p_tasks = nullptr, *p_lane = nullptr,
         *p_chain = nullptr, *p_x2 = nullptr, *p_ops = nullptr, *p_seg = nullptr, *p_res[3] = {nullptr, nullptr, nullptr};
    // timing events: 1 on every run (default), k > 1 on every k-th run, 0 never (sed_batch_set_timing; runs that
    // order buffer reuse through their events always record them)
    int time_every = 1;
    // SPLIT hand-off words' tag: the last run's epoch (1..32767), kept across fills, so that a refilled batch (the
    // per-call path fills the context's scratch batch every call) needs no memset; the buffer is zeroed when it is
    // (re)allocated (d_bnd.gen differs from bnd_zero_gen: a failed and a later successful reserve may return new
    // memory of the old capacity, so the capacity does not tell) and when the epoch wraps
    uint32_t split_epoch = 0;
    uint64_t bnd_zero_gen = 0;
    // band pruning: d_band holds every pair's window, rewritten by sed_band_kernel in every run
    DevBuf d_band;
    // the per-stripe regions of a band-pruned batch (sed_plan: band_stripes): [suffix costs | windows], and the host's
    // copy of the windows for sed_batch_band_chunks_run
    DevBuf d_bwin;
    std::vector<int32_t> h_bwin;
    // cutoff (sed_batch_set_cutoff): every run ends with sed_cut_filter_kernel (results above cut_cmp
    // become +inf; cut_cmp = the cutoff floored to the integer scale in integer mode).  cut_win: the wave pairs
    // (cut_list: every pair not on a lane kernel) leave their routes for the windowed stripe kernel, whose windows
    // sed_cut_band_kernel writes into d_band in every run.  d_cut = [cut_list | diagonal bounds (npairs) | hits (4)];
    // cut_diag = the diagonal bounds, read back once for the host's restatement (band_cells) and the routing rule.
    // band_cells: the cells the forward computes (the plan's, or under the current cutoff).
    bool cut_on = false, cut_win = false, cut_ready = false, cut_prune_ok = false, cut_last = false;
    double cutoff = 0, cut_cmp = 0, band_cells = 0;
    uint32_t cut_key = 0;
    std::vector<int32_t> cut_list;
    std::vector<uint32_t> cut_diag;
    DevBuf d_cut;
    // SED_PIPELINE: run k uses traceback/result buffer k % plan.nbuf and its traceback runs on a second
    // stream, overlapping the DP of run k+1.  Three buffers, so the DP of run k+3 is the first
    // to wait for that traceback: with two, a traceback starved of CUs during the next DP
    // (it only gets them in that DP's tail) delayed the DP after it (~0.7 ms per 27 ms step).
    DevBuf d_tb[3], d_res[3];
    hipStream_t tb_stream = nullptr;
    // Checkpoint batches in parts (plan.nparts): part 0 runs forward then traceback on the
    // context's stream, part i on part_stream[i - 1], so one part's traceback overlaps another part's forward.
    hipStream_t part_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_start = nullptr;
    // per event-log entry: the {dp start, dp end, tb start, tb end} events of parts 1..3 (created on first use)
    std::vector<std::array<hipEvent_t, 12>> plog;
    // per buffer: the event-log entry of the last run that used it (handles copied from `log`)
    std::array<hipEvent_t, 4> evk[3] = {};
    long runs = 0;
    // dynamic-CHAIN launches since the fill per buffer slot: each slot has its own device counter, whose base is
    // slot launches x (list + waves)
    long chain_launches[3] = {0, 0, 0};
    // pipelined batches whose runs share no scratch (plan.alt_dp: dynamic-CHAIN script batches, distance-only batches
    // of lane pairs): odd runs' DP on dp2_stream, so run k+1's kernels fill the tail of run k's (CHAIN: persistent
    // waves; lane kernels: the launch gap).  CHAIN slots have their own counters; a slot's runs are ordered through
    // the wait of buffer reuse (run_batch)
    hipStream_t dp2_stream = nullptr;
    bool ran = false;
    // per-run event log (sed_batch_times): {dp start, dp end, tb start, tb end}
    std::vector<std::array<hipEvent_t, 4>> log;
    size_t nlog = 0;
    long last_log = -1;  // the event-log entry of the last run (its parts' events: plog[last_log])
    std::vector<sed_result> h_res;

    int cur() const { return (int)((runs - 1) % plan.nbuf); }
    ~sed_batch() {
        if (zc_busy) (void)hipStreamSynchronize(ctx->stream);
        if (h_out) (void)hipHostFree(h_out);
        d_pd.release(); d_seqa.release(); d_seqb.release(); d_bnd.release(); d_ops.release(); d_tbmap.release();
        d_tasks.release(); d_lane.release(); d_chain.release(); d_x2.release(); d_small.release(); d_seg.release();
        d_band.release(); d_cut.release(); d_bwin.release();
        for (int i = 0; i < 3; ++i) {
            d_tb[i].release();
            d_res[i].release();
        }
        if (tb_stream) (void)hipStreamDestroy(tb_stream);
        if (dp2_stream) (void)hipStreamDestroy(dp2_stream);
        for (hipStream_t &ps : part_stream)
            if (ps) (void)hipStreamDestroy(ps);
        if (ev_start) (void)hipEventDestroy(ev_start);
        for (auto &a : plog)
            for (hipEvent_t e : a)
                if (e) (void)hipEventDestroy(e);
        for (auto &a : log)
            for (hipEvent_t e : a)
                if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// the next run's SPLIT epoch, zeroing the hand-off words first when no word may carry a tag of its own (see split_epoch)
hipError_t next_split_epoch(sed_batch *b, hipStream_t s, uint32_t *epoch) {
    *epoch = b->split_epoch % 32767u + 1u;
    b->split_epoch = *epoch;
    if (!b->plan.split || b->plan.bnd_words == 0) return hipSuccess;
    if (*epoch == 1 || b->d_bnd.gen != b->bnd_zero_gen) {
        hipError_t e = hipMemsetAsync(b->d_bnd.p, 0, b->d_bnd.cap, s);
        if (e != hipSuccess) return e;
        b->bnd_zero_gen = b->d_bnd.gen;
    }
    return hipSuccess;
}

// Event-log entries {DP start, DP end, traceback start, traceback end}, created ahead of the runs
// that use them (outside any timed loop for up to `more` runs).  Batches in parts also get the parts' entries
// (plog), up to the same count, so no event is created while runs are being timed.
hipError_t grow_log(sed_batch *b, size_t more) {
    for (size_t i = 0; i < more; ++i) {
        std::array<hipEvent_t, 4> a{};
        for (auto &x : a) {
            hipError_t e = hipEventCreate(&x);
            if (e != hipSuccess) return e;
        }
        b->log.push_back(a);
    }
    while (b->plan.nparts > 1 && b->plog.size() < b->log.size()) {
        std::array<hipEvent_t, 12> a{};
        for (auto &x : a) {
            hipError_t e = hipEventCreate(&x);
            if (e != hipSuccess) return e;
        }
        b->plog.push_back(a);
    }
    return hipSuccess;
}

// ---- a fill: wait, plan, reserve, upload, streams ----

// a refill must not overwrite a running part; a fault of the previous run is reported as such
int wait_previous_run(sed_batch *b) {
    sed_ctx *c = b->ctx;
    hipError_t e = hipSuccess;
    for (hipStream_t ps : b->part_stream)
        if (e == hipSuccess && ps) e = hipStreamSynchronize(ps);
    if (e == hipSuccess && b->dp2_stream) e = hipStreamSynchronize(b->dp2_stream);
    if (e == hipSuccess && b->tb_stream) e = hipStreamSynchronize(b->tb_stream);
    // zero-copy runs store into h_out from the context's stream, which a refill memsets (place_host_results)
    if (e == hipSuccess && b->zc_busy) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->hipfail(e, "previous run");
    b->zc_busy = false;
    return SED_OK;
}

// The input arrays of a batch (sed_plan.h: SED_UP_*): where each comes from on the host, its own device buffer (large
// batches), the kernels' pointer to it, and what a failed copy of it is called.  Sizes and blob offsets: the plan's.
struct UploadItem {
    const void *src;
    DevBuf *buf;
    void **slot;
    const char *what;
};
struct UploadTable {
    UploadItem item[SED_UP_COUNT];
    explicit UploadTable(sed_batch *b)
        : item{{b->plan.pd.data(), &b->d_pd, &b->p_pd, "upload descriptors"},
               {b->ha.data(), &b->d_seqa, &b->p_seqa, "upload str1"},
               {b->hb.data(), &b->d_seqb, &b->p_seqb, "upload str2"},
               {b->plan.tasks.data(), &b->d_tasks, &b->p_tasks, "upload tasks"},
               {b->plan.chain.data(), &b->d_chain, &b->p_chain, "upload chains"},
               {b->plan.lane.data(), &b->d_lane, &b->p_lane, "upload lane list"},
               {b->plan.x2.data(), &b->d_x2, &b->p_x2, "upload packed-wave list"},
               {b->plan.seg.data(), &b->d_seg, &b->p_seg, "upload segment list"}} {}
};

int reserve_batch(sed_batch *b) {
    const sed_plan &p = b->plan;
    const bool want_tb = (p.flags & SED_WANT_SCRIPT) != 0;
    bool ok = b->d_bnd.reserve(4 * std::max<uint64_t>(1, p.bnd_words)) &&
              b->d_tbmap.reserve(4 * std::max<uint64_t>(1, p.map_words)) &&
              (!p.band || (b->d_band.reserve(sizeof(sed_band) * (size_t)p.npairs) &&
                           b->d_bwin.reserve(12 * std::max<size_t>(1, (size_t)p.npairs * p.band_stripes))));
    if (p.small) {
        ok = ok && b->d_small.reserve(p.blob_bytes);
    } else {
        const UploadTable t(b);
        ok = ok && b->d_ops.reserve(4 * std::max<uint64_t>(1, p.ops_words));
        for (int i = 0; i < SED_UP_COUNT; ++i) ok = ok && t.item[i].buf->reserve(p.up_size[i]);
        for (int i = 0; i < p.nbuf; ++i) ok = ok && b->d_res[i].reserve(p.res_size);
    }
    for (int i = 0; i < p.nbuf; ++i) ok = ok && (!want_tb || b->d_tb[i].reserve(4 * std::max<uint64_t>(1, p.tb_words)));
    if (!ok)
        return b->ctx->fail(SED_E_OOM, "device allocation failed (traceback %d x %.3f GB)", p.nbuf, 4.0 * p.tb_words / 1e9);
    return SED_OK;
}

// zero-copy results: the batch's pinned block for `bytes` of results and scripts, zeroed (no run of this batch is in
// flight: wait_previous_run waited for zc_busy)
hipError_t place_host_results(sed_batch *b, size_t bytes) {
    if (bytes > b->h_out_cap) {
        if (b->h_out) (void)hipHostFree(b->h_out);
        b->h_out = nullptr;
        b->h_out_cap = 0;
        const size_t cap = std::max<size_t>(bytes, 1u << 16);
        const hipError_t e = hipHostMalloc(&b->h_out, cap, hipHostMallocDefault);
        if (e != hipSuccess) {
            b->h_out = nullptr;
            return e;
        }
        b->h_out_cap = cap;
    }
    memset(b->h_out, 0, bytes);
    return hipSuccess;
}

// Small batches: every input array and the zeroed results go up as one blob from the context's pinned staging buffer,
// with no upload sync (the staging buffer is not rewritten before that copy has completed: pin_busy).  Large ones: one
// pageable copy per array, the results' memsets and a sync.
int upload_batch(sed_batch *b) {
    sed_ctx *c = b->ctx;
    const sed_plan &p = b->plan;
    const UploadTable t(b);
    hipError_t e;
    if (p.small) {
        if ((e = pin_reserve(c, p.blob_bytes)) != hipSuccess) return c->hipfail(e, "pinned staging");
        char *h = (char *)c->pin.p, *d = (char *)b->d_small.p;
        for (int i = 0; i < SED_UP_COUNT; ++i) {
            if (p.up_copy[i]) memcpy(h + p.up_off[i], t.item[i].src, p.up_copy[i]);
            memset(h + p.up_off[i] + p.up_copy[i], 0, p.up_size[i] - p.up_copy[i]);  // (CHAIN: the counters)
            *t.item[i].slot = d + p.up_off[i];
        }
        memset(h + p.o_res, 0, p.res_size);
        // (zero-copy results: the results and scripts stay in h_out)
        if (p.zc && (e = place_host_results(b, p.blob_bytes - p.o_res)) != hipSuccess) return c->hipfail(e, "pinned results");
        if ((e = hipMemcpyAsync(d, h, p.zc ? p.o_res : p.blob_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return c->hipfail(e, "upload");
        c->pin_busy = true;
        b->p_res[0] = p.zc ? b->h_out : d + p.o_res;
        b->p_ops = p.zc ? (char *)b->h_out + (p.o_ops - p.o_res) : d + p.o_ops;
        return SED_OK;
    }
    b->p_ops = b->d_ops.p;
    for (int i = 0; i < 3; ++i) b->p_res[i] = b->d_res[i].p;
    for (int i = 0; i < SED_UP_COUNT; ++i) {
        *t.item[i].slot = t.item[i].buf->p;
        if (p.up_copy[i] && (e = hipMemcpyAsync(t.item[i].buf->p, t.item[i].src, p.up_copy[i], hipMemcpyHostToDevice,
                                                c->stream)) != hipSuccess)
            return c->hipfail(e, t.item[i].what);
    }
    for (int i = 0; i < p.nbuf; ++i)
        if ((e = hipMemsetAsync(b->p_res[i], 0, p.res_size, c->stream)) != hipSuccess) return c->hipfail(e, "zero results");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "upload sync");
    c->pin_busy = false;
    return SED_OK;
}

// the streams and events the plan's runs need (created once, kept across refills)
int make_streams(sed_batch *b) {
    sed_ctx *c = b->ctx;
    const sed_plan &p = b->plan;
    hipError_t e;
    // the event log is reused across refills (sed_run_batch's scratch batch): entries are created
    // only up to 64 ahead of the runs, and run_batch grows it on demand past that; batches in parts: the parts' entries
    b->nlog = 0;
    b->last_log = -1;
    if ((e = grow_log(b, b->log.size() < 64 ? 64 - b->log.size() : 0)) != hipSuccess) return c->hipfail(e, "event create");
    if (p.nbuf > 1 && !b->tb_stream &&
        (e = hipStreamCreateWithFlags(&b->tb_stream, hipStreamNonBlocking)) != hipSuccess)
        return c->hipfail(e, "traceback stream");
    if (p.alt_dp && !b->dp2_stream && (e = hipStreamCreateWithFlags(&b->dp2_stream, hipStreamNonBlocking)) != hipSuccess)
        return c->hipfail(e, "second DP stream");
    for (int i = 0; i + 1 < p.nparts; ++i)
        if (!b->part_stream[i] && (e = hipStreamCreateWithFlags(&b->part_stream[i], hipStreamNonBlocking)) != hipSuccess)
            return c->hipfail(e, "part stream");
    if (p.nparts > 1 && !b->ev_start && (e = hipEventCreateWithFlags(&b->ev_start, hipEventDisableTiming)) != hipSuccess)
        return c->hipfail(e, "event create");
    return SED_OK;
}

// The cutoff state, and the launches of a run under it.  The schedule is rebuilt where its inputs change (a fill, a
// cutoff) and nowhere else: a run only reads it.
void set_cut_state(sed_batch *b, bool on, bool win) {
    b->cut_on = on;
    b->cut_win = win;
    b->sched = sed_plan_run(b->plan, on, win);
}

int fill_batch(sed_batch *b, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
               const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, int32_t npairs,
               uint32_t flags) {
    sed_ctx *c = b->ctx;
    if (!c->have_costs) return c->fail(SED_E_STATE, "sed_set_costs() was not called");
    int rc = wait_previous_run(b);
    if (rc != SED_OK) return rc;
    rc = sed_plan_batch(c->costs, c->opt, codes_a, off_a, len_a, codes_b, off_b, len_b, npairs, flags, &b->plan, &c->err);
    if (rc != SED_OK) return rc;
    b->ran = false;
    b->runs = 0;
    b->cut_ready = b->cut_last = false;
    set_cut_state(b, false, false);  // (a refill starts without a cutoff)
    b->band_cells = b->plan.band_cells;
    b->chain_launches[0] = b->chain_launches[1] = b->chain_launches[2] = 0;
    if ((rc = reserve_batch(b)) != SED_OK) return rc;
    sed_pack_sequences(b->plan, codes_a, off_a, len_a, codes_b, off_b, len_b, b->ha, b->hb);
    if ((rc = upload_batch(b)) != SED_OK) return rc;
    return make_streams(b);
}

// SED_OPT_DEBUG_CORRUPT: overwrite the column checkpoint of the sink's row in the chunk before the
// sink's tile with the smallest distance key (D offset 0, no updates), which the recompute then
// spreads to the sink (test of the traceback's error path: the pair must come back SED_E_DEVICE).
// tb: the run's checkpoints; `s`: the stream that pair's traceback follows.
hipError_t debug_corrupt(const sed_batch *b, uint32_t *tb, hipStream_t s) {
    const sed_pair_desc &d = b->plan.pd[b->ctx->opt.debug_corrupt - 1];
    const int R = b->plan.R, ROWS = R * 64;
    if (d.lane || d.n <= 0 || d.m <= 0) return hipSuccess;
    const sed_geom g = sed_stripe_geom(d.n, d.m, R, 64);
    const int t = ((d.n - 1) % ROWS) / R, r = (d.n - 1) % R, cs = (d.m - 1 + t) >> 6;
    if (cs < 1) return hipSuccess;
    uint32_t *w = tb + d.tb_off + sed_ck_col_word(R, g.nstripes - 1, g.nchunks, cs - 1, r, t);
    // (dot keys are maximised: the largest key there instead)
    return hipMemsetD32Async((hipDeviceptr_t)w, b->plan.dot ? 0x3FFFFFFFu : 0x0000FFFCu, 1, s);
}
bool debug_corrupt_on(const sed_batch *b) {
    return b->ctx->opt.debug_corrupt > 0 && b->ctx->opt.debug_corrupt <= b->plan.npairs;
}

// One run: the planner's schedule (b->sched; sed_plan.h: sed_plan_run), step by step.  Which launcher runs when, on
// which stream role, and which launch carries which event is decided there; here a step gets its pairs, its stream,
// its events and its launcher's arguments.
//
// The event log's timestamps ride on the kernels' own dispatch packets (SED_LAUNCH): the first launch of a phase records
// the phase's start event at its start and the last one its end event at its end.  An event record is a marker packet
// on the queue: with records around the kernels, consecutive config-2 DP kernels were ~18 us apart, and for the
// ~25 us lane kernel (config 5) every avoided packet is measurable.  A phase that launches nothing records its events
// directly.
//
// A checkpoint batch in parts (sched.nparts): stream i runs forward(part i) then traceback(part i).  The other streams
// start each run after stream 0's previous work, and nothing joins the streams at a run's end, so the parts settle
// into a stagger: one part's traceback runs beside another part's forward (config 4: 11.42-11.47 ms in one part,
// 10.85-11.0 in two, 10.77-10.83 in three, 11.6-11.8 in four; with the select-free hold 9.86-9.93 in two against
// 10.30-10.54 in three, profiles/r03/parts2/; joined at every run's end two halves ran in lockstep and gained nothing;
// profiles/r03/halves/, parts/).  The parts share no buffer region (every pair has its own checkpoints, bottom rows,
// script words and result), and sync_batch waits for every stream.  Part 0's events are the run's own log entry,
// parts 1..3's are plog's: sed_batch_times reports the mean launch (sed_batch_dp_launches() = nparts).
int run_batch(sed_batch *b) {
    sed_ctx *c = b->ctx;
    const sed_plan &p = b->plan;
    const sed_run_plan &S = b->sched;
    if (p.npairs == 0) {
        b->ran = true;
        ++b->runs;
        return SED_OK;
    }
    const int k = (int)(b->runs % p.nbuf);
    const bool want_tb = (p.flags & SED_WANT_SCRIPT) != 0;
    hipError_t e;
    if (p.zc) b->zc_busy = true;
    // The run's events time it (sed_batch_times) and, when buffers rotate, order their reuse (evk below; S.need_ev).
    // Untimed runs (sed_batch_set_timing) launch without them.
    const bool timed = S.need_ev || b->time_every == 1 || (b->time_every > 1 && b->runs % b->time_every == 0);
    std::array<hipEvent_t, 4> lg{};   // part 0's {DP start, DP end, traceback start, traceback end}
    std::array<hipEvent_t, 12> pl{};  // parts 1..3's (grow_log created them with the run's own)
    if (timed) {
        if (b->nlog == b->log.size() && (e = grow_log(b, 64)) != hipSuccess) return c->hipfail(e, "event create");
        b->last_log = (long)b->nlog;
        lg = b->log[b->nlog++];
        if (S.nparts > 1) {
            if (b->plog.size() <= (size_t)b->last_log) return c->fail(SED_E_STATE, "parts event log not grown");
            pl = b->plog[b->last_log];
        }
    }
    const hipStream_t ds = p.alt_dp && (b->runs & 1) ? b->dp2_stream : c->stream;  // this run's DP stream
    const hipStream_t ts = p.nbuf > 1 ? b->tb_stream : c->stream;
    auto part_stream = [&](int i) { return i == 0 ? c->stream : b->part_stream[i - 1]; };
    auto part_first = [&](int i) { return (int)((int64_t)p.npairs * i / S.nparts); };
    sed_launch L{};
    L.pd = (const sed_pair_desc *)b->p_pd;
    L.npairs = p.npairs;
    L.seqa = b->p_seqa;
    L.seqb = b->p_seqb;
    L.tb = want_tb ? (uint32_t *)b->d_tb[k].p : nullptr;
    L.ops = (uint32_t *)b->p_ops;
    L.bnd = (uint32_t *)b->d_bnd.p;
    L.res = (sed_result *)b->p_res[k];
    L.R = p.R;
    L.tb_ladder = p.mode == SED_MODE_I32 && !p.split_ck;  // (split_ck codes are the plain ops)
    L.tb_wide = p.lad && p.ip.lad == 2;  // (a ladder-dot batch is a CHAIN batch: every wave pair's codes come from the LDOT kernel)
    L.ck = p.ck;
    L.band = p.band ? (sed_band *)b->d_band.p : nullptr;
    L.bandp = &p.bandp;
    if (L.band && p.band_stripes > 0) {
        const size_t per = (size_t)p.npairs * p.band_stripes;
        L.bstripes = p.band_stripes;
        L.bsuf = p.band_refine ? (uint32_t *)b->d_bwin.p : nullptr;
        L.bwin = (int2 *)((uint32_t *)b->d_bwin.p + per);
    }
    L.tasks = p.split ? (const int2 *)b->p_tasks : nullptr;
    L.ntasks = p.split ? p.ntasks : 0;
    // buffer k was last read by the traceback of run runs-3 (written by its DP, distance only): wait for it unless it
    // has finished already (a cross-queue wait is a barrier packet between this run's kernel and the previous one)
    if (S.reuse != SED_REUSE_NONE && b->runs >= p.nbuf && hipEventQuery(b->evk[k][S.reuse]) != hipSuccess &&
        (e = hipStreamWaitEvent(ds, b->evk[k][S.reuse], 0)) != hipSuccess)
        return c->hipfail(e, "stream wait");
    uint32_t *const hits = S.cut ? (uint32_t *)b->d_cut.p + b->cut_list.size() + (size_t)p.npairs + k : nullptr;
    if (S.cut && (e = hipMemsetAsync(hits, 0, 4, ds)) != hipSuccess) return c->hipfail(e, "reset cutoff hits");
    b->cut_last = S.cut;
    // SPLIT hand-off words carry the run's epoch (1..32767, next_split_epoch); every kernel writes all result
    // fields, err included
    sed_i32_params ip = p.ip;
    if ((e = next_split_epoch(b, ds, &ip.epoch)) != hipSuccess) return c->hipfail(e, "memset hand-off words");
    const bool len = want_tb || !(p.flags & SED_NO_LEN);
    if (S.nparts > 1) {  // the other parts' streams start after everything queued before this run (uploads, the previous run's part 0)
        if ((e = hipEventRecord(b->ev_start, c->stream)) != hipSuccess) return c->hipfail(e, "stream fork");
        for (int i = 1; i < S.nparts; ++i)
            if ((e = hipStreamWaitEvent(part_stream(i), b->ev_start, 0)) != hipSuccess) return c->hipfail(e, "stream fork");
    }
    auto launch = [&](const sed_step &st) {
        sed_launch Li = L;
        Li.stream = st.on == SED_ON_PART ? part_stream(st.part) : st.on == SED_ON_TB ? ts : ds;
        const int ev = 2 * st.phase;
        Li.ev0 = !st.first ? nullptr : st.part == 0 ? lg[ev] : pl[4 * (st.part - 1) + ev];
        Li.ev1 = !st.last ? nullptr : st.part == 0 ? lg[ev + 1] : pl[4 * (st.part - 1) + ev + 1];
        if (S.nparts > 1 && st.kind != SED_STEP_LANE) {  // the part's pairs (the lane list indexes the whole batch's)
            const int p0 = part_first(st.part);
            Li.pd += p0;
            Li.res += p0;
            if (Li.band) Li.band += p0;
            if (Li.bwin) Li.bwin += (size_t)p0 * L.bstripes;
            if (Li.bsuf) Li.bsuf += (size_t)p0 * L.bstripes;
            Li.npairs = part_first(st.part + 1) - p0;
        }
        uint32_t *const ops = (uint32_t *)b->p_ops;
        const double *const gtab = (const double *)c->gtab.p;
        const int32_t *const lane = (const int32_t *)b->p_lane;
        const bool typed = p.mode == SED_MODE_F64_TYPED;
        const char *what = st.phase == SED_PHASE_DP ? "DP kernel launch" : "traceback kernel launch";
        hipError_t le = hipSuccess;
        switch (st.kind) {
        case SED_STEP_WIN:
            what = "windowed DP kernel launch";
            Li.band = (sed_band *)b->d_band.p;
            Li.bandp = &p.cut_bp;
            le = sed_launch_i32_cut(Li, (const int32_t *)b->d_cut.p, (int)b->cut_list.size(), ip, b->cut_key);
            break;
        case SED_STEP_X2:
            what = "packed DP kernel launch";
            le = sed_launch_i32x2(Li, (const int32_t *)b->p_x2, p.nwave_x2, ip);
            break;
        case SED_STEP_CHAIN:
            Li.chain_pairs = (const int32_t *)b->p_chain;
            Li.chain_off = (const int32_t *)b->p_chain + p.chain_npairs;
            Li.nchains = p.nchains;
            Li.chain_list = (int)p.chain_npairs;
            if (p.chain_dyn) {  // zeroed on a batch's first launch only: a launch takes list + waves values
                // (counted per launch, not per run: a run that fails after its CHAIN launch has still advanced it)
                Li.chain_counter = (uint32_t *)b->p_chain + p.chain_npairs + 1 + k;
                Li.chain_base = (uint32_t)((uint64_t)b->chain_launches[k] * (uint64_t)(p.chain_npairs + p.nchains));
                what = "reset chain counter";
                if (b->chain_launches[k] == 0 && (le = hipMemsetAsync(Li.chain_counter, 0, 4, Li.stream)) != hipSuccess) break;
                what = "DP kernel launch";
            }
            le = sed_launch_i32_chain(Li, ip, len);
            if (le == hipSuccess && p.chain_dyn) ++b->chain_launches[k];
            break;
        case SED_STEP_I32:
            Li.ck = p.ck || p.split_ck;  // (a split_ck batch's forward stores checkpoints for the codes kernel)
            le = sed_launch_i32(Li, ip, len);
            break;
        case SED_STEP_CODES:  // the tile codes of this run's checkpoints
            if (st.phase == SED_PHASE_TB) what = "codes kernel launch";
            le = sed_launch_ck_codes(Li, p.ck_tiles, ip);
            break;
        case SED_STEP_F64: {
            sed_f64_params fp = p.fp;
            fp.epoch = ip.epoch;
            le = sed_launch_f64(Li, gtab, fp, typed);
            break;
        }
        case SED_STEP_F64_SEG:  // fp64 pairs in 16-lane segments, four per wave
            what = "segment DP kernel launch";
            le = sed_launch_f64_seg(Li, gtab, p.fp, typed, (const int32_t *)b->p_seg, p.nseg);
            break;
        case SED_STEP_LANE:
            what = "lane kernel launch";
            if (p.lane_bitpar)
                le = sed_launch_lane_bitpar(Li, lane, p.nlane);
            else if (p.nlane_x2 > 0)
                le = sed_launch_lane_i32x2(Li, lane, p.nlane_x2, ip);
            else if (p.mode == SED_MODE_I32)
                le = sed_launch_lane_i32(Li, lane, p.nlane, ip, len);
            else if (p.scaled)
                le = sed_launch_lane_scaled(Li, lane, p.nlane, p.sp);
            else
                le = sed_launch_lane_f64(Li, lane, p.nlane, gtab, c->costs.ins, c->costs.del, c->costs.K, p.umask);
            break;
        case SED_STEP_FILTER:
            what = "cutoff filter launch";
            le = sed_launch_cut_filter(Li, b->cut_cmp, hits);
            break;
        case SED_STEP_TB_CK: le = sed_launch_traceback_ck(Li, ops, ip); break;
        case SED_STEP_TB_CODES: le = sed_launch_traceback(Li, ops); break;
        case SED_STEP_TB_STRIPES:
            le = sed_launch_traceback_stripes(Li, ops, (uint32_t *)b->d_tbmap.p, p.tbpar_items, p.tbpar_kmax);
            break;
        case SED_STEP_TB_SEG: le = sed_launch_traceback_seg(Li, ops, (const int32_t *)b->p_seg, p.nseg); break;
        default: return c->fail(SED_E_STATE, "unknown step %d in the run's schedule", (int)st.kind);
        }
        return le == hipSuccess ? SED_OK : c->hipfail(le, what);
    };
    int i = 0, rc;
    for (; i < S.n && S.step[i].phase == SED_PHASE_DP; ++i)
        if ((rc = launch(S.step[i])) != SED_OK) return rc;
    if (i == 0 && lg[0] && ((e = hipEventRecord(lg[0], ds)) != hipSuccess || (e = hipEventRecord(lg[1], ds)) != hipSuccess))
        return c->hipfail(e, "event record");
    if (S.tb) {
        if (p.ck && debug_corrupt_on(b)) {  // on the stream of the part that holds the pair
            int part = 0;
            while (part + 1 < S.nparts && c->opt.debug_corrupt - 1 >= part_first(part + 1)) ++part;
            if ((e = debug_corrupt(b, L.tb, S.nparts > 1 ? part_stream(part) : ds)) != hipSuccess)
                return c->hipfail(e, "debug corrupt");
        }
        if (ts != ds && (e = hipStreamWaitEvent(ts, lg[1], 0)) != hipSuccess) return c->hipfail(e, "stream wait");
        if (i == S.n && lg[2] && ((e = hipEventRecord(lg[2], ts)) != hipSuccess || (e = hipEventRecord(lg[3], ts)) != hipSuccess))
            return c->hipfail(e, "event record");
        for (; i < S.n; ++i)
            if ((rc = launch(S.step[i])) != SED_OK) return rc;
    }
    b->evk[k] = lg;
    ++b->runs;
    b->ran = true;
    return SED_OK;
}

int sync_batch(sed_batch *b) {
    sed_ctx *c = b->ctx;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && b->tb_stream) e = hipStreamSynchronize(b->tb_stream);
    if (e == hipSuccess && b->dp2_stream) e = hipStreamSynchronize(b->dp2_stream);
    for (hipStream_t ps : b->part_stream)
        if (e == hipSuccess && ps) e = hipStreamSynchronize(ps);
    if (e == hipSuccess) b->zc_busy = false;
    return e == hipSuccess ? SED_OK : c->hipfail(e, "kernel execution");
}

int fetch_results(sed_batch *b, double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops,
                  const int64_t *ops_off) {
    sed_ctx *c = b->ctx;
    if (!b->ran) return c->fail(SED_E_STATE, "batch has not been run");
    const int np = b->plan.npairs;
    hipError_t e;
    const bool want_ops = out_ops && ops_off && (b->plan.flags & SED_WANT_SCRIPT) && np;
    const sed_result *hr = nullptr;
    const uint32_t *hops = nullptr;
    std::vector<uint32_t> h;
    if (b->plan.small && b->plan.nbuf == 1 && b->plan.nparts == 1 && !b->plan.alt_dp) {
        // every kernel ran on the context's stream: one download of the adjacent results and scripts into the pinned
        // staging, ordered after them, and one wait
        const size_t bytes = (b->plan.o_ops - b->plan.o_res) + (want_ops ? 4 * b->plan.ops_words : 0);
        const char *src = (const char *)b->h_out;
        if (!b->plan.zc) {
            if (bytes > c->pin.cap && (e = pin_reserve(c, bytes)) != hipSuccess) return c->hipfail(e, "pinned staging");
            if (np && (e = hipMemcpyAsync(c->pin.p, b->p_res[0], bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
                return c->hipfail(e, "download results");
            c->pin_busy = true;
            src = (const char *)c->pin.p;
        }
        int rc = sync_batch(b);
        if (rc != SED_OK) return rc;
        c->pin_busy = false;
        hr = (const sed_result *)src;
        hops = (const uint32_t *)(src + (b->plan.o_ops - b->plan.o_res));
    } else {
        int rc = sync_batch(b);
        if (rc != SED_OK) return rc;
        b->h_res.resize(np);
        if (np && (e = hipMemcpy(b->h_res.data(), b->p_res[b->cur()], sizeof(sed_result) * np, hipMemcpyDeviceToHost)) !=
                      hipSuccess)
            return c->hipfail(e, "download results");
        hr = b->h_res.data();
        if (want_ops) {
            h.resize(b->plan.ops_words);
            if ((e = hipMemcpy(h.data(), b->p_ops, 4 * b->plan.ops_words, hipMemcpyDeviceToHost)) != hipSuccess)
                return c->hipfail(e, "download scripts");
            hops = h.data();
        }
    }
    for (int p = 0; p < np; ++p) {
        switch (hr[p].err) {
        case 0: break;
        case SED_ERR_SPLIT_TIMEOUT: return c->fail(SED_E_DEVICE, "pair %d: inter-workgroup hand-off timed out", p);
        case SED_ERR_TB_CHECK:
            return c->fail(SED_E_DEVICE, "pair %d: traceback failed: a recomputed tile contradicts the path length "
                                         "(corrupt checkpoint)", p);
        case SED_ERR_TB_STALL: return c->fail(SED_E_DEVICE, "pair %d: traceback failed: a tile made no progress", p);
        case SED_ERR_TB_GUARD: return c->fail(SED_E_DEVICE, "pair %d: traceback failed: too many tile visits", p);
        case SED_ERR_TB_LENGTH:
            return c->fail(SED_E_DEVICE, "pair %d: traceback failed: script length differs from the sink's", p);
        case SED_ERR_TB_BAND:
            return c->fail(SED_E_DEVICE, "pair %d: traceback failed: the walk left the band the forward computed", p);
        case SED_ERR_FWD_BAND:
            return c->fail(SED_E_DEVICE, "pair %d: forward failed: no cell of a stripe's boundary row fits the bound", p);
        default: return c->fail(SED_E_DEVICE, "pair %d: device error code %d", p, (int)hr[p].err);
        }
    }
    for (int p = 0; p < np; ++p) {
        if (out_dist) out_dist[p] = hr[p].dist;
        if (out_is_int) out_is_int[p] = hr[p].is_int;
        if (out_len) out_len[p] = hr[p].len;
    }
    if (want_ops)
        for (int p = 0; p < np; ++p) {
            const uint64_t words = (uint64_t)(b->plan.pd[p].n + b->plan.pd[p].m + 15) / 16;
            memcpy(out_ops + ops_off[p], hops + b->plan.pd[p].ops_off, 4 * words);
        }
    return SED_OK;
}

}  // namespace

extern "C" {

const char *sed_version(void) { return "libsed 0.1 (gfx950)"; }

sed_ctx *sed_create(int device) {
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    sed_ctx *c = new sed_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        return nullptr;
    }
    return c;
}

void sed_destroy(sed_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c->scratch;
    c->pin.release();
    c->gtab.release();
    c->selftest.release();
    sed_fit_state_destroy(c->fit);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *sed_last_error(const sed_ctx *c) { return c ? c->err.c_str() : "null context"; }

int sed_set_option(sed_ctx *c, int key, int value) {
    if (!c) return SED_E_ARG;
    return sed_opts_set(c->opt, key, value, false) ? SED_OK : c->fail(SED_E_ARG, "bad option %d=%d", key, value);
}

int sed_set_costs(sed_ctx *c, int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int,
                  double del, int del_is_int) {
    if (!c) return SED_E_ARG;
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (K < 1 || K > 255 || !sub || !sub_int) return c->fail(SED_E_ARG, "bad cost table (K=%d)", K);
    if (!std::isfinite(ins) || !std::isfinite(del)) return c->fail(SED_E_ARG, "non-finite insert/delete cost");
    for (int e = 0; e < K * K; ++e)
        if (!std::isfinite(sub[e])) return c->fail(SED_E_ARG, "non-finite update cost at %d", e);
    (void)hipSetDevice(c->device);
    c->costs.K = K;
    c->costs.sub.assign(sub, sub + K * K);
    c->costs.sub_int.assign(sub_int, sub_int + K * K);
    c->costs.ins = ins;
    c->costs.del = del;
    c->costs.ins_int = ins_is_int ? 1 : 0;
    c->costs.del_int = del_is_int ? 1 : 0;
    if (K <= SED_MAX_K) {
        std::vector<uint64_t> t(2 * K * K);
        for (int e = 0; e < K * K; ++e) {
            memcpy(&t[2 * e], &sub[e], 8);
            t[2 * e + 1] = sub_int[e] ? 1 : 0;
        }
        if (!c->gtab.reserve(t.size() * 8)) return c->fail(SED_E_OOM, "cost table allocation");
        hipError_t e = hipMemcpy(c->gtab.p, t.data(), t.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return c->hipfail(e, "upload cost table");
    }
    c->have_costs = true;
    return SED_OK;
}

sed_batch *sed_batch_create(sed_ctx *c, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                            const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, int32_t npairs,
                            uint32_t flags) {
    if (!c) return nullptr;
    (void)hipSetDevice(c->device);
    sed_batch *b = new sed_batch();
    b->ctx = c;
    if (fill_batch(b, codes_a, off_a, len_a, codes_b, off_b, len_b, npairs, flags) != SED_OK) {
        delete b;
        return nullptr;
    }
    return b;
}

void sed_batch_destroy(sed_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    delete b;
}

int sed_batch_mode(const sed_batch *b) { return b ? b->plan.mode : SED_E_ARG; }
int sed_batch_rows_per_lane(const sed_batch *b) { return b ? b->plan.R : SED_E_ARG; }
int sed_batch_lane_pairs(const sed_batch *b) { return b ? b->plan.nlane : SED_E_ARG; }
int sed_batch_chains(const sed_batch *b) { return b ? sed_plan_chains(b->plan, b->cut_on && b->cut_win) : SED_E_ARG; }
int sed_batch_traceback_mode(const sed_batch *b) { return b ? sed_plan_traceback_mode(b->plan) : 0; }

double sed_batch_band_cells(const sed_batch *b) { return b ? b->band_cells : 0.0; }

double sed_batch_band_chunks_run(sed_batch *b, double *total) {
    if (!b || !b->plan.band || !b->ran || b->plan.band_stripes <= 0) return -1.0;
    sed_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (sync_batch(b) != SED_OK) return -1.0;
    const size_t per = (size_t)b->plan.npairs * b->plan.band_stripes;
    b->h_bwin.resize(2 * per);
    if (hipMemcpy(b->h_bwin.data(), (const uint32_t *)b->d_bwin.p + per, 8 * per, hipMemcpyDeviceToHost) != hipSuccess) {
        c->fail(SED_E_DEVICE, "download the stripes' windows");
        return -1.0;
    }
    double run = 0, all = 0;
    for (int p = 0; p < b->plan.npairs; ++p) {
        const sed_pair_desc &d = b->plan.pd[p];
        if (d.lane || d.n <= 0 || d.m <= 0) continue;
        const sed_geom g = sed_stripe_geom(d.n, d.m, b->plan.R, 64);
        for (int k = 0; k < g.nstripes; ++k) {
            const int32_t *w = &b->h_bwin[2 * ((size_t)p * b->plan.band_stripes + k)];
            run += (double)(w[1] - w[0] + 1);
        }
        all += (double)g.nstripes * g.nchunks;
    }
    if (total) *total = all;
    return run;
}

int sed_batch_set_cutoff(sed_batch *b, double max_dist) {
    if (!b) return SED_E_ARG;
    sed_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (!(max_dist >= 0)) return c->fail(SED_E_ARG, "cutoff must be >= 0 (or +inf for none)");
    if (b->plan.flags & SED_WANT_SCRIPT) return c->fail(SED_E_ARG, "a script batch takes no cutoff");
    int rc = sync_batch(b);  // a run in flight reads the windows and the cutoff's pair list
    if (rc != SED_OK) return rc;
    if (std::isinf(max_dist)) {
        set_cut_state(b, false, false);
        b->band_cells = b->plan.cells;
        return SED_OK;
    }
    hipError_t e;
    const int np = b->plan.npairs;
    if (!b->cut_ready) {  // once per fill: the pair list, the windows' buffer and the diagonal bounds (no input upload)
        b->cut_list.clear();
        for (int p = 0; p < np; ++p)
            if (b->plan.pd[p].lane != 1) b->cut_list.push_back(p);
        b->cut_prune_ok = sed_plan_cut_window_ok(b->plan);
        const size_t nl = b->cut_list.size();
        if (!b->d_cut.reserve(4 * (nl + (size_t)np + 4)) || (b->cut_prune_ok && !b->d_band.reserve(sizeof(sed_band) * (size_t)np)))
            return c->fail(SED_E_OOM, "device allocation failed (cutoff)");
        b->cut_diag.assign(np, 0xFFFFFFFFu);
        if (b->cut_prune_ok) {
            const sed_band_params bp = b->plan.cut_bp;
            sed_launch L{};
            L.pd = (const sed_pair_desc *)b->p_pd;
            L.npairs = np;
            L.seqa = b->p_seqa;
            L.seqb = b->p_seqb;
            L.band = (sed_band *)b->d_band.p;
            L.stream = c->stream;
            uint32_t *ddiag = (uint32_t *)b->d_cut.p + nl;
            if ((e = hipMemcpyAsync(b->d_cut.p, b->cut_list.data(), 4 * nl, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
                return c->hipfail(e, "upload cutoff pair list");
            if ((e = hipMemsetAsync(ddiag, 0xFF, 4 * (size_t)np, c->stream)) != hipSuccess ||
                (e = sed_launch_cut_band(L, (const int32_t *)b->d_cut.p, (int)nl, ddiag, bp, 0xFFFFu)) != hipSuccess ||
                (e = hipMemcpyAsync(b->cut_diag.data(), ddiag, 4 * (size_t)np, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                (e = hipStreamSynchronize(c->stream)) != hipSuccess)
                return c->hipfail(e, "diagonal bounds");
        }
        b->cut_ready = true;
    }
    b->cutoff = max_dist;
    if (b->plan.mode == SED_MODE_I32) {  // the integer scale: every distance is an integer below 2^16
        b->cut_cmp = std::floor(std::min(max_dist, 65535.0));
        b->cut_key = (uint32_t)b->cut_cmp;
    } else {
        b->cut_cmp = max_dist;
        b->cut_key = 0;
    }
    bool win = false;
    b->band_cells = b->plan.cells;
    if (b->cut_prune_ok && c->opt.cut != 2) {
        double nominal = 0, bc = 0;
        for (int32_t p : b->cut_list) {
            const int nn = b->plan.pd[p].n, mm = b->plan.pd[p].m;
            if (nn <= 0 || mm <= 0) continue;
            nominal += (double)nn * mm;
            const uint64_t gap = mm > nn ? (uint64_t)(mm - nn) * b->plan.cut_bp.ins : (uint64_t)(nn - mm) * b->plan.cut_bp.del;
            if (gap > b->cut_key) continue;  // runs no stripe
            bc += sed_band_pair_cells(nn, mm, b->plan.R, sed_band_window(nn, mm, b->plan.cut_bp.ins, b->plan.cut_bp.del,
                                                                    std::min<uint64_t>(b->cut_key, b->cut_diag[p])));
        }
        // x2 runs 4 VALU per 2 cells and CHAIN saves its pairs' ramps; the windowed kernel's cell costs 3 VALU
        // (SED_CUT_SHARE: DESIGN.md 3.6d); pairs already on the plain stripe kernel gain whatever the window skips
        const double share = (b->plan.nwave_x2 > 0 || b->plan.nchains > 0) ? SED_CUT_SHARE : 1.0;
        win = c->opt.cut == 1 || bc < share * nominal;
        if (win) b->band_cells = b->plan.cells - nominal + bc;
    }
    set_cut_state(b, true, win);
    return SED_OK;
}

int sed_batch_cutoff_hits(sed_batch *b, int32_t *within) {
    if (!b || !within) return SED_E_ARG;
    sed_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (!b->ran) return c->fail(SED_E_STATE, "batch has not been run");
    int rc = sync_batch(b);
    if (rc != SED_OK) return rc;
    uint32_t h = (uint32_t)b->plan.npairs;  // (a run without a cutoff: every pair is within +inf)
    if (b->cut_last && b->plan.npairs > 0) {
        const hipError_t e = hipMemcpy(&h, (uint32_t *)b->d_cut.p + b->cut_list.size() + (size_t)b->plan.npairs + b->cur(), 4,
                                       hipMemcpyDeviceToHost);
        if (e != hipSuccess) return c->hipfail(e, "download cutoff hits");
    }
    *within = (int32_t)h;
    return SED_OK;
}

int sed_batch_dot_keys(const sed_batch *b) { return b ? sed_plan_dot_keys(b->plan) : SED_E_ARG; }

int sed_batch_chain_stats(sed_batch *b, int32_t *fetched, int32_t *max_per_wave) {
    if (!b) return SED_E_ARG;
    sed_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (!b->ran) return c->fail(SED_E_STATE, "batch has not been run");
    int rc = sync_batch(b);
    if (rc != SED_OK) return rc;
    int32_t f = 0, mx = 0;
    if (b->plan.nchains > 0 && b->plan.npairs > 0) {
        hipError_t e;
        const int kk = (int)((b->runs + b->plan.nbuf - 1) % b->plan.nbuf);  // the last run's slot
        if (b->plan.chain_dyn && b->chain_launches[kk] > 0) {  // every persistent wave ends with one failed grab: a run takes list + waves
            uint32_t cnt = 0;
            if ((e = hipMemcpy(&cnt, (uint32_t *)b->p_chain + b->plan.chain_npairs + 1 + kk, 4, hipMemcpyDeviceToHost)) !=
                hipSuccess)
                return c->hipfail(e, "download chain counter");
            const uint32_t base =
                (uint32_t)((uint64_t)(b->chain_launches[kk] - 1) * (uint64_t)(b->plan.chain_npairs + b->plan.nchains));
            f = (int32_t)(cnt - base) - b->plan.nchains;
        }
        std::vector<sed_result> h(b->plan.npairs);
        if ((e = hipMemcpy(h.data(), b->p_res[b->cur()], sizeof(sed_result) * b->plan.npairs, hipMemcpyDeviceToHost)) !=
            hipSuccess)
            return c->hipfail(e, "download results");
        for (int p = 0; p < b->plan.npairs; ++p)
            if (!b->plan.pd[p].lane && b->plan.pd[p].n > 0 && b->plan.pd[p].m > 0) mx = std::max(mx, (int32_t)h[p].seq + 1);
    }
    if (fetched) *fetched = f;
    if (max_per_wave) *max_per_wave = mx;
    return SED_OK;
}

int sed_batch_bitpar_pairs(const sed_batch *b) { return b ? sed_plan_bitpar_pairs(b->plan) : SED_E_ARG; }

int sed_batch_segment_pairs(const sed_batch *b) { return b ? b->plan.nseg : SED_E_ARG; }

int sed_batch_split_tasks(const sed_batch *b) { return b ? sed_plan_split_tasks(b->plan) : SED_E_ARG; }

int sed_batch_scaled_pairs(const sed_batch *b) { return b ? sed_plan_scaled_pairs(b->plan) : SED_E_ARG; }

int sed_batch_packed_pairs(const sed_batch *b) {
    return b ? sed_plan_packed_pairs(b->plan, b->cut_on && b->cut_win) : SED_E_ARG;
}

int sed_batch_run(sed_batch *b) {
    if (!b) return SED_E_ARG;
    (void)hipSetDevice(b->ctx->device);
    return run_batch(b);
}

int sed_batch_sync(sed_batch *b) {
    if (!b) return SED_E_ARG;
    return sync_batch(b);
}

int sed_batch_last_times(const sed_batch *b, float *dp_ms, float *tb_ms) {
    if (!b || !b->ran) return SED_E_STATE;
    float a = 0, t = 0;
    const bool script = (b->plan.flags & SED_WANT_SCRIPT) != 0;
    if (b->plan.npairs) {
        const std::array<hipEvent_t, 4> &ev = b->evk[b->cur()];
        if (!ev[0]) return SED_E_STATE;  // the last run was not timed (sed_batch_set_timing)
        if (hipEventElapsedTime(&a, ev[0], ev[1]) != hipSuccess) return SED_E_DEVICE;
        if (script && hipEventElapsedTime(&t, ev[2], ev[3]) != hipSuccess) return SED_E_DEVICE;
        if (b->plan.nparts > 1 && b->last_log >= 0 && (size_t)b->last_log < b->plog.size()) {  // the mean over the parts
            const std::array<hipEvent_t, 12> &pl = b->plog[b->last_log];
            for (int p = 1; p < b->plan.nparts; ++p) {
                float ap = 0, tp = 0;
                if (hipEventElapsedTime(&ap, pl[4 * (p - 1)], pl[4 * (p - 1) + 1]) != hipSuccess ||
                    (script && hipEventElapsedTime(&tp, pl[4 * (p - 1) + 2], pl[4 * (p - 1) + 3]) != hipSuccess))
                    return SED_E_DEVICE;
                a += ap;
                t += tp;
            }
            a /= b->plan.nparts;
            t /= b->plan.nparts;
        }
    }
    if (dp_ms) *dp_ms = a;
    if (tb_ms) *tb_ms = t;
    return SED_OK;
}

int sed_batch_spans(sed_batch *b, float *out, int max_runs) {
    if (!b || (!out && max_runs > 0)) return SED_E_ARG;
    int rc = sync_batch(b);
    if (rc != SED_OK) return rc;
    const int cnt = (int)std::min<size_t>(b->nlog, (size_t)std::max(0, max_runs));
    const bool script = (b->plan.flags & SED_WANT_SCRIPT) != 0;
    const int P = b->plan.nparts;
    for (int i = 0; i < cnt; ++i)
        for (int p = 0; p < P; ++p)
            for (int k = 0; k < 4; ++k) {
                float t = 0;
                if (k < 2 || script) {
                    const hipEvent_t ev = p == 0 ? b->log[i][k] : b->plog[i][4 * (p - 1) + k];
                    if (hipEventElapsedTime(&t, b->log[0][0], ev) != hipSuccess)
                        return b->ctx->fail(SED_E_DEVICE, "event timing");
                }
                out[((size_t)i * P + p) * 4 + k] = t;
            }
    return cnt;
}

int sed_batch_times(sed_batch *b, float *dp_ms, float *tb_ms, int max_runs) {
    if (!b) return SED_E_ARG;
    int rc = sync_batch(b);
    if (rc != SED_OK) return rc;
    const int cnt = (int)std::min<size_t>(b->nlog, (size_t)std::max(0, max_runs));
    const bool script = (b->plan.flags & SED_WANT_SCRIPT) != 0;
    for (int i = 0; i < cnt; ++i) {
        float a = 0, t = 0;
        if (hipEventElapsedTime(&a, b->log[i][0], b->log[i][1]) != hipSuccess ||
            (script && hipEventElapsedTime(&t, b->log[i][2], b->log[i][3]) != hipSuccess))
            return b->ctx->fail(SED_E_DEVICE, "event timing");
        if (b->plan.nparts > 1 && (size_t)i < b->plog.size()) {  // parts: the mean launch of the run's parts
            for (int p = 1; p < b->plan.nparts; ++p) {
                float ap = 0, tp = 0;
                const std::array<hipEvent_t, 12> &pl = b->plog[i];
                if (hipEventElapsedTime(&ap, pl[4 * (p - 1)], pl[4 * (p - 1) + 1]) != hipSuccess ||
                    (script && hipEventElapsedTime(&tp, pl[4 * (p - 1) + 2], pl[4 * (p - 1) + 3]) != hipSuccess))
                    return b->ctx->fail(SED_E_DEVICE, "event timing");
                a += ap;
                t += tp;
            }
            a /= b->plan.nparts;
            t /= b->plan.nparts;
        }
        if (dp_ms) dp_ms[i] = a;
        if (tb_ms) tb_ms[i] = t;
    }
    return cnt;
}

int sed_batch_set_timing(sed_batch *b, int every) {
    if (!b || every < 0) return SED_E_ARG;
    b->time_every = every;
    return SED_OK;
}

int sed_batch_reset_times(sed_batch *b) {
    if (!b) return SED_E_ARG;
    b->nlog = 0;
    return SED_OK;
}

int sed_batch_results(sed_batch *b, double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops,
                      const int64_t *ops_off) {
    if (!b) return SED_E_ARG;
    (void)hipSetDevice(b->ctx->device);
    return fetch_results(b, out_dist, out_is_int, out_len, out_ops, ops_off);
}

int sed_batch_dp_launches(const sed_batch *b) { return b ? b->plan.nparts : SED_E_ARG; }

int sed_batch_device_results(const sed_batch *b, uint64_t *d_dist, uint64_t *d_is_int, uint64_t *d_len,
                             uint64_t *d_ops, uint64_t *ops_words) {
    if (!b) return SED_E_ARG;
    const uint64_t base = (uint64_t)(uintptr_t)b->p_res[b->runs ? b->cur() : 0];
    if (d_dist) *d_dist = base + offsetof(sed_result, dist);
    if (d_len) *d_len = base + offsetof(sed_result, len);
    if (d_is_int) *d_is_int = base + offsetof(sed_result, is_int);
    if (d_ops) *d_ops = (uint64_t)(uintptr_t)b->p_ops;
    if (ops_words) *ops_words = b->plan.ops_words;
    return SED_OK;
}

int sed_batch_export(sed_batch *b, uint64_t d_dist, uint64_t d_len, uint64_t d_ops) {
    if (!b) return SED_E_ARG;
    sed_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (!b->ran) return c->fail(SED_E_STATE, "batch has not been run");
    const int np = b->plan.npairs;
    int rc = sync_batch(b);
    if (rc != SED_OK) return rc;
    const void *resp = b->p_res[b->cur()];
    hipError_t e = hipSuccess;
    if (np && d_dist)
        e = hipMemcpy2DAsync((void *)(uintptr_t)d_dist, sizeof(double), (const char *)resp + offsetof(sed_result, dist),
                             sizeof(sed_result), sizeof(double), np, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && np && d_len)
        e = hipMemcpy2DAsync((void *)(uintptr_t)d_len, sizeof(int32_t), (const char *)resp + offsetof(sed_result, len),
                             sizeof(sed_result), sizeof(int32_t), np, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && d_ops && (b->plan.flags & SED_WANT_SCRIPT) && b->plan.ops_words)
        e = hipMemcpyAsync((void *)(uintptr_t)d_ops, b->p_ops, 4 * b->plan.ops_words, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? SED_OK : c->hipfail(e, "export results");
}

int sed_batch_work(const sed_batch *b, double *cells, double *algo_bytes) {
    if (!b) return SED_E_ARG;
    if (cells) *cells = b->plan.cells;
    if (algo_bytes) *algo_bytes = b->plan.algo_bytes;
    return SED_OK;
}

int sed_run_batch(sed_ctx *c, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                  const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, int32_t npairs, uint32_t flags,
                  double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops,
                  const int64_t *ops_off) {
    if (!c) return SED_E_ARG;
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    (void)hipSetDevice(c->device);
    if (!c->scratch) {
        c->scratch = new sed_batch();
        c->scratch->ctx = c;
        c->scratch->time_every = 0;  // nobody reads a one-shot run's times: no timing events on its kernels
    }
    if (npairs < 0 || (npairs > 0 && (!off_a || !len_a || !off_b || !len_b)))
        return c->fail(SED_E_ARG, "bad batch arguments");
    // Host-buffer batches are cut into chunks whose traceback workspace (2 bits per cell plus the
    // wavefront skew, and the SPLIT route's checkpoints beside its codes: ~0.13 B per cell more) stays under
    // SED_TB_BUDGET_GB (default 48): a list of many long pairs then runs in several launches instead of failing
    // with SED_E_OOM.
    double budget = 48e9;
    if (const char *e = getenv("SED_TB_BUDGET_GB")) budget = std::max(1e6, atof(e) * 1e9);
    int32_t p0 = 0;
    while (p0 < npairs || (npairs == 0 && p0 == 0)) {
        int32_t p1 = p0;
        double bytes = 0;
        if (flags & SED_WANT_SCRIPT) {
            while (p1 < npairs) {
                const double pb = 0.39 * (double)std::max(0, len_a[p1]) * (double)(std::max(0, len_b[p1]) + 127);
                if (p1 > p0 && bytes + pb > budget) break;
                bytes += pb;
                ++p1;
            }
        } else {
            p1 = npairs;
        }
        const int32_t np = p1 - p0;
        int rc = fill_batch(c->scratch, codes_a, off_a + p0, len_a + p0, codes_b, off_b + p0, len_b + p0, np, flags);
        if (rc != SED_OK) return rc;
        if ((rc = run_batch(c->scratch)) != SED_OK) return rc;
        rc = fetch_results(c->scratch, out_dist ? out_dist + p0 : nullptr, out_is_int ? out_is_int + p0 : nullptr,
                           out_len ? out_len + p0 : nullptr, out_ops, ops_off ? ops_off + p0 : nullptr);
        if (rc != SED_OK) return rc;
        if (npairs == 0) break;
        p0 = p1;
    }
    return SED_OK;
}

int sed_run_pair(sed_ctx *c, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m, uint32_t flags,
                 double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops) {
    if (!c) return SED_E_ARG;
    if (n < 0 || m < 0 || (n && !codes_a) || (m && !codes_b)) return c->fail(SED_E_ARG, "bad pair arguments");
    static const uint8_t none = 0;
    const int64_t off = 0;
    int32_t len = 0;
    return sed_run_batch(c, n ? codes_a : &none, &off, &n, m ? codes_b : &none, &off, &m, 1, flags, out_dist, out_is_int,
                         out_len ? out_len : &len, (flags & SED_WANT_SCRIPT) ? out_ops : nullptr,
                         (flags & SED_WANT_SCRIPT) && out_ops ? &off : nullptr);
}

int sed_pair_submit(sed_ctx *c, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m, uint32_t flags) {
    if (!c) return SED_E_ARG;
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (n < 0 || m < 0 || (n && !codes_a) || (m && !codes_b)) return c->fail(SED_E_ARG, "bad pair arguments");
    (void)hipSetDevice(c->device);
    if (!c->scratch) {
        c->scratch = new sed_batch();
        c->scratch->ctx = c;
        c->scratch->time_every = 0;
    }
    static const uint8_t none = 0;
    const int64_t off = 0;
    int rc = fill_batch(c->scratch, n ? codes_a : &none, &off, &n, m ? codes_b : &none, &off, &m, 1,
                        flags & ~(uint32_t)SED_PIPELINE);
    if (rc == SED_OK) rc = run_batch(c->scratch);
    c->pair_pending = rc == SED_OK;
    return rc;
}

int sed_pair_wait(sed_ctx *c, double *out_dist, uint8_t *out_is_int, int32_t *out_len, uint32_t *out_ops) {
    if (!c) return SED_E_ARG;
    if (!c->pair_pending) return c->fail(SED_E_STATE, "no pair submitted");
    c->pair_pending = false;
    (void)hipSetDevice(c->device);
    const int64_t off = 0;
    int32_t len = 0;
    const bool script = (c->scratch->plan.flags & SED_WANT_SCRIPT) != 0;
    return fetch_results(c->scratch, out_dist, out_is_int, out_len ? out_len : &len, script ? out_ops : nullptr,
                         script && out_ops ? &off : nullptr);
}

int sed_full_matrix(sed_ctx *c, const uint8_t *codes_a, int32_t n, const uint8_t *codes_b, int32_t m, double *D,
                    uint8_t *M) {
    if (!c) return SED_E_ARG;
    if (c->pair_pending) return c->fail(SED_E_STATE, "a submitted pair has not been waited for");
    if (n < 0 || m < 0 || !D || !M || (n && !codes_a) || (m && !codes_b)) return c->fail(SED_E_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    if (!c->have_costs) return c->fail(SED_E_STATE, "sed_set_costs() was not called");
    const int save_mode = c->opt.mode, save_R = c->opt.R;
    c->opt.mode = sed_simple_typing(c->costs) ? 2 : 3;
    c->opt.R = 4;
    sed_batch tmp;
    tmp.ctx = c;
    const int64_t zero = 0;
    int rc = fill_batch(&tmp, codes_a, &zero, &n, codes_b, &zero, &m, 1, 0);
    c->opt.mode = save_mode;
    c->opt.R = save_R;
    if (rc != SED_OK) return rc;
    const size_t cells = (size_t)(n + 1) * (size_t)(m + 1);
    DevBuf fD, fM;
    if (!fD.reserve(8 * cells) || !fM.reserve(cells)) {
        fD.release();
        fM.release();
        return c->fail(SED_E_OOM, "full matrix allocation (%zu cells)", cells);
    }
    sed_launch L{};
    L.pd = (const sed_pair_desc *)tmp.p_pd;
    L.npairs = 1;
    L.seqa = tmp.p_seqa;
    L.seqb = tmp.p_seqb;
    L.tb = nullptr;
    L.bnd = (uint32_t *)tmp.d_bnd.p;
    L.res = (sed_result *)tmp.p_res[0];
    L.R = 4;
    L.tasks = tmp.plan.split ? (const int2 *)tmp.p_tasks : nullptr;  // (a pair past 32 symbols: SPLIT)
    L.ntasks = tmp.plan.split ? tmp.plan.ntasks : 0;
    L.stream = c->stream;
    sed_full_out fo{(double *)fD.p, (uint8_t *)fM.p, n, m};
    sed_f64_params fp = tmp.plan.fp;
    hipError_t e = next_split_epoch(&tmp, c->stream, &fp.epoch);
    if (e == hipSuccess) e = sed_launch_f64_full(L, (const double *)c->gtab.p, fp, tmp.plan.mode == SED_MODE_F64_TYPED, fo);
    if (e == hipSuccess) e = hipMemcpyAsync(D, fD.p, 8 * cells, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(M, fM.p, cells, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    fD.release();
    fM.release();
    return e == hipSuccess ? SED_OK : c->hipfail(e, "full matrix");
}

int sed_selftest(sed_ctx *c) {
    if (!c) return SED_E_ARG;
    (void)hipSetDevice(c->device);
    if (!c->selftest.reserve(4)) return c->fail(SED_E_OOM, "selftest buffer");
    hipError_t e;
    uint32_t h = 0;
    if ((e = hipMemsetAsync(c->selftest.p, 0, 4, c->stream)) != hipSuccess) return c->hipfail(e, "memset");
    if ((e = sed_launch_selftest((uint32_t *)c->selftest.p, c->stream)) != hipSuccess) return c->hipfail(e, "launch");
    if ((e = hipMemcpyAsync(&h, c->selftest.p, 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return c->hipfail(e, "copy");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hipfail(e, "sync");
    return (int)h;
}

}  // extern "C"
