// sed_runtime.h — what the runtime's units share (sed_runtime.cpp: contexts and batches; sed_fit_runtime.cpp: fit
// search): the grow-only device and pinned buffers and the context.  Private to the library.
#pragma once
#include "../../include/sed.h"
#include "sed_plan.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint64_t gen = 0;  // bumped by every (re)allocation: memory of a new generation may hold anything
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // grow-only; returns false on OOM
    bool reserve(size_t bytes) {
        if (bytes <= cap) return true;
        release();
        size_t want = std::max<size_t>(bytes, 256);
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return false;
        }
        cap = want;
        ++gen;
        return true;
    }
};

// the same over pinned host memory (hipHostMalloc); a first allocation is of at least min_bytes
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    bool reserve(size_t bytes, size_t min_bytes) {
        if (bytes <= cap) return true;
        release();
        const size_t want = std::max(bytes, min_bytes);
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return false;
        }
        cap = want;
        return true;
    }
};

// The process's environment knobs, read once: the options of every new context start from them (sed_runtime.cpp).
const sed_opts &sed_env_opts();

struct sed_fit_state;  // fit search's device arrays and timer (sed_fit_runtime.cpp), made by the first sed_fit_search
void sed_fit_state_destroy(sed_fit_state *s);

struct sed_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool have_costs = false;
    sed_costs costs;
    DevBuf gtab;  // fp64 kernel table: per entry {value bits, is-int flag}
    sed_opts opt = sed_env_opts();
    DevBuf selftest;
    sed_batch *scratch = nullptr;
    PinBuf pin;  // pinned host staging of small batches: the upload blob, then the results' download
    bool pin_busy = false;  // a copy from / to `pin` may still be in flight on `stream`
    bool pair_pending = false;  // sed_pair_submit enqueued the scratch batch; sed_pair_wait has not fetched it
    sed_fit_state *fit = nullptr;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    int hipfail(hipError_t e, const char *what) {
        return fail(SED_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
    }
};
