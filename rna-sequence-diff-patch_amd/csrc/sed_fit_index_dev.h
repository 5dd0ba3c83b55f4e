// sed_fit_index_dev.h - the lane of an index kernel, for every fit unit of either numeric route (sed_fit.hip,
// sed_fit_f64.hip; sed_fit_long.hip, sed_fit_long_f64.hip): the chunk record, the sed_fit_lane derived from it
// (sed_internal.h: sed_fit_derive_lane, the function the device-free sed_fit_index_lanes checks against the lane
// builder), and pair = query * ntexts + text.  One copy of each; the DPs that run the lane stay in their units.
#pragma once
#include "sed_internal.h"

// One lane per (query, chunk record): q = the block's query (q0 + blockIdx.y), whose pattern record and length are
// uniform across the block; t = blockIdx.x * 64 + threadIdx.x = the chunk record.
__device__ __forceinline__ sed_fit_lane sed_fit_index_lane(const sed_fit_chunk *__restrict__ chunks,
                                                           const sed_fit_text *__restrict__ texts, int ntexts,
                                                           const int32_t *__restrict__ plens, int q, int32_t chunk, int32_t W,
                                                           int t) {
    const sed_fit_chunk ck = chunks[t];
    sed_fit_lane ln = sed_fit_derive_lane(ck, texts[ck.text], chunk, plens[q], W);
    ln.pair = q * ntexts + ck.text;
    return ln;
}

// One wave per (query, chunk record), R rows a lane: blockIdx.x = the chunk record, q0 + blockIdx.y = the query's place
// in its R group, whose record is pats[64 R place ...]; lane l reads bytes l R .. l R + R - 1 of it into pw, one byte a
// code from bit 0 of pw[0] on.  *query = the query itself, qlist[place]
// (written unconditionally: with a null test in front, two of the fp64 long kernels compiled to other code).
template <int R>
__device__ __forceinline__ sed_fit_lane sed_fit_long_lane(const sed_fit_chunk *__restrict__ chunks,
                                                          const sed_fit_text *__restrict__ texts, int ntexts,
                                                          const uint8_t *__restrict__ pats, const int32_t *__restrict__ plens,
                                                          const int32_t *__restrict__ qlist, int q0, int32_t chunk, int32_t W,
                                                          uint32_t (&pw)[(R + 3) / 4], int *query) {
    const int place = q0 + (int)blockIdx.y;
    const int q = qlist[place];
    const sed_fit_chunk ck = chunks[blockIdx.x];
    sed_fit_lane ln = sed_fit_derive_lane(ck, texts[ck.text], chunk, plens[q], W);
    ln.pair = q * ntexts + ck.text;
    *query = q;
    const uint8_t *rec = pats + (size_t)place * (64 * R) + threadIdx.x * R;
    if constexpr (R == 2) {
        pw[0] = *(const uint16_t *)rec;
    } else {
#pragma unroll
        for (int i = 0; i < R / 4; ++i) pw[i] = ((const uint32_t *)rec)[i];
    }
    return ln;
}
