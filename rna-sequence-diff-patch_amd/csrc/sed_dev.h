// sed_dev.h — device helpers every kernel family shares: cross-lane moves (whole wave and 16-lane segments), three-way
// and packed 16-bit min / add, L1-bypassing loads, the per-cell code group layout and its stores, compile-time loops,
// and the tagged words and LDS flags of the SPLIT hand-off (integer and fp64 SPLIT kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define DPP_WAVE_SHL1 0x130  // lane i <- lane i+1, lane 63 keeps `old`
#define DPP_WAVE_ROL1 0x134  // lane i <- lane i+1, lane 63 <- lane 0
#define DPP_WAVE_SHR1 0x138  // lane i <- lane i-1, lane 0 keeps `old`

__device__ __forceinline__ uint32_t dpp_shr1(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, DPP_WAVE_SHR1, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t dpp_shl1(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, DPP_WAVE_SHL1, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t dpp_rol1(uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)src, (int)src, DPP_WAVE_ROL1, 0xf, 0xf, false);
}
// lane i <- lane i-1's src + addv, lane 0 keeps `old`: one v_add_u32_dpp (the s_nop covers the DPP read of
// a VGPR written by the previous VALU instruction)
__device__ __forceinline__ uint32_t dpp_shr1_add(uint32_t old, uint32_t src, uint32_t addv) {
    asm("s_nop 1\n\tv_add_u32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(old) : "v"(src), "v"(addv));
    return old;
}
__device__ __forceinline__ double dpp_shr1_f64(double old, double src) {
    const uint64_t o = __double_as_longlong(old), s = __double_as_longlong(src);
    const uint32_t lo = dpp_shr1((uint32_t)o, (uint32_t)s);
    const uint32_t hi = dpp_shr1((uint32_t)(o >> 32), (uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double dpp_shl1_f64(double old, double src) {
    const uint64_t o = __double_as_longlong(old), s = __double_as_longlong(src);
    const uint32_t lo = dpp_shl1((uint32_t)o, (uint32_t)s);
    const uint32_t hi = dpp_shl1((uint32_t)(o >> 32), (uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double dpp_rol1_f64(double src) {
    const uint64_t s = __double_as_longlong(src);
    const uint32_t lo = dpp_rol1((uint32_t)s), hi = dpp_rol1((uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}

// The same moves inside segments of SW lanes (SW = 64: the whole wave; SW = 16: each DPP row, so a wave runs four
// independent segments, the fp64 kernel's short pairs): shr = lane i <- lane i-1 (the segment's lane 0 keeps `old`,
// row_shr:1), shl = lane i <- lane i+1 (the segment's last lane keeps `old`, row_shl:1), rol = lane i <- lane i+1
// mod SW (row_ror:15).
#define DPP_ROW_SHL1 0x101
#define DPP_ROW_SHR1 0x111
#define DPP_ROW_ROR15 0x12F
template <int SW> __device__ __forceinline__ uint32_t seg_shr1(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, SW == 64 ? DPP_WAVE_SHR1 : DPP_ROW_SHR1, 0xf, 0xf,
                                                 false);
}
template <int SW> __device__ __forceinline__ uint32_t seg_shl1(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, SW == 64 ? DPP_WAVE_SHL1 : DPP_ROW_SHL1, 0xf, 0xf,
                                                 false);
}
template <int SW> __device__ __forceinline__ uint32_t seg_rol1(uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)src, (int)src, SW == 64 ? DPP_WAVE_ROL1 : DPP_ROW_ROR15, 0xf, 0xf,
                                                 false);
}
template <int SW> __device__ __forceinline__ double seg_shr1_f64(double old, double src) {
    const uint64_t o = __double_as_longlong(old), s = __double_as_longlong(src);
    const uint32_t lo = seg_shr1<SW>((uint32_t)o, (uint32_t)s), hi = seg_shr1<SW>((uint32_t)(o >> 32), (uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}
template <int SW> __device__ __forceinline__ double seg_shl1_f64(double old, double src) {
    const uint64_t o = __double_as_longlong(old), s = __double_as_longlong(src);
    const uint32_t lo = seg_shl1<SW>((uint32_t)o, (uint32_t)s), hi = seg_shl1<SW>((uint32_t)(o >> 32), (uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}
template <int SW> __device__ __forceinline__ double seg_rol1_f64(double src) {
    const uint64_t s = __double_as_longlong(src);
    const uint32_t lo = seg_rol1<SW>((uint32_t)s), hi = seg_rol1<SW>((uint32_t)(s >> 32));
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { return min(min(a, b), c); }
__device__ __forceinline__ uint32_t umax3(uint32_t a, uint32_t b, uint32_t c) { return max(max(a, b), c); }
// An opaque v_min3_u32: over three selects (tie keys of the fp64 kernel) the compiler rewrites
// min(min(a, b), c) into select-of-min chains that cost one op more per cell.
__device__ __forceinline__ uint32_t umin3_op(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// relaxed agent-scope load = global_load sc1: bypasses this CU's L1 so a
// stripe reads the bottom row its own wave stored during the previous stripe.
__device__ __forceinline__ uint32_t load_sc1(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t load_sc1_u64(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Traceback codes are stored per "group" of G = 64/R steps: G steps x R rows x 2 bits
// = 16 bytes per lane, one dwordx4 store; the wave writes 1 KiB contiguous.
template <int R> struct Grp { static constexpr int G = 64 / R; };

__device__ __forceinline__ void store_tb(uint32_t *p, const uint32_t (&w)[4]) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
// G (a multiple of 4) consecutive words, 16-byte aligned
template <int G> __device__ __forceinline__ void store_words(uint32_t *p, const uint32_t (&w)[G]) {
#pragma unroll
    for (int k = 0; k < G; k += 4) *reinterpret_cast<uint4 *>(p + k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));  // v_pk_*_u16 operands
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t,
                              __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// f(integral_constant<int, I>) for I = B .. E-1, expanded at compile time
template <int B, int E, class F> __device__ __forceinline__ void static_for(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

template <bool B> struct BoolTag { static constexpr bool value = B; };

// Slots of a device hit list for the hitting lanes of a wave, one atomic add a wave: the hitting lane of rank 0 adds
// the wave's popcount to *count, every hitting lane's slot is the sum before + its rank among them.  True in the lanes
// that hit (whose *slot is then set); the callers store their record where the slot is below their list's room, so
// *count counts every hit, stored or not.  The one copy for the fit and join hit lists.
__device__ __forceinline__ bool wave_claim_slot(unsigned long long *count, bool hit, unsigned long long *slot) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(hit);
    if (b == 0) return false;
    if (!hit) return false;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    unsigned long long base = 0;
    if (rank == 0) base = atomicAdd(count, (unsigned long long)__popcll(b));
    // (the first active lane here is the hitting lane of rank 0, so readfirstlane hands every lane its sum)
    *slot = (((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)base)) + rank;
    return true;
}

// Inter-workgroup hand-off of stripe bottom rows (SPLIT mode), per 16-step group and self-validating: every
// bottom-row cell travels as one 64-bit word {tag, value}, stored with a relaxed agent-scope 64-bit atomic
// (single-copy atomic, so a reader sees the tag and the value of one store together), tag = the run's epoch
// (1..32767, prm.epoch) | poison << 31.  The consumer's feeder wave (split_feed) polls the words and re-polls any
// whose tag is not this run's.  No counter, fence or s_waitcnt on the producer side:
// with the per-chunk counter hand-off (stores, s_waitcnt, release fence, counter; the consumer prefetching a
// chunk ahead) each stripe ran 3 chunks (192 steps) behind the one above.
// The previous run's words carry another epoch; the host zeroes the buffer on a batch's first run and when the
// epoch wraps.  A stripe that gave up waiting publishes with the poison bit, so its consumer stops waiting too,
// and the last stripe reports err.
#define SED_PROG_POISON 0x80000000u
__device__ __forceinline__ void store_tagged(uint64_t *p, uint32_t tag, uint32_t v) {
    __hip_atomic_store(p, ((uint64_t)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the flags are relaxed workgroup-scope atomics: a volatile LDS access is followed by s_waitcnt vmcnt(0) lgkmcnt(0)
__device__ __forceinline__ uint32_t lds_flag_get(uint32_t *f) {
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_set(uint32_t *f, uint32_t v) {
    __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// issue priority of the SPLIT kernels' stripe waves, integer and fp64 (SED_SPLIT_PRIO): a single pair's stripe chain is latency-bound, and the
// previous run's traceback kernels may share its SIMDs.  Config 2 at 100 steps: 0.2974-0.3008 against 0.2984-0.3039
// ms per step at 0, 3 interleaved rounds (profiles/r05/s17)
#ifndef SED_SPLIT_PRIO
#define SED_SPLIT_PRIO 2
#endif
