// sed_i32_keys.h — the integer (packed-key) cell machinery that more than one kernel family uses: the dot-product
// update candidate and its hazard fence, the row ladders, one column step of a lane's rows (i32_step), the borders,
// the sink decode, the conversions from forward keys to traceback keys, the ramp sentinels and the stripe kernel's
// group of steps (i32_group).  Users: sed_kernels.hip (stripe / SPLIT, CHAIN), sed_tb.hip (the tracebacks'
// ladder patterns; through sed_ck_tile.h, sed_ck_codes_kernel) and, through sed_ck_tile.h, sed_cktb.hip.
#pragma once
#include "sed_internal.h"
#include "sed_dev.h"

// the dot keys' update candidate: diag + dot4(row vector, column vector) over signed bytes (v_dot4_i32_i8)
// (the VOP3P form with its own destination: the builtin picks v_dot4c_i32_i8, which accumulates in place and made
// the register allocator copy every diagonal first, 186 instead of 111 v_mov per 256 cells).  The hardware needs
// wait states between a v_dot4 and a VALU op reading its result, which the compiler cannot see through the asm
// (tools/ubench/dot_sem.hip: the next op reads a stale value), so the asm is volatile (issued in program order)
// and the caller keeps every consumer 4 dots behind its producer (dot_fence).
__device__ __forceinline__ uint32_t dot_add(uint32_t rowv, uint32_t colv, uint32_t diag) {
    uint32_t r;
    asm volatile("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(r) : "v"(rowv), "v"(colv), "v"(diag));
    return r;
}
// dots issued ahead of the max / min chain (>= 4: tools/ubench/dot_sem.hip shows the next op reading stale data;
// the fence then leaves 3 or more instructions between a dot and its reader).  A/B on config 4's forward kernel
// (tools/ab.sh, profiles/r02_dot/ab_ahead.jsonl): 4 -> 9.24-9.33 ms, 6 same, 8 -> 9.16-9.23 ms, 12 9.29, 16 9.18.
#ifndef SED_DOT_AHEAD
#define SED_DOT_AHEAD 8
#endif
// an empty volatile asm on a dot result, placed after the dots that must separate it from its consumer: the
// consumer cannot be scheduled above it.  (The compiler treats the asm as a write of x and puts an s_nop 0 between
// it and the max reading x, 50 per 64-cell group.  Fencing one row earlier drops that to 29 but lets the compiler
// pair up dependent maxes back to back: config 4's forward 9.19 -> 9.49 ms, so the fence stays next to its max.)
__device__ __forceinline__ void dot_fence(uint32_t &x) { asm volatile("" : "+v"(x)); }

// ---------------------------------------------------------------------------
// Integer (packed-key) kernels.  The reference's decision per cell is the
// lexicographic minimum of (distance, path length, op) over its candidates, i.e.
// one unsigned min over the keys
//     V = D << 16 + L << 3 + op        (op 0 insert, 1 delete, 2 update)
// with candidates V_left + Ki, V_up + Kd + 1, V_diag + (cost << 16) + 10, where
// Ki = (insert << 16) + 8 and Kd = (delete << 16) + 8.  The L field may run past
// its 13 bits: the three candidates of cell (i, j) have L in [max(i,j), i+j],
// so 8 * |L difference| <= 8 * min(n, m) < 2^16 and any distance difference
// still dominates (the host keeps min(n, m) < 8192); at the sink L is read
// modulo 8192 inside that window.
//
// Offset keys.  Subtracting the same amount from the three candidates of a cell
// keeps their order, so cells are stored as
//     W(i, j) = V(i, j) - i*Kd - j*Ki + B + c(i)        (B = SED_KB3)
// where i*Kd + j*Ki bounds V from above (the all-delete-then-insert path) and
// the host checks that it stays below B, so W never wraps.  c(i) in 0..5 is a
// per-row residue ("ladder") that steps down by one from row to row and jumps
// back up on a few rows (Ladder<R> below, periodic in i with a period dividing
// R, so every lane row has a compile-time rung).  With d = c(i) - c(i-1):
//     insert candidate = W_left,
//     delete candidate = W_up + (d + 1)          (no add on the d = -1 rows),
//     update candidate = W_diag + ((cost - delete - insert) << 16) - 6 + d.
// The update constant is one v_perm_b32 of a per-row byte vector (cost - delete
// - insert - 1; the bytes below it 0xFF / (d - 6) from the inline constant d - 6;
// the host requires cost <= insert + delete).  mm = min3 is a clean value (low 3
// bits = c(i)) plus the winning op, which never leaves the 8-block because
// c(i) + 2 <= 7, so clearing the op is one v_and_or: (mm & ~7) | c(i).  A cell
// therefore costs v_perm, v_add, v_min3, v_and_or, v_alignbit = 5 VALU, plus the
// delete add on 3 of 16 rows.  The traceback codes are mm's low 2 bits
// (c(i) + op) & 3; the traceback kernels subtract the rung of the row they are on.
// Every border is a constant: W(0, j) = B, W(i, 0) = B + c(i).
//
// Distance keys (!LEN): V = D << 16 - U without an op field, W = V -
// i*(delete << 16) - j*(insert << 16) + SED_KB, update constant ((cost - delete -
// insert) << 16) - 1: an update also subtracts 1 from the low half, which never
// borrows (fewer than 2^16 updates on any path), so D = (V + 0xFFFF) >> 16 and
// U = (D << 16) - V.  At equal D the smaller key has more updates, i.e. the
// shorter path (L = i + j - U), so the min is the (D, L) minimum; only the op
// tie-break is missing, which the CK traceback recomputes.  That is v_perm,
// v_add, v_min3 = 3 VALU per cell; every border is SED_KB.
// Lanes run unmasked all the time, and a lane past column m computes columns
// that nothing reads.
// ---------------------------------------------------------------------------
#define SED_KB3 0xFFFFFE00u  // bias of the ladder keys (= 0 mod 8, 512 below 2^32 for the ramp sentinel)

// The ladder: rung c(i) of row i by i mod P, 4 bits per rung; runs of 5,4,3,2,1,0 as long as the
// period allows (P = 16: jumps at i = 1, 7, 11 (mod 16); P = 8: at 1, 7; P = 4: at 1).
template <int R> struct Ladder {
    static constexpr int P = R >= 16 ? 16 : R;
    static constexpr uint64_t pat = P == 16 ? 0x1234501230123450ull : (P == 8 ? 0x10123450ull : 0x1230ull);
    static constexpr int rung(int i) { return (int)((pat >> (4 * (i & (P - 1)))) & 0xF); }
};
// The wide ladder of the ladder dot keys (LDOT = 2, the CHAIN kernel): rung + op in the low 4 bits (V = D*A + 16L + op,
// the host keeps 16 min(n, m) + 15 < A and A a multiple of 16), rungs up to 13, so the rung runs down through a whole period
// with one jump (P = 8: rows 1..7 on rungs 7..1; P = 16: 13..0 and two jumps): 1 jump row in 8 instead of 2, each a
// delete add and an update add fewer.  Same P, so the tracebacks read it through their runtime pattern alone.
template <int R> struct LadderW {
    static constexpr int P = R >= 16 ? 16 : R;
    static constexpr uint64_t pat = P == 16 ? 0x10123456789ABCD0ull : (P == 8 ? 0x12345670ull : 0x1230ull);
    static constexpr int rung(int i) { return (int)((pat >> (4 * (i & (P - 1)))) & 0xF); }
};

// One column step of a lane's R rows.  tv = {top, sel} of this step's column
// for lane 0 (the stripe's top row and str2 symbol): every lane reads the same
// LDS word, only lane 0 keeps it (the DPP move's `old` operand).  Lane rows are
// i = (multiple of P) + r + 1, so row r sits on rung Ladder::rung(r + 1).
// SELL: the lane's own selector arrives in tv.y (read from the wave's LDS selector ring, see
// sed_wf_i32_kernel), instead of flowing from lane 0 through a DPP move (one DPP + one copy per step).
// TOPC: lane 0's top is the row-0 constant, which its top_prev already holds (single-stripe pairs: the CHAIN
// kernel), so the DPP move writes over top_prev in place instead of over a copy of tv.x.
template <int R, bool TB, bool LEN, bool COLLECT = true, bool SELL = false, bool TOPC = false, bool DOT = false,
          int LDOT = 0>
__device__ __forceinline__ void i32_step(uint32_t (&V)[R], const uint32_t (&cv)[R], uint32_t &top_prev,
                                         uint32_t &bottom, uint32_t &selv, const uint2 tv, uint32_t &outc,
                                         uint32_t (&W)[4], const int u, const uint32_t jv = 0u) {
    using Lad = Ladder<R>;
    if constexpr (SELL) selv = tv.y;
    else selv = dpp_shr1(tv.y, selv);  // perm selector of this column's str2 symbol
    constexpr int d0 = Lad::rung(1) - Lad::rung(0);
    // row 0's update candidate from top_prev, before the DPP move overwrites top_prev in place (TOPC): the
    // empty asm makes the move's `old` depend on it, so top_prev needs no copy
    if constexpr (LEN && LDOT) {
        // ladder keys with the update addend as one v_dot4 (ladder dot keys, sed_runtime.cpp): the addend of a row
        // whose rung steps down by one (d = -1) is -(A*kappa + 7) over the 3-bit ladder (LDOT = 1: V = D*A + 8L) or
        // -(A*kappa + 15) over the wide one (LDOT = 2: V = D*A + 16L, LadderW) = the dot of the row's and the column's
        // byte vectors (column vectors negated by the host); a row with another step adds d + 1 to it, which is where
        // the perm took its inline constant d - 6.  Candidates run 4 rows ahead of the min chain (dot_add).  Per cell:
        // v_dot4, v_min3, v_and_or, v_alignbit = 4 VALU (5 with the perm), plus two adds on a jump row.
        using Lad = std::conditional_t<LDOT == 2, LadderW<R>, Ladder<R>>;
        constexpr uint32_t LOW = LDOT == 2 ? 15u : 7u;  // the rung + op field
        // the wide ladder's jump is row 0 of every lane (i = 1 mod P): its delete and update inputs, the cell above
        // the band and the diagonal, both take d + 1 = J0, which the DPP move from lane t - 1 adds itself (one
        // v_add_u32_dpp with jv = J0 instead of v_mov_b32_dpp), so top_prev carries it too (i32_reset: tpb)
        constexpr bool BIAS = LDOT == 2;
        constexpr uint32_t J0 = (uint32_t)(Lad::rung(1) - Lad::rung(0) + 1);
        constexpr int AH = R < 4 ? R : 4;
        uint32_t cand[R];
        cand[0] = dot_add(cv[0], selv, top_prev);
#pragma unroll
        for (int r = 1; r < AH; ++r) cand[r] = dot_add(cv[r], selv, V[r - 1]);
        const uint32_t topv = BIAS ? dpp_shr1_add(TOPC ? top_prev : tv.x + J0, bottom, jv)
                                   : dpp_shr1(TOPC ? top_prev : tv.x, bottom);
        uint32_t up = topv;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r + AH < R) cand[r + AH] = dot_add(cv[r + AH], selv, V[r + AH - 1]);
            dot_fence(cand[r]);
            const int c = Lad::rung(r + 1), d = c - Lad::rung(r);  // compile-time after unrolling
            const bool plain = d == -1 || (BIAS && r == 0);          // (BIAS: row 0's inputs carry d + 1)
            const uint32_t upd = plain ? cand[r] : cand[r] + (uint32_t)(d + 1);
            const uint32_t mm = umin3(V[r], plain ? up : up + (uint32_t)(d + 1), upd);
            if constexpr (TB) {
                const int k = u * R + r;
                W[k >> 4] = __builtin_amdgcn_alignbit(mm, W[k >> 4], 2);
            }
            up = (mm & ~LOW) | (uint32_t)c;
            V[r] = up;
        }
        top_prev = topv;
        bottom = V[R - 1];
        if constexpr (COLLECT) outc = dpp_shl1(bottom, outc);
        return;
    }
    if constexpr (DOT) {  // dot keys: maximise, the update addend is one v_dot4 of signed bytes
        // candidates run 4 rows ahead of the max chain (the dot's result hazard, dot_add): row r + 4's diagonal is
        // still the old value of row r + 3 when row r is updated
        constexpr int AH = R < SED_DOT_AHEAD ? R : SED_DOT_AHEAD;
        uint32_t cand[R];
        cand[0] = dot_add(cv[0], selv, top_prev);
#pragma unroll
        for (int r = 1; r < AH; ++r) cand[r] = dot_add(cv[r], selv, V[r - 1]);
        const uint32_t topv = dpp_shr1(TOPC ? top_prev : tv.x, bottom);
        uint32_t up = topv;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r + AH < R) cand[r + AH] = dot_add(cv[r + AH], selv, V[r + AH - 1]);
            dot_fence(cand[r]);  // row r's candidate was issued AH dots ago
            up = umax3(V[r], up, cand[r]);
            V[r] = up;
        }
        top_prev = topv;
        bottom = V[R - 1];
        if constexpr (COLLECT) outc = dpp_shl1(bottom, outc);
        return;
    }
    uint32_t dg0 = top_prev + __builtin_amdgcn_perm(cv[0], LEN ? (uint32_t)(d0 - 6) : 0xFFFFFFFFu, selv);
    if constexpr (TOPC) asm("" : "+v"(top_prev) : "v"(dg0));
    const uint32_t topv = dpp_shr1(TOPC ? top_prev : tv.x, bottom);  // cell above the band, this column
    uint32_t up = topv, diag = top_prev;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t left = V[r];
        uint32_t mm;
        if constexpr (LEN) {
            const int c = Lad::rung(r + 1), d = c - Lad::rung(r);  // compile-time after unrolling
            // insert (op 0) = left, delete (op 1) = up + d + 1, update (op 2) = diag + offset constant
            // (perm bytes 1:0 from the inline constant d - 6)
            mm = umin3(left, d == -1 ? up : up + (uint32_t)(d + 1),
                       r == 0 ? dg0 : diag + __builtin_amdgcn_perm(cv[r], (uint32_t)(d - 6), selv));
            if constexpr (TB) {
                const int k = u * R + r;
                W[k >> 4] = __builtin_amdgcn_alignbit(mm, W[k >> 4], 2);
            }
            up = (mm & ~7u) | (uint32_t)c;
        } else {
            mm = umin3(left, up, r == 0 ? dg0 : diag + __builtin_amdgcn_perm(cv[r], 0xFFFFFFFFu, selv));
            up = mm;
        }
        diag = left;
        V[r] = up;
    }
    top_prev = topv;
    bottom = V[R - 1];
    if constexpr (COLLECT) outc = dpp_shl1(bottom, outc);  // lane 63's bottom row (CK: the row checkpoints)
}

// Column-0 state of rows row0+1 .. row0+R (row0 = multiple of P) and of row0, the diagonal of the
// first column.
template <int R, bool LEN, bool DOT = false, bool WIDE = false>
__device__ __forceinline__ void i32_reset(uint32_t (&V)[R], uint32_t &top_prev) {
    // (WIDE: top_prev carries row 0's jump, i32_step LDOT = 2)
    top_prev = LEN ? SED_KB3 + (WIDE ? (uint32_t)(LadderW<R>::rung(1) - LadderW<R>::rung(0) + 1) : 0u)
                   : DOT ? SED_KB_DOT : SED_KB;
#pragma unroll
    for (int r = 0; r < R; ++r)
        V[r] = LEN ? SED_KB3 + (uint32_t)(WIDE ? LadderW<R>::rung(r + 1) : Ladder<R>::rung(r + 1)) : DOT ? SED_KB_DOT : SED_KB;
}
// row 0 (D = j*insert, L = j) in offset keys
template <bool LEN, bool DOT = false> __device__ __forceinline__ uint32_t i32_row0() {
    return LEN ? SED_KB3 : DOT ? SED_KB_DOT : SED_KB;
}

// The sink cell (n, m) back to V space; returns {D, L} (without LEN, L = n + m - U when WANT_L, else -1).
// Dot key k = A*X + U -> {X, U}: X = floor(k*kmax / (A*kmax + 1)) by a multiply-shift (the host checks k*kmax
// < 2^29 and picks dotM, dotS so the product is exact), U = k - A*X.
__device__ __forceinline__ uint2 dot_split(uint32_t w, const sed_i32_params &prm) {
    const uint32_t k = w - SED_KB_DOT;
    const uint32_t X = __umulhi(k, prm.dotM) >> (prm.dotS - 32u);  // dotM carries kmax (one v_mul_hi, full-rate rest)
    return make_uint2(X, k - __umul24(prm.dotA, X));
}
template <int R, bool LEN, bool WANT_L = false, bool DOT = false, int LDOT = 0>
__device__ __forceinline__ int2 i32_decode(uint32_t w, int n, int m, const sed_i32_params &prm) {
    if constexpr (LEN && LDOT) {  // V = D*A + uL: one division per pair
        // u = 8: the host keeps 8 (n + m) + 7 < A; u = 16 (the wide ladder): 16 min(n, m) + 15 < A, and L is read inside
        // its window [max(n, m), n + m] (the candidates of a cell differ in L by at most min(n, m), so that bound keeps
        // their order)
        constexpr uint32_t U = LDOT == 2 ? 16u : 8u;
        const uint32_t rg = (uint32_t)(LDOT == 2 ? LadderW<R>::rung(n) : Ladder<R>::rung(n));
        const uint32_t v = w - SED_KB3 - rg + (uint32_t)n * (prm.del * prm.ladA + U) + (uint32_t)m * (prm.ins * prm.ladA + U);
        const uint32_t lo = LDOT == 2 ? U * (uint32_t)max(n, m) : 0u;
        const uint32_t D = (v - lo) / prm.ladA;
        return make_int2((int)D, (int)((v - D * prm.ladA) / U));
    } else if constexpr (DOT) {  // D = n*delete + m*insert - X, L = n + m - U
        const uint2 xu = dot_split(w, prm);
        return make_int2((int)((uint32_t)n * prm.del + (uint32_t)m * prm.ins - xu.x), n + m - (int)xu.y);
    } else if constexpr (LEN) {
        const uint32_t v = w - SED_KB3 - (uint32_t)Ladder<R>::rung(n) + (uint32_t)n * ((prm.del << 16) + 8u) +
                           (uint32_t)m * ((prm.ins << 16) + 8u);
        const uint32_t lo = (uint32_t)max(n, m);
        const uint32_t L = lo + ((((v >> 3) & 0x1FFFu) - lo) & 0x1FFFu);  // L in [max(n,m), n+m]
        return make_int2((int)((v - 8u * L) >> 16), (int)L);
    } else {
        const uint32_t v = w - SED_KB + (((uint32_t)n * prm.del + (uint32_t)m * prm.ins) << 16);
        const uint32_t D = (v + 0xFFFFu) >> 16;
        return make_int2((int)D, WANT_L ? n + m - (int)((D << 16) - v) : -1);
    }
}

// The distance alone of cell (i, j) from its checkpoint-forward key (dot or distance keys), as the sink decode above
template <bool DOT>
__device__ __forceinline__ uint32_t ck_key_dist(uint32_t w, int i, int j, const sed_i32_params &prm) {
    const uint32_t base = (uint32_t)i * prm.del + (uint32_t)j * prm.ins;
    if constexpr (DOT) return base - dot_split(w, prm).x;
    return (w - SED_KB + (base << 16) + 0xFFFFu) >> 16;
}

// Distance key (!LEN) of a cell -> the traceback key of the same (D, L) (clean, op 0).  Traceback keys
// (sed_traceback_ck_kernel) are T = V - i*((delete << 16) + 4) - j*((insert << 16) + 4) + SED_KB over
// V = D << 16 | L << 2 | op: the insert candidate is the left cell, the delete candidate the cell above
// + 1, the update candidate the diagonal + ((cost - delete - insert) << 16) - 2, and the winner's low 2
// bits are the op itself.  With U = (SED_KB - w) & 0xFFFF (updates on the path) both keys share
// (D - i*delete - j*insert) << 16, and T = w - 3U; independent of the cell's position.
__device__ __forceinline__ uint32_t i32_dist_to_tb(uint32_t w) {
    const uint32_t U = (SED_KB - w) & 0xFFFFu;
    return w - 3u * U;
}
// either forward key format -> traceback key: T = SED_KB - (X << 16) - 4U (X = i*delete + j*insert - D)
__device__ __forceinline__ uint32_t ck_to_tb(uint32_t w, const sed_i32_params &prm) {
    if (prm.dot) {  // = SED_KB - 4k + 4A X - (X << 16)
        const uint32_t k = w - SED_KB_DOT;
        const uint32_t X = __umulhi(k, prm.dotM) >> (prm.dotS - 32u);
        return SED_KB - 4u * k + __umul24(4u * prm.dotA, X) - (X << 16);
    }
    return i32_dist_to_tb(w);
}

// Ramp for free.  Every lane starts a stripe at its column-0 state and lane t begins real work
// at step t.  Before that it runs "virtual" columns, which leave its state unchanged: their str2
// selector is a sentinel, so with every neighbour at its column-0 value the insert candidate
// (the border itself) is the minimum and keeps the border:
//   ladder keys: insert B + c(i), delete B + c(i) + 1, update B + c(i-1) + 255 (SED_SEL_SENT3:
//   update constant 0xFF >= any jump d);
//   distance keys (and the 16-bit packed ones): insert = delete = border, update border + 0.
// The lane's first real column then sees exactly D[row][0], D[row-1][0] and the cell above.
#define SED_SEL_SENT 0x0C0C0C0Cu
#define SED_SEL_SENT3 0x0C0C0C0Du
template <bool LEN, bool DOT = false> __device__ __forceinline__ uint32_t i32_sent() {
    return LEN ? SED_SEL_SENT3 : DOT ? 0u : SED_SEL_SENT;  // dot keys: the zero column vector adds 0
}
// perm selector of str2 symbol b: byte3 <- 0xFF, byte2 <- cost byte b, bytes 1:0 <- the constant
__device__ __forceinline__ uint32_t i32_sel(uint32_t b) { return 0x0D000100u | ((4u + b) << 16); }

// CAP: the group that produces the sink cell (captured on its lane); every extra variant is
// another merge point where the register allocator may insert copies of the whole state.
// The stripe kernel's group: lane 0's top values from the chunk's LDS slots (ltop, broadcast reads),
// each lane's str2 selectors from the wave's LDS selector ring at its own column (lsel: this group's
// first step for this lane, doubled ring so the G reads never wrap).
template <int R, bool TB, bool LEN, bool CAP, bool CK = false, bool DOT = false, bool COLLECT = !CK>
__device__ __forceinline__ void i32_group(uint32_t (&V)[R], const uint32_t (&cv)[R], uint32_t &top_prev,
                                          uint32_t &bottom, uint32_t &selv, const uint32_t *__restrict__ ltop,
                                          const uint32_t *__restrict__ lsel, uint32_t &outc, uint32_t (&W)[4],
                                          const int s0, const int lane, const int cap_step, const int cap_lane,
                                          const int cap_row, uint32_t &cap, uint32_t (&rcv)[Grp<R>::G]) {
    constexpr int G = Grp<R>::G;
    uint2 tv[G];
    const uint32_t *lp = ltop + (s0 & 63);  // G divides 64: a group never wraps the chunk
#pragma unroll
    for (int u = 0; u < G; ++u) tv[u] = make_uint2(lp[u], lsel[u]);
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int s = s0 + u;
        i32_step<R, TB, LEN, COLLECT, true, false, DOT>(V, cv, top_prev, bottom, selv, tv[u], outc, W, u);
        if constexpr (CK) rcv[u] = V[R - 1];  // the band's bottom row, step s (row checkpoints)
        if constexpr (CAP) {
            const bool hit = (s == cap_step) && (lane == cap_lane);
#pragma unroll
            for (int r = 0; r < R; ++r) cap = (hit && r == cap_row) ? V[r] : cap;
        }
    }
}
