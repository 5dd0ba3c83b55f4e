// sed_plan.cpp — the planner (sed_plan.h): mode selection, every route, the layout of every buffer and the kernels'
// parameters of a batch, from the cost model, the options and the pairs.  No HIP call: it links without the HIP
// runtime.  Also the device-free entry points of include/sed.h (sed_plan_routes, sed_dot_factor, sed_band_*); fit
// search's planner and its device-free entry points are sed_fit_plan.cpp.
#include "sed_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

int sed_plan_fail(std::string *err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

namespace {

bool is_integral_small(double v, int lim) { return v == std::floor(v) && v >= 0 && v < lim; }

// ---- dot keys ----
// The CK forward kernel's update candidate can be one signed-byte dot product v_dot4_i32_i8(row vector of str1's
// symbol a, column vector of str2's symbol b, diagonal) when the addends H(a, b) = A*kappa(a, b) + 1 (kappa =
// insert + delete - cost(a -> b)) factor as sum_k r_k(a) c_k(b) over bytes in [-127, 127]: keys W = A*X + U
// (X = sum of kappa over the path's updates, U = its number of updates) are maximised with v_max3, so the cell is
// v_dot4 + v_max3 (2 VALU) instead of v_perm + v_add + v_min3.  Ordering: at a fixed cell a candidate with a larger
// X must win whatever the U's, i.e. A > the U spread of two candidates, which is below min(i, j) (kmax - kmin) /
// kmin because every update contributes kappa in [kmin, kmax]; the same bound makes X = floor(k kmax / (A kmax +
// 1)) recover X from k = A*X + U.
// Construction (rank 3 + one constant slot): with det/S = num/den (S = 1^T adj(K) 1), N = den*K - num*J has rank 3
// and left null vector v = 1^T adj(K); if some |v_g| = 1, row g of N is an integer combination of the other three.
// Slot 0 is the constant x*y = num*a + 1, slots 1..3 are a*N's rank-3 factorisation (coordinates P0 scaled by a1,
// rows of N scaled by a2, a1*a2 = a), so sum_k r_k c_k = num*a + 1 + a*(den K - num) = A K + 1 with A = den*a.
struct DotKeys {
    bool ok = false;
    uint32_t A = 0, kmax = 0, kmin = 0, M = 0, S = 0;
    uint32_t row[4] = {0, 0, 0, 0}, col[4] = {0, 0, 0, 0};
};
int64_t det3(const int64_t m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
int64_t gcd64(int64_t a, int64_t b) {
    a = a < 0 ? -a : a;
    b = b < 0 ? -b : b;
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}
// the byte vectors of a factorisation as the kernels' words (ladder keys add -(A*kappa + beta): negated columns)
void dot_pack_words(DotKeys &dk, const int8_t R[4][4], const int8_t C[4][4], bool negate_cols) {
    for (int i = 0; i < 4; ++i) {
        uint32_t rw = 0, cw = 0;
        for (int k = 0; k < 4; ++k) {
            rw |= (uint32_t)(uint8_t)R[i][k] << (8 * k);
            cw |= (uint32_t)(uint8_t)(int8_t)(negate_cols ? -C[i][k] : C[i][k]) << (8 * k);
        }
        dk.row[i] = rw;
        dk.col[i] = cw;
    }
}
// The rank-3 structure of a kappa table (dot_keys_search's first half): false when it has none.
struct DotRank3 {
    int64_t kmax, kmin, num, den, N[4][4], P0[4][3], pmax[3], qmax[3];
    int sr[3];
};
bool dot_rank3(const int64_t kap[4][4], DotRank3 &q) {
    q.kmax = 0;
    q.kmin = INT64_MAX;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            q.kmax = std::max(q.kmax, kap[a][b]);
            q.kmin = std::min(q.kmin, kap[a][b]);
        }
    if (q.kmin < 1 || q.kmax > 255) return false;
    // adjugate (adj[b][a] = cofactor(a, b)) and determinant
    int64_t adj[4][4], det = 0;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            int64_t m3[3][3];
            for (int i = 0, ii = 0; i < 4; ++i) {
                if (i == a) continue;
                for (int j = 0, jj = 0; j < 4; ++j) {
                    if (j == b) continue;
                    m3[ii][jj++] = kap[i][j];
                }
                ++ii;
            }
            adj[b][a] = (((a + b) & 1) ? -1 : 1) * det3(m3);
        }
    for (int b = 0; b < 4; ++b) det += kap[0][b] * adj[b][0];
    int64_t S = 0, v[4] = {0, 0, 0, 0};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            S += adj[a][b];
            v[b] += adj[a][b];  // v = 1^T adj(K)
        }
    if (S == 0) return false;
    q.num = det;
    q.den = S;
    if (q.den < 0) { q.num = -q.num; q.den = -q.den; }
    const int64_t gd = gcd64(q.num, q.den);
    if (gd > 1) { q.num /= gd; q.den /= gd; }
    int64_t gv = 0;
    for (int a = 0; a < 4; ++a) gv = gcd64(gv, v[a]);
    if (gv == 0) return false;
    for (int a = 0; a < 4; ++a) v[a] /= gv;
    int g = -1;
    for (int a = 0; a < 4; ++a)
        if (v[a] == 1 || v[a] == -1) { g = a; break; }
    if (g < 0) return false;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) q.N[a][b] = q.den * kap[a][b] - q.num;
    // slots 1..3 <-> rows s[0..2] != g: P0[a][k] = [a == s_k] (a != g), P0[g][k] = -v[s_k] / v[g]
    int ns = 0;
    for (int a = 0; a < 4; ++a)
        if (a != g) q.sr[ns++] = a;
    for (int k = 0; k < 3; ++k) {
        q.pmax[k] = q.qmax[k] = 0;
        for (int a = 0; a < 4; ++a) {
            q.P0[a][k] = a == g ? -v[q.sr[k]] * v[g] : (a == q.sr[k] ? 1 : 0);  // v[g] = +-1: 1/v[g] = v[g]
            q.pmax[k] = std::max(q.pmax[k], q.P0[a][k] < 0 ? -q.P0[a][k] : q.P0[a][k]);
        }
        for (int b = 0; b < 4; ++b)
            q.qmax[k] = std::max(q.qmax[k], q.N[q.sr[k]][b] < 0 ? -q.N[q.sr[k]][b] : q.N[q.sr[k]][b]);
    }
    // the rank-3 identity must hold exactly
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            int64_t t = 0;
            for (int k = 0; k < 3; ++k) t += q.P0[a][k] * q.N[q.sr[k]][b];
            if (t != q.N[a][b]) return false;
        }
    return true;
}
// kap: kappa[a][b] (>= 1); maxmin: the largest min(n, m) of the batch's wave pairs.
// Ladder mode (lad_amin > 0, lad_beta): the factorisation of A*K + lad_beta*J for the per-cell-code kernels'
// ladder keys with A >= lad_amin and A < 2^16 (dot_ladder below); no ordering bound or decode constants.
DotKeys dot_keys_search(const int64_t kap[4][4], int64_t maxmin, int64_t lad_amin, int64_t lad_beta) {
    const bool lad = lad_amin > 0;
    const int64_t beta = lad ? lad_beta : 1;
    DotKeys dk;
    DotRank3 q;
    if (!dot_rank3(kap, q)) return dk;
    const int64_t kmax = q.kmax, kmin = q.kmin, num = q.num, den = q.den;
    // the largest a with every slot within bytes (larger A leaves more room for long pairs)
    const int64_t a_hi = num != 0 ? (127 * 127 + 127) / (num < 0 ? -num : num) : 127 * 127;  // |num a + 1| <= 127^2
    for (int64_t a = a_hi; a >= 1; --a) {
        const int64_t A = den * a;
        if (lad ? A < lad_amin : A * kmin <= maxmin * (kmax - kmin)) break;  // fails for every smaller a too
        // ladder keys keep the rung c(i) and the op in the low 3 (wide: 4) bits of W = A*(D - i*delete - j*insert) +
        // u*(L - i - j) + B + c(i), u = 8 (16): A must be a multiple of u, or the D part leaks into them (a random GUI
        // table found this: insert 2 / delete 1 factored with A = 8835, and its scripts came out wrong)
        if (lad && (A >= 65536 || (A & lad_beta))) continue;  // (lad_beta + 1 = the L unit, 8 or 16)
        const int64_t J = num * a + beta;
        int64_t x = 0, y = 0;
        for (int64_t t = 1; t <= 127 && !x; ++t)
            if (J % t == 0 && (J / t >= -127 && J / t <= 127)) { x = t; y = J / t; }
        if (!x) continue;
        int64_t a1[3], a2[3];
        bool fit = true;
        for (int k = 0; k < 3 && fit; ++k) {
            a1[k] = 0;
            for (int64_t t = 1; t <= 127; ++t)
                if (a % t == 0 && t * q.pmax[k] <= 127 && (a / t) * q.qmax[k] <= 127) { a1[k] = t; break; }
            if (!a1[k]) fit = false;
            else a2[k] = a / a1[k];
        }
        if (!fit) continue;
        // decode: k * kmax < 2^29 over every real cell (k <= A * kmax * maxmin + maxmin)
        if (!lad && (A * kmax * maxmin + maxmin) * kmax >= (int64_t)1 << 29) continue;
        int8_t R[4][4], C[4][4];
        for (int i = 0; i < 4; ++i) {
            R[i][0] = (int8_t)x;
            C[i][0] = (int8_t)y;
            for (int k = 0; k < 3; ++k) {
                R[i][k + 1] = (int8_t)(a1[k] * q.P0[i][k]);
                C[i][k + 1] = (int8_t)(a2[k] * q.N[q.sr[k]][i]);
            }
        }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                int64_t t = 0;
                for (int k = 0; k < 4; ++k) t += (int64_t)R[i][k] * C[j][k];
                if (t != A * kap[i][j] + beta) return dk;
            }
        dk.A = (uint32_t)A;
        dk.kmax = (uint32_t)kmax;
        dk.kmin = (uint32_t)kmin;
        if (lad) {  // min-form ladder keys add -(A*kappa + beta): the column vectors are negated
            dot_pack_words(dk, R, C, true);
            // the virtual-column sentinel {s, 0, 0, 0} adds s x in [u, 490] (wide: [16, 480]): above every ladder jump
            // (at most +5, wide +13), and below the 512 the border leaves to 2^32 (sed_kernels.hip: SED_KB3)
            const int64_t lo = lad_beta + 1, hi = lad_beta == 15 ? 480 : 490;
            const int64_t sx = x > 0 ? (lo + x - 1) / x : 0;
            dk.ok = x > 0 && sx * x <= hi;
            dk.S = (uint32_t)sx;
            return dk;
        }
        const uint64_t Dd = (uint64_t)A * kmax + 1;
        int lg = 0;
        while (((uint64_t)1 << lg) < Dd) ++lg;
        dk.S = (uint32_t)(29 + lg);
        const uint64_t M = ((((uint64_t)1 << dk.S) / Dd) + 1) * (uint64_t)kmax;  // the kernels multiply k by M
        if (M >> 32 || dk.S < 32 || 4 * A >= (1 << 24)) return dk;
        dk.M = (uint32_t)M;
        dot_pack_words(dk, R, C, false);
        dk.ok = true;
        return dk;
    }
    return dk;
}
// dot_keys_search walks the factorisation's scale a down from ~16 000 / |num| with byte searches at every step (~75 us
// for user_costs on the build host): per-call batches (the GUI's script calls) would pay it before every launch, so
// the last few results are kept per thread, keyed by the whole input.
DotKeys dot_keys(const int64_t kap[4][4], int64_t maxmin, int64_t lad_amin = 0, int64_t lad_beta = 0) {
    struct Memo {
        int64_t kap[4][4], maxmin, amin, beta;
        DotKeys dk;
        bool used;
    };
    static thread_local Memo memo[4] = {};
    static thread_local int next = 0;
    for (Memo &e : memo)
        if (e.used && e.maxmin == maxmin && e.amin == lad_amin && e.beta == lad_beta &&
            std::memcmp(e.kap, kap, sizeof(e.kap)) == 0)
            return e.dk;
    Memo &e = memo[next];
    next = (next + 1) & 3;
    std::memcpy(e.kap, kap, sizeof(e.kap));
    e.maxmin = maxmin;
    e.amin = lad_amin;
    e.beta = lad_beta;
    e.dk = dot_keys_search(kap, maxmin, lad_amin, lad_beta);
    e.used = true;
    return e.dk;
}

int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// Mode selection.  The packed-integer kernel is exact when
// every value a cell can add is an integral positive Python float, or the int
// 0 of a match; then a cell's Python value is an int exactly when it is 0.
bool i32_eligible(const sed_costs &c) {
    if (c.K > 4) return false;
    if (c.ins_int || c.del_int) return false;
    if (!is_integral_small(c.ins, 256) || !is_integral_small(c.del, 256) || c.ins < 1 || c.del < 1) return false;
    // offset keys (sed_kernels.hip): the update constant cost - insert - delete - 1 is one byte
    // below 0xFF, i.e. 0 <= cost <= insert + delete <= 255
    if (c.ins + c.del > 255) return false;
    for (int e = 0; e < c.K * c.K; ++e) {
        const double v = c.sub[e];
        if (c.sub_int[e]) {
            if (v != 0) return false;
        } else if (!is_integral_small(v, 256) || v < 1 || v > c.ins + c.del) {
            return false;
        }
    }
    return true;
}

// 16-bit packed distance keys (i32x2 kernels) need every substitution strictly cheaper than
// delete + insert: their update constant cost - delete - insert is a 16-bit 0xFFxx.
bool x2_costs_ok(const sed_costs &c) {
    for (int a = 0; a < c.K; ++a)
        for (int bb = 0; bb < c.K; ++bb)
            if (a != bb && !(c.sub[a * c.K + bb] < c.ins + c.del)) return false;
    return true;
}

// Unit costs (insert = delete = 1, every mismatch 1, every match the int 0): the bit-parallel lane kernel
// (sed_lane.hip: sed_lane_bitpar_kernel) computes exactly the reference's distance.
bool unit_costs(const sed_costs &c) {
    if (c.K > 4 || c.ins_int || c.del_int || c.ins != 1.0 || c.del != 1.0) return false;
    for (int a = 0; a < c.K; ++a)
        for (int bb = 0; bb < c.K; ++bb) {
            const int e = a * c.K + bb;
            if (a == bb ? !(c.sub_int[e] && c.sub[e] == 0) : (c.sub_int[e] || c.sub[e] != 1.0)) return false;
        }
    return true;
}

// A set of at most 4 codes with unit costs among themselves (insert = delete = 1.0, every mismatch 1.0, every match
// the int 0), as a bit mask, greedily in code order; 0 when insert / delete are not 1.0.  A pair whose symbols all
// lie in it has the unit-cost distance whatever the other symbols cost (config 5 with N: the pairs without N).
// The first code always joins an empty set, so a pass that ends with that code alone starts again at the next one:
// codes follow the first occurrences of the batch's symbols, and a batch whose first symbol is N has the same subset
// as one whose first symbol is A.
uint32_t unit_subset(const sed_costs &c) {
    if (c.K > SED_MAX_K || c.ins_int || c.del_int || c.ins != 1.0 || c.del != 1.0) return 0;
    for (int first = 0; first + 1 < c.K; ++first) {
        uint32_t S = 0;
        int cnt = 0;
        for (int a = first; a < c.K && cnt < 4; ++a) {
            bool ok = c.sub_int[a * c.K + a] && c.sub[a * c.K + a] == 0;
            for (int bb = first; bb < a && ok; ++bb)
                if ((S >> bb) & 1u) {
                    const int e1 = a * c.K + bb, e2 = bb * c.K + a;
                    ok = !c.sub_int[e1] && c.sub[e1] == 1.0 && !c.sub_int[e2] && c.sub[e2] == 1.0;
                }
            if (ok) {
                S |= 1u << a;
                ++cnt;
            }
        }
        if (cnt >= 2) return S;
    }
    return 0;
}

// Dyadic costs over at most 8 symbols (sed_lane.hip: sed_lane_scaled_kernel): the smallest S = 2^k (k <= 8) that makes
// insert, delete and every update cost integral, with 1 <= insert * S, delete * S, 0 <= cost * S <= (insert + delete)
// * S <= 255 (the offset keys' update byte) and the lane block's n * delete + 32 * insert within the 16-bit D field.
// Simple typing is the caller's condition (every value a float, or the int 0 of a match).
bool scaled_costs(const sed_costs &c, sed_scaled_params *sp) {
    if (c.K > 8) return false;
    for (int k = 0; k <= 8; ++k) {
        const double S = std::ldexp(1.0, k);
        auto integral = [&](double v) { const double x = v * S; return x == std::floor(x) && x >= 0 && x <= 255; };
        bool ok = integral(c.ins) && integral(c.del) && c.ins * S >= 1 && c.del * S >= 1 &&
                  (c.ins + c.del) * S <= 255;
        for (int e = 0; e < c.K * c.K && ok; ++e) ok = integral(c.sub[e]) && c.sub[e] <= c.ins + c.del;
        if (!ok) continue;
        const uint32_t ins = (uint32_t)(c.ins * S), del = (uint32_t)(c.del * S);
        if ((double)SED_LANE_MAXN * del + (SED_LANE_MAXM + 1) * (double)ins > 65533.0) return false;
        *sp = sed_scaled_params{};
        sp->ins = ins;
        sp->del = del;
        sp->inv_scale = std::ldexp(1.0, -k);
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b) {
                const uint32_t v = (a < c.K && b < c.K) ? (uint32_t)(c.sub[a * c.K + b] * S) : 0u;
                sp->row[a][b >> 2] |= ((v - ins - del - 1u) & 0xFFu) << (8 * (b & 3));
            }
        return true;
    }
    return false;
}

int choose_R(int mode, int max_n, int forced) {
    if (forced) return forced;
    const int want = next_pow2(std::max(1, (max_n + 63) / 64));
    if (mode == SED_MODE_I32) return std::min(16, std::max(4, want));
    return std::min(8, std::max(4, want));
}

// fp64 wave kernel: R = 4 or 8 by a cost model over the batch, not by its longest pair.  A pair costs
// stripes(R) * (m + 63) steps of R rows plus a per-step overhead worth ~0.6 rows (fitted to the iupac workload,
// 1024^2: R = 8 5.01 ms, R = 4 5.34 ms).  The timing workload (lengths 10..500) then takes R = 4: 4.59 against
// 4.82 ms at R = 8 (profiles/r03/fp64_R.jsonl).
// lane: the batch routes short pairs to the fp64 lane kernel (plan_layout: use_lane), which never runs the wave
// kernel, so they are left out of the model.
// seg: pairs may run in 16-lane segments, four per wave (sed_kernels.hip: sed_wf_f64_kernel SW = 16): stripes of 16 R
// rows and a 15-step ramp, at a quarter of a wave: stripes16(R) * (m + 15) * (R + 0.6) / 4, times a penalty for the
// segments' per-lane loop control and stripe changes, fitted to the two fp64 workloads (profiles/r04/seg/ab_seg.jsonl):
// timing (R = 4) ran 3.34 against 4.48 ms where the bare model says 0.71 of it (penalty 1.05), iupac (1024^2, R = 8)
// 5.41 against 4.87 ms where it says 0.96 (penalty 1.16).
double f64_cost(int n, int m, int R, int SW) {
    const double pen = SW == 16 ? (R >= 8 ? 1.16 : 1.05) : 1.0;
    return (double)((n + SW * R - 1) / (SW * R)) * (m + SW - 1) * (R + 0.6) * SW / 64.0 * pen;
}
bool f64_seg_better(int n, int m, int R) { return f64_cost(n, m, R, 16) < f64_cost(n, m, R, 64); }
int choose_R_f64(const int32_t *len_a, const int32_t *len_b, int npairs, bool lane, bool seg) {
    double cost[2] = {0, 0};
    for (int p = 0; p < npairs; ++p) {
        if (lane && len_a[p] >= 1 && len_a[p] <= SED_LANE_MAXN && len_b[p] >= 1 && len_b[p] <= SED_LANE_MAXM) continue;
        for (int k = 0; k < 2; ++k) {
            const int R = 4 << k;
            const double c64 = f64_cost(len_a[p], len_b[p], R, 64);
            cost[k] += seg ? std::min(c64, f64_cost(len_a[p], len_b[p], R, 16)) : c64;
        }
    }
    return cost[1] < cost[0] ? 8 : 4;
}

// fp64 batches of several pairs: does the SPLIT route (R = 2) beat one wave per pair?  A SPLIT workgroup holds its slot
// for its pair's whole stripe chain, m + 63 steps plus ~64 steps of lag per stripe above it, so a batch whose stripes
// outnumber the resident workgroups (~256) runs in rounds, and long narrow pairs (n >> m) spend most of each round
// waiting on the lag.  The lone waves (one per pair, all resident) take the f64_cost units of their stripes.  Fitted to
// 32 batches of 16..256 pairs, 300..4000 rows, 100..2000 columns, scripts and distances (tools/fp64_split_batch.py,
// profiles/r06/fp64_split): the model picks the faster route in all 32; SPLIT lost up to 2.7x on 256 pairs of
// 2000 x 100 (1.34 against 0.49 ms) and won up to 3.8x on 64 pairs of 2000^2 (0.95 against 3.65 ms).
bool f64_split_pays(const int32_t *len_a, const int32_t *len_b, int npairs, bool script) {
    double lone = 0, lat_max = 0, slots = 0;
    for (int p = 0; p < npairs; ++p) {
        const int n = len_a[p], m = len_b[p];
        if (n <= 0 || m <= 0) continue;
        lone = std::max(lone, std::min(f64_cost(n, m, 4, 64), f64_cost(n, m, 8, 64)));
        const double ns = (double)((n + 127) / 128), lat = (double)m + 63.0 + 64.0 * ns;
        lat_max = std::max(lat_max, lat);
        slots += ns * lat;
    }
    const double t_split = (script ? 0.318 : 0.138) + (script ? 7.40e-5 : 6.53e-5) * std::max(lat_max, slots / 256.0);
    const double t_lone = (script ? 0.359 : 0.140) + (script ? 5.44e-5 : 5.09e-5) * lone;
    return t_split < t_lone;
}

// The planner's working set: the inputs, and what one step hands to the next beside the plan itself.
struct Planning {
    const sed_costs &c;
    const sed_opts &o;
    const uint8_t *codes_a;
    const int64_t *off_a;
    const int32_t *len_a;
    const uint8_t *codes_b;
    const int64_t *off_b;
    const int32_t *len_b;
    const int npairs;
    const uint32_t flags;
    sed_plan &b;
    std::string *err;
    int max_n = 0, max_m = 0;
    bool want_tb = false, f64_lane = false, seg_ok = false, use_lane = false;
    double in_bytes = 0, tb_bytes = 0;
    double sum_nm = 0, sum_len = 0;  // sum n m and sum (n + m) over the pairs
    uint64_t aw = 0, bw = 0;  // the sequences' words (integer mode) or bytes
    std::vector<uint64_t> diag_ub;  // every pair's diagonal bound where the rows-per-lane rule took it (else empty)

    // the automatic rows per lane of an fp64 batch
    int auto_R_f64(int mode) const {
        return choose_R_f64(len_a, len_b, npairs, f64_lane && mode == SED_MODE_F64, seg_ok);
    }
    // ---- the routes' conditions, each asked by the step that decides the route and by the rows-per-lane rule of
    // banded checkpoint batches (band_rows_rule), which runs before those steps ----
    // integer SPLIT (plan_mode): forced, or a batch too small to fill the GPU with one wave per pair
    bool i32_split() const {
        return o.split != 2 && (o.split == 1 || (npairs <= 256 && max_n > 256 && o.chain != 1 && o.chain < 3));
    }
    // offset keys at R rows per lane (plan_mode): i*delete + j*insert over every computed cell (padded rows, the
    // columns the wave or the lane kernel runs past m) must stay below the bias, and L < 2^14
    bool i32_fits(int R) const {
        const int ROWS = 64 * R;
        for (int p = 0; p < npairs; ++p) {
            const double npad = (double)((len_a[p] + ROWS - 1) / ROWS) * ROWS;
            const double cols = (double)std::max(len_b[p] + 64 + 64 / R, SED_LANE_MAXM);
            if (npad * c.del + cols * c.ins > 65533.0 || npad + cols >= 16384.0) return false;
        }
        return true;
    }
    // the lane-per-pair kernels take the batch's short pairs (plan_layout)
    bool lane_route(int mode, bool split) const {
        return !split && o.lane != 2 && (mode == SED_MODE_I32 || (mode == SED_MODE_F64 && !want_tb && (flags & SED_NO_LEN)));
    }
    // pair p is one of them.  A batch of a few pairs (the per-call path) leaves the GPU empty, so one lane walking a
    // pair alone only pays off for a small distance-only pair: a 30-nt script call took 42 us on the lane kernel and
    // 34 us on the wave kernels, a 30-nt distance call 19 against 22 us (tools/zc_ab.py SED_OPT_LANE, profiles/r05/s38)
    bool lane_pair(int p, bool lane_on) const {
        const int nn = len_a[p], mm = len_b[p];
        const bool few_pairs = npairs <= 16 && o.lane == 0;
        return lane_on && nn >= 1 && nn <= SED_LANE_MAXN && mm >= 1 && mm <= SED_LANE_MAXM &&
               !(few_pairs && (want_tb || (double)nn * mm > 1024.0));
    }
    // CK traceback (plan_traceback; R = 4/8/16 wave kernels, stripe or CHAIN, not SPLIT).  Auto: batches past the
    // window kernel's 256 pairs whose pairs are large enough.  The forward kernel saves ~1.7 VALU per cell (n m), the
    // tile recompute costs per path step (n + m): measured, config 4 (4096^2) step 20.4 -> 15.0 ms, config 3 (512^2)
    // 2.90 -> 4.40 ms; break-even near 1024^2, i.e. sum(n m) / sum(n + m) = 512.
    bool ck_route(int mode, bool split, int R) const {
        return want_tb && mode == SED_MODE_I32 && !split && (R == 4 || R == 8 || R == 16) && o.tb != 1 &&
               (o.tb == 2 || (npairs > 256 && sum_nm >= 512.0 * sum_len));
    }
    // CHAIN (plan_chain) runs at R = 4 or 8, wave pairs of one stripe with no empty side
    bool chain_R(int R) const { return o.chain != 2 && (R == 4 || R == 8); }
    bool chain_pair(int p, int R) const { return len_a[p] >= 1 && len_a[p] <= 64 * R && len_b[p] >= 1; }
    // band pruning of a checkpoint batch of the stripe kernel (plan_band): not switched off, and substitution costs
    // >= 0 over at most 4 symbols (the window's lower bound counts indels only)
    bool band_costs_ok() const {
        if (!(c.K <= 4 && c.ins + c.del > 0)) return false;
        for (int e = 0; e < c.K * c.K; ++e)
            if (!(c.sub[e] >= 0)) return false;
        return true;
    }
    bool band_route() const { return o.band != 2 && o.env_band != 0 && band_costs_ok(); }
    // kappa = insert + delete - cost, the dot keys' table
    void kappa(int64_t kap[4][4]) const {
        for (int a = 0; a < 4; ++a)
            for (int bb = 0; bb < 4; ++bb) kap[a][bb] = (int64_t)b.ip.ins + b.ip.del - (int64_t)c.sub[a * 4 + bb];
    }
};

// Rows per lane of a banded checkpoint batch ("Rows per lane").  A stripe of 64 R rows sweeps its
// window in about 64 R + 2w steps (w = the band's half-width), of which a lane does in-band work in about 2w: with
// a narrow band most of a tall stripe's steps are its two triangular corners, and a shorter stripe computes fewer
// cells the result does not need.  Against that a step of R rows costs R cells plus a fixed part (the lane-to-lane
// move, the top-row read, the loop), and every stripe pays its prologue (the refinement scan of the row above, the
// checkpoint set-up).  The model counts, for R = 16, 8 and 4, the steps of every wave pair's stripes from the static
// windows (as plan_band counts band_cells) and takes
//     cost(R) = steps(R) (R + BAND_STEP_C[R]) + stripes(R) BAND_STRIPE_C        (in rows of one step)
// summed over the batch.  Fitted to the step times of 8192 x 4096^2 and 16384 x 2048^2 forced to each R, three
// interleaved rounds (profiles/rows_rule/README.md, "Fit"): step = T0(shape) + 3.43e-9 ms x cost with one step
// constant for every R leaves residuals of at most 0.010 ms (the runs' widest range is 0.027 ms), and 3.43e-9 ms is
// 8.4 cycles of one of 1024 SIMDs at 2.4 GHz, the cell's two VALU ops.  Measured against modelled gains: 4096^2
// 16 -> 8 0.571 against 0.584 ms and 8 -> 4 0.140 against 0.130; 2048^2 0.466 against 0.448 and 0.133 against 0.146.
// A smaller R wins only by more than BAND_RESOLVE of the larger one's cost.  The project's criterion for two runs
// to differ (ten times the wider range, here 0.27 ms) is 7 to 11 % of the modelled R = 8 forward of the two shapes,
// and by it R = 4 and R = 8 could not be told apart on either (cost ratios 0.96 and 0.94): the larger R then
// stands, with half the stripes and smaller checkpoints.
const double BAND_STEP_C[3] = {0.1, 0.1, 0.1};  // R = 16, 8, 4
const double BAND_STRIPE_C = 800.0;
const double BAND_RESOLVE = 0.10;
// The rule applies to batches whose wave pairs all have at least two full R = 16 stripes: a shorter pair is one
// full stripe and a padded remainder or less, and no run has measured the rule there.
const int BAND_RULE_MIN_ROWS = 2 * 64 * 16;

double band_rows_cost(int n, int m, int R, double step_c, sed_band w) {
    const sed_geom g = sed_stripe_geom(n, m, R, 64);
    double steps = 0;
    for (int k = 0; k < g.nstripes; ++k) {
        int clo, chi;
        sed_band_chunks(n, m, 64 * R, g.nchunks, w, k, &clo, &chi);
        steps += (double)(std::min(g.SG, 64 * (chi + 1)) - 64 * clo);
    }
    return steps * (R + step_c) + (double)g.nstripes * BAND_STRIPE_C;
}

// The automatic R of an integer batch: R0 (choose_R's), or the model's choice when the batch will run the checkpoint
// route on the stripe kernel with band pruning at every candidate.  Leaves the pairs' diagonal bounds in P.diag_ub
// when it ran the model.
int band_rows_rule(Planning &P, int R0) {
    static const int cand[3] = {16, 8, 4};
    if (R0 != 16 || P.i32_split() || !P.band_route()) return R0;
    const bool lane_on = P.lane_route(SED_MODE_I32, false);
    int nwave = 0;
    for (int p = 0; p < P.npairs; ++p) {
        if (P.len_a[p] <= 0 || P.len_b[p] <= 0 || P.lane_pair(p, lane_on)) continue;
        if (P.len_a[p] < BAND_RULE_MIN_ROWS) return R0;  // the gate
        ++nwave;
    }
    if (!nwave) return R0;
    bool ok[3];
    for (int k = 0; k < 3; ++k) {
        const int R = cand[k];
        ok[k] = P.ck_route(SED_MODE_I32, false, R) && P.i32_fits(R);
        // CHAIN would take the wave pairs off the stripe kernel (it never does past the gate: a pair of 2048 rows is
        // no single stripe at R = 4 or 8)
        bool chain = P.chain_R(R);
        for (int p = 0; p < P.npairs && chain; ++p)
            if (!P.lane_pair(p, lane_on) && !P.chain_pair(p, R)) chain = false;
        if (chain) ok[k] = false;
    }
    if (!ok[0]) return R0;
    const sed_band_params bp = sed_band_params_from(P.c);
    double cost[3] = {0, 0, 0};
    P.diag_ub.assign(P.npairs, 0);
    for (int p = 0; p < P.npairs; ++p) {
        const int nn = P.len_a[p], mm = P.len_b[p];
        if (nn <= 0 || mm <= 0 || P.lane_pair(p, lane_on)) continue;
        P.diag_ub[p] = sed_band_diag_bound(bp, P.codes_a + P.off_a[p], nn, P.codes_b + P.off_b[p], mm);
        const sed_band w = sed_band_window(nn, mm, bp.ins, bp.del, P.diag_ub[p]);
        for (int k = 0; k < 3; ++k)
            if (ok[k]) cost[k] += band_rows_cost(nn, mm, cand[k], BAND_STEP_C[k], w);
    }
    int best = 0;
    for (int k = 1; k < 3; ++k)
        if (ok[k] && cost[k] < cost[best] * (1.0 - BAND_RESOLVE)) best = k;
    return cand[best];
}

int plan_validate(Planning &P) {
    if (P.npairs < 0 ||
        (P.npairs > 0 && (!P.codes_a || !P.off_a || !P.len_a || !P.codes_b || !P.off_b || !P.len_b)))
        return sed_plan_fail(P.err, SED_E_ARG, "bad batch arguments");
    for (int p = 0; p < P.npairs; ++p) {
        if (P.len_a[p] < 0 || P.len_b[p] < 0) return sed_plan_fail(P.err, SED_E_ARG, "negative length at pair %d", p);
        P.max_n = std::max(P.max_n, P.len_a[p]);
        P.max_m = std::max(P.max_m, P.len_b[p]);
        P.sum_nm += (double)P.len_a[p] * P.len_b[p];
        P.sum_len += (double)P.len_a[p] + P.len_b[p];
        const uint8_t *pa = P.codes_a + P.off_a[p], *pb = P.codes_b + P.off_b[p];
        for (int i = 0; i < P.len_a[p]; ++i)
            if (pa[i] >= P.c.K) return sed_plan_fail(P.err, SED_E_ARG, "code %d >= K at pair %d", pa[i], p);
        for (int j = 0; j < P.len_b[p]; ++j)
            if (pb[j] >= P.c.K) return sed_plan_fail(P.err, SED_E_ARG, "code %d >= K at pair %d", pb[j], p);
    }
    return SED_OK;
}

// ---- mode, rows per lane, SPLIT ----
int plan_mode(Planning &P) {
    const sed_costs &c = P.c;
    const sed_opts &o = P.o;
    const int32_t *len_a = P.len_a, *len_b = P.len_b;
    const int npairs = P.npairs;
    const uint32_t flags = P.flags;
    int mode;
    const bool elig = i32_eligible(c);
    switch (o.mode) {
    case 1:
        if (!elig) return sed_plan_fail(P.err, SED_E_RANGE, "costs are not eligible for the integer kernel");
        mode = SED_MODE_I32;
        break;
    case 2: mode = sed_simple_typing(c) ? SED_MODE_F64 : SED_MODE_F64_TYPED; break;
    case 3: mode = SED_MODE_F64_TYPED; break;
    default: mode = elig ? SED_MODE_I32 : (sed_simple_typing(c) ? SED_MODE_F64 : SED_MODE_F64_TYPED);
    }
    // fp64 batches whose short pairs go to the lane kernel (use_lane below: distance only, simple typing)
    P.f64_lane = o.lane != 2 && !(flags & SED_WANT_SCRIPT) && (flags & SED_NO_LEN) && sed_simple_typing(c);
    // fp64 batches of more than 256 wave pairs may run short pairs in 16-lane segments (SED_OPT_SEG; the window
    // traceback of smaller batches reads the 64-lane layout only)
    int nwave_f64 = 0;
    double lane_cells_f64 = 0;  // the largest fp64 lane pair (n m): one lane walks all of it
    for (int p = 0; p < npairs; ++p) {
        if (len_a[p] <= 0 || len_b[p] <= 0) continue;
        if (P.f64_lane && len_a[p] <= SED_LANE_MAXN && len_b[p] <= SED_LANE_MAXM)
            lane_cells_f64 = std::max(lane_cells_f64, (double)len_a[p] * len_b[p]);
        else
            ++nwave_f64;
    }
    P.seg_ok = o.seg != 2 && nwave_f64 > 256;
    int R = (mode == SED_MODE_I32 || o.R) ? choose_R(mode, P.max_n, o.R) : P.auto_R_f64(mode);
    if (mode == SED_MODE_I32) {
        if (!o.R) R = band_rows_rule(P, R);
        if (!P.i32_fits(R)) {  // (the keys' range at the R the batch runs)
            if (o.mode == 1) return sed_plan_fail(P.err, SED_E_RANGE, "integer key would overflow (D < 2^16, L < 2^14)");
            mode = sed_simple_typing(c) ? SED_MODE_F64 : SED_MODE_F64_TYPED;
            // (a forced R the fp64 kernels do not have, 16 or 32, asked for the integer kernel this batch cannot run:
            // the fallback picks its own, as it does unforced, instead of failing the batch)
            R = (o.R == 2 || o.R == 4 || o.R == 8) ? o.R : P.auto_R_f64(mode);
        }
    } else if (c.K > SED_MAX_K) {
        return sed_plan_fail(P.err, SED_E_ALPHABET, "alphabet of %d symbols exceeds %d", c.K, SED_MAX_K);
    }
    if (mode == SED_MODE_I32 ? !(R == 4 || R == 8 || R == 16 || R == 32) : !(R == 2 || R == 4 || R == 8))
        return sed_plan_fail(P.err, SED_E_ARG, "unsupported rows-per-lane %d for mode %d", R, mode);
    // SPLIT (integer kernel): one wave per stripe with inter-workgroup hand-offs, for
    // batches too small to fill the GPU with one wave per pair (config 2, GUI calls).
    bool split = false;
    if (mode == SED_MODE_I32 && o.split != 2) {
        split = P.i32_split();
        if (split && !o.R) R = 4;
        if (split && R != 4 && R != 8 && R != 16 && R != 32) split = false;
    } else if (mode != SED_MODE_I32 && o.split != 2 && (!P.seg_ok || o.split == 1)) {
        // fp64 SPLIT (sed_wf_f64_split_kernel, R = 4): batches of few pairs, whose lone fp64 waves are otherwise one
        // SIMD each.  It also runs the one-stripe pairs (tools/fp64_call_scaling.py, profiles/r05/s25: 30 nt 39.9
        // against 40.6 us per call, 200 nt 72 against 87, 500 nt 151 against 255, 2000 nt 544 against 3497), since
        // its lone wave reads each step's table entries a step ahead; distance-only batches whose pairs all fit the
        // lane kernels keep those
        // R = 2 by default: a lone fp64 wave is issue-bound (~80 VALU per step at R = 4), so halving the rows per
        // step outweighs the twice as many hand-offs (per call, 500^2: 150 us at R = 4, tools/fp64_call_scaling.py)
        // A lane pair past 256 cells also goes SPLIT: 30^2 distance-only took 45 us per call on the lane kernel,
        // 32 us SPLIT (10^2: 27 against 33 us)
        split = (o.split == 1 || (npairs <= 256 && (nwave_f64 > 0 || lane_cells_f64 > 256.0) &&
                                  (npairs == 1 || f64_split_pays(len_a, len_b, npairs, (flags & SED_WANT_SCRIPT) != 0)))) &&
                (!o.R || o.R == 2 || o.R == 4);
        if (split) R = o.R ? o.R : 2;
        // (automatic route: its hand-off words, 24 B per column and stripe, stay under 4 GB)
        if (split && o.split != 1 && !o.R) {
            double words = 0;
            for (int p = 0; p < npairs; ++p) {
                const double st = (double)((len_a[p] + 64 * R - 1) / (64 * R)), ch = (double)((len_b[p] + 127) / 64 + 2);
                if (st > 1) words += st * ch * 64.0 * 6.0;
            }
            if (4.0 * words > 4e9) {
                split = false;
                R = P.auto_R_f64(mode);
            }
        }
    }
    if (split && mode != SED_MODE_I32) P.seg_ok = false;  // (SED_OPT_SPLIT = 1 over the segments of > 256 wave pairs)
    // rows per lane 2 is the fp64 SPLIT route's; an fp64 batch that does not take it runs the automatic R
    if (mode != SED_MODE_I32 && R == 2 && !split) R = P.auto_R_f64(mode);
    P.b.split = split;
    P.b.mode = mode;
    P.b.R = R;
    return SED_OK;
}

// ---- the traceback's route ----
void plan_traceback(Planning &P) {
    const sed_opts &o = P.o;
    sed_plan &b = P.b;
    const int R = b.R, mode = b.mode, npairs = P.npairs;
    const bool want_tb = P.want_tb;
    // CK traceback: distance-key forward kernel + checkpoints, traceback recomputes tiles (Planning::ck_route)
    b.ck = P.ck_route(mode, b.split, R);
    // SED_PIPELINE is a hint: checkpoint batches run their traceback after the DP on one stream (in parts on
    // several, sed_plan_run).  Both kernels are issue-bound, so overlapping a run's traceback with the next run's
    // forward only adds contention (config 4: 20.33 ms sequential against 20.5-20.8 ms pipelined in round 1,
    // profiles/r01_ck/ab_pipeline.jsonl; 11.13 against 9.78 ms for 2 pipelined parts in round 5,
    // profiles/r05/s14/ab.jsonl) and saves two checkpoint buffers.
    b.nbuf = (P.flags & SED_PIPELINE) ? 3 : 1;
    if (b.ck) b.nbuf = 1;
    // few pairs with per-cell codes (config 2, the GUI): the traceback walks the stripes of a pair in parallel
    // (a map of every stripe's exits, then one wave per stripe segment) instead of one ~n+m step chain;
    // SED_TBPAR=0/1 overrides (A/B)
    // (never with fp64 pairs in 16-lane segments: the stripe kernels read the 64-lane code layout only)
    b.tbpar = want_tb && !b.ck && (R == 4 || R == 2) && (o.env_tbpar < 0 ? npairs <= 64 : o.env_tbpar > 0) &&
              !(P.seg_ok && mode != SED_MODE_I32);
    b.tbpar_items = b.tbpar_kmax = 0;
    // SPLIT script batches: checkpoints + a tile-parallel recompute of the codes (dot or distance keys in the forward:
    // 2-3 VALU per cell against the ladder keys' 5.2 on the latency-bound stripe chain)
    b.split_ck = want_tb && b.split && mode == SED_MODE_I32 && R == 4 && o.splitck != 2;
    b.ck_tiles = 0;
}

// ---- layout: every pair's descriptor, the word counts, the lane / segment / task lists ----
void plan_layout(Planning &P) {
    const sed_opts &o = P.o;
    sed_plan &b = P.b;
    const int R = b.R, mode = b.mode, npairs = P.npairs;
    const bool want_tb = P.want_tb, split = b.split;
    b.pd.assign(npairs, sed_pair_desc{});
    b.tasks.clear();
    b.lane.clear();
    b.seg.clear();
    // lane-per-pair kernels: integer keys (any flags), or fp64 distance-only in "simple typing" mode
    P.use_lane = P.lane_route(mode, split);
    uint64_t aw = 0, bw = 0, tbw = 0, bndw = 0, opw = 0, mapw = 0;
    const bool packed = (mode == SED_MODE_I32);
    double cells = 0, in_bytes = 0, ck_bytes = 0;
    for (int p = 0; p < npairs; ++p) {
        const int nn = P.len_a[p], mm = P.len_b[p];
        sed_pair_desc &d = b.pd[p];
        d.n = nn;
        d.m = mm;
        d.a_off = aw;
        d.b_off = bw;
        if (packed) {
            aw += (nn + 15) / 16;
            bw += (mm + 15) / 16;
        } else {  // bytes, each sequence 16-byte aligned (the lane kernels read str2 as two 16-byte words)
            aw += ((uint64_t)nn + 15) & ~(uint64_t)15;
            bw += ((uint64_t)mm + 15) & ~(uint64_t)15;
        }
        d.tb_off = tbw;
        d.bnd_off = bndw;
        d.ops_off = opw;
        d.map_off = (int32_t)mapw;  // stripe-parallel traceback: this pair's exit map
        if (P.lane_pair(p, P.use_lane)) {
            d.lane = 1;
            b.lane.push_back(p);
            if (want_tb) tbw += 2 * (uint64_t)nn;  // one uint2 of 2-bit ops per row
        } else if (nn > 0 && mm > 0) {
            // fp64 pairs the cost model prefers in 16-lane segments (sed_kernels.hip: sed_wf_f64_kernel SW = 16)
            const bool seg = !packed && P.seg_ok && (o.seg == 1 || f64_seg_better(nn, mm, R));
            const uint64_t SW = seg ? 16 : 64;
            if (seg) {
                d.pad[1] = 1;
                b.seg.push_back(p);
            }
            const uint64_t G = 64 / R;  // steps per 16-byte traceback group (sed_kernels.hip: Grp)
            const sed_geom g = sed_stripe_geom(nn, mm, R, (int)SW);
            const uint64_t nstripes = g.nstripes, SG = g.SG, nchunks = g.nchunks;
            if (want_tb) {  // CK: per stripe nchunks x (R+1) x 64 column checkpoints + (SG/G) x 64 row checkpoints
                const uint64_t wck = nstripes * (nchunks * (R + 1) * 64 + (SG / G) * SED_CK_RW);
                const uint64_t w = b.ck ? wck : nstripes * (SG / G) * SW * 4 + (b.split_ck ? wck : 0);
                tbw += w;
                ck_bytes += 4.0 * (double)w;
                if (b.split_ck) b.ck_tiles = std::max<int>(b.ck_tiles, (int)(nstripes * R * nchunks));
            }
            // SPLIT: 64-bit {epoch tag, value} words per column and stripe (the tagged hand-off, sed_kernels.hip)
            // (fp64: D, L and T planes; SPLIT: three 64-bit {tag, D low | D high | L key and T} words)
            if (nstripes > 1) bndw += (nchunks + 2) * SW * (packed ? (split ? 2 : 1) : (split ? 6 : 4)) * (split ? nstripes : 1);
            if (b.tbpar && nstripes >= 3) {  // {exit column, ops} per stripe and column, then per 64-row band and column
                const uint64_t nbands = ((uint64_t)nn + 63) / 64 - 1;  // bands 1 .. nbt-1 (the banded emit's)
                mapw += (nstripes + nbands) * (uint64_t)(mm + 1) * 2;
                // band map: workgroups of 256 columns per band (a superset of the stripe map kernel's middle
                // stripes + sink; the compose kernel's grid is derived from it, sed_launch_traceback_stripes)
                b.tbpar_items = std::max<int>(b.tbpar_items, (int)(nbands * ((mm + 256) / 256) * 256));
            }
            b.tbpar_kmax = std::max<int>(b.tbpar_kmax, (int)(nstripes >= 3 ? nstripes : 1));
            if (split) {
                for (uint64_t k = 0; k < nstripes; ++k) b.tasks.push_back(make_int2(p, (int)k));
            }
        } else if (split) {
            b.tasks.push_back(make_int2(p, 0));
        }
        if (b.tbpar && !d.lane) {
            b.tbpar_items = std::max<int>(b.tbpar_items, (nn + mm + 15) / 16);  // the map kernel zeroes these
            b.tbpar_kmax = std::max(b.tbpar_kmax, 1);
        }
        opw += (uint64_t)(nn + mm + 15) / 16;
        cells += (double)nn * mm;
        in_bytes += packed ? (nn + mm) / 4.0 : (double)(nn + mm);
    }
    // a SPLIT script batch whose pairs all have an empty side has no tile to recompute: plain per-cell codes (the
    // traceback walks only the border)
    if (b.split_ck && b.ck_tiles == 0) b.split_ck = false;
    // no pair with 3 stripes or more: the stripe map has nothing to do and the emit kernel walks every pair in one
    // segment, as the window traceback does without the map launch and the OR into zeroed scripts (so zero-copy
    // results apply)
    if (b.tbpar && b.tbpar_kmax < 3 && o.env_tbpar < 0) {
        b.tbpar = false;
        b.tbpar_items = b.tbpar_kmax = 0;
    }
    // algorithmic traceback bytes: the 2-bit choice of every cell, or (CK) the checkpoints written
    P.tb_bytes = b.ck ? ck_bytes : cells * 0.25;
    P.in_bytes = in_bytes;
    P.aw = aw;
    P.bw = bw;
    b.tb_words = tbw;
    b.bnd_words = bndw;
    b.map_words = mapw;
    b.ops_words = opw;
    b.cells = cells;
    b.ntasks = (int)b.tasks.size();
    b.nlane = (int)b.lane.size();
    b.nwave = npairs - b.nlane;
    // segment pairs by shape, so the four pairs of a wave run alike
    const int32_t *len_a = P.len_a, *len_b = P.len_b;
    std::stable_sort(b.seg.begin(), b.seg.end(), [&](int32_t x, int32_t y) {
        return len_a[x] != len_a[y] ? len_a[x] < len_a[y] : len_b[x] < len_b[y];
    });
    b.nseg = (int)b.seg.size();
}

// ---- the lane pairs' kernel: bit-parallel, scaled-integer, two per lane ----
void plan_lane_routes(Planning &P, bool x2_ok) {
    const sed_costs &c = P.c;
    const sed_opts &o = P.o;
    sed_plan &b = P.b;
    const int mode = b.mode;
    const int32_t *len_a = P.len_a;
    const bool dist_only = !P.want_tb && (P.flags & SED_NO_LEN);
    // distance-only integer lane pairs: two pairs of equal n per lane (sed_lane.hip: i32x2). Stable
    // sort by n, pair neighbours of equal n; a pair without a partner shares its lane with itself.
    b.nlane_x2 = 0;
    // unit costs: one pair per lane, bit-parallel (~18 word ops per str1 symbol instead of 2 per cell)
    b.lane_bitpar = mode == SED_MODE_I32 && dist_only && o.bitpar != 2 && !b.lane.empty() && unit_costs(c);
    // fp64 lane pairs whose symbols all lie in a unit-cost subset: bit-parallel inside the fp64 lane kernel, first
    // in the lane list so that waves stay uniform
    b.umask = 0;
    b.nbitpar_f64 = 0;
    if (mode == SED_MODE_F64 && P.use_lane && dist_only && o.bitpar != 2 && !b.lane.empty() &&
        (b.umask = unit_subset(c)) != 0) {
        auto inside = [&](const uint8_t *s, int len) {
            for (int i = 0; i < len; ++i)
                if (!((b.umask >> s[i]) & 1u)) return false;
            return true;
        };
        for (int32_t x : b.lane)
            if (inside(P.codes_a + P.off_a[x], len_a[x]) && inside(P.codes_b + P.off_b[x], P.len_b[x])) {
                b.pd[x].pad[0] = 1;
                ++b.nbitpar_f64;
            }
        std::stable_partition(b.lane.begin(), b.lane.end(), [&](int32_t x) { return b.pd[x].pad[0] != 0; });
    }
    // fp64 lane pairs under dyadic costs over <= 8 symbols: the scaled-integer lane kernel (exact, 3 VALU per cell)
    b.scaled = mode == SED_MODE_F64 && P.use_lane && dist_only && o.scaled != 2 && !b.lane.empty() &&
               scaled_costs(c, &b.sp);
    if (b.scaled) {
        b.sp.umask = b.umask;
        b.sp.umap = 0;  // 2-bit unit-subset code of every code < 8 (the bit-parallel pairs)
        for (uint32_t cc = 0; cc < 8; ++cc)
            if ((b.umask >> cc) & 1u) b.sp.umap |= (uint32_t)__builtin_popcount(b.umask & ((1u << cc) - 1u)) << (2 * cc);
    }
    // 16-bit offset keys: n*delete + 32*insert (the lane kernel's whole block) within 0xFFFF
    // (never false in an integer batch: i32_fits already holds n*delete + 32*insert < 65533, its cols >= m + 68 > 32)
    bool lane_fit16 = true;
    for (int32_t x : b.lane)
        if ((double)len_a[x] * c.del + SED_LANE_MAXM * c.ins > 65535.0) lane_fit16 = false;
    if (x2_ok && lane_fit16 && !b.lane_bitpar && dist_only && o.pack != 2 && !b.lane.empty()) {
        std::stable_sort(b.lane.begin(), b.lane.end(), [&](int32_t x, int32_t y) { return len_a[x] < len_a[y]; });
        std::vector<int32_t> &two = b.tmp;
        two.clear();
        two.reserve(b.lane.size() + 1);
        for (size_t q = 0; q < b.lane.size();) {
            const int32_t x = b.lane[q];
            const bool partner = q + 1 < b.lane.size() && len_a[b.lane[q + 1]] == len_a[x];
            two.push_back(x);
            two.push_back(partner ? b.lane[q + 1] : x);
            q += partner ? 2 : 1;
        }
        b.lane.swap(two);
        b.nlane_x2 = (int)(b.lane.size() / 2);
    }
}

// distance-only integer wave pairs: two of equal n per wave (sed_kernels.hip: i32x2), the one with
// the larger m first (its bottom-row buffer serves both).  Partners come from a (n, m) sort and
// must have 3 min(m) > max(m): the wave runs max(m) columns at 4 ops per 2 cells, which beats 3 ops
// per cell of each pair alone while 4 max(m) < 3 (m_P + m_Q).  Packed pairs are marked lane = 2,
// so the other wave kernels (and CHAIN mode) skip them.
void plan_wave_x2(Planning &P, bool x2_ok) {
    const sed_costs &c = P.c;
    sed_plan &b = P.b;
    const int32_t *len_a = P.len_a, *len_b = P.len_b;
    const int R = b.R, ROWS = 64 * R;
    b.x2.clear();
    b.nwave_x2 = 0;
    if (!(x2_ok && !b.split && !P.want_tb && (P.flags & SED_NO_LEN) && P.o.pack != 2 && b.nwave > 1)) return;
    std::vector<int32_t> &w = b.tmp;
    w.clear();
    for (int p = 0; p < P.npairs; ++p) {
        // 16-bit offset keys over the wave's block: padded rows x (m + 63 + G) columns within 0xFFFF
        const double npad = (double)((len_a[p] + ROWS - 1) / ROWS) * ROWS;
        const bool fit16 = npad * c.del + (double)(len_b[p] + 64 + 64 / R) * c.ins <= 65535.0;
        if (!b.pd[p].lane && len_a[p] > 0 && len_b[p] > 0 && fit16) w.push_back(p);
    }
    std::stable_sort(w.begin(), w.end(), [&](int32_t x, int32_t y) {
        return len_a[x] != len_a[y] ? len_a[x] < len_a[y] : len_b[x] < len_b[y];
    });
    for (size_t q = 0; q + 1 < w.size();) {
        const int32_t x = w[q], y = w[q + 1];  // len_b[x] <= len_b[y]
        if (len_a[x] == len_a[y] && 3LL * len_b[x] > len_b[y]) {
            b.x2.push_back(y);
            b.x2.push_back(x);
            b.pd[x].lane = b.pd[y].lane = 2;
            q += 2;
        } else {
            ++q;
        }
    }
    b.nwave_x2 = (int)(b.x2.size() / 2);
    b.nwave -= (int)b.x2.size();
}

// ---- CHAIN mode (integer keys): single-stripe wave pairs run back to back, one chain per
// wave, so each pair's 63-step ramp overlaps the previous pair's drain (sed_kernels.hip) ----
// b.chain = [the chains' pairs | static chains: chain c runs pairs [off[c], off[c + 1])]
void plan_chain(Planning &P) {
    const sed_opts &o = P.o;
    sed_plan &b = P.b;
    const int32_t *len_b = P.len_b;
    const int npairs = P.npairs, R = b.R;
    b.chain.clear();
    b.nchains = 0;
    b.chain_npairs = 0;
    b.chain_dyn = false;
    if (!(b.mode == SED_MODE_I32 && !b.split && P.chain_R(R) && b.nwave > 0)) return;
    // SIMDs x the chain kernel's waves per SIMD, unless capped (tests: several fetched pairs per wave)
    const int resident = o.chain_waves > 0 ? o.chain_waves : 1024 * 5;
    bool ok = true;
    for (int p = 0; p < npairs && ok; ++p)
        if (!b.pd[p].lane && !P.chain_pair(p, R)) ok = false;
    if (ok && o.chain >= 3) {  // static chains of o.chain pairs (tests, A/B)
        const int L = o.chain;
        double total = 0;
        for (int p = 0; p < npairs; ++p)
            if (!b.pd[p].lane) total += (double)((len_b[p] + 63) & ~63);
        const int nch = std::max(1, (b.nwave + L - 1) / L);
        const double target = total / nch;
        double acc = 0;
        std::vector<int32_t> &chain_off = b.tmp;
        chain_off.clear();
        chain_off.push_back(0);
        for (int p = 0; p < npairs; ++p) {
            if (b.pd[p].lane) continue;
            b.chain.push_back(p);
            acc += (double)((len_b[p] + 63) & ~63);
            if (acc >= target * (double)chain_off.size() && (int)chain_off.size() < nch)
                chain_off.push_back((int32_t)b.chain.size());
        }
        if (chain_off.back() != (int32_t)b.chain.size()) chain_off.push_back((int32_t)b.chain.size());
        b.nchains = (int)chain_off.size() - 1;
        b.chain_npairs = b.chain.size();
        b.chain.insert(b.chain.end(), chain_off.begin(), chain_off.end());
    } else if (ok && (o.chain == 1 || b.nwave >= 2 * resident)) {
        // dynamic: `resident` persistent waves take the next pair from a device counter
        for (int p = 0; p < npairs; ++p)
            if (!b.pd[p].lane) b.chain.push_back(p);
        b.nchains = std::min(b.nwave, resident);
        b.chain_npairs = b.chain.size();
        b.chain_dyn = true;
    }
}

// Band pruning: checkpoint batches of the stripe kernel (not CHAIN, not SPLIT), substitution costs >= 0 (the
// window's lower bound counts indels only).  SED_BAND=0 in the environment turns it off (A/B through bench.py).
// The cells and checkpoint bytes of a run come from the host's restatement of the device's bound.
// Also a cutoff's windows, and the run's algorithmic bytes.
void plan_band(Planning &P) {
    const sed_costs &c = P.c;
    sed_plan &b = P.b;
    const int npairs = P.npairs, R = b.R, ROWS = 64 * R;
    const bool costs_ok = P.band_costs_ok();  // (what both windows need of the table)
    b.band = b.ck && b.nchains == 0 && P.band_route();
    b.band_cells = b.cells;
    b.band_refine = false;
    b.band_stripes = 0;
    if (b.band) {
        const sed_band_params bp = b.bandp = sed_band_params_from(c);
        // refined windows unless switched to the static ones; their 32-bit arithmetic needs (insert + delete) (n + m)
        // below 2^30 for every wave pair (sed_internal.h: sed_refine_cell)
        b.band_refine = P.o.band != 3 && P.o.env_band != 3;
        for (int p = 0; p < npairs; ++p) {
            const int64_t nn = P.len_a[p], mm = P.len_b[p];
            if (b.pd[p].lane || nn <= 0 || mm <= 0) continue;
            b.band_stripes = std::max(b.band_stripes, sed_stripe_geom((int)nn, (int)mm, R, 64).nstripes);
            if (((int64_t)bp.ins + bp.del) * (nn + mm) >= (1ll << 30)) b.band_refine = false;
        }
        double bc = 0, ckb = 0;
        const int G = 64 / R;
        for (int p = 0; p < npairs; ++p) {
            const int nn = P.len_a[p], mm = P.len_b[p];
            if (b.pd[p].lane || nn <= 0 || mm <= 0) {
                bc += (double)nn * mm;
                continue;
            }
            const uint64_t ub = !P.diag_ub.empty() ? P.diag_ub[p]
                                                   : sed_band_diag_bound(bp, P.codes_a + P.off_a[p], nn, P.codes_b + P.off_b[p], mm);
            const sed_band w = sed_band_window(nn, mm, bp.ins, bp.del, ub);
            bc += sed_band_pair_cells(nn, mm, R, w);
            const sed_geom g = sed_stripe_geom(nn, mm, R, 64);
            for (int k = 0; k < g.nstripes; ++k) {  // checkpoints of the chunks the forward runs
                int clo, chi;
                sed_band_chunks(nn, mm, ROWS, g.nchunks, w, k, &clo, &chi);
                const int steps = std::min(g.SG, 64 * (chi + 1)) - 64 * clo;
                ckb += 4.0 * ((double)(chi - clo + 1) * (R + 1) * 64 + (double)(steps / G) * SED_CK_RW);
            }
        }
        b.band_cells = bc;
        P.tb_bytes = ckb + 8.0 * npairs;  // (and every pair's window, written and read)
    }
    b.algo_bytes = P.in_bytes + (P.want_tb ? P.tb_bytes : 0) + 16.0 * npairs;
    // a cutoff's windows (sed_batch_set_cutoff): this fill's costs, as the kernels' parameters below
    b.cut_costs_ok = b.mode == SED_MODE_I32 && costs_ok;
    b.cut_bp = b.mode == SED_MODE_I32 && c.K <= 4 && c.ins + c.del > 0 ? sed_band_params_from(c) : sed_band_params{};
}

// ---- kernel parameters ----
void plan_i32_params(Planning &P) {
    const sed_costs &c = P.c;
    sed_plan &b = P.b;
    sed_i32_params &ip = b.ip;
    ip = sed_i32_params{};
    ip.ins = (uint32_t)c.ins;
    ip.del = (uint32_t)c.del;
    for (int a = 0; a < 4; ++a) {
        uint32_t row = 0, row16 = 0;
        for (int bb = 0; bb < 4; ++bb) {
            // symbols outside the alphabet never occur in real cells: any cost <= ins + del will do
            const uint32_t v = (a < c.K && bb < c.K) ? (uint32_t)c.sub[a * c.K + bb] : 0u;
            row |= ((v - ip.ins - ip.del - 1u) & 0xFFu) << (8 * bb);
            row16 |= ((v - ip.ins - ip.del) & 0xFFu) << (8 * bb);
        }
        ip.costrow[a] = row;
        ip.costrow16[a] = row16;
    }
    ip.kins = (ip.ins << 16) + 4u;
    ip.kdel = (ip.del << 16) + 5u;
    int64_t kap[4][4], maxsum = 0, maxmin = 0;  // over the wave pairs
    if (c.K == 4 && P.o.dot != 2) {
        P.kappa(kap);
        for (int p = 0; p < P.npairs; ++p)
            if (!b.pd[p].lane) {
                maxsum = std::max<int64_t>(maxsum, (int64_t)P.len_a[p] + P.len_b[p]);
                maxmin = std::max<int64_t>(maxmin, std::min(P.len_a[p], P.len_b[p]));
            }
    }
    // dot keys: checkpoint batches of the stripe kernel (CHAIN batches share the traceback's key format)
    if ((b.ck || b.split_ck) && b.nchains == 0 && c.K == 4 && P.o.dot != 2) {
        const DotKeys dk = dot_keys(kap, maxmin);
        if (dk.ok) {
            ip.dot = 1;
            ip.dotA = dk.A;
            ip.dotkmax = dk.kmax;
            ip.dotM = dk.M;
            ip.dotS = dk.S;
            for (int a = 0; a < 4; ++a) {
                ip.dotrow[a] = dk.row[a];
                ip.dotcol[a] = dk.col[a];
            }
            b.dot = true;
        }
    }
    // ladder dot keys: the CHAIN kernel's ladder keys (L field, with or without codes) with the update addend
    // as one v_dot4.  V = D*A + uL needs A < 2^16 and the factorisation of A*K + (u - 1)J (the d = -1 rows'
    // constant) in bytes: u = 16 over the wide ladder (sed_kernels.hip: LadderW, ip.lad = 2) with 16 min(n, m) + 15
    // < A, else u = 8 over the 3-bit one (ip.lad = 1) with 8 (n + m) + 7 < A (the L field below the D unit).
    if (b.nchains > 0 && !b.ck && (P.want_tb || !(P.flags & SED_NO_LEN)) && c.K == 4 && P.o.dot != 2) {
        // the wide ladder first (one jump row in 8; its sink decode reads L inside [max(n, m), n + m], so A > 16
        // min(n, m) + 15 keeps the keys apart), the 3-bit one where that does not fit bytes
        DotKeys lk = P.o.dot == 3 ? DotKeys{} : dot_keys(kap, 0, 16 * maxmin + 16, 15);  // (3: tests)
        uint32_t lad = 2;
        if (!lk.ok) {
            lk = dot_keys(kap, 0, 8 * maxsum + 8, 7);
            lad = 1;
        }
        if (lk.ok) {
            ip.lad = lad;
            ip.ladA = lk.A;
            ip.ladsent = lk.S;  // (ladder mode: the sentinel's byte 0)
            for (int a = 0; a < 4; ++a) {
                ip.ladrow[a] = lk.row[a];
                ip.ladcol[a] = lk.col[a];
            }
            b.lad = true;
        }
    }
}

void plan_params(Planning &P) {
    sed_plan &b = P.b;
    b.dot = b.lad = false;
    if (b.mode == SED_MODE_I32) {
        plan_i32_params(P);
    } else {
        sed_f64_params fp{};
        fp.ins = P.c.ins;
        fp.del = P.c.del;
        fp.ins_int = P.c.ins_int;
        fp.del_int = P.c.del_int;
        fp.K = P.c.K;
        b.fp = fp;
    }
}

// ---- the device arrays' sizes, the small path's blob, the streams a run uses ----
void plan_buffers(Planning &P) {
    const sed_opts &o = P.o;
    sed_plan &b = P.b;
    const int npairs = P.npairs;
    const bool packed = b.mode == SED_MODE_I32;
    const uint64_t pad_words = (uint64_t)(64 * b.R) / 16 * 2 + 64;
    const size_t sa = packed ? (P.aw + pad_words) * 4 : P.aw + 64, sb = packed ? (P.bw + pad_words) * 4 : P.bw + 64;
    const size_t nchain = b.chain.size();
    const size_t size[SED_UP_COUNT] = {sizeof(sed_pair_desc) * std::max(1, npairs), sa, sb,
                                       sizeof(int2) * std::max<size_t>(1, b.tasks.size()), 4 * (nchain + 4),
                                       4 * std::max<size_t>(1, b.lane.size()), 4 * std::max<size_t>(1, b.x2.size()),
                                       4 * std::max<size_t>(1, b.seg.size())};
    const size_t copy[SED_UP_COUNT] = {sizeof(sed_pair_desc) * (size_t)npairs, sa, sb, sizeof(int2) * b.tasks.size(),
                                       4 * nchain, 4 * b.lane.size(), 4 * b.x2.size(), 4 * b.seg.size()};
    // Small batches (the drop-in module's per-call pairs, sed_run_batch): every input array and the zeroed results go
    // up as one blob from the context's pinned staging buffer, with no upload sync, instead of one pageable copy per
    // array and a memset.
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    for (int i = 0; i < SED_UP_COUNT; ++i) {
        b.up_size[i] = size[i];
        b.up_copy[i] = copy[i];
        b.up_off[i] = off;
        off += al(size[i]);
    }
    b.res_size = sizeof(sed_result) * std::max(1, npairs);
    b.o_res = off;
    b.o_ops = b.o_res + al(b.res_size);
    b.blob_bytes = b.o_ops + al(4 * std::max<uint64_t>(1, b.ops_words));  // (results and scripts adjacent: one download)
    b.small = b.nbuf == 1 && b.blob_bytes <= SED_SMALL_BATCH_BYTES;
    b.zc = b.small && !b.tbpar && o.zc != 2;
    // SED_ALT_DP=0 keeps every DP on the context's stream (A/B)
    // pipelined batches whose runs share no scratch (dynamic-CHAIN script batches, distance-only batches of lane
    // pairs): odd runs' DP on a second stream
    b.alt_dp = o.env_alt_dp != 0 && b.nbuf > 1 &&
               ((b.chain_dyn && (P.flags & SED_WANT_SCRIPT)) ||
                (b.nwave == 0 && b.nwave_x2 == 0 && !(P.flags & SED_WANT_SCRIPT)));
    // distance-only lane batches on two streams use two result slots, one per stream: a slot's runs are then
    // ordered by their stream and need no event query or cross-stream wait
    if (b.alt_dp && !(P.flags & SED_WANT_SCRIPT)) b.nbuf = 2;
    // SED_CK_HALVES: parts per checkpoint batch of >= 1024 wave pairs per part (1 = off; default
    // SED_CK_HALVES_DEFAULT; at most 4, the hardware queues a process gets)
    const int want = std::min(4, std::max(1, o.env_ck_halves < 0 ? SED_CK_HALVES_DEFAULT : o.env_ck_halves));
    b.nparts = 1;
    if (b.ck && b.nchains == 0 && b.nbuf == 1 && b.nwave_x2 == 0) b.nparts = std::max(1, std::min(want, b.nwave / 1024));
}

// 16 codes per word, each word built in a register (an OR into memory per code was ~1 ns per symbol)
void pack2(const uint8_t *src, int len, uint32_t *dst) {
    const int full = len >> 4;
    for (int w = 0; w < full; ++w) {
        const uint8_t *q = src + 16 * w;
        uint32_t v = 0;
        for (int k = 0; k < 16; ++k) v |= (uint32_t)q[k] << (2 * k);
        dst[w] = v;
    }
    if (len & 15) {
        uint32_t v = 0;
        for (int k = 0; k < (len & 15); ++k) v |= (uint32_t)src[16 * full + k] << (2 * k);
        dst[full] = v;
    }
}

// {key, field, the values it takes: a bit set of values < 64, or 0 = every value in [0, hi]}
struct OptSpec {
    int key;
    int sed_opts::*field;
    uint64_t values;
    int hi;
};
constexpr uint64_t V(int a, int b = -1, int c = -1) {
    return (1ull << a) | (b < 0 ? 0 : 1ull << b) | (c < 0 ? 0 : 1ull << c);
}
const OptSpec opt_table[] = {
    {SED_OPT_MODE, &sed_opts::mode, 0, 3},
    {SED_OPT_SPLIT, &sed_opts::split, 0, 2},
    {SED_OPT_LANE, &sed_opts::lane, 0, 2},
    {SED_OPT_TB, &sed_opts::tb, 0, 2},
    {SED_OPT_PACK, &sed_opts::pack, V(0, 2), 0},
    {SED_OPT_BITPAR, &sed_opts::bitpar, V(0, 2), 0},
    {SED_OPT_SEG, &sed_opts::seg, 0, 2},
    {SED_OPT_SPLITCK, &sed_opts::splitck, V(0, 2), 0},
    {SED_OPT_ZEROCOPY, &sed_opts::zc, V(0, 2), 0},
    {SED_OPT_SCALED, &sed_opts::scaled, V(0, 2), 0},
    {SED_OPT_DOT, &sed_opts::dot, V(0, 2, 3), 0},
    {SED_OPT_CHAIN_WAVES, &sed_opts::chain_waves, 0, INT_MAX},
    {SED_OPT_CUT, &sed_opts::cut, 0, 2},
    {SED_OPT_BAND, &sed_opts::band, V(0, 2, 3), 0},
    {SED_OPT_FIT_CHUNK, &sed_opts::fit_chunk, 0, INT_MAX},
    {SED_OPT_FIT_ROWS, &sed_opts::fit_rows, V(0, 2, 4) | V(8, 16, 32), 0},
    {SED_OPT_JOIN_DP, &sed_opts::join_dp, V(0, 2), 0},
    {SED_OPT_JOIN_ROWS, &sed_opts::join_rows, 0, INT_MAX},
    {SED_OPT_DEBUG_CORRUPT, &sed_opts::debug_corrupt, 0, INT_MAX},
    {SED_OPT_CHAIN, &sed_opts::chain, 0, 1024},
    {SED_OPT_ROWS_PER_LANE, &sed_opts::R, V(0, 1, 2) | V(4, 8, 16) | V(32), 0},
};
// the environment knobs, as sed_plan_routes takes them (any int, as atoi gives the runtime)
const OptSpec env_table[] = {
    {SED_PLAN_ENV_TBPAR, &sed_opts::env_tbpar, 0, 0},
    {SED_PLAN_ENV_BAND, &sed_opts::env_band, 0, 0},
    {SED_PLAN_ENV_ALT_DP, &sed_opts::env_alt_dp, 0, 0},
    {SED_PLAN_ENV_CK_HALVES, &sed_opts::env_ck_halves, 0, 0},
};

}  // namespace

bool sed_opts_set(sed_opts &o, int key, int value, bool env_keys) {
    for (const OptSpec &s : opt_table)
        if (s.key == key) {
            if (value < 0 || (s.values ? value > 63 || !((s.values >> value) & 1) : value > s.hi)) return false;
            o.*s.field = value;
            return true;
        }
    for (const OptSpec &s : env_table)
        if (env_keys && s.key == key) {
            o.*s.field = value;
            return true;
        }
    return false;
}

// "simple typing": a cell's value is an int exactly when it equals 0.
bool sed_simple_typing(const sed_costs &c) {
    if (c.ins_int || c.del_int || !(c.ins > 0) || !(c.del > 0)) return false;
    for (int e = 0; e < c.K * c.K; ++e) {
        if (c.sub_int[e] ? c.sub[e] != 0 : !(c.sub[e] > 0)) return false;
    }
    return true;
}

sed_band_params sed_band_params_from(const sed_costs &c) {
    sed_band_params bp{};
    for (int a = 0; a < 4; ++a)
        for (int bb = 0; bb < 4; ++bb)
            bp.cost[a * 4 + bb] = (a < c.K && bb < c.K) ? (uint32_t)c.sub[a * c.K + bb] : 0u;
    bp.ins = (uint32_t)c.ins;
    bp.del = (uint32_t)c.del;
    return bp;
}

uint64_t sed_band_diag_bound(const sed_band_params &bp, const uint8_t *a, int n, const uint8_t *b, int m) {
    uint64_t ub = 0;
    const int len = std::min(n, m);
    for (int i = 0; i < len; ++i) ub += bp.cost[(a[i] & 3) * 4 + (b[i] & 3)];
    return ub + (m > n ? (uint64_t)(m - n) * bp.ins : (uint64_t)(n - m) * bp.del);
}

int sed_plan_batch(const sed_costs &c, const sed_opts &o, const uint8_t *codes_a, const int64_t *off_a,
                   const int32_t *len_a, const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                   int32_t npairs, uint32_t flags, sed_plan *plan, std::string *err) {
    Planning P{c, o, codes_a, off_a, len_a, codes_b, off_b, len_b, npairs, flags, *plan, err};
    int rc = plan_validate(P);
    if (rc != SED_OK) return rc;
    plan->npairs = npairs;
    plan->flags = flags;
    P.want_tb = (flags & SED_WANT_SCRIPT) != 0;
    if ((rc = plan_mode(P)) != SED_OK) return rc;
    plan_traceback(P);
    plan_layout(P);
    const bool x2_ok = plan->mode == SED_MODE_I32 && x2_costs_ok(c);
    plan_lane_routes(P, x2_ok);
    plan_wave_x2(P, x2_ok);
    plan_chain(P);
    plan_band(P);
    plan_params(P);
    plan_buffers(P);
    return SED_OK;
}

void sed_pack_sequences(const sed_plan &plan, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
                        const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, std::vector<uint32_t> &ha,
                        std::vector<uint32_t> &hb) {
    ha.assign((plan.up_copy[SED_UP_SEQA] + 3) / 4, 0);
    hb.assign((plan.up_copy[SED_UP_SEQB] + 3) / 4, 0);
    for (int p = 0; p < plan.npairs; ++p) {
        const sed_pair_desc &d = plan.pd[p];
        if (plan.mode == SED_MODE_I32) {
            pack2(codes_a + off_a[p], len_a[p], ha.data() + d.a_off);
            pack2(codes_b + off_b[p], len_b[p], hb.data() + d.b_off);
        } else {
            if (len_a[p]) memcpy((uint8_t *)ha.data() + d.a_off, codes_a + off_a[p], len_a[p]);
            if (len_b[p]) memcpy((uint8_t *)hb.data() + d.b_off, codes_b + off_b[p], len_b[p]);
        }
    }
}

bool sed_plan_cut_window_ok(const sed_plan &p) {
    int nwork = 0;  // wave pairs with cells
    for (const sed_pair_desc &d : p.pd) nwork += d.lane != 1 && d.n > 0 && d.m > 0;
    return p.mode == SED_MODE_I32 && !p.split && (p.flags & SED_NO_LEN) && p.nseg == 0 &&
           (p.R == 4 || p.R == 8 || p.R == 16) && p.cut_costs_ok && nwork > 0;
}

sed_run_plan sed_plan_run(const sed_plan &p, bool cut_on, bool cut_win) {
    sed_run_plan s;
    const bool want_tb = (p.flags & SED_WANT_SCRIPT) != 0;
    s.tb = want_tb;
    // rotating buffers are ordered through the events of their runs; two-slot lane batches order by stream instead
    s.need_ev = p.nbuf > 1 && !(p.alt_dp && p.nbuf == 2 && !want_tb);
    // a slot was last read by its previous run's traceback (distance only: written by its DP)
    if (p.nbuf > 1 && (want_tb || (p.alt_dp && p.nbuf != 2))) s.reuse = want_tb ? SED_REUSE_TB_END : SED_REUSE_DP_END;
    if (p.npairs == 0) return s;
    auto add = [&s](uint8_t kind, uint8_t phase, uint8_t on, int part) {
        if (s.n < SED_MAX_STEPS) s.step[s.n++] = sed_step{kind, phase, on, (uint8_t)part, false, false};
    };
    if (p.nparts > 1 && want_tb) {
        // A checkpoint batch in parts: part i runs its forward and then its traceback on its own stream.  The whole
        // batch's lane kernel follows part 0's forward inside part 0's DP window.
        s.nparts = std::min(p.nparts, SED_MAX_PARTS);
        for (int i = 0; i < s.nparts; ++i) add(SED_STEP_I32, SED_PHASE_DP, SED_ON_PART, i);
        if (p.nlane > 0) add(SED_STEP_LANE, SED_PHASE_DP, SED_ON_PART, 0);
        for (int i = 0; i < s.nparts; ++i) add(SED_STEP_TB_CK, SED_PHASE_TB, SED_ON_PART, i);
    } else {
        const int nw64 = p.nwave - p.nseg;  // wave pairs of the one-wave-per-pair kernels
        const bool i32 = p.mode == SED_MODE_I32;
        const bool tb_apart = p.nbuf > 1;  // the traceback has a stream of its own
        // a cutoff: the filter as the DP phase's last kernel, and under cut_win the wave pairs on the windowed stripe
        // kernel instead of their own routes
        s.cut = cut_on && !want_tb;
        if (s.cut && cut_win) {
            add(SED_STEP_WIN, SED_PHASE_DP, SED_ON_DP, 0);
        } else {
            if (p.nwave_x2 > 0) add(SED_STEP_X2, SED_PHASE_DP, SED_ON_DP, 0);
            if (nw64 > 0) add(i32 && p.nchains ? SED_STEP_CHAIN : i32 ? SED_STEP_I32 : SED_STEP_F64, SED_PHASE_DP, SED_ON_DP, 0);
            // split_ck: the tile codes close the DP phase when the traceback shares its stream; pipelined runs open the
            // traceback phase with them, so the next run's forward follows this one directly (config 2 ran
            // 0.297-0.301 ms per step with it on the DP stream)
            if (nw64 > 0 && i32 && !p.nchains && p.split_ck && !tb_apart) add(SED_STEP_CODES, SED_PHASE_DP, SED_ON_DP, 0);
            if (p.nseg > 0) add(SED_STEP_F64_SEG, SED_PHASE_DP, SED_ON_DP, 0);
        }
        if (p.nlane > 0) add(SED_STEP_LANE, SED_PHASE_DP, SED_ON_DP, 0);
        if (s.cut) add(SED_STEP_FILTER, SED_PHASE_DP, SED_ON_DP, 0);
        if (want_tb && p.nwave > 0) {
            if (p.split_ck && tb_apart) add(SED_STEP_CODES, SED_PHASE_TB, SED_ON_TB, 0);
            if (p.tbpar) {  // (the map kernel zeroes the scripts the segments OR into)
                add(SED_STEP_TB_STRIPES, SED_PHASE_TB, SED_ON_TB, 0);
            } else {
                if (nw64 > 0) add(p.ck ? SED_STEP_TB_CK : SED_STEP_TB_CODES, SED_PHASE_TB, SED_ON_TB, 0);
                if (p.nseg > 0) add(SED_STEP_TB_SEG, SED_PHASE_TB, SED_ON_TB, 0);
            }
        }
    }
    // the events: the first and the last step of every (phase, part)
    int first[2][SED_MAX_PARTS], last[2][SED_MAX_PARTS];
    std::fill(&first[0][0], &first[0][0] + 2 * SED_MAX_PARTS, -1);
    std::fill(&last[0][0], &last[0][0] + 2 * SED_MAX_PARTS, -1);
    for (int i = 0; i < s.n; ++i) {
        const sed_step &st = s.step[i];
        if (first[st.phase][st.part] < 0) first[st.phase][st.part] = i;
        last[st.phase][st.part] = i;
    }
    for (int ph = 0; ph < 2; ++ph)
        for (int part = 0; part < SED_MAX_PARTS; ++part)
            if (first[ph][part] >= 0) s.step[first[ph][part]].first = s.step[last[ph][part]].last = true;
    return s;
}

namespace {
// the costs, options and pairs of a device-free probe (sed_plan_routes, sed_plan_schedule) as a plan
int probe_plan(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del, int del_is_int,
               const int32_t *options, int noptions, const uint8_t *codes_a, const int64_t *off_a, const int32_t *len_a,
               const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b, int32_t npairs, uint32_t flags,
               sed_opts *o, sed_plan *p) {
    if (K < 1 || K > 255 || !sub || !sub_int || noptions < 0 || (noptions && !options)) return SED_E_ARG;
    sed_costs c;
    c.K = K;
    c.sub.assign(sub, sub + K * K);
    c.sub_int.assign(sub_int, sub_int + K * K);
    c.ins = ins;
    c.del = del;
    c.ins_int = ins_is_int ? 1 : 0;
    c.del_int = del_is_int ? 1 : 0;
    for (int i = 0; i < noptions; ++i)  // (the fit and join options are no options of a batch: their plan calls take them)
        if (options[2 * i] == SED_OPT_FIT_CHUNK || options[2 * i] == SED_OPT_FIT_ROWS ||
            options[2 * i] == SED_OPT_JOIN_DP || options[2 * i] == SED_OPT_JOIN_ROWS ||
            !sed_opts_set(*o, options[2 * i], options[2 * i + 1], true))
            return SED_E_ARG;
    return sed_plan_batch(c, *o, codes_a, off_a, len_a, codes_b, off_b, len_b, npairs, flags, p, nullptr);
}
}  // namespace

extern "C" {

int sed_plan_routes(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                    int del_is_int, const int32_t *options, int noptions, const uint8_t *codes_a, const int64_t *off_a,
                    const int32_t *len_a, const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                    int32_t npairs, uint32_t flags, double *out, int nout) {
    if (nout < 0 || (nout && !out)) return SED_E_ARG;
    sed_opts o;
    sed_plan p;
    const int rc = probe_plan(K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions, codes_a, off_a, len_a,
                              codes_b, off_b, len_b, npairs, flags, &o, &p);
    if (rc != SED_OK) return rc;
    const double v[] ={(double)p.mode, (double)p.R, (double)p.nlane, (double)sed_plan_chains(p, false),
                        (double)sed_plan_traceback_mode(p), (double)sed_plan_dot_keys(p), (double)sed_plan_bitpar_pairs(p),
                        (double)p.nseg, (double)sed_plan_split_tasks(p), (double)sed_plan_scaled_pairs(p),
                        (double)sed_plan_packed_pairs(p, false), (double)p.nparts, p.band_cells, p.cells, p.algo_bytes};
    for (int i = 0; i < nout && i < (int)(sizeof v / sizeof *v); ++i) out[i] = v[i];
    return SED_OK;
}

int sed_plan_schedule(int K, const double *sub, const uint8_t *sub_int, double ins, int ins_is_int, double del,
                      int del_is_int, const int32_t *options, int noptions, const uint8_t *codes_a, const int64_t *off_a,
                      const int32_t *len_a, const uint8_t *codes_b, const int64_t *off_b, const int32_t *len_b,
                      int32_t npairs, uint32_t flags, int cut_on, int cut_win, int32_t *out, int max_steps,
                      int32_t *info) {
    if (max_steps < 0 || (max_steps && !out)) return SED_E_ARG;
    sed_opts o;
    sed_plan p;
    const int rc = probe_plan(K, sub, sub_int, ins, ins_is_int, del, del_is_int, options, noptions, codes_a, off_a, len_a,
                              codes_b, off_b, len_b, npairs, flags, &o, &p);
    if (rc != SED_OK) return rc;
    // the cutoff states sed_batch_set_cutoff can leave a batch in
    if ((cut_on && (flags & SED_WANT_SCRIPT)) || (cut_win && !(cut_on && o.cut != 2 && sed_plan_cut_window_ok(p))))
        return SED_E_ARG;
    const sed_run_plan s = sed_plan_run(p, cut_on != 0, cut_win != 0);
    for (int i = 0; i < s.n && i < max_steps; ++i) {
        const sed_step &st = s.step[i];
        const int32_t row[6] = {st.kind, st.phase, st.on, st.part, st.first, st.last};
        std::copy(row, row + 6, out + 6 * i);
    }
    if (info) {
        const int32_t v[4] = {s.need_ev, s.reuse, s.nparts, SED_MAX_STEPS};
        std::copy(v, v + 4, info);
    }
    return s.n;
}

int sed_dot_factor(const double *sub, double ins, double del, int maxmin, int ladder_maxsum, uint32_t *out) {
    if (!sub || !out || maxmin < 0 || ladder_maxsum < 0) return SED_E_ARG;
    int64_t kap[4][4];
    for (int a = 0; a < 4; ++a)
        for (int bb = 0; bb < 4; ++bb) {
            const double v = ins + del - sub[a * 4 + bb];
            if (v != (double)(int64_t)v) return 0;  // integer tables only (the packed-integer kernels' domain)
            kap[a][bb] = (int64_t)v;
        }
    // ladder: the wide ladder's factorisation where it exists, else the 3-bit one (as batch creation); out[9] = the L unit
    // (the wide ladder's bound is on min(n, m): maxmin, or ladder_maxsum when maxmin is 0)
    const int64_t lmin = maxmin > 0 ? std::min<int64_t>(maxmin, ladder_maxsum) : ladder_maxsum;
    DotKeys dk = ladder_maxsum > 0 ? dot_keys(kap, 0, 16 * lmin + 16, 15) : dot_keys(kap, maxmin);
    uint32_t unit = 16;
    if (ladder_maxsum > 0 && !dk.ok) {
        dk = dot_keys(kap, 0, 8 * (int64_t)ladder_maxsum + 8, 7);
        unit = 8;
    }
    if (!dk.ok) return 0;
    for (int a = 0; a < 4; ++a) {
        out[a] = dk.row[a];
        out[4 + a] = dk.col[a];
    }
    out[8] = dk.S;  // decode shift (dot keys) or sentinel byte (ladder)
    out[9] = ladder_maxsum > 0 ? unit : dk.M;  // decode multiplier (dot keys) or the L unit (ladder)
    return (int)dk.A;
}

int sed_band_bounds(int32_t n, int32_t m, double ins, double del, double ub, int32_t *out) {
    if (!out || n < 0 || m < 0 || !(ins >= 0) || !(del >= 0) || !(ins + del > 0) || !(ub >= 0) || ins >= 65536 ||
        del >= 65536 || ub >= 9e15)
        return SED_E_ARG;
    const sed_band w = sed_band_window(n, m, (uint32_t)ins, (uint32_t)del, (uint64_t)ub);
    out[0] = w.elo;
    out[1] = w.ehi;
    return SED_OK;
}

int sed_band_refine_row(int32_t n, int32_t m, int32_t rows_per_lane, double ins, double del, int32_t stripe,
                        double ub_prev, double suf, const int32_t *drow, int32_t clo_prev, int32_t chi_prev,
                        int32_t *out) {
    const int R = rows_per_lane;
    if (!out || !drow || n < 1 || m < 1 || (R != 4 && R != 8 && R != 16) || stripe < 1 ||
        stripe >= sed_stripe_geom(n, m, R, 64).nstripes || !(ins >= 0) || !(del >= 0) || !(ins + del > 0) ||
        (ins + del) * ((double)n + m) >= (double)(1 << 30) || !(ub_prev >= 0) || ub_prev >= (double)(1u << 31) ||
        suf >= (double)(1u << 31))
        return SED_E_ARG;
    const int ROWS = 64 * R, nchunks = sed_stripe_geom(n, m, R, 64).nchunks, r0 = stripe * ROWS;
    if (clo_prev < 0 || chi_prev < clo_prev || chi_prev >= nchunks) return SED_E_ARG;
    const uint32_t ui = (uint32_t)ins, ud = (uint32_t)del;
    const int j0 = 64 * clo_prev + 1, j1 = std::min(m, 64 * chi_prev + 1);  // the columns the stripe above computed
    uint32_t ub = (uint32_t)ub_prev;
    if (suf >= 0 && r0 >= j0 && r0 <= j1) ub = std::min(ub, (uint32_t)drow[r0] + (uint32_t)suf);
    int32_t lo = SED_REFINE_LO_INIT, hi = SED_REFINE_HI_INIT;
    for (int j = j0; j <= j1; ++j) sed_refine_cell(n, m, ui, ud, r0, j, (uint32_t)drow[j], ub, &lo, &hi);
    int clo, chi;
    const bool any = sed_refine_chunks(n, m, ROWS, nchunks, ui, ud, ub, lo, hi, stripe, clo_prev, chi_prev, &clo, &chi);
    out[0] = clo;
    out[1] = chi;
    out[2] = (int32_t)ub;
    out[3] = any ? 1 : 0;
    return SED_OK;
}

int sed_band_chunk_range(int32_t n, int32_t m, int32_t rows_per_lane, int32_t elo, int32_t ehi, int32_t stripe,
                         int32_t *out) {
    const int R = rows_per_lane;
    if (!out || n < 1 || m < 1 || (R != 4 && R != 8 && R != 16) || stripe < 0 || stripe >= sed_stripe_geom(n, m, R, 64).nstripes)
        return SED_E_ARG;
    const int nchunks = sed_stripe_geom(n, m, R, 64).nchunks;
    int clo, chi;
    sed_band_chunks(n, m, 64 * R, nchunks, sed_band{elo, ehi}, stripe, &clo, &chi);
    out[0] = clo;
    out[1] = chi;
    out[2] = nchunks;
    return SED_OK;
}

double sed_band_cells(const double *sub, double ins, double del, const uint8_t *codes_a, int32_t n,
                      const uint8_t *codes_b, int32_t m, int32_t rows_per_lane) {
    const int R = rows_per_lane;
    if (!sub || !codes_a || !codes_b || n < 1 || m < 1 || (R != 4 && R != 8 && R != 16) || !(ins >= 0) || !(del >= 0) ||
        !(ins + del > 0) || ins >= 65536 || del >= 65536)
        return -1.0;
    for (int i = 0; i < 16; ++i)
        if (!(sub[i] >= 0) || sub[i] >= 65536) return -1.0;
    sed_costs c;
    c.K = 4;
    c.sub.assign(sub, sub + 16);
    c.ins = ins;
    c.del = del;
    const sed_band_params bp = sed_band_params_from(c);
    for (int i = 0; i < n; ++i)
        if (codes_a[i] > 3) return -1.0;
    for (int i = 0; i < m; ++i)
        if (codes_b[i] > 3) return -1.0;
    return sed_band_pair_cells(n, m, R, sed_band_window(n, m, bp.ins, bp.del, sed_band_diag_bound(bp, codes_a, n, codes_b, m)));
}

}  // extern "C"
