"""The numeric envelope of the similarity join (sed_join_self / sed_join_search and their _f64 siblings, DESIGN.md 3.6k
and 3.6l) as cost models, sequence sets, cutoffs and lane models, shared by the CPU tests (tests/test_join_envelope.py)
and the GPU tests (tests/test_gpu_join_envelope.py).  No device is needed here.

The integer planner admits a table whose costs are integers on some scale S = 2^k, k <= 8, with insert S >= 1,
delete S >= 1, every substitution <= insert + delete, (insert + delete) S <= 255 and K <= 8; the limit tables sit on
those borders and refused_neighbours() one step past each.  The sets place every column and row length 0..32, the
largest distances a table allows, single hits at chosen lanes, full ballots with one hole, and waves the length skip
splits.  The reference is join_cases.oracle_matrix throughout; dp_lane_matrix and bitpar_matrix restate the two integer
kernels' lanes word for word."""
import math
import sys

import numpy as np

import fit_envelope as fe
import join_cases as jc
import join_f64_cases as jf
import sedgpu
from conftest import load_golden
from test_bitpar_model import bitpar_distance

INF = math.inf
ALPHA = "ACGUNRYSK"   # code c = ALPHA[c]; the integer route takes the first 8 at most
MAXLEN = 32
CUT_ALL = 65535       # SED_JOIN_CUT_ALL
KB = 0xFFFFFFFC       # SED_KB
M32 = 0xFFFFFFFF


class CodePlan(fe.Plan):
    """fit_envelope.Plan over the symbols ALPHA[:K], with the encoders join_cases' helpers call."""

    def encode(self, s):
        return np.array([ALPHA.index(c) for c in s], np.uint8)

    def encode_many(self, seqs):
        parts = [self.encode(s) for s in seqs]
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.array([len(s) for s in seqs], np.int32)


def scale_of(plan):
    """The planner's scale: the smallest S = 2^k, k <= 8, that makes every cost an integer (None: there is none)."""
    vals = [float(plan.ins), float(plan.dele)] + [float(v) for v in np.asarray(plan.sub).ravel()]
    for k in range(9):
        if all(v * 2.0 ** k == math.floor(v * 2.0 ** k) for v in vals):
            return 2 ** k
    return None


# ---- the integer route's limit tables and their first refused neighbours ----

LIMITS = {"i1_d254": (1, 1, 254, 4), "i254_d1": (1, 254, 1, 5), "i127_d128": (1, 127, 128, 8),
          "s256": (256, 100, 155, 6), "s256_i1": (256, 1, 254, 4)}  # name -> (S, insert S, delete S, K)
ZERO_CELL, FULL_CELL, UNIT_CELL, BELOW_CELL = (0, 1), (1, 0), (0, 2), (2, 0)


def limit_table(name):
    """Seeded asymmetric substitutions 0..insert + delete on the integer scale, a zero diagonal, and four forced cells:
    ZERO_CELL = 0 off the diagonal (addend byte 0x00 where insert + delete = 255), UNIT_CELL = 1 / S (an odd numerator,
    so no smaller scale serves an S = 256 table), FULL_CELL = insert + delete exactly (addend byte 0xFF) and BELOW_CELL
    one step below it.  i127_d128 also has a nonzero diagonal entry, which Context.set_costs and the oracle honour."""
    S, i, d, K = LIMITS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    sub = rng.integers(0, i + d + 1, size=(K, K))
    np.fill_diagonal(sub, 0)
    sub[ZERO_CELL], sub[UNIT_CELL], sub[FULL_CELL], sub[BELOW_CELL] = 0, 1, i + d, i + d - 1
    if name == "i127_d128":
        sub[1, 1] = 3
    assert (sub != sub.T).any() and sub.max() <= i + d
    return CodePlan(sub / float(S), i / float(S), d / float(S))


def limit_tables():
    """name -> (plan, S)"""
    return {name: (limit_table(name), LIMITS[name][0]) for name in LIMITS}


def refused_neighbours():
    """name -> (plan, regex of its own rule's text): one step past each border of the planner's envelope.  Every one is
    finite and nonnegative over at most 16 symbols, so the fp64 rule admits it."""
    def table(K, i, d, S, edit=None):
        rng = np.random.default_rng(K + i + d)
        sub = rng.integers(0, i + d + 1, size=(K, K)).astype(np.float64)
        np.fill_diagonal(sub, 0)
        if edit:
            edit(sub)
        return CodePlan(sub / S, i / float(S), d / float(S))
    unit = (1.0 - np.eye(8)) * 256
    unit[0, 1] = 257  # insert = delete = 1 in steps of 1 / 256: (insert + delete) S = 512
    return {"sum 256": (table(4, 128, 128, 1), r"\(insert \+ delete\) \* S = 256 exceeds 255"),
            "k = 9": (table(8, 127, 128, 1, lambda s: s.__setitem__((3, 4), 1 / 512)), r"multiples of 2\^-k for any k <= 8"),
            "insert 0": (table(4, 0, 100, 1), r"insert \* S = 0, delete \* S = 100: both must be at least 1"),
            "delete 0": (table(4, 100, 0, 256), r"delete \* S = 0: both must be at least 1"),
            "sub above": (table(6, 100, 155, 256, lambda s: s.__setitem__((2, 5), 256)),
                          r"cost\(2 -> 5\) = 1 exceeds insert \+ delete = 0\.996"),
            "K = 9": (table(9, 127, 128, 1), r"9 symbols"),
            "unit at 1/256": (CodePlan(unit / 256, 1.0, 1.0), r"\(insert \+ delete\) \* S = 512 exceeds 255")}


# ---- tables for the bit-parallel kernel at S > 1 and under code maps that are not the identity ----

UNIT_SHIFT = 6  # insert = delete = 1 admits S <= 64: (insert + delete) S <= 255


def unit_block_table():
    """8 symbols, insert = delete = 1, the block over codes {1, 3, 6, 7} unit, every other entry a multiple of 1 / 64
    in 0..2 with an odd numerator among them: S = 64, the largest scale the planner admits beside insert = delete = 1
    (1 / 256 is refused_neighbours' "unit at 1/256")."""
    rng = np.random.default_rng(1367)
    sub = rng.integers(0, 129, size=(8, 8))
    np.fill_diagonal(sub, 0)
    sub[0, 1] = 1
    for a in (1, 3, 6, 7):
        for b in (1, 3, 6, 7):
            sub[a, b] = 0 if a == b else 64
    return CodePlan(sub / 64.0, 1.0, 1.0)


def one_way_table():
    """8 symbols in halves, insert = delete = 1: codes {0, 1} -> codes {6, 7} cost 1, codes {6, 7} -> codes {0, 1} cost
    0.5.  Unit for queries over {0, 1} against an index over {6, 7}, and not the other way."""
    rng = np.random.default_rng(67)
    sub = rng.integers(1, 5, size=(8, 8))
    np.fill_diagonal(sub, 0)
    for a in (0, 1):
        for b in (6, 7):
            sub[a, b], sub[b, a] = 2, 1
    return CodePlan(sub / 2.0, 1.0, 1.0)


def bitpar_tables():
    """name -> (plan, S, the symbols the sequences draw from)"""
    return {"costs ACGUN": (jc.plan_for(load_golden("costs.json"), "ACGUN"), 4, "ACGU"),
            "unit block": (unit_block_table(), 1 << UNIT_SHIFT, "".join(ALPHA[c] for c in (1, 3, 6, 7))),
            "one way": (one_way_table(), 2, None)}  # (queries over ALPHA[0:2], the index over ALPHA[6:8])


BITPAR_CUTOFFS = (0.0, 1.0, 1.25, 2.0 - 2.0 ** -52, 2.0, INF)


def near_set(seed, symbols, count, lengths=(0, 33)):
    """Random sequences over `symbols` with lengths in [lengths), each followed by copies one edit away."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < count:
        s = jc.random_seq(rng, symbols, int(rng.integers(*lengths)))
        seqs.append(s)
        for _ in range(2):
            if len(s) >= 2:
                p, kind = int(rng.integers(len(s))), int(rng.integers(3))
                c = jc.random_seq(rng, symbols, 1)
                seqs.append(s if kind == 0 else s[:p] + c + s[p + 1:] if kind == 1 else s[:p] + s[p + 1:])
    return seqs[:count]


# ---- sequence sets ----

def length_grid(symbols, seed):
    """One sequence of every length 0..32 over the two `symbols`, shuffled."""
    assert len(symbols) == 2
    rng = np.random.default_rng(seed)
    seqs = [jc.random_seq(rng, symbols, n) for n in range(MAXLEN + 1)]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def length_grids(symbols, seeds=(1, 2, 3)):
    """The 99 sequences of three grids: a self join meets every (n, m), n != m, nine times, and a search with the same
    99 as queries meets every n = m, identical pairs included."""
    return [s for seed in seeds for s in length_grid(symbols, seed)]


def max_pairs(plan):
    """[(row, column)]: the pairs that reach the largest distances a table allows: a * 32 against b * 32 for the cell
    (a -> b) that holds insert + delete, the empty sequence against 32 symbols both ways, and 32 against 31."""
    a, b = np.argwhere(np.asarray(plan.sub) == plan.ins + plan.dele)[0]
    a, b = ALPHA[a], ALPHA[b]
    return [(a * 32, b * 32), ("", a * 32), (a * 32, ""), ("", b * 32), (b * 32, ""), (a * 32, b * 31), (a * 31, b * 32)]


def zero_pairs(plan):
    """[(row, column)]: 32 free substitutions, the smallest sink key a table allows (B - 32 ((insert + delete) S << 16)
    - 32), and its neighbours of 31 symbols."""
    off = np.asarray(plan.sub) + np.eye(plan.K)
    a, b = np.argwhere(off == 0)[0]
    a, b = ALPHA[a], ALPHA[b]
    return [(a * 32, b * 32), (a * 31, b * 32), (a * 32, b * 31)]


def limit_set(plan):
    """100 sequences for one limit table: a length grid over the symbols of ZERO_CELL / FULL_CELL, max_pairs,
    zero_pairs, one pair a single UNIT_CELL substitution (1 / S) apart, and near-duplicates over the whole alphabet."""
    seqs = length_grid(ALPHA[0] + ALPHA[1], 1)
    a, b = ALPHA[UNIT_CELL[0]], ALPHA[UNIT_CELL[1]]
    for a, b in max_pairs(plan) + zero_pairs(plan) + [(a * 5, a + b + a * 3)]:
        seqs += [s for s in (a, b) if s not in seqs]
    return seqs + near_set(plan.K, ALPHA[:plan.K], 100 - len(seqs), (20, 33))


LANE_QUERIES = (0, 31, 32, 63, 64, 255, 256)


def lane_position_set():
    """257 distinct sequences over ACGU, all 17 long: the stable sort keeps their order, so sorted column p is original
    p, and the query seqs[p] has exactly one column at distance 0 under any table that charges every substitution."""
    rng = np.random.default_rng(257)
    seqs = []
    while len(seqs) < 257:
        s = jc.random_seq(rng, "ACGU", 17)
        if s not in seqs:
            seqs.append(s)
    return seqs


def identical_set():
    """130 copies of one 17-symbol sequence: in a self join at T = 0 every running wave has a full ballot but for the
    lane of the row itself."""
    return [jc.random_seq(np.random.default_rng(130), "ACGU", 17)] * 130


SPLIT_COUNTS = {10: 13, 11: 17, 12: 15, 13: 19, 14: 1}


def split_wave_set(symbols="ACGU"):
    """65 sequences of lengths 10..14 given in interleaved order, 13 / 17 / 15 / 19 / 1 of them: the sorted columns
    change length at lanes 13, 30 and 45 of the first wave and between lanes 63 and 64, the wave edge.  (13 of each
    length would put no boundary on the wave edge.)  Every sequence is a prefix of one base sequence, half of them with
    one substitution, so distances of one or two indels occur."""
    rng = np.random.default_rng(65)
    base = jc.random_seq(rng, symbols, 14)
    left = dict(SPLIT_COUNTS)
    seqs = []
    while any(left.values()):
        for n in sorted(left):
            if left[n]:
                left[n] -= 1
                s, p = base[:n], int(rng.integers(n))
                seqs.append(s[:p] + jc.random_seq(rng, symbols, 1) + s[p + 1:] if rng.random() < 0.5 else s)
    return seqs


def sorted_lengths(seqs):
    """The column lengths in the index's order (a stable sort by length)."""
    return sorted(len(s) for s in seqs)


# ---- cutoffs and the reference's cut ----

def cutoffs(plan, D, S):
    """The integer route's cutoffs: 0, the smallest positive double, 1 / S, the largest occurring distance and one ulp
    below it, both sides of the clamp, and the values whose product with S is huge or overflows."""
    top = float(D.max())
    return [0.0, 5e-324, 1.0 / S, float(np.nextafter(top, 0.0)), top, 65535.0 / S, 65536.0 / S, 1e300,
            sys.float_info.max, INF]


CLAMP_CUTOFFS = (65535.0, 65536.0, 1e300, sys.float_info.max, INF)  # (divided by S on the integer route)


def cutoffs_f64(table, D):
    return jf.cutoffs(table, D)[:-1] + [1e300, sys.float_info.max, INF]


def expected_hits(D, T, S, self_join=False, row_lo=0):
    """join_cases.expected_hits with a product T S >= 65535 (+inf included) read as "every pair": D S <= 32 * 255."""
    p = T * S
    return jc.expected_hits(D, INF if p >= CUT_ALL else T, S, self_join, row_lo)


def classes_differing(got, want, len_rows, len_cols, row_lo=0):
    """The (n, m) classes in which two hit lists differ, for a failure's message."""
    def by_class(h):
        out = {}
        for r, c, d in zip(h["row"].tolist(), h["col"].tolist(), h["dist"].view(np.uint64).tolist()):
            out.setdefault((len_rows[r - row_lo], len_cols[c]), []).append((r, c, d))
        return out
    g, w = by_class(got), by_class(want)
    return sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))


# ---- the scaled DP's lane (sed_join.hip: sed_join_kernel<false>, sed_lane_dp.h), word for word ----

def cost_rows(plan, S):
    """sed_join_costs_rule: row[a][b >> 2] |= ((cost S - ins - del - 1) & 0xFF) << (8 (b & 3)), zeros past K."""
    ins, dele = int(plan.ins * S), int(plan.dele * S)
    row = np.zeros((8, 2), np.int64)
    for a in range(8):
        for b in range(8):
            v = int(plan.sub[a][b] * S) if a < plan.K and b < plan.K else 0
            row[a, b >> 2] |= ((v - ins - dele - 1) & 0xFF) << (8 * (b & 3))
    return row


def scaled_sel(b):
    """sed_scaled_sel: byte 3 <- 0xFF, byte 2 <- table byte b, bytes 1:0 <- 0xFF."""
    return 0x0D000D0D | ((b & 7) << 16)


def perm(s0, s1, sel):
    """v_perm_b32 on arrays: result byte i = byte sel_i of the 8 bytes {s0, s1} (0..3: s1, 4..7: s0), 0x0C -> 0x00,
    0x0D and above -> 0xFF."""
    out = np.zeros_like(sel)
    for i in range(4):
        k = (sel >> (8 * i)) & 0xFF
        byte = np.where(k >= 0x0D, 0xFF, np.where(k == 0x0C, 0, np.where(k >= 4, s0 >> (8 * (k & 3)), s1 >> (8 * (k & 3))) & 0xFF))
        out = out | (byte << (8 * i))
    return out


def umin3(a, b, c):
    return np.minimum(np.minimum(a, b), c)


def scaled_decode(cap, n, m, ins, dele):
    """sed_scaled_decode: (cap - B + ((n del + m ins) << 16) + 0xFFFF) >> 16 in 32-bit words."""
    return ((cap - KB + (((n * dele + m * ins) & M32) << 16) + 0xFFFF) & M32) >> 16


def dp_lane_matrix(plan, S, rows, cols):
    """Every (row, column) pair through the DP variant's lane, side by side in numpy with 32-bit words held in int64:
    the column's 32 perm selectors over its zero-padded codes, V[0..32] = B, n rows of sed_scaled_row over all 32
    columns, the sink select at the column's length m, sed_scaled_decode.  Returns (D S, the smallest key met, the
    largest count a key's low half-word is below B's): the keys are unsigned, so the first must stay above 0, and a
    low half-word that ran below 0 would have borrowed from the distance."""
    ins, dele = int(plan.ins * S), int(plan.dele * S)
    tab = cost_rows(plan, S)
    R, Cn = len(rows), len(cols)
    a = np.zeros((R, MAXLEN), np.int64)
    b = np.zeros((Cn, MAXLEN), np.int64)
    for i, s in enumerate(rows):
        a[i, :len(s)] = plan.encode(s)
    for j, s in enumerate(cols):
        b[j, :len(s)] = plan.encode(s)
    n = np.array([len(s) for s in rows], np.int64)
    m = np.array([len(s) for s in cols], np.int64)
    sel = scaled_sel(b)                                     # [column, j]
    V = np.full((R, Cn, MAXLEN + 1), KB, np.int64)
    lo_key, hi_low = KB, 0
    for i in range(MAXLEN):
        live = (i < n)[:, None]
        cx, cy = tab[a[:, i] & 7, 0][:, None], tab[a[:, i] & 7, 1][:, None]  # cur = tab[row symbol]
        dg = (V[:, :, 0] + perm(cy, cx, sel[None, :, 0])) & M32
        left = V[:, :, 0]
        for j in range(1, MAXLEN + 1):
            up = V[:, :, j]
            dnext = (up + perm(cy, cx, sel[None, :, j])) & M32 if j < MAXLEN else 0
            v = umin3(left, up, dg)
            dg = dnext
            V[:, :, j] = np.where(live, v, up)
            left = v
        lo_key = min(lo_key, int(V.min()))
        hi_low = max(hi_low, int(((KB - V) & 0xFFFF).max()))
    cap = V[:, :, 0]  # m = 0: the border column
    for j in range(1, MAXLEN + 1):
        cap = np.where((j == m)[None, :], V[:, :, j], cap)
    return scaled_decode(cap, n[:, None], m[None, :], ins, dele), lo_key, hi_low


def planner_cut(T, S):
    """sed_join_plan_of: cut = min(floor(T S), SED_JOIN_CUT_ALL), the product exact or +inf."""
    cs = T * S
    return CUT_ALL if cs >= CUT_ALL else math.floor(cs)


def hits_of_scaled(DS, cut, S, self_join=False):
    """The kernel's hit rule D S <= cut on a matrix of scaled distances, as JOIN_HIT_DTYPE records."""
    keep = DS <= cut
    if self_join:
        np.fill_diagonal(keep, False)
    r, c = np.nonzero(keep)
    out = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
    out["row"], out["col"], out["dist"] = r, c, DS[r, c] / float(S)
    return out


# ---- the bit-parallel lane under the planner's 2-bit code map ----

def unit_map(plan, row_codes, col_codes):
    """sed_join_plan.cpp: join_unit_costs, word for word: the 2-bit codes of the codes seen, in code order, two bits
    per code (None: the bit-parallel kernel does not serve these costs and codes)."""
    seen = row_codes | col_codes
    if plan.ins != 1.0 or plan.dele != 1.0 or bin(seen).count("1") > 4:
        return None
    umap = nxt = 0
    for a in range(plan.K):
        if not (seen >> a) & 1:
            continue
        for b in range(plan.K):
            if (row_codes >> a) & 1 and (col_codes >> b) & 1 and plan.sub[a][b] != (0.0 if a == b else 1.0):
                return None
        umap |= nxt << (2 * a)
        nxt += 1
    return umap


def bitpar_matrix(plan, S, rows, cols):
    """D S of every (row, column) pair through the bit-parallel lane: both sides' codes through umap's 2-bit fields,
    test_bitpar_model.bitpar_distance, the sink shifted left by log2 S."""
    umap = unit_map(plan, jc.codes_mask(plan, rows), jc.codes_mask(plan, cols))
    assert umap is not None
    shift = S.bit_length() - 1
    u = lambda s: [(umap >> (2 * (int(c) & 7))) & 3 for c in plan.encode(s)]
    ur, uc = [u(s) for s in rows], [u(s) for s in cols]
    return np.array([[bitpar_distance(x, y) << shift for y in uc] for x in ur], np.int64).reshape(len(rows), len(cols))
