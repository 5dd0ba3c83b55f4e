"""The similarity join over sequences of 0..128 symbols (sed_join_long_self / sed_join_long_search):
the sequence sets, the planner's recount and the two lanes of sed_join_long.hip restated word for word, shared by the
CPU tests (tests/test_join_long_host.py) and the GPU tests (tests/test_gpu_join_long.py, and across the envelope - code
maps and shifts, row and column geometry, the last query's look-ahead, code positions, the cutoff clamp -
tests/test_gpu_join_long_envelope.py).  No device is needed here.  The reference is join_cases.oracle_matrix throughout."""
import math

import numpy as np

import join_cases as jc
import join_envelope as je
import sedgpu

INF = math.inf
MAXLEN = 128   # SED_JOIN_LONG_MAXLEN
BLOCK = 32     # SED_JOIN_LONG_BLOCK: the columns of a block of the DP, the bits of a word of the bit-parallel state
KB = je.KB
M32 = je.M32
LOWEST_KEY = 0x807FFF7C  # B - 128 (255 << 16) - 128: 128 free substitutions under (insert + delete) S = 255
TOP_SCALED = 128 * 255   # the largest scaled distance: 128 substitutions at insert + delete


def unit_plan():
    """costs.json over ACGU: insert = delete = 1 and unit substitutions, the bit-parallel variant's table (S = 1)."""
    return jc.plan_for(jc.load_golden("costs.json"), "ACGU"), 1


def user_plan():
    """user_costs.json over ACGUN (S = 4): the scaled DP."""
    return jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN"), 4


# ---- sequence sets ----

def near_grid(seed, symbols, extra=None):
    """One sequence of every length 0..128, shuffled: prefixes of one 128-mer over `symbols`, each with up to three
    substitutions (from `extra` when given, else from `symbols`), so distances are small and cutoffs split them."""
    rng = np.random.default_rng(seed)
    base = jc.random_seq(rng, symbols, MAXLEN)
    seqs = []
    for n in range(MAXLEN + 1):
        s = list(base[:n])
        for _ in range(int(rng.integers(0, 4)) if n else 0):
            s[int(rng.integers(n))] = jc.random_seq(rng, extra or symbols, 1)
        seqs.append("".join(s))
    return [seqs[i] for i in rng.permutation(len(seqs))]


def length_grid(seed=7):
    """Every length 0..128 once over the symbols of ZERO_CELL / FULL_CELL, shuffled, and the two 128-symbol runs: row
    ALPHA[0] * 128 against column ALPHA[1] * 128 is 128 free substitutions, the other way 128 at insert + delete."""
    rng = np.random.default_rng(seed)
    two = je.ALPHA[0] + je.ALPHA[1]
    seqs = [jc.random_seq(rng, two, n) for n in range(MAXLEN + 1)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    return seqs + [je.ALPHA[0] * MAXLEN, je.ALPHA[1] * MAXLEN]


def extremes_set(plan):
    """A small set with the 128-symbol extremes of one limit table: all-equal pairs (duplicates), all-mismatch pairs at
    insert + delete and at 0 (the two runs, both ways), the empty sequence against 128 symbols both ways, their
    neighbours of 127, and a few sequences over the whole alphabet."""
    a, b = je.ALPHA[0], je.ALPHA[1]
    rng = np.random.default_rng(plan.K)
    al = je.ALPHA[:plan.K]
    mid = jc.random_seq(rng, al, MAXLEN)
    return ["", a * MAXLEN, b * MAXLEN, a * MAXLEN, b * MAXLEN, a * 127, b * 127, a * 64 + b * 64, mid, mid[:100],
            mid[:50] + b + mid[51:], jc.random_seq(rng, al, 97), jc.random_seq(rng, al, 33), a]


GUARD_COUNTS = {32: 13, 33: 13, 64: 13, 65: 12, 96: 13, 97: 1}


def guard_set(symbols="ACGU", extra=None):
    """65 sequences given in interleaved order whose sorted lengths cross 32 / 33 at lane 13 and 64 / 65 at lane 39 of
    the first wave and 96 / 97 on its edge (lane 63 has 96 symbols, the second wave's one column 97): the first wave
    runs three blocks (words), the second four.  Prefixes of one 97-mer, half of them with one substitution."""
    rng = np.random.default_rng(6597)
    base = jc.random_seq(rng, symbols, 97)
    left = dict(GUARD_COUNTS)
    seqs = []
    while any(left.values()):
        for n in sorted(left):
            if left[n]:
                left[n] -= 1
                s, p = base[:n], int(rng.integers(n))
                seqs.append(s[:p] + jc.random_seq(rng, extra or symbols, 1) + s[p + 1:] if rng.random() < 0.5 else s)
    assert len(seqs) == 65
    return seqs


LANE_QUERIES = (0, 63, 64, 255, 256)


def lane_position_set(n=70):
    """257 distinct sequences over ACGU, all n long: the stable sort keeps their order, so sorted column p is original
    p, and the query seqs[p] has exactly one column at distance 0."""
    rng = np.random.default_rng(257 + n)
    seqs = []
    while len(seqs) < 257:
        s = jc.random_seq(rng, "ACGU", n)
        if s not in seqs:
            seqs.append(s)
    return seqs


def identical_set():
    """130 copies of one 128-symbol sequence: a self join at T = 0 has full ballots but for the lane of the row."""
    return [jc.random_seq(np.random.default_rng(131), "ACGU", MAXLEN)] * 130


def random_set(seed=2024, count=300):
    """Lengths U[0, 128] over ACGU with 1 % of a fifth symbol, N, so the scaled DP runs; near-duplicates planted."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < count:
        s = jc.random_seq(rng, "ACGUN", int(rng.integers(0, MAXLEN + 1)), pn=0.01)
        seqs.append(s)
        if len(s) >= 2 and rng.random() < 0.3:
            p = int(rng.integers(len(s)))
            seqs.append(s[:p] + s[p + 1:] if rng.random() < 0.5 else s[:p] + "A" + s[p + 1:])
    return seqs[:count]


# ---- the envelope's sets: code maps and shifts, code positions, the last query, column geometry ----

EDGE_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)  # the word (block) edges and their neighbours


def near_set_long(seed, symbols, count):
    """`count` near-prefixes of one 128-mer over `symbols`: every EDGE_LENGTHS length as the exact prefix and once more
    as a variant, a second exact copy of 32, 96 and 128 symbols (pairs at distance 0), and random lengths 0..128; a
    variant has 0..3 substitutions, or is the prefix of one more symbol with one deletion.  Shuffled."""
    rng = np.random.default_rng(seed)
    base = jc.random_seq(rng, symbols, MAXLEN)
    exact = list(EDGE_LENGTHS) + [32, 96, 128]
    assert count >= len(exact) + len(EDGE_LENGTHS)
    lens = list(EDGE_LENGTHS) + [int(x) for x in rng.integers(0, MAXLEN + 1, size=count - len(exact) - len(EDGE_LENGTHS))]
    seqs = [base[:n] for n in exact]
    for n in lens:
        kind = int(rng.integers(5))
        if kind == 4 and n < MAXLEN:
            p = int(rng.integers(n + 1))
            seqs.append(base[:p] + base[p + 1:n + 1])
        else:
            s = list(base[:n])
            for _ in range(min(kind, 3) if n else 0):
                s[int(rng.integers(n))] = jc.random_seq(rng, symbols, 1)
            seqs.append("".join(s))
    return [seqs[i] for i in rng.permutation(len(seqs))]


def bitpar_long_sets():
    """name -> (plan, S, rows, columns) over je.bitpar_tables(): S > 1 and, but for "costs ACGUN", a code map that is not
    the identity.  The two square sets (rows is columns) are near_set_longs of 100; "one way" has 30 queries over codes
    {0, 1} and one more, the last, carrying a fifth code (which plans the DP), against 70 columns over codes {6, 7}."""
    out = {}
    for name, (plan, S, symbols) in je.bitpar_tables().items():
        if symbols is None:
            rows = near_set_long(11, je.ALPHA[0:2], 30)
            q = max(rows, key=len)
            out[name] = (plan, S, rows + [q[:5] + je.ALPHA[2] + q[5:100]], near_set_long(12, je.ALPHA[6:8], 70))
        else:
            seqs = near_set_long(13 + S, symbols, 100)
            out[name] = (plan, S, seqs, seqs)
    return out


def code_position_set():
    """40 sequences over the eight codes: the rotations of ALPHA[:8] * 16 by 0..7 (code (j + r) % 8 at position j, so
    every code stands at every j & 3 of a code word in every block of 32 columns), each once more with one
    substitution, and the rotations' prefixes of 96, 64 and 32 symbols."""
    rng = np.random.default_rng(8)
    al = je.ALPHA[:8]
    rot = [(al[r:] + al[:r]) * (MAXLEN // 8) for r in range(8)]
    sub = []
    for s in rot:
        p = int(rng.integers(MAXLEN))
        sub.append(s[:p] + al[(al.index(s[p]) + 1 + int(rng.integers(7))) % 8] + s[p + 1:])
    return rot + sub + [s[:n] for n in (96, 64, 32) for s in rot]


def code_positions(seqs):
    """{(code, j & 3, j >> 5)} over the 128-symbol sequences of seqs."""
    return {(je.ALPHA.index(c), j & 3, j >> 5) for s in seqs if len(s) == MAXLEN for j, c in enumerate(s)}


def last_query_sets():
    """(plan, S, columns, query lists, a larger query list) under je's "unit block" table (the bit-parallel variant
    through a code map that is not the identity; the DP when forced).  Every list ends with one 128-symbol query, and
    one list is that query alone: its record is the last of the upload [records | spare | lengths], so the row reader's
    look-ahead past it reads the spare bytes.  The query's last four symbols are the block's four codes, all different
    and nonzero; the columns hold it once exactly and once with two substitutions, among a near_set_long of 40."""
    plan, S, symbols = je.bitpar_tables()["unit block"]
    rng = np.random.default_rng(33)
    head = jc.random_seq(rng, symbols, MAXLEN - 4)
    q128 = head + symbols[2] + symbols[0] + symbols[3] + symbols[1]
    near = q128[:40] + symbols[(symbols.index(q128[40]) + 1) % 4] + q128[41:126] + q128[127] + q128[127]
    cols = near_set_long(34, symbols, 40) + [q128, near]
    other = near_set_long(35, symbols, 30)
    lists = [[q128], other[:3] + [q128], ["", q128[:127], other[5], q128[1:], q128]]
    return plan, S, cols, lists, other[:20]


def column_geometry_set():
    """257 sequences over ACGU for the prefixes seqs[:N], N = 1, 2, 63, 64, 65, 255, 256, 257: the first has 128 symbols
    and every other at most 96, so in each prefix the sorted columns end with that one in the last wave, beside columns
    that stop at or below the 96 / 97 block edge it crosses, and (N & 63 != 0) beside spare lanes that copy it.
    Near-prefixes of one 128-mer, so small cutoffs keep some pairs."""
    rng = np.random.default_rng(257)
    base = jc.random_seq(rng, "ACGU", MAXLEN)
    seqs = [base]
    while len(seqs) < 257:
        s = list(base[:int(rng.integers(0, 97))])
        for _ in range(int(rng.integers(0, 3)) if s else 0):
            s[int(rng.integers(len(s)))] = jc.random_seq(rng, "ACGU", 1)
        seqs.append("".join(s))
    return seqs


COLUMN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257)


def waves_of(nrows, ncols, launch_rows, G=4, block=256):
    """sed_join_plan's "waves": the column blocks x the row groups of every launch x the block's waves."""
    groups = sum((min(launch_rows, nrows - r) + G - 1) // G for r in range(0, nrows, launch_rows))
    return ((ncols + block - 1) // block) * groups * (block // 64) if ncols else 0


# ---- the planner's counts, from their definition ----

def lane_cells(len_rows, len_cols, keep):
    """sed_join_long_plan's out[6]: the columns sorted by length, 64 to a wave (the last wave's spare lanes take the
    longest column); for every wave and every row one of its columns passes keep(n, m) for: 64 lanes x n x the blocks of
    32 columns up to the wave's longest."""
    cols = sorted(len_cols)
    total = 0
    for w in range(0, len(cols), 64):
        wave = cols[w:w + 64]
        longest = cols[-1] if len(wave) < 64 else wave[-1]
        width = BLOCK * ((longest + BLOCK - 1) // BLOCK)
        for n in len_rows:
            if any(keep(n, m) for m in set(wave)):
                total += 64 * n * width
    return total


def keep_rule(ins, dele, T, S):
    """The integer route's length bound within the cutoff, on the integer scale."""
    cut = je.planner_cut(T, S)
    return lambda n, m: (ins * S * max(m - n, 0) + dele * S * max(n - m, 0)) <= cut


# ---- the scaled DP's lane (sed_join_long.hip: sed_join_long_kernel<false, false>), word for word ----

def dp_lane_matrix(plan, S, rows, cols):
    """Every (row, column) pair through the long DP lane, side by side in numpy with 32-bit words held in int64: the
    column's 32 code words; per row symbol one perm with the code word as selector (four cost bytes) and one perm with
    the constant selector 0x0D0t0D0D (the addend of column 4 w + t); V[0..128] = B; a row in blocks of 32 columns, block
    b run when the column reaches it (32 b < m; a wave runs at least those); umin3; the sink select at m;
    sed_scaled_decode.  Returns (D S, the smallest key met, the largest count a key's low half-word is below B's)."""
    ins, dele = int(plan.ins * S), int(plan.dele * S)
    tab = je.cost_rows(plan, S)
    R, Cn = len(rows), len(cols)
    a = np.zeros((R, MAXLEN), np.int64)
    b = np.zeros((Cn, MAXLEN), np.int64)
    for i, s in enumerate(rows):
        a[i, :len(s)] = plan.encode(s)
    for j, s in enumerate(cols):
        b[j, :len(s)] = plan.encode(s)
    n = np.array([len(s) for s in rows], np.int64)
    m = np.array([len(s) for s in cols], np.int64)
    cw = (b[:, 0::4] | (b[:, 1::4] << 8) | (b[:, 2::4] << 16) | (b[:, 3::4] << 24)) & 0x07070707  # [column, word]
    # the addends by row symbol: add[sym, column, j] (a row symbol's perms give the same words in every row)
    add = np.zeros((8, Cn, MAXLEN), np.int64)
    for sym in range(8):
        cx, cy = np.int64(tab[sym, 0]), np.int64(tab[sym, 1])
        for w in range(MAXLEN // 4):
            p = je.perm(np.full(Cn, cy), np.full(Cn, cx), cw[:, w])
            for t in range(4):
                add[sym, :, 4 * w + t] = je.perm(p, p, np.full(Cn, 0x0D000D0D | (t << 16), np.int64))
    nblk = (m + BLOCK - 1) // BLOCK
    V = np.full((R, Cn, MAXLEN + 1), KB, np.int64)
    lo_key, hi_low = KB, 0
    for i in range(MAXLEN):
        live = (i < n)[:, None]
        ad = add[a[:, i] & 7]                                # [row, column, j]
        dg = (V[:, :, 0] + ad[:, :, 0]) & M32
        left = V[:, :, 0]
        for j in range(1, MAXLEN + 1):
            run = live & ((j - 1) // BLOCK < nblk)[None, :]
            up = V[:, :, j]
            dnext = (up + ad[:, :, j]) & M32 if j < MAXLEN else 0
            v = je.umin3(left, up, dg)
            dg = dnext
            V[:, :, j] = np.where(run, v, up)
            left = v
        lo_key = min(lo_key, int(V.min()))
        hi_low = max(hi_low, int(((KB - V) & 0xFFFF).max()))
    cap = V[:, :, 0]  # m = 0: the border column
    for j in range(1, MAXLEN + 1):
        cap = np.where((j == m)[None, :], V[:, :, j], cap)
    return je.scaled_decode(cap, n[:, None], m[None, :], ins, dele), lo_key, hi_low


# ---- the bit-parallel lane over four 32-bit words (sed_lane_dp.h: sed_bitpar_word), word for word ----

def bitpar_word(Pv, Mv, tq, cadd, cph, cmh):
    """One word of one row: returns (Pv, Mv, cadd, cph, cmh); every value a 32-bit word, the carries one bit."""
    eq = ~tq & M32
    Xv = Mv | eq
    s = (Pv & eq) + Pv + cadd
    cadd = s >> 32
    Xh = ((s & M32) ^ Pv) | eq
    ph = (Mv | (~(Xh | Pv) & M32)) & M32
    mh = Pv & Xh
    Ph = ((ph << 1) & M32) | cph
    Mh = ((mh << 1) & M32) | cmh
    return Mh | (~(Xv | Ph) & M32), Ph & Xv, cadd, ph >> 31, mh >> 31


def bitpar_distance(x, y, words=None):
    """The unit-cost distance of 2-bit code lists x (str1, the rows) and y (str2, the bit dimension, at most 128) through
    the long lane: the two bit planes of y over four words, per row symbol every word below `words` (default: those y
    reaches, as a wave of columns of y's length runs) with the addition's carry and the shifts' top bits handed upward
    and the top border's 1 into word 0, then the sink over y's m bits word by word."""
    m = len(y)
    nw = (m + BLOCK - 1) // BLOCK if words is None else words
    assert nw * BLOCK >= m and nw <= MAXLEN // BLOCK
    E0, E1 = [0] * 4, [0] * 4
    for j, u in enumerate(y):
        E0[j >> 5] |= (u & 1) << (j & 31)
        E1[j >> 5] |= (u >> 1) << (j & 31)
    Pv, Mv = [M32] * 4, [0] * 4
    for u in x:
        cadd, cph, cmh = 0, 1, 0
        for k in range(nw):
            tq = (E0[k] ^ (M32 if u & 1 else 0)) | (E1[k] ^ (M32 if u >> 1 else 0))
            Pv[k], Mv[k], cadd, cph, cmh = bitpar_word(Pv[k], Mv[k], tq, cadd, cph, cmh)
    D = len(x)
    for k in range(nw):
        bits = max(m - BLOCK * k, 0)
        keep = M32 if bits >= 32 else (1 << bits) - 1
        D += bin(Pv[k] & keep).count("1") - bin(Mv[k] & keep).count("1")
    return D & M32


# ---- the bit-parallel kernel's lane under the planner's code map (sed_join_long_kernel<true, ...>), word for word ----

SPARE = 16  # sed_join_runtime.cpp: the spare bytes that end a record buffer


def record_words(seqs):
    """[records | spare] as the runtime uploads byte codes (128 zero-padded bytes a sequence), as 32-bit words."""
    buf = np.zeros(MAXLEN * len(seqs) + SPARE, np.uint8)
    for r, c in enumerate(seqs):
        buf[MAXLEN * r:MAXLEN * r + len(c)] = c
    return buf.view("<u4").astype(np.int64)


def popcount(x):
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) & M32) >> 24


def bitpar_lane_matrix(umap, shift, rows, cols, words=0):
    """D S of every (row, column) pair of byte-code arrays through the bit-parallel kernel's lane, side by side in numpy
    with 32-bit words held in int64: the column's 128 zero-padded codes through ubfe(umap, 2 code, 2) into two bit
    planes over four words (the padding maps through umap's field 0); the row reader (w0, w1 and the look-ahead
    pr[(i >> 2) + 2] over [records | spare]); the row symbol through umap; every word k < nblk, nblk = the larger of
    the column's own count and `words` (what a wave with a longer column runs); the sink over m bits; D << shift."""
    NW = MAXLEN // 4
    R, Cn = len(rows), len(cols)
    n = np.array([len(s) for s in rows], np.int64)
    m = np.array([len(s) for s in cols], np.int64)
    pr = record_words(rows)
    base = NW * np.arange(R)
    cw = record_words(cols)[:NW * Cn].reshape(Cn, NW) & 0x07070707
    E0, E1 = np.zeros((Cn, 4), np.int64), np.zeros((Cn, 4), np.int64)
    for j in range(MAXLEN):
        u = (umap >> (2 * ((cw[:, j >> 2] >> (8 * (j & 3))) & 7))) & 3
        E0[:, j >> 5] |= (u & 1) << (j & 31)
        E1[:, j >> 5] |= (u >> 1) << (j & 31)
    nblk = np.maximum((m + BLOCK - 1) // BLOCK, words)
    assert words <= MAXLEN // BLOCK
    Pv = [np.full((R, Cn), M32, np.int64) for _ in range(4)]
    Mv = [np.zeros((R, Cn), np.int64) for _ in range(4)]
    w0, w1 = pr[base], pr[base + 1]
    for i in range(int(n.max()) if R else 0):
        live = i < n
        c = (w0 >> (8 * (i & 3))) & 7
        if (i & 3) == 3:
            w0 = np.where(live, w1, w0)
            w1 = np.where(live, pr[base + (i >> 2) + 2], w1)
        u = (umap >> (2 * c)) & 3
        f0, f1 = np.where(u & 1, M32, 0)[:, None], np.where(u >> 1, M32, 0)[:, None]
        cadd, cph, cmh = np.zeros((R, Cn), np.int64), np.ones((R, Cn), np.int64), np.zeros((R, Cn), np.int64)
        for k in range(4):
            run = live[:, None] & (k < nblk)[None, :]
            tq = (E0[None, :, k] ^ f0) | (E1[None, :, k] ^ f1)
            P, M, cadd, cph, cmh = bitpar_word(Pv[k], Mv[k], tq, cadd, cph, cmh)
            Pv[k], Mv[k] = np.where(run, P, Pv[k]), np.where(run, M, Mv[k])
    D = np.broadcast_to(n[:, None], (R, Cn)).copy()
    for k in range(4):
        bits = np.clip(m - BLOCK * k, 0, 32)
        keep = ((np.int64(1) << bits) - 1)[None, :]
        D += np.where((k < nblk)[None, :], popcount(Pv[k] & keep) - popcount(Mv[k] & keep), 0)
    return (D << shift) & M32


def mapped_matrix(plan, S, rows, cols, words=0):
    """bitpar_lane_matrix of sequences under the planner's map (je.unit_map restates join_unit_costs) and shift log2 S."""
    umap = je.unit_map(plan, jc.codes_mask(plan, rows), jc.codes_mask(plan, cols))
    assert umap is not None
    return bitpar_lane_matrix(umap, S.bit_length() - 1, jc.encode(plan, rows), jc.encode(plan, cols), words)


# ---- an oracle-backed engine for the Python layers ----

class OracleEngine:
    """A JoinIndex engine for wfsearch's index_fn and sedshard's join_fn: the C oracle's distances over the golden
    tables, cut at T.  It records the keywords it was built with."""

    built = []

    def __init__(self, seqs, user_cost=False, **kw):
        self.seqs = list(seqs)
        self.kw = kw
        self.plan = jc.plan_for(jc.load_golden("user_costs.json" if user_cost else "costs.json"), "ACGUN")
        self.closed = False
        OracleEngine.built.append(self)

    def self_join(self, max_dist, rows=None):
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        D = jc.oracle_matrix(self.plan, self.seqs[lo:hi], self.seqs)
        return [(lo + i, j, float(D[i, j])) for i in range(hi - lo) for j in range(len(self.seqs))
                if lo + i != j and D[i, j] <= max_dist]

    def search(self, queries, max_dist):
        D = jc.oracle_matrix(self.plan, list(queries), self.seqs)
        return [(q, j, float(D[q, j])) for q in range(len(queries)) for j in range(len(self.seqs)) if D[q, j] <= max_dist]

    def close(self):
        self.closed = True
