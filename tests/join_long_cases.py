"""The similarity join over sequences of 0..128 symbols (sed_join_long_self / sed_join_long_search):
the sequence sets, the planner's recount and the two lanes of sed_join_long.hip restated word for word, shared by the
CPU tests (tests/test_join_long_host.py) and the GPU tests (tests/test_gpu_join_long.py).  No device is needed here.
The reference is join_cases.oracle_matrix throughout."""
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
