"""The k nearest neighbours of every sequence (sed_join_knn_self / sed_join_knn_search and their _long_ twins, DESIGN.md
3.6o): the sequence sets, the expected trimmed list and a numpy model of the kernels' first pass, all from the C
oracle's distance matrix (join_cases.oracle_matrix), and oracle-backed engines for the Python layers.  Shared by
tests/test_join_knn_host.py and tests/test_gpu_join_knn.py.  No device is needed here."""
import math

import numpy as np

import join_cases as jc
import join_long_cases as jl
import sedgpu

INF = math.inf
CUT_ALL = 65535  # SED_JOIN_CUT_ALL: the cutoff on the integer scale that admits every pair
WAVE = 64


def scaled(D, S):
    """D * S as exact integers."""
    DS = np.rint(np.asarray(D) * S).astype(np.int64)
    assert np.array_equal(DS / S, D)
    return DS


def cut_of(T, S):
    return CUT_ALL if T == INF else min(int(math.floor(T * S)), CUT_ALL)


def in_scope(shape, self_join, row_lo):
    ok = np.ones(shape, bool)
    if self_join:
        for r in range(shape[0]):
            ok[r, row_lo + r] = False
    return ok


def expected_knn(D, k, T, S, self_join=False, row_lo=0):
    """The trimmed list from the oracle's matrix: per row the in-scope columns with D * S <= floor(T * S), ordered by
    (D * S, column), the first k; JOIN_HIT_DTYPE records sorted by (row, dist, col).  D's row r is row row_lo + r."""
    DS, cut = scaled(D, S), cut_of(T, S)
    ok = in_scope(D.shape, self_join, row_lo) & (DS <= cut)
    rows, cols = [], []
    for r in range(D.shape[0]):
        c = np.nonzero(ok[r])[0]
        c = c[np.lexsort((c, DS[r, c]))][:k]
        rows += [r] * len(c)
        cols += c.tolist()
    out = np.zeros(len(rows), sedgpu.JOIN_HIT_DTYPE)
    r, c = np.array(rows, np.int64), np.array(cols, np.int64)
    out["row"], out["col"], out["dist"] = r + row_lo, c, D[r, c] if len(r) else []
    return out


def pass1_model(D, len_cols, k, T, S, self_join=False, row_lo=0):
    """(bound[r] of every row, the candidates) as the two passes leave them, whatever the schedule: the columns in the
    index's order (a stable sort by length), 64 to a wave, the last wave partial; a wave with k in-scope columns at
    D * S <= cut contributes its k-th smallest; bound[r] = min(cut, those); candidates = the in-scope pairs with
    D * S <= bound[r]."""
    DS, cut = scaled(D, S), cut_of(T, S)
    ok = in_scope(D.shape, self_join, row_lo)
    order = np.argsort(np.asarray(len_cols), kind="stable")
    bound = np.full(D.shape[0], cut, np.int64)
    for w in range(0, len(order), WAVE):
        wave = order[w:w + WAVE]
        for r in range(D.shape[0]):
            v = np.sort(DS[r, wave][ok[r, wave]])
            if len(v) >= k and v[k - 1] <= cut:
                bound[r] = min(bound[r], v[k - 1])
    return bound, int((ok & (DS <= bound[:, None])).sum())


def pass2_pairs(len_rows, len_cols, bound, ins, dele, S, self_join=False, row_lo=0):
    """The pairs pass 2 runs: in scope, with the length bound (insert (m - n)+ + delete (n - m)+) S <= bound[r]."""
    n, m = np.asarray(len_rows)[:, None], np.asarray(len_cols)[None, :]
    lb = np.rint((ins * np.maximum(m - n, 0) + dele * np.maximum(n - m, 0)) * S).astype(np.int64)
    return int((in_scope(lb.shape, self_join, row_lo) & (lb <= np.asarray(bound)[:, None])).sum())


# ---- sequence sets ----

def random_set(seed=300, count=300, symbols="ACGUN", pn=0.01):
    """`count` sequences of 20..32 symbols: over ACGU with 1 % N (the scaled DP under user_costs.json), or over ACGU
    alone with pn = 0 (the bit-parallel variant under costs.json).  300 columns are 2 blocks and 5 waves, the last of
    44 lanes."""
    rng = np.random.default_rng(seed)
    return [jc.random_seq(rng, symbols, int(rng.integers(20, 33)), pn) for _ in range(count)]


def tie_set(copies=70, others=200, seed=70):
    """`copies` copies of one sequence scattered among `others` random ones: all of one length, so the stable sort keeps
    their order and the copies of a wave are that wave's lowest distances."""
    rng = np.random.default_rng(seed)
    one = jc.random_seq(rng, "ACGU", 28)
    seqs = [jc.random_seq(rng, "ACGU", 28) for _ in range(others)]
    assert one not in seqs
    at = np.sort(rng.choice(others + copies, copies, replace=False))
    for p in at:
        seqs.insert(int(p), one)
    return seqs, [int(p) for p in at]


def lone_pair_set(seed=11):
    """130 sequences: three waves of columns.  Sequence 0 and sequence 129 are one substitution apart and far from all
    others, which are random: with k = 1 the nearest of row 0 sits in the last wave (2 lanes), whose only other in-scope
    column for that row is far."""
    rng = np.random.default_rng(seed)
    a = "ACGU" * 7
    seqs = [a] + [jc.random_seq(rng, "ACGU", 28) for _ in range(128)] + [a[:13] + "A" + a[14:]]
    assert a[13] != "A" and len(seqs) == 130
    return seqs


LONG_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)


def long_set(seed=128, count=300, symbols="ACGUN", pn=0.01):
    """`count` sequences whose lengths straddle 32 / 64 / 96 / 128 (waves of 1..4 column blocks): every LONG_LENGTHS
    length, then lengths within 3 of 29, 60, 96 and 126; near-prefixes of four 128-mers, so neighbours are near."""
    rng = np.random.default_rng(seed)
    bases = [jc.random_seq(rng, symbols, jl.MAXLEN, pn) for _ in range(4)]
    letters = [c for c in symbols if c != "N"]
    seqs = []
    for i in range(count):
        n = LONG_LENGTHS[i] if i < len(LONG_LENGTHS) else int(np.clip(rng.choice([29, 60, 96, 126]) + rng.integers(-3, 4), 0, 128))
        s = list(bases[int(rng.integers(4))][:n])
        for _ in range(int(rng.integers(0, 6)) if n else 0):
            s[int(rng.integers(n))] = letters[int(rng.integers(len(letters)))]
        seqs.append("".join(s))
    return [seqs[i] for i in rng.permutation(count)]


# ---- oracle-backed engines for the Python layers ----

def _nearest(D, k, max_dist, skip=None, row_lo=0):
    """[(row, j, dist)] sorted by (row, dist, j): the first k of every row within max_dist (None: no cap)."""
    out = []
    for r in range(D.shape[0]):
        c = [(float(D[r, j]), j) for j in range(D.shape[1])
             if not (skip and row_lo + r == j) and (max_dist is None or D[r, j] <= max_dist)]
        out += [(row_lo + r, j, d) for d, j in sorted(c)[:k]]
    return out


class OracleEngine(jl.OracleEngine):
    """join_long_cases.OracleEngine with the k-nearest calls of wfsearch's index_fn protocol."""

    def self_nearest(self, k, max_dist=None, rows=None):
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        return _nearest(jc.oracle_matrix(self.plan, self.seqs[lo:hi], self.seqs), k, max_dist, True, lo)

    def search_nearest(self, queries, k, max_dist=None):
        return _nearest(jc.oracle_matrix(self.plan, list(queries), self.seqs), k, max_dist)


class CodesEngine:
    """An engine of StringEditDistance.join_index (codes, off, lens -> self_knn / search_knn over a CostPlan): the C
    oracle over the codes it was given, as JOIN_HIT_DTYPE records.  It records its keywords and calls."""

    built = []

    def __init__(self, codes, off, lens, **kw):
        self.seqs = [np.asarray(codes[o:o + n], np.uint8) for o, n in zip(off, lens)]
        self.kw = kw
        self.calls = []
        CodesEngine.built.append(self)

    def _matrix(self, plan, rows):
        if not rows or not self.seqs:
            return np.zeros((len(rows), len(self.seqs)))
        import oracle
        pp = sedgpu.PackedPairs([a for a in rows for _ in self.seqs], [b for _ in rows for b in self.seqs])
        d = oracle.batch(oracle.Costs.from_plan(plan), pp.codes_a, pp.off_a, pp.len_a, pp.codes_b, pp.off_b, pp.len_b,
                         pp.npairs, nthreads=4)[0]
        return d.reshape(len(rows), len(self.seqs))

    @staticmethod
    def _records(hits):
        out = np.zeros(len(hits), sedgpu.JOIN_HIT_DTYPE)
        for i, h in enumerate(hits):
            out[i] = h
        return out

    def self_knn(self, plan, k, max_dist, rows):
        self.calls.append(("self_knn", k, max_dist, rows))
        lo, hi = rows
        return self._records(_nearest(self._matrix(plan, self.seqs[lo:hi]), k, max_dist, True, lo))

    def search_knn(self, plan, packed, k, max_dist):
        self.calls.append(("search_knn", k, max_dist, packed.npairs))
        q = [packed.codes_a[o:o + n] for o, n in zip(packed.off_a, packed.len_a)]
        return self._records(_nearest(self._matrix(plan, q), k, max_dist))

    def close(self):
        pass
