"""The k nearest neighbours on the fp64 route (sed_join_knn_self_f64 / sed_join_knn_search_f64): the
expected trimmed list, the two passes restated on 64-bit keys, the cost tables and sequence sets, and oracle-backed
engines for the Python layers.  Every expected value comes from the C oracle's fp64 matrix (join_cases.oracle_matrix).
Shared by tests/test_join_knn_f64_host.py and tests/test_gpu_join_knn_f64.py.  No device is needed here."""
import math

import numpy as np

import join_cases as jc
import join_f64_cases as jf
import join_knn_cases as kc
import sedgpu

INF = math.inf
WAVE = 64
N1 = jf.MAXLEN + 1


def keys(D):
    """The bit patterns of doubles that are finite or +inf and >= +0, as uint64: they order as the values do."""
    D = np.ascontiguousarray(D, np.float64)
    assert not np.isnan(D).any() and not np.signbit(D).any()
    return D.view(np.uint64)


def expected_knn(D, k, T, self_join=False, row_lo=0):
    """The trimmed list from the oracle's matrix: per row the in-scope columns with D <= T (a plain fp64 compare),
    ordered by (D, column), the first k; JOIN_HIT_DTYPE records sorted by (row, dist, col)."""
    ok = kc.in_scope(D.shape, self_join, row_lo) & (D <= T)
    rows, cols = [], []
    for r in range(D.shape[0]):
        c = np.nonzero(ok[r])[0]
        c = c[np.lexsort((c, D[r, c]))][:k]
        rows += [r] * len(c)
        cols += c.tolist()
    out = np.zeros(len(rows), sedgpu.JOIN_HIT_DTYPE)
    r, c = np.array(rows, np.int64), np.array(cols, np.int64)
    out["row"], out["col"], out["dist"] = r + row_lo, c, D[r, c] if len(r) else []
    return out


def lower_table(plan):
    return sedgpu.join_f64_lower(plan.ins, plan.dele)


def lower_model(ins, dele):
    """sed_join_plan.cpp: sed_join_f64_lower_rule, word for word."""
    ins, dele = float(ins) + 0.0, float(dele) + 0.0
    low = np.zeros((N1, N1))
    for n in range(N1):
        for m in range(N1):
            if n == 0 or m == 0:
                low[n, m] = float(m) * ins if n == 0 else float(n) * dele
            elif n != m:
                p = float(m - n) * ins if m > n else float(n - m) * dele
                if math.isfinite(p) and p >= 2.0 ** -900:
                    low[n, m] = p - p * 2.0 ** -40
    return low


def pass1_by_definition(D, len_cols, k, T, self_join=False, row_lo=0):
    """bound[r] = min(T, the smallest k-th smallest of any wave that has k in-scope columns within T), whatever the
    schedule, and the candidates {in scope, D <= bound[r]}: the columns in the index's order (a stable sort by length),
    64 to a wave."""
    ok = kc.in_scope(D.shape, self_join, row_lo)
    order = np.argsort(np.asarray(len_cols), kind="stable")
    bound = np.full(D.shape[0], float(T))
    for w in range(0, len(order), WAVE):
        wave = order[w:w + WAVE]
        for r in range(D.shape[0]):
            v = np.sort(D[r, wave][ok[r, wave]])
            if len(v) >= k and v[k - 1] <= T:
                bound[r] = min(bound[r], v[k - 1])
    return bound, int((ok & (D <= bound[:, None])).sum())


def kth_by_bisection(key_lane, cand, k):
    """The kernel's 63 rounds, word for word, on the (up to) 64 lanes of the last axis: x = 0; for bit 62..0: c = x | 1 <<
    bit; if popcount(cand && key < c) < k: x = c.  With at least k candidates x ends as their k-th smallest key."""
    key_lane, cand = np.asarray(key_lane, np.uint64), np.asarray(cand, bool)
    x = np.zeros(key_lane.shape[:-1], np.uint64)
    for bit in range(62, -1, -1):
        c = x | np.uint64(1 << bit)
        x = np.where((cand & (key_lane < c[..., None])).sum(-1) < k, c, x)
    return x


def low_of(low, len_rows, len_cols):
    return np.asarray(low)[np.asarray(len_rows, np.int64)[:, None], np.asarray(len_cols, np.int64)[None, :]]


def bound_pass_model(D, ok, len_rows, len_cols, low, k, T, order="sequential", kth=kth_by_bisection, read=None):
    """sed_join_f64.hip's pass 1 wave by wave, as join_knn_cases.bound_pass_model states the integer one: per wave and row
    b = the bound read; go = ok && low[n][m] <= b; nothing when no lane goes; cand = go && D <= b; nothing when fewer
    than k candidates; x = the bisection on the keys; atomicMin(bound[r], x) when x < b's key.  `order` as there.  `read`
    (tests of the tests): what a wave makes of the 64-bit word it loaded, the identity in the kernel.  Returns (the final
    bounds as doubles, the pairs the pass ran)."""
    D, ok = np.asarray(D, np.float64), np.asarray(ok, bool)
    K = keys(D)
    R = D.shape[0]
    lo = low_of(low, len_rows, len_cols)
    index = np.argsort(np.asarray(len_cols), kind="stable")
    waves = [index[w:w + WAVE] for w in range(0, len(index), WAVE)]
    seq, rng = list(range(len(waves))), None
    if order == "reverse":
        seq.reverse()
    elif order not in ("sequential", "stale"):
        rng = np.random.default_rng(order)
        seq = rng.permutation(len(waves)).tolist()
    bound = np.full(R, keys(np.float64(T) + 0.0), np.uint64)
    history, pairs = [bound], 0
    for w in seq:
        lanes = waves[w]
        if order == "stale":
            b = history[0]
        elif rng is not None:
            b = np.stack(history)[rng.integers(len(history), size=R), np.arange(R)]
        else:
            b = bound
        if read is not None:
            b = read(b)
        bd = b.view(np.float64)
        go = ok[:, lanes] & (lo[:, lanes] <= bd[:, None])
        pairs += int(go.sum())
        cand = go & (D[:, lanes] <= bd[:, None])
        x = kth(K[:, lanes], cand, k)
        write = go.any(1) & (cand.sum(1) >= k) & (x < b)
        bound = np.where(write, np.minimum(bound, x), bound)
        history.append(bound)
    return bound.view(np.float64), pairs


def emit_pass_model(D, ok, len_rows, len_cols, low, bound, read=None):
    """Pass 2: go = ok && low[n][m] <= bound[r]; (the candidates' mask go && D <= bound[r], the pairs run, the (wave,
    row) that no lane went for).  `read` as in bound_pass_model."""
    b = np.ascontiguousarray(bound, np.float64)
    if read is not None:
        b = read(b.view(np.uint64)).view(np.float64)
    b = b[:, None]
    go = np.asarray(ok, bool) & (low_of(low, len_rows, len_cols) <= b)
    index = np.argsort(np.asarray(len_cols), kind="stable")
    skipped = sum(int((~go[:, index[w:w + WAVE]].any(1)).sum()) for w in range(0, len(index), WAVE))
    return go & (np.asarray(D) <= b), int(go.sum()), skipped


def pairs_at(ok, len_rows, len_cols, low, T):
    """The pairs in scope the length skip keeps at one cutoff for every row: the fp64 plan's run."""
    return int((np.asarray(ok, bool) & (low_of(low, len_rows, len_cols) <= T)).sum())


# ---- cost tables: name -> (table, alphabet) ----

def near_tie_table():
    """insert 0.1, delete 0.2, substitutions 0.3 and 1/3: 0.2 + 0.1 != 0.3 in fp64, so one substitution and one shift lie
    an ulp apart."""
    al = "ACGU"
    return {"insert": 0.1, "delete": 0.2,
            "update": {a: {b: (0.0 if a == b else (0.3 if (i + j) % 2 else 1 / 3)) for j, b in enumerate(al)}
                       for i, a in enumerate(al)}}, al


def flat_table(v, ins=None, dele=None):
    al = "ACGU"
    return {"insert": v if ins is None else ins, "delete": v if dele is None else dele,
            "update": {a: {b: (0.0 if a == b else v) for b in al} for a in al}}, al


def tables():
    out = {"costs15": (jc.load_golden("costs.json"), jf.IUPAC), "costs N": (jc.load_golden("costs.json"), "ACGUN"),
           "near ties": near_tie_table(), "overflow": flat_table(1e308), "zero": flat_table(0.0),
           "spread": jf.rounding_table()}
    return out


# ---- sequence sets ----

def iupac_set(seed=15, count=300):
    """Sequences of 20..32 symbols over all 15 IUPAC codes, with near-duplicates: the integer route refuses them."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < count:
        s = jc.random_seq(rng, jf.IUPAC, int(rng.integers(20, 33)))
        seqs.append(s)
        if rng.random() < 0.3 and len(seqs) < count:
            p = int(rng.integers(len(s)))
            seqs.append(s[:p] + jc.random_seq(rng, jf.IUPAC, 1) + s[p + 1:])
    return [seqs[i] for i in rng.permutation(count)]


def near_tie_set(seed=3, groups=12, others=100):
    """Per group a base s of 28 symbols, s with one substitution that costs 0.3, and s shifted (its first symbol
    removed, one appended: 0.2 + 0.1); then random sequences of 28 symbols."""
    rng = np.random.default_rng(seed)
    table, al = near_tie_table()
    seqs = []
    for _ in range(groups):
        s = jc.random_seq(rng, al, 28)
        p = int(rng.integers(4, 24))
        c = next(b for b in al if b != s[p] and table["update"][s[p]][b] == 0.3)
        seqs += [s, s[:p] + c + s[p + 1:], s[1:] + jc.random_seq(rng, al, 1)]
    seqs += [jc.random_seq(rng, al, 28) for _ in range(others)]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def overflow_set(seed=8, count=140):
    """Random sequences of 24..32 symbols with duplicates and one-substitution neighbours: under costs of 1e308 two edits
    overflow to +inf, so most of a row's columns lie at +inf, a few at 0 and at 1e308."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < count:
        s = jc.random_seq(rng, "ACGU", int(rng.integers(24, 33)))
        seqs.append(s)
        r = rng.random()
        p = int(rng.integers(len(s)))
        if r < 0.3 and len(seqs) < count:
            seqs.append(s)
        elif r < 0.6 and len(seqs) < count:
            seqs.append(s[:p] + jc.random_seq(rng, "ACGU".replace(s[p], ""), 1) + s[p + 1:])
    return [seqs[i] for i in rng.permutation(count)]


def spread_set(seed=32, count=300):
    """Lengths spread over 0..32, several empty sequences, prefixes of a few bases so that neighbours are near."""
    rng = np.random.default_rng(seed)
    bases = [jc.random_seq(rng, "ACGU", 32) for _ in range(3)]
    seqs = ["", "", ""]
    while len(seqs) < count:
        s = list(bases[int(rng.integers(3))][:int(rng.integers(0, 33))])
        for _ in range(int(rng.integers(0, 3)) if s else 0):
            s[int(rng.integers(len(s)))] = "ACGU"[int(rng.integers(4))]
        seqs.append("".join(s))
    return [seqs[i] for i in rng.permutation(count)]


class Case:
    """A table, its plan, a set of columns and the oracle's matrix of the columns against themselves (computed once,
    never changed)."""

    def __init__(self, table_name, seqs):
        table, al = tables()[table_name]
        self.plan = jc.plan_for(table, al)
        self.seqs = seqs
        self.lens = [len(s) for s in seqs]
        self.D = jc.oracle_matrix(self.plan, seqs, seqs)
        self.D.setflags(write=False)
        self.low = lower_table(self.plan)


_CASES = {}


def case(name):
    if name not in _CASES:
        make = {"random N": lambda: Case("costs N", kc.random_set()),
                "iupac": lambda: Case("costs15", iupac_set()),
                "ties": lambda: Case("costs N", kc.tie_set()[0]),
                "near ties": lambda: Case("near ties", near_tie_set()),
                "overflow": lambda: Case("overflow", overflow_set()),
                "zero": lambda: Case("zero", jc.mixed_set(77, "ACGU", 140)),
                "spread": lambda: Case("spread", spread_set())}
        _CASES[name] = make[name]()
    return _CASES[name]


# ---- oracle-backed engines for the Python layers ----

class OracleEngine:
    """A JoinIndex engine for wfsearch's index_fn: the C oracle over the golden tables (costs.json over the 15 IUPAC
    symbols), with the integer calls and their _f64 twins; it records its keywords and which calls served.  The integer
    calls refuse IUPAC symbols as the engine does."""

    built = []

    def __init__(self, seqs, user_cost=False, **kw):
        self.seqs = list(seqs)
        self.kw = kw
        self.plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN") if user_cost else \
            jc.plan_for(jc.load_golden("costs.json"), jf.IUPAC)
        self.calls = []
        self.closed = False
        OracleEngine.built.append(self)

    def _int(self, rows):
        if any(c not in "ACGUN" for s in list(rows) + self.seqs for c in s):
            raise sedgpu.SedError("join: 15 symbols (the scaled cost rows hold at most 8)")

    def self_nearest(self, k, max_dist=None, rows=None, _name="self_nearest"):
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        self.calls.append(_name)
        if _name == "self_nearest":
            self._int(self.seqs[lo:hi])
        return kc._nearest(jc.oracle_matrix(self.plan, self.seqs[lo:hi], self.seqs), k, max_dist, True, lo)

    def search_nearest(self, queries, k, max_dist=None, _name="search_nearest"):
        self.calls.append(_name)
        if _name == "search_nearest":
            self._int(queries)
        return kc._nearest(jc.oracle_matrix(self.plan, list(queries), self.seqs), k, max_dist)

    def self_nearest_f64(self, k, max_dist=None, rows=None):
        return self.self_nearest(k, max_dist, rows, "self_nearest_f64")

    def search_nearest_f64(self, queries, k, max_dist=None):
        return self.search_nearest(queries, k, max_dist, "search_nearest_f64")

    def close(self):
        self.closed = True


class CodesEngine(kc.CodesEngine):
    """join_knn_cases.CodesEngine with the fp64 calls of StringEditDistance.join_index's engine."""

    def self_knn_f64(self, plan, k, max_dist, rows):
        out = self.self_knn(plan, k, max_dist, rows)
        self.calls[-1] = ("self_knn_f64",) + self.calls[-1][1:]
        return out

    def search_knn_f64(self, plan, packed, k, max_dist):
        out = self.search_knn(plan, packed, k, max_dist)
        self.calls[-1] = ("search_knn_f64",) + self.calls[-1][1:]
        return out
