"""The k nearest neighbours of every sequence (sed_join_knn_self / sed_join_knn_search and their _long_ twins, DESIGN.md
3.6o): the sequence sets, the expected trimmed list and a numpy model of the kernels' first pass, all from the C
oracle's distance matrix (join_cases.oracle_matrix), and oracle-backed engines for the Python layers.  Shared by
tests/test_join_knn_host.py and tests/test_gpu_join_knn.py.  No device is needed here.

The envelope (the second half of this file): the bound pass restated wave by wave with its bisection word for word
(kth_by_bisection, bound_pass_model) under several schedules, the emit pass (emit_pass_model), the ladders that reach the
bisection's high bits, and the list of every call tests/test_gpu_join_knn_envelope.py makes (envelope_calls), which
tests/test_join_knn_host.py proves on the CPU first."""
import math
import sys

import numpy as np

import join_cases as jc
import join_envelope as je
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
    """sed_join_plan_of's cut: min(floor(T S), SED_JOIN_CUT_ALL); the product may be +inf (T = the largest double)."""
    p = T * S
    return CUT_ALL if p >= CUT_ALL else int(math.floor(p))


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


# ---- the bound pass, restated (sed_join_dev.h: sed_join_knn_bound_rows) ----

def kth_by_bisection(D_lane, cand, k):
    """The kernel's 16 rounds, word for word, on the (up to) 64 lanes of the last axis: x = 0; for bit 15..0: c = x | 1 <<
    bit; if popcount(cand && D < c) < k: x = c.  With at least k candidates x ends as their k-th smallest D."""
    D_lane, cand = np.asarray(D_lane, np.int64), np.asarray(cand, bool)
    x = np.zeros(D_lane.shape[:-1], np.int64)
    for bit in range(15, -1, -1):
        c = x | (1 << bit)
        x = np.where((cand & (D_lane < c[..., None])).sum(-1) < k, c, x)
    return x


def length_bound(len_rows, len_cols, ins_S, del_S):
    """lb = m > n ? (m - n) insert S : (n - m) delete S, of every (row, column)."""
    n, m = np.asarray(len_rows, np.int64)[:, None], np.asarray(len_cols, np.int64)[None, :]
    return np.where(m > n, (m - n) * ins_S, (n - m) * del_S)


ORDERS = ("sequential", "reverse", "stale", 1, 2)  # the schedules of bound_pass_model; a number seeds a random one


def bound_pass_model(DS, ok, len_rows, len_cols, ins_S, del_S, k, cut, order="sequential", kth=kth_by_bisection):
    """sed_join_knn_bound_rows wave by wave.  DS[r, c] = the scaled distance pair() returns, ok = the pairs in scope
    (valid and not the row's own column), the columns in the index's order (a stable sort by length), 64 to a wave.  Per
    wave and row: b = the bound read; lb; go = ok && lb <= b; nothing when no lane goes; cand = go && D <= b; nothing
    when fewer than k candidates; x = the bisection; atomicMin(bound[r], x) when x < b.  `order`: "sequential" (the
    waves in index order, each reading the bound as the one before left it), "reverse", "stale" (every wave reads b =
    cut), or a seed (the waves in a random order, each row reading a random earlier value of its bound, as a relaxed
    load may return).  Returns (the final bounds, the pairs the pass ran: the lanes that went, which depends on the
    order, [(wave, x of every row that wrote, else -1)] in the order written)."""
    DS, ok = np.asarray(DS, np.int64), np.asarray(ok, bool)
    R = DS.shape[0]
    lb = length_bound(len_rows, len_cols, ins_S, del_S)
    index = np.argsort(np.asarray(len_cols), kind="stable")
    waves = [index[w:w + WAVE] for w in range(0, len(index), WAVE)]
    seq, rng = list(range(len(waves))), None
    if order == "reverse":
        seq.reverse()
    elif order not in ("sequential", "stale"):
        rng = np.random.default_rng(order)
        seq = rng.permutation(len(waves)).tolist()
    bound = np.full(R, cut, np.int64)
    history, pairs, writes = [bound], 0, []
    for w in seq:
        lanes = waves[w]
        if order == "stale":
            b = history[0]
        elif rng is not None:
            b = np.stack(history)[rng.integers(len(history), size=R), np.arange(R)]
        else:
            b = bound
        go = ok[:, lanes] & (lb[:, lanes] <= b[:, None])
        pairs += int(go.sum())
        cand = go & (DS[:, lanes] <= b[:, None])
        x = kth(DS[:, lanes], cand, k)
        write = go.any(1) & (cand.sum(1) >= k) & (x < b)
        bound = np.where(write, np.minimum(bound, x), bound)
        history.append(bound)
        writes.append((w, np.where(write, x, -1)))
    return bound, pairs, writes


def emit_pass_model(DS, ok, len_rows, len_cols, ins_S, del_S, bound):
    """sed_join_knn_emit_rows: go = ok && lb <= bound[r]; the candidates appended = go && D <= bound[r] (a mask), and the
    pairs the pass runs = the lanes that went (pass2_pairs' count)."""
    b = np.asarray(bound, np.int64)[:, None]
    go = np.asarray(ok, bool) & (length_bound(len_rows, len_cols, ins_S, del_S) <= b)
    return go & (np.asarray(DS, np.int64) <= b), int(go.sum())


# ---- the ladders: distances up to the largest the planner admits, all in one wave ----

def ladder(plan, L, lo, hi, copies=1):
    """(the query a * L, the columns a^(L - j) b^j for j = lo..hi, each `copies` times) for (a -> b) the cell of a limit
    table that je.max_pairs picks (cost = insert + delete).  All columns have L symbols, so the index's order is the
    list's.  Column j is j substitutions at insert + delete from the query - about 255 j on the integer scale, exactly
    what the oracle's matrix says (i127_d128 charges a -> a too)."""
    a, b = je.max_pairs(plan)[0]
    a, b = a[0], b[0]
    return a * L, [a * (L - j) + b * j for j in range(lo, hi + 1) for _ in range(copies)]


FAR_K = (1, 2, 31, 32, 33, 63, 64)
TOP_SHORT, TOP_LONG = 32 * 255, 128 * 255  # the largest D * S of either index: 8160 and 32640


# ---- the envelope's sets: name -> (plan, S, columns, queries, D of the columns against themselves, D of the queries) ----

class EnvelopeSet:
    def __init__(self, plan, S, cols, queries=None):
        """queries None: the columns themselves (one matrix serves the self joins and the searches)."""
        self.plan, self.S, self.cols = plan, S, cols
        self.queries = cols if queries is None else queries
        self._D = None
        self.Dq = self.D if queries is None else jc.oracle_matrix(plan, queries, cols)
        self.Dq.setflags(write=False)
        self.ins_S, self.del_S = int(round(plan.ins * S)), int(round(plan.dele * S))

    @property
    def D(self):
        """The columns against themselves (computed when a self join first asks)."""
        if self._D is None:
            self._D = jc.oracle_matrix(self.plan, self.cols, self.cols)
            self._D.setflags(write=False)
        return self._D


def _near(s):
    return s[:len(s) // 2] + s[len(s) // 2 + 1:]


def _make_set(what, kind, arg=None):
    lng = kind == "long"
    L = jl.MAXLEN if lng else je.MAXLEN
    if what in ("far", "near", "limit"):  # (the limit tables: the scaled DP)
        plan, S = je.limit_tables()[arg]
        if what == "far":    # 64 columns, one wave: j = 65..128, or every j = 1..32 twice
            q, cols = ladder(plan, L, 65, 128) if lng else ladder(plan, L, 1, 32, copies=2)
            return EnvelopeSet(plan, S, cols, [q])
        if what == "near":   # j = 0..L: 33 columns, or 129 in three waves
            q, cols = ladder(plan, L, 0, L)
            return EnvelopeSet(plan, S, cols, [q])
        return EnvelopeSet(plan, S, jl.extremes_set(plan) + jl.near_grid(6, je.ALPHA[:plan.K])[:40] if lng else je.limit_set(plan))
    if what == "limit wide":  # every length 0..128: three waves of columns, so the length skip can leave a whole wave out
        plan, S = je.limit_tables()[arg]
        return EnvelopeSet(plan, S, jl.extremes_set(plan) + jl.near_grid(6, je.ALPHA[:plan.K]))
    if what == "bitpar":
        plan, S, symbols = je.bitpar_tables()[arg]
        return EnvelopeSet(plan, S, jl.bitpar_long_sets()[arg][2] if lng else je.near_set(13, symbols, 100))
    if what == "one way":    # the last query carries a fifth code
        plan, S, _ = je.bitpar_tables()["one way"]
        if lng:
            _, _, rows, cols = jl.bitpar_long_sets()["one way"]
            return EnvelopeSet(plan, S, cols, rows)
        queries = je.near_set(11, je.ALPHA[0:2], 40)
        return EnvelopeSet(plan, S, je.near_set(12, je.ALPHA[6:8], 100), queries + [queries[3][:5] + je.ALPHA[2] + queries[3][5:31]])
    if what == "geometry":   # 140 columns in three waves; 11 queries: three row groups, the last of 3 rows
        plan, S = jl.user_plan()
        cols = long_set(128, 140) if lng else jc.mixed_set(31, "ACGUN", 140, pn=0.01)
        full = max(cols, key=len)
        top = full + "ACGU" * ((L - len(full)) // 4)
        assert len(top) == L and "" in cols
        return EnvelopeSet(plan, S, cols, [cols[11], cols[11], "", top, cols[40], _near(cols[40]), "ACG", _near(cols[77]), cols[3],
                                           _near(cols[100]), cols[139]])
    plan, S = jl.unit_plan()
    if what == "ties":
        return EnvelopeSet(plan, S, tie_set()[0])
    if what == "columns":
        return EnvelopeSet(plan, S, jl.column_geometry_set() if lng else je.lane_position_set())
    if what == "identical":
        return EnvelopeSet(plan, S, jl.identical_set() if lng else je.identical_set())
    if what == "lanes":
        return EnvelopeSet(plan, S, jl.lane_position_set() if lng else je.lane_position_set())
    raise KeyError(what)


_ENV = {}  # computed once, shared, never changed


def envelope_set(name):
    if name in (("ties", "long"), ("lanes", "short")):  # the same sequences under the same table: one matrix
        name = ("ties", "short") if name[0] == "ties" else ("columns", "short")
    if name not in _ENV:
        _ENV[name] = _make_set(*name)
    return _ENV[name]


# ---- the envelope's calls ----

FORCED_DP = ((sedgpu.SED_OPT_JOIN_DP, 2),)
CLAMP_CAPS = ("65535 / S", "65536 / S", 1e300, sys.float_info.max)
LAUNCH_ROWS = (0, 4, 8)  # SED_OPT_JOIN_ROWS: one launch, launches of one row group, of two


class Call:
    """One self_knn (queries None; rows = (lo, hi) or None) or search_knn (queries = indices into the set's queries) of
    tests/test_gpu_join_knn_envelope.py: `group` its test, `case` the test's parameter, `ncols` the prefix of the set's
    columns the index holds (None: all), `options` the context's options during the call, `note` what the test asks of
    it beyond the common checks."""

    def __init__(self, group, case, set_name, k, T=INF, rows=None, queries=None, ncols=None, options=(), note=""):
        self.group, self.case, self.set, self.kind, self.k, self.T = group, case, set_name, set_name[1], k, T
        self.rows, self.queries, self.ncols, self.options, self.note = rows, queries, ncols, tuple(options), note

    def key(self):
        """What the models depend on (the options change the launches and the kernel, never the result)."""
        return (self.set, self.k, self.T, self.rows, None if self.queries is None else tuple(self.queries), self.ncols)

    def __repr__(self):
        return "Call(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()) if kv[1] not in (None, (), ""))


def short_cap(D, k, S):
    """tests/test_gpu_join_knn.py's a_short_cap: the median over the rows of the k-th nearest."""
    from test_gpu_join_knn import a_short_cap
    return a_short_cap(D, k, S)


def _kth_row(s, k):
    """(r, d): the first row of a square set whose k-th nearest (a self join) lies at a distance d > 0."""
    DS = scaled(s.D, s.S) + np.diag(np.full(len(s.cols), 1 << 20))
    kth = np.sort(DS, axis=1)[:, k - 1]
    r = int(np.nonzero(kth > 0)[0][0])
    return r, float(kth[r]) / s.S


def _build_calls():
    out = []
    add = lambda *a, **kw: out.append(Call(*a, **kw))
    for kind in ("short", "long"):
        for name in je.LIMITS:
            S = je.LIMITS[name][0]
            # 1. ladders: one query
            for k in (range(1, 65) if name == "s256" else FAR_K):
                add("ladders", name, ("far", kind, name), k, queries=[0])
            for k in (1, 64):
                add("ladders", name, ("near", kind, name), k, queries=[0])
            # 2. the limit tables on their extreme sets
            s = ("limit", kind, name)
            for k in (1, 8):
                add("limits", name, s, k, note="inf")
                add("limits", name, s, k, short_cap(envelope_set(s).D, k, S), note="median")
                for T in CLAMP_CAPS:
                    add("limits", name, s, k, float(T[:5]) / S if isinstance(T, str) else T, note="clamp")
                if kind == "long":  # (the long extreme set is one wave of 54 columns)
                    add("limits", name, ("limit wide", kind, name), k, note="wide")
        # 3. the bit-parallel tables: as planned, then the DP forced
        for name in ("costs ACGUN", "unit block"):
            for k in (1, 8):
                for opt in ((), FORCED_DP):
                    add("bitpar", name, ("bitpar", kind, name), k, options=opt)
        s = ("one way", kind)
        last = len(envelope_set(s).queries) - 1
        for k in (1, 8):
            for opt in ((), FORCED_DP):
                add("bitpar", "one way", s, k, queries=list(range(last)), options=opt)
            add("bitpar", "one way", s, k, queries=[last], note="fifth")
        # 4. geometry: row ranges and row groups under forced launch rows; the overflow rerun across launches
        for step in LAUNCH_ROWS:
            opt = ((sedgpu.SED_OPT_JOIN_ROWS, step),)
            for rows in ((5, 23), (1, 2)):
                for T in (INF, 9.0):
                    add("geometry", "self", ("geometry", kind), 3, T, rows=rows, options=opt)
            for k, T in ((1, INF), (4, INF), (4, 12.0), (64, INF)):
                add("geometry", "search", ("geometry", kind), k, T, queries=list(range(11)), options=opt)
        opt = ((sedgpu.SED_OPT_JOIN_ROWS, 4),)
        add("overflow", None, ("ties", kind), 1, rows=(0, 4), options=opt, note="small")
        add("overflow", None, ("ties", kind), 1, options=opt, note="grows")
        # 5. column counts around the wave and block edges
        for N in jl.COLUMN_COUNTS:
            for k in (1, 2, 64):
                add("columns", N, ("columns", kind), k, ncols=N)
                add("columns", N, ("columns", kind), k, ncols=N, queries=[3 % N, 0, N - 1])
        # 6. k against the lanes in scope; a cut of 0 with hits
        for N in (130, 66):  # waves of 64, 64, 2: two full waves; of 64, 2: one
            for k in (63, 64):
                add("scope", "identical", ("identical", kind), k, ncols=N)
            add("scope", "identical", ("identical", kind), 64, ncols=N, queries=[0, 1])
        add("scope", "identical", ("identical", kind), 8, 0.0, note="zero")
        add("scope", "ties", ("ties", kind), 8, 0.0, note="zero")
        # 7. the nearest column at the half-wave, wave and block edges
        for k in (1, 2):
            for opt in ((), FORCED_DP):
                add("lanes", None, ("lanes", kind), k, queries=list(je.LANE_QUERIES), options=opt)
        # 8. cutoffs on and beside a row's k-th distance
        for s in (("limit", kind, "i254_d1"), ("bitpar", kind, "unit block")):
            r, d = _kth_row(envelope_set(s), 8)
            for T, note in ((d, "at d"), (float(np.nextafter(d, 0)), "below d"), (5e-324, "tiny"), (0.0, "zero")):
                add("cutoffs", s[2], s, 8, T, rows=(r, r + 1), note=note)
    return out


_CALLS = []


def envelope_calls(group=None, kind=None, case=None):
    """Every call of the GPU envelope tests, in the order they are made (those of one group, index kind and case)."""
    if not _CALLS:
        _CALLS.extend(_build_calls())
    return [c for c in _CALLS if (group is None or c.group == group) and (kind is None or c.kind == kind) and
            (case is None or c.case == case)]


def call_inputs(call, set_of=envelope_set):
    """(the set, the index's columns, the call's rows, D of rows against columns, self join?, the first row); set_of: the
    sets the call's name is looked up in (join_knn_f64_envelope.py has its own)."""
    s = set_of(call.set)
    cols = s.cols if call.ncols is None else s.cols[:call.ncols]
    if call.queries is None:
        lo, hi = call.rows or (0, len(cols))
        return s, cols, cols[lo:hi], s.D[lo:hi, :len(cols)], True, lo
    q = list(call.queries)
    return s, cols, [s.queries[i] for i in q], s.Dq[q][:, :len(cols)], False, 0


def call_plan(call):
    """What the planner decides for the call (sedgpu.join_knn_plan)."""
    s, cols, rows, _, self_join, _ = call_inputs(call)
    mask = jc.codes_mask(s.plan, cols)
    return sedgpu.join_knn_plan(jc.costs_of(s.plan), dict(call.options), [len(x) for x in rows], [len(x) for x in cols], self_join,
                                mask if self_join else jc.codes_mask(s.plan, rows), mask, call.k, call.T, call.kind == "long")


_MODELS = {}


def call_model(call, order="sequential"):
    """bound_pass_model of the call under `order`, computed once."""
    key = call.key() + (order,)
    if key not in _MODELS:
        s, cols, rows, D, self_join, lo = call_inputs(call)
        _MODELS[key] = bound_pass_model(scaled(D, s.S), in_scope(D.shape, self_join, lo), [len(x) for x in rows],
                                        [len(x) for x in cols], s.ins_S, s.del_S, call.k, cut_of(call.T, s.S), order)
    return _MODELS[key]


def call_emit(call):
    """emit_pass_model of the call on the bounds of call_model: (the candidates' mask, the pairs pass 2 runs)."""
    s, cols, rows, D, self_join, lo = call_inputs(call)
    return emit_pass_model(scaled(D, s.S), in_scope(D.shape, self_join, lo), [len(x) for x in rows], [len(x) for x in cols],
                           s.ins_S, s.del_S, call_model(call)[0])
