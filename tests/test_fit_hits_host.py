"""CPU: the host side of the hits search (sed_fit_index_hits): the definition of the hits restated in
pure Python (the last row of test_fit_host.fit_definition's DP, kept whole) and pinned against brute force over every
substring with the C oracle as G; the same row computed for many texts at once in integers (what the GPU tests compare
the device with), pinned against the restatement; the occurrence filter on hand-made sequences; the cutoff rule through
sed_fit_cutoff_scaled; and wfsearch's occurrences over an index_fn engine that serves the restated definition."""
import math

import numpy as np
import pytest

from conftest import load_golden
import oracle
import sedgpu
from test_fit_host import E_RANGE, _brute_cases, costs_of, fit_definition, unit_costs, wfsearch  # noqa: F401  (a fixture)

E_ARG = -1


def hits_row(sub, ins, dele, p, t):
    """[(E(e), S(e)) for e = 0..n]: fit_definition's DP (rows = the pattern, D[0][j] = 0, D[i][0] = i delete, every
    cell the lexicographic minimum of (D, -start) over insert, delete and update), its last row kept whole."""
    n = len(t)
    row = [(0.0, -j) for j in range(n + 1)]
    for i, a in enumerate(p, 1):
        cost = sub[a]
        cur = [(i * dele, 0)]
        for j in range(1, n + 1):
            up, dg, left = row[j], row[j - 1], cur[j - 1]
            cur.append(min((left[0] + ins, left[1]), (up[0] + dele, up[1]), (dg[0] + cost[t[j - 1]], dg[1])))
        row = cur
    return [(d, -s) for d, s in row]


def hits_of(row, T):
    """The hits within T of one (pattern, text) from its row: [(start, end, dist)] by end."""
    return [(s, e, d) for e, (d, s) in enumerate(row) if d <= T]


def _brute_row(costs, p, t):
    """(E(e), S(e)) for every e by brute force: G(s, e) of every substring from the C oracle."""
    n = len(t)
    spans = [(s, e) for e in range(n + 1) for s in range(e + 1)]
    packed = sedgpu.PackedPairs([p] * len(spans), [t[s:e] for s, e in spans])
    d = oracle.batch(costs, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b, packed.off_b, packed.len_b,
                     packed.npairs)[0]
    row = []
    for e in range(n + 1):
        col = [(float(v), s) for (s, e2), v in zip(spans, d) if e2 == e]
        best = min(v for v, _ in col)
        row.append((best, max(s for v, s in col if v == best)))
    return row


def scale_of(sub, ins, dele):
    """The smallest S = 2^k on which every cost is an integer (the tests' tables are dyadic)."""
    vals = np.concatenate([np.asarray(sub, np.float64).ravel(), [ins, dele]])
    for k in range(0, 12):
        if np.all(vals * 2.0 ** k == np.floor(vals * 2.0 ** k)):
            return 2 ** k
    raise AssertionError("the cost table is not dyadic")


def hits_rows(sub, ins, dele, p, texts):
    """hits_row for one pattern and many texts at once: [(E float64[n + 1], S int64[n + 1])] per text.  The same DP in
    integers on the scale S, keys D * BIG + (nmax - start) whose plain minimum is the minimum of (D, -start), all
    texts side by side in one padded matrix (a column depends only on columns to its left, so the padding never
    reaches a text's own columns), the insert chain of a row as a running minimum:
    cur[j] = min over k <= j of (x[k] + (j - k) insert), x = min(delete from above, update from the diagonal)."""
    S = scale_of(sub, ins, dele)
    isub = np.rint(np.asarray(sub, np.float64) * S).astype(np.int64)
    iins, idel = int(round(ins * S)), int(round(dele * S))
    nmax = max([len(t) for t in texts] + [0])
    BIG = 1 << 20
    assert nmax + 1 < BIG
    T = np.zeros((len(texts), nmax), np.int64)
    for d, t in enumerate(texts):
        T[d, :len(t)] = t
    j = np.arange(nmax + 1, dtype=np.int64)
    row = np.broadcast_to(nmax - j, (len(texts), nmax + 1)).copy()  # row 0: D = 0, start = the column
    for i, a in enumerate(p, 1):
        x = np.empty_like(row)
        x[:, 0] = i * idel * BIG + nmax
        x[:, 1:] = np.minimum(row[:, 1:] + idel * BIG, row[:, :-1] + isub[a][T] * BIG)
        row = np.minimum.accumulate(x - j * (iins * BIG), axis=1) + j * (iins * BIG)
    out = []
    for d, t in enumerate(texts):
        r = row[d, :len(t) + 1]
        out.append(((r // BIG).astype(np.float64) / S, nmax - r % BIG))
    return out


def test_row_against_brute_force():
    for it, sub, ins, dele, p, t in _brute_cases():
        K = len(sub)
        costs = oracle.Costs(sub, np.zeros((K, K), np.uint8), ins, 0, dele, 0)
        row = hits_row(sub.tolist(), ins, dele, p.tolist(), t.tolist())
        assert row == _brute_row(costs, p, t), (it, p, t)
        assert row[0] == (len(p) * dele, 0)  # column 0 is a column
        # fit search's hit is the row's first strict minimum
        d, s, e = fit_definition(sub.tolist(), ins, dele, p.tolist(), t.tolist())
        assert (d, s) == row[e] and all(row[j][0] > d for j in range(e)) and all(r[0] >= d for r in row)


def test_batched_rows_equal_the_restatement():
    cases = list(_brute_cases())
    rng = np.random.default_rng(5)
    for it in range(40):  # larger ones: P up to 32, texts up to 300, costs multiples of 1/4 and 1/256
        K = int(rng.integers(2, 9))
        q = 256.0 if it % 5 == 0 else 4.0
        sub = rng.integers(0, 40, size=(K, K)) / q
        sub[np.eye(K) > 0] = 0 if it % 3 else 1 / q
        ins, dele = float(rng.integers(0 if it % 4 == 0 else 1, 9)) / q, float(rng.integers(0, 9)) / q
        p = rng.integers(0, K, size=int(rng.integers(1, 33))).astype(np.uint8)
        t = rng.integers(0, K, size=int(rng.integers(0, 300))).astype(np.uint8)
        cases.append((1000 + it, sub, ins, dele, p, t))
    for it, sub, ins, dele, p, t in cases:
        others = [t[:len(t) // 2], np.zeros(0, np.uint8), np.concatenate([t, t])]
        got = hits_rows(sub, ins, dele, p, [t] + others)
        for text, (E, S) in zip([t] + others, got):
            want = hits_row(sub.tolist(), ins, dele, p.tolist(), text.tolist())
            assert list(zip(E.tolist(), S.tolist())) == want, (it, p, text)


# ---- the occurrence filter ----

def _occ(wfsearch, E, T):
    """The ends local_minima keeps of one text whose columns have best distances E, under cutoff T."""
    hits = [(0, 0, 0, e, d) for e, d in enumerate(E) if d <= T]
    kept = wfsearch.local_minima(hits)
    want = [e for e, d in enumerate(E) if d <= T and d < (E[e - 1] if e > 0 else math.inf)
            and d <= (E[e + 1] if e + 1 < len(E) else math.inf)]  # the rule on the whole sequence
    assert [h[3] for h in kept] == want
    return want


def test_occurrence_filter(wfsearch):
    assert _occ(wfsearch, [5, 3, 1, 1, 1, 4, 6], 2) == [2]                # a plateau: its earliest end
    assert _occ(wfsearch, [0, 2, 5, 5, 3, 1], 1) == [0, 5]                # valleys at column 0 and at column n
    assert _occ(wfsearch, [4, 1, 3, 1, 4], 2) == [1, 3]                   # two valleys, one non-hit between them
    assert _occ(wfsearch, [4, 1, 2, 1, 4], 2) == [1, 3]                   # ... and a hit between them
    assert _occ(wfsearch, [3, 3, 2, 1, 2, 3, 3, 1, 1, 3], 3) == [0, 3, 7]  # T >= P delete: every column is a hit
    assert _occ(wfsearch, [3, 3, 3], 3) == [0]
    assert _occ(wfsearch, [3, 2, 1], 0) == [] and _occ(wfsearch, [], 1) == []
    assert _occ(wfsearch, [2, 1, 1, 2, 1], 1) == [1, 4]                   # a hit whose left neighbour is no hit
    # hits of several (query, text) pairs in one list never look across a pair's border
    hits = [(0, 0, 0, 3, 1.0), (0, 1, 0, 4, 1.0), (1, 1, 0, 5, 1.0), (1, 1, 0, 6, 0.5)]
    assert wfsearch.local_minima(hits) == [hits[0], hits[1], hits[3]]


def test_best_hit_is_an_occurrence(wfsearch):
    for it, sub, ins, dele, p, t in _brute_cases():
        row = hits_row(sub.tolist(), ins, dele, p.tolist(), t.tolist())
        d, s, e = fit_definition(sub.tolist(), ins, dele, p.tolist(), t.tolist())
        for T in (d, d + 0.5, len(p) * dele, math.inf):
            hits = [(0, 0, a, b, v) for a, b, v in hits_of(row, T)]
            assert (0, 0, s, e, d) in wfsearch.local_minima(hits), (it, T)
        assert hits_of(row, d - 0.25) == []  # nothing is below the best
        assert len(hits_of(row, len(p) * dele)) == len(t) + 1  # E(e) <= P delete everywhere


# ---- the cutoff rule ----

def _cut(costs, T, len_p=(5,), len_t=(10,)):
    return sedgpu.fit_cutoff_scaled(costs, {}, list(len_p), list(len_t), T)


def _cut_code(costs, T, len_p=(5,), len_t=(10,)):
    with pytest.raises(sedgpu.SedError) as ex:
        _cut(costs, T, len_p, len_t)
    return ex.value.code


@pytest.mark.parametrize("S", [1, 2, 4, 256])
def test_cutoff_is_floor_of_t_times_s(S):
    costs = unit_costs(4, 1.0 / S, 1.0 / S, sub=1.0 / S)
    assert sedgpu.fit_plan(costs, {}, [5], [10])["scale"] == S
    for k in (0, 1, 2, 7, 300):
        lo, up = k / S, (k + 1) / S  # two representable distances next to each other
        assert _cut(costs, lo) == k and _cut(costs, up) == k + 1
        for T in (lo + 0.25 / S, (lo + up) / 2, np.nextafter(up, 0)):  # between them: the lower is in, the upper out
            cut = _cut(costs, T)
            assert cut == k == math.floor(T * S) and lo * S <= cut < up * S
    assert _cut(costs, 0.0) == 0 and _cut(costs, -0.0) == 0
    assert _cut(costs, math.inf) == 65535 and _cut(costs, 1e300) == 65535 and _cut(costs, 65535.0 / S) == 65535
    assert _cut(costs, 65534.0 / S) == 65534
    for bad in (math.nan, -1.0, -1e-300, -math.inf):
        assert _cut_code(costs, bad) == E_ARG


def test_cutoff_refusals_are_the_plans():
    t = load_golden("costs.json")
    refused = [(costs_of(t, "ARD"), [5], [10]), (unit_costs(9, 1, 1), [5], [10]), (unit_costs(4, 1, 1), [33], [10]),
               (unit_costs(4, 1, 1), [4, 33], [10, 10]), (unit_costs(4, 1, 3000), [32], [10]),
               (unit_costs(4, 1, 2100.25), [32], [10]), (unit_costs(4, 1, 1), [5], [-1]),
               (unit_costs(4, 0, 1), [5], [70000])]
    for costs, lp, lt in refused:
        with pytest.raises(sedgpu.SedError) as ex:
            sedgpu.fit_plan(costs, {}, lp, lt)
        for T in (1.0, math.inf, math.nan):  # (the plan's refusal comes first)
            assert _cut_code(costs, T, lp, lt) == ex.value.code
    assert {E_RANGE, E_ARG} == {_cut_code(c, 1.0, lp, lt) for c, lp, lt in refused}
    assert _cut(costs_of(t, "ARG"), 1.3, [5], [10]) == 2  # S = 2


def test_abi_symbols_are_exported_and_bound():
    lib = sedgpu.load()
    names = {n for n, _, _ in sedgpu.SIGNATURES}
    for sym in ("sed_fit_index_hits", "sed_fit_index_hits_last_time", "sed_fit_cutoff_scaled"):
        assert sym in names and getattr(lib, sym).argtypes is not None
    assert all(callable(getattr(sedgpu.FitIndex, a)) for a in ("hits", "hits_last_ms"))
    assert sedgpu.FIT_HIT_DTYPE.itemsize == 24 and [sedgpu.FIT_HIT_DTYPE.fields[f][1] for f in sedgpu.FIT_HIT_DTYPE.names] \
        == [0, 4, 8, 12, 16]
    # the forked child's proxy serves no index, hence no hits
    assert not hasattr(sedgpu.EngineClient, "hits")
    with pytest.raises(sedgpu.SedError, match="does not serve resident indexes"):
        sedgpu.EngineClient.fit_index(object.__new__(sedgpu.EngineClient), np.zeros(1, np.uint8), [0], [1])


# ---- wfsearch's occurrences with the restated definition standing in for the device ----

class DefinitionEngine:
    """StringEditDistance.FitIndex's device half on the CPU: search through oracle.fit, hits through hits_rows."""

    def __init__(self, codes, off, lens):
        self.texts = [np.asarray(codes[o:o + n], np.uint8) for o, n in zip(off, lens)]
        self.codes, self.off, self.lens = np.concatenate([codes, np.zeros(1, np.uint8)]), off, lens
        self.calls = 0

    def search(self, plan, packed):
        Q, D = packed.npairs, len(self.lens)
        qi, di = np.divmod(np.arange(Q * D), max(D, 1))
        d, s, e = oracle.fit(oracle.Costs.from_plan(plan), packed.codes_a, packed.off_a[qi].copy(), packed.len_a[qi].copy(),
                             self.codes, self.off[di].copy(), self.lens[di].copy(), Q * D, 1)
        return d.reshape(Q, D), s.reshape(Q, D), e.reshape(Q, D)

    def hits(self, plan, packed, max_dist):
        self.calls += 1
        out = []
        for q in range(packed.npairs):
            p = packed.codes_a[packed.off_a[q]:packed.off_a[q] + packed.len_a[q]]
            for d, (E, S) in enumerate(hits_rows(plan.sub, plan.ins, plan.dele, p, self.texts)):
                out += [(q, d, int(S[e]), e, float(E[e])) for e in np.nonzero(E <= max_dist)[0].tolist()]
        return np.array(out, sedgpu.FIT_HIT_DTYPE)

    def close(self):
        pass


@pytest.fixture()
def index_fn(wfsearch, monkeypatch):
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    return lambda texts, user_cost: SED.fit_index(texts, user_cost, engine=DefinitionEngine)


def _docs(rng, query, count=10, n=90):
    """Documents with 0..3 planted copies of the query (some mutated); the first is empty, the second the query."""
    docs = ["", query]
    for k in range(2, count):
        d = list(rng.choice(list("ACGU"), size=n))
        for c in range(k % 4):
            m = list(query)
            for _ in range(c):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, n - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    return docs


def _fake_scripts(monkeypatch, SED):
    """edit_script_batch without the device: the pairs it was asked for, as the script."""
    calls = []

    def fake(strs1, strs2, userCosts=False):
        calls.append(len(strs1))
        return [(0, ("es", a, b)) for a, b in zip(strs1, strs2)]
    monkeypatch.setattr(SED, "edit_script_batch", fake)
    return calls


@pytest.mark.parametrize("user_cost", [False, True])
def test_wfsearch_occurrences(wfsearch, index_fn, monkeypatch, user_cost):
    SED = wfsearch.SED
    rng = np.random.default_rng(31)
    query = "".join(rng.choice(list("ACGU"), size=20))
    docs = _docs(rng, query)
    ix = wfsearch.FitIndex(docs, user_cost, index_fn=index_fn)
    plan = SED.batch_plan([query], ["ACGU"], user_cost)

    def want(q, T, all_ends):
        out = []
        for doc in docs:
            row = hits_row(plan.sub.tolist(), plan.ins, plan.dele, plan.encode(q).tolist(), plan.encode(doc).tolist())
            ends = [e for e, (d, _) in enumerate(row) if d <= T]
            if not all_ends:
                ends = [e for e in ends if row[e][0] < (row[e - 1][0] if e else math.inf)
                        and row[e][0] <= (row[e + 1][0] if e < len(doc) else math.inf)]
            out += [(doc, 1 / (1 + row[e][0]), row[e][1], e) for e in ends]
        return out

    Pdel = len(query) * plan.dele
    for T in (0, 4, 9.5, Pdel, math.inf):
        for all_ends in (False, True):
            got = ix.occurrences(query, T, all_ends=all_ends)
            assert got == want(query, T, all_ends), (T, all_ends)
            assert got == wfsearch.fit_occurrences(query, docs, T, user_cost, all_ends=all_ends, index_fn=index_fn)
    exact = ix.occurrences(query, 0)
    assert (docs[1], 1.0, 0, len(query)) in exact and all(s[a:b] == query and sc == 1.0 for s, sc, a, b in exact)
    assert len(exact) > 1
    assert len(ix.occurrences(query, math.inf, all_ends=True)) == sum(len(d) + 1 for d in docs)
    assert ix.occurrences(query, Pdel, all_ends=True) == ix.occurrences(query, math.inf, all_ends=True)
    # collection order, then by end
    some = ix.occurrences(query, 9.5)
    keys = [(docs.index(s), b) for s, _, _, b in some]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) > len(docs) - 1
    # search()'s best hit is one of the occurrences wherever it is within T
    for (s, sc, a, b) in ix.search(query, max_dist=9.5):
        assert (s, sc, a, b) in some
    # many queries: one engine call, one list per query
    queries = [query, query[:1], query[3:], "ACGU" * 8]
    dev = ix._ix._dev
    calls = dev.calls
    many = ix.occurrences_many(queries, 6)
    assert dev.calls == calls + 1
    assert many == [want(q, 6, False) for q in queries] == [ix.occurrences(q, 6) for q in queries]
    # scripts: one edit_script_batch call for every returned tuple, of (query, sequence[start:end])
    batches = _fake_scripts(monkeypatch, SED)
    withes = ix.occurrences_many(queries, 6, scripts=True)
    assert batches == [sum(len(o) for o in many)]
    for q, o, w in zip(queries, many, withes):
        assert [h[:4] for h in w] == o and all(h[4] == ("es", q, h[0][h[2]:h[3]]) for h in w)
    assert ix.occurrences(query, 0, all_ends=True, scripts=True) == [h + (("es", query, query),) for h in exact]
    assert ix.occurrences("ACGU" * 8, 0, scripts=True) == [] and len(batches) == 2  # nothing kept: no script call
    # empty queries, empty collection
    assert ix.occurrences_many([], 3) == []
    empty = wfsearch.FitIndex([], user_cost, index_fn=index_fn)
    assert empty.occurrences(query, 3) == [] and empty.occurrences_many([query, query], 3, scripts=True) == [[], []]
    assert wfsearch.fit_occurrences(query, [], 3, user_cost, index_fn=index_fn) == []
    with pytest.raises(KeyError):
        ix.occurrences("AXG", 3)  # the reference's KeyError, as search raises it
    with pytest.raises(sedgpu.SedError, match="9 symbols"):
        ix.occurrences("RYKMS", 3)
    ix.close()
    ix.close()
