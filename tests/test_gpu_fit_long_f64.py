"""GPU: the fp64 route for long patterns (sed_fit_index_search_long_f64, sed_fit_index_hits_long_f64)
against its references, exactly: dist as float64 with ==, start and end.  Best hits against oracle.fit; hits against
the last-row reference of fit_long_f64_cases (P <= 130) and, at any P, against the integer long calls on the tables
those serve; P <= 32 against the short fp64 calls.  The shapes are the smallest that reach each seam: every R at
P = 64 R, 64 R - 1 and 64 R / 2 + 1, P = 33 behind 2015 front rows, texts shorter than the skew, chunks of 8 and W + 4."""
import importlib
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import sedgpu
import fit_f64_cases as fc
import fit_long_f64_cases as lc

pytestmark = pytest.mark.gpu

CHUNK, ROWS = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300]
TABLES = [("rounding", fc.rounding_table()), ("costs15", fc.golden15("costs.json"))] + fc.zero_tables()


class opts:
    """The context under a cost model, a chunk option and a forced R, both options reset on the way out."""

    def __init__(self, gpu, plan, chunk=0, rows=0):
        self.gpu, self.plan, self.chunk, self.rows = gpu, plan, chunk, rows

    def __enter__(self):
        self.gpu.set_costs(self.plan)
        self.gpu.set_option(CHUNK, self.chunk)
        self.gpu.set_option(ROWS, self.rows)

    def __exit__(self, *exc):
        self.gpu.set_option(CHUNK, 0)
        self.gpu.set_option(ROWS, 0)


def _queries(pats):
    return sedgpu.PackedPairs(pats, [np.zeros(0, np.uint8)] * len(pats))


def _triples(res):
    d, s, e = res
    return list(zip(d.ravel().tolist(), s.ravel().tolist(), e.ravel().tolist()))


def _hits_list(h):
    return list(zip(h["query"].tolist(), h["text"].tolist(), h["start"].tolist(), h["end"].tolist(), h["dist"].tolist()))


def _window(plan, pats, len_t, rows=0):
    return sedgpu.fit_index_long_f64_plan(plan.costs(), {ROWS: rows} if rows else {}, [len(p) for p in pats], len_t)["W"]


def _texts(rng, plan, pats):
    """Every length, random, with a copy of some pattern planted mid-text and at the end where it fits."""
    out = []
    for k, n in enumerate(LENGTHS):
        p = pats[k % len(pats)]
        out.append(fc.plant(rng, plan.K, p, n, [n // 2 + len(p) // 2, n]))
    return out


@pytest.mark.parametrize("R", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("name", [n for n, _ in TABLES])
def test_best_hits_equal_the_oracle(gpu, name, R):
    plan = dict(TABLES)[name]
    rng = np.random.default_rng(R + len(name))
    pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in (64 * R, 64 * R - 1, 64 * R // 2 + 1)]
    texts = _texts(rng, plan, pats)
    want = fc.oracle_fit(plan, *lc.cross(pats, texts))
    assert sedgpu.fit_index_long_f64_plan(plan.costs(), {}, [len(p) for p in pats], LENGTHS)["rows"].tolist() == [R] * 3
    W = _window(plan, pats, LENGTHS)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    for chunk in (8, W + 4 if W > 0 else 12, 0, 1 << 30):
        with opts(gpu, plan, chunk):
            got = _triples(ix.search_long_f64(_queries(pats)))
        assert got == want, (chunk, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w))
    assert ix.last_ms() > 0
    ix.close()


@pytest.mark.parametrize("name", ["rounding", "costs15"])
def test_33_symbols_behind_2015_front_rows(gpu, name):
    plan = dict(TABLES)[name]
    rng = np.random.default_rng(33)
    pats = [rng.integers(0, plan.K, size=33).astype(np.uint8)]
    texts = _texts(rng, plan, pats) + [rng.integers(0, plan.K, size=n).astype(np.uint8) for n in (17, 40, 62)]
    want = fc.oracle_fit(plan, *lc.cross(pats, texts))
    W = _window(plan, pats, [len(t) for t in texts], 32)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    for R in (32, 16, 2):
        for chunk in (8, W + 4, 0):
            with opts(gpu, plan, chunk, R):
                assert _triples(ix.search_long_f64(_queries(pats))) == want, (R, chunk)
    ix.close()


def test_short_patterns_equal_the_short_fp64_calls(gpu):
    plan = fc.golden15("costs.json")
    rng = np.random.default_rng(32)
    pats = [rng.integers(0, 15, size=P).astype(np.uint8) for P in (1, 2, 31, 32)]
    texts = _texts(rng, plan, pats)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    q = _queries(pats)
    for chunk in (8, 104, 0):
        with opts(gpu, plan, chunk):
            for a, b in zip(ix.search_f64(q), ix.search_long_f64(q)):
                assert np.array_equal(a, b)
            for T in (0.0, 1.0, np.inf):
                a, b = ix.hits_f64(q, T), ix.hits_long_f64(q, T)
                assert len(a) and a.tobytes() == b.tobytes()
    ix.close()


@pytest.mark.parametrize("name,alphabet", [("user_costs.json", "ACGU"), ("costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_cross_route_at_any_P(gpu, name, alphabet):
    """Where the integer long calls serve the table every fp64 sum is exact: the two routes agree record for record.
    This is the hits check for large P."""
    plan = fc.golden_dyadic(name, alphabet)
    rng = np.random.default_rng(len(alphabet) + len(name))
    lens = [0, 5, 300, 1100, 2300]
    Ps = [P for P in (76, 256, 1024, 2048) if sedgpu.fit_long_route(plan.costs(), {}, [P], lens)[0] == "int"]
    assert Ps[:2] == [76, 256] and (name != "user_costs.json" or len(Ps) == 4)
    pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in Ps]
    texts = [fc.plant(rng, plan.K, fc_mut(rng, pats[k % len(pats)], plan.K), n, [n]) for k, n in enumerate(lens)]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    q = _queries(pats)
    for chunk in (0, 400):
        with opts(gpu, plan, chunk):
            a, b = ix.search_long(q), ix.search_long_f64(q)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            mid = float(np.median(a[0]))
            for T in (0.0, mid, np.inf):
                x, y = ix.hits_long(q, T), ix.hits_long_f64(q, T)
                assert x.tobytes() == y.tobytes() and (T == 0.0 or len(x))
            assert len(y) == len(pats) * sum(n + 1 for n in lens)
    ix.close()


def fc_mut(rng, p, K):
    """p with three substitutions"""
    m = p.copy()
    m[rng.integers(0, len(p), size=3)] = rng.integers(0, K, size=3)
    return m


@pytest.fixture(scope="module")
def row_cases():
    """{(table, P): (plan, pattern, texts, sorted hits of every column)}: the last-row reference, computed once."""
    out = {}
    for name in ("rounding", "costs15"):
        plan = dict(TABLES)[name]
        for P in (33, 130):
            rng = np.random.default_rng(P)
            p = rng.integers(0, plan.K, size=P).astype(np.uint8)
            n = 190
            seams = fc.seam_columns(sedgpu.fit_index_long_f64_lanes(plan.costs(), {CHUNK: 8}, [P], [n]))
            fit = [e for e in seams if e >= P]
            texts = [fc.plant(rng, plan.K, p, n, [e]) for e in fit[::5]] + [fc.plant(rng, plan.K, p, n, fit), np.zeros(0, np.uint8),
                                                                              rng.integers(0, plan.K, size=61).astype(np.uint8)]
            ref = lc.hits_reference(plan, [p] * len(texts), texts, np.inf)
            out[name, P] = (plan, p, texts, [(0, k, s, e, d) for k, s, e, d in ref])
    return out


@pytest.mark.parametrize("R", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("name", ["rounding", "costs15"])
def test_hits_equal_the_last_row(gpu, row_cases, name, R):
    for P in (33, 130):
        if P > 64 * R:
            continue
        plan, p, texts, every = row_cases[name, P]
        assert len(every) == sum(len(t) + 1 for t in texts)  # T = +inf: n + 1 hits per pair
        W = _window(plan, [p], [len(t) for t in texts], R)
        mid = sorted(h[4] for h in every)[len(every) // 5]
        ix = sedgpu.FitIndex.from_texts(gpu, texts)
        for chunk in (8, W + 4, 0):
            with opts(gpu, plan, chunk, R):
                for T in (np.inf, mid, 0.0):
                    got = _hits_list(ix.hits_long_f64(_queries([p]), T))
                    assert got == [h for h in every if h[4] <= T], (P, chunk, T)
                best = _triples(ix.search_long_f64(_queries([p])))
            for d in range(len(texts)):  # the hit of smallest (dist, end) is the search's
                h = min((h for h in every if h[1] == d), key=lambda h: (h[4], h[3]))
                assert best[d] == (h[4], h[2], h[3])
        ix.close()


def test_cap_protocol_and_hit_density(gpu):
    plan = fc.unit(9)
    rng = np.random.default_rng(8)
    p = rng.integers(0, 8, size=40).astype(np.uint8)
    far = np.full(200, 8, np.uint8)
    one = far.copy()
    one[100:140] = p
    texts = [one, far, far[:50]]
    q = _queries([p])
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    with opts(gpu, plan, 8):
        # one hit in total; then the sink within the cutoff at every owned column of every wave
        assert _hits_list(ix.hits_long_f64(q, 0.0)) == [(0, 0, 100, 140, 0.0)]
        every = ix.hits_long_f64(q, 40.0)
        assert len(every) == sum(len(t) + 1 for t in texts) and every["dist"].max() == 40.0
        found = len(ix.hits_long_f64(q, 39.0))
        assert 3 < found < len(every)
        assert len(ix.hits_long_f64(q, 39.0, cap=found)) == found
        with pytest.raises(sedgpu.SedError, match="found %d hits, cap %d" % (found, found - 1)):
            ix.hits_long_f64(q, 39.0, cap=found - 1)
        assert ix.found == found
        n = sedgpu.C.c_int64(0)
        rc = gpu._lib.sed_fit_index_hits_long_f64(ix.ptr, q.codes_a, q.off_a, q.len_a, 1, 39.0, None, 0, sedgpu.C.byref(n))
        assert rc == sedgpu.SED_E_RANGE and n.value == found  # cap = 0 with NULL: a count query
        assert len(ix.hits_long_f64(q, 39.0)) == found and ix.hits_last_ms() > 0  # usable after the refusals
        with pytest.raises(sedgpu.SedError):
            ix.hits_long_f64(q, float("nan"))
    ix.close()


def test_ties_on_homopolymers(gpu):
    plan = fc.unit(4)
    pats = [np.full(P, a, np.uint8) for P in (33, 64, 129) for a in (0, 2)]
    texts = [np.full(n, b, np.uint8) for n in (0, 31, 64, 129, 300) for b in (0, 2)]
    want = fc.oracle_fit(plan, *lc.cross(pats, texts))
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    for chunk in (8, 0):
        with opts(gpu, plan, chunk):
            assert _triples(ix.search_long_f64(_queries(pats))) == want
            # every column e >= P of a matching homopolymer is an exact hit; of its equal-cost starts the largest wins
            got = _hits_list(ix.hits_long_f64(_queries(pats[:1]), 0.0))
            assert got == [(0, d, e - 33, e, 0.0) for d, t in enumerate(texts) if len(t) and t[0] == 0
                           for e in range(33, len(t) + 1)]
    ix.close()


def test_one_wave_per_text(gpu):
    plan = fc.unit(4, 0.0, 1.0)  # insert = 0: no window, and the integer long calls refuse the span
    rng = np.random.default_rng(70000)
    p = rng.integers(0, 2, size=40).astype(np.uint8)
    p[17] = 2
    t = np.zeros(70000, np.uint8)
    t[::2] = 1
    t[69000:69040] = p
    want = fc.oracle_fit(plan, [p, p], [t, t[:50]])
    assert want[0][0] == 0.0 and want[0][2] > 65536
    ix = sedgpu.FitIndex.from_texts(gpu, [t, t[:50]])
    with opts(gpu, plan, 8):
        with pytest.raises(sedgpu.SedError, match="span more than 65535"):
            ix.search_long(_queries([p]))
        assert _triples(ix.search_long_f64(_queries([p]))) == want
        assert _hits_list(ix.hits_long_f64(_queries([p]), 0.0))[0] == (0, 0, 69000, 69040, 0.0)  # (insert = 0: every later column too)
    ix.close()


def test_query_mix_and_reuse(gpu):
    """65 queries of mixed R groups against 130 texts, results at q D + d whatever the grouping; two indexes; searches of
    every kind and a batch run alternate; the chunk-table cache; the costs change under one index."""
    c15, u15 = fc.golden15("costs.json"), fc.golden15("user_costs.json")
    rng = np.random.default_rng(65)
    lens = [int(rng.integers(1, 33)) for _ in range(20)] + [int(rng.integers(33, 129)) for _ in range(25)] + \
        [int(rng.integers(129, 257)) for _ in range(12)] + [300, 500, 513, 700, 1025, 40, 2, 128]
    order = rng.permutation(65)
    pats = [rng.integers(0, 15, size=lens[k]).astype(np.uint8) for k in order]
    texts = [fc.plant(rng, 15, pats[d % 65][:60], int(rng.integers(0, 90)), [70]) for d in range(130)]
    rows = sedgpu.fit_index_long_f64_plan(c15.costs(), {}, [len(p) for p in pats], [len(t) for t in texts])["rows"]
    assert sorted(set(rows.tolist())) == [2, 4, 8, 16, 32]
    q = _queries(pats)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    small = [t % 4 for t in texts[:10]]
    ix4 = sedgpu.FitIndex.from_texts(gpu, small)
    d4 = fc.golden_dyadic("user_costs.json", "AGCU")
    q4 = _queries([p % 4 for p in pats[:6]])
    short = [k for k, p in enumerate(pats) if len(p) <= 32][:5]
    qs = _queries([pats[k] for k in short])
    pk = sedgpu.PackedPairs([p % 4 for p in pats[:4]], small[:4])
    for plan, chunk in ((c15, 8), (u15, 72), (c15, 8)):
        want = fc.oracle_fit(plan, *lc.cross(pats, texts))
        with opts(gpu, plan, chunk):
            assert _triples(ix.search_long_f64(q)) == want
            with pytest.raises(sedgpu.SedError, match="15 symbols"):
                ix.search_long(q)  # the integer long route keeps its refusal, and the index stays usable
            a = ix.search_f64(qs)
            b = ix.search_long_f64(qs)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert _triples(b) == [want[k * 130 + d] for k in short for d in range(130)]
        with opts(gpu, d4, chunk):
            r = [ix4.search_long(q4), ix4.search_long_f64(q4), ix4.search_long(q4)]
            assert all(np.array_equal(x, y) for x, y in zip(r[0], r[1])) and all(np.array_equal(x, y) for x, y in zip(r[0], r[2]))
            qq = _queries([p % 4 for p in pats[:6] if len(p) <= 32] or [pats[0][:5] % 4])
            assert all(np.array_equal(x, y) for x, y in zip(ix4.search(qq), ix4.search_long_f64(qq)))
            dist = gpu.run(pk, False)[0]
            assert len(dist) == 4 and np.isfinite(dist).all()
            assert all(np.array_equal(x, y) for x, y in zip(r[1], ix4.search_long_f64(q4)))
    ix.close()
    ix4.close()


def test_refusals_leave_context_and_index_usable(gpu):
    good = fc.unit(9)
    rng = np.random.default_rng(9)
    p = rng.integers(0, 9, size=50).astype(np.uint8)
    texts = [fc.plant(rng, 9, p, 120, [90]) for _ in range(3)]
    want = fc.oracle_fit(good, [p] * 3, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    neg = fc.unit(9)
    neg.sub[2, 3] = -1.0
    for plan, pat, words in ((fc.unit(17), p, "17 symbols (at most 16)"), (good, np.zeros(2049, np.uint8), "pattern length 2049"),
                             (neg, p, "cost(2 -> 3) = -1")):
        gpu.set_costs(plan)
        for call in (lambda: ix.search_long_f64(_queries([pat])), lambda: ix.hits_long_f64(_queries([pat]), 1.0)):
            with pytest.raises(sedgpu.SedError, match=words.replace("(", r"\(").replace(")", r"\)")):
                call()
        gpu.set_costs(good)
        assert _triples(ix.search_long_f64(_queries([p]))) == want
        assert ix.last_ms() > 0
    ix.close()


def test_wfsearch_auto_route_long_query_with_scripts(gpu, monkeypatch):
    """A 76-nt query over IUPAC documents under costs.json: refused (SedError -4) before this route existed."""
    from test_fit_long_f64_host import LongF64Engine, _docs
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    rng = np.random.default_rng(76)
    query = "".join(rng.choice(list("ACGU"), size=76))
    docs = _docs(rng, query, fc.IUPAC, 6, 200)
    T = 1.5
    ix = wfsearch.FitIndex(docs, route="auto")
    got = ix.occurrences(query, T, scripts=True, long_patterns=True)
    ref = wfsearch.FitIndex(docs, route="auto", index_fn=lambda t, uc, f64=False: SED.fit_index(t, uc, engine=LongF64Engine, f64=f64))
    want = ref.occurrences(query, T, scripts=True, long_patterns=True)
    assert ref._ix._dev.log == [("hits_long_f64", [76])]
    assert got == want and len(got) >= 2 and (docs[1], 1.0, 0, 76) in [g[:4] for g in got]
    for s, score, a, b, es in got:
        assert SED.patching(es, query)[1] == s[a:b]
    assert ix.search(query, long_patterns=True) == ref.search(query, long_patterns=True)
    assert ix.search(query, long_patterns=True, route="f64") == ref.search(query, long_patterns=True)
    with pytest.raises(sedgpu.SedError):
        ix.occurrences(query, T, long_patterns=True, route="int")  # the default route still refuses
    ix.close()
    ref.close()
