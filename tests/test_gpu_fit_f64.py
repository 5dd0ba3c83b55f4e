"""GPU: fit search's fp64 route (sed_fit_search_f64, sed_fit_index_search_f64, sed_fit_index_hits_f64)
against its references, exactly: dist as float64 with ==, start and end.  Best hits against oracle.fit, hits against
fit_f64_cases.rows_reference (pinned on the CPU, tests/test_fit_f64_host.py).  The shapes are the smallest that reach
each seam: every table of the case file under chunk 8, 72, automatic and one lane per text, P in 1, 2, 31, 32 and
mixed, texts of 0 .. 300 symbols with copies planted to end on lane seams."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import sedgpu
import fit_f64_cases as fc

pytestmark = pytest.mark.gpu

CHUNK = sedgpu.SED_OPT_FIT_CHUNK
CHUNKS = [8, 72, 0, 1 << 30]
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300]


class chunked:
    def __init__(self, gpu, plan, chunk):
        self.gpu, self.plan, self.chunk = gpu, plan, chunk

    def __enter__(self):
        self.gpu.set_costs(self.plan)
        self.gpu.set_option(CHUNK, self.chunk)

    def __exit__(self, *exc):
        self.gpu.set_option(CHUNK, 0)


def _pairs(plan, chunk, seed):
    """(pats, texts): P in 1, 2, 31, 32 and a mixed one, each against every length, random and with copies planted on the
    seams of the planner's lanes for that (P, n), on column n and on column 0's side (a copy at the text's start)."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for P in (1, 2, 31, 32, int(rng.integers(3, 31))):
        p = rng.integers(0, plan.K, size=P).astype(np.uint8)
        for n in LENGTHS:
            seams = fc.seam_columns(sedgpu.fit_f64_lanes(plan.costs(), {CHUNK: chunk} if chunk else {}, [P], [n]))
            for ends in ([], seams, [n], [P]):
                pats.append(p)
                texts.append(fc.plant(rng, plan.K, p, n, ends))
    return pats, texts


def _fit(gpu, pats, texts):
    d, s, e = gpu.fit_f64(sedgpu.PackedPairs(pats, texts))
    return list(zip(d.tolist(), s.tolist(), e.tolist()))


@pytest.fixture(scope="module")
def table_cases():
    """{(table, chunk): (plan, pats, texts, oracle hits)}, computed once."""
    out = {}
    for k, (name, plan) in enumerate(fc.all_tables()):
        for chunk in CHUNKS:
            pats, texts = _pairs(plan, chunk, 100 * k + CHUNKS.index(chunk))
            out[name, chunk] = (plan, pats, texts, fc.oracle_fit(plan, pats, texts))
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", [n for n, _ in fc.all_tables()])
def test_best_hits_equal_the_oracle(gpu, table_cases, name, chunk):
    plan, pats, texts, want = table_cases[name, chunk]
    with chunked(gpu, plan, chunk):
        got = _fit(gpu, pats, texts)
        ix = sedgpu.FitIndex.from_texts(gpu, texts[:24])
        d, s, e = ix.search_f64(sedgpu.PackedPairs(pats[::48], [texts[0]] * len(pats[::48])))
        ix.close()
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)
    qs = pats[::48]
    cross = fc.oracle_fit(plan, [q for q in qs for _ in texts[:24]], texts[:24] * len(qs))
    assert list(zip(d.ravel().tolist(), s.ravel().tolist(), e.ravel().tolist())) == cross


def test_ties_on_homopolymers(gpu):
    plan = fc.rounding_table()
    pats, texts = [], []
    for P in (1, 5, 32):
        for n in (0, 31, 64, 129, 300):
            for a, b in ((0, 0), (0, 1), (2, 2)):
                pats.append(np.full(P, a, np.uint8))
                texts.append(np.full(n, b, np.uint8))
    want = fc.oracle_fit(plan, pats, texts)
    assert len(set(want)) > 6
    hom = [np.full(n, 2, np.uint8) for n in (64, 129, 300)]
    for chunk in (8, 72, 0):
        with chunked(gpu, plan, chunk):
            assert _fit(gpu, pats, texts) == want, chunk
            # every column e >= P of a matching homopolymer is an exact hit, and of its equal-cost starts the largest wins
            ix = sedgpu.FitIndex.from_texts(gpu, hom)
            h = ix.hits_f64(sedgpu.PackedPairs([np.full(5, 2, np.uint8)], [hom[0]]), 0.0)
            ix.close()
            assert _hits_list(h) == [(0, d, e - 5, e, 0.0) for d, t in enumerate(hom) for e in range(5, len(t) + 1)]


@pytest.mark.parametrize("npairs", [1, 64, 65, 257])
def test_wave_geometry(gpu, npairs):
    """Ragged last blocks, and pairs whose lanes straddle blocks (chunk 8: a 100-symbol text has 13 lanes)."""
    plan = fc.golden15("costs.json")
    rng = np.random.default_rng(npairs)
    pats = [rng.integers(0, plan.K, size=int(rng.integers(1, 33))).astype(np.uint8) for _ in range(npairs)]
    texts = [fc.plant(rng, plan.K, p, int(rng.integers(60, 101)), [50]) for p in pats]
    want = fc.oracle_fit(plan, pats, texts)
    for chunk in (8, 0):
        with chunked(gpu, plan, chunk):
            assert _fit(gpu, pats, texts) == want


@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_cross_route_on_dyadic_tables(gpu, name, alphabet):
    """Where the integer kernels serve the table every fp64 sum is exact: the two routes agree bit for bit."""
    plan = fc.golden_dyadic(name, alphabet)
    rng = np.random.default_rng(len(alphabet))
    pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in (1, 7, 28, 32)]
    texts = [fc.plant(rng, plan.K, pats[k % 4], n, [n // 2]) for k, n in enumerate((0, 5, 64, 129, 300, 77))]
    for chunk in (8, 0):
        with chunked(gpu, plan, chunk):
            pk = sedgpu.PackedPairs([p for p in pats for _ in texts], texts * len(pats))
            for a, b in zip(gpu.fit(pk), gpu.fit_f64(pk)):
                assert np.array_equal(a, b)
            ix = sedgpu.FitIndex.from_texts(gpu, texts)
            q = sedgpu.PackedPairs(pats, [texts[0]] * len(pats))
            for a, b in zip(ix.search(q), ix.search_f64(q)):
                assert np.array_equal(a, b)
            for T in (0.0, 2.0, np.inf):
                a, b = ix.hits(q, T), ix.hits_f64(q, T)
                assert len(a) and a.tobytes() == b.tobytes()
            ix.close()


def _hits_list(h):
    return list(zip(h["query"].tolist(), h["text"].tolist(), h["start"].tolist(), h["end"].tolist(),
                    h["dist"].tolist()))


def _want_hits(plan, pats, texts, T):
    ref = fc.rows_reference(plan, [p for p in pats for _ in texts], texts * len(pats), T)
    return [(k // len(texts), k % len(texts), s, e, d) for k, s, e, d in ref]


def test_index_of_65_queries_and_130_texts(gpu):
    """Searches, hits searches and integer-route searches alternate on one index while the costs change."""
    c15, u15 = fc.golden15("costs.json"), fc.golden15("user_costs.json")
    rng = np.random.default_rng(65)
    pats = [rng.integers(0, 15, size=int(rng.integers(1, 33))).astype(np.uint8) for _ in range(65)]
    texts = [fc.plant(rng, 15, pats[d % 65], int(rng.integers(0, 90)), [40]) for d in range(130)]
    q = sedgpu.PackedPairs(pats, [texts[0]] * 65)
    flat_p, flat_t = [p for p in pats for _ in texts], texts * 65
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    for plan, chunk in ((c15, 8), (u15, 0), (c15, 72)):
        want = fc.oracle_fit(plan, flat_p, flat_t)
        with chunked(gpu, plan, chunk):
            d, s, e = ix.search_f64(q)
            assert list(zip(d.ravel().tolist(), s.ravel().tolist(), e.ravel().tolist())) == want
            with pytest.raises(sedgpu.SedError, match="15 symbols"):
                ix.search(q)  # the integer route keeps its refusal, and the index stays usable
            q3 = sedgpu.PackedPairs(pats[:3], [texts[0]] * 3)
            assert _hits_list(ix.hits_f64(q3, 1.0)) == _want_hits(plan, pats[:3], texts, 1.0)
    # an integer-route search on the same index: texts of codes 0..3 only are needed for that, so a second index
    ix.close()
    small = [t % 4 for t in texts[:10]]
    ix = sedgpu.FitIndex.from_texts(gpu, small)
    d4 = fc.golden_dyadic("user_costs.json", "AGCU")
    q4 = sedgpu.PackedPairs([p % 4 for p in pats[:5]], [small[0]] * 5)
    with chunked(gpu, d4, 8):
        a = ix.search(q4)
        b = ix.search_f64(q4)
        h = ix.hits_f64(q4, 2.0)
        a2 = ix.search(q4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, a2)) and len(h)
    ix.close()


def test_hits_thresholds_and_cap_protocol(gpu):
    plan = fc.rounding_table()
    rng = np.random.default_rng(8)
    pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in (4, 4, 4)]
    texts = [fc.plant(rng, plan.K, pats[0], n, [n // 2, n]) for n in (0, 3, 64, 129, 300)]
    q = sedgpu.PackedPairs(pats, [texts[0]] * 3)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    every = _want_hits(plan, pats, texts, np.inf)
    Pdel = 4 * plan.dele
    mid = sorted(h[4] for h in every)[len(every) // 4]
    for chunk in (8, 72, 0):
        with chunked(gpu, plan, chunk):
            for T in (0.0, mid, Pdel, np.inf):
                got = _hits_list(ix.hits_f64(q, T))
                assert got == [h for h in every if h[4] <= T], (chunk, T)
                keys = [(h[0], h[1], h[3]) for h in got]
                assert keys == sorted(set(keys))
            assert len(_hits_list(ix.hits_f64(q, Pdel))) == 3 * sum(len(t) + 1 for t in texts)  # every column: E <= P delete
    with chunked(gpu, plan, 8):
        found = len([h for h in every if h[4] <= mid])
        assert found > 3
        assert len(ix.hits_f64(q, mid, cap=found)) == found
        with pytest.raises(sedgpu.SedError, match="found %d hits, cap %d" % (found, found - 1)):
            ix.hits_f64(q, mid, cap=found - 1)
        assert ix.found == found
        n = sedgpu.C.c_int64(0)
        rc = gpu._lib.sed_fit_index_hits_f64(ix.ptr, q.codes_a, q.off_a, q.len_a, 3, float(mid), None, 0, sedgpu.C.byref(n))
        assert rc == sedgpu.SED_E_RANGE and n.value == found  # cap = 0 with NULL: a count query
        assert len(ix.hits_f64(q, mid)) == found  # the index is usable after the refusals
        with pytest.raises(sedgpu.SedError):
            ix.hits_f64(q, float("nan"))
    ix.close()


def test_hits_full_wave_and_single_hit_wave(gpu):
    """A wave whose 64 lanes all hit in the same column step, and a wave where one lane hits."""
    plan = fc.unit(9)
    p = np.arange(8, dtype=np.uint8)
    far = np.full(40, 8, np.uint8)
    texts = [np.concatenate([far[:20], p, far[:12]]) for _ in range(64)] + [far] * 63 + [np.concatenate([far[:5], p, far[:27]])]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    q = sedgpu.PackedPairs([p], [texts[0]])
    with chunked(gpu, plan, 1 << 30):
        got = _hits_list(ix.hits_f64(q, 0.0))
    ix.close()
    assert got == [(0, d, 20, 28, 0.0) for d in range(64)] + [(0, 127, 5, 13, 0.0)]


def test_long_text_in_one_lane(gpu):
    plan = fc.unit(4, 0.0, 1.0)  # insert = 0: one lane, and the integer route refuses the span
    rng = np.random.default_rng(70000)
    p = rng.integers(0, 4, size=8).astype(np.uint8)
    t = np.full(70000, 0, np.uint8)
    t[::2] = 1  # 0 1 0 1 ...: no copy of p before the planted one unless p is in {0, 1}*
    p[3] = 2
    t[69000:69008] = p
    want = fc.oracle_fit(plan, [p], [t])
    assert want[0][0] == 0.0 and want[0][2] > 65536
    gpu.set_costs(plan)
    with pytest.raises(sedgpu.SedError, match="span more than 65535"):
        gpu.fit(sedgpu.PackedPairs([p], [t]))
    assert _fit(gpu, [p], [t]) == want


def test_refusals_leave_context_and_index_usable(gpu):
    good = fc.unit(9)
    rng = np.random.default_rng(9)
    p = rng.integers(0, 9, size=6).astype(np.uint8)
    texts = [fc.plant(rng, 9, p, 50, [30]) for _ in range(3)]
    want = fc.oracle_fit(good, [p] * 3, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    neg = fc.unit(9)
    neg.sub[2, 3] = -1.0
    for plan, pat, words in ((fc.unit(17), p, "17 symbols (at most 16)"), (good, np.zeros(33, np.uint8), "pattern length 33"),
                             (neg, p, "cost(2 -> 3) = -1")):
        gpu.set_costs(plan)
        for call in (lambda: gpu.fit_f64(sedgpu.PackedPairs([pat] * 3, texts)),
                     lambda: ix.search_f64(sedgpu.PackedPairs([pat], [texts[0]])),
                     lambda: ix.hits_f64(sedgpu.PackedPairs([pat], [texts[0]]), 1.0)):
            with pytest.raises(sedgpu.SedError, match=words.replace("(", r"\(").replace(")", r"\)")):
                call()
        gpu.set_costs(good)
        assert _fit(gpu, [p] * 3, texts) == want
        d, s, e = ix.search_f64(sedgpu.PackedPairs([p], [texts[0]]))
        assert list(zip(d[0].tolist(), s[0].tolist(), e[0].tolist())) == want
        assert gpu.fit_last_ms() > 0 and ix.last_ms() > 0
    ix.close()


def test_wfsearch_auto_route_with_scripts(gpu, monkeypatch):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    query = "ACGUACGGAUCA"
    docs = ["GGNACGUACGGAUCAGG", "ACGRACGGDUCA", "UUACGUACGGAUCADDD", "NNNN", "RYKMSWBVHN" + query[2:9]]
    got = wfsearch.fit_search(query, docs, route="auto", scripts=True)
    assert [g[0] for g in got] == docs and wfsearch.fit_route([query], docs) == "f64"
    plan = SED.batch_plan([query] * len(docs), docs)
    want = fc.oracle_fit(fc.Plan(plan.sub, plan.ins, plan.dele), [plan.encode(query)] * len(docs), [plan.encode(d) for d in docs])
    for (s, score, a, b, es), (d, ws, we) in zip(got, want):
        assert (a, b) == (ws, we) and score == 1 / (1 + d)
        assert SED.patching(es, query)[1] == s[a:b]
    assert got[0][1] == 1.0 and got[0][2:4] == (3, 15)
    with pytest.raises(sedgpu.SedError, match="symbols"):
        wfsearch.fit_search(query, docs)  # the default route still refuses
    ix = wfsearch.FitIndex(docs, route="auto")
    assert ix.search(query) == [g[:4] for g in got]
    assert [o[:4] for o in ix.occurrences(query, 0.0)] == [g[:4] for g in got if g[1] == 1.0]
    ix.close()
