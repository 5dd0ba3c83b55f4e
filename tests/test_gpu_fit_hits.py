"""GPU: every occurrence within a distance over a resident index (sed_fit_index_hits).  In every case
the sorted hit list must equal the restated definition's (test_fit_hits_host.hits_rows, pinned there against brute
force) exactly: the same (query, text, start, end), dist bit for bit."""
import importlib
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import fit_envelope
import sedgpu
from test_fit_hits_host import DefinitionEngine, hits_rows
from test_gpu_fit import _golden_plan
from test_gpu_fit_index import _cross, _queries

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_RANGE = r"\(-1\)", r"\(-6\)", r"\(-4\)"


def _rows(plan, pats, texts):
    """The definition's whole rows, [query][text] -> (E, S): computed once per case, cut at each T by _want."""
    return [hits_rows(plan.sub, plan.ins, plan.dele, p, texts) for p in pats]


def _want(rows, T):
    out = []
    for q, per_text in enumerate(rows):
        for d, (E, S) in enumerate(per_text):
            ends = np.flatnonzero(E <= T)
            rec = np.zeros(len(ends), sedgpu.FIT_HIT_DTYPE)
            rec["query"], rec["text"], rec["start"], rec["end"], rec["dist"] = q, d, S[ends], ends, E[ends]
            out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, sedgpu.FIT_HIT_DTYPE)


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("query", "text", "start", "end"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (f, [(got[i], want[i]) for i in bad[:5]])
    bad = np.flatnonzero(got["dist"].view(np.uint64) != want["dist"].view(np.uint64))
    assert not len(bad), [(got[i], want[i]) for i in bad[:5]]


def _check(gpu, plan, ix, pats, rows, T, chunk=0):
    gpu.set_costs(plan)
    try:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, chunk)
        got = ix.hits(_queries(pats), T)
    finally:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)
    want = _want(rows, T)
    _same(got, want)
    assert ix.found == len(want) and ix.hits_last_ms() > 0
    return got


def _unit(K=4, sub=2.0):
    return np.where(np.eye(K) > 0, 0.0, sub)


def _plan(name, alphabet):
    g = _golden_plan(name, alphabet)
    return fit_envelope.Plan(g.sub, g.ins, g.dele)


# 1. golden tables and chunking

@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_golden_tables_and_chunking(gpu, name, alphabet):
    K = len(alphabet)
    plan = _plan(name, alphabet)
    rng = np.random.default_rng(400 + len(name) + K)
    pats = [rng.integers(0, K, size=P).astype(np.uint8) for P in (1, 17, 32)]
    lens = [0, 1, 2, 300] + rng.integers(0, 301, size=36).tolist()
    texts = [fit_envelope.planted_text(rng, K, pats[1 + d % 2], n) if n > 40 else rng.integers(0, K, size=n).astype(np.uint8)
             for d, n in enumerate(lens)]
    rows = _rows(plan, pats, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        with pytest.raises(sedgpu.SedError, match=E_STATE):
            ix.hits_last_ms()
        for chunk in (8, 72, 0, 1 << 20):  # forced, automatic, one lane per text
            few = _check(gpu, plan, ix, pats, rows, 0, chunk)
            mid = _check(gpu, plan, ix, pats, rows, 3 * plan.dele, chunk)
            every = _check(gpu, plan, ix, pats, rows, 32 * plan.dele, chunk)
            assert len(few) < len(mid) < len(every) == len(pats) * sum(n + 1 for n in lens)
            _same(_check(gpu, plan, ix, pats, rows, math.inf, chunk), every)
    finally:
        ix.close()


# 2. seams

def test_seams(gpu):
    """Chunk 40, P = 12, insert = delete = 1 (W = 24): exact copies end on a lane's first owned column (80), on its last
    (119), on column n (200), and column 0 of a first lane and of a zero-length text are hits through T >= P delete."""
    plan = fit_envelope.Plan(_unit(), 1, 1)
    rng = np.random.default_rng(40)
    p = rng.integers(0, 4, size=12).astype(np.uint8)
    texts = []
    for end in (80, 119, 200, 41, 79):
        t = rng.integers(0, 4, size=200).astype(np.uint8)
        t[end - 12:end] = p
        texts.append(t)
    texts += [np.zeros(0, np.uint8), p[:5].copy(), p.copy()]
    lanes, _ = sedgpu.fit_index_lanes(plan.costs(), {sedgpu.SED_OPT_FIT_CHUNK: 40}, [12], [len(t) for t in texts])
    own = sorted(zip(lanes["pair"].tolist(), lanes["c0"].tolist(), lanes["cnt"].tolist(), lanes["lead"].tolist()))
    assert own[:6] == [(0, 0, 40, 0), (0, 40, 40, 24), (0, 80, 40, 24), (0, 120, 40, 24), (0, 160, 40, 24), (0, 200, 1, 24)]
    assert (5, 0, 1, 0) in own and (7, 0, 13, 0) in own
    rows = _rows(plan, [p], texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        exact = _check(gpu, plan, ix, [p], rows, 0, chunk=40)
        ends = {(int(h["text"]), int(h["end"])) for h in exact}
        assert {(0, 80), (1, 119), (2, 200), (3, 41), (4, 79), (7, 12)} <= ends and all(h["start"] == h["end"] - 12 for h in exact)
        for chunk in (40, 0, 1 << 20):
            below = _check(gpu, plan, ix, [p], rows, 11.5, chunk)  # just under P delete: no column 0
            assert not np.any(below["end"] == 0)
            every = _check(gpu, plan, ix, [p], rows, 12, chunk)
            zero = every[every["end"] == 0]
            assert len(zero) == len(texts) and np.all(zero["start"] == 0) and np.all(zero["dist"] == 12.0)
            assert len(every) == sum(len(t) + 1 for t in texts)
    finally:
        ix.close()


# 3. rebase

def test_rebase(gpu):
    """One lane per text of 300 columns: the insert offset is rebased after columns 128 and 256, and exact copies end at
    columns 127, 128, 129 and 256."""
    plan = _plan("user_costs.json", "ACGU")
    rng = np.random.default_rng(128)
    p = rng.integers(0, 4, size=21).astype(np.uint8)
    texts = []
    for end in (127, 128, 129, 256, 257):
        t = rng.integers(0, 4, size=300).astype(np.uint8)
        t[end - 21:end] = p
        texts.append(t)
    got = sedgpu.fit_index_plan(plan.costs(), {sedgpu.SED_OPT_FIT_CHUNK: 1 << 20}, [21], [300] * 5)
    assert got["lanes"] == 5
    rows = _rows(plan, [p], texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        exact = _check(gpu, plan, ix, [p], rows, 0, chunk=1 << 20)
        assert {(0, 127), (1, 128), (2, 129), (3, 256), (4, 257)} <= {(int(h["text"]), int(h["end"])) for h in exact}
        _check(gpu, plan, ix, [p], rows, 4 * plan.dele, chunk=1 << 20)
        _check(gpu, plan, ix, [p], rows, 21 * plan.dele, chunk=1 << 20)
    finally:
        ix.close()


# 4. ballot paths

def test_ballot_paths(gpu):
    """150 texts of 64..90 symbols, one lane each: three blocks, the last ragged.  T large: all 64 lanes of a wave hit
    at every column step they share.  T = 0 with one planted copy of a random 32-mer: exactly one lane of one wave
    hits, once."""
    plan = fit_envelope.Plan(_unit(), 1, 1)
    rng = np.random.default_rng(64)
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    texts = [rng.integers(0, 4, size=int(rng.integers(64, 91))).astype(np.uint8) for _ in range(150)]
    texts[77][20:52] = p
    lens = [len(t) for t in texts]
    assert sedgpu.fit_index_plan(plan.costs(), {sedgpu.SED_OPT_FIT_CHUNK: 1 << 20}, [32], lens)["lanes"] == 150
    rows = _rows(plan, [p], texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        every = _check(gpu, plan, ix, [p], rows, 32, chunk=1 << 20)
        assert len(every) == sum(n + 1 for n in lens)
        one = _check(gpu, plan, ix, [p], rows, 0, chunk=1 << 20)
        assert one.tolist() == [(0, 77, 20, 52, 0.0)]
        # the same under chunk 8: many lanes a text, a ragged last block as well
        n8 = sedgpu.fit_index_plan(plan.costs(), {sedgpu.SED_OPT_FIT_CHUNK: 8}, [32], lens)["lanes"]
        assert n8 > 64 and n8 % 64
        _same(_check(gpu, plan, ix, [p], rows, 32, chunk=8), every)
        _same(_check(gpu, plan, ix, [p], rows, 0, chunk=8), one)
    finally:
        ix.close()


# 5. overflow

def test_overflow_and_interleaved_search(gpu):
    plan = _plan("user_costs.json", "ACGU")
    rng = np.random.default_rng(5)
    pats = [rng.integers(0, 4, size=P).astype(np.uint8) for P in (9, 28)]
    texts = [fit_envelope.planted_text(rng, 4, pats[d % 2], 120 + d) for d in range(20)]
    rows = _rows(plan, pats, texts)
    T = 3 * plan.dele
    want = _want(rows, T)
    found = len(want)
    assert found > 40
    gpu.set_costs(plan)
    q = _queries(pats)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        with pytest.raises(sedgpu.SedError, match=E_RANGE + ".*found %d hits, cap %d" % (found, found - 1)):
            ix.hits(q, T, cap=found - 1)
        assert ix.found == found
        got = ix.hits(q, T, cap=found)  # the index is usable, and exactly enough room is enough
        _same(got, want)
        with pytest.raises(sedgpu.SedError, match=E_RANGE + ".*found %d hits, cap 0" % found):
            ix.hits(q, T, cap=0)  # the count query: out = NULL
        assert ix.found == found
        _same(ix.hits(q, T, cap=found + 1000), want)
        # a plain search on the same index: still bit-equal to Context.fit
        d, s, e = ix.search(q)
        fd, fs, fe = gpu.fit(_cross(pats, texts))
        assert np.array_equal(d.ravel().view(np.uint64), fd.view(np.uint64))
        assert np.array_equal(s.ravel(), fs) and np.array_equal(e.ravel(), fe)
        # ... and its best hit is the hit of smallest (dist, end) of each pair that has one
        for qi in range(len(pats)):
            for di in range(len(texts)):
                mine = want[(want["query"] == qi) & (want["text"] == di)]
                if d[qi, di] <= T:
                    best = mine[np.lexsort((mine["end"], mine["dist"]))[0]]
                    assert (best["dist"], best["start"], best["end"]) == (d[qi, di], s[qi, di], e[qi, di])
                else:
                    assert len(mine) == 0
        _same(ix.hits(q, T), want)  # hits after a search, grow-and-retry from the room it has
        for bad in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=E_ARG + ".*max_dist"):
                ix.hits(q, bad)
        assert len(ix.hits(_queries([]), T)) == 0
    finally:
        ix.close()
    with pytest.raises(sedgpu.SedError, match="closed"):
        ix.hits(q, T)
    empty = sedgpu.FitIndex.from_texts(gpu, [])
    assert len(empty.hits(q, T)) == 0
    empty.close()


# 6. long text

def test_long_text(gpu):
    """One text of 70 000 symbols under the automatic rule (it is split): exact and 3-edit copies with ends past 2^16."""
    plan = fit_envelope.Plan(_unit(), 1, 4)
    rng = np.random.default_rng(70001)
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    pats = [p, rng.integers(0, 4, size=20).astype(np.uint8)]
    long = rng.integers(0, 4, size=70000).astype(np.uint8)
    m = fit_envelope.mutate(rng, p, 4, 3)
    for end in (300, 65535, 65536 + len(m), 69000):
        long[end - len(m):end] = m
    long[66000 - 32:66000] = p
    long[70000 - 20:] = pats[1]
    texts = [rng.integers(0, 4, size=50).astype(np.uint8), long, np.zeros(0, np.uint8)]
    chunk = sedgpu.fit_index_plan(plan.costs(), {}, [32, 20], [len(t) for t in texts])["chunk"]
    assert 0 < chunk < 70000
    rows = _rows(plan, pats, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        exact = _check(gpu, plan, ix, pats, rows, 0)
        assert [(0, 1, 66000 - 32, 66000, 0.0), (1, 1, 70000 - 20, 70000, 0.0)] == exact.tolist()
        near = _check(gpu, plan, ix, pats, rows, 15)
        assert np.sum(near["end"] > 1 << 16) >= 4 and {300, 65535, 69000, 70000} <= set(near["end"].tolist())
    finally:
        ix.close()


def test_zero_insert(gpu):
    """insert = 0: a text of 3000 symbols runs in one lane, whatever the chunk option says."""
    plan = fit_envelope.Plan(_unit(), 0, 1.5)
    rng = np.random.default_rng(3000)
    pats = [rng.integers(0, 4, size=P).astype(np.uint8) for P in (1, 31)]
    texts = [fit_envelope.planted_text(rng, 4, pats[1], 3000), rng.integers(0, 4, size=129).astype(np.uint8),
             np.zeros(0, np.uint8)]
    assert sedgpu.fit_index_plan(plan.costs(), {sedgpu.SED_OPT_FIT_CHUNK: 64}, [1, 31], [3000, 129, 0])["lanes"] == 6
    rows = _rows(plan, pats, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        for chunk in (0, 64):
            _check(gpu, plan, ix, pats, rows, 0, chunk)
            _check(gpu, plan, ix, pats, rows, 6, chunk)
            assert len(_check(gpu, plan, ix, pats, rows, 31 * 1.5, chunk)) == 2 * (3001 + 130 + 1)
    finally:
        ix.close()


# 7. many queries

def test_many_queries(gpu):
    """65 queries of differing P against 130 texts in one launch under chunk 8, every pair against the definition."""
    rng = np.random.default_rng(65131)
    plan = _plan("user_costs.json", "ACGU")
    pats = [rng.integers(0, 4, size=1 + (q * 7) % 32).astype(np.uint8) for q in range(65)]
    texts = [rng.integers(0, 4, size=int(rng.integers(0, 90))).astype(np.uint8) for _ in range(130)]
    for q in range(0, 65, 2):
        t = texts[2 * q]
        if len(t) >= len(pats[q]):
            t[len(t) - len(pats[q]):] = pats[q]
    rows = _rows(plan, pats, texts)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        got = _check(gpu, plan, ix, pats, rows, 2 * plan.dele, chunk=8)
        assert len(np.unique(got["query"])) > 30 and len(np.unique(got["text"])) > 100
        _check(gpu, plan, ix, pats, rows, 0, chunk=8)
    finally:
        ix.close()


# 8. the engine path

def test_wfsearch_occurrences_on_the_engine(gpu, monkeypatch):
    """wfsearch.FitIndex.occurrences on the engine equals the same call over the index_fn engine that serves the
    restated definition, scripts included, and patching(es, query) gives sequence[start:end]."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    rng = np.random.default_rng(41)
    query = "".join(rng.choice(list("ACGU"), size=28))
    docs = [""]
    for k in range(1, 30):
        d = list(rng.choice(list("ACGU"), size=int(rng.integers(60, 400))))
        for c in range(k % 3):  # 0..2 sites a document
            m = list(query)
            for _ in range((k // 3) % 4):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, len(d) - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    cpu = wfsearch.FitIndex(docs, user_cost=True, index_fn=lambda t, uc: SED.fit_index(t, uc, engine=DefinitionEngine))
    ix = wfsearch.FitIndex(docs, user_cost=True)
    try:
        for T in (0, 6, 12.5):
            for all_ends in (False, True):
                assert ix.occurrences(query, T, all_ends=all_ends) == cpu.occurrences(query, T, all_ends=all_ends)
        occ = ix.occurrences(query, 6, scripts=True)
        assert occ == cpu.occurrences(query, 6, scripts=True) and len(occ) > 10
        assert max(sum(1 for o in occ if o[0] == s) for s in docs) >= 2  # several sites in one document
        for s, score, a, b, es in occ:
            assert SED.patching(es, query)[1] == s[a:b]
        for hit in ix.search(query, max_dist=6):
            assert hit in [o[:4] for o in occ]
        queries = [query, query[:5], "GGNAU", query[::-1]]
        assert ix.occurrences_many(queries, 8) == cpu.occurrences_many(queries, 8)
        assert wfsearch.fit_occurrences(query, docs, 6, user_cost=True) == [o[:4] for o in occ]
    finally:
        ix.close()
        cpu.close()
