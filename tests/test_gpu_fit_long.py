"""GPU: fit search for patterns of up to 2048 symbols over a resident index (sed_fit_index_search_long,
sed_fit_index_hits_long).  Every (query, text) is compared with oracle.fit, every hit list with the
restated definition's rows (test_fit_hits_host.hits_rows: the same (query, text, start, end), dist bit for bit), and for
P <= 32 keys and hit lists with the short kernels' on the same index."""
import importlib
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import fit_envelope
import sedgpu
from fit_envelope import Plan, oracle_fit, planted_text
from test_fit_hits_host import hits_rows
from test_fit_long_host import LongDefinitionEngine
from test_gpu_fit_hits import _plan as golden_plan, _same, _want
from test_gpu_fit_index import _queries

pytestmark = pytest.mark.gpu
E_RANGE = r"\(-4\)"
ROWS = (2, 4, 8, 16, 32)
CHUNK, FORCE = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS


def _unit(K=4, sub=2.0):
    return np.where(np.eye(K) > 0, 0.0, sub)


def _pat(rng, K, P):
    return rng.integers(0, K, size=P).astype(np.uint8)


class _opts:
    def __init__(self, gpu, chunk=0, rows=0):
        self.gpu, self.chunk, self.rows = gpu, chunk, rows

    def __enter__(self):
        self.gpu.set_option(CHUNK, self.chunk)
        self.gpu.set_option(FORCE, self.rows)

    def __exit__(self, *a):
        self.gpu.set_option(CHUNK, 0)
        self.gpu.set_option(FORCE, 0)


def _best(rows):
    """[(dist, start, end)] query-major from the definition's rows: the first strict minimum of E."""
    out = []
    for per_text in rows:
        for E, S in per_text:
            e = int(np.argmin(E))
            out.append((float(E[e]), int(S[e]), e))
    return out


def _check(gpu, plan, ix, pats, texts, chunk=0, rows=0, T=(), oracle=True, defn=None):
    """search_long against the definition's rows (and oracle.fit), hits_long at each T against the rows."""
    gpu.set_costs(plan)
    defn = defn or [hits_rows(plan.sub, plan.ins, plan.dele, p, texts) for p in pats]
    with _opts(gpu, chunk, rows):
        d, s, e = ix.search_long(_queries(pats))
        got = list(zip(d.ravel().tolist(), s.ravel().tolist(), e.ravel().tolist()))
        want = _best(defn)
        bad = [(divmod(i, len(texts)), g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, bad[:5]
        assert ix.last_ms() > 0
        for t in T:
            _same(ix.hits_long(_queries(pats), t), _want(defn, t))
    if oracle:
        assert want == oracle_fit(plan, [p for p in pats for _ in texts], [t for _ in pats for t in texts])
    return defn


def test_long_against_short(gpu):
    """P in {1, 31, 32} at every forced R: keys and sorted hit lists equal the short kernels', bit for bit."""
    plan = golden_plan("user_costs.json", "ACGU")
    rng = np.random.default_rng(1)
    pats = [_pat(rng, 4, P) for P in (1, 31, 32)]
    texts = [planted_text(rng, 4, pats[1 + d % 2], n) for d, n in enumerate((300, 64, 190))] + [np.zeros(0, np.uint8), pats[0][:1]]
    gpu.set_costs(plan)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        for chunk in (72, 0):
            with _opts(gpu, chunk):
                short = ix.search(_queries(pats))
                short_hits = ix.hits(_queries(pats), 3 * plan.dele)
            for R in ROWS:
                with _opts(gpu, chunk, R):
                    lng = ix.search_long(_queries(pats))
                    for a, b in zip(short, lng):
                        assert a.tobytes() == b.tobytes(), (chunk, R)
                    assert ix.hits_long(_queries(pats), 3 * plan.dele).tobytes() == short_hits.tobytes(), (chunk, R)
    finally:
        ix.close()


@pytest.mark.parametrize("R", ROWS)
def test_pattern_and_text_lengths(gpu, R):
    """P = 64 R - 1, 64 R, 64 R + 1 (the next R, or the refusal past 2048), and 33; text lengths 0, 1, P - 1 and 62..65
    around the 63-step skew."""
    plan = Plan(_unit(), 1, 1.5)
    rng = np.random.default_rng(R)
    Ps = [33, 64 * R - 1, 64 * R] + ([64 * R + 1] if R < 32 else [])
    pats = [_pat(rng, 4, P) for P in Ps]
    texts = [np.zeros(0, np.uint8), _pat(rng, 4, 1), pats[1][:-1].copy()] + [planted_text(rng, 4, pats[0], n) for n in (62, 63, 64, 65)]
    texts.append(planted_text(rng, 4, pats[2], 64 * R + 70, copies=1))
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        _check(gpu, plan, ix, pats, texts, T=(2.0,))
        if R == 32:
            with pytest.raises(sedgpu.SedError, match=E_RANGE):
                ix.search_long(_queries([_pat(rng, 4, 2049)]))
            with pytest.raises(sedgpu.SedError, match=E_RANGE):
                ix.hits_long(_queries([_pat(rng, 4, 2049)]), 1.0)
            _check(gpu, plan, ix, pats[:1], texts)  # (the index is usable after a refusal)
    finally:
        ix.close()


def test_planted_copies_on_seams_and_rebases(gpu):
    """Chunk 200, P = 150 (R = 4: the lanes rebase at different steps), insert = delete = 1: copies with substitutions,
    an insertion and a deletion; ends on a wave's first owned column (400), its last (599), column n, column 0 of an
    empty text; and ends at the wave columns 127, 128, 129 and 256 of the one-chunk waves."""
    plan = Plan(_unit(), 1, 1)
    rng = np.random.default_rng(150)
    p = _pat(rng, 4, 150)
    variants = [p.copy(), p.copy(), np.delete(p, 70), np.insert(p, 40, (p[40] + 1) % 4)]
    variants[1][[3, 77, 140]] = (variants[1][[3, 77, 140]] + 1) % 4
    texts = []
    for i, end in enumerate((400, 599, 700, 300)):
        t = rng.integers(0, 4, size=700).astype(np.uint8)
        v = variants[i]
        t[end - len(v):end] = v
        texts.append(t)
    texts.append(np.zeros(0, np.uint8))
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        defn = _check(gpu, plan, ix, [p], texts, chunk=200, T=(0.0, 3.0))
        assert [int(np.argmin(E)) for E, _ in defn[0]][:3] == [400, 599, 700]
        _check(gpu, plan, ix, [p], texts, chunk=0, T=(3.0,), defn=defn, oracle=False)
    finally:
        ix.close()
    texts = []
    for end in (127, 128, 129, 256):  # one chunk per text: wave column = text column
        t = rng.integers(0, 4, size=300).astype(np.uint8)
        t[end - 100:end] = p[50:]
        texts.append(t)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        defn = _check(gpu, plan, ix, [p[50:], p], texts, chunk=1 << 20, T=(0.0, 2.0))
        assert [int(np.argmin(E)) for E, _ in defn[0]] == [127, 128, 129, 256]
    finally:
        ix.close()


def test_ties(gpu):
    """A homopolymer text and a periodic text (largest start, smallest end), and all eight symbols."""
    plan = Plan(_unit(), 1, 1)
    p = np.array(([0] * 20 + [1] * 20) * 2, np.uint8)
    texts = [np.zeros(200, np.uint8), np.array(([0] * 20 + [1] * 20) * 6, np.uint8), np.ones(77, np.uint8)]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        for chunk in (72, 0):
            _check(gpu, plan, ix, [p, p[:33]], texts, chunk=chunk, T=(5.0, math.inf))
    finally:
        ix.close()
    plan8 = fit_envelope.eight_symbol_table(8)
    rng = np.random.default_rng(8)
    p8 = _pat(rng, 8, 100)
    p8[:8] = rng.permutation(8)
    texts = [planted_text(rng, 8, p8, 400), planted_text(rng, 8, p8, 90)]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        _check(gpu, plan8, ix, [p8], texts, chunk=72, T=(300.0,))
    finally:
        ix.close()


def test_chunks_and_chunk_table_cache(gpu):
    """Forced chunks 8 and 72, automatic, one chunk per text; then 8, 72, 8 again on the same index."""
    plan = Plan(_unit(), 1, 1.25)
    rng = np.random.default_rng(72)
    pats = [_pat(rng, 4, P) for P in (40, 129)]
    texts = [planted_text(rng, 4, pats[d % 2], n) for d, n in enumerate((333, 64, 7, 500))]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        defn = None
        for chunk in (8, 72, 0, 1 << 20, 8, 72, 8):
            defn = _check(gpu, plan, ix, pats, texts, chunk=chunk, T=(4.0,), defn=defn, oracle=defn is None)
    finally:
        ix.close()


@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_golden_cost_tables(gpu, name, alphabet):
    K = len(alphabet)
    plan = golden_plan(name, alphabet)
    rng = np.random.default_rng(len(name) + K)
    pats = [_pat(rng, K, P) for P in (76, 200)]
    texts = [planted_text(rng, K, pats[d % 2], n) for d, n in enumerate((300, 450, 50))]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        _check(gpu, plan, ix, pats, texts, chunk=72, T=(3 * plan.dele,))
        _check(gpu, plan, ix, pats, texts, T=(0.0,), oracle=False)
    finally:
        ix.close()


def test_envelope_limits(gpu):
    """(insert + delete) S = 255; the D-field limit P delete S + 128 insert S = 65535 and its refusal one past; with
    insert = 0 the limit is D = 65535 itself."""
    rng = np.random.default_rng(255)
    for name, plan in fit_envelope.cost_limit_tables()[:4]:
        P = min(100, int((65535 - 128 * plan.ins) // max(plan.dele, 1)))
        p = _pat(rng, plan.K, P)
        texts = [planted_text(rng, plan.K, p, 300)]
        ix = sedgpu.FitIndex.from_texts(gpu, texts)
        try:
            _check(gpu, plan, ix, [p], texts, chunk=72, T=(float(plan.dele * 3),))
        finally:
            ix.close()
    sub = _unit(4, 255.0)
    for ins, dele, P in ((0, 255, 257), (3, 252, 258)):
        assert P * dele + 128 * ins <= 65535 < (P + 1) * dele + 128 * ins
        plan = Plan(sub, ins, dele)
        p = _pat(rng, 4, P + 1)
        t = planted_text(rng, 4, p[:P], 330, copies=1)
        texts = [t, (3 - t[:20]).astype(np.uint8)]
        ix = sedgpu.FitIndex.from_texts(gpu, texts)
        try:
            _check(gpu, plan, ix, [p[:P]], texts, T=(0.0, math.inf))
            with pytest.raises(sedgpu.SedError, match=E_RANGE):
                ix.search_long(_queries([p]))
        finally:
            ix.close()


def test_zero_costs_and_long_texts(gpu):
    """delete = 0; insert = 0 over 3000 symbols in one wave; a 70 000-symbol text whose best end is past 2^16."""
    rng = np.random.default_rng(70000)
    p = _pat(rng, 4, 90)
    for ins, dele, n in ((1.25, 0, 400), (0, 2.5, 3000)):
        plan = Plan(_unit(4, 1.5), ins, dele)
        texts = [planted_text(rng, 4, p, n)]
        ix = sedgpu.FitIndex.from_texts(gpu, texts)
        try:
            _check(gpu, plan, ix, [p], texts, T=(1.5,))
            if ins == 0:
                assert sedgpu.FitIndex.long_plan(plan.costs(), {}, [90], [n])["lanes"] == 1
        finally:
            ix.close()
    plan = Plan(_unit(), 1, 1)
    t = rng.integers(0, 4, size=70000).astype(np.uint8)
    t[69000:69090] = p
    ix = sedgpu.FitIndex.from_texts(gpu, [t])
    try:
        gpu.set_costs(plan)
        d, s, e = ix.search_long(_queries([p]))
        assert (d[0, 0], s[0, 0], e[0, 0]) == (0.0, 69000, 69090)
        assert [(d0, s0, e0) for d0, s0, e0 in zip(d.ravel(), s.ravel(), e.ravel())] == oracle_fit(plan, [p], [t])
        hits = ix.hits_long(_queries([p]), 0.0)
        assert hits["end"].tolist() == [69090] and hits["start"].tolist() == [69000]
    finally:
        ix.close()


def test_hits_thresholds_and_cap(gpu):
    """T = 0, mid, >= P delete (exactly Q sum(n + 1) hits) and +inf; cap = found - 1, found and 0, then a search_long on
    the same index."""
    plan = golden_plan("user_costs.json", "ACGU")
    rng = np.random.default_rng(9)
    pats = [_pat(rng, 4, P) for P in (50, 140)]
    texts = [planted_text(rng, 4, pats[d % 2], n) for d, n in enumerate((260, 0, 33, 150))]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        defn = _check(gpu, plan, ix, pats, texts, chunk=72, T=(0.0, 6 * plan.dele, 140 * plan.dele, math.inf))
        every = _want(defn, math.inf)
        assert len(every) == len(pats) * sum(len(t) + 1 for t in texts) == len(_want(defn, 140 * plan.dele))
        want = _want(defn, 6 * plan.dele)
        assert 0 < len(want) < len(every)
        for cap in (len(want) - 1, 0):
            with pytest.raises(sedgpu.SedError, match=E_RANGE):
                ix.hits_long(_queries(pats), 6 * plan.dele, cap=cap)
            assert ix.found == len(want)
        _same(ix.hits_long(_queries(pats), 6 * plan.dele, cap=len(want)), want)
        _check(gpu, plan, ix, pats, texts, defn=defn, oracle=False)
    finally:
        ix.close()


def test_query_mix_and_reuse(gpu):
    """65 queries of mixed lengths in three R groups x 130 texts (a ragged last block of chunk records), results in query
    order whatever the grouping; then long and short searches alternating on one index with a batch between."""
    plan = Plan(_unit(), 1, 1)
    rng = np.random.default_rng(65)
    lens = [(20, 100, 200)[i % 3] + i for i in range(65)]
    pats = [_pat(rng, 4, P) for P in lens]
    texts = [planted_text(rng, 4, pats[d % 65], 60 + d) if d % 4 else rng.integers(0, 4, size=d).astype(np.uint8) for d in range(130)]
    assert set(sedgpu.FitIndex.long_plan(plan.costs(), {}, lens, [len(t) for t in texts])["rows"].tolist()) == {2, 4, 8}
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        _check(gpu, plan, ix, pats, texts)
        short = [p for p in pats if len(p) <= 32][:3]
        for _ in range(2):
            with _opts(gpu, 72):
                a = ix.search(_queries(short))
                packed = sedgpu.PackedPairs(pats[:4], texts[100:104])
                gpu.run(packed, True)
                b = ix.search_long(_queries(short))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        ix.close()


def test_wfsearch_long_patterns(gpu, monkeypatch):
    """wfsearch.FitIndex.occurrences(long_patterns=True, scripts=True) on the engine equals the same call over the
    index_fn engine that serves the definition, and patching(es, query) gives sequence[start:end]."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    rng = np.random.default_rng(76)
    query = "".join(rng.choice(list("ACGU"), size=76))
    docs = [""]
    for k in range(1, 12):
        d = list(rng.choice(list("ACGU"), size=int(rng.integers(200, 400))))
        for c in range(k % 3):
            m = list(query)
            for _ in range((k // 3) % 4):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, len(d) - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    cpu = wfsearch.FitIndex(docs, user_cost=True, index_fn=lambda t, uc: SED.fit_index(t, uc, engine=LongDefinitionEngine))
    ix = wfsearch.FitIndex(docs, user_cost=True)
    try:
        with pytest.raises(sedgpu.SedError, match=E_RANGE):
            ix.occurrences(query, 6)
        for T in (0, 6):
            assert ix.occurrences(query, T, long_patterns=True) == cpu.occurrences(query, T, long_patterns=True)
        occ = ix.occurrences(query, 6, scripts=True, long_patterns=True)
        assert occ == cpu.occurrences(query, 6, scripts=True, long_patterns=True) and len(occ) >= 8
        for s, score, a, b, es in occ:
            assert SED.patching(es, query)[1] == s[a:b]
        for hit in ix.search(query, max_dist=6, long_patterns=True):
            assert hit in [o[:4] for o in occ]
        queries = [query[:20], query, query[5:45], query + query[::-1]]
        assert ix.occurrences_many(queries, 8, long_patterns=True) == cpu.occurrences_many(queries, 8, long_patterns=True)
        assert ix.search_many(queries, long_patterns=True) == cpu.search_many(queries, long_patterns=True)
        assert wfsearch.fit_occurrences(query, docs, 6, user_cost=True, long_patterns=True) == [o[:4] for o in occ]
    finally:
        ix.close()
        cpu.close()
