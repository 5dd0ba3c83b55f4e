"""GPU: fit search over a resident index (sed_fit_index_search).  Every (query, text) hit must equal,
bit for bit, what Context.fit (sed_fit_search) returns for the materialised cross product under the same costs and
chunk option, and what the compiled definition, oracle.fit, gives."""
import importlib
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import fit_envelope
import oracle
import sedgpu
from test_gpu_fit import _fuzz_pairs, _golden_plan

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_RANGE = r"\(-1\)", r"\(-6\)", r"\(-4\)"


def _queries(pats):
    """The queries as side a of a PackedPairs (side b: empty texts, not read)."""
    return sedgpu.PackedPairs(pats, [np.zeros(0, np.uint8)] * len(pats))


def _cross(pats, texts):
    """The queries x texts cross product, query-major, one copy of each sequence shared through the offsets."""
    Q, D = len(pats), len(texts)
    offp = np.concatenate([[0], np.cumsum([len(x) for x in pats])]).astype(np.int64)
    offt = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64)
    qi, di = np.divmod(np.arange(Q * D), D)
    return types.SimpleNamespace(
        npairs=Q * D, codes_a=np.concatenate(list(pats) + [np.zeros(1, np.uint8)]), off_a=offp[qi].copy(),
        len_a=np.array([len(pats[q]) for q in qi], np.int32), codes_b=np.concatenate(list(texts) + [np.zeros(1, np.uint8)]),
        off_b=offt[di].copy(), len_b=np.array([len(texts[d]) for d in di], np.int32))


def _check(gpu, plan, ix, pats, texts, chunk=0, want=None):
    """Search the index and compare with Context.fit on the cross product (same costs, same chunk option), bit for
    bit, and with oracle.fit.  want: the oracle's hits when the caller has them already."""
    Q, D = len(pats), len(texts)
    gpu.set_costs(plan)
    xp = _cross(pats, texts)
    try:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, chunk)
        d, s, e = ix.search(_queries(pats))
        fd, fs, fe = gpu.fit(xp)
    finally:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)
    assert d.shape == s.shape == e.shape == (Q, D)
    assert np.array_equal(d.ravel().view(np.uint64), fd.view(np.uint64))
    assert np.array_equal(s.ravel(), fs) and np.array_equal(e.ravel(), fe)
    if want is None:
        want = oracle.fit(oracle.Costs.from_plan(plan), xp.codes_a, xp.off_a, xp.len_a, xp.codes_b, xp.off_b, xp.len_b,
                          xp.npairs, 8)
    bad = np.flatnonzero((fd != want[0]) | (fs != want[1]) | (fe != want[2]))
    assert not len(bad), [(int(i), (fd[i], fs[i], fe[i]), tuple(w[i] for w in want)) for i in bad[:5]]
    assert ix.last_ms() > 0
    return want


def _basic(K, seed):
    """70 texts of 0..300 symbols with planted mutated copies (text 3 empty, a 1-symbol text), 5 queries: P = 1, 31, 32
    and two of random length that are planted in texts."""
    rng = np.random.default_rng(seed)
    pats, texts = _fuzz_pairs(rng, K, 70)
    texts[4] = texts[4][:1] if len(texts[4]) else np.zeros(1, np.uint8)
    assert len(texts[3]) == 0 and len(texts[4]) == 1 and [len(p) for p in pats[:3]] == [1, 31, 32]
    return [pats[0], pats[1], pats[2], pats[5], pats[7]], texts


@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_basic_parity(gpu, name, alphabet):
    plan = _golden_plan(name, alphabet)
    pats, texts = _basic(len(alphabet), 70 + len(name) + len(alphabet))
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        assert ix.ntexts == 70 and ix.symbols == sum(len(t) for t in texts)
        with pytest.raises(sedgpu.SedError, match=E_STATE):
            ix.last_ms()
        want = None
        for chunk in (8, 72, 0, 1 << 20):  # forced, automatic, one lane per text
            want = _check(gpu, plan, ix, pats, texts, chunk, want)
    finally:
        ix.close()


def test_chunk_table_cache(gpu):
    plan = _golden_plan("user_costs.json", "ACGU")
    pats, texts = _basic(4, 872)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        want = None
        for chunk in (8, 72, 8, 8, 0, 8):
            want = _check(gpu, plan, ix, pats[:3], texts, chunk, want)
    finally:
        ix.close()


def test_costs_change_under_the_index(gpu):
    pats, texts = _basic(4, 12)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        a = _check(gpu, _golden_plan("costs.json", "ACGU"), ix, pats, texts)
        b = _check(gpu, _golden_plan("user_costs.json", "ACGU"), ix, pats, texts)
        assert not np.array_equal(a[0], b[0])
        _check(gpu, _golden_plan("costs.json", "ACGU"), ix, pats, texts, want=a)
        _check(gpu, _golden_plan("costs.json", "ACGUN"), ix, pats, texts)  # (a fifth symbol no text holds)
    finally:
        ix.close()


def test_text_code_beyond_k_is_refused_before_any_launch(gpu):
    rng = np.random.default_rng(5)
    texts = [rng.integers(0, 4, size=40).astype(np.uint8) for _ in range(6)]
    texts[2][7] = 4  # the code K - 1 of a 5-symbol alphabet
    pats = [rng.integers(0, 4, size=9).astype(np.uint8)]
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        gpu.set_costs(_golden_plan("costs.json", "ACGU"))
        with pytest.raises(sedgpu.SedError, match=E_ARG + ".*text code 4"):
            ix.search(_queries(pats))
        with pytest.raises(sedgpu.SedError, match=E_STATE):  # nothing ran
            ix.last_ms()
        with pytest.raises(sedgpu.SedError, match=E_ARG + ".*pattern code"):
            gpu.set_costs(_golden_plan("costs.json", "ACGUN"))
            ix.search(_queries([np.array([0, 5], np.uint8)]))
        _check(gpu, _golden_plan("costs.json", "ACGUN"), ix, pats, texts)
    finally:
        ix.close()


def _unit(K=4, sub=2.0):
    return np.where(np.eye(K) > 0, 0.0, sub)


def test_long_text(gpu):
    """One text of 70 000 among short ones under the automatic rule: it is split (insert 1, delete 4, P = 32: W = 160),
    copies sit across seams and at the very end, where end needs more than 16 bits."""
    plan = fit_envelope.Plan(_unit(), 1, 4)
    rng = np.random.default_rng(70000)
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    pats = [p, p[:9].copy(), rng.integers(0, 4, size=20).astype(np.uint8)]
    texts = [fit_envelope.planted_text(rng, 4, p, n) if n > 40 else rng.integers(0, 4, size=n).astype(np.uint8)
             for n in (0, 1, 3, 299, 150)]
    long = rng.integers(0, 4, size=70000).astype(np.uint8)
    got = sedgpu.fit_index_plan(plan.costs(), {}, [32, 9, 20], [len(t) for t in texts] + [70000])
    chunk = got["chunk"]
    assert got["W"] == 160 and 0 < chunk < 70000
    # 3-edit copies of p end one column before a seam, at one and one after one
    m = fit_envelope.mutate(rng, p, 4, 3)
    for end in (chunk - 1, 7 * chunk, 300 * chunk + 1):
        long[end - len(m):end] = m
    long[70000 - 20:] = pats[2]  # (an exact copy of a random 20-mer: nowhere else, by all odds)
    texts.insert(2, long)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        d, s, e = _check(gpu, plan, ix, pats, texts)
        d, s, e = (x.reshape(3, len(texts)) for x in (d, s, e))
        assert (d[2, 2], s[2, 2], e[2, 2]) == (0.0, 70000 - 20, 70000) and e[2, 2] > 1 << 16
        assert d[0, 2] <= 3 * 5  # (a 3-edit copy of p)
        _check(gpu, plan, ix, pats, texts, chunk=65535 - 160 - 3)  # the longest lanes there are
    finally:
        ix.close()


def test_zero_insert(gpu):
    """insert = 0: one chunk per text whatever the option says; 65 534 symbols is the longest text served, and an
    index that holds 65 535 is refused at search, not at creation, and serves other costs."""
    plan = fit_envelope.Plan(_unit(), 0, 1.5)
    rng = np.random.default_rng(65534)
    pats = [rng.integers(0, 4, size=P).astype(np.uint8) for P in (1, 31, 32)]
    texts = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (0, 1, 127, 128, 129)]
    texts.append(fit_envelope.planted_text(rng, 4, pats[2], 65534))
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        want = _check(gpu, plan, ix, pats, texts)
        _check(gpu, plan, ix, pats, texts, chunk=64, want=want)
    finally:
        ix.close()
    texts[-1] = np.concatenate([texts[-1], np.zeros(1, np.uint8)])  # 65 535
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        gpu.set_costs(plan)
        with pytest.raises(sedgpu.SedError, match=E_RANGE + ".*span.*insert = 0"):
            ix.search(_queries(pats))
        with pytest.raises(sedgpu.SedError, match=E_STATE):
            ix.last_ms()
        _check(gpu, fit_envelope.Plan(_unit(), 1, 1.5), ix, pats[:1], texts)
    finally:
        ix.close()


@pytest.mark.parametrize("K", [6, 8])
def test_all_eight_symbols(gpu, K):
    rng = np.random.default_rng(800 + K)
    plan = fit_envelope.eight_symbol_table(K)
    pats, texts = _fuzz_pairs(rng, K, 60)
    pats = pats[:3] + pats[5:8]
    assert set(np.concatenate(pats).tolist()) == set(range(K)) == set(np.concatenate(texts).tolist())
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        want = _check(gpu, plan, ix, pats, texts)
        _check(gpu, plan, ix, pats, texts, chunk=8, want=want)
    finally:
        ix.close()


def test_many_queries_ragged_chunks(gpu):
    """65 queries of differing P against 130 texts under chunk 8: more than one block in x, its last block partly idle
    for every query."""
    rng = np.random.default_rng(65130)
    plan = _golden_plan("user_costs.json", "ACGU")
    pats = [rng.integers(0, 4, size=1 + (q * 7) % 32).astype(np.uint8) for q in range(65)]
    texts = [rng.integers(0, 4, size=int(rng.integers(0, 90))).astype(np.uint8) for _ in range(130)]
    for q in range(0, 65, 2):
        t = texts[2 * q]
        if len(t) >= len(pats[q]):
            t[len(t) - len(pats[q]):] = pats[q]
    nchunks = sedgpu.fit_index_plan(fit_envelope.Plan(plan.sub, plan.ins, plan.dele).costs(), {sedgpu.SED_OPT_FIT_CHUNK: 8},
                                    [1], [len(t) for t in texts])["lanes"]
    assert nchunks > 64 and nchunks % 64
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        _check(gpu, plan, ix, pats, texts, chunk=8)
    finally:
        ix.close()


def _two_launches():
    """65 537 queries, two more than one launch's 65 535 (the grid's y limit): all 20 patterns of length 1-2 over ACGU
    in turn, against two texts of 6 and 9 symbols.  Returns (the 20 patterns, the queries, the texts)."""
    base = [np.array([a], np.uint8) for a in range(4)] + [np.array([a, b], np.uint8) for a in range(4) for b in range(4)]
    rng = np.random.default_rng(65537)
    texts = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (6, 9)]
    return base, [base[q % 20] for q in range(65537)], texts


def test_search_beyond_one_launch_of_queries(gpu):
    """The search's second launch, and the events around both: every (query, text) equals oracle.fit (one run per
    distinct pattern and text, broadcast), and the search's time is that of a run."""
    plan = _golden_plan("user_costs.json", "ACGU")
    base, pats, texts = _two_launches()
    xp = _cross(base, texts)
    want = oracle.fit(oracle.Costs.from_plan(plan), xp.codes_a, xp.off_a, xp.len_a, xp.codes_b, xp.off_b, xp.len_b,
                      xp.npairs, 8)
    which = np.arange(len(pats)) % 20
    gpu.set_costs(plan)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        got = ix.search(_queries(pats))
        for g, w in zip(got, want):
            assert g.shape == (65537, 2) and np.array_equal(g, np.asarray(w).reshape(20, 2)[which])
        ms = ix.last_ms()
        assert ms > 0 and np.isfinite(ms)
    finally:
        ix.close()


def test_hits_beyond_one_launch_of_queries(gpu):
    """The same queries through hits(max_dist=0): the sorted list equals the definition's (test_gpu_fit_hits: _rows and
    _want, one row set per distinct pattern), found is its length, and the hits kernels' time is that of a run."""
    from test_gpu_fit_hits import _plan, _rows, _same, _want  # (that module imports this one)
    plan = _plan("user_costs.json", "ACGU")
    base, pats, texts = _two_launches()
    rows = _rows(plan, base, texts)
    want = _want([rows[q % 20] for q in range(len(pats))], 0)
    gpu.set_costs(plan)
    ix = sedgpu.FitIndex.from_texts(gpu, texts)
    try:
        got = ix.hits(_queries(pats), 0)
        _same(got, want)
        assert ix.found == len(want) > 65537 and ix.hits_last_ms() > 0
    finally:
        ix.close()


def test_two_indexes_on_one_context(gpu):
    """Two indexes searched alternately, with a Context.fit and a sed_run_batch between: each keeps its own buffers."""
    plan = _golden_plan("user_costs.json", "ACGU")
    pa, ta = _basic(4, 1)
    pb, tb = _basic(4, 2)
    tb = tb[:33]
    a, b = sedgpu.FitIndex.from_texts(gpu, ta), sedgpu.FitIndex.from_texts(gpu, tb)
    try:
        wa = _check(gpu, plan, a, pa, ta)
        wb = _check(gpu, plan, b, pb, tb, chunk=8)
        x, y = np.array([0, 1, 2, 3, 0], np.uint8), np.array([0, 1, 3, 3], np.uint8)
        dist, _, ln, _ = gpu.run(sedgpu.PackedPairs([x] * 3, [y] * 3), True)
        o = oracle.pair(oracle.Costs.from_plan(plan), x, y)
        assert dist.tolist() == [o["dist"]] * 3 and ln.tolist() == [o["len"]] * 3
        _check(gpu, plan, a, pa[:2], ta)
        _check(gpu, plan, b, pb, tb, chunk=8, want=wb)
        _check(gpu, plan, a, pa, ta, want=wa)
    finally:
        a.close()
        b.close()


def test_empty_cases_and_close(gpu):
    gpu.set_costs(_golden_plan("costs.json", "ACGU"))
    p = [np.array([0, 1, 2], np.uint8)]
    empty = sedgpu.FitIndex.from_texts(gpu, [])
    d, s, e = empty.search(_queries(p))
    assert d.shape == s.shape == e.shape == (1, 0) and empty.ntexts == 0 and empty.symbols == 0
    ix = sedgpu.FitIndex.from_texts(gpu, [np.zeros(5, np.uint8), np.zeros(0, np.uint8)])
    d, s, e = ix.search(_queries([]))
    assert d.shape == s.shape == e.shape == (0, 2)
    for x in (empty, ix):
        with pytest.raises(sedgpu.SedError, match=E_STATE):  # no launch so far
            x.last_ms()
    texts = [np.zeros(5, np.uint8), np.zeros(0, np.uint8)]
    d, s, e = _check(gpu, _golden_plan("costs.json", "ACGU"), ix, p, texts)
    assert (s.tolist(), e.tolist()) == ([0, 0], [1, 0])  # (A of ACG matches; the empty text: the empty window)
    for x in (empty, ix):
        x.close()
        x.close()
    with pytest.raises(sedgpu.SedError, match="closed"):
        ix.search(_queries(p))


def test_pair_in_flight_is_a_state_error(gpu):
    gpu.set_costs(_golden_plan("costs.json", "ACGU"))
    ix = sedgpu.FitIndex.from_texts(gpu, [np.zeros(5, np.uint8)])
    try:
        gpu.submit_pair(bytes([0, 1, 2]), bytes([0, 1]), False)
        try:
            with pytest.raises(sedgpu.SedError, match=E_STATE):
                ix.search(_queries([np.zeros(2, np.uint8)]))
        finally:
            gpu.wait_pair()
        assert ix.search(_queries([np.zeros(2, np.uint8)]))[0].tolist() == [[0.0]]
    finally:
        ix.close()


def test_wfsearch_fit_index_on_the_engine(gpu, monkeypatch):
    """wfsearch.FitIndex.search(query, max_dist, scripts=True) equals fit_search with the same arguments on 40
    sequences, and search_many equals one search per query."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    monkeypatch.setattr(wfsearch.SED, "user_costs", load_golden("user_costs.json"))
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    rng = np.random.default_rng(40)
    query = "".join(rng.choice(list("ACGU"), size=28))
    docs = []
    for k in range(40):
        d = list(rng.choice(list("ACGU"), size=int(rng.integers(60, 400))))
        if k % 2 == 0:
            m = list(query)
            for _ in range(k // 4):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, len(d) - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    ix = wfsearch.FitIndex(docs, user_cost=True)
    try:
        for max_dist in (None, 6, 0):
            want = wfsearch.fit_search(query, docs, user_cost=True, max_dist=max_dist, scripts=True)
            assert ix.search(query, max_dist=max_dist, scripts=True) == want
        assert len(want) >= 1 and want[0][1] == 1.0 and wfsearch.SED.patching(want[0][4], query) == (0, query)
        queries = [query, query[:5], "GGNAU", query[::-1]]
        assert ix.search_many(queries, max_dist=8) == [wfsearch.fit_search(q, docs, True, max_dist=8) for q in queries]
    finally:
        ix.close()
        ix.close()
