"""GPU: fit search (sed_fit_search) against the pure-Python restatement of its definition
(tests/test_fit_host.py: fit_definition); for every hit the C oracle must also give G(start, end) = dist.  The tests of
the numeric envelope (second half) take the compiled restatement, oracle.fit, which is pinned to the same definition on
the CPU (tests/test_fit_host.py), so that long texts and large batches stay quick."""
import importlib
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import fit_envelope
import oracle
import sedcost
import sedgpu
from test_fit_host import fit_definition, fit_definition_str

pytestmark = pytest.mark.gpu


class _Plan:
    """A cost model over codes 0..K-1, as Context.set_costs and oracle.Costs.from_plan read it."""

    def __init__(self, sub, ins, dele):
        self.sub = np.ascontiguousarray(sub, np.float64)
        self.K = len(self.sub)
        self.sub_int = np.zeros((self.K, self.K), np.uint8)
        self.ins, self.ins_int, self.dele, self.del_int = float(ins), 0, float(dele), 0

    def key(self):
        return (self.K, self.sub.tobytes(), self.ins, self.dele)


def _golden_plan(name, alphabet):
    p = sedcost.build_plan(load_golden(name), [alphabet], [alphabet])
    return _Plan(p.sub, p.ins, p.dele)


def _check(gpu, plan, pats, texts, packed=None):
    """Run the pairs and compare every hit with the definition and with the oracle's G(start, end)."""
    gpu.set_costs(plan)
    packed = packed or sedgpu.PackedPairs(pats, texts)
    dist, start, end = gpu.fit(packed)
    sub = plan.sub.tolist()
    want = [fit_definition(sub, plan.ins, plan.dele, p.tolist(), t.tolist()) for p, t in zip(pats, texts)]
    got = list(zip(dist.tolist(), start.tolist(), end.tolist()))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
    win = sedgpu.PackedPairs(pats, [t[s:e] for t, (_, s, e) in zip(texts, got)])
    g = oracle.batch(oracle.Costs.from_plan(plan), win.codes_a, win.off_a, win.len_a, win.codes_b, win.off_b, win.len_b,
                     win.npairs)[0]
    assert g[:len(got)].tolist() == dist.tolist()
    return got


def _mutate(rng, p, K, edits):
    s = p.tolist()
    for _ in range(edits):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(s) + 1))
        if kind == 0 and len(s) > 1:
            del s[min(at, len(s) - 1)]
        elif kind == 1:
            s.insert(at, int(rng.integers(0, K)))
        else:
            s[min(at, len(s) - 1)] = int(rng.integers(0, K))
    return np.array(s, np.uint8)


def _fuzz_pairs(rng, K, count):
    pats, texts = [], []
    for it in range(count):
        P = (1, 31, 32)[it] if it < 3 else int(rng.integers(1, 33))
        n = 0 if it == 3 else int(rng.integers(0, 301))
        p = rng.integers(0, K, size=P).astype(np.uint8)
        t = rng.integers(0, K, size=n).astype(np.uint8)
        if it % 2 and n:  # a mutated copy of the pattern somewhere in the text
            m = _mutate(rng, p, K, int(rng.integers(0, 4)))[:n]
            at = int(rng.integers(0, n - len(m) + 1))
            t[at:at + len(m)] = m
        pats.append(p)
        texts.append(t)
    return pats, texts


@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_fuzz(gpu, name, alphabet):
    rng = np.random.default_rng(len(name) * 100 + len(alphabet))
    pats, texts = _fuzz_pairs(rng, len(alphabet), 200)  # (x 3 cost models: 600 pairs)
    _check(gpu, _golden_plan(name, alphabet), pats, texts)


def test_seams(gpu):
    """One 3000-symbol text, P = 32, insert 1 and delete 4 (W = 160): occurrences ending one column before, at and one
    after a seam of every chunking give the same hits as one chunk, which are the definition's."""
    rng = np.random.default_rng(160)
    sub = np.where(np.eye(4) > 0, 0.0, 2.0)
    plan = _Plan(sub, 1, 4)
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    chunks = (160, 161, 255, 1024)
    pats, texts = [], []
    for c in chunks:
        for seam in (c, 2 * c):  # the second chunk's first owned column c0, and the third's
            for end in (seam - 1, seam, seam + 1):
                for edits in (0, 3):
                    t = rng.integers(0, 4, size=3000).astype(np.uint8)
                    m = p if edits == 0 else _mutate(rng, p, 4, 3)
                    t[end - len(m):end] = m
                    pats.append(p)
                    texts.append(t)
    base = None
    try:
        for c in chunks + (1 << 20,):
            gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, c)
            got = _check(gpu, plan, pats, texts)
            base = base or got
            assert got == base
    finally:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)
    assert sum(d == 0 for d, _, _ in base) >= len(base) // 2  # (the exact copies were found)


def test_ties(gpu):
    plan = _golden_plan("costs.json", "ACGU")
    aa = np.zeros(2, np.uint8)
    assert _check(gpu, plan, [aa], [np.zeros(40, np.uint8)]) == [(0.0, 0, 2)]  # the smallest end, then the largest start
    a = np.zeros(1, np.uint8)
    assert _check(gpu, plan, [a], [np.zeros(9, np.uint8)]) == [(0.0, 0, 1)]
    occ = np.array([0, 1, 2, 3, 0], np.uint8)
    t = np.concatenate([np.full(20, 3, np.uint8), occ, np.full(30, 3, np.uint8), occ, np.full(10, 3, np.uint8)])
    assert _check(gpu, plan, [occ], [t]) == [(0.0, 20, 25)]  # the same occurrence twice: the first
    # equal distance from a longer and a shorter window ending at the same column: the shorter (largest start)
    assert _check(gpu, _Plan(np.where(np.eye(4) > 0, 0.0, 1.0), 1, 1), [np.array([0, 1], np.uint8)],
                  [np.array([2, 2, 0, 2, 2], np.uint8)]) == [(1.0, 2, 3)]


@pytest.mark.parametrize("npairs", [1, 64, 65, 257])
def test_wave_geometry(gpu, npairs):
    rng = np.random.default_rng(npairs)
    plan = _golden_plan("user_costs.json", "ACGU")
    pats = [rng.integers(0, 4, size=int(rng.integers(1, 33))).astype(np.uint8) for _ in range(npairs)]
    texts = [rng.integers(0, 4, size=int(rng.integers(0, 260))).astype(np.uint8) for _ in range(npairs)]
    _check(gpu, plan, pats, texts)


def test_shared_patterns_and_texts(gpu):
    """16 patterns x 16 texts through the offsets: one copy of each."""
    rng = np.random.default_rng(1616)
    plan = _golden_plan("costs.json", "ACGUN")
    P = [rng.integers(0, 5, size=int(rng.integers(1, 33))).astype(np.uint8) for _ in range(16)]
    T = [rng.integers(0, 5, size=int(rng.integers(0, 400))).astype(np.uint8) for _ in range(16)]
    for k in range(16):  # each text holds one of the patterns
        if len(T[k]) >= len(P[k]):
            T[k][:len(P[k])] = P[k]
    offp = np.concatenate([[0], np.cumsum([len(x) for x in P])]).astype(np.int64)
    offt = np.concatenate([[0], np.cumsum([len(x) for x in T])]).astype(np.int64)
    qi, di = np.divmod(np.arange(256), 16)
    packed = types.SimpleNamespace(
        npairs=256, codes_a=np.concatenate(P + [np.zeros(1, np.uint8)]), off_a=offp[qi].copy(),
        len_a=np.array([len(P[q]) for q in qi], np.int32), codes_b=np.concatenate(T + [np.zeros(1, np.uint8)]),
        off_b=offt[di].copy(), len_b=np.array([len(T[d]) for d in di], np.int32))
    _check(gpu, plan, [P[q] for q in qi], [T[d] for d in di], packed=packed)


def test_refused_models_raise_and_leave_the_context_usable(gpu):
    p5, t = np.zeros(5, np.uint8), np.ones(40, np.uint8)
    t66 = load_golden("costs.json")
    ard = sedcost.build_plan(t66, ["ARD"], ["ARD"])
    cases = [(_Plan(ard.sub, ard.ins, ard.dele), p5),                              # 0.66: not dyadic
             (_Plan(np.where(np.eye(9) > 0, 0.0, 1.0), 1, 1), p5),                 # 9 symbols
             (_golden_plan("costs.json", "ACGU"), np.zeros(33, np.uint8))]         # P = 33
    for plan, p in cases:
        gpu.set_costs(plan)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*fit search"):
            gpu.fit(sedgpu.PackedPairs([p], [t]))
    plan = _golden_plan("user_costs.json", "ACGU")
    gpu.set_costs(plan)
    a, b = np.array([0, 1, 2, 3, 0], np.uint8), np.array([0, 1, 3, 3], np.uint8)
    d, is_int, ln, _ = gpu.run_pair(a.tobytes(), b.tobytes(), False)
    o = oracle.pair(oracle.Costs.from_plan(plan), a, b)
    assert d == o["dist"] and ln == o["len"]
    assert _check(gpu, plan, [a], [b])[0][0] <= d


def test_fit_search_with_scripts(gpu, monkeypatch):
    """wfsearch.fit_search(scripts=True) on 8 documents of 400 nt: the script of every hit patches the query into
    the matched substring and costs dist."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    SED = wfsearch.SED
    table = load_golden("user_costs.json")
    monkeypatch.setattr(SED, "user_costs", table)
    monkeypatch.setattr(sedgpu, "context", lambda: gpu)
    rng = np.random.default_rng(400)
    query = "".join(rng.choice(list("ACGU"), size=28))
    docs = []
    for k in range(8):
        d = list(rng.choice(list("ACGU"), size=400))
        if k % 2 == 0:
            m = list(query)
            for _ in range(k // 2):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, 400 - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    hits = wfsearch.fit_search(query, docs, user_cost=True, scripts=True)
    assert [h[0] for h in hits] == docs
    for seq, score, start, end, es in hits:
        dist = 1 / score - 1
        want = fit_definition_str(table, query, seq)
        assert (pytest.approx(dist, abs=1e-9), start, end) == (want[0], want[1], want[2])
        assert SED.patching(es, query) == (0, seq[start:end])
        cost = 0.0
        for r in es:
            a, b = r["source"]["character"], r["destination"]["character"]
            cost += {"insert": table["insert"], "delete": table["delete"],
                     "update": 0 if a == b else table["update"][a][b]}[r["operation"]]
        assert cost == want[0]
    assert hits[0][1] == 1.0  # the exact copy
    assert wfsearch.fit_search(query, docs, user_cost=True, max_dist=0) == [hits[0][:4]]


# ---- the numeric envelope: every pair against the compiled definition, oracle.fit, exactly ----

def _packed(pats, texts, filler=0):
    """PackedPairs of the pairs, then `filler` more pairs of one 1-symbol pattern and one empty text, shared through
    their offsets."""
    pk = sedgpu.PackedPairs(pats, texts)
    if not filler:
        return pk
    n = pk.npairs
    return types.SimpleNamespace(
        npairs=n + filler, codes_a=pk.codes_a, codes_b=pk.codes_b,  # (the spare last byte of each is the filler's)
        off_a=np.concatenate([pk.off_a[:n], np.full(filler, len(pk.codes_a) - 1, np.int64)]),
        len_a=np.concatenate([pk.len_a[:n], np.ones(filler, np.int32)]),
        off_b=np.concatenate([pk.off_b[:n], np.full(filler, len(pk.codes_b) - 1, np.int64)]),
        len_b=np.concatenate([pk.len_b[:n], np.zeros(filler, np.int32)]))


def _check_oracle(gpu, plan, pats, texts, filler=0):
    """Run the pairs and compare every hit with oracle.fit, and every hit's distance with the oracle's G(start, end)."""
    gpu.set_costs(plan)
    pk = _packed(pats, texts, filler)
    dist, start, end = gpu.fit(pk)
    costs = oracle.Costs.from_plan(plan)
    wd, ws, we = oracle.fit(costs, pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b, pk.npairs, 8)
    bad = np.flatnonzero((dist != wd) | (start != ws) | (end != we))
    assert not len(bad), [(int(i), (dist[i], start[i], end[i]), (wd[i], ws[i], we[i])) for i in bad[:5]]
    n = len(pats)
    assert ((0 <= start) & (start <= end)).all() and (end[:n] <= [len(t) for t in texts]).all() and not end[n:].any()
    win = _packed(pats, [t[s:e] for t, s, e in zip(texts, start.tolist(), end.tolist())], filler)
    g = oracle.batch(costs, win.codes_a, win.off_a, win.len_a, win.codes_b, win.off_b, win.len_b, win.npairs, nthreads=8)[0]
    assert np.array_equal(g, dist)
    return list(zip(dist[:n].tolist(), start[:n].tolist(), end[:n].tolist()))


def _chunked(gpu, chunk, fn):
    try:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, chunk)
        return fn()
    finally:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)


@pytest.mark.parametrize("name", [n for n, _ in fit_envelope.cost_limit_tables()])
def test_cost_limits(gpu, name):
    """Scaled costs on the limits of the byte addend, the 16-bit distance field and the clamp: P in {1, 31, 32}, texts
    of 600..1500 (4 to 11 rebases a lane) with planted mutated copies, under the automatic chunk and a chunk of 255."""
    plan = dict(fit_envelope.cost_limit_tables())[name]
    rng = np.random.default_rng(600 + len(name))
    pats, texts = [], []
    for P in (1, 31, 32):
        for n in (600, 1001, 1500, int(rng.integers(600, 1501))):
            p = rng.integers(0, plan.K, size=P).astype(np.uint8)
            pats.append(p)
            texts.append(fit_envelope.planted_text(rng, plan.K, p, n))
    auto = _check_oracle(gpu, plan, pats, texts)
    assert _chunked(gpu, 255, lambda: _check_oracle(gpu, plan, pats, texts)) == auto


def test_widest_window(gpu):
    """insert 1, delete 254, P = 32: W = 8160.  One text of 30 000 under the automatic chunk and under a chunk of W."""
    plan = dict(fit_envelope.cost_limit_tables())["i1_d254"]
    rng = np.random.default_rng(8160)
    p = rng.integers(0, plan.K, size=32).astype(np.uint8)
    t = fit_envelope.planted_text(rng, plan.K, p, 30000, copies=8)
    got = sedgpu.fit_plan(plan.costs(), {}, [32], [30000])
    assert got["W"] == 8160 and got["lanes"] > 1
    auto = _check_oracle(gpu, plan, [p], [t])
    assert _chunked(gpu, 8160, lambda: _check_oracle(gpu, plan, [p], [t])) == auto


def _unit(K=4, sub=2.0):
    return np.where(np.eye(K) > 0, 0.0, sub)


def test_zero_insert(gpu):
    """insert = 0 runs one lane per text whatever the chunk option says: texts of 0, 1, around one rebase, and 65 534
    symbols, the longest lane there is."""
    plan = fit_envelope.Plan(_unit(), 0, 1.5)
    rng = np.random.default_rng(65534)
    pats, texts = [], []
    for n in (0, 1, 127, 128, 129, 65534):
        for P in (1, 31, 32):
            p = rng.integers(0, 4, size=P).astype(np.uint8)
            pats.append(p)
            texts.append(fit_envelope.planted_text(rng, 4, p[:n], n) if n else np.zeros(0, np.uint8))
    lens = ([len(p) for p in pats], [len(t) for t in texts])
    for opts in ({}, {sedgpu.SED_OPT_FIT_CHUNK: 64}):
        assert sedgpu.fit_plan(plan.costs(), opts, *lens)["lanes"] == len(pats)
    auto = _check_oracle(gpu, plan, pats, texts)
    assert _chunked(gpu, 64, lambda: _check_oracle(gpu, plan, pats, texts)) == auto


def test_span_refusal(gpu):
    plan = fit_envelope.Plan(_unit(), 0, 1.5)
    rng = np.random.default_rng(65535)
    p = rng.integers(0, 4, size=7).astype(np.uint8)
    gpu.set_costs(plan)
    with pytest.raises(sedgpu.SedError, match=r"\(-4\).*span"):
        gpu.fit(sedgpu.PackedPairs([p], [rng.integers(0, 4, size=65535).astype(np.uint8)]))
    _check_oracle(gpu, plan, [p] * 2, [fit_envelope.planted_text(rng, 4, p, 500), rng.integers(0, 4, size=65534).astype(np.uint8)])


def test_zero_delete(gpu):
    """delete = 0: deleting the whole pattern is free, so every hit is (0, 0, 0)."""
    rng = np.random.default_rng(255)
    for plan in (fit_envelope.Plan(_unit(), 1.25, 0), dict(fit_envelope.cost_limit_tables())["i255_d0"]):
        pats, texts = _fuzz_pairs(rng, plan.K, 60)
        got = _check_oracle(gpu, plan, pats, texts)
        assert got == [(0.0, 0, 0)] * len(pats)


@pytest.mark.parametrize("K", [6, 7, 8])
def test_all_eight_symbols(gpu, K):
    """Symbols 4..7 select the second addend word (chi): a table whose rows differ in every column."""
    rng = np.random.default_rng(800 + K)
    plan = fit_envelope.eight_symbol_table(K)
    pats, texts = _fuzz_pairs(rng, K, 200)
    assert set(np.concatenate(pats).tolist()) == set(range(K)) == set(np.concatenate(texts).tolist())
    _check_oracle(gpu, plan, pats, texts)


def test_long_texts(gpu):
    """Texts of 65 534 (the largest unsplit lane), 65 535 (the first that must split), 65 536, 70 001 and 200 000
    symbols in a batch large enough that the automatic rule keeps one lane per text, so only the span limit splits
    them: exact and 3-edit copies end one column before, at and one after every forced seam and at the end of the
    200 000 text, where end needs more than 16 bits."""
    plan = fit_envelope.Plan(_unit(), 1, 4)
    rng = np.random.default_rng(200000)
    filler = 1 << 17
    lens = (65534, 65535, 65536, 70001, 200000)
    got = sedgpu.fit_plan(plan.costs(), {}, [32] * len(lens) + [1] * filler, list(lens) + [0] * filler)
    chunk = got["chunk"]
    # (the chunk is the batch's: 65 534 runs as one lane only in a batch without longer texts, below)
    assert got["W"] == 160 and chunk == 65535 - 160 - 3 and got["lanes"] == filler + 2 + 2 + 2 + 2 + 4
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    pats, texts = [], []
    for n in lens:
        ends = [e for seam in range(chunk, n + 1, chunk) for e in (seam - 1, seam, seam + 1)]
        ends += [n] if n < 70000 else [n - 1, n]
        for end in ends:
            for edits in (0, 3):
                t = rng.integers(0, 4, size=n).astype(np.uint8)
                m = p if edits == 0 else _mutate(rng, p, 4, 3)
                t[end - len(m):end] = m
                pats.append(p)
                texts.append(t)
    hits = _check_oracle(gpu, plan, pats, texts, filler)
    assert sum(d == 0 for d, _, _ in hits) >= len(hits) // 2  # (the exact copies were found)
    assert max(e for _, _, e in hits) > 0x20000
    gpu.set_costs(plan)
    try:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 1 << 20)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*span"):
            gpu.fit(_packed(pats, texts, filler))
    finally:
        gpu.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)
    assert _check_oracle(gpu, plan, pats[-2:], texts[-2:]) == hits[-2:]
    alone = sedgpu.fit_plan(plan.costs(), {}, [32, 32] + [1] * filler, [65534, 65534] + [0] * filler)
    assert alone["chunk"] == 0 and alone["lanes"] == filler + 2  # one lane of 65 535 columns each
    assert _check_oracle(gpu, plan, pats[:2], texts[:2], filler) == hits[:2]


def test_auto_chunk_above_window(gpu):
    """512 texts of 20 000, unit costs, P <= 8: the automatic rule picks a chunk longer than W."""
    plan = fit_envelope.Plan(_unit(sub=1.0), 1, 1)
    rng = np.random.default_rng(512)
    pats = [rng.integers(0, 4, size=int(rng.integers(1, 9))).astype(np.uint8) for _ in range(512)]
    texts = [rng.integers(0, 4, size=20000).astype(np.uint8) for _ in range(512)]
    got = sedgpu.fit_plan(plan.costs(), {}, [len(p) for p in pats], [20000] * 512)
    assert got["chunk"] > got["W"] > 0 and got["lanes"] > 512
    _check_oracle(gpu, plan, pats, texts)


def test_buffer_reuse(gpu):
    """A large search, a one-pair search, the large one again, on one context: the device buffers are kept across
    calls, and each search must read only its own."""
    plan = _golden_plan("user_costs.json", "ACGU")
    rng = np.random.default_rng(77)
    pats = [rng.integers(0, 4, size=int(rng.integers(1, 33))).astype(np.uint8) for _ in range(300)]
    texts = [fit_envelope.planted_text(rng, 4, p, int(rng.integers(2000, 4000))) for p in pats]
    big = _check_oracle(gpu, plan, pats, texts)
    one = _check_oracle(gpu, plan, [pats[-1]], [texts[-1][:50]])
    assert _check_oracle(gpu, plan, pats, texts) == big
    assert _check_oracle(gpu, plan, [pats[-1]], [texts[-1][:50]]) == one
