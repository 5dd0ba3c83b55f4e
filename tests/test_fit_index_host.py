"""CPU: the host side of fit search over a resident index (sed_fit_index_search).  The lane records the
index kernel derives (sed_fit_index_lanes: the chunk table and the shared derivation) against the existing lane
builder (sed_fit_lanes) on the materialised cross product, the index plan against sed_fit_plan of that cross product,
the ABI, and wfsearch.FitIndex with oracle.fit standing in for the device."""
import numpy as np
import pytest

from conftest import load_golden
import oracle
import sedgpu
from test_fit_host import costs_of, unit_costs, wfsearch  # noqa: F401  (wfsearch: a fixture)

E_ARG, E_RANGE = -1, -4
TEXT_LENS = [0, 1, 3, 4, 5, 299, 70000]
QUERY_SETS = [[1], [31], [32], [1, 31, 32], [32, 1, 7], [5, 31, 2]]
PLAN_FIELDS = ("scale", "W", "chunk", "lanes", "cells")


def cross(len_p, len_t):
    """The lengths of the materialised cross product, query-major: pair q * len(len_t) + d."""
    return [p for p in len_p for _ in len_t], [n for _ in len_p for n in len_t]


def _cost_models():
    return [("costs.json", costs_of(load_golden("costs.json"), "ACGU")),
            ("user_costs.json", costs_of(load_golden("user_costs.json"), "ACGU")),
            ("costs.json+N", costs_of(load_golden("costs.json"), "ACGUN"))]


@pytest.mark.parametrize("name", [n for n, _ in _cost_models()])
@pytest.mark.parametrize("chunk", [0, 4, 8, 72, 70001, 1 << 20])
def test_lane_records_equal_the_lane_builder(name, chunk):
    """Every field but pat (0 in both) and the 18 parameter words, for every query set: forced chunks 4, 8 and 72, the
    automatic chunk (which must split the 70 000 text), and chunks of at least every length + 1 (refused here, as for
    the cross product: a 70 001-column lane is beyond the span; served without the long text)."""
    costs = dict(_cost_models())[name]
    for lp in QUERY_SETS:
        for lt in (TEXT_LENS, TEXT_LENS[:-1]):
            opts = {sedgpu.SED_OPT_FIT_CHUNK: chunk}
            xp, xt = cross(lp, lt)
            if chunk > 65535 and lt[-1] == 70000:
                for fn, args in ((sedgpu.fit_lanes, (xp, xt)), (sedgpu.fit_index_lanes, (lp, lt))):
                    with pytest.raises(sedgpu.SedError) as ex:
                        fn(costs, opts, *args)
                    assert ex.value.code == E_RANGE
                continue
            plan = sedgpu.fit_index_plan(costs, opts, lp, lt)
            # the builder under the index plan's chunk (the automatic rule: the chunk it chose)
            want, wpar = sedgpu.fit_lanes(costs, {sedgpu.SED_OPT_FIT_CHUNK: plan["chunk"]} if plan["chunk"] else opts, xp, xt)
            got, gpar = sedgpu.fit_index_lanes(costs, opts, lp, lt)
            for f in sedgpu.FIT_LANE_FIELDS:
                assert np.array_equal(got[f], want[f]), (lp, len(lt), f)
            assert np.array_equal(gpar["row"], wpar["row"]) and (gpar["ins"], gpar["del"]) == (wpar["ins"], wpar["del"])
            assert len(got["pair"]) == plan["lanes"]
            if chunk == 0 and lt[-1] == 70000:
                assert (got["pair"] == len(lt) - 1).sum() > 1  # the long text was split
            if chunk in (0, 1 << 20) and lt[-1] != 70000 and chunk:
                assert plan["lanes"] == len(lp) * len(lt)  # one lane per (query, text)


def test_insert_zero_is_one_chunk_per_text():
    costs = unit_costs(4, 0, 1.5)
    lt = [0, 1, 3, 4, 5, 299, 65534]
    for opts in ({}, {sedgpu.SED_OPT_FIT_CHUNK: 8}):
        for lp in QUERY_SETS:
            xp, xt = cross(lp, lt)
            want, wpar = sedgpu.fit_lanes(costs, opts, xp, xt)
            got, gpar = sedgpu.fit_index_lanes(costs, opts, lp, lt)
            assert len(got["pair"]) == len(lp) * len(lt)
            for f in sedgpu.FIT_LANE_FIELDS:
                assert np.array_equal(got[f], want[f]), (lp, f)
            assert np.array_equal(gpar["row"], wpar["row"])
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.fit_index_plan(costs, {}, [5], lt + [65535])
    assert ex.value.code == E_RANGE


def _both_plans(costs, opts, lp, lt):
    """(index plan | error code, cross-product plan | error code)."""
    out = []
    for fn, args in ((sedgpu.fit_index_plan, (lp, lt)), (sedgpu.fit_plan, cross(lp, lt))):
        try:
            out.append(fn(costs, opts, *args))
        except sedgpu.SedError as ex:
            out.append(ex.code)
    return out


def test_plan_equals_the_cross_products():
    rng = np.random.default_rng(36)
    user = costs_of(load_golden("user_costs.json"), "ACGU")
    cases = [(user, {}, [28], [4096] * 8192),               # DESIGN 3.6e's workload
             (user, {}, [28] * 64, [4096] * 8192),          # enough pairs that one lane per text is kept
             (user, {}, [3, 32, 9], [4096] * 300),          # W from the longest query
             (unit_costs(4, 1, 1), {}, [28] * 3, [30] * 70000),
             (unit_costs(4, 1, 4), {}, [32, 1], [65534, 65535, 70001, 200000, 0]),
             (unit_costs(4, 1, 4), {}, [32], [65534] * 2),
             (unit_costs(4, 1, 1), {}, [], [5, 6]), (unit_costs(4, 1, 1), {}, [5, 6], []),
             (unit_costs(4, 1, 1), {}, [], [])]
    for c in (1, 7, 64, 65, 200, 5000):
        lt = rng.integers(0, 900, size=40).tolist() + [0, 1, 63, 64, 65]
        cases.append((costs_of(load_golden("costs.json"), "ACGUN"), {sedgpu.SED_OPT_FIT_CHUNK: c},
                      rng.integers(1, 33, size=5).tolist(), lt))
    for costs, opts, lp, lt in cases:
        got, want = _both_plans(costs, opts, lp, lt)
        assert isinstance(want, dict), (lp[:3], lt[:3])
        assert got == want, (opts, lp[:3], lt[:3])  # (every field: nominal cells too)
        assert all(got[f] == want[f] for f in PLAN_FIELDS)


def test_every_refusal_of_the_plan_is_reproduced():
    t66 = load_golden("costs.json")
    u = unit_costs(4, 1, 1)
    cases = [(costs_of(t66, "ARD"), {}, [5], [10], E_RANGE),                   # 0.66: not dyadic
             (unit_costs(9, 1, 1), {}, [5], [10], E_RANGE),                    # 9 symbols
             (u, {}, [33], [10], E_RANGE), (u, {}, [4, 33], [10, 10], E_RANGE), (u, {}, [0], [10], E_RANGE),
             (unit_costs(4, 1, 3000), {}, [32], [10], E_RANGE),                # P * delete * S > 65535
             (unit_costs(4, 1, 2100.25), {}, [32], [10], E_RANGE),
             (unit_costs(4, 1, 300), {}, [3], [10], E_RANGE),                  # delete * S > 255
             (unit_costs(4, 100, 200), {}, [3], [10], E_RANGE),                # (insert + delete) * S > 255
             (u, {}, [5], [-1], E_ARG), (u, {}, [5, 6], [3, -1], E_ARG),
             (u, {}, [33, 5], [3, -1], E_RANGE),                               # pair 0's pattern before pair 1's text
             (u, {}, [5, 33], [3, -1], E_ARG),                                 # pair 1's text before pair 2's pattern
             (u, {}, [33], [-1, 4], E_ARG),                                    # pair 0's text before its pattern
             (unit_costs(9, 1, 1), {}, [5], [-1], E_RANGE),                    # (the symbol count comes first)
             (unit_costs(4, 0, 1), {}, [5], [65535], E_RANGE),                 # insert = 0: one chunk, n <= 65534
             (u, {sedgpu.SED_OPT_FIT_CHUNK: 1 << 20}, [5], [3, 70000], E_RANGE),
             (u, {sedgpu.SED_OPT_FIT_CHUNK: 65530}, [5], [3, 70000], E_RANGE),  # chunk + W + 3 beyond the span
             (u, {sedgpu.SED_OPT_FIT_CHUNK: 1}, [28] * 40000, [4096] * 20, E_RANGE)]  # more than 2^31 lanes
    for costs, opts, lp, lt, code in cases:
        got, want = _both_plans(costs, opts, lp, lt)
        assert want == code, (opts, lp[:3], lt[:3], want)
        assert got == code, (opts, lp[:3], lt[:3], got)
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.fit_index_lanes(unit_costs(9, 1, 1), {}, [5], [10])
    assert ex.value.code == E_RANGE


def test_abi_symbols_are_exported_and_bound():
    lib = sedgpu.load()
    names = {n for n, _, _ in sedgpu.SIGNATURES}
    for sym in ("sed_fit_index_create", "sed_fit_index_destroy", "sed_fit_index_search", "sed_fit_index_last_time",
                "sed_fit_index_texts", "sed_fit_index_symbols", "sed_fit_index_plan", "sed_fit_index_lanes"):
        assert sym in names and getattr(lib, sym).argtypes is not None
    for attr in ("fit_index",):
        assert callable(getattr(sedgpu.Context, attr)) and callable(getattr(sedgpu.EngineClient, attr))
    assert all(callable(getattr(sedgpu.FitIndex, a)) for a in ("search", "last_ms", "close"))
    with pytest.raises(sedgpu.SedError, match="does not serve resident indexes"):
        sedgpu.EngineClient.fit_index(object.__new__(sedgpu.EngineClient), np.zeros(1, np.uint8), [0], [1])


# ---- wfsearch.FitIndex with oracle.fit standing in for the device ----

class OracleEngine:
    """StringEditDistance.FitIndex's device half on the CPU: every query against every text through oracle.fit."""

    opened = 0

    def __init__(self, codes, off, lens):
        type(self).opened += 1
        self.codes, self.off, self.lens = np.concatenate([codes, np.zeros(1, np.uint8)]), off, lens
        self.K = []

    def search(self, plan, packed):
        Q, D = packed.npairs, len(self.lens)
        self.K.append(plan.K)
        qi, di = np.divmod(np.arange(Q * D), max(D, 1))
        d, s, e = oracle.fit(oracle.Costs.from_plan(plan), packed.codes_a, packed.off_a[qi].copy(), packed.len_a[qi].copy(),
                             self.codes, self.off[di].copy(), self.lens[di].copy(), Q * D, 1)
        return d.reshape(Q, D), s.reshape(Q, D), e.reshape(Q, D)

    def close(self):
        pass


def _oracle_fit_fn(SED):
    def fit_fn(patterns, texts, user_cost):
        plan = SED.batch_plan(patterns, texts, user_cost)
        pk = sedgpu.PackedPairs([plan.encode(p) for p in patterns], [plan.encode(t) for t in texts])
        d, s, e = oracle.fit(oracle.Costs.from_plan(plan), pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b,
                             pk.npairs, 1)
        return list(zip(d.tolist(), s.tolist(), e.tolist()))
    return fit_fn


def _docs(rng, query, count=12, n=120):
    docs = []
    for k in range(count):
        d = list(rng.choice(list("ACGU"), size=n if k else 0))  # (the first document is empty)
        if k % 2:
            m = list(query)
            for _ in range(k // 2):
                m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
            at = int(rng.integers(0, n - len(m)))
            d[at:at + len(m)] = m
        docs.append("".join(d))
    return docs


@pytest.fixture()
def index_fn(wfsearch, monkeypatch):
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    return lambda texts, user_cost: SED.fit_index(texts, user_cost, engine=OracleEngine)


@pytest.mark.parametrize("user_cost", [False, True])
def test_wfsearch_fit_index_equals_fit_search(wfsearch, index_fn, user_cost):
    rng = np.random.default_rng(28)
    query = "".join(rng.choice(list("ACGU"), size=28))
    docs = _docs(rng, query)
    fit_fn = _oracle_fit_fn(wfsearch.SED)
    ix = wfsearch.FitIndex(docs, user_cost, index_fn=index_fn)
    want = wfsearch.fit_search(query, docs, user_cost, fit_fn=fit_fn)
    assert ix.search(query) == want and len(want) == len(docs)
    assert want[1][1] == 1.0 and want[0][2:] == (0, 0)  # the exact copy; the empty document
    for max_dist in (0, 2, 4.5, 1000):
        kept = wfsearch.fit_search(query, docs, user_cost, max_dist=max_dist, fit_fn=fit_fn)
        assert ix.search(query, max_dist=max_dist) == kept
    assert 0 < len(wfsearch.fit_search(query, docs, user_cost, max_dist=2, fit_fn=fit_fn)) < len(docs)
    queries = [query, query[:1], query[3:], "ACGU" * 8]
    opened = OracleEngine.opened
    many = ix.search_many(queries, max_dist=6)
    assert many == [ix.search(q, max_dist=6) for q in queries]
    assert many == [wfsearch.fit_search(q, docs, user_cost, max_dist=6, fit_fn=fit_fn) for q in queries]
    assert OracleEngine.opened == opened  # (the texts were encoded and handed over once)
    assert ix.search_many([]) == [] and wfsearch.FitIndex([], user_cost, index_fn=index_fn).search(query) == []
    ix.close()
    ix.close()


def test_wfsearch_fit_index_alphabet_grows_and_stops_at_eight(wfsearch, index_fn):
    docs = ["ACGUACGGAU", "GGAUC", ""]
    fit_fn = _oracle_fit_fn(wfsearch.SED)
    ix = wfsearch.FitIndex(docs, False, index_fn=index_fn)
    dev = ix._ix._dev
    assert ix._ix.symbols == list("ACGU")
    assert ix.search("GGAU") == wfsearch.fit_search("GGAU", docs, fit_fn=fit_fn) and dev.K[-1] == 4
    # N is no symbol of the texts: it joins the alphabet at its end for that search only
    assert ix.search("GGNAU") == wfsearch.fit_search("GGNAU", docs, fit_fn=fit_fn) and dev.K[-1] == 5
    assert ix.search("GGAU") == wfsearch.fit_search("GGAU", docs, fit_fn=fit_fn) and dev.K[-1] == 4
    assert ix._ix.symbols == list("ACGU")
    assert ix.search_many(["RYKM", "GA"]) == [wfsearch.fit_search(q, docs, fit_fn=fit_fn) for q in ("RYKM", "GA")]
    assert dev.K[-1] == 8
    searches = len(dev.K)
    with pytest.raises(sedgpu.SedError, match="9 symbols"):
        ix.search("RYKMS")  # the ninth symbol
    with pytest.raises(KeyError):
        ix.search("AXG")  # no row of the cost table: the reference's KeyError, as fit_batch raises it
    with pytest.raises(KeyError):
        wfsearch.fit_search("AXG", docs, fit_fn=fit_fn)
    assert len(dev.K) == searches  # (neither reached the device)
    assert ix.search("GGAU") == wfsearch.fit_search("GGAU", docs, fit_fn=fit_fn)
