"""CPU: the planner of long fit search (sed_fit_index_long_plan, sed_fit_index_long_lanes) - its
refusals, the rows-per-lane rule and grouping, the chunk rule, its records - the refusal of P = 33 by the existing calls,
and wfsearch's long_patterns over an index_fn engine built on oracle.fit."""
import math

import numpy as np
import pytest

import sedgpu
from fit_envelope import Plan
from test_fit_hits_host import DefinitionEngine, _fake_scripts, hits_row, index_fn, wfsearch  # noqa: F401  (fixtures)

E_ARG, E_RANGE = -1, -4
CHUNK, ROWS = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS
UNIT = np.where(np.eye(4) > 0, 0.0, 2.0)


def plan_of(plan, len_p, len_t, options=None):
    return sedgpu.FitIndex.long_plan(plan.costs(), options or {}, len_p, len_t)


def code_of(plan, len_p, len_t, options=None):
    try:
        plan_of(plan, len_p, len_t, options)
    except sedgpu.SedError as e:
        return e.code
    return 0


def test_abi():
    names = {n for n, _, _ in sedgpu.SIGNATURES}
    assert {"sed_fit_index_search_long", "sed_fit_index_hits_long", "sed_fit_index_long_plan", "sed_fit_index_long_lanes"} <= names
    assert all(callable(getattr(sedgpu.FitIndex, a)) for a in ("search_long", "hits_long", "long_plan", "long_lanes"))
    assert not hasattr(sedgpu.EngineClient, "search_long")  # the forked child's proxy serves no index
    assert sedgpu.SED_OPT_FIT_ROWS == 19


def test_refusals():
    p = Plan(UNIT, 1, 1)
    assert code_of(p, [0], [10]) == E_RANGE and code_of(p, [2049], [10]) == E_RANGE
    assert code_of(p, [2048], [10]) == 0 and code_of(p, [1], [10]) == 0
    # more than 8 symbols, non-dyadic costs, (insert + delete) S > 255
    assert code_of(Plan(np.zeros((9, 9)), 1, 1), [5], [10]) == E_RANGE
    assert code_of(Plan(UNIT, 1 / 3, 1), [5], [10]) == E_RANGE
    assert code_of(Plan(UNIT, 128, 128), [5], [10]) == E_RANGE and code_of(Plan(UNIT, 127, 128), [5], [10]) == 0
    # the D field: P delete S + 128 insert S <= 65535
    for ins, dele, P in ((0, 255, 257), (3, 252, 258), (15, 31, 2048), (255, 0, 2048)):
        assert P * dele + 128 * ins <= 65535
        assert code_of(Plan(np.where(np.eye(4) > 0, 0.0, 255.0), ins, dele), [P], [100]) == 0, (ins, dele, P)
    for ins, dele, P in ((0, 255, 258), (3, 252, 259), (16, 31, 2048), (1, 32, 2048)):
        assert P * dele + 128 * ins > 65535
        assert code_of(Plan(np.where(np.eye(4) > 0, 0.0, 255.0), ins, dele), [P], [100]) == E_RANGE, (ins, dele, P)
    # (a quarter-unit table: the condition is on the scaled costs)
    assert code_of(Plan(UNIT, 0.25, 8), [2043], [100]) == 0 and code_of(Plan(UNIT, 0.25, 8), [2044], [100]) == E_RANGE
    # the span: chunk + W + 3 <= 65535 columns a wave (the 3: a wave's first column is aligned to a 4-symbol word)
    W = plan_of(p, [100], [70000])["W"]
    assert W == 200
    assert code_of(p, [100], [70000], {CHUNK: 65535 - W - 3}) == 0
    assert code_of(p, [100], [70000], {CHUNK: 65535 - W - 2}) == E_RANGE
    assert plan_of(p, [100], [70000])["chunk"] + W + 3 <= 65535
    # insert = 0: one chunk per text, texts over 65534 refused
    z = Plan(UNIT, 0, 1)
    assert plan_of(z, [100], [65534, 5])["lanes"] == 2 and code_of(z, [100], [65535]) == E_RANGE
    # a forced R too small for a P
    assert code_of(p, [128, 129], [10], {ROWS: 2}) == E_RANGE and code_of(p, [128, 129], [10], {ROWS: 4}) == 0
    with pytest.raises(sedgpu.SedError):
        plan_of(p, [10], [10], {ROWS: 3})
    # bad arguments
    assert code_of(p, [10], [-1]) == E_ARG


def test_rows_rule_and_grouping():
    p = Plan(UNIT, 1, 1)
    lens = [1, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
    want = [2, 2, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert plan_of(p, lens, [50])["rows"].tolist() == want
    mixed = [700, 5, 130, 2000, 64, 129]
    assert plan_of(p, mixed, [50, 60])["rows"].tolist() == [16, 2, 4, 32, 2, 4]
    assert plan_of(p, mixed, [50, 60], {ROWS: 32})["rows"].tolist() == [32] * 6
    # the records come in query order whatever the grouping
    lanes, _ = sedgpu.FitIndex.long_lanes(p.costs(), {}, mixed, [50, 60])
    assert lanes["pair"].tolist() == list(range(12)) and lanes["plen"].tolist() == [P for P in mixed for _ in range(2)]
    # the options of the long calls are no options of a batch
    with pytest.raises(sedgpu.SedError):
        sedgpu.plan_routes(p.costs(), {ROWS: 2}, sedgpu.PackedPairs([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)]), 0)


def test_chunk_rule():
    """One chunk per text when the pairs alone give 2 waves on each of the 1024 SIMDs; else the chunk that gives 4, a
    multiple of 4, never below W."""
    p = Plan(UNIT, 1, 1)
    assert plan_of(p, [76] * 2, [4096] * 1024)["chunk"] == 0           # 2048 waves
    got = plan_of(p, [76], [4096] * 2047)                             # 2047 waves: split
    cols = 2047 * 4097
    assert got["W"] == 152 and got["chunk"] == max((math.ceil(cols / 4096) + 3) // 4 * 4, 152) == 2048
    assert got["lanes"] == 2047 * 3
    got = plan_of(p, [1024], [4096] * 8)
    assert got["W"] == 2048 and got["chunk"] == 2048                  # never below W
    got = plan_of(p, [40], [100000] * 100)
    assert got["chunk"] == (math.ceil(100 * 100001 / 4096) + 3) // 4 * 4 and got["chunk"] % 4 == 0
    assert plan_of(p, [40], [1000], {CHUNK: 72})["chunk"] == 72
    # the short plan counts lanes where this one counts waves
    assert sedgpu.fit_index_plan(p.costs(), {}, [20], [4096] * 2047)["chunk"] < 2048


def test_records_equal_the_short_plans():
    """For P <= 32 and the same chunk the wave records are sed_fit_index_lanes' lane records, word for word."""
    p = Plan(UNIT, 1, 1.5)
    len_p, len_t = [1, 31, 32], [0, 1, 64, 333, 1000]
    for chunk in (8, 72, 1 << 20):
        a, pa = sedgpu.fit_index_lanes(p.costs(), {CHUNK: chunk}, len_p, len_t)
        b, pb = sedgpu.FitIndex.long_lanes(p.costs(), {CHUNK: chunk}, len_p, len_t)
        assert all((a[k] == b[k]).all() for k in sedgpu.FIT_LANE_FIELDS)
        assert (pa["row"] == pb["row"]).all() and (pa["ins"], pa["del"]) == (pb["ins"], pb["del"])
    # and for longer patterns they are what the short derivation gives for the long plan's chunk and W
    b, _ = sedgpu.FitIndex.long_lanes(p.costs(), {CHUNK: 100}, [200], [1000])
    W = plan_of(p, [200], [1000], {CHUNK: 100})["W"]
    assert W == 500 and b["c0"].tolist() == list(range(0, 1001, 100))
    assert b["lead"].tolist() == [c0 - (0 if c0 <= W else (c0 - W) & ~3) for c0 in b["c0"].tolist()]
    assert (b["nsteps"] == b["lead"] + b["cnt"] - 1).all() and b["cnt"].sum() == 1001


def test_existing_calls_still_refuse_33():
    p = Plan(UNIT, 1, 1)
    for fn in (sedgpu.fit_plan, sedgpu.fit_lanes):
        with pytest.raises(sedgpu.SedError) as e:
            fn(p.costs(), {}, [33], [100])
        assert e.value.code == E_RANGE
    for fn in (sedgpu.fit_index_plan, sedgpu.fit_index_lanes):
        with pytest.raises(sedgpu.SedError) as e:
            fn(p.costs(), {}, [32, 33], [100])
        assert e.value.code == E_RANGE
    # (they do not read the option)
    assert sedgpu.fit_index_plan(p.costs(), {ROWS: 8}, [32], [100]) == sedgpu.fit_index_plan(p.costs(), {}, [32], [100])


class LongDefinitionEngine(DefinitionEngine):
    """DefinitionEngine with the long calls: oracle.fit and the restated rows have no length in them."""

    def __init__(self, codes, off, lens):
        super().__init__(codes, off, lens)
        self.log = []

    def search(self, plan, packed):
        self.log.append(("search", packed.len_a.tolist()))
        return super().search(plan, packed)

    def hits(self, plan, packed, max_dist):
        self.log.append(("hits", packed.len_a.tolist()))
        return super().hits(plan, packed, max_dist)

    def search_long(self, plan, packed):
        self.log.append(("search_long", packed.len_a.tolist()))
        return DefinitionEngine.search(self, plan, packed)

    def hits_long(self, plan, packed, max_dist):
        self.log.append(("hits_long", packed.len_a.tolist()))
        return DefinitionEngine.hits(self, plan, packed, max_dist)


def test_wfsearch_long_patterns(wfsearch, monkeypatch):
    from conftest import load_golden
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    rng = np.random.default_rng(76)
    query = "".join(rng.choice(list("ACGU"), size=76))
    docs = ["", query]
    for k in range(2, 8):
        d = list(rng.choice(list("ACGU"), size=200))
        m = list(query)
        for _ in range(k % 3):
            m[int(rng.integers(0, len(m)))] = str(rng.choice(list("ACGU")))
        at = int(rng.integers(0, len(d) - len(m)))
        d[at:at + len(m)] = m
        docs.append("".join(d))
    ix = wfsearch.FitIndex(docs, True, index_fn=lambda t, uc: SED.fit_index(t, uc, engine=LongDefinitionEngine))
    dev = ix._ix._dev
    plan = SED.batch_plan([query], ["ACGU"], True)

    def want(q, T):
        out = []
        for doc in docs:
            row = hits_row(plan.sub.tolist(), plan.ins, plan.dele, plan.encode(q).tolist(), plan.encode(doc).tolist())
            ends = [e for e, (d, _) in enumerate(row) if d <= T and d < (row[e - 1][0] if e else math.inf)
                    and d <= (row[e + 1][0] if e < len(doc) else math.inf)]
            out += [(doc, 1 / (1 + row[e][0]), row[e][1], e) for e in ends]
        return out

    queries = [query[:20], query, query[40:], query[:33], query + query[:10]]
    # the default keeps today's calls: every query goes to hits(), whose engine refuses the long ones
    ix.occurrences_many(queries, 6)
    assert dev.log == [("hits", [20, 76, 36, 33, 86])]
    del dev.log[:]
    many = ix.occurrences_many(queries, 6, long_patterns=True)
    assert dev.log == [("hits", [20]), ("hits_long", [76, 36, 33, 86])]
    assert many == [want(q, 6) for q in queries] and any(many[1]) and any(many[0])
    assert ix.occurrences(query, 6, long_patterns=True) == many[1]
    assert (docs[1], 1.0, 0, 76) in many[1]
    del dev.log[:]
    best = ix.search_many(queries, long_patterns=True)
    assert dev.log == [("search", [20]), ("search_long", [76, 36, 33, 86])]
    assert best == [ix.search(q, long_patterns=True) for q in queries]
    for q, hits in zip(queries, best):
        for (s, sc, a, b), doc in zip(hits, docs):
            assert s == doc and (not want(q, math.inf) or (s, sc, a, b) in ix.occurrences(q, math.inf, long_patterns=True))
    # scripts: one edit_script_batch call for every returned tuple, of (query, sequence[start:end]), in merge order
    batches = _fake_scripts(monkeypatch, SED)
    withes = ix.occurrences_many(queries, 6, scripts=True, long_patterns=True)
    assert batches == [sum(len(m) for m in many)]
    for q, got, plain in zip(queries, withes, many):
        assert [g[:4] for g in got] == plain and all(g[4] == ("es", q, g[0][g[2]:g[3]]) for g in got)
    assert wfsearch.fit_occurrences(query, docs, 6, True, long_patterns=True,
                                    index_fn=lambda t, uc: SED.fit_index(t, uc, engine=LongDefinitionEngine)) == many[1]
    ix.close()
