"""CPU: the host side of the fp64 route for long patterns (sed_fit_index_search_long_f64): the planner's
envelope, rows, window and records, sed_fit_long_route, the step-by-step model of the kernel's wave
(fit_long_f64_cases.run_waves) over the planner's own records, equal to oracle.fit and to the last-row reference to the
bit, and wfsearch's route keyword over the long queries of an index_fn engine built on the definition."""
import ctypes
import math

import numpy as np
import pytest

import oracle  # noqa: F401
import sedgpu
import fit_f64_cases as fc
import fit_long_f64_cases as lc
from test_fit_host import unit_costs
from test_fit_hits_host import DefinitionEngine, _fake_scripts, wfsearch  # noqa: F401  (fixtures)
from conftest import load_golden

E_ARG, E_RANGE = -1, -4
CHUNK, ROWS = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS
TABLES = {"rounding": fc.rounding_table(), "costs15": fc.golden15("costs.json")}


def test_abi_exports_and_binds_the_new_calls(wfsearch):
    names = {"sed_fit_index_search_long_f64", "sed_fit_index_hits_long_f64", "sed_fit_index_long_f64_plan",
             "sed_fit_index_long_f64_lanes", "sed_fit_long_route"}
    lib = ctypes.CDLL(sedgpu.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert names <= {n for n, _, _ in sedgpu.SIGNATURES}
    assert all(callable(getattr(sedgpu.FitIndex, a)) for a in ("search_long_f64", "hits_long_f64"))
    assert all(callable(getattr(sedgpu, a)) for a in ("fit_index_long_f64_plan", "fit_index_long_f64_lanes", "fit_long_route"))
    assert all(callable(getattr(wfsearch.SED.FitIndex, a)) for a in ("search_long_f64", "hits_long_f64"))


def _refusal(costs, len_p, len_t, options=None):
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.fit_index_long_f64_plan(costs, options or {}, len_p, len_t)
    return ex.value.code


def test_refusals_name_the_bound_or_the_cost():
    ok = fc.unit(4)
    for costs, lp, words in ((unit_costs(17, 1, 1), [40], "17 symbols (at most 16)"),
                             (unit_costs(4, -1.0, 1), [40], "insert = -1 is not a finite cost >= 0"),
                             (ok.costs(), [0], "pattern length 0 outside 1..2048"),
                             (ok.costs(), [40, 2049], "pattern length 2049 outside 1..2048")):
        assert _refusal(costs, lp, [10]) == E_RANGE
        with pytest.raises(sedgpu.SedError):
            sedgpu.fit_index_long_f64_lanes(costs, {}, lp, [10])
        route, why = sedgpu.fit_long_route(costs, {}, lp, [10])
        assert route is None and words in why.split("; ")[1], why
    neg = fc.unit(4)
    neg.sub[1, 2] = -0.5
    assert "cost(1 -> 2) = -0.5" in sedgpu.fit_long_route(neg.costs(), {}, [40], [10])[1]
    assert sedgpu.fit_index_long_f64_plan(ok.costs(), {}, [2048, 1], [10])["rows"].tolist() == [32, 2]
    assert _refusal(ok.costs(), [128, 129], [10], {ROWS: 2}) == E_RANGE
    assert _refusal(ok.costs(), [10], [-1]) == E_ARG


def test_rows_window_and_one_wave_rule():
    r = TABLES["rounding"]  # P delete / insert = 2 P exactly: W = P + 2 P + 2
    lens = [1, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
    got = sedgpu.fit_index_long_f64_plan(r.costs(), {}, lens, [50])
    assert got["rows"].tolist() == [2, 2, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32] and got["W"] == 3 * 2048 + 2 and got["scale"] == 0
    assert sedgpu.fit_index_long_f64_plan(r.costs(), {ROWS: 32}, [33, 5], [50])["rows"].tolist() == [32, 32]
    for P in (33, 76, 2048):
        got = sedgpu.fit_index_long_f64_plan(r.costs(), {CHUNK: 8}, [P], [300])
        assert (got["W"], got["one_lane"], got["chunk"]) == (3 * P + 2, 0, 8)
    # slot 6: insert = 0 (1); x = P delete / insert above 2^20, a cost out of 2^-900 .. 2^900 (2)
    for plan, P, why in ((fc.unit(9, 0.0, 1.0), 76, 1), (fc.unit(9, 1e-3, 1.0), 2048, 2), (fc.unit(9, 1e-300, 1.0), 76, 2)):
        got = sedgpu.fit_index_long_f64_plan(plan.costs(), {CHUNK: 8}, [P, 3], [300, 70000])
        assert (got["W"], got["one_lane"], got["chunk"], got["lanes"]) == (-1, why, 0, 4)
    assert sedgpu.fit_index_long_f64_plan(fc.unit(9, 1e-3, 1.0).costs(), {CHUNK: 8}, [1000], [300])["one_lane"] == 0
    # the chunk rule counts waves: 2048 pairs keep one chunk per text, 2047 are split, never below W
    u = fc.unit(9)
    assert sedgpu.fit_index_long_f64_plan(u.costs(), {}, [76] * 2, [4096] * 1024)["chunk"] == 0
    got = sedgpu.fit_index_long_f64_plan(u.costs(), {}, [76], [4096] * 2047)
    assert got["W"] == 154 and got["chunk"] == 2048 and got["lanes"] == 2047 * 3
    assert sedgpu.fit_index_long_f64_plan(u.costs(), {}, [1024], [4096] * 8)["chunk"] == 2050
    assert sedgpu.fit_index_f64_plan(u.costs(), {}, [20], [4096] * 2047)["chunk"] < 2048  # (the short plan counts lanes)


def test_records_equal_the_short_fp64_plans():
    p = TABLES["rounding"]
    len_p, len_t = [1, 31, 32], [0, 1, 64, 333, 1000]
    for chunk in (8, 104, 1 << 20):
        a = sedgpu.fit_index_f64_lanes(p.costs(), {CHUNK: chunk}, len_p, len_t)
        b = sedgpu.fit_index_long_f64_lanes(p.costs(), {CHUNK: chunk}, len_p, len_t)
        assert all((a[k] == b[k]).all() for k in sedgpu.FIT_LANE_FIELDS)
        pa = sedgpu.fit_index_f64_plan(p.costs(), {CHUNK: chunk}, len_p, len_t)
        pb = sedgpu.fit_index_long_f64_plan(p.costs(), {CHUNK: chunk}, len_p, len_t)
        assert pb.pop("rows").tolist() == [2, 2, 2] and pa == pb
    b = sedgpu.fit_index_long_f64_lanes(p.costs(), {CHUNK: 100}, [200, 40], [1000, 3])
    assert b["pair"].tolist() == [0] * 11 + [1] + [2] * 11 + [3] and b["c0"][:11].tolist() == list(range(0, 1001, 100))
    W = 602
    assert b["lead"][:11].tolist() == [c0 - (0 if c0 <= W else (c0 - W) & ~3) for c0 in range(0, 1001, 100)]


def test_long_route():
    user = fc.golden_dyadic("user_costs.json", "ACGU")
    assert sedgpu.fit_long_route(user.costs(), {}, [76, 5, 2048], [4096, 0]) == ("int", "")
    route, why = sedgpu.fit_long_route(TABLES["costs15"].costs(), {}, [76], [4096])
    assert route == "f64" and "15 symbols (at most 8)" in why
    third = fc.unit(4)
    third.sub[0, 1] = 1.0 / 3.0
    route, why = sedgpu.fit_long_route(third.costs(), {}, [76], [4096])
    assert route == "f64" and "not all multiples" in why
    route, why = sedgpu.fit_long_route(unit_costs(17, 1, 1), {}, [76], [4096])
    assert route is None and "17 symbols (at most 8)" in why.split("; ")[0] and "17 symbols (at most 16)" in why.split("; ")[1]
    # the integer long calls' own limits: the D field and the span
    big = fc.unit(4, 16.0, 31.0)
    assert sedgpu.fit_long_route(big.costs(), {}, [2048], [100])[0] == "f64"
    assert sedgpu.fit_long_route(fc.unit(4, 0.0, 1.0).costs(), {}, [76], [70000])[0] == "f64"


LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 62, 63, 64, 65, 100, 127, 128, 129, 199, 200]


def _model_cases(plan, options, rng, P, lengths=LENGTHS):
    """Texts of 0..200 symbols, and for length 200 copies of the pattern planted to end on the seams of the planner's
    own records, on the last column and over all of them; a homopolymer for ties."""
    p = rng.integers(0, plan.K, size=P).astype(np.uint8)
    texts = [rng.integers(0, plan.K, size=n).astype(np.uint8) for n in lengths]
    n = 200
    if P <= n:
        seams = [e for e in fc.seam_columns(sedgpu.fit_index_long_f64_lanes(plan.costs(), options, [P], [n])) if e >= P]
        pick = seams[:: max(1, len(seams) // 4)]
        texts += [fc.plant(rng, plan.K, p, n, [e]) for e in pick + [n]] + [fc.plant(rng, plan.K, p, n, seams)]
    texts.append(np.full(150, p[0], np.uint8))
    return p, texts


def _check_model(plan, options, P, rng, hits_too, lengths=LENGTHS):
    p, texts = _model_cases(plan, options, rng, P, lengths)
    len_t = [len(t) for t in texts]
    out = sedgpu.fit_index_long_f64_plan(plan.costs(), options, [P], len_t)
    lanes = sedgpu.fit_index_long_f64_lanes(plan.costs(), options, [P], len_t)
    assert out["lanes"] == len(lanes["pair"]) and out["lanes"] > len(texts)
    T = math.inf if hits_too else None
    best, hits = lc.run_waves_grouped(plan, lanes, out["rows"], [p], texts, T)
    got = fc.reduce_lanes(best, lanes, len(texts))
    want = fc.oracle_fit(plan, [p] * len(texts), texts)
    assert got == want, next((k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w)
    if hits_too:
        ref = lc.hits_reference(plan, [p] * len(texts), texts, T)
        assert sorted((q, s, e, d) for q, e, s, d in hits) == ref and len(ref) == sum(len_t) + len(texts)
    return out


@pytest.mark.parametrize("tname", ["rounding", "costs15"])
@pytest.mark.parametrize("R", [2, 4, 8, 16, 32])
def test_wave_model_every_forced_R(tname, R):
    """The wave restated, over the planner's records, equals oracle.fit (and the last row, P = 33): P = 33, behind
    64 R - 33 front rows that fill whole lanes from R = 4 on, and the smallest P of the group."""
    plan = TABLES[tname]
    rng = np.random.default_rng(R)
    lengths = LENGTHS if R <= 8 else LENGTHS[::2]
    for P in sorted({33, 64 * R // 2 + 1}):
        W = sedgpu.fit_index_long_f64_plan(plan.costs(), {ROWS: R}, [P], [200])["W"]
        for chunk in ((8, W + 4) if P == 33 and tname == "rounding" else (W + 4,) if P == 33 else (8,)):
            out = _check_model(plan, {ROWS: R, CHUNK: chunk}, P, rng, P == 33 and chunk == 8, lengths)
            assert out["rows"].tolist() == [R] and out["chunk"] == chunk


@pytest.mark.parametrize("P", [127, 128, 129])
def test_wave_model_automatic_R(P):
    plan = TABLES["rounding"]
    out = _check_model(plan, {CHUNK: 8}, P, np.random.default_rng(P), P == 128, LENGTHS[::2])
    assert out["rows"].tolist() == [2 if P <= 128 else 4] and out["W"] == 3 * P + 2


def test_last_row_reference_is_the_definition():
    from test_fit_hits_host import hits_row
    rng = np.random.default_rng(5)
    for plan in TABLES.values():
        pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in (1, 9, 40, 40)]
        texts = [fc.plant(rng, plan.K, p, n, [n // 2, n]) for p, n in zip(pats, (0, 30, 90, 7))]
        want = fc.oracle_fit(plan, pats, texts)
        for k, (E, S) in enumerate(lc.last_rows(plan, pats, texts)):
            assert list(zip(E.tolist(), S.tolist())) == hits_row(plan.sub.tolist(), plan.ins, plan.dele, pats[k].tolist(),
                                                                 texts[k].tolist())
            assert lc.best_of_row(E, S) == want[k]


class LongF64Engine(DefinitionEngine):
    """DefinitionEngine with every call of the index, logged: the integer ones refuse what the device's refuse (more
    than 8 symbols), the fp64 hits come from the last-row reference."""

    def __init__(self, codes, off, lens):
        super().__init__(codes, off, lens)
        self.log = []

    def _int(self, plan):
        if plan.K > 8:
            err = sedgpu.SedError("fit search: the batch has %d symbols (at most 8)" % plan.K)
            err.code = E_RANGE
            raise err

    def _rows(self, plan, packed, max_dist):
        out = []
        for q in range(packed.npairs):
            p = packed.codes_a[packed.off_a[q]:packed.off_a[q] + packed.len_a[q]]
            for d, (E, S) in enumerate(lc.last_rows(plan, [p] * len(self.texts), self.texts)):
                out += [(q, d, int(S[e]), e, float(E[e])) for e in np.nonzero(E <= max_dist)[0].tolist()]
        return np.array(out, sedgpu.FIT_HIT_DTYPE)

    def search(self, plan, packed):
        self.log.append(("search", packed.len_a.tolist()))
        self._int(plan)
        return super().search(plan, packed)

    def search_long(self, plan, packed):
        self.log.append(("search_long", packed.len_a.tolist()))
        self._int(plan)
        return super().search(plan, packed)

    def search_f64(self, plan, packed):
        self.log.append(("search_f64", packed.len_a.tolist()))
        return super().search(plan, packed)

    def search_long_f64(self, plan, packed):
        self.log.append(("search_long_f64", packed.len_a.tolist()))
        return super().search(plan, packed)

    def hits(self, plan, packed, max_dist):
        self.log.append(("hits", packed.len_a.tolist()))
        self._int(plan)
        return self._rows(plan, packed, max_dist)

    def hits_long(self, plan, packed, max_dist):
        self.log.append(("hits_long", packed.len_a.tolist()))
        self._int(plan)
        return self._rows(plan, packed, max_dist)

    def hits_f64(self, plan, packed, max_dist):
        self.log.append(("hits_f64", packed.len_a.tolist()))
        return self._rows(plan, packed, max_dist)

    def hits_long_f64(self, plan, packed, max_dist):
        self.log.append(("hits_long_f64", packed.len_a.tolist()))
        return self._rows(plan, packed, max_dist)


def _docs(rng, query, alphabet, count, n):
    docs = ["", query]
    for k in range(2, count):
        d = list(rng.choice(list(alphabet), size=n))
        m = list(query)
        for _ in range(k % 3):
            m[int(rng.integers(0, len(m)))] = str(rng.choice(list(alphabet)))
        at = int(rng.integers(0, len(d) - len(m)))
        d[at:at + len(m)] = m
        docs.append("".join(d))
    return docs


def test_wfsearch_routes_the_long_queries(wfsearch, monkeypatch):
    SED = wfsearch.SED
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    monkeypatch.setattr(SED, "user_costs", load_golden("user_costs.json"))
    rng = np.random.default_rng(76)
    query = "".join(rng.choice(list("ACGU"), size=40))
    queries = [query[:12], query, query[:33], query[3:20]]
    make = lambda t, uc, f64=False: SED.fit_index(t, uc, engine=LongF64Engine, f64=f64)
    T = 0.9
    for alphabet, user_cost, serves in (("ACGU", True, "int"), (fc.IUPAC, False, "f64")):
        docs = _docs(rng, query, alphabet, 5, 90)
        plan = SED.FitIndex(docs, user_cost, engine=LongF64Engine, f64=True).plan(queries)

        def want(q):
            out = []
            E, S = zip(*lc.last_rows(plan, [plan.encode(q)] * len(docs), [plan.encode(d) for d in docs]))
            for doc, e_row, s_row in zip(docs, E, S):
                row = list(zip(e_row.tolist(), s_row.tolist()))
                ends = [e for e, (d, _) in enumerate(row) if d <= T and d < (row[e - 1][0] if e else math.inf)
                        and d <= (row[e + 1][0] if e < len(doc) else math.inf)]
                out += [(doc, 1 / (1 + row[e][0]), int(row[e][1]), e) for e in ends]
            return out

        wanted = [want(q) for q in queries]
        assert any(wanted[1]) and any(wanted[0])
        ix = wfsearch.FitIndex(docs, user_cost, index_fn=make, route="auto")
        dev = ix._ix._dev
        short_call, long_call = ("hits", "hits_long") if serves == "int" else ("hits_f64", "hits_long_f64")
        # auto: the integer calls whenever they serve, else the fp64 ones; merged in query order
        assert ix.occurrences_many(queries, T, long_patterns=True) == wanted
        assert dev.log == [(short_call, [12, 17]), (long_call, [40, 33])]
        del dev.log[:]
        # f64: both halves on the fp64 calls, the same results
        assert ix.occurrences_many(queries, T, long_patterns=True, route="f64") == wanted
        assert dev.log == [("hits_f64", [12, 17]), ("hits_long_f64", [40, 33])]
        del dev.log[:]
        # int: today's calls, and today's refusal over 15 symbols
        if serves == "int":
            assert ix.occurrences_many(queries, T, long_patterns=True, route="int") == wanted
            assert dev.log == [("hits", [12, 17]), ("hits_long", [40, 33])]
        else:
            with pytest.raises(sedgpu.SedError):
                ix.occurrences_many(queries[1:2], T, long_patterns=True, route="int")
            assert dev.log == [("hits_long", [40])]
        del dev.log[:]
        best = ix.search_many(queries, long_patterns=True)
        assert [c for c, _ in dev.log] == [short_call.replace("hits", "search"), long_call.replace("hits", "search")]
        for q, hits in zip(queries, best):
            every = ix.occurrences(q, math.inf, long_patterns=True)
            assert [h[0] for h in hits] == docs and all(h in every for h in hits)
        # scripts: one edit_script_batch call for the merged list, of (query, sequence[start:end])
        with monkeypatch.context() as m:
            batches = _fake_scripts(m, SED)
            withes = ix.occurrences_many(queries, T, scripts=True, long_patterns=True)
            assert batches == [sum(len(m) for m in wanted)]
        for q, got, plain in zip(queries, withes, wanted):
            assert [g[:4] for g in got] == plain and all(g[4] == ("es", q, g[0][g[2]:g[3]]) for g in got)
        assert wfsearch.fit_occurrences(query, docs, T, user_cost, long_patterns=True, index_fn=make, route="auto") == wanted[1]
        ix.close()
    with pytest.raises(ValueError):
        wfsearch.FitIndex(["ACGU"], index_fn=make).occurrences("A" * 40, 1, long_patterns=True, route="fp64")
