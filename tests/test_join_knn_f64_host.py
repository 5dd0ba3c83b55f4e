"""CPU: the fp64 route of the k-nearest calls, device-free - the new exports, the lower-bound table
(sed_join_f64_lower) against the keep rule and the oracle, the two passes restated on 64-bit keys under several
schedules, k through the planner (sed_join_knn_f64_plan), and the Python layers (StringEditDistance.JoinIndex
.self_nearest_f64 / search_nearest_f64, wfsearch's and sedshard's route=) over oracle-backed engines."""
import inspect
import math

import numpy as np
import pytest

import join_cases as jc
import join_f64_cases as jf
import join_knn_cases as kc
import join_knn_f64_cases as kf
import sedgpu
import sedshard

INF = math.inf


@pytest.fixture(scope="module")
def wfsearch():
    return jc.import_shim("wfsearch")


# ---- exports ----

def test_the_new_exports_exist(wfsearch):
    lib = sedgpu.load()
    for name in ("sed_join_knn_self_f64", "sed_join_knn_search_f64", "sed_join_knn_bounds_f64", "sed_join_knn_f64_plan",
                 "sed_join_f64_lower"):
        assert getattr(lib, name)
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(sedgpu.JoinIndex.self_knn_f64) == ["self", "k", "max_dist", "rows", "cap"]
    assert params(sedgpu.JoinIndex.search_knn_f64) == ["self", "packed", "k", "max_dist", "cap"]
    assert params(sedgpu.JoinIndex.knn_bounds_f64) == ["self"]
    assert params(sedgpu.join_knn_f64_plan) == ["costs", "options", "len_rows", "len_cols", "self_join", "row_codes",
                                                "col_codes", "k", "max_dist"]
    assert params(sedgpu.join_f64_lower) == ["ins", "dele"]
    SED = jc.import_shim("StringEditDistance")
    assert params(SED.JoinIndex.self_nearest_f64) == ["self", "k", "max_dist", "rows"]
    assert params(SED.JoinIndex.search_nearest_f64) == ["self", "queries", "k", "max_dist"]
    assert hasattr(SED._EngineJoin, "self_knn_f64") and hasattr(SED._EngineJoin, "search_knn_f64")
    assert params(wfsearch.JoinIndex.nearest) == ["self", "k", "max_dist", "rows", "route"]
    assert params(wfsearch.JoinIndex.nearest_many) == ["self", "queries", "k", "max_dist", "route"]
    assert inspect.signature(wfsearch.nearest_neighbors).parameters["route"].default == "int"
    assert inspect.signature(sedshard.nearest_neighbors).parameters["route"].default == "int"
    ix = object.__new__(sedgpu.LongJoinIndex)
    for call in (lambda: ix.self_knn_f64(1), lambda: ix.search_knn_f64(None, 1), lambda: ix.knn_bounds_f64()):
        with pytest.raises(sedgpu.SedError, match="no fp64 route yet"):
            call()
    ix.ptr = None


# ---- the lower-bound table ----

COSTS = [(1.0, 1.0), (0.625, 1.25), (0.1, 0.3), (0.3, 0.1), (5e-324, 3 * 5e-324), (2.0 ** -1030, 2.0 ** -890),
         (1e300, 1e300), (1e308, 0.5), (0.0, 0.0), (0.0, 1.0), (-0.0, 0.25)]


@pytest.mark.parametrize("ins,dele", COSTS)
def test_lower_table_is_what_the_keep_rule_compares(ins, dele):
    low = sedgpu.join_f64_lower(ins, dele)
    assert low.shape == (33, 33) and not np.isnan(low).any() and not np.signbit(low).any()
    assert np.array_equal(low.view(np.uint64), kf.lower_model(ins, dele).view(np.uint64))
    cuts = {0.0, INF}
    for v in np.unique(low):
        cuts |= {float(v), float(np.nextafter(v, INF)), float(np.nextafter(v, -INF))}
    for T in sorted(t for t in cuts if t >= 0):
        keep = sedgpu.join_f64_keep(ins, dele, T)
        assert np.array_equal(keep, low <= T), T
        assert np.array_equal(keep, jf.keep_rule(ins, dele, T)), T  # the rule as it was spelled before the table


def test_lower_table_refuses_what_keep_refuses():
    for ins, dele in ((-1.0, 1.0), (1.0, math.nan), (INF, 1.0), (1.0, -5e-324)):
        with pytest.raises(sedgpu.SedError):
            sedgpu.join_f64_lower(ins, dele)
        with pytest.raises(sedgpu.SedError):
            sedgpu.join_f64_keep(ins, dele, 1.0)


@pytest.mark.parametrize("name", ["iupac", "near ties", "overflow", "zero", "spread"])
def test_lower_table_bounds_every_oracle_distance(name):
    c = kf.case(name)
    assert (kf.low_of(c.low, c.lens, c.lens) <= c.D).all()


# ---- the two passes on 64-bit keys ----

def test_keys_order_as_the_values_do():
    v = np.array([0.0, 5e-324, 2.0 ** -1022, 0.1, 0.30000000000000004, 0.3, 1.0, 1e308, 1.7976931348623157e308, INF])
    k = kf.keys(v)
    for i in range(len(v)):
        for j in range(len(v)):
            assert (v[i] < v[j]) == (k[i] < k[j]) and (v[i] == v[j]) == (k[i] == k[j])
    assert int(k[-1]) == 0x7FF0000000000000 and int(k.max()) < 1 << 63


def test_bisection_is_the_kth_smallest():
    rng = np.random.default_rng(64)
    pool = np.concatenate([rng.random(40) * 10.0 ** rng.integers(-300, 300, 40), [0.0, 0.0, INF, INF, 5e-324, 0.3,
                                                                                   0.30000000000000004, 1e308]])
    for trial in range(60):
        D = rng.choice(pool, size=(5, 64))
        cand = rng.random((5, 64)) < rng.random()
        for k in (1, 2, 8, 63, 64):
            x = kf.kth_by_bisection(kf.keys(D), cand, k)
            for r in range(5):
                v = np.sort(D[r][cand[r]])
                if len(v) >= k:
                    assert x[r] == kf.keys(v[k - 1:k])[0]


CASE_CALLS = [("random N", 8, INF), ("iupac", 8, INF), ("iupac", 3, 2.5), ("ties", 8, INF), ("near ties", 2, INF),
              ("near ties", 3, 0.3), ("overflow", 8, INF), ("overflow", 64, INF), ("zero", 8, INF), ("spread", 8, INF),
              ("spread", 8, 1.0), ("spread", 3, 0.65)]


@pytest.mark.parametrize("name,k,T", CASE_CALLS)
def test_bounds_are_the_same_in_every_schedule(name, k, T):
    c = kf.case(name)
    ok = kc.in_scope(c.D.shape, True, 0)
    want, cand = kf.pass1_by_definition(c.D, c.lens, k, T, True)
    ran = []
    for order in kc.ORDERS:
        bound, pairs = kf.bound_pass_model(c.D, ok, c.lens, c.lens, c.low, k, T, order)
        assert np.array_equal(bound.view(np.uint64), want.view(np.uint64)), order
        ran.append(pairs)
    mask, p2, _ = kf.emit_pass_model(c.D, ok, c.lens, c.lens, c.low, want)
    assert int(mask.sum()) == cand
    assert p2 <= min(ran) and max(ran) <= kf.pairs_at(ok, c.lens, c.lens, c.low, T) == ran[kc.ORDERS.index("stale")]
    # the emit set trimmed to k is the expected list
    r, col = np.nonzero(mask)
    hits = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
    hits["row"], hits["col"], hits["dist"] = r, col, c.D[r, col]
    assert jc.same_hits(sedgpu.join_knn_trim(hits[np.random.default_rng(1).permutation(len(hits))], k),
                        kf.expected_knn(c.D, k, T, True))


def test_the_sets_have_the_properties_the_device_tests_rest_on():
    c = kf.case("iupac")
    assert c.plan.K == 15 and bin(jc.codes_mask(c.plan, c.seqs)).count("1") == 15
    mask = jc.codes_mask(c.plan, c.seqs)
    with pytest.raises(sedgpu.SedError, match="15 symbols"):
        sedgpu.join_knn_plan(jc.costs_of(c.plan), {}, c.lens, c.lens, True, mask, mask, 8, INF)
    assert sedgpu.join_knn_f64_plan(jc.costs_of(c.plan), {}, c.lens, c.lens, True, mask, mask, 8, INF)["kernel"] == 3
    # near ties: a row with two in-scope distances that differ, within 1e-12 relative
    c = kf.case("near ties")
    close = 0
    for r in range(len(c.seqs)):
        v = np.unique(np.delete(c.D[r], r))
        close += int(((np.diff(v) > 0) & (np.diff(v) <= 1e-12 * v[1:])).any())
    assert close >= 10
    # overflow: +inf among the k nearest
    c = kf.case("overflow")
    want = kf.expected_knn(c.D, 8, INF, True)
    assert np.isinf(want["dist"]).any() and (want["dist"] == 1e308).any() and (want["dist"] == 0).any()
    assert not c.D[np.isfinite(c.D)].max() > 1e308
    # zero: every distance ties
    assert not kf.case("zero").D.any()
    # spread: pass 2 skips whole (wave, row)s under bounds below the cap; some wave has fewer than k within a cap
    c = kf.case("spread")
    ok = kc.in_scope(c.D.shape, True, 0)
    assert c.plan.ins != c.plan.dele and min(c.lens) == 0 and max(c.lens) == 32 and c.lens.count(0) >= 3
    bound, _ = kf.pass1_by_definition(c.D, c.lens, 8, INF, True)
    assert (bound < INF).all() and kf.emit_pass_model(c.D, ok, c.lens, c.lens, c.low, bound)[2] > 0
    bound, _ = kf.pass1_by_definition(c.D, c.lens, 3, 0.65, True)
    assert (bound == 0.65).any() and (bound < 0.65).any()


# ---- k through the planner ----

def test_planner_refuses_k_before_anything_else():
    t17 = {"insert": 1.0, "delete": 1.0, "update": {a: {b: float(a != b) for b in "ABCDEFGHIJKLMNOPQ"} for a in "ABCDEFGHIJKLMNOPQ"}}
    p17 = jc.plan_for(t17, "ABCDEFGHIJKLMNOPQ")
    neg, al = kf.flat_table(1.0, ins=-1.0)
    pneg = jc.plan_for(neg, al)
    plan = kf.case("iupac").plan
    lens = [5, 20, 32]
    mask = 0x7FFF
    for k in (0, 65, -1):
        for p in (p17, pneg, plan):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d .*1\.\.64" % k) as e:
                sedgpu.join_knn_f64_plan(jc.costs_of(p), {}, lens, lens, True, 1, 1, k, math.nan)
            assert e.value.code == -1
    with pytest.raises(sedgpu.SedError, match=r"\(-1\).*max_dist is NaN or negative"):
        sedgpu.join_knn_f64_plan(jc.costs_of(p17), {}, lens, lens, True, 1, 1, 1, math.nan)
    with pytest.raises(sedgpu.SedError, match=r"\(-4\).*join \(fp64\): 17 symbols \(at most 16\)") as e:
        sedgpu.join_knn_f64_plan(jc.costs_of(p17), {}, lens, lens, True, 1, 1, 64, INF)
    assert e.value.code == -4
    with pytest.raises(sedgpu.SedError, match=r"\(-4\).*join \(fp64\): insert = -1 is not a finite cost >= 0"):
        sedgpu.join_knn_f64_plan(jc.costs_of(pneg), {}, lens, lens, True, 1, 1, 1, INF)
    with pytest.raises(sedgpu.SedError, match=r"\(-1\).*column code is outside the alphabet \(K=15\)"):
        sedgpu.join_knn_f64_plan(jc.costs_of(plan), {}, lens, lens, True, mask, 1 << 15, 1, INF)
    with pytest.raises(sedgpu.SedError, match=r"\(-1\).*33 symbols"):
        sedgpu.join_knn_f64_plan(jc.costs_of(plan), {}, [33], lens, False, mask, mask, 1, INF)
    for T in (2.0, INF):
        join = sedgpu.join_f64_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, T)
        for k in (1, 64):
            assert sedgpu.join_knn_f64_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, k, T) == join


# ---- the shim over a codes-level oracle engine ----

def test_shim_self_nearest_f64_and_search_nearest_f64():
    SED = jc.import_shim("StringEditDistance")
    seqs = kf.iupac_set(5, 40) + ["", "ACGU"]
    plan = jc.plan_for(jc.load_golden("costs.json"), jf.IUPAC)
    ix = SED.join_index(seqs, False, alphabet=jf.IUPAC, engine=kf.CodesEngine, f64=True)
    assert ix.symbols == list(jf.IUPAC)
    D = jc.oracle_matrix(plan, seqs, seqs)
    N = len(seqs)
    for k, T in ((1, None), (5, None), (64, None), (5, 6.0), (3, 0)):
        want = kc._nearest(D, k, T, True)
        assert ix.self_nearest_f64(k, T) == want
        assert ix.self_nearest_f64(k, T, rows=(7, 19)) == [h for h in want if 7 <= h[0] < 19]
    assert ix.self_nearest_f64(3, None, rows=(4, 4)) == []
    assert ix._dev.calls[0] == ("self_knn_f64", 1, INF, (0, N))  # None reaches the engine as +inf
    assert {c[0] for c in ix._dev.calls} == {"self_knn_f64"}
    ncalls = len(ix._dev.calls)
    for k in (0, 65, -1, 2.0, True):  # check_k first, also where the engine would not be reached
        for call in (lambda: ix.self_nearest_f64(k), lambda: ix.self_nearest_f64(k, rows=(4, 4)),
                     lambda: ix.search_nearest_f64(["ACG"], k), lambda: ix.search_nearest_f64([], k)):
            with pytest.raises(sedgpu.SedError, match=r"k = .* \(1\.\.64\)"):
                call()
    assert len(ix._dev.calls) == ncalls
    queries = [seqs[3], "", seqs[9][:-1] + "R", "ACGU"]
    Dq = jc.oracle_matrix(plan, queries, seqs)
    for k, T in ((1, None), (4, None), (4, 6.5)):
        assert ix.search_nearest_f64(queries, k, T) == kc._nearest(Dq, k, T)
    assert ix._dev.calls[-1][0] == "search_knn_f64" and ix._dev.calls[-3][2] == INF
    assert ix.search_nearest_f64([], 3) == []
    with pytest.raises(ValueError, match="no range"):
        ix.self_nearest_f64(1, rows=(3, N + 1))
    ix.self_nearest(2)  # unchanged: the integer call, also on an index built f64=True
    assert ix._dev.calls[-1][0] == "self_knn"
    ix.close()


# ---- wfsearch ----

def _lists(D, k, T, seqs=None):
    if seqs is None:
        return [[(j, 1 / (1 + d)) for _, j, d in kc._nearest(D[i:i + 1], k, T, True, i)] for i in range(D.shape[0])]
    return [[(seqs[j], 1 / (1 + d)) for _, j, d in kc._nearest(D[q:q + 1], k, T)] for q in range(D.shape[0])]


def test_wfsearch_routes_agree_where_the_integer_route_serves(wfsearch):
    seqs = kc.random_set(8, 50)
    plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, seqs, seqs)
    queries = [seqs[3], "", seqs[9][:-1] + "A"]
    Dq = jc.oracle_matrix(plan, queries, seqs)
    for ctor in ("int", "f64", "auto"):
        ix = wfsearch.JoinIndex(seqs, True, index_fn=kf.OracleEngine, route=ctor)
        eng = kf.OracleEngine.built[-1]
        assert eng.kw == ({} if ctor == "int" else {"f64": True})
        for k, T in ((1, None), (8, None), (8, 20.0)):
            want = _lists(D, k, T)
            for route, call in ((None, {"int": "self_nearest", "f64": "self_nearest_f64", "auto": "self_nearest"}[ctor]),
                                ("int", "self_nearest"), ("f64", "self_nearest_f64"), ("auto", "self_nearest")):
                assert ix.nearest(k, T, route=route) == want and eng.calls[-1] == call, (ctor, route)
            assert ix.nearest(k, T, rows=(7, 19), route="f64") == want[7:19]
            wq = _lists(Dq, k, T, seqs)
            for route, call in (("int", "search_nearest"), ("f64", "search_nearest_f64"), ("auto", "search_nearest")):
                assert ix.nearest_many(queries, k, T, route=route) == wq and eng.calls[-1] == call
        with pytest.raises(ValueError, match="route must be one of"):
            ix.nearest(1, route="fp64")
        ix.close()
    for route in ("int", "f64", "auto"):
        assert wfsearch.nearest_neighbors(seqs, 8, None, True, index_fn=kf.OracleEngine, route=route) == _lists(D, 8, None)
        assert kf.OracleEngine.built[-1].closed
        assert kf.OracleEngine.built[-1].calls == ["self_nearest_f64" if route == "f64" else "self_nearest"]


def test_wfsearch_iupac_collections_are_served_by_f64_and_auto(wfsearch):
    seqs = kf.iupac_set(9, 40)
    plan = jc.plan_for(jc.load_golden("costs.json"), jf.IUPAC)
    D = jc.oracle_matrix(plan, seqs, seqs)
    queries = [seqs[5], "", "ACGURY"]
    Dq = jc.oracle_matrix(plan, queries, seqs)
    for route in ("f64", "auto"):
        for k, T in ((1, None), (8, None), (8, 5.0)):
            assert wfsearch.nearest_neighbors(seqs, k, T, index_fn=kf.OracleEngine, route=route) == _lists(D, k, T)
            assert kf.OracleEngine.built[-1].calls == ["self_nearest_f64"]
        ix = wfsearch.JoinIndex(seqs, index_fn=kf.OracleEngine, route=route)
        assert ix.nearest(8) == _lists(D, 8, None)
        assert ix.nearest_many(queries, 3, 9.0) == _lists(Dq, 3, 9.0, seqs)
        assert kf.OracleEngine.built[-1].calls == ["self_nearest_f64", "search_nearest_f64"]
        with pytest.raises(sedgpu.SedError):
            ix.nearest(8, route="int")
        ix.close()
    with pytest.raises(sedgpu.SedError):
        wfsearch.nearest_neighbors(seqs, 8, index_fn=kf.OracleEngine)
    for route in ("f64", "auto"):  # the long index: unchanged
        with pytest.raises(ValueError, match="no fp64 route yet"):
            wfsearch.nearest_neighbors(seqs, 8, index_fn=kf.OracleEngine, long_sequences=True, route=route)
        with pytest.raises(ValueError, match="no fp64 route yet"):
            wfsearch.JoinIndex(seqs, index_fn=kf.OracleEngine, long_sequences=True).nearest(8, route=route)
        with pytest.raises(ValueError, match="no fp64 route yet"):
            wfsearch.JoinIndex(seqs, index_fn=kf.OracleEngine, long_sequences=True).nearest_many(["ACG"], 8, route=route)


# ---- sedshard ----

def test_sedshard_nearest_neighbors_passes_the_route():
    seen = []

    def join_fn(seqs, lo, hi, k, max_dist, user, **kw):
        seen.append(kw)
        return kf.OracleEngine(seqs, user).self_nearest_f64(k, max_dist, (lo, hi))

    seqs = kc.random_set(9, 11)
    D = jc.oracle_matrix(jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN"), seqs, seqs)
    for route, kw in (("int", {}), ("f64", {"f64": True}), ("auto", {})):
        for T in (None, 20.0):
            got = sedshard.nearest_neighbors(seqs, 3, T, True, world=1, join_fn=join_fn, route=route)
            assert jc.same_hits(got, kf.expected_knn(D, 3, INF if T is None else T, True)) and seen[-1] == kw
    assert sedshard.nearest_neighbors(seqs, 3, None, True, join_fn=join_fn) is not None and seen[-1] == {}
    iu = kf.iupac_set(9, 12)
    Di = jc.oracle_matrix(jc.plan_for(jc.load_golden("costs.json"), jf.IUPAC), iu, iu)
    for route in ("f64", "auto"):
        got = sedshard.nearest_neighbors(iu, 3, None, False, join_fn=join_fn, route=route)
        assert jc.same_hits(got, kf.expected_knn(Di, 3, INF, True)) and seen[-1] == {"f64": True}
    with pytest.raises(ValueError, match="route must be one of"):
        sedshard.nearest_neighbors(seqs, 3, join_fn=join_fn, route="fp64")
    for route in ("f64", "auto"):
        with pytest.raises(ValueError, match="no fp64 route yet"):
            sedshard.nearest_neighbors(seqs, 3, join_fn=join_fn, long_sequences=True, route=route)
