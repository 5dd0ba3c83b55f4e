"""GPU: the fp64 route of the similarity join (sed_join_self_f64, sed_join_search_f64) against the C oracle over the full
cross product, cut with D <= T on the host.  Hits match exactly: the same (row, col), and dist bit for bit."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_f64_cases as jf
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # (table, set) -> (plan, seqs, D): computed once, shared, never changed


def ref(name, kind="mixed", count=130):
    key = (name, kind, count)
    if key not in _REF:
        table, al = jf.subnormal_table() if name == "subnormal" else jf.tables()[name]
        plan = jc.plan_for(table, al)
        seqs = jf.edge_length_set(name, count) if kind == "edge" else jf.mixed_set(name, count)
        D = jc.oracle_matrix(plan, seqs, seqs)
        D.setflags(write=False)
        _REF[key] = (plan, seqs, D)
    return _REF[key]


def index_of(gpu, plan, seqs):
    gpu.set_costs(plan)
    return sedgpu.JoinIndex.from_seqs(gpu, jc.encode(plan, seqs))


def f64_plan(plan, rows, cols, self_join, T, options=None):
    return sedgpu.join_f64_plan(jc.costs_of(plan), options or {}, [len(s) for s in rows], [len(s) for s in cols], self_join,
                                jc.codes_mask(plan, rows), jc.codes_mask(plan, cols), T)


@pytest.fixture
def rows_option(gpu):
    yield lambda rows: gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, rows)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 257])
def test_column_geometry(gpu, N):
    """Wave and block edges on the column side, self and search, every pair (T = +inf)."""
    plan, seqs, D = ref("costs15", count=257)
    ix = index_of(gpu, plan, seqs[:N])
    try:
        got = ix.self_join_f64(INF)
        assert jc.same_hits(got, jf.expected_hits_f64(D[:N, :N], INF, True))
        assert len(got) == N * (N - 1)
        q = [3 % N, 0, N - 1]
        got = ix.search_f64(jc.packed_queries(plan, [seqs[i] for i in q]), INF)
        assert jc.same_hits(got, jf.expected_hits_f64(D[q][:, :N], INF))
    finally:
        ix.close()


def test_row_geometry(gpu):
    """G - 1, G, G + 1 and 2 G + 1 rows, by rows= ranges and by query counts."""
    G = sedgpu.join_rows_per_group()
    plan, seqs, D = ref("costs15", count=257)
    N = 70
    ix = index_of(gpu, plan, seqs[:N])
    try:
        for R in (G - 1, G, G + 1, 2 * G + 1):
            for lo in (0, 5, N - R):
                got = ix.self_join_f64(INF, rows=(lo, lo + R))
                assert jc.same_hits(got, jf.expected_hits_f64(D[lo:lo + R, :N], INF, True, lo)), (R, lo)
            q = list(range(100, 100 + R))
            got = ix.search_f64(jc.packed_queries(plan, [seqs[i] for i in q]), INF)
            assert jc.same_hits(got, jf.expected_hits_f64(D[q][:, :N], INF)), R
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["costs15", "rounding", "random16", "user_costs", "subnormal"])
def test_tables_cutoffs_and_plan_equals_run(gpu, name):
    """Every table at T in {0, 2, an occurring D, its neighbour below, +inf}: the hits are the oracle's, the count steps
    by exactly the pairs at that D, and the pairs the waves ran are the planner's."""
    plan, seqs, D = ref(name)
    N = len(seqs)
    off = ~np.eye(N, dtype=bool)
    d = float(np.unique(D[off])[3])  # a distance that occurs
    ix = index_of(gpu, plan, seqs)
    try:
        counts = {}
        for T in (0.0, 2.0, d, float(np.nextafter(d, 0.0)), INF):
            got = ix.self_join_f64(T)
            assert jc.same_hits(got, jf.expected_hits_f64(D, T, True)), (name, T)
            p = f64_plan(plan, seqs, seqs, True, T)
            assert p["kernel"] == 3 and p["scale"] == 0
            assert ix.pairs_run() == p["run"], (name, T)
            counts[T] = (len(got), p["run"], p["scope"])
        at_d = int((D[off] == d).sum())
        assert at_d > 0 and counts[d][0] - counts[float(np.nextafter(d, 0.0))][0] == at_d
        if name != "subnormal":  # (subnormal costs: every bound is below 2^-900 and nothing is skipped on n, m >= 1)
            assert counts[0.0][1] < counts[0.0][2]  # the length skip left pairs out
        assert counts[INF][1] == counts[INF][2] == N * (N - 1)
        q = [1, 17, 40, 99]
        got = ix.search_f64(jc.packed_queries(plan, [seqs[i] for i in q]), d)
        assert jc.same_hits(got, jf.expected_hits_f64(D[q], d))
        assert ix.pairs_run() == f64_plan(plan, [seqs[i] for i in q], seqs, False, d)["run"]
    finally:
        ix.close()
    if name == "random16":  # the direction matters under this table
        assert not np.array_equal(D, D.T)


@pytest.mark.parametrize("name", ["costs15", "rounding"])
def test_edge_lengths(gpu, name):
    """Only lengths 0, 1, 31, 32, the buffer's last sequence 32 long: the sink select at m = 0, 1, 32, rows of n = 0,
    and the last record's 16-byte loads."""
    plan, seqs, D = ref(name, kind="edge", count=97)
    ix = index_of(gpu, plan, seqs)
    try:
        for T in (0.0, 1.0, INF):
            assert jc.same_hits(ix.self_join_f64(T), jf.expected_hits_f64(D, T, True)), (name, T)
            assert ix.pairs_run() == f64_plan(plan, seqs, seqs, True, T)["run"]
        queries = ["", seqs[-1], seqs[0]]
        Dq = jc.oracle_matrix(plan, queries, seqs)
        for T in (1.0, INF):
            assert jc.same_hits(ix.search_f64(jc.packed_queries(plan, queries), T), jf.expected_hits_f64(Dq, T))
    finally:
        ix.close()


def test_the_rounded_sum_below_the_product(gpu):
    """insert = 0.1, "A" against "A" + ten other symbols: the oracle's D is 0.9999999999999999 although fl(10 * 0.1) =
    1.0; the pair is a hit at nextafter(1.0, 0) and none one step further down."""
    table, al = jf.rounding_table()
    plan = jc.plan_for(table, al)
    seqs = jf.mixed_set("rounding", 68, seed=77) + ["A", "A" + "CGUCGUCGUC"]
    i, j = len(seqs) - 2, len(seqs) - 1
    D = jc.oracle_matrix(plan, seqs, seqs)
    below = float(np.nextafter(1.0, 0.0))
    assert D[i, j] == below
    ix = index_of(gpu, plan, seqs)
    try:
        for T, there in ((below, True), (float(np.nextafter(below, 0.0)), False)):
            got = ix.self_join_f64(T)
            assert jc.same_hits(got, jf.expected_hits_f64(D, T, True)), T
            assert ((got["row"] == i) & (got["col"] == j)).any() == there
    finally:
        ix.close()


def test_alternating_routes_on_one_index(gpu):
    """user_costs through both routes on one index: equal as (row, col, dist), and the integer call is unchanged by
    having run the fp64 one."""
    plan, seqs, D = ref("user_costs")
    queries = jc.packed_queries(plan, seqs[:5])
    ix = index_of(gpu, plan, seqs)
    try:
        for T in (0.0, 2.0, 2.5, INF):
            before = ix.self_join(T)
            f64 = ix.self_join_f64(T)
            after = ix.self_join(T)
            assert jc.same_hits(before, jf.expected_hits_f64(D, T, True)), T
            assert jc.same_hits(f64, before) and jc.same_hits(after, before), T
            assert jc.same_hits(ix.search_f64(queries, T), ix.search(queries, T)), T
    finally:
        ix.close()


def test_cap_protocol(gpu):
    plan, seqs, D = ref("costs15")
    want = jf.expected_hits_f64(D, 3.0, True)
    wq = jf.expected_hits_f64(D[:5], 3.0)
    queries = jc.packed_queries(plan, seqs[:5])
    ix = index_of(gpu, plan, seqs)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap 0" % len(want)):
            ix.self_join_f64(3.0, cap=0)  # the count query: nothing is stored, found is the total
        assert ix.found == len(want)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap %d" % (len(want), len(want) - 1)):
            ix.self_join_f64(3.0, cap=len(want) - 1)
        assert ix.found == len(want)
        assert jc.same_hits(ix.self_join_f64(3.0, cap=len(want)), want)  # the index stays usable; exact room is enough
        for _ in range(2):
            assert jc.same_hits(ix.search_f64(queries, 3.0), wq)
            assert jc.same_hits(ix.self_join_f64(3.0), want)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\)"):
            ix.search_f64(queries, 3.0, cap=1)
        assert ix.found == len(wq)
        empty = ix.self_join_f64(0.0, rows=(0, 0), cap=0)
        assert len(empty) == 0 and ix.found == 0
    finally:
        ix.close()


def test_more_rows_than_one_launch(gpu, rows_option):
    G = sedgpu.join_rows_per_group()
    plan, seqs, D = ref("costs15")
    N = 2 * (G + 1) + 3  # three launches of G + 1, G + 1 and 3 rows
    ix = index_of(gpu, plan, seqs[:N])
    try:
        rows_option(G + 1)
        for T in (1.0, INF):
            assert jc.same_hits(ix.self_join_f64(T), jf.expected_hits_f64(D[:N, :N], T, True))
            p = f64_plan(plan, seqs[:N], seqs[:N], True, T, {sedgpu.SED_OPT_JOIN_ROWS: G + 1})
            assert ix.pairs_run() == p["run"] and p["waves"] == 4 * (2 + 2 + 1)
        got = ix.search_f64(jc.packed_queries(plan, seqs[20:20 + N]), 2.0)
        assert jc.same_hits(got, jf.expected_hits_f64(D[20:20 + N, :N], 2.0))
        assert ix.last_ms() > 0
    finally:
        ix.close()


def test_costs_change_between_calls(gpu):
    plan, seqs, D = ref("costs15")
    table, al = jf.random16_table()
    other = jc.plan_for(table, al)  # the same first 15 codes under other costs
    Do = jc.oracle_matrix(other, [s for s in seqs[:60]], [s for s in seqs[:60]])
    ix = index_of(gpu, plan, seqs[:60])
    try:
        assert jc.same_hits(ix.self_join_f64(2.0), jf.expected_hits_f64(D[:60, :60], 2.0, True))
        gpu.set_costs(other)
        assert jc.same_hits(ix.self_join_f64(2.0), jf.expected_hits_f64(Do, 2.0, True))
        gpu.set_costs(plan)
        assert jc.same_hits(ix.self_join_f64(2.0), jf.expected_hits_f64(D[:60, :60], 2.0, True))
    finally:
        ix.close()


def test_refusals_and_errors(gpu):
    plan, seqs, _ = ref("costs15")
    ix = index_of(gpu, plan, seqs[:20])
    try:
        al17 = jf.AL16 + "Z"
        t17 = {"insert": 1.0, "delete": 1.0, "update": {a: {b: float(a != b) for b in al17} for a in al17}}
        neg = jc.plan_for(*jf.random16_table())
        neg.sub[2, 3] = -0.5
        for bad, why in ((jc.plan_for(t17, al17), r"17 symbols \(at most 16\)"), (neg, r"cost\(2 -> 3\) = -0\.5")):
            gpu.set_costs(bad)
            with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
                ix.self_join_f64(1.0)
            with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
                ix.search_f64(jc.packed_queries(plan, ["ACG"]), 1.0)
        gpu.set_costs(plan)
        for T in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\)"):
                ix.self_join_f64(T)
        q33 = sedgpu.PackedPairs([np.zeros(33, np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*33 symbols"):
            ix.search_f64(q33, 1.0)
        qk = sedgpu.PackedPairs([np.array([0, 15, 1], np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*row code.*K=15"):
            ix.search_f64(qk, 1.0)
        assert len(ix.self_join_f64(0.0)) >= 0  # still usable
    finally:
        ix.close()
    fresh = sedgpu.Context(gpu.device)
    try:
        ix2 = sedgpu.JoinIndex.from_seqs(fresh, jc.encode(plan, seqs[:4]))
        with pytest.raises(sedgpu.SedError, match=r"\(-6\).*sed_set_costs"):
            ix2.self_join_f64(1.0)
        ix2.close()
    finally:
        fresh.close()


def test_neighbors_auto_over_iupac_end_to_end(gpu):
    """wfsearch.neighbors over an ordinary IUPAC collection under costs.json, which the integer route refuses twice over,
    against the brute force of the definition: every pair through the C oracle, cut at 1.5."""
    wfsearch = jc.import_shim("wfsearch")
    seqs = jc.mixed_set(41, jf.IUPAC, 300)
    D = jc.oracle_matrix(jc.plan_for(jf.tables()["costs15"][0], jf.IUPAC), seqs, seqs)
    want = [(i, j, 1 / (1 + float(D[i, j]))) for i in range(300) for j in range(300) if i != j and D[i, j] <= 1.5]
    assert want and len({c for s in seqs for c in s}) == 15
    assert wfsearch.neighbors(seqs, 1.5, route="auto") == want
    assert wfsearch.neighbors(seqs, 1.5, route="f64") == want
    with pytest.raises(sedgpu.SedError, match="at most 8"):
        wfsearch.neighbors(seqs, 1.5)
