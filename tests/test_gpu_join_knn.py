"""GPU: the k nearest neighbours of every sequence (sed_join_knn_self / sed_join_knn_search and their _long_ twins)
against the expectation derived from the C oracle's distance matrix (join_knn_cases.expected_knn): the lists are equal
record for record, dist bit for bit; the per-row bounds and the candidate count equal the numpy model of the first pass
(join_knn_cases.pass1_model), which no schedule changes.  Both index types, both kernel variants."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_knn_cases as kc
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # name -> (plan, S, seqs, D): computed once, shared, never changed

INDEX = {"short": sedgpu.JoinIndex, "long": sedgpu.LongJoinIndex}


def _build(name):
    user = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN"), 4
    unit = jc.plan_for(jc.load_golden("costs.json"), "ACGU"), 1
    if name == "set1":       # random set 1: the scaled DP
        (plan, S), seqs = user, kc.random_set()
    elif name == "set2":     # random set 2: the unit table, bit-parallel
        (plan, S), seqs = unit, kc.random_set(301, 300, "ACGU", 0.0)
    elif name == "ties":
        (plan, S), seqs = unit, kc.tie_set()[0]
    elif name == "lone":
        (plan, S), seqs = unit, kc.lone_pair_set()
    elif name == "eighths":  # an asymmetric table
        table, al, S = jc.served_tables()["eighths"]
        plan, seqs = jc.plan_for(table, al), jc.mixed_set(88, al, 90)
    elif name == "mixed":    # lengths 0, 1, 2, 31, 32 among 20..32: empty sequences in the index
        (plan, S), seqs = user, jc.mixed_set(31, "ACGUN", 140, pn=0.01)
    elif name == "long dp":
        (plan, S), seqs = user, kc.long_set()
    elif name == "long bitpar":
        (plan, S), seqs = unit, kc.long_set(129, 300, "ACGU", 0.0)
    D = jc.oracle_matrix(plan, seqs, seqs)
    D.setflags(write=False)
    return plan, S, seqs, D


def ref(name):
    if name not in _REF:
        _REF[name] = _build(name)
    return _REF[name]


def index_of(gpu, plan, seqs, kind="short"):
    gpu.set_costs(plan)
    return INDEX[kind].from_seqs(gpu, jc.encode(plan, seqs))


@pytest.fixture
def options(gpu):
    yield gpu.set_option
    gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


def check_self(ix, D, lens, k, T, S, rows=None):
    """One self_knn call against the expectation and the model; returns the records."""
    lo, hi = (0, len(lens)) if rows is None else rows
    got = ix.self_knn(k, T, rows)
    want = kc.expected_knn(D[lo:hi], k, T, S, True, lo)
    assert jc.same_hits(got, want), (k, T, rows, len(got), len(want))
    bound, cand = kc.pass1_model(D[lo:hi], lens, k, T, S, True, lo)
    assert np.array_equal(ix.knn_bounds(), bound), (k, T, rows)
    assert ix.knn_candidates == cand, (k, T, rows)
    assert ix.found == len(want)
    return got


def a_short_cap(D, k, S):
    """A max_dist that leaves some rows short of k and others not: the median over the rows of the k-th nearest."""
    DS = kc.scaled(D, S) + np.diag(np.full(len(D), 1 << 20))
    return float(np.median(np.sort(DS, axis=1)[:, k - 1])) / S


@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_random_set_1(gpu, kind, k):
    """300 columns: 2 blocks, 5 waves, the last of 44 lanes (with k = 64 it never tightens a bound); the scaled DP."""
    plan, S, seqs, D = ref("set1")
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    assert sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, k, INF, kind == "long")["kernel"] == 1
    ix = index_of(gpu, plan, seqs, kind)
    try:
        T = a_short_cap(D, k, S)
        for cap in (INF, T, 0.0):
            got = check_self(ix, D, lens, k, cap, S)
            per_row = np.bincount(got["row"], minlength=len(seqs))
            if cap == INF:
                assert (per_row == k).all()
            elif cap == T:
                assert (per_row < k).any() and (per_row == k).any()
            assert not (got["row"] == got["col"]).any()
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_random_set_2_both_variants(gpu, options, kind):
    plan, S, seqs, D = ref("set2")
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    for forced, kernel in ((0, 2), (2, 1)):  # bit-parallel as planned, the scaled DP when forced
        assert sedgpu.join_knn_plan(jc.costs_of(plan), {sedgpu.SED_OPT_JOIN_DP: forced}, lens, lens, True, mask, mask, 8, INF,
                                    kind == "long")["kernel"] == kernel
    ix = index_of(gpu, plan, seqs, kind)
    try:
        for forced in (0, 2):
            options(sedgpu.SED_OPT_JOIN_DP, forced)
            for k in (1, 3, 8, 64):
                for cap in (INF, a_short_cap(D, k, S), 0.0):
                    check_self(ix, D, lens, k, cap, S)
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_ties_go_to_the_lowest_columns(gpu, kind):
    """70 copies of one sequence among 200 others, k = 8: every copy's row has more than k candidates at D = 0 from one
    wave; the lowest column indices win, and the row's own column is not among them."""
    plan, S, seqs, D = ref("ties")
    copies = kc.tie_set()[1]
    lens = [len(s) for s in seqs]
    ix = index_of(gpu, plan, seqs, kind)
    try:
        got = check_self(ix, D, lens, 8, INF, S)
        order = np.argsort(lens, kind="stable")
        assert max(sum(1 for c in order[w:w + 64] if c in copies) for w in range(0, len(seqs), 64)) > 9
        for i in copies:
            row = got[got["row"] == i]
            assert row["col"].tolist() == [c for c in copies if c != i][:8] and not row["dist"].any()
        assert ix.knn_candidates >= len(copies) * (len(copies) - 1)
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_nearest_is_not_self_and_comes_from_another_wave(gpu, kind):
    """130 columns of one length: waves of 64, 64 and 2.  Sequences 0 and 129 are one substitution apart."""
    plan, S, seqs, D = ref("lone")
    lens = [len(s) for s in seqs]
    ix = index_of(gpu, plan, seqs, kind)
    try:
        got = check_self(ix, D, lens, 1, INF, S)
        assert len(got) == len(seqs) and not (got["row"] == got["col"]).any()
        assert tuple(got[0]) == (0, 129, 1.0) and tuple(got[129]) == (129, 0, 1.0)
        # k = 2: for row 129 the last wave (columns 128 and 129) holds one column in scope, fewer than k, so it never
        # lowers the bound; the row's neighbours, column 0 first, come from the full waves
        got = check_self(ix, D, lens, 2, INF, S)
        assert got[got["row"] == 129]["col"][0] == 0
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_asymmetric_table_rows_follow_their_direction(gpu, kind):
    plan, S, seqs, D = ref("eighths")
    assert not np.array_equal(D, D.T)
    lens = [len(s) for s in seqs]
    ix = index_of(gpu, plan, seqs, kind)
    try:
        got = check_self(ix, D, lens, 3, INF, S)
        swapped = kc.expected_knn(D.T.copy(), 3, INF, S, True)
        assert not jc.same_hits(got, swapped)
        q = [4, 50, 77]
        gq = ix.search_knn(jc.packed_queries(plan, [seqs[i] for i in q]), 3)
        assert jc.same_hits(gq, kc.expected_knn(D[q], 3, INF, S))
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_geometry_and_search(gpu, options, kind):
    plan, S, seqs, D = ref("mixed")
    assert "" in seqs
    lens = [len(s) for s in seqs]
    ix = index_of(gpu, plan, seqs, kind)
    try:
        for k in (1, 5):
            check_self(ix, D, lens, k, INF, S, rows=(7, 19))
            whole = check_self(ix, D, lens, k, 9.0, S)
            options(sedgpu.SED_OPT_JOIN_ROWS, 4)  # 35 launches
            assert jc.same_hits(check_self(ix, D, lens, k, 9.0, S), whole)
            options(sedgpu.SED_OPT_JOIN_ROWS, 0)
        top = "ACGU" * (32 if kind == "long" else 8)
        queries = ["", top, seqs[11], seqs[11], "ACG"]
        Dq = jc.oracle_matrix(plan, queries, seqs)
        for k, T in ((1, INF), (4, INF), (4, 12.0), (64, INF)):
            got = ix.search_knn(jc.packed_queries(plan, queries), k, T)
            assert jc.same_hits(got, kc.expected_knn(Dq, k, T, S)), (k, T)
            bound, cand = kc.pass1_model(Dq, lens, k, T, S)
            assert np.array_equal(ix.knn_bounds(), bound) and ix.knn_candidates == cand
        dup = ix.search_knn(jc.packed_queries(plan, [seqs[11]]), 1)
        assert dup["dist"][0] == 0.0 and seqs[int(dup["col"][0])] == seqs[11]  # a search reports the sequence itself
        assert ix.last_ms() > 0 and 0 < ix.knn_bound_ms() <= ix.last_ms()
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_empty_index_and_empty_ranges(gpu, kind):
    plan, S, seqs, D = ref("mixed")
    ix = index_of(gpu, plan, [], kind)
    try:
        assert len(ix.self_knn(3)) == 0 and ix.knn_candidates == 0 and len(ix.knn_bounds()) == 0
        got = ix.search_knn(jc.packed_queries(plan, ["ACG", ""]), 3, 2.0)
        assert len(got) == 0 and ix.knn_bounds().tolist() == [8, 8] and ix.knn_candidates == 0
    finally:
        ix.close()
    ix = index_of(gpu, plan, seqs[:10], kind)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-6\)"):
            ix.knn_bounds()  # no k-nearest call yet
        with pytest.raises(sedgpu.SedError, match=r"\(-6\)"):
            ix.knn_candidates
        assert len(ix.self_knn(3, rows=(4, 4))) == 0 and len(ix.knn_bounds()) == 0
        one = ix.self_knn(64)  # fewer columns than k
        assert jc.same_hits(one, kc.expected_knn(D[:10, :10], 64, INF, S, True)) and len(one) == 90
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_cap_protocol_and_refusals(gpu, kind):
    plan, S, seqs, D = ref("set1")
    want = kc.expected_knn(D, 3, INF, S, True)
    ix = index_of(gpu, plan, seqs, kind)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap 0" % len(want)):
            ix.self_knn(3, cap=0)  # the count query
        assert ix.found == len(want) == 900
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found 900 hits, cap 899"):
            ix.self_knn(3, cap=899)
        assert ix.found == 900
        assert jc.same_hits(ix.self_knn(3, cap=900), want)  # the index still answers; exact room is enough
        assert jc.same_hits(ix.self_join(2.0), jc.expected_hits(D, 2.0, S, True))  # joins and k-nearest calls alternate
        assert jc.same_hits(ix.self_knn(3), want)
        for k in (0, 65, -1):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d " % k):
                ix.self_knn(k)
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d " % k):
                ix.search_knn(jc.packed_queries(plan, ["ACG"]), k)
        for T in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*max_dist"):
                ix.self_knn(3, T)
        qk = sedgpu.PackedPairs([np.array([0, 5, 1], np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*row code.*K=5"):
            ix.search_knn(qk, 3)
        table, al, why = jc.refused_tables()["N at 0.66"]
        gpu.set_costs(jc.plan_for(table, al))
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
            ix.self_knn(3)
        gpu.set_costs(plan)
        assert jc.same_hits(ix.self_knn(3), want)
    finally:
        ix.close()
    fresh = sedgpu.Context(gpu.device)
    try:
        ix2 = INDEX[kind].from_seqs(fresh, jc.encode(plan, seqs[:4]))
        with pytest.raises(sedgpu.SedError, match=r"\(-6\).*sed_set_costs"):
            ix2.self_knn(1)
        ix2.close()
    finally:
        fresh.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_undersized_device_list_grows(gpu, kind):
    """A fresh index: a small call sizes the device list, then a call whose candidates (the copies' ties: over 4 800)
    exceed the room made for 2 k records a row: the second pass runs again and the result is whole."""
    plan, S, seqs, D = ref("ties")
    lens = [len(s) for s in seqs]
    ix = index_of(gpu, plan, seqs, kind)
    try:
        check_self(ix, D, lens, 1, INF, S, rows=(0, 4))
        _, cand = kc.pass1_model(D, lens, 1, INF, S, True)
        assert cand > 2 * len(seqs) + 1024
        check_self(ix, D, lens, 1, INF, S)
        assert ix.pairs_run() <= 2 * len(seqs) * (len(seqs) - 1)  # the repeated second pass is not counted
        check_self(ix, D, lens, 1, INF, S)
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["long dp", "long bitpar"])
def test_long_index_across_the_block_edges(gpu, name):
    """Lengths straddling 32 / 64 / 96 / 128: waves of 1..4 column blocks, 300 columns."""
    plan, S, seqs, D = ref(name)
    lens = [len(s) for s in seqs]
    order = np.sort(lens)
    assert {(int(order[min(w + 63, len(order) - 1)]) + 31) // 32 for w in range(0, len(order), 64)} >= {1, 2, 3, 4} and order[0] == 0
    mask = jc.codes_mask(plan, seqs)
    kernel = sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, 8, INF, True)["kernel"]
    assert kernel == (1 if name == "long dp" else 2)
    ix = index_of(gpu, plan, seqs, "long")
    try:
        for k in (1, 8):
            check_self(ix, D, lens, k, INF, S)
            check_self(ix, D, lens, k, a_short_cap(D, k, S), S)
        q = [0, 17, 150, 299]
        got = ix.search_knn(jc.packed_queries(plan, [seqs[i] for i in q]), 8)
        assert jc.same_hits(got, kc.expected_knn(D[q], 8, INF, S))
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_pruning_is_real(gpu, kind):
    """Random set 1, k = 3, no cap: both passes together run fewer than twice the pairs in scope, and the second pass
    appends fewer candidates than there are pairs in scope (tests/test_join_knn_host.py checks both in the model)."""
    plan, S, seqs, D = ref("set1")
    lens = [len(s) for s in seqs]
    scope = len(seqs) * (len(seqs) - 1)
    ix = index_of(gpu, plan, seqs, kind)
    try:
        check_self(ix, D, lens, 3, INF, S)
        bound = ix.knn_bounds()
        p2 = kc.pass2_pairs(lens, lens, bound, plan.ins, plan.dele, S, True)
        assert p2 < ix.pairs_run() < 2 * scope
        assert ix.pairs_run() <= scope + p2
        assert ix.knn_candidates < scope
    finally:
        ix.close()


def test_python_layers_end_to_end(gpu):
    wfsearch = jc.import_shim("wfsearch")
    plan, S, seqs, D = ref("set1")
    sub = seqs[:80]
    want = kc._nearest(D[:80, :80], 8, None, True)
    got = wfsearch.nearest_neighbors(sub, 8, user_cost=True)
    assert got == [[(j, 1 / (1 + d)) for i, j, d in want if i == r] for r in range(80)]
    lng = wfsearch.nearest_neighbors(sub, 8, user_cost=True, long_sequences=True)
    assert lng == got
    ix = wfsearch.JoinIndex(sub, True)
    try:
        many = ix.nearest_many([sub[5], ""], 2, 30.0)
        wq = kc._nearest(jc.oracle_matrix(plan, [sub[5], ""], sub), 2, 30.0)
        assert many == [[(sub[j], 1 / (1 + d)) for q, j, d in wq if q == r] for r in range(2)]
    finally:
        ix.close()
