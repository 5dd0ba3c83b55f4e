"""GPU: the k nearest neighbours on the fp64 route (sed_join_knn_self_f64 / sed_join_knn_search_f64) against the C
oracle's fp64 matrix: the records are equal one for one, dist bit for bit; the per-row bounds and the candidate count
are those of the definition (join_knn_f64_cases.pass1_by_definition), which no schedule changes.  The pairs run: pass 2
runs exactly the pairs whose table entry is <= the row's final bound (p2); a lane of pass 1 goes when its entry is <=
the bound it read, which lies between the final bound and max_dist, so pass 1 runs between p2 and the fp64 join's
plan at max_dist (run): 2 p2 <= pairs_run <= run + p2, and where the skip removes nothing all three are equal."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_f64_cases as jf
import join_knn_cases as kc
import join_knn_f64_cases as kf
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
KS = (1, 2, 8, 63, 64)


def index_of(gpu, c, ncols=None):
    gpu.set_costs(c.plan)
    return sedgpu.JoinIndex.from_seqs(gpu, jc.encode(c.plan, c.seqs[:ncols]))


@pytest.fixture
def options(gpu):
    yield gpu.set_option
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


def check(ix, c, D, len_rows, k, T, self_join, row_lo, call, ncols=None, reruns=False):
    """One call against the oracle: records, bounds, candidates, pairs run; returns (the records, the bounds)."""
    lens = c.lens[:ncols]
    got = call()
    want = kf.expected_knn(D, k, T, self_join, row_lo)
    assert jc.same_hits(got, want), (k, T, len(got), len(want))
    assert ix.found == len(want)
    bound, cand = kf.pass1_by_definition(D, lens, k, T, self_join, row_lo)
    assert np.array_equal(ix.knn_bounds_f64().view(np.uint64), bound.view(np.uint64)), (k, T)
    assert ix.knn_candidates == cand, (k, T)
    ok = kc.in_scope(D.shape, self_join, row_lo)
    p2 = kf.emit_pass_model(D, ok, len_rows, lens, c.low, bound)[1]
    run = kf.pairs_at(ok, len_rows, lens, c.low, T)
    print("k %d T %r: pairs_run %d, 2 p2 %d, run + p2 %d, candidates %d" % (k, T, ix.pairs_run(), 2 * p2, run + p2, cand))
    assert 2 * p2 <= ix.pairs_run() <= run + p2, (k, T)
    return got, bound


def check_self(ix, c, k, T, rows=None, ncols=None):
    lo, hi = (0, len(c.seqs[:ncols])) if rows is None else rows
    D = c.D[lo:hi, :len(c.seqs[:ncols])]
    return check(ix, c, D, c.lens[lo:hi], k, T, True, lo, lambda: ix.self_knn_f64(k, T, rows), ncols)


def check_search(ix, c, q, k, T):
    packed = jc.packed_queries(c.plan, [c.seqs[i] for i in q])
    return check(ix, c, c.D[q], [c.lens[i] for i in q], k, T, False, 0, lambda: ix.search_knn_f64(packed, k, T))


def realised(c, k):
    """A realised distance: the middle one of the rows' k-th nearest (the row it belongs to falls short of k below it)."""
    D = c.D + np.diag(np.full(len(c.D), INF))
    kth = np.sort(np.sort(D, axis=1)[:, min(k, len(D) - 1) - 1])
    return float(kth[len(kth) // 2])


@pytest.mark.parametrize("name", ["random N", "iupac"])
@pytest.mark.parametrize("k", KS)
def test_random_sets(gpu, name, k):
    """300 columns: 2 blocks, 5 waves, the last of 44 lanes.  ACGU with 1 % N, and all 15 IUPAC codes, which the integer
    route refuses; rows of all, 1, 4 and 5; self joins and searches; +inf, 0, a realised distance and the double below."""
    c = kf.case(name)
    if name == "iupac":
        mask = jc.codes_mask(c.plan, c.seqs)
        with pytest.raises(sedgpu.SedError, match="15 symbols"):
            sedgpu.join_knn_plan(jc.costs_of(c.plan), {}, c.lens, c.lens, True, mask, mask, k, INF)
    ix = index_of(gpu, c)
    try:
        d = realised(c, k)
        assert d > 0
        for T in (INF, 0.0, d, float(np.nextafter(d, 0.0))):
            got, _ = check_self(ix, c, k, T)
            assert not (got["row"] == got["col"]).any()
            if T == INF:
                assert (np.bincount(got["row"], minlength=len(c.seqs)) == k).all()
        at, below = (len(ix.self_knn_f64(k, T)) for T in (d, float(np.nextafter(d, 0.0))))
        assert below < at
        for rows in ((17, 18), (100, 104), (295, 300)):
            check_self(ix, c, k, INF, rows)
            check_self(ix, c, k, d, rows)
        q = [0, 63, 64, 299, 150]
        for T in (INF, d, 0.0):
            got, _ = check_search(ix, c, q, k, T)
            if T == 0.0:
                assert got["col"][got["row"] == 0][0] == 0  # a search reports the sequence itself
        check_search(ix, c, q[:1], k, INF)
    finally:
        ix.close()


def test_k_greater_than_the_columns_in_scope(gpu):
    c = kf.case("iupac")
    ix = index_of(gpu, c, 10)
    try:
        for k in (9, 10, 64):
            got, bound = check_self(ix, c, k, INF, ncols=10)
            assert len(got) == 90 and ((bound == INF).all() if k > 9 else (bound < INF).all())
        packed = jc.packed_queries(c.plan, c.seqs[20:23])
        got = ix.search_knn_f64(packed, 64)
        assert jc.same_hits(got, kf.expected_knn(c.D[20:23, :10], 64, INF)) and len(got) == 30
    finally:
        ix.close()


def test_ties_at_the_kth_place_go_to_the_lowest_columns(gpu):
    """70 copies of one sequence among 200 others: more than k candidates at D = 0 from several waves."""
    c = kf.case("ties")
    copies = kc.tie_set()[1]
    ix = index_of(gpu, c)
    try:
        for k in (8, 64):
            got, bound = check_self(ix, c, k, INF)
            for i in copies:
                row = got[got["row"] == i]
                assert row["col"].tolist()[:min(k, 69)] == [x for x in copies if x != i][:k]
            assert k == 64 or all(bound[i] == 0 for i in copies)  # (no wave holds 64 copies)
        assert ix.knn_candidates >= len(copies) * (len(copies) - 1)
    finally:
        ix.close()


def test_order_rests_on_the_last_bits(gpu):
    """0.2 + 0.1 != 0.3: rows with two distances that differ within 1e-12 relative, asserted from the oracle."""
    c = kf.case("near ties")
    rows = [r for r in range(len(c.seqs)) for v in [np.unique(np.delete(c.D[r], r))]
            if ((np.diff(v) > 0) & (np.diff(v) <= 1e-12 * v[1:])).any()]
    assert len(rows) >= 10
    ix = index_of(gpu, c)
    try:
        for k in (1, 2, 8):
            got, _ = check_self(ix, c, k, INF)
        for T in (0.3, 0.30000000000000004, float(np.nextafter(0.3, 0))):
            check_self(ix, c, 2, T)
        one = ix.self_knn_f64(1, 0.30000000000000004)
        assert {0.3, 0.30000000000000004} <= set(one["dist"].tolist())
        check_search(ix, c, rows[:5], 2, INF)
    finally:
        ix.close()


def test_overflowed_distances_are_ordinary_values(gpu):
    c = kf.case("overflow")
    ix = index_of(gpu, c)
    try:
        for k in (1, 8, 64):
            got, bound = check_self(ix, c, k, INF)
            assert (np.bincount(got["row"], minlength=len(c.seqs)) == k).all()
        assert np.isinf(got["dist"]).any() and np.isinf(bound).any()
        got, _ = check_self(ix, c, 8, 1.7976931348623157e308)  # the largest double leaves +inf out
        assert np.isfinite(got["dist"]).all() and (np.bincount(got["row"], minlength=len(c.seqs)) < 8).any()
        check_search(ix, c, [0, 5, 139], 8, INF)
    finally:
        ix.close()


def test_all_zero_table_every_distance_ties(gpu):
    c = kf.case("zero")
    assert not c.D.any()
    ix = index_of(gpu, c)
    try:
        for k in (1, 8, 64):
            got, bound = check_self(ix, c, k, INF)
            assert not bound.any() and got["col"][got["row"] == 5].tolist() == [x for x in range(k + 1) if x != 5][:k]
        check_self(ix, c, 8, 0.0)
        assert ix.knn_candidates == len(c.seqs) * (len(c.seqs) - 1)
    finally:
        ix.close()


def test_the_lower_bound_table_skips_whole_waves(gpu, options):
    """Lengths spread over 0..32, insert != delete, empty sequences: pass 2 leaves whole (wave, row)s out, some bounds end
    below max_dist, and under a cap some waves have fewer than k columns within it."""
    c = kf.case("spread")
    ok = kc.in_scope(c.D.shape, True, 0)
    ix = index_of(gpu, c)
    try:
        for k, T in ((8, INF), (8, 1.0), (3, 0.65), (64, INF)):
            got, bound = check_self(ix, c, k, T)
            _, p2, skipped = kf.emit_pass_model(c.D, ok, c.lens, c.lens, c.low, bound)
            if k != 64:
                assert skipped > 0 and (bound < T).any() and p2 < len(c.seqs) * (len(c.seqs) - 1)
        _, bound = check_self(ix, c, 3, 0.65)
        assert (bound == 0.65).any() and (bound < 0.65).any()
        empties = [i for i, n in enumerate(c.lens) if n == 0]
        check_search(ix, c, empties[:2] + [c.lens.index(32), 7, 8], 8, INF)
        # SED_OPT_JOIN_ROWS = 4: launches of one row group each
        whole, _ = check_self(ix, c, 8, 1.0)
        options(sedgpu.SED_OPT_JOIN_ROWS, 4)
        again, _ = check_self(ix, c, 8, 1.0)
        assert jc.same_hits(again, whole)
        check_self(ix, c, 2, INF, rows=(3, 16))
        check_search(ix, c, list(range(9)), 2, 1.0)
    finally:
        ix.close()


def test_cap_protocol_refusals_and_alternating_calls(gpu):
    c = kf.case("random N")
    S = 4
    want = kf.expected_knn(c.D, 3, INF, True)
    ix = index_of(gpu, c)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-6\)"):
            ix.knn_bounds_f64()  # no k-nearest call yet
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap 0" % len(want)):
            ix.self_knn_f64(3, cap=0)  # the count query
        assert ix.found == len(want) == 900
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found 900 hits, cap 899"):
            ix.self_knn_f64(3, cap=899)
        assert ix.found == 900
        assert jc.same_hits(ix.self_knn_f64(3, cap=900), want)  # the index still answers; exact room is enough
        # calls of every kind alternate on one index; each bounds call answers for its own route only
        assert jc.same_hits(ix.self_knn(3), kc.expected_knn(c.D, 3, INF, S, True))
        assert len(ix.knn_bounds()) == 300
        with pytest.raises(sedgpu.SedError, match=r"\(-6\)"):
            ix.knn_bounds_f64()
        assert jc.same_hits(ix.self_join_f64(2.0), jf.expected_hits_f64(c.D, 2.0, True))
        assert jc.same_hits(ix.self_knn_f64(3), want)
        assert len(ix.knn_bounds_f64()) == 300
        with pytest.raises(sedgpu.SedError, match=r"\(-6\)"):
            ix.knn_bounds()
        assert jc.same_hits(ix.self_join(2.0), jc.expected_hits(c.D, 2.0, S, True))
        assert jc.same_hits(ix.self_knn_f64(3, -0.0), kf.expected_knn(c.D, 3, 0.0, True))  # -0.0 counts as 0
        assert ix.last_ms() > 0 and 0 < ix.knn_bound_ms() <= ix.last_ms()
        for k in (0, 65, -1):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d " % k):
                ix.self_knn_f64(k, math.nan)
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d " % k):
                ix.search_knn_f64(jc.packed_queries(c.plan, ["ACG"]), k)
        for T in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*max_dist"):
                ix.self_knn_f64(3, T)
        qk = sedgpu.PackedPairs([np.array([0, 5, 1], np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*row code.*K=5"):
            ix.search_knn_f64(qk, 3)
        neg, al = kf.flat_table(1.0, dele=-2.0)
        gpu.set_costs(jc.plan_for(neg, al))
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*delete = -2 is not a finite cost"):
            ix.self_knn_f64(3)
        gpu.set_costs(c.plan)
        assert jc.same_hits(ix.self_knn_f64(3), want)
        # a call that launches nothing reports max_dist for every row
        assert len(ix.self_knn_f64(3, 2.5, rows=(4, 4))) == 0 and len(ix.knn_bounds_f64()) == 0
    finally:
        ix.close()
    empty = sedgpu.JoinIndex.from_seqs(gpu, [])
    try:
        got = empty.search_knn_f64(jc.packed_queries(c.plan, ["ACG", ""]), 3, 2.5)
        assert len(got) == 0 and empty.knn_bounds_f64().tolist() == [2.5, 2.5] and empty.knn_candidates == 0
    finally:
        empty.close()
    fresh = sedgpu.Context(gpu.device)
    try:
        ix2 = sedgpu.JoinIndex.from_seqs(fresh, jc.encode(c.plan, c.seqs[:4]))
        with pytest.raises(sedgpu.SedError, match=r"\(-6\).*sed_set_costs"):
            ix2.self_knn_f64(1)
        ix2.close()
    finally:
        fresh.close()


def test_undersized_device_list_grows(gpu):
    """A fresh index: a small call sizes the device list, then a call whose candidates (the copies' ties: over 4 800)
    exceed the room made for 2 k records a row: pass 2 runs again (not counted in the pairs) and the result is whole."""
    c = kf.case("ties")
    ix = index_of(gpu, c)
    try:
        check_self(ix, c, 1, INF, rows=(0, 4))
        _, cand = kf.pass1_by_definition(c.D, c.lens, 1, INF, True)
        assert cand > 2 * len(c.seqs) + 1024
        check_self(ix, c, 1, INF)
        check_self(ix, c, 1, INF)
    finally:
        ix.close()


def test_python_layers_end_to_end(gpu):
    wfsearch = jc.import_shim("wfsearch")
    c = kf.case("iupac")
    sub = c.seqs[:80]
    want = kc._nearest(c.D[:80, :80], 8, None, True)
    want = [[(j, 1 / (1 + d)) for i, j, d in want if i == r] for r in range(80)]
    assert wfsearch.nearest_neighbors(sub, 8, route="f64") == want
    assert wfsearch.nearest_neighbors(sub, 8, route="auto") == want
    with pytest.raises(sedgpu.SedError):
        wfsearch.nearest_neighbors(sub, 8)
