"""CPU: the k-nearest calls' device-free half - the trim (sed_join_knn_trim), k's validation through the planner
(sed_join_knn_plan), the numpy model of the first pass on the GPU tests' inputs, and the Python layers
(StringEditDistance.JoinIndex.self_nearest / search_nearest, wfsearch.JoinIndex.nearest / nearest_many /
nearest_neighbors, sedshard.nearest_neighbors) over oracle-backed engines."""
import math
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

import join_cases as jc
import join_knn_cases as kc
import sedgpu
import sedshard

INF = math.inf


@pytest.fixture(scope="module")
def wfsearch():
    return jc.import_shim("wfsearch")


def recs(rows):
    out = np.zeros(len(rows), sedgpu.JOIN_HIT_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


# ---- the trim ----

def test_trim_breaks_ties_at_the_kth_place_by_column():
    hits = recs([(0, 9, 1.0), (0, 4, 1.0), (0, 7, 0.5), (0, 2, 1.0), (0, 5, 2.0), (1, 3, 0.0), (1, 1, 0.0), (1, 2, 0.0)])
    got = sedgpu.join_knn_trim(hits, 3)
    assert got.tolist() == [(0, 7, 0.5), (0, 2, 1.0), (0, 4, 1.0), (1, 1, 0.0), (1, 2, 0.0), (1, 3, 0.0)]
    assert sedgpu.join_knn_trim(hits, 2).tolist() == [(0, 7, 0.5), (0, 2, 1.0), (1, 1, 0.0), (1, 2, 0.0)]
    assert len(hits) == 8 and hits[0]["col"] == 9  # the caller's array is not touched


def test_trim_rows_with_fewer_than_k_and_empty_input():
    hits = recs([(5, 1, 3.0), (2, 8, 1.0), (2, 0, 4.0), (9, 9, 0.25)])
    assert sedgpu.join_knn_trim(hits, 3).tolist() == [(2, 8, 1.0), (2, 0, 4.0), (5, 1, 3.0), (9, 9, 0.25)]
    assert len(sedgpu.join_knn_trim(recs([]), 8)) == 0


@pytest.mark.parametrize("k", [1, 64])
def test_trim_k_1_and_64_on_shuffled_input(k):
    rng = np.random.default_rng(k)
    rows = [(r, c, float(rng.integers(0, 12)) / 4) for r in range(7) for c in range(100) if c != r]
    want = []
    for r in range(7):
        want += sorted([h for h in rows if h[0] == r], key=lambda h: (h[2], h[1]))[:k]
    for _ in range(3):
        shuffled = [rows[i] for i in rng.permutation(len(rows))]
        assert sedgpu.join_knn_trim(recs(shuffled), k).tolist() == want


def test_trim_refuses_bad_arguments():
    for k in (0, 65, -1):
        with pytest.raises(sedgpu.SedError) as e:
            sedgpu.join_knn_trim(recs([(0, 1, 1.0)]), k)
        assert e.value.code == -1
    with pytest.raises(sedgpu.SedError):
        sedgpu.join_knn_trim(recs([(0, 1, math.nan)]), 1)


# ---- k through the planner, without a device ----

@pytest.mark.parametrize("long_index", [False, True])
def test_planner_refuses_k_outside_1_to_64(long_index):
    plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN")
    lens = [5, 20, 32]
    mask = sedgpu.codes_seen(np.arange(5, dtype=np.uint8))
    for k in (0, 65, -1):
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d .*1\.\.64" % k) as e:
            sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, k, INF, long_index)
        assert e.value.code == -1
    # k comes first, then the join's refusals in their order, then the join's own plan
    with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = 0"):
        sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, 0, math.nan, long_index)
    with pytest.raises(sedgpu.SedError, match=r"\(-1\).*max_dist is NaN or negative"):
        sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, 1, math.nan, long_index)
    table, al, why = jc.refused_tables()["N at 0.66"]
    with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
        sedgpu.join_knn_plan(jc.costs_of(jc.plan_for(table, al)), {}, lens, lens, True, mask, mask, 64, INF, long_index)
    join = (sedgpu.join_long_plan if long_index else sedgpu.join_plan)(jc.costs_of(plan), {}, lens, lens, True, mask, mask, 2.0)
    for k in (1, 64):
        assert sedgpu.join_knn_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, k, 2.0, long_index) == join
    with pytest.raises(sedgpu.SedError, match=r"33 symbols" if not long_index else r"129 symbols"):
        sedgpu.join_knn_plan(jc.costs_of(plan), {}, [129 if long_index else 33], lens, False, mask, mask, 1, INF, long_index)


# ---- the model of pass 1 on the GPU tests' first set: pruning is real there ----

def test_model_prunes_on_random_set_1():
    """What tests/test_gpu_join_knn.py::test_pruning_is_real asks of the device holds in the model: with k = 3 and no
    cap, pass 2 alone runs fewer pairs than are in scope (so both passes run fewer than twice as many, whatever pass 1
    skips) and the candidates are fewer than the pairs in scope."""
    plan, S = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN"), 4
    seqs = kc.random_set()
    lens = [len(s) for s in seqs]
    D = jc.oracle_matrix(plan, seqs, seqs)
    scope = len(seqs) * (len(seqs) - 1)
    bound, cand = kc.pass1_model(D, lens, 3, INF, S, True)
    assert (bound < kc.CUT_ALL).all()
    assert 3 * len(seqs) <= cand < scope
    assert kc.pass2_pairs(lens, lens, bound, plan.ins, plan.dele, S, True) < scope
    # k = 64: the last wave holds 44 columns and never tightens; the bound is still the minimum over the full waves
    b64, _ = kc.pass1_model(D, lens, 64, INF, S, True)
    order = np.argsort(lens, kind="stable")
    DS = kc.scaled(D, S)
    for r in (0, 151, 299):
        full = [np.sort(DS[r, [c for c in order[w:w + 64] if c != r]]) for w in range(0, 256, 64)]
        assert b64[r] == min(v[63] for v in full if len(v) >= 64)
    assert len(kc.expected_knn(D, 64, INF, S, True)) == 64 * len(seqs)


def test_expected_list_orders_ties_by_column():
    seqs, copies = kc.tie_set()
    plan = jc.plan_for(jc.load_golden("costs.json"), "ACGU")
    D = jc.oracle_matrix(plan, seqs, seqs)
    want = kc.expected_knn(D, 8, INF, 1, True)
    for i in copies[:3] + copies[-2:]:
        row = want[want["row"] == i]
        assert row["col"].tolist() == [c for c in copies if c != i][:8] and not row["dist"].any()
    bound, cand = kc.pass1_model(D, [len(s) for s in seqs], 8, INF, 1, True)
    assert all(bound[i] == 0 for i in copies) and cand >= len(copies) * (len(copies) - 1)


# ---- the shim over a codes-level oracle engine ----

@pytest.mark.parametrize("long_seqs", [False, True])
def test_shim_self_nearest_and_search_nearest(long_seqs):
    SED = jc.import_shim("StringEditDistance")
    seqs = (kc.long_set(5, 40) if long_seqs else kc.random_set(5, 40)) + ["", "ACGU"]
    plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, seqs, seqs)
    ix = SED.join_index(seqs, True, engine=kc.CodesEngine, long_seqs=long_seqs)
    assert kc.CodesEngine.built[-1].kw == ({"long_seqs": True} if long_seqs else {})
    N = len(seqs)
    for k, T in ((1, None), (5, None), (64, None), (5, 20.0), (3, 0)):
        want = kc._nearest(D, k, T, True)
        got = ix.self_nearest(k, T)
        assert got == want
        assert all(i != j for i, j, _ in got)
        per_row = [[h for h in got if h[0] == i] for i in range(N)]
        assert all(len(r) == min(k, N - 1) for r in per_row) if T is None else any(len(r) < k for r in per_row)
        assert all([d for _, _, d in r] == sorted(d for _, _, d in r) for r in per_row)  # nearest first
        assert ix.self_nearest(k, T, rows=(7, 19)) == [h for h in want if 7 <= h[0] < 19]
    assert ix.self_nearest(3, None, rows=(4, 4)) == []
    ncalls = len(ix._dev.calls)
    for k in (0, 65, -1, 2.0, True):  # refused before the engine, also where the engine would not be reached
        for call in (lambda: ix.self_nearest(k), lambda: ix.self_nearest(k, rows=(4, 4)),
                     lambda: ix.search_nearest(["ACG"], k), lambda: ix.search_nearest([], k)):
            with pytest.raises(sedgpu.SedError, match=r"k = .* \(1\.\.64\)"):
                call()
    assert len(ix._dev.calls) == ncalls
    assert ix._dev.calls[0] == ("self_knn", 1, INF, (0, N))  # None reaches the engine as +inf
    queries = [seqs[3], "", seqs[9][:-1] + "A", "ACGU"]
    Dq = jc.oracle_matrix(plan, queries, seqs)
    for k, T in ((1, None), (4, None), (4, 6.5)):
        assert ix.search_nearest(queries, k, T) == kc._nearest(Dq, k, T)
    assert ix.search_nearest([], 3) == []
    with pytest.raises(sedgpu.SedError, match=r"query 0 has %d symbols" % (ix.max_len + 1)):
        ix.search_nearest(["A" * (ix.max_len + 1)], 1)
    with pytest.raises(ValueError, match="no range"):
        ix.self_nearest(1, rows=(3, N + 1))
    ix.close()


def test_shim_f64_index_runs_the_integer_calls():
    SED = jc.import_shim("StringEditDistance")
    seqs = kc.random_set(6, 12)
    ix = SED.join_index(seqs, True, engine=kc.CodesEngine, f64=True)
    ix.self_nearest(2)
    ix.search_nearest(seqs[:2], 2, 3.0)
    assert [c[0] for c in ix._dev.calls] == ["self_knn", "search_knn"]


# ---- wfsearch over the oracle engine ----

@pytest.mark.parametrize("user,long_sequences", [(False, False), (True, False), (True, True)])
def test_wfsearch_nearest(wfsearch, user, long_sequences):
    seqs = kc.long_set(8, 50) if long_sequences else kc.random_set(8, 50)
    plan = jc.plan_for(jc.load_golden("user_costs.json" if user else "costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, seqs, seqs)
    N = len(seqs)
    ix = wfsearch.JoinIndex(seqs, user, index_fn=kc.OracleEngine, long_sequences=long_sequences)
    assert kc.OracleEngine.built[-1].kw == ({"long_seqs": True} if long_sequences else {})
    for k, T in ((1, None), (8, None), (8, 20.0 if user else 12.0), (2, 0)):
        want = [[(j, 1 / (1 + d)) for _, j, d in kc._nearest(D[i:i + 1], k, T, True, i)] for i in range(N)]
        got = ix.nearest(k, T)
        assert got == want and len(got) == N
        assert all([s for _, s in r] == sorted((s for _, s in r), reverse=True) for r in got)  # the best score first
        if T is None:
            assert all(len(r) == k for r in got)
        else:
            assert any(len(r) < k for r in got)  # max_dist is a cap
        assert ix.nearest(k, T, rows=(7, 19)) == want[7:19]
        assert wfsearch.nearest_neighbors(seqs, k, T, user, index_fn=kc.OracleEngine, long_sequences=long_sequences) == want
        assert kc.OracleEngine.built[-1].closed
    queries = [seqs[3], "", seqs[9][:-1] + "A"]
    Dq = jc.oracle_matrix(plan, queries, seqs)
    for k, T in ((1, None), (5, None), (5, 10.0)):
        want = [[(seqs[j], 1 / (1 + d)) for _, j, d in kc._nearest(Dq[q:q + 1], k, T)] for q in range(len(queries))]
        assert ix.nearest_many(queries, k, T) == want
    assert ix.nearest_many([], 3) == []
    ix.close()
    assert wfsearch.nearest_neighbors([], 3, index_fn=kc.OracleEngine) == []
    empty = wfsearch.JoinIndex([], index_fn=kc.OracleEngine)
    assert empty.nearest_many(["ACG"], 2) == [[]]
    for call in (lambda: empty.nearest(0), lambda: empty.nearest_many(["ACG"], 65)):
        with pytest.raises(sedgpu.SedError, match=r"k = "):
            call()
    with pytest.raises(ValueError, match="no range"):
        empty.nearest(1, rows=(0, 1))


# ---- sedshard.nearest_neighbors ----

def _oracle_knn(seqs, lo, hi, k, max_dist, user, long_seqs=False):
    return kc.OracleEngine(seqs, user).self_nearest(k, max_dist, (lo, hi))


def _oracle_knn_long(seqs, lo, hi, k, max_dist, user, long_seqs=False):
    assert long_seqs is True
    return kc.OracleEngine(seqs, user).self_nearest(k, max_dist, (lo, hi))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, seqs, k, T, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = sedshard.nearest_neighbors(seqs, k, T, True, world=world, rank=rank, join_fn=_oracle_knn)
    if rank == 0:
        q.put((got["row"].tolist(), got["col"].tolist(), got["dist"].tolist()))
    else:
        assert got is None
    dist.destroy_process_group()


def test_sharded_nearest_world_3_reassembles_world_1():
    seqs = kc.random_set(9, 11)
    plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, seqs, seqs)
    k, T = 3, 20.0
    want = kc.expected_knn(D, k, T, 4, True)
    assert len(seqs) < len(want) < k * len(seqs)  # the cap leaves some rows short
    one = sedshard.nearest_neighbors(seqs, k, T, True, join_fn=_oracle_knn)
    assert jc.same_hits(one, want)
    assert jc.same_hits(sedshard.nearest_neighbors(seqs, k, None, True, join_fn=_oracle_knn), kc.expected_knn(D, k, INF, 4, True))
    lng = sedshard.nearest_neighbors(seqs, k, T, True, join_fn=_oracle_knn_long, long_sequences=True)
    assert jc.same_hits(lng, want)
    world = 3
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, seqs, k, T, q)) for r in range(world)]
    for p in procs:
        p.start()
    rows, cols, dist = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert (rows, cols, dist) == (want["row"].tolist(), want["col"].tolist(), want["dist"].tolist())


# ---- the envelope (tests/test_gpu_join_knn_envelope.py): its calls proved on the CPU before a device sees them ----

def distinct_calls(**which):
    """The envelope's calls, one per input of the models (the options change launches and kernels, not results)."""
    seen = {}
    for c in kc.envelope_calls(**which):
        seen.setdefault(c.key(), c)
    return list(seen.values())


def model_inputs(c):
    """bound_pass_model's arguments but for the order."""
    s, cols, rows, D, self_join, lo = kc.call_inputs(c)
    return [kc.scaled(D, s.S), kc.in_scope(D.shape, self_join, lo), [len(x) for x in rows], [len(x) for x in cols], s.ins_S,
            s.del_S, c.k, kc.cut_of(c.T, s.S)]


def sorted_bound(c):
    s, cols, _, D, self_join, lo = kc.call_inputs(c)
    return kc.pass1_model(D, [len(x) for x in cols], c.k, c.T, s.S, self_join, lo)


def test_bisection_is_the_kth_smallest():
    """kth_by_bisection against a sort: 1..64 lanes, values up to the largest a long index reaches, ties, lanes that
    are no candidates, every k the lanes allow; and the starting bound's bit 15 is never kept."""
    rng = np.random.default_rng(16)
    for lanes in (1, 2, 31, 32, 33, 63, 64):
        for top in (0, 1, 255, 8160, kc.TOP_LONG, 65535):
            D = rng.integers(0, top + 1, size=(40, lanes))
            D[::3] = D[::3] // 7 * 7  # ties
            cand = rng.random((40, lanes)) < 0.8
            for k in sorted({1, 2, lanes // 2, lanes - 1, lanes} - {0}):
                x = kc.kth_by_bisection(D, cand, k)
                for i in range(40):
                    v = np.sort(D[i][cand[i]])
                    if len(v) >= k:
                        assert x[i] == v[k - 1], (lanes, top, k, i)
    assert kc.kth_by_bisection([kc.TOP_LONG] * 64, [True] * 64, 64) == kc.TOP_LONG < 1 << 15
    assert int(kc.kth_by_bisection([3, 1, 2], [True, False, True], 2)) == 3


def test_bounds_are_the_same_in_every_schedule():
    """On every call of the GPU envelope tests the bound pass ends at the same bounds whether its waves run in index
    order, in reverse, all reading the starting bound, or in a random order reading stale bounds: those of the sorting
    model.  This is sed_join_dev.h's "in every schedule", proved on the CPU.  The emit pass then appends the sorting
    model's candidates and runs pass2_pairs' pairs; the bound pass runs at least as many pairs as the emit pass and at
    most those of the schedule in which every wave reads the cut."""
    calls = distinct_calls()
    assert len(calls) > 400
    for c in calls:
        want, cand = sorted_bound(c)
        stale = kc.call_model(c, "stale")[1]
        mask, p2 = kc.call_emit(c)
        for order in kc.ORDERS:
            bound, p1, writes = kc.call_model(c, order)
            assert np.array_equal(bound, want), (c, order)
            assert p2 <= p1 <= stale, (c, order)
            for _, x in writes:  # every value written is some wave's k-th smallest: no less than the row's bound
                assert (x[x >= 0] >= bound[x >= 0]).all(), (c, order)
        assert int(mask.sum()) == cand, c
        s, cols, rows, D, self_join, lo = kc.call_inputs(c)
        assert p2 == kc.pass2_pairs([len(x) for x in rows], [len(x) for x in cols], want, s.plan.ins, s.plan.dele, s.S, self_join, lo)
        per_row = np.bincount(kc.expected_knn(D, c.k, c.T, s.S, self_join, lo)["row"] - lo, minlength=len(rows))
        assert (per_row <= mask.sum(1)).all() and (per_row <= c.k).all(), c  # the candidates hold the answer


def final_bounds(calls):
    """[(call, row's final bound, the call's cut)] over the rows of the calls."""
    out = []
    for c in calls:
        cut = kc.cut_of(c.T, kc.envelope_set(c.set).S)
        out += [(c, int(b), cut) for b in kc.call_model(c)[0]]
    return out


def test_the_ladders_reach_every_bit_of_the_bisection():
    """Every bit 0..14 is both kept and dropped in some final bound of the ladder calls; the far ladders' k = 64 ends at
    the largest D * S either index reaches; bit 15 belongs to the starting bound 65535 alone."""
    ladders = final_bounds(distinct_calls(group="ladders"))
    lowered = [b for _, b, cut in ladders if b != cut]
    for bit in range(15):
        assert any(b >> bit & 1 for b in lowered) and any(not b >> bit & 1 for b in lowered), bit
    for kind, top in (("short", kc.TOP_SHORT), ("long", kc.TOP_LONG)):
        for name in kc.je.LIMITS:
            far = [c for c in kc.envelope_calls("ladders", kind, name) if c.set[0] == "far"]
            assert {c.k for c in far} >= set(kc.FAR_K)
            for c in far:
                s, cols, rows, D, _, _ = kc.call_inputs(c)
                assert len(cols) == 64 and len(rows) == 1 and len({len(x) for x in cols}) == 1
                bound = kc.call_model(c)[0]
                assert bound[0] == np.sort(kc.scaled(D, s.S)[0])[c.k - 1]
                if c.k == 64:
                    assert bound[0] == top
            if kind == "long":  # rounds 14 and 13 keep their bit, or the first bound is above 2^13 = what a loop from bit 12 ends at
                assert min(kc.call_model(c)[0][0] for c in far) > 1 << 13
    for c, b, cut in final_bounds(distinct_calls()):
        assert b == cut or b < 1 << 15, c
        assert cut <= kc.CUT_ALL


def test_some_bounds_stay_at_the_cut_and_some_come_from_a_later_wave():
    near = [c for c in kc.envelope_calls("ladders", "short") if c.set[0] == "near" and c.k == 64]
    assert near
    for c in near:  # 33 columns: no wave has 64
        assert kc.call_model(c)[0].tolist() == [kc.CUT_ALL] and len(kc.call_inputs(c)[1]) == 33
    later = 0
    for c in distinct_calls(group="geometry") + distinct_calls(group="limits"):
        bound, _, writes = kc.call_model(c, "stale")  # every wave with k columns within the cut writes its k-th smallest
        first = dict(writes)[0]
        later += int(((bound < np.where(first < 0, 1 << 20, first)) & (bound < kc.cut_of(c.T, kc.envelope_set(c.set).S))).sum())
    assert later > 0


@pytest.mark.parametrize("kind", ["short", "long"])
def test_k_against_the_lanes_in_scope(kind):
    """Identical sequences: a full wave that holds the row's own column has 63 in scope.  k = 63 tightens everywhere;
    k = 64 only through a full wave that does not hold the row; in a search every full wave has 64."""
    calls = kc.envelope_calls("scope", kind, "identical")
    assert {(c.k, c.ncols, c.queries is None) for c in calls if c.note == ""} == {
        (63, 130, True), (64, 130, True), (64, 130, False), (63, 66, True), (64, 66, True), (64, 66, False)}
    for c in calls:
        bound = kc.call_model(c)[0].tolist()
        if c.note == "zero" or c.k == 63 or c.queries is not None or c.ncols == 130:
            assert bound == [0] * len(bound), c
        else:  # 66 columns: the one full wave holds rows 0..63 themselves; rows 64 and 65 see all 64 of it
            assert bound == [kc.CUT_ALL] * 64 + [0, 0], c
    ties = kc.envelope_calls("scope", kind, "ties")
    assert len(ties) == 1 and ties[0].T == 0.0
    bound = kc.call_model(ties[0])[0]
    want = kc.expected_knn(kc.call_inputs(ties[0])[3], 8, 0.0, 1, True)
    assert not bound.any() and len(want) == 8 * len(kc.tie_set()[1]) and not want["dist"].any()  # a cut of 0 with hits


@pytest.mark.parametrize("name", ["i1_d254", "i254_d1"])
@pytest.mark.parametrize("kind", ["short", "long"])
def test_the_length_skip_of_pass_2_removes_whole_waves_and_keeps_others(kind, name):
    gone = kept = 0
    for c in distinct_calls(group="limits", kind=kind, case=name):
        DS, ok, len_rows, len_cols, ins_S, del_S, k, cut = model_inputs(c)
        bound = kc.call_model(c)[0]
        go = ok & (kc.length_bound(len_rows, len_cols, ins_S, del_S) <= bound[:, None])
        index = np.argsort(len_cols, kind="stable")
        for w in range(0, len(index), kc.WAVE):
            lanes = index[w:w + kc.WAVE]
            gone += int((ok[:, lanes].any(1) & ~go[:, lanes].any(1)).sum())
            kept += int(go[:, lanes].any(1).sum())
        assert kc.call_emit(c)[1] == int(go.sum()) <= int(ok.sum())
    assert gone > 0 and kept > 0


def test_the_planner_runs_both_kernels_on_the_bit_parallel_tables():
    for kind in ("short", "long"):
        for name in ("costs ACGUN", "unit block", "one way"):
            calls = kc.envelope_calls("bitpar", kind, name)
            assert {(c.k, c.options) for c in calls if not c.note} == {(k, o) for k in (1, 8) for o in ((), kc.FORCED_DP)}
            for c in calls:
                assert kc.envelope_set(c.set).S > 1
                assert kc.call_plan(c)["kernel"] == (1 if c.options == kc.FORCED_DP or c.note == "fifth" else 2), c
            if name == "one way":
                fifth = [c for c in calls if c.note == "fifth"]
                assert len(fifth) == 2 and all(len(c.queries) == 1 for c in fifth)
        for c in kc.envelope_calls("ladders", kind) + kc.envelope_calls("limits", kind):
            assert kc.call_plan(c)["kernel"] == 1
        for c in kc.envelope_calls("lanes", kind):
            assert kc.call_plan(c)["kernel"] == (1 if c.options else 2)


def test_cutoffs_beside_a_kth_distance():
    for c in kc.envelope_calls("cutoffs"):
        s, _, _, D, self_join, lo = kc.call_inputs(c)
        n = len(kc.expected_knn(D, c.k, c.T, s.S, self_join, lo))
        zero = len(kc.expected_knn(D, c.k, 0.0, s.S, self_join, lo))
        assert {"at d": n == c.k, "below d": zero <= n < c.k, "tiny": n == zero, "zero": n == zero}[c.note], c


# ---- bite checks: a restatement that is subtly wrong must disagree with the sorting model on some envelope call ----

def bisection(D, cand, k, top=15, below=np.less, need=0):
    """kc.kth_by_bisection with its three choices open: the first bit, the compare, the count asked for."""
    D, cand = np.asarray(D, np.int64), np.asarray(cand, bool)
    x = np.zeros(D.shape[:-1], np.int64)
    for bit in range(top, -1, -1):
        c = x | (1 << bit)
        x = np.where((cand & below(D, c[..., None])).sum(-1) < k + need, c, x)
    return x


def mutant_model(c, mutant):
    DS, ok, len_rows, len_cols, ins_S, del_S, k, cut = model_inputs(c)
    kth = kc.kth_by_bisection
    if mutant == "as written":
        kth = bisection
    elif mutant == "from bit 12":
        kth = lambda D, cand, k: bisection(D, cand, k, top=12)
    elif mutant == "D <= c":
        kth = lambda D, cand, k: bisection(D, cand, k, below=np.less_equal)
    elif mutant == "k - 1":
        kth = lambda D, cand, k: bisection(D, cand, k, need=-1)
    elif mutant == "no self rule":
        ok = np.ones_like(ok)
    elif mutant == "insert and delete swapped":
        ins_S, del_S = del_S, ins_S
    elif mutant == "D unshifted":
        s = kc.envelope_set(c.set)
        if s.S == 1 or kc.call_plan(c)["kernel"] != 2:
            return None  # the shift is the bit-parallel kernel's
        DS = DS >> (s.S.bit_length() - 1)
    return kc.bound_pass_model(DS, ok, len_rows, len_cols, ins_S, del_S, k, cut, kth=kth)[0]


MUTANTS = {"from bit 12": ("ladders", "long"), "D <= c": (), "k - 1": (), "no self rule": ("scope",),
           "insert and delete swapped": ("limits",), "D unshifted": ("bitpar",)}


def killers(mutant, calls):
    out = []
    for c in calls:
        got = mutant_model(c, mutant)
        if got is not None and not np.array_equal(got, sorted_bound(c)[0]):
            out.append(c)
    return out


def test_the_open_bisection_is_the_model():
    calls = distinct_calls(group="ladders", kind="long") + distinct_calls(group="scope")
    assert not killers("as written", calls)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_of_the_bound_pass_are_caught(mutant):
    """Each mutant differs from the sorting model on the calls of the group built against it."""
    where = MUTANTS[mutant]
    calls = kc.envelope_calls(*where) if where else kc.envelope_calls("columns", "short")
    dead = killers(mutant, [c for c in calls if not c.options or mutant == "D unshifted"][:60])
    assert dead, mutant
    if mutant == "from bit 12":  # what only the long far ladder sees: no other bound reaches 2^13
        assert "far" in {c.set[0] for c in dead}
        assert not killers(mutant, distinct_calls(kind="short")[::7])
