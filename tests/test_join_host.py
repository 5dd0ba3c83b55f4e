"""CPU: the similarity join's planner (sed_join_plan), its Python layers over an injected definition engine
(wfsearch.JoinIndex, wfsearch.neighbors) and the sharded join over gloo (sedshard.neighbors)."""
import math
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import join_cases as jc
import sedgpu
import sedshard

INF = math.inf


@pytest.fixture(scope="module")
def wfsearch():
    return jc.import_shim("wfsearch")


def _plan(name, len_rows, len_cols, T, self_join=False, row_mask=None, col_mask=None, options=None, tables=None):
    table, al, _ = (tables or jc.served_tables())[name]
    plan = jc.plan_for(table, al)
    full = (1 << len(al)) - 1
    return sedgpu.join_plan(jc.costs_of(plan), options or {}, len_rows, len_cols, self_join,
                            full if row_mask is None else row_mask, full if col_mask is None else col_mask, T)


def test_scale_per_table():
    for name, (_, _, S) in jc.served_tables().items():
        assert _plan(name, [5], [7], 1.0)["scale"] == S, name


def test_refused_tables_are_range_errors():
    for name, (table, al, _) in jc.refused_tables().items():
        plan = jc.plan_for(table, al)
        with pytest.raises(sedgpu.SedError) as ei:
            sedgpu.join_plan(jc.costs_of(plan), {}, [5], [7], False, 1, 1, 1.0)
        assert ei.value.code == sedgpu.SED_E_RANGE, name


def test_variant_choice():
    acgu = 0b01111
    assert _plan("costs ACGU", [5], [7], 1.0)["kernel"] == 2
    assert _plan("costs ACGUN", [5], [7], 1.0, row_mask=acgu, col_mask=acgu)["kernel"] == 2
    assert _plan("costs ACGUN", [5], [7], 1.0, row_mask=acgu | 16, col_mask=acgu)["kernel"] == 1
    assert _plan("costs ACGUN", [5], [7], 1.0, row_mask=acgu, col_mask=acgu | 16)["kernel"] == 1
    assert _plan("user_costs", [5], [7], 1.0, row_mask=acgu, col_mask=acgu)["kernel"] == 1
    assert _plan("costs ACGU", [5], [7], 1.0, options={sedgpu.SED_OPT_JOIN_DP: 2})["kernel"] == 1
    assert _plan("eighths", [5], [7], 1.0)["kernel"] == 1


def test_code_outside_alphabet_is_arg_error():
    for rm, cm in ((1 << 4, 1), (1, 1 << 7)):
        with pytest.raises(sedgpu.SedError) as ei:
            _plan("costs ACGU", [5], [7], 1.0, row_mask=rm, col_mask=cm)
        assert ei.value.code == sedgpu.SED_E_ARG


@pytest.mark.parametrize("T", [math.nan, -1.0, -0.0001])
def test_bad_cutoff_is_arg_error(T):
    with pytest.raises(sedgpu.SedError) as ei:
        _plan("costs ACGU", [5], [7], T)
    assert ei.value.code == sedgpu.SED_E_ARG


def test_length_over_32_is_arg_error():
    for lr, lc in (([33], [5]), ([5], [33]), ([-1], [5])):
        with pytest.raises(sedgpu.SedError) as ei:
            _plan("costs ACGU", lr, lc, 1.0)
        assert ei.value.code == sedgpu.SED_E_ARG


def test_plan_routes_refuses_the_join_options():
    plan = jc.plan_for(*jc.served_tables()["costs ACGU"][:2])
    pp = sedgpu.PackedPairs([np.zeros(4, np.uint8)], [np.zeros(4, np.uint8)])
    for key in (sedgpu.SED_OPT_JOIN_DP, sedgpu.SED_OPT_JOIN_ROWS):
        with pytest.raises(sedgpu.SedError):
            sedgpu.plan_routes(jc.costs_of(plan), {key: 2}, pp, sedgpu.SED_NO_LEN)


@pytest.mark.parametrize("name", ["costs ACGU", "user_costs", "eighths"])
def test_scope_and_run_counts(name):
    table, al, S = jc.served_tables()[name]
    seqs = jc.mixed_set(11, al, 90)
    lens = [len(s) for s in seqs]
    qlens = lens[:13][::-1]
    ins, dele = table["insert"], table["delete"]
    for T in (0.0, 1.0, 2.5, INF):
        # a search: every query against every column
        p = _plan(name, qlens, lens, T)
        assert p["scope"] == len(qlens) * len(lens)
        run, cells = jc.lower_bound_count(qlens, lens, ins, dele, T, S)
        assert (p["run"], p["cells"]) == (run, cells), (name, T)
        # self joins over the whole set and over row ranges
        for lo, hi in ((0, len(lens)), (0, 1), (17, 60), (89, 90), (40, 40)):
            p = _plan(name, lens[lo:hi], lens, T, self_join=True)
            assert p["scope"] == (hi - lo) * (len(lens) - 1)
            run, cells = jc.lower_bound_count(lens[lo:hi], lens, ins, dele, T, S, self_rows=list(range(lo, hi)))
            assert (p["run"], p["cells"]) == (run, cells), (name, T, lo, hi)
            if T == INF:
                assert p["run"] == p["scope"]
    assert _plan(name, lens, lens, 0.0, self_join=True)["run"] < _plan(name, lens, lens, 0.0, self_join=True)["scope"]


def test_cutoff_at_an_exact_scaled_integer():
    """costs.json over ACGUN, S = 4, insert = 1: a length difference of 3 has bound 3 = 12 / S.  At T = 3 it runs, one
    ulp below it does not."""
    lens_r, lens_c = [10, 10], [13, 12]
    assert _plan("costs ACGUN", lens_r, lens_c, 3.0)["run"] == 4
    assert _plan("costs ACGUN", lens_r, lens_c, np.nextafter(3.0, 0.0))["run"] == 2
    assert _plan("costs ACGUN", lens_r, lens_c, 2.75)["run"] == 2
    # eighths: delete = 1.25 = 10 / 8; rows one symbol longer than the columns
    assert _plan("eighths", [11], [10], 1.25)["run"] == 1
    assert _plan("eighths", [11], [10], np.nextafter(1.25, 0.0))["run"] == 0


def test_waves_follow_the_launches():
    G = sedgpu.join_rows_per_group()
    p = _plan("costs ACGU", [5] * (2 * G + 1), [5] * 257, 1.0)
    assert p["waves"] == 2 * 4 * 3
    p = _plan("costs ACGU", [5] * (2 * G + 1), [5] * 257, 1.0, options={sedgpu.SED_OPT_JOIN_ROWS: G})
    assert p["waves"] == 2 * 4 * 3
    p = _plan("costs ACGU", [5] * (2 * G + 2), [5] * 257, 1.0)
    assert p["waves"] == 2 * 4 * 3
    p = _plan("costs ACGU", [5] * (2 * G + 2), [5] * 257, 1.0, options={sedgpu.SED_OPT_JOIN_ROWS: G + 1})
    assert p["waves"] == 2 * 4 * 4  # two launches of G + 1 rows: 2 groups each


# ---- the Python layers over a definition engine ----

@pytest.fixture(scope="module")
def small_set():
    return jc.mixed_set(5, "ACGUN", 40, pn=0.05)


@pytest.mark.parametrize("user", [False, True])
def test_definition_engine_matches_the_oracle(small_set, user):
    table = jc.load_golden("user_costs.json" if user else "costs.json")
    plan = jc.plan_for(table, "ACGUN")
    D = jc.oracle_matrix(plan, small_set, small_set)
    eng = jc.DefinitionEngine(small_set, user)
    got = np.array([[eng.dist(a, b) for b in small_set] for a in small_set])
    assert np.array_equal(got.view(np.uint64), D.view(np.uint64))


@pytest.mark.parametrize("user", [False, True])
def test_wfsearch_join_index_over_the_engine(wfsearch, small_set, user):
    table = jc.load_golden("user_costs.json" if user else "costs.json")
    D = jc.oracle_matrix(jc.plan_for(table, "ACGUN"), small_set, small_set)
    ix = wfsearch.JoinIndex(small_set, user, index_fn=jc.DefinitionEngine)
    N = len(small_set)
    for T in (0, 1, 2.5, INF):
        want = [(i, j, 1 / (1 + D[i, j])) for i in range(N) for j in range(N) if i != j and D[i, j] <= T]
        assert ix.neighbors(T) == want
        assert ix.neighbors(T, rows=(7, 19)) == [h for h in want if 7 <= h[0] < 19]
        assert ix.neighbors(T, rows=(7, 7)) == []
    queries = [small_set[3], "", "ACGU", small_set[9][:-1] + "A"]
    Dq = jc.oracle_matrix(jc.plan_for(table, "ACGUN"), queries, small_set)
    for T in (0, 2, INF):
        # the stand-in for search_within: the distances of one query against every document, filtered, in order
        within = [[(s, 1 / (1 + Dq[q, j])) for j, s in enumerate(small_set) if Dq[q, j] <= T] for q in range(len(queries))]
        assert ix.search_many(queries, T) == within
        assert ix.search(queries[0], T) == within[0]
    assert ix.search_many([], 1) == []
    ix.close()
    assert ix._ix is None


def test_empty_collections_and_queries(wfsearch):
    ix = wfsearch.JoinIndex([], index_fn=jc.DefinitionEngine)
    assert ix.neighbors(3) == [] and ix.search_many(["ACG", ""], 3) == [[], []] and ix.search("A", 1) == []
    ix.close()
    assert wfsearch.neighbors([], 2, index_fn=jc.DefinitionEngine) == []
    one = wfsearch.JoinIndex(["ACGU"], index_fn=jc.DefinitionEngine)
    assert one.neighbors(INF) == []
    assert one.search_many(["", "ACGU"], INF) == [[("ACGU", 1 / 5)], [("ACGU", 1.0)]]
    one.close()


def test_one_shot_neighbors_closes_its_index(wfsearch, small_set):
    made = []

    def index_fn(seqs, user_cost):
        made.append(jc.DefinitionEngine(seqs, user_cost))
        return made[-1]
    got = wfsearch.neighbors(small_set, 2, True, index_fn=index_fn)
    ix = wfsearch.JoinIndex(small_set, True, index_fn=jc.DefinitionEngine)
    assert got == ix.neighbors(2) and len(made) == 1 and made[0].closed

    class Collection:
        def find(self, _):
            return [{"sequence": s} for s in small_set]
    assert wfsearch.neighbors(Collection(), 2, True, index_fn=jc.DefinitionEngine) == got


# ---- sedshard.neighbors over gloo ----

def _engine_join(seqs, lo, hi, max_dist, user):
    return jc.DefinitionEngine(seqs, user).self_join(max_dist, (lo, hi))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _nb_worker(rank, world, port, seqs, T, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = sedshard.neighbors(seqs, T, True, world=world, rank=rank, join_fn=_engine_join)
    if rank == 0:
        q.put((got["row"].tolist(), got["col"].tolist(), got["dist"].tolist()))
    else:
        assert got is None
    dist.destroy_process_group()


@pytest.mark.parametrize("world,nseq", [(2, 9), (3, 7)])
def test_sharded_neighbors_reassemble(world, nseq):
    seqs = jc.mixed_set(70 + world, "ACGUN", nseq, pn=0.05)
    T = 12.0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_nb_worker, args=(r, world, port, seqs, T, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    one = sedshard.neighbors(seqs, T, True, join_fn=_engine_join)
    assert len(one) > 0 and len(one) < nseq * (nseq - 1)
    assert got == (one["row"].tolist(), one["col"].tolist(), one["dist"].tolist())
    assert list(zip(*got[:2])) == sorted(zip(*got[:2]))
