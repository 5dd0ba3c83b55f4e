"""CPU: the long similarity join (sequences of 0..128 symbols): its planner (sed_join_long_plan), the two lanes of
sed_join_long.hip as word-for-word models against the C oracle across their numeric envelope, and the Python layers
(wfsearch.JoinIndex / neighbors, sedshard.neighbors with long_sequences=True) over an oracle-backed engine; and the cases
of tests/test_gpu_join_long_envelope.py proved before a device sees them: the planner's choice, the bit-parallel lane
under a code map and a shift, what each set claims to hold, and the planner's counts of every call made there."""
import math
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import join_cases as jc
import join_envelope as je
import join_long_cases as jl
import sedgpu
import sedshard

INF = math.inf
ACGU = 0b1111


@pytest.fixture(scope="module")
def wfsearch():
    return jc.import_shim("wfsearch")


def _long(plan, len_rows, len_cols, T, self_join=False, rm=ACGU, cm=ACGU, options=None):
    return sedgpu.join_long_plan(jc.costs_of(plan), options or {}, len_rows, len_cols, self_join, rm, cm, T)


def _short(plan, len_rows, len_cols, T, self_join=False, rm=ACGU, cm=ACGU, options=None):
    return sedgpu.join_plan(jc.costs_of(plan), options or {}, len_rows, len_cols, self_join, rm, cm, T)


# ---- the planner ----

def test_max_len_is_128():
    assert sedgpu.join_long_max_len() == jl.MAXLEN == 128


def test_lengths_accepted_and_refused():
    plan, _ = jl.unit_plan()
    assert _long(plan, [0, 128], [128, 0], 1.0)["scope"] == 4
    for lr, lc, text in (([129], [5], r"row 0 has 129 symbols \(0\.\.128\)"), ([5], [7, 129], r"column 1 has 129 symbols \(0\.\.128\)"),
                         ([-1], [5], r"row 0 has -1 symbols"), ([5], [-1], r"column 0 has -1 symbols")):
        with pytest.raises(sedgpu.SedError, match=text) as ei:
            _long(plan, lr, lc, 1.0)
        assert ei.value.code == sedgpu.SED_E_ARG
    with pytest.raises(sedgpu.SedError) as ei:  # the short planner's bound has not moved
        _short(plan, [33], [5], 1.0)
    assert ei.value.code == sedgpu.SED_E_ARG


def test_refusal_order():
    """The arguments, max_dist, the costs rule, the code set, the rows, the columns: each refusal hides the later ones."""
    plan, _ = jl.unit_plan()
    bad = je.refused_neighbours()["sum 256"][0]
    with pytest.raises(sedgpu.SedError, match="max_dist is NaN or negative") as ei:
        _long(bad, [129], [129], -1.0, rm=1 << 7)
    assert ei.value.code == sedgpu.SED_E_ARG
    with pytest.raises(sedgpu.SedError, match=r"exceeds 255") as ei:
        _long(bad, [129], [129], 1.0, rm=1 << 7)
    assert ei.value.code == sedgpu.SED_E_RANGE
    with pytest.raises(sedgpu.SedError, match=r"a row code is outside the alphabet \(K=4\)") as ei:
        _long(plan, [129], [129], 1.0, rm=1 << 4)
    assert ei.value.code == sedgpu.SED_E_ARG
    with pytest.raises(sedgpu.SedError, match=r"a column code is outside the alphabet \(K=4\)"):
        _long(plan, [129], [129], 1.0, cm=1 << 4)
    with pytest.raises(sedgpu.SedError, match=r"row 0 has 129 symbols"):
        _long(plan, [129], [129], 1.0)
    with pytest.raises(sedgpu.SedError, match=r"column 0 has 129 symbols"):
        _long(plan, [128], [129], 1.0)
    with pytest.raises(sedgpu.SedError, match="bad join arguments"):  # a self join of more rows than columns
        _long(plan, [5, 5], [5], 1.0, self_join=True)


def test_refused_neighbours_give_their_own_text():
    for name, (plan, why) in je.refused_neighbours().items():
        with pytest.raises(sedgpu.SedError, match=why) as ei:
            sedgpu.join_long_plan(jc.costs_of(plan), {}, [128], [128], False, 1, 1, 1.0)
        assert ei.value.code == sedgpu.SED_E_RANGE, name


def test_limit_tables_are_served():
    for name, (plan, S) in je.limit_tables().items():
        assert _long(plan, [128], [128], 1.0, rm=3, cm=3)["scale"] == S, name


@pytest.mark.parametrize("which", ["unit", "user"])
def test_counts_match_a_recount(which):
    """scope, run, cells and lane_cells over a shuffled set holding every length 0..128, self and search."""
    plan, S = jl.unit_plan() if which == "unit" else jl.user_plan()
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.permutation(np.concatenate([np.arange(129), rng.integers(0, 129, size=40)]))]
    qlens = lens[:23][::-1]
    ins, dele = float(plan.ins), float(plan.dele)
    mask = ACGU if which == "unit" else 0b11111
    for T in (0.0, 1.0, 7.5, 40.0, INF):
        keep = jl.keep_rule(ins, dele, T, S)
        p = _long(plan, qlens, lens, T, rm=mask, cm=mask)
        assert p["scope"] == len(qlens) * len(lens)
        assert (p["run"], p["cells"]) == jc.lower_bound_count(qlens, lens, ins, dele, T, S), (which, T)
        assert p["lane_cells"] == jl.lane_cells(qlens, lens, keep), (which, T)
        for lo, hi in ((0, len(lens)), (17, 60), (40, 40)):
            p = _long(plan, lens[lo:hi], lens, T, self_join=True, rm=mask, cm=mask)
            assert p["scope"] == (hi - lo) * (len(lens) - 1)
            want = jc.lower_bound_count(lens[lo:hi], lens, ins, dele, T, S, self_rows=list(range(lo, hi)))
            assert (p["run"], p["cells"]) == want, (which, T, lo, hi)
            assert p["lane_cells"] == jl.lane_cells(lens[lo:hi], lens, keep)
            assert p["lane_cells"] >= p["cells"]
    # what padding costs: 64 columns of 40 symbols run two blocks a row, of 33..64 two, of 65 three
    assert _long(plan, [10], [40] * 64, INF)["lane_cells"] == 64 * 10 * 64
    assert _long(plan, [10], [32] * 64, INF)["lane_cells"] == 64 * 10 * 32
    assert _long(plan, [10], [65] * 64, INF)["lane_cells"] == 64 * 10 * 96
    assert _long(plan, [10], [0] * 64, INF)["lane_cells"] == 0
    assert _long(plan, [10], [5] * 64 + [128], INF)["lane_cells"] == 64 * 10 * (32 + 128)


def test_kernel_choice():
    plan, _ = jl.unit_plan()
    uplan, _ = jl.user_plan()
    cn = jc.plan_for(jc.load_golden("costs.json"), "ACGUN")
    assert _long(plan, [100], [128], 1.0)["kernel"] == 2
    assert _long(plan, [100], [128], 1.0, options={sedgpu.SED_OPT_JOIN_DP: 2})["kernel"] == 1
    assert _long(cn, [100], [128], 1.0)["kernel"] == 2
    assert _long(cn, [100], [128], 1.0, rm=ACGU | 16)["kernel"] == 1
    assert _long(cn, [100], [128], 1.0, cm=ACGU | 16)["kernel"] == 1
    assert _long(uplan, [100], [128], 1.0)["kernel"] == 1


def test_cut_clamp():
    """cut = min(floor(T S), 65535): one below the clamp a length difference whose bound is 65535 is left out only when
    the bound exceeds the cut.  Under i254_d1 (S = 1, insert = 254) a column 128 longer has bound 32512 <= 65534; no
    bound of <= 128 symbols reaches the clamp, so both sides of it, and every larger cutoff, run every pair."""
    plan, S = je.limit_tables()["i254_d1"]
    for T in (65534.0, 65535.0, 65536.0, 1e300, INF):
        p = _long(plan, [0, 128], [128, 0], T, rm=3, cm=3)
        assert p["run"] == p["scope"] == 4
    assert _long(plan, [0], [128], 128 * 254.0, rm=3, cm=3)["run"] == 1
    assert _long(plan, [0], [128], 128 * 254.0 - 1, rm=3, cm=3)["run"] == 0
    p256, S256 = je.limit_tables()["s256"]  # S = 256: T = 255.99 S = 65533 (floor), 256 S = 65536 -> the clamp
    for T in (65534.0 / 256, 65535.0 / 256, 256.0, INF):
        assert _long(p256, [128], [0], T, rm=3, cm=3)["run"] == 1  # 128 deletes = 128 * 155 = 19840 on the scale


def test_equals_the_short_plan_on_short_lengths():
    rng = np.random.default_rng(32)
    for name, (table, al, _) in jc.served_tables().items():
        plan = jc.plan_for(table, al)
        seqs = jc.mixed_set(17, al, 150)
        lens = [len(s) for s in seqs]
        q = [int(x) for x in rng.integers(0, 33, size=19)]
        mask = (1 << len(al)) - 1
        for T in (0.0, 1.25, 3.0, INF):
            for opts in ({}, {sedgpu.SED_OPT_JOIN_DP: 2}, {sedgpu.SED_OPT_JOIN_ROWS: 5}):
                for self_join, rows in ((False, q), (True, lens[10:90]), (True, lens)):
                    long_p = _long(plan, rows, lens, T, self_join, mask, mask, opts)
                    short_p = _short(plan, rows, lens, T, self_join, mask, mask, opts)
                    assert {k: long_p[k] for k in short_p} == short_p, (name, T, opts)
                    assert list(long_p)[:len(short_p)] == list(short_p)


# ---- the scaled DP's lane at MM = 128 ----

@pytest.fixture(scope="module")
def grid():
    return jl.length_grid()


@pytest.mark.parametrize("name", sorted(je.LIMITS))
def test_dp_lane_model_across_the_envelope(grid, name):
    plan, S = je.limit_tables()[name]
    D = jc.oracle_matrix(plan, grid, grid)
    DS, lo_key, hi_low = jl.dp_lane_matrix(plan, S, grid, grid)
    assert sorted(set(len(s) for s in grid)) == list(range(129))
    assert np.array_equal(DS, (D * S).astype(np.int64))
    assert np.array_equal((DS / float(S)).view(np.uint64), D.view(np.uint64))
    # the margins: 128 free substitutions under (insert + delete) S = 255 give the smallest key there is, the low
    # half-word sinks by one per update and never borrows, and 128 substitutions at insert + delete are the top
    assert lo_key == jl.LOWEST_KEY
    assert hi_low == 128 and hi_low < (je.KB & 0xFFFF)
    assert int(DS.max()) == jl.TOP_SCALED == 32640 < je.CUT_ALL


def test_dp_lane_model_under_user_costs():
    plan, S = jl.user_plan()
    seqs = jl.near_grid(11, "ACGU", extra="N")
    D = jc.oracle_matrix(plan, seqs[:40], seqs)
    DS, lo_key, hi_low = jl.dp_lane_matrix(plan, S, seqs[:40], seqs)
    assert np.array_equal(DS, (D * S).astype(np.int64)) and lo_key > jl.LOWEST_KEY and hi_low <= 128


# ---- the multi-word bit-parallel step ----

EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)


def test_bitpar_model_at_the_word_edges():
    plan, _ = jl.unit_plan()
    rng = np.random.default_rng(128)
    rows, cols = [], []
    for n in EDGES:
        rows += [[0] * n, [1] * n, [int(c) for c in rng.integers(0, 4, size=n)]]
    base = [int(c) for c in rng.integers(0, 4, size=128)]
    for m in EDGES:
        cols += [[0] * m, base[:m]]
    rows += [base[:n] for n in EDGES]  # prefixes of a column: matches that run through every word
    to_s = lambda codes: "".join("ACGU"[c] for c in codes)
    D = jc.oracle_matrix(plan, [to_s(r) for r in rows], [to_s(c) for c in cols])
    for i, x in enumerate(rows):
        for j, y in enumerate(cols):
            assert jl.bitpar_distance(x, y) == D[i, j], (len(x), len(y), i, j)
            if len(y) <= 96 and i % 3 == 2:  # in a wave whose longest column is longer: words above m run too
                assert jl.bitpar_distance(x, y, words=4) == D[i, j]
    # all-match and all-mismatch pairs carry through every word
    assert jl.bitpar_distance([0] * 128, [0] * 128) == 0 and jl.bitpar_distance([1] * 128, [0] * 128) == 128
    assert jl.bitpar_distance([], [0] * 128) == 128 and jl.bitpar_distance([0] * 128, []) == 128


def test_bitpar_model_one_word_is_the_short_step():
    from test_bitpar_model import bitpar_distance as short
    rng = np.random.default_rng(3)
    for _ in range(200):
        x = [int(c) for c in rng.integers(0, 4, size=int(rng.integers(0, 33)))]
        y = [int(c) for c in rng.integers(0, 4, size=int(rng.integers(0, 33)))]
        assert jl.bitpar_distance(x, y) == short(x, y)


# ---- the Python layers over an oracle-backed engine ----

@pytest.fixture(scope="module")
def long_set():
    return jl.random_set(77, 60)


@pytest.mark.parametrize("user", [False, True])
def test_wfsearch_long_join_index(wfsearch, long_set, user):
    plan = jc.plan_for(jc.load_golden("user_costs.json" if user else "costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, long_set, long_set)
    ix = wfsearch.JoinIndex(long_set, user, index_fn=jl.OracleEngine, long_sequences=True)
    assert jl.OracleEngine.built[-1].kw == {"long_seqs": True}
    N = len(long_set)
    assert max(len(s) for s in long_set) > 32
    for T in (0, 1, 6.5, INF):
        want = [(i, j, 1 / (1 + D[i, j])) for i in range(N) for j in range(N) if i != j and D[i, j] <= T]
        assert ix.neighbors(T) == want
        assert ix.neighbors(T, rows=(7, 19)) == [h for h in want if 7 <= h[0] < 19]
        assert wfsearch.neighbors(long_set, T, user, index_fn=jl.OracleEngine, long_sequences=True) == want
        assert jl.OracleEngine.built[-1].closed
    queries = [long_set[3], "", "ACGU" * 32, long_set[9][:-1] + "A"]
    Dq = jc.oracle_matrix(plan, queries, long_set)
    for T in (0, 5, INF):
        within = [[(s, 1 / (1 + Dq[q, j])) for j, s in enumerate(long_set) if Dq[q, j] <= T] for q in range(len(queries))]
        assert ix.search_many(queries, T) == within
        assert ix.search(queries[0], T) == within[0]
    ix.close()


def test_long_has_no_fp64_route(wfsearch, long_set):
    for route in ("f64", "auto"):
        with pytest.raises(ValueError, match="no fp64 route yet"):
            wfsearch.JoinIndex(long_set, index_fn=jl.OracleEngine, route=route, long_sequences=True)
        with pytest.raises(ValueError, match="no fp64 route yet"):
            wfsearch.neighbors(long_set, 2, index_fn=jl.OracleEngine, route=route, long_sequences=True)
        with pytest.raises(ValueError, match="no fp64 route yet"):
            sedshard.neighbors(long_set, 2, join_fn=_oracle_join, route=route, long_sequences=True)
    ix = wfsearch.JoinIndex(long_set, index_fn=jl.OracleEngine, long_sequences=True)
    for route in ("f64", "auto"):
        with pytest.raises(ValueError, match="no fp64 route yet"):
            ix.neighbors(2, route=route)
        with pytest.raises(ValueError, match="no fp64 route yet"):
            ix.search_many(["ACGU"], 2, route=route)
    assert ix.neighbors(0, route="int") == ix.neighbors(0)
    ix.close()
    SED = jc.import_shim("StringEditDistance")
    with pytest.raises(ValueError, match="no fp64 route yet"):
        SED.join_index(long_set, f64=True, long_seqs=True, engine=_no_engine)


def _no_engine(*a, **kw):
    raise AssertionError("the engine is not reached")


class _Codes:
    """An engine of StringEditDistance.join_index that keeps what it was given."""

    def __init__(self, codes, off, lens, **kw):
        self.lens, self.kw = lens, kw

    def close(self):
        pass


def test_defaults_still_refuse_33_symbols(wfsearch):
    SED = jc.import_shim("StringEditDistance")
    with pytest.raises(sedgpu.SedError, match=r"sequence 1 has 33 symbols \(the join serves at most 32\)"):
        SED.join_index(["ACGU", "A" * 33], engine=_Codes)
    ix = SED.join_index(["ACGU", "A" * 32], engine=_Codes)
    assert ix._dev.kw == {}  # the default engine call has not changed
    with pytest.raises(sedgpu.SedError, match=r"query 0 has 33 symbols \(the join serves at most 32\)"):
        ix.search(["A" * 33], 1)
    with pytest.raises(sedgpu.SedError, match=r"33 symbols"):
        wfsearch.JoinIndex(["A" * 33])
    long_ix = SED.join_index(["ACGU", "A" * 128], engine=_Codes, long_seqs=True)
    assert long_ix._dev.kw == {"long_seqs": True} and list(long_ix._dev.lens) == [4, 128]
    with pytest.raises(sedgpu.SedError, match=r"sequence 0 has 129 symbols \(the join serves at most 128\)"):
        SED.join_index(["A" * 129], engine=_Codes, long_seqs=True)
    with pytest.raises(sedgpu.SedError, match=r"query 1 has 129 symbols \(the join serves at most 128\)"):
        long_ix.search(["A", "C" * 129], 1)


def test_forked_proxy_refuses_the_long_index():
    for name in ("join_index", "join_long_index"):  # (the method reads nothing of the client)
        with pytest.raises(sedgpu.SedError, match="forked child's engine proxy does not serve resident indexes"):
            getattr(sedgpu.EngineClient, name)(None, None, None, None)


# ---- sedshard.neighbors ----

def _oracle_join(seqs, lo, hi, max_dist, user, long_seqs=False):
    assert long_seqs is True
    return jl.OracleEngine(seqs, user).self_join(max_dist, (lo, hi))


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
    got = sedshard.neighbors(seqs, T, True, world=world, rank=rank, join_fn=_oracle_join, long_sequences=True)
    if rank == 0:
        q.put((got["row"].tolist(), got["col"].tolist(), got["dist"].tolist()))
    else:
        assert got is None
    dist.destroy_process_group()


def test_sharded_long_neighbors_world_1_and_2():
    seqs = jl.random_set(9, 11)
    T = 30.0
    plan = jc.plan_for(jc.load_golden("user_costs.json"), "ACGUN")
    D = jc.oracle_matrix(plan, seqs, seqs)
    want = jc.expected_hits(D, T, 4, True)
    one = sedshard.neighbors(seqs, T, True, join_fn=_oracle_join, long_sequences=True)
    assert 0 < len(one) < len(seqs) * (len(seqs) - 1)
    assert (one["row"].tolist(), one["col"].tolist(), one["dist"].tolist()) == \
        (want["row"].tolist(), want["col"].tolist(), want["dist"].tolist())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_nb_worker, args=(r, 2, port, seqs, T, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == (one["row"].tolist(), one["col"].tolist(), one["dist"].tolist())


# ---- the envelope's cases, proved before tests/test_gpu_join_long_envelope.py runs them on a device ----

_ENV = {}  # computed once, shared, never changed
IDENTITY_MAP = 0b11100100  # ubfe(umap, 2 c, 2) = c for c = 0..3


def bitpar_case(name):
    """(plan, S, rows, columns, the oracle's D) of jl.bitpar_long_sets()[name]."""
    if name not in _ENV:
        plan, S, rows, cols = jl.bitpar_long_sets()[name]
        D = jc.oracle_matrix(plan, rows, cols)
        D.setflags(write=False)
        _ENV[name] = (plan, S, rows, cols, D)
    return _ENV[name]


def _plan_of(plan, rows, cols, T, self_join=False, options=None):
    return sedgpu.join_long_plan(jc.costs_of(plan), options or {}, [len(s) for s in rows], [len(s) for s in cols], self_join,
                                 jc.codes_mask(plan, rows), jc.codes_mask(plan, cols), T)


@pytest.mark.parametrize("name", list(je.bitpar_tables()))
def test_bitpar_cases_plan_the_bit_parallel_kernel(name):
    plan, S, rows, cols, _ = bitpar_case(name)
    forced = {sedgpu.SED_OPT_JOIN_DP: 2}
    assert S > 1 and je.scale_of(plan) == S
    if name == "one way":
        queries = rows[:-1]
        assert (jc.codes_mask(plan, queries), jc.codes_mask(plan, rows), jc.codes_mask(plan, cols)) == (0b11, 0b111, 0b11000000)
        assert len(queries) == 30 and len(cols) == 70 and len(rows[-1]) > 96
        assert _plan_of(plan, rows, cols, 1.0)["kernel"] == 1  # the fifth code
        assert _plan_of(plan, cols, queries, 1.0)["kernel"] == 1  # the other way costs 0.5
        rows = queries
    else:
        assert rows is cols
    for self_join in ((False,) if name == "one way" else (False, True)):
        for T in je.BITPAR_CUTOFFS:
            p = _plan_of(plan, rows, cols, T, self_join)
            assert (p["scale"], p["kernel"]) == (S, 2), (name, T)
            assert _plan_of(plan, rows, cols, T, self_join, forced)["kernel"] == 1
    umap = je.unit_map(plan, jc.codes_mask(plan, rows), jc.codes_mask(plan, cols))
    assert (umap == IDENTITY_MAP) == (name == "costs ACGUN")


@pytest.mark.parametrize("name", list(je.bitpar_tables()))
def test_bitpar_lane_model_under_the_code_map(name):
    """The kernel's umap step on both sides (the columns' zero padding included), its row reader and its << shift
    against oracle * S: on every pair of the set, under every count of words a wave could run for a column (words = 0:
    the column's own; 1..4: at least that many, as beside a longer column)."""
    plan, S, rows, cols, D = bitpar_case(name)
    square = rows is cols
    if name == "one way":
        rows, D = rows[:-1], D[:-1]
    want = D * S
    assert np.array_equal(want, np.floor(want)) and (want.max() > 100 * S or name == "one way")
    for words in range(5):
        DS = jl.mapped_matrix(plan, S, rows, cols, words)
        assert np.array_equal(DS, want.astype(np.int64)), (name, words)
    for T in je.BITPAR_CUTOFFS:
        got = je.hits_of_scaled(DS, je.planner_cut(T, S), S, square)
        assert jc.same_hits(got, je.expected_hits(D, T, S, square)), (name, T)
    if not square:
        assert not np.array_equal(D, jc.oracle_matrix(plan, cols, rows).T)  # the other way costs 0.5


def test_bitpar_lane_matrix_is_the_scalar_model_under_the_identity_map():
    rng = np.random.default_rng(44)
    rows = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (0, 1, 5, 33, 97, 128)]
    cols = [rng.integers(0, 4, size=m).astype(np.uint8) for m in (0, 2, 32, 64, 65, 128)]
    for words in (0, 4):
        DS = jl.bitpar_lane_matrix(IDENTITY_MAP, 3, rows, cols, words)
        for i, x in enumerate(rows):
            for j, y in enumerate(cols):
                assert DS[i, j] == jl.bitpar_distance(x.tolist(), y.tolist(), words or None) << 3


@pytest.mark.parametrize("name", ["costs ACGUN", "unit block"])
def test_square_sets_are_split_by_every_cutoff(name):
    plan, S, seqs, _, D = bitpar_case(name)
    symbols = je.bitpar_tables()[name][2]
    lens = {len(s) for s in seqs}
    assert len(seqs) == 100 and not set("".join(seqs)) - set(symbols)
    assert set(jl.EDGE_LENGTHS) <= lens and len(lens) > 40 and max(lens) == 128 and min(lens) == 0
    counts = [len(je.expected_hits(D, T, S, True)) for T in je.BITPAR_CUTOFFS]
    assert 0 < counts[0] < counts[1] == counts[2] == counts[3] < counts[4] < counts[5] == 100 * 99
    # distances 0, 1 and 2 among sequences of 95 symbols and more: all four words are live where the cutoffs split
    long = [i for i, s in enumerate(seqs) if len(s) >= 95]
    assert {0.0, 1.0, 2.0} <= set(D[np.ix_(long, long)][~np.eye(len(long), dtype=bool)].tolist())


def test_code_position_set_covers_every_position():
    seqs = jl.code_position_set()
    assert len(seqs) == 40 and sorted({len(s) for s in seqs}) == [32, 64, 96, 128]
    assert jl.code_positions(seqs[:8]) == {(c, p, b) for c in range(8) for p in range(4) for b in range(4)}
    assert len(jl.code_positions(seqs)) == 8 * 4 * 4
    assert all(sum(a != b for a, b in zip(seqs[r], seqs[8 + r])) == 1 for r in range(8))
    for name in ("i127_d128", "unit block"):
        plan = je.limit_tables()[name][0] if name == "i127_d128" else je.unit_block_table()
        assert plan.K == 8 and jc.codes_mask(plan, seqs) == 0xFF
        assert _plan_of(plan, seqs, seqs, 1.0, True)["kernel"] == 1  # eight codes: the DP
        D = jc.oracle_matrix(plan, seqs[:16], seqs[:16])
        assert len(np.unique(D)) > 4, name


def test_last_query_sets_end_with_the_128_symbol_query():
    plan, S, cols, lists, larger = jl.last_query_sets()
    q128 = lists[0][0]
    assert lists[0] == [q128] and len(q128) == 128 and all(q[-1] == q128 for q in lists)
    assert len(larger) > max(len(q) for q in lists) and all(len(q) >= 2 for q in lists[1:])
    last4 = [int(c) for c in plan.encode(q128[-4:])]
    assert len(set(last4)) == 4 and 0 not in last4
    assert S == 64 and max(len(s) for s in cols) == 128
    D = jc.oracle_matrix(plan, [q128], cols)[0]
    assert (D[-2], D[-1]) == (0.0, 2.0) and sorted(D.tolist())[2] > 3.0  # the planted copies, and nothing else near
    assert _plan_of(plan, lists[2], cols, 3.0)["kernel"] == 2
    # the model reads the look-ahead words past the last record from the spare bytes: pr[32] and pr[33]
    assert len(jl.record_words([plan.encode(q128)])) == 32 + jl.SPARE // 4 >= 34
    for q in lists:
        Dq = jc.oracle_matrix(plan, q, cols)
        assert np.array_equal(jl.mapped_matrix(plan, S, q, cols, 4), (Dq * S).astype(np.int64))


def test_column_geometry_set_ends_every_prefix_with_the_longest_column():
    seqs = jl.column_geometry_set()
    lens = [len(s) for s in seqs]
    assert len(seqs) == 257 and lens[0] == 128 and max(lens[1:]) <= 96 and min(lens) == 0 and set("".join(seqs)) == set("ACGU")
    for N in jl.COLUMN_COUNTS:
        col = je.sorted_lengths(seqs[:N])
        last = col[64 * ((N - 1) // 64):]
        assert last[-1] == 128 and all(m <= 96 for m in last[:-1]) and len(last) == (N - 1) % 64 + 1
    assert max(je.sorted_lengths(seqs[:65])[:64]) <= 96  # N = 65: a wave of three blocks, then the one column of four


@pytest.mark.parametrize("which", ["unit", "user"])
def test_counts_of_the_geometry_cases(which):
    """scope, run, cells, lane_cells and waves of the calls the GPU envelope makes: the column counts around the wave
    and block edges, rows=(lo, hi) ranges and query counts around a row group, and more rows than one launch."""
    G = sedgpu.join_rows_per_group()
    plan, S = jl.unit_plan() if which == "unit" else jl.user_plan()
    ins, dele = float(plan.ins), float(plan.dele)
    one_launch = 65535 * G

    def check(len_rows, len_cols, T, self_rows=None, options=None, launch_rows=one_launch):
        p = _long(plan, len_rows, len_cols, T, self_rows is not None, options=options)
        assert p["scope"] == len(len_rows) * len(len_cols) - (len(len_rows) if self_rows is not None else 0)
        assert (p["run"], p["cells"]) == jc.lower_bound_count(len_rows, len_cols, ins, dele, T, S, self_rows=self_rows)
        assert p["lane_cells"] == jl.lane_cells(len_rows, len_cols, jl.keep_rule(ins, dele, T, S))
        assert p["waves"] == jl.waves_of(len(len_rows), len(len_cols), launch_rows, G)
        return p

    lens = [len(s) for s in jl.column_geometry_set()]
    for N in jl.COLUMN_COUNTS:
        for T in (2.0, INF):
            p = check(lens[:N], lens[:N], T, list(range(N)))
            assert (p["run"] == N * (N - 1)) == (T == INF or N == 1)
            check([lens[3 % N], lens[0], lens[N - 1]], lens[:N], T)
    grid = [len(s) for s in jl.near_grid(1, "ACGU")]
    N = 70
    for R in (G - 1, G, G + 1, 2 * G + 1):
        for T in (2.0, INF):
            for lo in (0, 5, N - R):
                check(grid[lo:lo + R], grid[:N], T, list(range(lo, lo + R)))
            check(grid[N:N + R], grid[:N], T)
    N = 2 * (G + 1) + 3
    rows_opt = {sedgpu.SED_OPT_JOIN_ROWS: G + 1}
    for T in (1.0, INF):
        p = check(grid[:N], grid[:N], T, list(range(N)), rows_opt, G + 1)
        assert p["waves"] == 4 * (2 + 2 + 1)
        q = check(grid[:N], grid[:N], T, list(range(N)))
        assert q["waves"] == 4 * 4 and {k: p[k] for k in p if k != "waves"} == {k: q[k] for k in q if k != "waves"}
        check(grid[20:20 + N], grid[:N], T, None, rows_opt, G + 1)
