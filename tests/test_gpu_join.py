"""GPU: the similarity join (sed_join_self, sed_join_search) against the C oracle over the full cross product, cut at T
on the host.  Hits match exactly: the same (row, col), and dist bit for bit."""
import math

import numpy as np
import pytest

import join_cases as jc
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # (table, set) -> (plan, seqs, D): computed once, shared, never changed


def ref(name, kind="mixed", count=130, pn=0.0):
    key = (name, kind, count, pn)
    if key not in _REF:
        table, al, S = jc.served_tables()[name]
        plan = jc.plan_for(table, al)
        seed = 1000 + len(name) + count
        seqs = jc.edge_length_set(seed, al, count) if kind == "edge" else jc.mixed_set(seed, al, count, pn)
        D = jc.oracle_matrix(plan, seqs, seqs)
        D.setflags(write=False)
        _REF[key] = (plan, seqs, D, S)
    return _REF[key]


def index_of(gpu, plan, seqs):
    gpu.set_costs(plan)
    return sedgpu.JoinIndex.from_seqs(gpu, jc.encode(plan, seqs))


@pytest.fixture
def dp_forced(gpu):
    yield lambda on: gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if on else 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 257])
def test_column_geometry(gpu, N):
    """Wave and block edges on the column side, self and search, every pair (T = +inf)."""
    plan, seqs, D, S = ref("costs ACGUN", count=257, pn=0.05)
    ix = index_of(gpu, plan, seqs[:N])
    try:
        got = ix.self_join(INF)
        assert jc.same_hits(got, jc.expected_hits(D[:N, :N], INF, S, True))
        assert len(got) == N * (N - 1)
        q = [3 % N, 0, N - 1]
        got = ix.search(jc.packed_queries(plan, [seqs[i] for i in q]), INF)
        assert jc.same_hits(got, jc.expected_hits(D[q][:, :N], INF, S))
    finally:
        ix.close()


def test_row_geometry(gpu):
    """G - 1, G, G + 1 and 2 G + 1 rows, by rows= ranges and by query counts."""
    G = sedgpu.join_rows_per_group()
    plan, seqs, D, S = ref("costs ACGUN", count=257, pn=0.05)
    N = 70
    ix = index_of(gpu, plan, seqs[:N])
    try:
        for R in (G - 1, G, G + 1, 2 * G + 1):
            for lo in (0, 5, N - R):
                got = ix.self_join(INF, rows=(lo, lo + R))
                assert jc.same_hits(got, jc.expected_hits(D[lo:lo + R, :N], INF, S, True, lo)), (R, lo)
            q = list(range(100, 100 + R))
            got = ix.search(jc.packed_queries(plan, [seqs[i] for i in q]), INF)
            assert jc.same_hits(got, jc.expected_hits(D[q][:, :N], INF, S)), R
    finally:
        ix.close()


@pytest.mark.parametrize("name,pn", [("costs ACGU", 0.0), ("costs ACGUN", 0.01), ("costs ACGUN", 0.2), ("user_costs", 0.05),
                                     ("eighths", 0.0)])
def test_both_variants_against_the_oracle(gpu, dp_forced, name, pn):
    plan, seqs, D, S = ref(name, pn=pn)
    N = len(seqs)
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    ix = index_of(gpu, plan, seqs)
    try:
        for T in (0.0, 2.0, INF):
            want = jc.expected_hits(D, T, S, True)
            kernel = sedgpu.join_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, T)["kernel"]
            assert kernel == (2 if name == "costs ACGU" else 1)
            got = ix.self_join(T)
            assert jc.same_hits(got, want), (name, T)
            if kernel == 2:  # the same set through the DP kernel
                dp_forced(True)
                forced = ix.self_join(T)
                dp_forced(False)
                assert jc.same_hits(forced, got) and jc.same_hits(forced, want)
        q = [1, 17, 40, 99]
        got = ix.search(jc.packed_queries(plan, [seqs[i] for i in q]), 3.0)
        assert jc.same_hits(got, jc.expected_hits(D[q], 3.0, S))
    finally:
        ix.close()
    if name == "eighths":  # the direction matters under this table
        assert not np.array_equal(D, D.T)


@pytest.mark.parametrize("name", ["costs ACGU", "costs ACGUN"])
def test_edge_lengths(gpu, dp_forced, name):
    """Only lengths 0, 1, 31, 32, the buffer's last sequence 32 long: the sink select at m = 0, 1, 32, rows of n = 0,
    `keep` at m = 32, and the last record's 16-byte loads."""
    plan, seqs, D, S = ref(name, kind="edge", count=97)
    ix = index_of(gpu, plan, seqs)
    try:
        for forced in (False, True):
            dp_forced(forced)
            for T in (0.0, 1.0, INF):
                assert jc.same_hits(ix.self_join(T), jc.expected_hits(D, T, S, True)), (name, forced, T)
            got = ix.search(jc.packed_queries(plan, ["", seqs[-1], seqs[0]]), INF)
            Dq = jc.oracle_matrix(plan, ["", seqs[-1], seqs[0]], seqs)
            assert jc.same_hits(got, jc.expected_hits(Dq, INF, S))
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["costs ACGU", "costs ACGUN", "eighths"])
def test_cutoff_is_exact_and_plan_equals_run(gpu, name):
    plan, seqs, D, S = ref(name, pn=0.2 if name == "costs ACGUN" else 0.0)
    table = jc.served_tables()[name][0]
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    k = int(np.unique(D * S)[3])  # an integer-scale distance that occurs
    ix = index_of(gpu, plan, seqs)
    try:
        counts = {}
        for T in (0.0, table["insert"], k / S, np.nextafter(k / S, 0.0), INF):
            got = ix.self_join(T)
            assert jc.same_hits(got, jc.expected_hits(D, T, S, True)), (name, T)
            p = sedgpu.join_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, T)
            assert ix.pairs_run() == p["run"], (name, T)
            counts[T] = (len(got), p["run"], p["scope"])
        # the pairs at D * S = k appear exactly at T = k / S
        at_k = int(((D * S) == k).sum()) - int((np.diag(D) * S == k).sum())
        assert at_k > 0 and counts[k / S][0] - counts[np.nextafter(k / S, 0.0)][0] == at_k
        assert counts[0.0][1] < counts[0.0][2]  # the length skip left pairs out
        assert counts[INF][1] == counts[INF][2] == len(seqs) * (len(seqs) - 1)
    finally:
        ix.close()


def test_self_join_semantics(gpu):
    plan, seqs, D, S = ref("costs ACGUN", pn=0.01)
    N = len(seqs)
    ix = index_of(gpu, plan, seqs)
    try:
        full = ix.self_join(INF)
        assert len(full) == N * (N - 1) and not (full["row"] == full["col"]).any()
        dups = [(i, j) for i in range(N) for j in range(N) if i != j and seqs[i] == seqs[j]]
        assert dups
        zero = ix.self_join(0.0)
        pairs = set(zip(zero["row"].tolist(), zero["col"].tolist()))
        assert all((i, j) in pairs and (j, i) in pairs for i, j in dups) and not zero["dist"].any()
        for k in (1, 64, N - 1):
            both = np.concatenate([ix.self_join(2.0, rows=(0, k)), ix.self_join(2.0, rows=(k, N))])
            assert jc.same_hits(both, ix.self_join(2.0)), k
    finally:
        ix.close()


def test_cap_protocol(gpu):
    plan, seqs, D, S = ref("costs ACGUN", pn=0.01)
    want = jc.expected_hits(D, 3.0, S, True)
    wq = jc.expected_hits(D[:5], 3.0, S)
    queries = jc.packed_queries(plan, seqs[:5])
    ix = index_of(gpu, plan, seqs)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap 0" % len(want)):
            ix.self_join(3.0, cap=0)  # the count query: nothing is stored, found is the total
        assert ix.found == len(want)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap %d" % (len(want), len(want) - 1)):
            ix.self_join(3.0, cap=len(want) - 1)
        assert ix.found == len(want)
        assert jc.same_hits(ix.self_join(3.0, cap=len(want)), want)  # the index stays usable; exact room is enough
        for _ in range(2):  # self joins and searches alternate on one index
            assert jc.same_hits(ix.search(queries, 3.0), wq)
            assert jc.same_hits(ix.self_join(3.0), want)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\)"):
            ix.search(queries, 3.0, cap=1)
        assert ix.found == len(wq)
        empty = ix.self_join(0.0, rows=(0, 0), cap=0)
        assert len(empty) == 0 and ix.found == 0
    finally:
        ix.close()


def test_costs_change_between_calls(gpu):
    plan, seqs, D, S = ref("costs ACGUN", pn=0.01)
    uplan = jc.plan_for(jc.served_tables()["user_costs"][0], "ACGUN")
    Du = jc.oracle_matrix(uplan, seqs[:60], seqs[:60])
    refused = jc.plan_for(jc.refused_tables()["N at 0.66"][0], "ACGUN")
    ix = index_of(gpu, plan, seqs[:60])
    try:
        assert jc.same_hits(ix.self_join(2.0), jc.expected_hits(D[:60, :60], 2.0, S, True))
        gpu.set_costs(uplan)
        assert jc.same_hits(ix.self_join(2.0), jc.expected_hits(Du, 2.0, 4, True))
        gpu.set_costs(refused)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\)"):
            ix.self_join(2.0)
        gpu.set_costs(plan)
        assert jc.same_hits(ix.self_join(2.0), jc.expected_hits(D[:60, :60], 2.0, S, True))
    finally:
        ix.close()


def test_refusals_and_errors(gpu):
    plan, seqs, _, _ = ref("costs ACGUN", pn=0.01)
    ix = index_of(gpu, plan, seqs[:20])
    try:
        for name, (table, al, why) in jc.refused_tables().items():
            gpu.set_costs(jc.plan_for(table, al))
            with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
                ix.self_join(1.0)
            with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
                ix.search(jc.packed_queries(plan, ["ACG"]), 1.0)
        gpu.set_costs(plan)
        for T in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\)"):
                ix.self_join(T)
        q33 = sedgpu.PackedPairs([np.zeros(33, np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*33 symbols"):
            ix.search(q33, 1.0)
        qk = sedgpu.PackedPairs([np.array([0, 5, 1], np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*row code.*K=5"):
            ix.search(qk, 1.0)
        gpu.set_costs(jc.plan_for(jc.served_tables()["costs ACGU"][0], "ACGU"))  # K = 4: the index holds N = code 4
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*column code.*K=4"):
            ix.self_join(1.0)
        gpu.set_costs(plan)
        assert len(ix.self_join(0.0, cap=None)) >= 0  # still usable
        with pytest.raises(sedgpu.SedError, match=r"33 symbols"):
            sedgpu.JoinIndex.from_seqs(gpu, [np.zeros(33, np.uint8)])
    finally:
        ix.close()
    fresh = sedgpu.Context(gpu.device)
    try:
        ix2 = sedgpu.JoinIndex.from_seqs(fresh, jc.encode(plan, seqs[:4]))
        with pytest.raises(sedgpu.SedError, match=r"\(-6\).*sed_set_costs"):
            ix2.self_join(1.0)
        ix2.close()
    finally:
        fresh.close()


@pytest.mark.parametrize("user", [False, True])
def test_search_many_equals_search_within(gpu, user):
    wfsearch = jc.import_shim("wfsearch")
    seqs = jc.mixed_set(31, "ACGUN", 300, pn=0.01)
    queries = [seqs[7], seqs[150][:-1], "", "ACGUACGUACGUACGUACGUACGU", seqs[299]]
    ix = wfsearch.JoinIndex(seqs, user)
    try:
        for T in (0, 2.5):
            assert ix.search_many(queries, T) == [wfsearch.search_within(q, seqs, T, user) for q in queries]
    finally:
        ix.close()


def test_more_rows_than_one_launch(gpu, dp_forced):
    G = sedgpu.join_rows_per_group()
    plan, seqs, D, S = ref("costs ACGUN", pn=0.01)
    N = 2 * (G + 1) + 3  # three launches of G + 1, G + 1 and 3 rows
    ix = index_of(gpu, plan, seqs[:N])
    try:
        gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, G + 1)
        lens = [len(s) for s in seqs[:N]]
        mask = jc.codes_mask(plan, seqs[:N])
        for T in (1.0, INF):
            assert jc.same_hits(ix.self_join(T), jc.expected_hits(D[:N, :N], T, S, True))
            p = sedgpu.join_plan(jc.costs_of(plan), {sedgpu.SED_OPT_JOIN_ROWS: G + 1}, lens, lens, True, mask, mask, T)
            assert ix.pairs_run() == p["run"] and p["waves"] == 4 * (2 + 2 + 1)
        got = ix.search(jc.packed_queries(plan, seqs[20:20 + N]), 2.0)
        assert jc.same_hits(got, jc.expected_hits(D[20:20 + N, :N], 2.0, S))
        assert ix.last_ms() > 0
    finally:
        ix.close()
