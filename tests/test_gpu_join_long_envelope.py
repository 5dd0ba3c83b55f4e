"""GPU: the two kernels of the long similarity join (sed_join_long.hip: the scaled DP and the bit-parallel kernel over
sequences of 0..128 symbols) across their envelope (tests/join_long_cases.py): the bit-parallel kernel at S > 1 and
under code maps that are not the identity, row ranges and row groups, more rows than one launch, column counts around
the wave and block edges, a 128-symbol query as the upload's last record, eight codes at every byte of a code word in
every block, the cutoff clamp, cost changes on a live index, and sedshard.neighbors on the engine.

Every comparison is join_cases.same_hits against the C oracle's matrix cut on the host - the same (row, col), dist bit
for bit, every pair in scope - and every checked call also holds the kernel the planner names and the pairs the waves ran
against the planner's count."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_envelope as je
import join_long_cases as jl
import sedgpu
import sedshard

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # computed once, shared, never changed

DP, BITPAR = 1, 2


def memo(key, make):
    if key not in _REF:
        _REF[key] = make()
        for x in _REF[key]:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return _REF[key]


def square(key, plan, S, seqs):
    """(plan, S, seqs, D) with D the oracle's matrix of seqs against seqs."""
    return memo(key, lambda: (plan, S, seqs, jc.oracle_matrix(plan, seqs, seqs)))


def bitpar_case(name):
    """(plan, S, rows, columns, D) of jl.bitpar_long_sets()[name]."""
    def make():
        plan, S, rows, cols = jl.bitpar_long_sets()[name]
        return plan, S, rows, cols, jc.oracle_matrix(plan, rows, cols)
    return memo(("bitpar", name), make)


def grid(which):
    """One near-prefix of every length 0..128, shuffled: over ACGU under costs.json (the bit-parallel kernel), with
    some N under user_costs.json (the DP)."""
    plan, S = jl.unit_plan() if which == "unit" else jl.user_plan()
    return square(("grid", which), plan, S, jl.near_grid(1, "ACGU") if which == "unit" else jl.near_grid(2, "ACGU", extra="ACGUN"))


@pytest.fixture
def opts(gpu):
    yield gpu
    gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


class Long:
    """One long index and the checked calls on it: hits against the oracle's matrix cut on the host, the kernel the
    planner chose, and pairs_run against the plan's run.  D is the matrix of the call's rows (a self join's: of every
    sequence) against the index."""

    def __init__(self, gpu, plan, S, seqs, kernel, forced=False):
        self.gpu, self.plan, self.S, self.seqs, self.kernel = gpu, plan, S, seqs, kernel
        self.options = {}
        gpu.set_costs(plan)
        self.force(forced)
        self.ix = sedgpu.LongJoinIndex.from_seqs(gpu, jc.encode(plan, seqs))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ix.close()

    def option(self, key, value):
        self.gpu.set_option(key, value)
        self.options[key] = value

    def force(self, on):
        """Every later call through the DP kernel (SED_OPT_JOIN_DP = 2), or the planner's own choice again."""
        self.option(sedgpu.SED_OPT_JOIN_DP, 2 if on else 0)
        self.forced = on

    def plan_of(self, rows, self_join, T):
        mask = jc.codes_mask(self.plan, self.seqs)
        return sedgpu.join_long_plan(jc.costs_of(self.plan), self.options, [len(s) for s in rows], [len(s) for s in self.seqs],
                                     self_join, mask if self_join else jc.codes_mask(self.plan, rows), mask, T)

    def check(self, got, D, rows, T, self_join, what, kernel, row_lo=0):
        want = je.expected_hits(D, T, self.S, self_join, row_lo)
        if not jc.same_hits(got, want):
            bad = je.classes_differing(got, want, [len(s) for s in rows], [len(s) for s in self.seqs], row_lo)
            pytest.fail("%s, T = %r: %d hits for %d, differing in the (n, m) classes %s" % (what, T, len(got), len(want), bad[:12]))
        p = self.plan_of(rows, self_join, T)
        assert p["kernel"] == (DP if self.forced else kernel or self.kernel), (what, T, p)
        assert self.ix.pairs_run() == p["run"], (what, T)
        return got

    def self_join(self, D, T, what="", rows=None):
        lo, hi = rows or (0, len(self.seqs))
        return self.check(self.ix.self_join(T, rows), D[lo:hi], self.seqs[lo:hi], T, True, what + " self join", None, lo)

    def search(self, queries, D, T, what="", kernel=None):
        return self.check(self.ix.search(jc.packed_queries(self.plan, queries), T), D, queries, T, False, what + " search", kernel)


# ---- 1. the bit-parallel kernel at S > 1 and under code maps that are not the identity ----

@pytest.mark.parametrize("name", ["costs ACGUN", "unit block"])
def test_bitpar_scaled_and_mapped(opts, name):
    plan, S, seqs, _, D = bitpar_case(name)
    assert S > 1
    with Long(opts, plan, S, seqs, BITPAR) as j:
        for T in je.BITPAR_CUTOFFS:
            got = j.self_join(D, T, name)
            j.force(True)
            assert jc.same_hits(j.self_join(D, T, name + ", the DP forced"), got), (name, T)
            j.force(False)
        got = j.search(seqs, D, 1.25, name)
        j.force(True)
        assert jc.same_hits(j.search(seqs, D, 1.25, name + ", the DP forced"), got)
        counts = [len(je.expected_hits(D, T, S, True)) for T in je.BITPAR_CUTOFFS]
        assert counts[0] < counts[1] == counts[2] == counts[3] < counts[4] < counts[5]


def test_bitpar_one_way_and_disjoint_codes(opts):
    """Queries over codes {0, 1} against an index over {6, 7}: unit from row code to column code, 0.5 the other way.  The
    list with one more query, which carries a fifth code, plans the DP and still matches."""
    plan, S, fifth, seqs, D = bitpar_case("one way")
    queries = fifth[:-1]
    with Long(opts, plan, S, seqs, BITPAR) as j:
        for T in je.BITPAR_CUTOFFS + (5.0, 20.0):
            got = j.search(queries, D[:-1], T, "one way")
            j.force(True)
            assert jc.same_hits(j.search(queries, D[:-1], T, "one way, the DP forced"), got), T
            j.force(False)
            j.search(fifth, D, T, "one way, a fifth code", kernel=DP)
        assert 0 < len(got) < len(queries) * len(seqs)


# ---- 2. row geometry: rows=(lo, hi) ranges, row groups, more rows than one launch ----

@pytest.mark.parametrize("which", ["unit", "user"])
def test_row_geometry(opts, which):
    """G - 1, G, G + 1 and 2 G + 1 rows against 70 columns of mixed lengths 0..128, by rows= ranges (the self rule under
    a row offset, as every rank of sedshard.neighbors calls it) and by query counts."""
    G = sedgpu.join_rows_per_group()
    plan, S, seqs, D = grid(which)
    N = 70
    with Long(opts, plan, S, seqs[:N], BITPAR if which == "unit" else DP) as j:
        for R in (G - 1, G, G + 1, 2 * G + 1):
            for T in (INF, 2.0):
                for lo in (0, 5, N - R):
                    got = j.self_join(D[:N, :N], T, "%d rows from %d" % (R, lo), (lo, lo + R))
                    assert T != INF or len(got) == R * (N - 1)
                j.search(seqs[N:N + R], D[N:N + R, :N], T, "%d queries" % R)


@pytest.mark.parametrize("which", ["unit", "unit forced DP", "user"])
def test_more_rows_than_one_launch(opts, which):
    G = sedgpu.join_rows_per_group()
    plan, S, seqs, D = grid(which.split()[0])
    N = 2 * (G + 1) + 3  # three launches of G + 1, G + 1 and 3 rows
    with Long(opts, plan, S, seqs[:N], BITPAR if which == "unit" else DP, "forced" in which) as j:
        j.option(sedgpu.SED_OPT_JOIN_ROWS, G + 1)
        for T in (1.0, INF):
            j.self_join(D[:N, :N], T, which)
            p = j.plan_of(seqs[:N], True, T)
            assert p["waves"] == jl.waves_of(N, N, G + 1, G) == 4 * (2 + 2 + 1)
            j.search(seqs[20:20 + N], D[20:20 + N, :N], T, which)
        assert j.ix.last_ms() > 0


# ---- 3. column geometry: the last wave's spare lanes and the block edge ----

@pytest.mark.parametrize("N", jl.COLUMN_COUNTS)
def test_column_geometry(opts, N):
    """The first N of a set whose longest column, of 128 symbols, sorts into the last wave beside columns of at most 96
    and, when N is no multiple of 64, beside spare lanes that copy it: the hits and pairs_run are those of N columns."""
    plan, S = jl.unit_plan()
    _, _, seqs, D = square("columns", plan, S, jl.column_geometry_set())
    q = [3 % N, 0, N - 1]
    with Long(opts, plan, S, seqs[:N], BITPAR) as j:
        for forced in (False, True):
            j.force(forced)
            for T in (INF, 2.0):
                got = j.self_join(D[:N, :N], T, "N = %d" % N)
                assert T != INF or len(got) == N * (N - 1)
                j.search([seqs[i] for i in q], D[q][:, :N], T, "N = %d" % N)


# ---- 4. the row reader's look-ahead past the last record of the query buffer ----

def test_last_query_is_128_symbols(opts):
    plan, S, cols, lists, larger = jl.last_query_sets()
    refs = memo("last query", lambda: tuple(jc.oracle_matrix(plan, q, cols) for q in lists + [larger]))
    with Long(opts, plan, S, cols, BITPAR) as j:
        for forced in (False, True):
            j.force(forced)
            for again in (False, True):  # the second time after a larger search: the query block is reused at a smaller size
                for q, D in zip(lists, refs):
                    if again:
                        j.search(larger, refs[-1], 3.0, "the larger list")
                    for T in (0.0, 3.0, INF):
                        got = j.search(q, D, T, "%d queries, the last of 128 symbols" % len(q))
                        assert (len(q) - 1, len(cols) - 2, 0.0) in list(zip(got["row"].tolist(), got["col"].tolist(), got["dist"].tolist()))


# ---- 5. eight codes at every byte of a code word, in every block ----

@pytest.mark.parametrize("name", ["i127_d128", "unit block"])
def test_eight_codes_at_every_byte_position(opts, name):
    plan, S = je.limit_tables()[name] if name == "i127_d128" else je.bitpar_tables()[name][:2]
    _, _, seqs, D = square(("positions", name), plan, S, jl.code_position_set())
    assert len(jl.code_positions(seqs)) == 8 * 4 * 4
    occ = np.unique(D[~np.eye(len(seqs), dtype=bool)])
    with Long(opts, plan, S, seqs, DP, name == "unit block") as j:
        for T in (float(occ[len(occ) // 4]), float(occ[len(occ) // 2]), INF):
            j.self_join(D, T, name)
            j.search(seqs, D, T, name)


# ---- 6. the cutoff clamp ----

@pytest.mark.parametrize("route", ["dp s256", "bitpar S = 4"])
def test_cutoff_clamp(opts, route):
    """T S = 65535 and 65536, 1e300, the largest double (whose product with S overflows) and +inf: every pair in scope,
    with equal records."""
    if route == "dp s256":
        (plan, S), kernel = je.limit_tables()["s256"], DP
        _, _, seqs, D = square("clamp s256", plan, S, jl.extremes_set(plan) + jl.near_grid(6, je.ALPHA[:plan.K])[:40])
    else:
        kernel = BITPAR
        plan, S, seqs, _, D = bitpar_case("costs ACGUN")
    N = len(seqs)
    with Long(opts, plan, S, seqs, kernel) as j:
        first = None
        for T in je.CLAMP_CUTOFFS:
            got = j.self_join(D, T / S, route)
            assert len(got) == N * (N - 1)
            first = got if first is None else first
            assert jc.same_hits(got, first)
        for T in je.CLAMP_CUTOFFS[2:]:
            assert len(j.search(seqs[:9], D[:9], T, route)) == 9 * N


# ---- 7. cost changes on a live index, refusals ----

def test_costs_change_between_calls(opts):
    gpu = opts
    cn = jc.plan_for(jc.load_golden("costs.json"), "ACGUN")  # over ACGU sequences: unit, S = 4
    uplan, _ = jl.user_plan()
    _, _, seqs, D = square("change unit", cn, 4, jl.near_set_long(5, "ACGU", 60))
    _, _, _, Du = square("change user", uplan, 4, seqs)
    assert not np.array_equal(D, Du)
    refused = jc.plan_for(jc.refused_tables()["N at 0.66"][0], "ACGUN")
    query = jc.packed_queries(cn, ["ACG"])
    with Long(gpu, cn, 4, seqs, BITPAR) as j:
        j.self_join(D, 2.0, "unit")
        j.search(seqs[:7], D[:7], 2.0, "unit")
        j.plan, j.kernel = uplan, DP
        gpu.set_costs(uplan)  # the other kernel, its cost rows uploaded anew
        j.self_join(Du, 2.0, "user costs")
        j.search(seqs[:7], Du[:7], 2.0, "user costs")
        gpu.set_costs(refused)
        for call in (lambda: j.ix.self_join(2.0), lambda: j.ix.search(query, 2.0)):
            with pytest.raises(sedgpu.SedError, match=r"\(-4\).*multiples of 2\^-k"):
                call()
        j.plan, j.kernel = cn, BITPAR
        gpu.set_costs(cn)
        j.self_join(D, 2.0, "unit again")
        j.search(seqs[:7], D[:7], 2.0, "unit again")
    with_n = seqs[:20] + ["ACGUN" * 20]
    _, _, _, Dn = square("change with N", uplan, 4, with_n)
    with Long(gpu, uplan, 4, with_n, DP) as j:
        j.self_join(Dn, 2.0, "an index with N")
        gpu.set_costs(jl.unit_plan()[0])  # K = 4: the index holds N = code 4
        for call in (lambda: j.ix.self_join(1.0), lambda: j.ix.search(query, 1.0)):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*column code.*K=4"):
                call()
        for name, (table, al, why) in jc.refused_tables().items():
            gpu.set_costs(jc.plan_for(table, al))
            for call in (lambda: j.ix.self_join(1.0), lambda: j.ix.search(query, 1.0)):
                with pytest.raises(sedgpu.SedError, match=r"\(-4\).*" + why):
                    call()
        gpu.set_costs(uplan)
        j.self_join(Dn, 2.0, "served again")
    fresh = sedgpu.Context(gpu.device)
    try:
        ix = sedgpu.LongJoinIndex.from_seqs(fresh, jc.encode(cn, seqs[:4]))
        for call in (lambda: ix.self_join(1.0), lambda: ix.search(query, 1.0)):
            with pytest.raises(sedgpu.SedError, match=r"\(-6\).*sed_set_costs"):
                call()
        ix.close()
    finally:
        fresh.close()


# ---- 8. sedshard.neighbors(..., long_sequences=True) on the engine ----

@pytest.mark.parametrize("user", [False, True])
def test_sharded_neighbors_on_the_engine(gpu, user):
    SED = jc.import_shim("StringEditDistance")
    plan = jc.plan_for(jc.load_golden("user_costs.json" if user else "costs.json"), "ACGUN")
    _, _, seqs, D = square(("sharded", user), plan, 4, jl.random_set(12, 120))
    N, T = len(seqs), 12.0
    assert max(map(len, seqs)) > 120 and min(map(len, seqs)) < 5 and any("N" in s for s in seqs)
    want = jc.expected_hits(D, T, 4, True)
    listed = list(zip(want["row"].tolist(), want["col"].tolist(), want["dist"].tolist()))
    assert 0 < len(want) < N * (N - 1)
    one = sedshard.neighbors(seqs, T, user, world=1, long_sequences=True)
    assert list(zip(one["row"].tolist(), one["col"].tolist(), one["dist"].tolist())) == listed
    both = []
    for r in range(2):  # what rank r of a world of 2 joins: its block of rows under an offset
        lo, hi = sedshard.shard_range(N, 2, r)
        ix = SED.join_index(seqs, user, long_seqs=True)
        try:
            both += ix.self_join(T, (lo, hi))
        finally:
            ix.close()
    assert lo > 0 and both == listed
