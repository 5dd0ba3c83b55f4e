"""GPU: the three kernels of the similarity join (sed_join.hip: the scaled DP and the bit-parallel kernel;
sed_join_f64.hip) across their numeric envelope (tests/join_envelope.py): every column and row length, the integer
planner's limit tables, the bit-parallel kernel at S > 1 and under code maps that are not the identity, the cutoff
clamp, single hits at chosen lanes and full ballots with one hole, and waves the length skip splits.

Every comparison is join_cases.same_hits against the C oracle's matrix cut on the host - the same (row, col), dist bit
for bit, every pair in scope - and every call also checks the pairs the waves ran against the planner's count."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_envelope as je
import join_f64_cases as jf
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # computed once, shared, never changed

DP, BITPAR, F64 = 1, 2, 3


def memo(key, make):
    if key not in _REF:
        _REF[key] = make()
        for x in _REF[key]:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return _REF[key]


def square(key, plan, seqs):
    """(plan, seqs, D) with D the oracle's matrix of seqs against seqs."""
    return memo(key, lambda: (plan, seqs, jc.oracle_matrix(plan, seqs, seqs)))


def served(name):
    table, al, S = jc.served_tables()[name]
    return jc.plan_for(table, al), S


def f64_table(name):
    return jc.plan_for(*jf.tables()[name])


# (kernel, cost plan, S, forced): the routes the geometry cases run on
ROUTES = {"dp": lambda: (DP,) + served("costs ACGU") + (True,),
          "bitpar": lambda: (BITPAR,) + served("costs ACGU") + (False,),
          "f64": lambda: (F64, f64_table("costs15"), 0, False)}


class Join:
    """One index and the checked calls on it: hits against the oracle's matrix cut on the host, the kernel the planner
    chose, and pairs_run against the plan's run."""

    def __init__(self, gpu, plan, S, seqs, kernel, forced=False):
        self.gpu, self.plan, self.S, self.seqs, self.kernel = gpu, plan, S, seqs, kernel
        self.opts = {sedgpu.SED_OPT_JOIN_DP: 2} if forced else {}
        gpu.set_costs(plan)
        gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
        self.ix = sedgpu.JoinIndex.from_seqs(gpu, jc.encode(plan, seqs))

    def close(self):
        self.ix.close()
        self.gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def plan_of(self, rows, self_join, T, kernel=None):
        fn = sedgpu.join_f64_plan if self.kernel == F64 else sedgpu.join_plan
        p = fn(jc.costs_of(self.plan), self.opts, [len(s) for s in rows], [len(s) for s in self.seqs], self_join,
               jc.codes_mask(self.plan, rows), jc.codes_mask(self.plan, self.seqs), T)
        assert p["kernel"] == (kernel or self.kernel), (p, T)
        return p

    def want(self, D, T, self_join):
        return jf.expected_hits_f64(D, T, self_join) if self.kernel == F64 else je.expected_hits(D, T, self.S, self_join)

    def check(self, got, D, rows, T, self_join, what, kernel=None):
        want = self.want(D, T, self_join)
        if not jc.same_hits(got, want):
            bad = je.classes_differing(got, want, [len(s) for s in rows], [len(s) for s in self.seqs])
            pytest.fail("%s, T = %r: %d hits for %d, differing in the (n, m) classes %s" % (what, T, len(got), len(want), bad[:12]))
        assert self.ix.pairs_run() == self.plan_of(rows, self_join, T, kernel)["run"], (what, T)
        return got

    def self_join(self, D, T, what=""):
        got = self.ix.self_join_f64(T) if self.kernel == F64 else self.ix.self_join(T)
        return self.check(got, D, self.seqs, T, True, what + " self join")

    def forced_dp(self, call):
        """The same index through the DP kernel: call() under SED_OPT_JOIN_DP = 2."""
        self.gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 2)
        try:
            return call()
        finally:
            self.gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)

    def search(self, queries, D, T, what="", kernel=None, cap=None):
        packed = jc.packed_queries(self.plan, queries)
        got = self.ix.search_f64(packed, T, cap=cap) if self.kernel == F64 else self.ix.search(packed, T, cap=cap)
        return self.check(got, D, queries, T, False, what + " search", kernel)


# ---- 1. every column and row length, all three kernels ----

def grid_case(name):
    """(kernel, plan, S, forced, the 99 sequences of three length grids, D)"""
    def make():
        if name == "dp i127_d128":
            (plan, S), kernel, forced, symbols = je.limit_tables()["i127_d128"], DP, False, "AC"
        elif name in ("f64 costs15", "f64 rounding"):
            plan, S, kernel, forced, symbols = f64_table(name[4:]), 0, F64, False, "AC" if name == "f64 rounding" else "GU"
        else:
            (plan, S), kernel, forced, symbols = served("costs ACGU"), DP if name == "dp costs ACGU" else BITPAR, name == "dp costs ACGU", "CU"
        seqs = je.length_grids(symbols)
        return kernel, plan, S, forced, seqs, jc.oracle_matrix(plan, seqs, seqs)
    return memo(("grid", name), make)


@pytest.mark.parametrize("name", ["dp i127_d128", "dp costs ACGU", "bitpar costs ACGU", "f64 costs15", "f64 rounding"])
def test_every_length_class(gpu, name):
    """Three grids of one sequence per length 0..32: the self join meets every (n, m), n != m, the search with the same
    99 as queries every n = m, identical pairs included; at T = +inf and at two occurring distances."""
    kernel, plan, S, forced, seqs, D = grid_case(name)
    occ = np.unique(D[~np.eye(len(seqs), dtype=bool)])
    cuts = [float(occ[len(occ) // 4]), float(occ[len(occ) // 2]), INF]
    with Join(gpu, plan, S, seqs, kernel, forced) as j:
        for T in cuts:
            got = j.self_join(D, T, name)
            j.search(seqs, D, T, name)
        assert len(got) == 99 * 98 and len({(len(seqs[r]), len(seqs[c])) for r, c in zip(got["row"], got["col"])}) == 33 * 33


# ---- 2. the limit tables on the DP kernel ----

@pytest.mark.parametrize("name", list(je.LIMITS))
def test_limit_tables_at_every_cutoff(gpu, name):
    plan, S = je.limit_tables()[name]
    _, seqs, D = square(("limit", name), plan, je.limit_set(plan))
    N = len(seqs)
    off = ~np.eye(N, dtype=bool)
    assert D[off].max() * S == 32 * 255 and D[off].min() == 0
    counts = {}
    with Join(gpu, plan, S, seqs, DP) as j:
        for T in je.cutoffs(plan, D[off], S):
            counts[T] = len(j.self_join(D, T, name))
        j.search(seqs[:40], D[:40], float(np.median(D)), name)
    top = float(D[off].max())
    at_top = int((D[off] == top).sum())
    assert at_top > 0 and counts[top] - counts[float(np.nextafter(top, 0.0))] == at_top
    assert counts[top] == counts[INF] == counts[1e300] == N * (N - 1) and counts[0.0] == counts[5e-324] < counts[1.0 / S]


# ---- 3. the bit-parallel kernel at S > 1 and under code maps that are not the identity ----

@pytest.mark.parametrize("name", ["costs ACGUN", "unit block"])
def test_bitpar_scaled_and_mapped(gpu, name):
    plan, S, symbols = je.bitpar_tables()[name]
    _, seqs, D = square(("bitpar", name), plan, je.length_grid(symbols[1] + symbols[3], 4) + je.near_set(13, symbols, 67))
    assert S > 1 and not set("".join(seqs)) - set(symbols)
    with Join(gpu, plan, S, seqs, BITPAR) as j:
        for T in je.BITPAR_CUTOFFS:
            got = j.self_join(D, T, name)
            assert jc.same_hits(j.forced_dp(lambda: j.ix.self_join(T)), got), (name, T)
        counts = [len(je.expected_hits(D, T, S, True)) for T in je.BITPAR_CUTOFFS]
        assert counts[0] < counts[1] == counts[2] == counts[3] < counts[4] < counts[5]


def test_bitpar_one_way_table_and_disjoint_codes(gpu):
    """Queries over codes {0, 1} against an index over {6, 7}: unit from row code to column code, 0.5 the other way.  One
    more query with a fifth code plans the DP and still matches."""
    plan, S, _ = je.bitpar_tables()["one way"]
    queries, seqs = je.near_set(11, je.ALPHA[0:2], 40), je.near_set(12, je.ALPHA[6:8], 100)
    fifth = queries + [queries[3][:5] + je.ALPHA[2] + queries[3][5:31]]
    _, _, D = memo("one way", lambda: (plan, seqs, jc.oracle_matrix(plan, fifth, seqs)))
    assert not np.array_equal(D[:40], jc.oracle_matrix(plan, seqs, queries).T)
    with Join(gpu, plan, S, seqs, BITPAR) as j:
        for T in je.BITPAR_CUTOFFS + (5.0, 20.0):
            got = j.search(queries, D[:40], T, "one way")
            assert jc.same_hits(j.forced_dp(lambda: j.ix.search(jc.packed_queries(plan, queries), T)), got), T
            j.search(fifth, D, T, "one way, a fifth code", kernel=DP)


# ---- 4. the cutoff clamp ----

@pytest.mark.parametrize("route", ["dp s256", "bitpar S = 4", "f64 rounding"])
def test_cutoff_clamp(gpu, route):
    """T S = 65535 and 65536, 1e300, the largest double (whose product with S overflows) and +inf: every pair in scope,
    with equal records."""
    if route == "dp s256":
        (plan, S), kernel = je.limit_tables()["s256"], DP
        _, seqs, D = square(("limit", "s256"), plan, je.limit_set(plan))
    elif route == "bitpar S = 4":
        (plan, S, symbols), kernel = je.bitpar_tables()["costs ACGUN"], BITPAR
        _, seqs, D = square(("bitpar", "costs ACGUN"), plan, je.length_grid(symbols[1] + symbols[3], 4) + je.near_set(13, symbols, 67))
    else:
        plan, S, kernel = f64_table("rounding"), 0, F64
        _, seqs, D = square("clamp f64", plan, je.length_grid("AC", 1) + je.near_set(5, "ACGUN", 67))
    N = len(seqs)
    with Join(gpu, plan, S, seqs, kernel) as j:
        first = None
        for T in je.CLAMP_CUTOFFS:
            got = j.self_join(D, T / S if S else T, route)
            assert len(got) == N * (N - 1)
            first = got if first is None else first
            assert jc.same_hits(got, first)
        got = j.search(seqs[:9], D[:9], je.CLAMP_CUTOFFS[3], route)
        assert len(got) == 9 * N
        if kernel == F64:  # on and next to every cost and three occurring distances, in `keep` and in D <= max_dist
            for T in je.cutoffs_f64(jf.tables()["rounding"][0], D):
                j.self_join(D, T, route)
            off = D[~np.eye(N, dtype=bool)]
            top = float(off.max())  # the largest occurring distance and one ulp below it
            below = j.self_join(D, float(np.nextafter(top, 0.0)), route)
            assert len(j.self_join(D, top, route)) - len(below) == int((off == top).sum()) > 0


# ---- 5. the wave-wide append: single hits at chosen lanes, full ballots with one hole ----

@pytest.mark.parametrize("route", list(ROUTES))
def test_single_hits_at_chosen_lanes(gpu, route):
    kernel, plan, S, forced = ROUTES[route]()
    seqs = je.lane_position_set()
    queries = [seqs[p] for p in je.LANE_QUERIES]
    _, _, D = memo(("lanes", route), lambda: (plan, seqs, jc.oracle_matrix(plan, queries, seqs)))
    with Join(gpu, plan, S, seqs, kernel, forced) as j:
        got = j.search(queries, D, 0.0, route)
        assert list(zip(got["row"].tolist(), got["col"].tolist())) == list(enumerate(je.LANE_QUERIES)) and not got["dist"].any()
        assert jc.same_hits(j.search(queries, D, 0.0, route, cap=7), got)
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found 7 hits, cap 6"):
            j.search(queries, D, 0.0, route, cap=6)
        assert j.ix.found == 7


@pytest.mark.parametrize("route", list(ROUTES))
def test_full_ballots_with_one_hole(gpu, route):
    kernel, plan, S, forced = ROUTES[route]()
    seqs = je.identical_set()
    N = len(seqs)
    D = np.zeros((N, N))
    assert jc.oracle_matrix(plan, seqs[:1], seqs[:1])[0, 0] == 0
    with Join(gpu, plan, S, seqs, kernel, forced) as j:
        got = j.self_join(D, 0.0, route)
        assert len(got) == 130 * 129 and not got["dist"].any()
        assert list(zip(got["row"].tolist(), got["col"].tolist())) == [(i, c) for i in range(N) for c in range(N) if i != c]


# ---- 6. waves in which the length skip splits the lanes ----

@pytest.mark.parametrize("route", list(ROUTES) + ["dp S = 4", "f64 rounding"])
def test_split_waves(gpu, route):
    """65 columns whose lengths 10..14 change inside the first wave and on the wave edge: lanes out of scope run with
    their wave and must be neither reported nor counted."""
    if route == "f64 rounding":
        kernel, plan, S, forced = F64, f64_table("rounding"), 0, False
        cuts = [float(np.nextafter(0.1, INF)), float(np.nextafter(0.2, INF)), 0.1, INF]
    elif route == "dp S = 4":
        kernel, (plan, S), forced = DP, served("costs ACGUN"), False
        cuts = [1.0, 0.0, float(np.nextafter(1.0, 0.0)), 2.0, INF]
    else:
        kernel, plan, S, forced = ROUTES[route]()
        cuts = [1.0, 0.0, 2.0, INF]
    seqs = je.split_wave_set("ACGN" if route == "dp S = 4" else "ACGU")
    _, _, D = square(("split", route), plan, seqs)
    runs = []
    with Join(gpu, plan, S, seqs, kernel, forced) as j:
        for T in cuts:
            got = j.self_join(D, T, route)
            runs.append(j.ix.pairs_run())
            j.search(seqs[:9], D[:9], T, route)
        assert 0 < len(got) and runs[0] < runs[-1] == 65 * 64  # the first cutoff left lengths of the first wave out
