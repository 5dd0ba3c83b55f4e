"""GPU: the similarity join over sequences of 0..128 symbols (sed_join_long_self, sed_join_long_search) against the C
oracle over the full cross product, cut at T on the host.  Hits match exactly: the same (row, col), dist bit for bit."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_envelope as je
import join_long_cases as jl
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
_REF = {}  # name -> (plan, S, seqs, D): computed once, shared, never changed


def ref(name):
    if name not in _REF:
        if name in ("grid unit", "guard unit", "mixed unit"):
            plan, S = jl.unit_plan()
        else:
            plan, S = jl.user_plan()
        seqs = {"grid unit": lambda: jl.near_grid(1, "ACGU"), "grid user": lambda: jl.near_grid(2, "ACGU", extra="ACGUN"),
                "guard unit": lambda: jl.guard_set(), "guard user": lambda: jl.guard_set(extra="ACGUN"),
                "mixed unit": lambda: jc.mixed_set(41, "ACGU", 130), "mixed user": lambda: jc.mixed_set(42, "ACGUN", 130, pn=0.05),
                "random user": lambda: jl.random_set()}[name]()
        D = jc.oracle_matrix(plan, seqs, seqs)
        D.setflags(write=False)
        _REF[name] = (plan, S, seqs, D)
    return _REF[name]


def long_index(gpu, plan, seqs):
    gpu.set_costs(plan)
    return sedgpu.LongJoinIndex.from_seqs(gpu, jc.encode(plan, seqs))


@pytest.fixture
def opts(gpu):
    yield gpu
    gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


def _kernel(plan, seqs, T, options=None):
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    return sedgpu.join_long_plan(jc.costs_of(plan), options or {}, lens, lens, True, mask, mask, T)


@pytest.mark.parametrize("which", ["unit", "user"])
def test_every_length_against_the_oracle(opts, which):
    """One near-set with every length 0..128 once: self join and search of every pair, in both variants."""
    plan, S, seqs, D = ref("grid " + which)
    assert sorted(len(s) for s in seqs) == list(range(129))
    assert _kernel(plan, seqs, INF)["kernel"] == (2 if which == "unit" else 1)
    ix = long_index(opts, plan, seqs)
    try:
        got = ix.self_join(INF)
        assert len(got) == 129 * 128
        assert jc.same_hits(got, jc.expected_hits(D, INF, S, True)), je.classes_differing(
            got, jc.expected_hits(D, INF, S, True), [len(s) for s in seqs], [len(s) for s in seqs])
        found = ix.search(jc.packed_queries(plan, seqs), INF)
        assert jc.same_hits(found, jc.expected_hits(D, INF, S))
        for T in (0.0, 2.0, 9.0):
            assert jc.same_hits(ix.self_join(T), jc.expected_hits(D, T, S, True)), T
        if which == "unit":  # the same set through the DP kernel
            opts.set_option(sedgpu.SED_OPT_JOIN_DP, 2)
            assert _kernel(plan, seqs, INF, {sedgpu.SED_OPT_JOIN_DP: 2})["kernel"] == 1
            forced = ix.self_join(INF)
            assert jc.same_hits(forced, got)
            assert jc.same_hits(ix.search(jc.packed_queries(plan, seqs), 3.0), jc.expected_hits(D, 3.0, S))
    finally:
        ix.close()


@pytest.mark.parametrize("name", sorted(je.LIMITS))
def test_limit_tables_at_the_128_symbol_extremes(opts, name):
    plan, S = je.limit_tables()[name]
    seqs = jl.extremes_set(plan)
    D = jc.oracle_matrix(plan, seqs, seqs)
    top = float(D.max())
    assert top * S == jl.TOP_SCALED
    ix = long_index(opts, plan, seqs)
    try:
        for T in (0.0, top, float(np.nextafter(top, 0.0)), 65535.0 / S, 65536.0 / S, INF):
            got = ix.self_join(T)
            want = je.expected_hits(D, T, S, True)
            assert jc.same_hits(got, want), (name, T, je.classes_differing(got, want, [len(s) for s in seqs],
                                                                           [len(s) for s in seqs]))
            assert jc.same_hits(ix.search(jc.packed_queries(plan, seqs), T), je.expected_hits(D, T, S))
        full = ix.self_join(top)
        assert len(full) == len(seqs) * (len(seqs) - 1) > len(ix.self_join(float(np.nextafter(top, 0.0))))
    finally:
        ix.close()


@pytest.mark.parametrize("which", ["unit", "user"])
def test_skip_rule_and_pairs_run(opts, which):
    plan, S, seqs, D = ref("grid " + which)
    ix = long_index(opts, plan, seqs)
    try:
        runs = []
        for T in (0.0, 3.0, 20.0):
            got = ix.self_join(T)
            assert jc.same_hits(got, jc.expected_hits(D, T, S, True)), T
            p = _kernel(plan, seqs, T)
            assert ix.pairs_run() == p["run"], T
            runs.append(p["run"])
            q = seqs[5:30]
            found = ix.search(jc.packed_queries(plan, q), T)
            assert jc.same_hits(found, jc.expected_hits(D[5:30], T, S))
            lens, mask = [len(s) for s in seqs], jc.codes_mask(plan, seqs)
            assert ix.pairs_run() == sedgpu.join_long_plan(jc.costs_of(plan), {}, lens[5:30], lens, False, mask, mask, T)["run"]
        assert runs[0] < runs[1] < runs[2] < 129 * 128
    finally:
        ix.close()


def test_single_hits_at_chosen_lanes(opts):
    plan, S = jl.unit_plan()
    seqs = jl.lane_position_set()
    ix = long_index(opts, plan, seqs)
    try:
        for forced in (False, True):
            opts.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
            got = ix.search(jc.packed_queries(plan, [seqs[p] for p in jl.LANE_QUERIES]), 0.0)
            assert [(int(r), int(c), float(d)) for r, c, d in zip(got["row"], got["col"], got["dist"])] == \
                [(q, p, 0.0) for q, p in enumerate(jl.LANE_QUERIES)], forced
    finally:
        ix.close()


@pytest.mark.parametrize("which", ["unit", "user"])
def test_block_and_word_guards(opts, which):
    """65 columns whose lengths cross 32 / 33 and 64 / 65 inside the first wave and 96 / 97 on its edge."""
    plan, S, seqs, D = ref("guard " + which)
    lens = je.sorted_lengths(seqs)
    assert (lens[12], lens[13], lens[38], lens[39], lens[63], lens[64]) == (32, 33, 64, 65, 96, 97)
    ix = long_index(opts, plan, seqs)
    try:
        for forced in ((False, True) if which == "unit" else (False,)):
            opts.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
            for T in (0.0, 1.0, 33.0, INF):
                assert jc.same_hits(ix.self_join(T), jc.expected_hits(D, T, S, True)), (forced, T)
            assert jc.same_hits(ix.search(jc.packed_queries(plan, seqs[:9]), 2.0), jc.expected_hits(D[:9], 2.0, S))
    finally:
        ix.close()


def test_identical_128_mers(opts):
    plan, S = jl.unit_plan()
    seqs = jl.identical_set()
    ix = long_index(opts, plan, seqs)
    try:
        for forced in (False, True):
            opts.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
            got = ix.self_join(0.0)
            assert len(got) == 130 * 129 and not got["dist"].any() and not (got["row"] == got["col"]).any()
            assert np.array_equal(got["row"], np.repeat(np.arange(130), 129))
            assert ix.pairs_run() == 130 * 129
    finally:
        ix.close()


@pytest.mark.parametrize("which", ["unit", "user"])
def test_agrees_with_the_short_route(opts, which):
    plan, S, seqs, D = ref("mixed " + which)
    opts.set_costs(plan)
    short = sedgpu.JoinIndex.from_seqs(opts, jc.encode(plan, seqs))
    ix = long_index(opts, plan, seqs)
    try:
        q = jc.packed_queries(plan, seqs[3:40])
        for T in (0.0, 1.0, 2.5, INF):
            a, b = ix.self_join(T), short.self_join(T)
            assert jc.same_hits(a, b) and jc.same_hits(a, jc.expected_hits(D, T, S, True)), T
            assert ix.pairs_run() == short.pairs_run()
            assert jc.same_hits(ix.search(q, T), short.search(q, T))
    finally:
        ix.close()
        short.close()


def test_protocol(opts):
    plan, S, seqs, D = ref("grid user")
    want = jc.expected_hits(D, 6.0, S, True)
    ix = long_index(opts, plan, seqs)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap 0" % len(want)):
            ix.self_join(6.0, cap=0)  # the count query
        assert ix.found == len(want) > 0
        with pytest.raises(sedgpu.SedError, match=r"\(-4\).*found %d hits, cap %d" % (len(want), len(want) - 1)):
            ix.self_join(6.0, cap=len(want) - 1)
        assert jc.same_hits(ix.self_join(6.0, cap=len(want)), want)  # the index stays usable
        opts.set_option(sedgpu.SED_OPT_JOIN_ROWS, 4)
        assert jc.same_hits(ix.self_join(6.0), want)
        assert jc.same_hits(ix.search(jc.packed_queries(plan, seqs[:21]), 6.0), jc.expected_hits(D[:21], 6.0, S))
        opts.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)
        assert ix.last_ms() > 0
        q129 = sedgpu.PackedPairs([np.zeros(129, np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*129 symbols"):
            ix.search(q129, 1.0)
        qk = sedgpu.PackedPairs([np.array([0, 5, 1], np.uint8)], [np.zeros(0, np.uint8)])
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*row code.*K=5"):
            ix.search(qk, 1.0)
        for T in (math.nan, -1.0):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\)"):
                ix.self_join(T)
        with pytest.raises(sedgpu.SedError, match="no fp64 route yet"):
            ix.self_join_f64(1.0)
        none = ix.search(sedgpu.PackedPairs.from_concat(np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                                                        np.zeros(0, np.int32)), 1.0)
        assert len(none) == 0 and ix.found == 0
        assert jc.same_hits(ix.self_join(6.0), want)
    finally:
        ix.close()
    with pytest.raises(sedgpu.SedError, match=r"sed_join_long_index_create failed.*129 symbols \(at most 128\)"):
        sedgpu.LongJoinIndex.from_seqs(opts, [np.zeros(129, np.uint8)])
    with pytest.raises(sedgpu.SedError, match=r"33 symbols"):  # the short index has not moved
        sedgpu.JoinIndex.from_seqs(opts, [np.zeros(33, np.uint8)])
    empty = sedgpu.LongJoinIndex.from_seqs(opts, [])
    try:
        assert len(empty.self_join(INF)) == 0
        assert len(empty.search(jc.packed_queries(plan, ["ACGU" * 32]), INF)) == 0
    finally:
        empty.close()


def test_random_set_through_wfsearch(gpu):
    wfsearch = jc.import_shim("wfsearch")
    plan, S, seqs, D = ref("random user")
    N = len(seqs)
    assert N == 300 and max(map(len, seqs)) > 120 and any("N" in s for s in seqs)
    for T in (1.0, 12.0):
        got = wfsearch.neighbors(seqs, T, True, long_sequences=True)
        want = [(i, j, 1 / (1 + D[i, j])) for i in range(N) for j in range(N) if i != j and D[i, j] <= T]
        assert got == want and len(want) > 0
    with pytest.raises(ValueError, match="no fp64 route yet"):
        wfsearch.neighbors(seqs, 1.0, True, route="auto", long_sequences=True)
