"""GPU: the eight kernels of the k-nearest calls (bound pass and emit pass, the scaled DP and the bit-parallel variant,
the 32-symbol and the 128-symbol index) across their envelope.  The calls are join_knn_cases.envelope_calls(), which
tests/test_join_knn_host.py proves on the CPU first: ladders whose distances reach every bit of the bound pass's
bisection, the planner's limit tables and the cutoff clamp, the bit-parallel kernels at S > 1 and under code maps that are
not the identity, row ranges and row groups under forced launch rows, the overflow rerun across launches, column counts
around the wave and block edges, k against the lanes in scope, a cut of 0 with hits, the nearest column at the ballots'
edges, and cutoffs on and beside a k-th distance.

Every call is compared record for record, dist bit for bit, with join_knn_cases.expected_knn over the C oracle's matrix;
its bounds with bound_pass_model (which no schedule changes), its candidates with emit_pass_model, and the pairs both
passes ran with the models' sandwich: twice the emit pass's at least, the emit pass's and an all-stale bound pass's at
most."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_envelope as je
import join_knn_cases as kc
import join_long_cases as jl
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
INDEX = {"short": sedgpu.JoinIndex, "long": sedgpu.LongJoinIndex}
KINDS = ["short", "long"]


@pytest.fixture
def opts(gpu):
    yield gpu
    gpu.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


class Index:
    """The index over (a prefix of) an envelope set's columns, and the checked call on it."""

    def __init__(self, gpu, call):
        self.gpu, self.set, self.ncols = gpu, call.set, call.ncols
        s, cols = kc.call_inputs(call)[:2]
        gpu.set_costs(s.plan)
        self.ix = INDEX[call.kind].from_seqs(gpu, jc.encode(s.plan, cols))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ix.close()

    def run(self, c):
        """One call against the oracle's list and the models; returns the records."""
        assert (c.set, c.ncols) == (self.set, self.ncols)
        s, cols, rows, D, self_join, lo = kc.call_inputs(c)
        for key in (sedgpu.SED_OPT_JOIN_DP, sedgpu.SED_OPT_JOIN_ROWS):
            self.gpu.set_option(key, dict(c.options).get(key, 0))
        if self_join:
            got = self.ix.self_knn(c.k, c.T, c.rows)
        else:
            got = self.ix.search_knn(jc.packed_queries(s.plan, rows), c.k, c.T)
        want = kc.expected_knn(D, c.k, c.T, s.S, self_join, lo)
        assert jc.same_hits(got, want), (c, len(got), len(want))
        assert self.ix.found == len(want)
        bound, _, _ = kc.call_model(c)
        assert np.array_equal(self.ix.knn_bounds(), bound), c
        mask, p2 = kc.call_emit(c)
        assert self.ix.knn_candidates == int(mask.sum()), c
        assert 2 * p2 <= self.ix.pairs_run() <= p2 + kc.call_model(c, "stale")[1], c
        return got


def run_all(gpu, calls):
    """Every call, each set's (and column count's) on one index; [(call, records)]."""
    assert calls
    out, done = [], set()
    for first in calls:
        if (first.set, first.ncols) in done:
            continue
        done.add((first.set, first.ncols))
        with Index(gpu, first) as ix:
            out += [(c, ix.run(c)) for c in calls if (c.set, c.ncols) == (first.set, first.ncols)]
    assert len(out) == len(calls)
    return out


def per_row(c, got):
    _, _, rows, _, _, lo = kc.call_inputs(c)
    return np.bincount(got["row"] - lo, minlength=len(rows))


# ---- 1. ladders: D * S up to 32 * 255 and 128 * 255 in one wave ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(je.LIMITS))
def test_ladders(opts, kind, name):
    """One query a^L against columns a^(L - j) b^j, (a -> b) at insert + delete: the far ladder's 64 columns for k = 1,
    2, 31, 32, 33, 63, 64 (under s256: every k), the near ladder's j = 0..L for k = 1 and 64."""
    for c, got in run_all(opts, kc.envelope_calls("ladders", kind, name)):
        ncols = len(kc.call_inputs(c)[1])
        assert per_row(c, got).tolist() == [min(c.k, ncols)], c
        if c.set[0] == "far":
            assert got["col"].tolist() == list(range(c.k)), c  # nearest first, ties to the lower column
            if c.k == 64:
                assert got["dist"][-1] * kc.envelope_set(c.set).S == (kc.TOP_LONG if kind == "long" else kc.TOP_SHORT)


# ---- 2. the limit tables on their extreme sets, and the cutoff clamp ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(je.LIMITS))
def test_limit_tables(opts, kind, name):
    got = run_all(opts, kc.envelope_calls("limits", kind, name))
    for k in (1, 8):
        of = lambda note: [g for c, g in got if c.k == k and c.note == note]
        (whole,), (capped,), clamp = of("inf"), of("median"), of("clamp")
        assert len(clamp) == len(kc.CLAMP_CAPS) and all(jc.same_hits(g, whole) for g in clamp)
        assert len(whole) == k * len(kc.envelope_set(("limit", kind, name)).cols) > len(capped) > 0


# ---- 3. the bit-parallel kernels at S > 1 and through a code map ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["costs ACGUN", "unit block", "one way"])
def test_bit_parallel_tables(opts, kind, name):
    """As planned (the bit-parallel kernels: pair() returns D << shift beside a bound on the scaled side), then with the
    DP forced: equal lists, equal to the oracle's.  "one way" is a search; its query with a fifth code plans the DP."""
    calls = kc.envelope_calls("bitpar", kind, name)
    for c in calls:
        assert kc.call_plan(c)["kernel"] == (1 if c.options == kc.FORCED_DP or c.note == "fifth" else 2), c
    got = run_all(opts, calls)
    for k in (1, 8):
        (planned,), (forced,) = ([g for c, g in got if c.k == k and c.options == o and not c.note] for o in ((), kc.FORCED_DP))
        assert jc.same_hits(planned, forced) and len(planned) > 0


# ---- 4. geometry: bound[] by absolute row across launches and row groups ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["self", "search"])
def test_row_ranges_and_row_groups_under_forced_launch_rows(opts, kind, case):
    """Self joins of rows (5, 23) and (1, 2), and a search with 11 queries (three row groups, the last of 3 rows; two
    copies of an index sequence, the empty query, one of the maximum length), each in one launch, in launches of one row
    group and of two."""
    got = run_all(opts, kc.envelope_calls("geometry", kind, case))
    assert {dict(c.options)[sedgpu.SED_OPT_JOIN_ROWS] for c, _ in got} == set(kc.LAUNCH_ROWS)
    first = {}
    for c, g in got:
        assert jc.same_hits(g, first.setdefault(c.key(), g)), c
    assert len(first) * len(kc.LAUNCH_ROWS) == len(got)
    if case == "search":
        s = kc.envelope_set(("geometry", kind))
        assert sedgpu.join_rows_per_group() == 4 and len(s.queries) == 11 and s.queries[0] == s.queries[1] == s.cols[11]
        assert "" in s.queries and max(map(len, s.queries)) == (jl.MAXLEN if kind == "long" else je.MAXLEN)
        k1 = [g for c, g in got if c.k == 1][0]
        assert k1["dist"][0] == k1["dist"][1] == 0.0  # a search reports the sequence itself


@pytest.mark.parametrize("kind", KINDS)
def test_overflow_rerun_across_launches(opts, kind):
    """tests/test_gpu_join_knn.py::test_undersized_device_list_grows under SED_OPT_JOIN_ROWS = 4: a fresh index, a small
    call that sizes the device list, then 68 launches whose candidates overflow it: pass 2 alone runs again, over every
    launch, with the bounds pass 1 left."""
    small, grows = kc.envelope_calls("overflow", kind)
    assert (small.note, grows.note) == ("small", "grows")
    rows = len(kc.call_inputs(grows)[2])
    assert int(kc.call_emit(grows)[0].sum()) > 2 * rows * grows.k + 1024 and rows > 64 * 4
    with Index(opts, small) as ix:
        ix.run(small)
        ix.run(grows)  # (the pairs counted leave the repeated second pass out: run() holds them to the models' sandwich)
        ix.run(grows)


# ---- 5. column counts: the partial last wave and the spare lanes ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", jl.COLUMN_COUNTS)
def test_column_counts(opts, kind, N):
    for c, got in run_all(opts, kc.envelope_calls("columns", kind, N)):
        scope = N - 1 if c.queries is None else N
        assert (per_row(c, got) == min(c.k, scope)).all(), c
        if scope < c.k or (N < 64 + (c.queries is None) and c.k == 64):
            assert (kc.call_model(c)[0] == kc.CUT_ALL).all()  # no wave has k in scope: the bound stays


# ---- 6. k against the lanes in scope; a cut of 0 with hits ----

@pytest.mark.parametrize("kind", KINDS)
def test_k_against_the_lanes_in_scope(opts, kind):
    """Identical sequences (tests/test_join_knn_host.py states the bounds: 0, but the cut for a row whose only full wave
    holds the row itself at k = 64): the list is the lowest columns by index, the row's own left out."""
    for c, got in run_all(opts, kc.envelope_calls("scope", kind, "identical")):
        N = len(kc.call_inputs(c)[1])
        rows = range(N) if c.queries is None else range(len(c.queries))
        want = [(r, j) for r in rows for j in [j for j in range(N) if c.queries is not None or j != r][:c.k]]
        assert list(zip(got["row"].tolist(), got["col"].tolist())) == want and not got["dist"].any(), c
    (c, got), = run_all(opts, kc.envelope_calls("scope", kind, "ties"))
    copies = kc.tie_set()[1]
    assert c.T == 0.0 and not got["dist"].any() and not kc.call_model(c)[0].any()
    assert list(zip(got["row"].tolist(), got["col"].tolist())) == [(i, j) for i in copies for j in [j for j in copies if j != i][:8]]


# ---- 7. the nearest column at the half-wave, wave and block edges ----

@pytest.mark.parametrize("kind", KINDS)
def test_nearest_column_at_the_ballots_edges(opts, kind):
    for c, got in run_all(opts, kc.envelope_calls("lanes", kind)):
        first = got[np.unique(got["row"], return_index=True)[1]]
        assert first["col"].tolist() == list(je.LANE_QUERIES) and not first["dist"].any(), c
        assert (per_row(c, got) == c.k).all()
        if c.k == 1:
            assert not kc.call_model(c)[0].any()
        else:
            assert (got["dist"][1::2] > 0).all()


# ---- 8. cutoffs on and beside a row's k-th distance ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["i254_d1", "unit block"])
def test_cutoffs_beside_a_kth_distance(opts, kind, name):
    got = {c.note: g for c, g in run_all(opts, kc.envelope_calls("cutoffs", kind, name))}
    assert len(got["at d"]) == 8 > len(got["below d"]) >= len(got["zero"])
    assert jc.same_hits(got["tiny"], got["zero"])
    assert jc.same_hits(got["below d"], got["at d"][:len(got["below d"])])
