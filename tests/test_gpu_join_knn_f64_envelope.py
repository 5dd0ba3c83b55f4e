"""GPU: the two passes of the fp64 k-nearest calls (sed_join_knn_self_f64 / sed_join_knn_search_f64) across their
envelope.  The calls are join_knn_f64_envelope.envelope_calls(), which tests/test_join_knn_f64_envelope.py proves on the
CPU first: ladders whose distances are chosen doubles, from the smallest subnormal to +inf, so that every round of the
63-round bisection goes both ways in a wave that sets a final bound; column counts on and beside the wave and the block
with the 16th symbol in rows and columns; k against the lanes in scope; row ranges off the row group under forced
launch rows; cutoffs on adjacent bit patterns; the overflow rerun across launches; and both routes on a table both serve.

Every call is compared record for record, dist bit for bit, with join_knn_f64_cases.expected_knn over the C oracle's
matrix; its bounds, as 64-bit patterns, with bound_pass_model (which no schedule changes), its candidates with
emit_pass_model, and the pairs both passes ran with the models' sandwich: twice the emit pass's at least, the emit
pass's and an all-stale bound pass's at most.  Nothing here has a tolerance."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_knn_f64_envelope as ke
import sedgpu

pytestmark = pytest.mark.gpu
INF = math.inf
U64 = np.uint64


@pytest.fixture
def opts(gpu):
    yield gpu
    gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, 0)


class Index:
    """The index over (a prefix of) an envelope set's columns, and the checked call on it."""

    def __init__(self, gpu, call):
        self.gpu, self.set, self.ncols = gpu, call.set, call.ncols
        s, cols = ke.call_inputs(call)[:2]
        self.plan = s.plan
        gpu.set_costs(s.plan)
        self.ix = sedgpu.JoinIndex.from_seqs(gpu, jc.encode(s.plan, cols))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ix.close()

    def run(self, c):
        """One call against the oracle's list and the models; returns the records."""
        assert (c.set, c.ncols) == (self.set, self.ncols)
        s, cols, rows, D, self_join, lo = ke.call_inputs(c)
        self.gpu.set_option(sedgpu.SED_OPT_JOIN_ROWS, dict(c.options).get(sedgpu.SED_OPT_JOIN_ROWS, 0))
        if self_join:
            got = self.ix.self_knn_f64(c.k, c.T, c.rows)
        else:
            got = self.ix.search_knn_f64(jc.packed_queries(s.plan, rows), c.k, c.T)
        want = ke.call_expected(c)
        assert jc.same_hits(got, want), (c, len(got), len(want))
        assert self.ix.found == len(want), c
        bound, _ = ke.call_model(c)
        got_bound = self.ix.knn_bounds_f64()
        assert len(got_bound) == len(rows) and np.array_equal(got_bound.view(U64), bound.view(U64)), c
        mask, p2, _ = ke.call_emit(c)
        assert self.ix.knn_candidates == int(mask.sum()), c
        assert 2 * p2 <= self.ix.pairs_run() <= p2 + ke.call_model(c, "stale")[1], c
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
    _, _, rows, _, _, lo = ke.call_inputs(c)
    return np.bincount(got["row"] - lo, minlength=len(rows))


# ---- 1. ladders: chosen doubles in one wave, every k ----

@pytest.mark.parametrize("name", ke.LADDERS)
def test_ladders(opts, name):
    """One query, BASE, against 64 columns (two waves: 128) each one substitution away at a chosen double: powers of
    two from 2^-1074 to 2^999 and pairs that differ in one exponent bit; pairs that differ in fraction bit t, t = 0..31
    and 32..51; keys around the seam of the two 32-bit words; costs up to the largest double and two columns at +inf."""
    for c, got in run_all(opts, ke.envelope_calls("ladders", name)):
        assert len(got) == c.k, c
        D = ke.call_inputs(c)[3][0]
        assert np.array_equal(got["dist"].view(U64), np.sort(D)[:c.k].view(U64)), c  # the k smallest, nearest first
    if name == "top":
        assert np.isinf(got["dist"][-2:]).all() and got["dist"][-3] == ke.MAX_DOUBLE


# ---- 2. column counts on and beside the wave and the block; the 16th symbol ----

@pytest.mark.parametrize("N", ke.COLUMN_COUNTS)
def test_column_counts_with_the_sixteenth_symbol(opts, N):
    for c, got in run_all(opts, ke.envelope_calls("columns", N)):
        scope = N - 1 if c.queries is None else N
        assert (per_row(c, got) == min(c.k, scope)).all(), c


# ---- 3. k against the lanes in scope ----

def test_k_against_the_lanes_in_scope(opts):
    """130 columns in waves of 64, 64 and 2: k = 1, 2, 63, 64 for every row, and for one row of the first wave and one of
    the last; 127 columns: at k = 64 no wave has 64 in scope for a row of the first, its bound stays at max_dist and pass
    2 is the fp64 join at max_dist, of which the trim keeps 64.  k = 65 and 129 are refused before anything runs."""
    got = run_all(opts, ke.envelope_calls("k", "whole") + ke.envelope_calls("k", "one row"))
    for c, g in got:
        assert (per_row(c, g) == c.k).all(), c
    (none,) = [c for c in ke.envelope_calls("k", "none") if c.note == "none"]
    with Index(opts, none) as ix:
        for c in ke.envelope_calls("k", "none"):
            g = ix.run(c)
            assert (per_row(c, g) == c.k).all(), c
        ix.run(none)
        assert (ix.ix.knn_bounds_f64() == INF).all() and ix.ix.knn_candidates == 64 * 126
        join = ix.ix.self_join_f64(none.T, none.rows)
        assert len(join) == 64 * 126 and jc.same_hits(sedgpu.join_knn_trim(join, 64), ke.call_expected(none))
        for k in ke.REFUSED_K:
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d .*1\.\.64" % k):
                ix.ix.self_knn_f64(k)
            with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d .*1\.\.64" % k):
                ix.ix.search_knn_f64(jc.packed_queries(ix.plan, [ke.envelope_set(none.set).cols[0]]), k)


# ---- 4. row ranges and row groups under forced launch rows ----

@pytest.mark.parametrize("case", ["self", "search"])
def test_row_ranges_under_forced_launch_rows(opts, case):
    """Self joins of rows (1, 2), (3, 9), (5, 6) and the last row alone, searches of 1, 4, 5 and 9 queries, in launches
    of 1, 3, 4 and 5 rows: the bounds are those of exactly the call's rows, whatever the launches."""
    got = run_all(opts, ke.envelope_calls("rows", case))
    assert {dict(c.options)[sedgpu.SED_OPT_JOIN_ROWS] for c, _ in got} == set(ke.LAUNCH_ROWS)
    first = {}
    for c, g in got:
        assert jc.same_hits(g, first.setdefault(c.key(), g)), c
    assert len(first) * len(ke.LAUNCH_ROWS) == len(got)


# ---- 5. cutoffs on adjacent bit patterns ----

@pytest.mark.parametrize("case", ["fraction high", "exponents", "same length", "top"])
def test_cutoffs_beside_a_kth_distance(opts, case):
    got = {c.note: (c, g) for c, g in run_all(opts, ke.envelope_calls("cutoffs", case))}
    if case == "top":
        assert len(got["largest"][1]) == 62 and np.isfinite(got["largest"][1]["dist"]).all()
        return
    k = got["at d"][0].k
    assert len(got["at d"][1]) == k == len(got["below d"][1]) + 1
    for note in ("above d", "largest"):
        assert jc.same_hits(got[note][1], got["at d"][1])
    assert jc.same_hits(got["below d"][1], got["at d"][1][:k - 1])
    assert jc.same_hits(got["minus zero"][1], got["zero"][1]) and not got["zero"][1]["dist"].any()
    assert len(got["zero"][1]) == {"fraction high": 0, "exponents": 1}.get(case, len(got["zero"][1])) <= len(got["tiny"][1])


# ---- 6. the overflow rerun across launches ----

def test_overflow_rerun_across_launches(opts):
    """tests/test_gpu_join_knn_f64.py::test_undersized_device_list_grows under SED_OPT_JOIN_ROWS = 5: a fresh index, a small
    call that sizes the device list, then 54 launches whose candidates overflow it: pass 2 alone runs again over every
    launch.  All sequences have one length, so the length skip removes nothing and the sandwich of run() is 2 p2 on
    both sides: the pairs counted are the first two passes' exactly."""
    small, grows = ke.envelope_calls("rerun")
    rows = len(ke.call_inputs(grows)[2])
    _, p2, _ = ke.call_emit(grows)
    assert int(ke.call_emit(grows)[0].sum()) > 2 * rows * grows.k + 1024 and ke.launches(grows) == 54
    with Index(opts, small) as ix:
        ix.run(small)
        ix.run(grows)
        assert ix.ix.pairs_run() == 2 * p2 == 2 * rows * (rows - 1)
        ix.run(grows)
        assert ix.ix.pairs_run() == 2 * p2


# ---- 7. both routes where both serve ----

def test_the_integer_route_agrees_where_it_serves(opts):
    """user_costs.json over ACGU + N, 300 columns: the fp64 call and the integer call return the same (row, col) lists
    and equal distances."""
    (c,) = ke.envelope_calls("cross")
    with Index(opts, c) as ix:
        f64 = ix.run(c)
        i32 = ix.ix.self_knn(c.k, c.T)
        assert len(f64) == 300 * c.k and jc.same_hits(f64, i32)
        q = jc.packed_queries(ix.plan, ke.envelope_set(c.set).cols[:9])
        assert jc.same_hits(ix.ix.search_knn_f64(q, c.k), ix.ix.search_knn(q, c.k))
