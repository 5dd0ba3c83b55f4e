"""GPU: band pruning of checkpoint script batches (SED_OPT_BAND).  The forward skips the chunks of every stripe that
no optimal path can reach and the traceback takes the border constant where the forward did; distances, lengths and
scripts must not change.  Every batch is checked three ways: every pair against the C oracle op by op, the whole
packed `ops` buffer against the same batch run with SED_OPT_BAND = 2, and err == 0 on every pair (results() raises
SedError naming the pair otherwise)."""
import os

import numpy as np
import pytest

from conftest import padding_errors
import oracle
import sedcost
import sedgpu
import synth

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
S = "ACGU"


def _plan(table):
    return sedcost.build_plan(table, [S], [S])


def _diag_ub(table, a, b):
    sub = np.array([[0.0 if x == y else table["update"][x][y] for y in S] for x in S])
    k = min(len(a), len(b))
    return float(sub[a[:k], b[:k]].sum()) + (table["insert"] * (len(b) - len(a)) if len(b) > len(a)
                                             else table["delete"] * (len(a) - len(b)))


def _run(gpu, packed, R, band):
    gpu.set_option(sedgpu.SED_OPT_TB, 2)
    gpu.set_option(sedgpu.SED_OPT_CHAIN, 2)
    gpu.set_option(sedgpu.SED_OPT_SPLIT, 2)  # (a few long pairs: one wave per pair all the same)
    gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, R)
    gpu.set_option(sedgpu.SED_OPT_BAND, 0 if band else 2)
    try:
        b = sedgpu.Batch(gpu, packed, True)
        try:
            b.run()
            out = b.results()  # raises when any pair's err != 0
            assert b.traceback_mode == 2 and b.rows_per_lane == R
            return out, b.band_cells, b.work()[0]
        finally:
            b.close()
    finally:
        gpu.set_option(sedgpu.SED_OPT_BAND, 0)
        gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, 0)
        gpu.set_option(sedgpu.SED_OPT_SPLIT, 0)
        gpu.set_option(sedgpu.SED_OPT_CHAIN, 0)
        gpu.set_option(sedgpu.SED_OPT_TB, 0)


def _check(gpu, table, A, B, R, pruned):
    """The three checks; pruned: True / False = the forward must / must not skip cells, None = either."""
    plan = _plan(table)
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    (d, ii, ln, ops), cells, nominal = _run(gpu, packed, R, True)
    (d0, ii0, ln0, ops0), cells0, _ = _run(gpu, packed, R, False)
    assert cells0 == nominal and cells <= nominal
    if pruned is not None:
        assert (cells < nominal) == pruned, (cells, nominal)
    assert np.array_equal(ops, ops0), np.flatnonzero(ops != ops0)[:10]  # the whole buffer, padding included
    assert np.array_equal(d, d0) and np.array_equal(ln, ln0) and np.array_equal(ii, ii0)
    cs = oracle.Costs.from_plan(plan)
    P = packed.npairs
    od, oi, ol, oops, ooff = oracle.batch(cs, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b,
                                          packed.off_b, packed.len_b, P, want_ops=True, nthreads=THREADS)
    assert np.array_equal(d, od) and np.array_equal(ln, ol) and np.array_equal(ii.astype(bool), oi.astype(bool))
    bad = [p for p in range(P) if not np.array_equal(sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])),
                                                     oops[ooff[p]:ooff[p] + ol[p]])]
    assert not bad, bad[:10]
    assert not padding_errors(ops, packed.ops_off, packed.len_a, packed.len_b, ln)


@pytest.mark.parametrize("n, R", [(1536, 16), (768, 4), (768, 8)])
def test_related_pairs(gpu, tables, n, R):
    """10 % mutated copies: at n = 1536, R = 16 two stripes, both windows narrower than m; at 768 three (R = 4) and
    two (R = 8) stripes."""
    a, b = synth.related_codes(np.arange(6), n)
    _check(gpu, tables[True], list(a), list(b), R, True)


@pytest.mark.parametrize("user", [True, False])
def test_path_next_to_the_window_edge(gpu, tables, user):
    """b = a without its first s symbols, s random ones appended, with (insert + delete) s just under the diagonal's
    cost: the optimal path runs about s columns off the diagonal, beside the window's edge."""
    t = tables[user]
    rng = np.random.default_rng(99 + user)
    n = 1536
    a = rng.integers(0, 4, size=n).astype(np.uint8)
    tail = rng.integers(0, 4, size=n).astype(np.uint8)
    step = t["insert"] + t["delete"]
    A, B = [], []
    for s in range(n // 2, 0, -1):  # the largest s whose shift costs less than its own diagonal
        b = np.concatenate([a[s:], tail[:s]])
        if step * s < _diag_ub(t, a, b):
            break
    assert s > 64
    for ds in (0, 1, 7):  # s and a little less
        A.append(a)
        B.append(np.concatenate([a[s - ds:], tail[:s - ds]]))
    _check(gpu, t, A, B, 16, True)  # (the second stripe starts right of column 1)


def test_unequal_lengths(gpu, tables):
    """(1536, 1100) and (1100, 1536), str2 a mutated prefix / suffix / independent; then the same mixed with a 40-symbol
    pair and a pair of identical strings (UB 0, the narrowest window)."""
    rng = np.random.default_rng(4096)

    def mut(x):
        return np.where(rng.random(len(x)) < 0.1, rng.integers(0, 4, size=len(x)), x).astype(np.uint8)

    a = rng.integers(0, 4, size=1536).astype(np.uint8)
    A = [a, a, a, mut(a[:1100]), mut(a[436:]), rng.integers(0, 4, size=1100).astype(np.uint8)]
    B = [mut(a[:1100]), mut(a[436:]), rng.integers(0, 4, size=1100).astype(np.uint8), a, a, a]
    _check(gpu, tables[True], A, B, 16, True)
    A2 = A + [a[:40], a, a[:1100]]
    B2 = B + [mut(a[:40]), a.copy(), a[:1100].copy()]
    _check(gpu, tables[True], A2, B2, 16, True)
    _check(gpu, tables[False], A2, B2, 8, True)


def test_nothing_pruned(gpu, tables):
    """Independent random 1024 x 1024 at R = 16: one stripe, whose window reaches past both ends."""
    A, B = synth.pair_codes(np.arange(4), 1024, 0), synth.pair_codes(np.arange(4), 1024, 1)
    _check(gpu, tables[True], list(A), list(B), 16, False)
