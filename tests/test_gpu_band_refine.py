"""GPU: refined band windows of checkpoint script batches (SED_OPT_BAND 0 against 3, the static windows, and 2, off).
Every stripe below a pair's first narrows its chunk range from the row the stripe above left behind, and the traceback
reads the ranges the forward stored; distances, lengths and scripts must not change.  The shapes are the smallest with
a refined stripe that follows a refined stripe (three stripes) at each R.  Every batch: whole `ops` buffers, distances
and lengths equal between the three settings, every pair against the C oracle, err == 0 on every pair (results()
raises otherwise), and the chunks the forward ran (summed from the stored ranges) no more than under the static
windows."""
import os

import numpy as np
import pytest

from band_cases import mut as _mut, random_family as _batch
from conftest import padding_errors
import oracle
import sedcost
import sedgpu

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
S = "ACGU"


def _run(gpu, packed, R, band, times=1, dot=0, route=None):
    """dot: SED_OPT_DOT for the batch (2 = distance keys); route(batch, band): further asserts on the route taken."""
    gpu.set_option(sedgpu.SED_OPT_TB, 2)
    gpu.set_option(sedgpu.SED_OPT_CHAIN, 2)
    gpu.set_option(sedgpu.SED_OPT_SPLIT, 2)
    gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, R)
    gpu.set_option(sedgpu.SED_OPT_BAND, band)
    gpu.set_option(sedgpu.SED_OPT_DOT, dot)
    try:
        b = sedgpu.Batch(gpu, packed, True)
        try:
            outs = []
            for _ in range(times):
                b.run()
                outs.append(b.results())  # raises when any pair's err != 0
            assert b.traceback_mode == 2 and b.rows_per_lane == R
            if route is not None:
                route(b, band)
            return outs, b.band_chunks_run()
        finally:
            b.close()
    finally:
        gpu.set_option(sedgpu.SED_OPT_DOT, 0)
        gpu.set_option(sedgpu.SED_OPT_BAND, 0)
        gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, 0)
        gpu.set_option(sedgpu.SED_OPT_SPLIT, 0)
        gpu.set_option(sedgpu.SED_OPT_CHAIN, 0)
        gpu.set_option(sedgpu.SED_OPT_TB, 0)


def _check(gpu, table, A, B, R, times=1, dot=0, route=None):
    """Returns the refined run's first results and the (run, unpruned) chunks of the refined and the static run."""
    plan = sedcost.build_plan(table, [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    outs, chunks = _run(gpu, packed, R, 0, times, dot, route)
    (outs3, chunks3), (outs2, chunks2) = _run(gpu, packed, R, 3, 1, dot, route), _run(gpu, packed, R, 2, 1, dot, route)
    assert chunks2 is None and chunks is not None and chunks3 is not None
    print("R = %d: chunks run %d refined, %d static, %d unpruned" % (R, chunks[0], chunks3[0], chunks[1]))
    assert chunks[1] == chunks3[1] and chunks[0] <= chunks3[0] <= chunks[1]
    for d, ii, ln, ops in outs:
        for d0, ii0, ln0, ops0 in (outs3[0], outs2[0]):
            assert np.array_equal(ops, ops0), np.flatnonzero(ops != ops0)[:10]  # the whole buffer, padding included
            assert np.array_equal(d, d0) and np.array_equal(ln, ln0) and np.array_equal(ii, ii0)
    d, ii, ln, ops = outs[0]
    cs = oracle.Costs.from_plan(plan)
    P = packed.npairs
    od, oi, ol, oops, ooff = oracle.batch(cs, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b,
                                          packed.off_b, packed.len_b, P, want_ops=True, nthreads=THREADS)
    assert np.array_equal(d, od) and np.array_equal(ln, ol) and np.array_equal(ii.astype(bool), oi.astype(bool))
    bad = [p for p in range(P) if not np.array_equal(sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])),
                                                     oops[ooff[p]:ooff[p] + ol[p]])]
    assert not bad, bad[:10]
    assert not padding_errors(ops, packed.ops_off, packed.len_a, packed.len_b, ln)
    return outs[0], chunks, chunks3


def test_three_stripes_with_lane_pairs_r4(gpu, tables):
    rng = np.random.default_rng(600)
    A, B = _batch(rng, 600, 4)
    a = A[0]
    A += [a, a[:200], a[:9]]  # short str2: the lane-per-pair kernel's pairs between the wave pairs
    B += [_mut(rng, a[:20]), a[:5].copy(), a[:9].copy()]
    _check(gpu, tables[True], A, B, 4)


@pytest.mark.parametrize("user", [True, False])
def test_three_stripes_three_runs_r8(gpu, tables, user):
    A, B = _batch(np.random.default_rng(1100 + user), 1100, 8)
    _check(gpu, tables[user], A, B, 8, times=3)


def test_three_stripes_r16(gpu, tables):
    A, B = _batch(np.random.default_rng(2100), 2100, 16)
    _check(gpu, tables[True], A, B, 16)
