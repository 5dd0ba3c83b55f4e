"""GPU: the rows-per-lane rule of banded checkpoint batches (csrc/sed_plan.cpp: band_rows_rule; DESIGN.md 3.6c, "Rows per
lane") on the smallest batch that reaches it: 260 pairs (past the checkpoint route's 256) of n in {2048, 2049, 2111}
rows (the gate's edge, one row and one chunk past it) against m in {1990, 2048, 2300} columns under user_costs.json,
automatic options.  The families are those of tests/band_cases.py: identical, 10 % mutated, unrelated, and one block
deleted inside a stripe; str2 is cut or extended with random symbols to m.  The batch must run at the R the planner
reports for the same fill, give bit for bit what the same batch gives at R = 16, agree with the C oracle op by op,
and run fewer forward steps than at R = 16.  One pair of 2047 rows more closes the gate: R = 16, same results."""
import os

import numpy as np
import pytest

from band_cases import mut
from conftest import load_golden, padding_errors
import oracle
import plan_route_cases as pc
import sedcost
import sedgpu

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
S = "ACGU"
NS, MS, PAIRS = (2048, 2049, 2111), (1990, 2048, 2300), 260


def _pairs():
    rng = np.random.default_rng(20482300)
    r = lambda k: rng.integers(0, 4, size=k).astype(np.uint8)  # noqa: E731
    A, B = [], []
    for p in range(PAIRS):
        n, m, fam = NS[p % 3], MS[(p // 3) % 3], (p // 9) % 4
        a = r(n)
        b = (a.copy(), mut(rng, a), r(n), np.concatenate([a[:300], a[450:]]))[fam]  # (rows 300..449: inside a stripe at every R)
        A.append(a)
        B.append(np.concatenate([b, r(max(m - len(b), 0))])[:m])
    return A, B


def _run(gpu, packed, R):
    """One run at SED_OPT_ROWS_PER_LANE = R (0: automatic): (results, R the batch ran, forward steps of its chunks)."""
    gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, R)
    try:
        b = sedgpu.Batch(gpu, packed, True)
        try:
            b.run()
            out = b.results()  # raises when any pair's err != 0
            chunks = b.band_chunks_run()
            assert b.mode == "i32" and b.traceback_mode == 2 and chunks is not None  # (band windows stored)
            return out, b.rows_per_lane, chunks[0] * 64 * b.rows_per_lane
        finally:
            b.close()
    finally:
        gpu.set_option(sedgpu.SED_OPT_ROWS_PER_LANE, 0)


@pytest.fixture(scope="module")
def runs(gpu):
    plan = sedcost.build_plan(load_golden("user_costs.json"), [S], [S])
    gpu.set_costs(plan)
    A, B = _pairs()
    packed = sedgpu.PackedPairs(A, B)
    return plan, A, B, packed, _run(gpu, packed, 0), _run(gpu, packed, 16)


def test_the_batch_runs_at_the_planned_r_and_gives_the_r16_results(runs):
    plan, A, B, packed, (auto, R, steps), (ref, R16, steps16) = runs
    want = sedgpu.plan_routes(pc._costs(True, S), {}, packed, sedgpu.SED_WANT_SCRIPT)
    print("R = %d (planned %d): %d forward steps against %d at R = 16" % (R, want["rows_per_lane"], steps, steps16))
    assert R == want["rows_per_lane"] and R16 == 16 and want["traceback_mode"] == 2
    for x, y in zip(auto, ref):  # distance, is_int, length and the whole ops buffer, padding included
        assert np.array_equal(x, y)
    assert steps < steps16


def test_every_pair_equals_the_oracle(runs):
    plan, A, B, packed, ((d, ii, ln, ops), _, _), _ = runs
    cs = oracle.Costs.from_plan(plan)
    P = packed.npairs
    od, oi, ol, oops, ooff = oracle.batch(cs, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b, packed.off_b,
                                          packed.len_b, P, want_ops=True, nthreads=THREADS)
    assert np.array_equal(d, od) and np.array_equal(ln, ol) and np.array_equal(ii.astype(bool), oi.astype(bool))
    bad = [p for p in range(P) if not np.array_equal(sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])),
                                                     oops[ooff[p]:ooff[p] + ol[p]])]
    assert not bad, bad[:10]
    assert not padding_errors(ops, packed.ops_off, packed.len_a, packed.len_b, ln)


def test_one_pair_below_the_gate_runs_the_batch_at_r16(gpu, runs):
    plan, A, B, packed, ((d, ii, ln, ops), _, _), _ = runs
    gpu.set_costs(plan)
    more = sedgpu.PackedPairs(A + [A[0][:2047]], B + [B[0]])
    (d2, ii2, ln2, ops2), R, _ = _run(gpu, more, 0)
    assert R == 16 == sedgpu.plan_routes(pc._costs(True, S), {}, more, sedgpu.SED_WANT_SCRIPT)["rows_per_lane"]
    P, words = packed.npairs, int(packed.ops_off[packed.npairs])
    assert np.array_equal(more.ops_off[:P + 1], packed.ops_off[:P + 1])
    assert np.array_equal(d2[:P], d) and np.array_equal(ln2[:P], ln) and np.array_equal(ii2[:P], ii)
    assert np.array_equal(ops2[:words], ops[:words])
