"""GPU: the fp64 pair kernels across the alphabet and numeric envelope they promise (tests/f64_pair_cases.py): tables
of 17, 31 and 32 symbols whose every entry is live, a typed one, a unit-cost subset in the mask's top four bits, sums
that tie or sit 1 ulp apart, values at +-inf and subnormals, on every route of the family: one wave per pair at R = 4
and 8, 16-lane segments, SPLIT at R = 2 and 4, the lane kernel and the full matrix.  A wrong stride, a table load that
stops early, a reassociated add or a half-word dropped at a hand-off faults nothing: it gives a plausible distance, or a
valid script that is not the reference's.  So every comparison is for equality with the C oracle: distance (==, so inf
equals inf; the sign of a zero is not compared), int / float typing, length, the script op by op and its zero padding.
Each case first asserts its route from the Batch getters (tests/test_f64_pair_cases.py proves the same without a
device), so a table that slid to the integer or the scaled route cannot quietly pass, and prints it as one line."""
import os

import numpy as np
import pytest

from conftest import padding_errors
import f64_pair_cases as fc
import oracle
import sedcost
import sedgpu

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
MODES = {"i32": 1, "f64": 2, "f64-typed": 3}

_REFS = {}


def _plan(case):
    return sedcost.build_plan(case.table, [case.alphabet], [case.alphabet])


def _reference(case):
    """The oracle's results of a batch, once per (table, pairs): shared by the cases that run it, never changed."""
    if case.ref not in _REFS:
        if len(_REFS) >= 4:  # (a test's cases come together: the few last batches are all it shares)
            _REFS.clear()
        p = sedgpu.PackedPairs(case.A, case.B)
        out = oracle.batch(oracle.Costs.from_plan(_plan(case)), p.codes_a, p.off_a, p.len_a, p.codes_b, p.off_b, p.len_b,
                           p.npairs, want_ops=True, nthreads=THREADS)
        for x in out:
            x.setflags(write=False)
        _REFS[case.ref] = out
    return _REFS[case.ref]


def _getters(b):
    return {"mode": MODES[b.mode], "rows_per_lane": b.rows_per_lane, "lane_pairs": b.lane_pairs,
            "segment_pairs": b.segment_pairs, "split_tasks": b.split_tasks, "bitpar_pairs": b.bitpar_pairs,
            "scaled_pairs": b.scaled_pairs, "traceback_mode": b.traceback_mode}


def run_case(gpu, case):
    """Sets the case's mode, costs and options, creates the batch, prints and asserts its route, runs it and compares
    every pair with the oracle; every option is reset on the way out.  Returns (dist, is_int, len, ops)."""
    gpu.set_mode(case.mode)
    try:
        gpu.set_costs(_plan(case))
        packed = sedgpu.PackedPairs(case.A, case.B)
        for key, val in case.opts.items():
            gpu.set_option(key, val)
        b = sedgpu.Batch(gpu, packed, case.script, no_len=case.no_len)
        try:
            r = _getters(b)
            print("%s: %s; mode %s, R = %d, lane pairs %d (bit-parallel %d), segment pairs %d, SPLIT tasks %d, "
                  "traceback %d" % (case.label, case.shape(), b.mode, r["rows_per_lane"], r["lane_pairs"],
                                    r["bitpar_pairs"], r["segment_pairs"], r["split_tasks"], r["traceback_mode"]))
            assert not fc.misses(case.expect, r), (case.label, fc.misses(case.expect, r))
            b.run()
            d, ii, ln, ops = b.results()  # raises when any pair's err != 0
        finally:
            b.close()
    finally:
        for key in case.opts:
            gpu.set_option(key, 0)
        gpu.set_mode(0)
    od, oi, ol, oops, ooff = _reference(case)
    assert not np.isnan(d).any() and not np.isnan(od).any(), case.label
    assert np.array_equal(d, od), (case.label, np.flatnonzero(d != od)[:10])
    assert np.array_equal(ii.astype(bool), oi.astype(bool)), (case.label, np.flatnonzero(ii.astype(bool) != oi.astype(bool))[:10])
    if case.script or not case.no_len:
        assert np.array_equal(ln, ol), (case.label, np.flatnonzero(ln != ol)[:10])
    if case.script:
        bad = [p for p in range(packed.npairs)
               if not np.array_equal(sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])), oops[ooff[p]:ooff[p] + ol[p]])]
        assert not bad, (case.label, bad[:10])
        assert not padding_errors(ops, packed.ops_off, packed.len_a, packed.len_b, ln), case.label
    return d, ii, ln, ops


@pytest.mark.parametrize("R", fc.WAVE_R)
@pytest.mark.parametrize("name", fc.WAVE_TABLES)
def test_one_wave_per_pair(gpu, name, R):
    """sed_wf_f64_kernel, SW = 64: n in {1, 64 R - 1, 64 R, 64 R + 1} x m in {1, 63, 64, 65, 130}, with the sweep of the
    tables past 16 symbols; script, distance + length and distance only, simple and typed."""
    for case in fc.wave_cases(name, R):
        run_case(gpu, case)


@pytest.mark.parametrize("R", fc.WAVE_R)
@pytest.mark.parametrize("name", fc.WAVE_TABLES)
def test_segments(gpu, name, R):
    """sed_wf_f64_kernel, SW = 16: n in {1, 16 R - 1, 16 R, 16 R + 1, 32 R + 1} x m in {1, 15, 16, 17, 40} and the
    sweep, filled to 300 pairs, every one of them in a segment."""
    for case in fc.seg_cases(name, R):
        assert case.expect["segment_pairs"] == len(case.A) > 0
        run_case(gpu, case)


@pytest.mark.parametrize("R", fc.SPLIT_R)
@pytest.mark.parametrize("name", fc.WAVE_TABLES)
def test_split(gpu, name, R):
    """sed_wf_f64_split_kernel forced: two and three stripes against m in {1, 63, 64, 65, 255, 256, 257}; every value
    crosses a stripe as two tagged halves, the typing bit inside the L key."""
    for case in fc.split_cases(name, R):
        assert case.expect["split_tasks"] > 0
        run_case(gpu, case)


@pytest.mark.parametrize("name", fc.LANE_TABLES)
def test_lane_kernel(gpu, name):
    """sed_lane_f64_kernel: n in {1, 2, 255, 512} x m in {1, 31, 32} and the sweep, distance only.  Under
    k32_unit_high the pairs inside the last four symbols run bit-parallel; switched off, the batch gives the same.
    Under n_first (N as code 0) the subset is codes 1..4: the pairs with an N run sed_lane_scaled_kernel and the others
    its bit-parallel branch; with either switched off the batch gives the same."""
    cases = fc.lane_cases(name)
    got = [run_case(gpu, case) for case in cases]
    assert cases[0].expect["lane_pairs"] == len(cases[0].A) > 0
    if name in fc.UNIT_LO:
        assert cases[0].expect["bitpar_pairs"] == len(fc.in_unit_subset(name, cases[0].A, cases[0].B)) > 0
        for other in got[1:]:
            assert np.array_equal(got[0][0], other[0]) and np.array_equal(got[0][1], other[1])


@pytest.mark.parametrize("route", list(fc.FULL_SHAPES))
@pytest.mark.parametrize("name", fc.FULL_TABLES)
def test_full_matrix(gpu, name, route):
    """sed_full_matrix: every cell's value, edge mask and typing bit against the oracle's matrices, 70 x 70 on the
    one-wave kernel (SPLIT off) and 300 x 90 on SPLIT.  sed_full_matrix has no getters: which kernel a pair runs is
    what its planner call decides under mode 2 (simple typing), R = 4, no flags and the context's SED_OPT_SPLIT, and
    f64_pair_cases.full_case restates exactly those settings, so tests/test_f64_pair_cases.py proves the route on the
    CPU (split_tasks 0 and 2).  If sed_full_matrix changes what it plans with, full_case has to follow."""
    case = fc.full_case(name, route)
    (a,), (b,) = case.A, case.B
    gpu.set_costs(_plan(case))
    split_off = case.opts.get(fc.O_SPLIT, 0)
    gpu.set_option(fc.O_SPLIT, split_off)
    try:
        D, M = gpu.full_matrix(a, b)
    finally:
        gpu.set_option(fc.O_SPLIT, 0)
    print("%s: %d x %d, SED_OPT_SPLIT = %d" % (case.label, len(a), len(b), split_off))
    o = oracle.pair(oracle.Costs.from_plan(_plan(case)), a, b, want_ops=False, full=True)
    assert not np.isnan(D).any() and not np.isnan(o["D"]).any()
    assert np.array_equal(D, o["D"]), (case.label, np.argwhere(D != o["D"])[:10])
    assert np.array_equal(M & 7, o["M"]), (case.label, np.argwhere((M & 7) != o["M"])[:10])
    assert np.array_equal(M >> 3, o["T"]), (case.label, np.argwhere((M >> 3) != o["T"])[:10])
