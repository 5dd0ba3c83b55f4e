"""GPU: every integer and lane route at the edges of its key range (tests/key_cases.py).  A gate or a decode that is
off by one faults nothing: it gives a plausible distance, or a valid script that is not the reference's.  So every batch
here sits on one of the planner's inequalities (tests/test_key_envelope.py proves that without a device) and every
comparison is for bit equality with the C oracle: distance, int / float typing, length, the script op by op and its zero
padding.  Each case first asserts its route from the Batch getters, so a table that is not eligible cannot quietly
pass on fp64, and prints it as one line: table, shape, mode and key format.

  1. the lane block: the three sed_lane_i32_kernel variants, the 16-bit halves, and the wave kernels on the same pairs;
  2. the i32_fits border on the wave kernels at R = 4, 8, 16: the last m that fits beside the first that does not;
  3. the L limit: 8192 and 15360 rows under i4_d4 and user_costs.json (D = 65260 with L >= 8192 on i4_d4/eq);
  4. CHAIN on the wide-ladder dot keys, the 3-bit ladder's and the perm ladder; integer SPLIT;
  5. the scaled lane kernel at its last accepted and first refused (insert, delete)."""
import os

import numpy as np
import pytest

from conftest import padding_errors
import key_cases as kc
import oracle
import sedcost
import sedgpu

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
MODES = {"i32": 1, "f64": 2, "f64-typed": 3}


_REFS = {}


def _reference(case):
    """The oracle's results of a batch, once per (table, pairs): shared by the cases that run it, never changed."""
    if case.ref not in _REFS:
        if len(_REFS) >= 4:  # (a test's cases come together: the few last batches are all it shares)
            _REFS.clear()
        plan = sedcost.build_plan(case.table, [case.alphabet], [case.alphabet])
        p = sedgpu.PackedPairs(case.A, case.B)
        out = oracle.batch(oracle.Costs.from_plan(plan), p.codes_a, p.off_a, p.len_a, p.codes_b, p.off_b, p.len_b,
                           p.npairs, want_ops=True, nthreads=THREADS)
        for x in out:
            x.setflags(write=False)
        _REFS[case.ref] = out
    return _REFS[case.ref]


def _getters(b):
    return {"mode": MODES[b.mode], "rows_per_lane": b.rows_per_lane, "lane_pairs": b.lane_pairs, "chains": b.chains,
            "traceback_mode": b.traceback_mode, "split_tasks": b.split_tasks, "packed_pairs": b.packed_pairs,
            "bitpar_pairs": b.bitpar_pairs, "scaled_pairs": b.scaled_pairs,
            "dot_keys": b.dot_keys | 2 * b.ladder_dot_keys | 4 * b.ladder_wide}


def _keys(case, r):
    if r["mode"] != 1:
        return "scaled integer" if r["scaled_pairs"] else "fp64"
    if r["dot_keys"] & 2:
        return "ladder dot keys, %s" % ("wide" if r["dot_keys"] & 4 else "3-bit")
    if r["traceback_mode"] in (2, 4):  # checkpoints: the forward runs without the L field, tiles are recomputed
        return "%s keys + tile recompute" % ("dot" if r["dot_keys"] & 1 else "distance")
    if r["packed_pairs"]:
        return "16-bit halves (%d pairs)" % r["packed_pairs"]
    return "length keys" if case.script or not case.no_len else "distance keys"


def run_case(gpu, case):
    """Creates the batch under the case's options, asserts its route, runs it and compares every pair with the oracle.
    Returns (dist, is_int, len, ops) and the getters."""
    plan = sedcost.build_plan(case.table, [case.alphabet], [case.alphabet])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(case.A, case.B)
    for key, val in case.opts.items():
        gpu.set_option(key, val)
    try:
        b = sedgpu.Batch(gpu, packed, case.script, no_len=case.no_len)
        try:
            r = _getters(b)
            print("%s: %s; mode %s, R = %d, %s, traceback %d, chains %d, SPLIT tasks %d" % (
                case.label, case.shape(), b.mode, r["rows_per_lane"], _keys(case, r), r["traceback_mode"], r["chains"],
                r["split_tasks"]))
            assert not kc.misses(case.expect, r), (case.label, kc.misses(case.expect, r))
            b.run()
            d, ii, ln, ops = b.results()  # raises when any pair's err != 0
        finally:
            b.close()
    finally:
        for key in case.opts:
            gpu.set_option(key, 0)
    od, oi, ol, oops, ooff = _reference(case)
    assert np.array_equal(d, od), (case.label, np.flatnonzero(d != od)[:10])
    assert np.array_equal(ii.astype(bool), oi.astype(bool)), case.label
    if case.script or not case.no_len:
        assert np.array_equal(ln, ol), (case.label, np.flatnonzero(ln != ol)[:10])
    if case.script:
        bad = [p for p in range(packed.npairs)
               if not np.array_equal(sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])), oops[ooff[p]:ooff[p] + ol[p]])]
        assert not bad, (case.label, bad[:10])
        assert not padding_errors(ops, packed.ops_off, packed.len_a, packed.len_b, ln), case.label
    return (d, ii, ln, ops), r


@pytest.mark.parametrize("name", kc.INT_NAMES)
def test_lane_block(gpu, name):
    """1. Every builder at n in {1, 16, 17, 255, 256, the largest that fits} x m in {1, 16, 17, 31, 32}: script,
    distance + length, distance only (two pairs per lane under `lt`) and distance only unpacked, then the same on the
    wave kernels.  Packed and unpacked runs give the same arrays."""
    got = {}
    for case in kc.lane_cases(name):
        got[case.label] = run_case(gpu, case)[0]
    for lane in (0, 2):
        d2, i2, _, _ = got["lane %s, dist, lane=%d" % (name, lane)]
        d0, i0, _, _ = got["lane %s, dist, pack off, lane=%d" % (name, lane)]
        assert np.array_equal(d0, d2) and np.array_equal(i0, i2)


@pytest.mark.parametrize("R", [4, 8, 16])
@pytest.mark.parametrize("name", kc.INT_NAMES)
def test_fits_border_on_the_wave_kernels(gpu, name, R):
    """2. For n in {1, 64 R, 64 R + 1} while some m fits: the batch at border[0] runs the integer kernel (per-cell
    codes, checkpoints, distance + length, distance only, and distance only with a partner that packs), the same batch
    with one pair at border[1] runs fp64; all exact."""
    ns = kc.border_ns(name, R)
    if not ns:
        print("border %s R=%d: 64 R padded rows alone pass the D field, nothing fits" % (name, R))
    for n in ns:
        for case in kc.border_cases(name, R, n):
            run_case(gpu, case)


@pytest.mark.parametrize("name", kc.L_TABLES)
def test_l_limit(gpu, name):
    """3. (8192, 8123) is the last that fits (npad + cols = 16383) and (8192, 8124) runs fp64; (15360, 955) fits;
    (1, 16251) does not (key_cases.l_cases), so (1, 16047) runs beside it.  One max-distance and one mutated pair per
    shape: script and distance only as planned (SPLIT at R = 4 for two long pairs), and script with SPLIT off, the
    stripe kernel's length keys at R = 16 with L past 8192 next to D = 65260."""
    for case in kc.l_cases(name):
        run_case(gpu, case)


@pytest.mark.parametrize("name, R", kc.CHAIN_CASES)
def test_chain_on_every_ladder(gpu, name, R):
    """4. Single-stripe pairs, m from 1 to the border, through CHAIN (dynamic and static chains of 3) under SED_OPT_DOT
    0, 2 and 3.  Where the ladder-dot factorisation is refused the batch runs the perm ladder: printed, not failed."""
    for case in kc.chain_cases(name, R):
        _, r = run_case(gpu, case)
        if case.opts[kc.O_DOT] != 2 and not r["dot_keys"] & 2:
            print("    (ladder-dot factorisation refused: perm ladder)")


@pytest.mark.parametrize("name, R", kc.SPLIT_CASES)
def test_integer_split_at_the_largest_shape(gpu, name, R):
    """4. SPLIT forced on one pair at the most stripes that fit at R, script and distance."""
    for case in kc.split_cases(name, R):
        run_case(gpu, case)


@pytest.mark.parametrize("name", kc.SCALED_NAMES)
def test_scaled_lane_kernel(gpu, name):
    """5. (15, 127) and (254, 1) run every lane pair on the scaled (or the bit-parallel) kernel, (16, 127) none; exact,
    and equal with the scaled kernel off and with the bit-parallel one off."""
    got = [run_case(gpu, case) for case in kc.scaled_cases(name)]
    (d, ii, _, _), r = got[0]
    if kc.SCALED_BASES[name][4]:
        assert r["scaled_pairs"] + r["bitpar_pairs"] == r["lane_pairs"] > 0
    else:
        assert r["scaled_pairs"] == 0
    for (d2, i2, _, _), _ in got[1:]:
        assert np.array_equal(d, d2) and np.array_equal(ii, i2)
