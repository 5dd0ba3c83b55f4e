"""GPU: bounded search (sed_batch_set_cutoff) across its envelope: the tables, families and cutoffs of
tests/cut_cases.py.  tests/test_gpu_cutoff.py runs two factorable tables on random or 10 % mutated pairs of two or three
stripes; that leaves unvisited what the windowed kernel restates of the checkpoint forward on its own bottom-row layout
(mismatches that tie with delete + insert, lopsided indels, distances next to the 16-bit limit, co-optimal paths out to
the window's edge, m of 1, 33, 63, 64, 65 and 64 c +- 1, a last stripe of one row, ten stripes whose window moves at each,
empty sides in the cutoff's pair list), the clamp and the floor of the cutoff, the fp64 filter one ulp either side of a
distance, and the hit counter of a pipelined batch.  A window one chunk too narrow, or a stale word of the in-place
buffer taken for this run's, faults nothing: it reports +inf for a pair within T or a value a little too large, which
only a comparison with the oracle on such inputs sees (tests/test_cut_envelope.py shows that these inputs would).

One resident batch per case runs every cutoff of cut_cases.cutoffs from the widest down to the narrowest and up again,
so that a narrow run meets a wide run's words in the bottom-row buffer.  Every run is held to test_gpu_cutoff's
_contract against the C oracle, bit for bit, its hit count, its route (integer mode at the forced R, one wave per
pair) and the cells the host's restatement says the cutoff keeps."""
import time

import numpy as np
import pytest

import band_cases as bc
import cut_cases as cc
import sedcost
import sedgpu
from test_gpu_cutoff import INF, S, STRIPE, _Batch, _contract, _oracle

pytestmark = pytest.mark.gpu
O = sedgpu


def _same(x, y):
    return all(np.array_equal(u, v) for u, v in zip(x[:3], y[:3]))


def _down_and_up(Ts, times=1):
    """Widest to narrowest and back up, `times` over."""
    down = sorted(Ts, reverse=True)
    return (down + down[-2::-1]) * times


def _envelope(gpu, name, family, R, n=None, times=1, extra=(), opts=(), check_cells=True):
    """Every cutoff of the case on one resident batch of the windowed stripe route; {T: (results, hits, cells)}."""
    t0 = time.perf_counter()
    A, B = cc.pairs(name, family, R, n)
    sub, ins, dele = bc.costs(name)
    plan = sedcost.build_plan(bc.TABLES[name], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    Ts = sorted(set(cc.cutoffs(ref[0], ins, dele, [(len(a), len(b)) for a, b in zip(A, B)])) | set(extra))
    with _Batch(gpu, packed, STRIPE + tuple(opts), R) as fresh:
        fresh.run()
        want = fresh.results()
        nominal = fresh.work()[0]
        assert fresh.cutoff_hits() == packed.npairs and fresh.band_cells == nominal
    assert _contract(want, ref, INF) == packed.npairs
    seen = {}
    with _Batch(gpu, packed, STRIPE + tuple(opts), R) as b:
        for T in _down_and_up(Ts, times):
            b.set_cutoff(T)
            assert b.mode == "i32" and b.rows_per_lane == R and b.traceback_mode == 0 and b.lane_pairs == 0
            assert b.chains == b.packed_pairs == b.split_tasks == 0
            b.run()
            out = b.results()
            hits = _contract(out, ref, T)
            assert b.cutoff_hits() == hits, T
            assert b.work()[0] == nominal and b.band_cells <= nominal
            if check_cells:
                cells, host_nominal = cc.batch_cells(sub, ins, dele, A, B, R, T)
                assert host_nominal == nominal and b.band_cells == cells, (T, b.band_cells, cells)
            if T in seen:  # the way up: what the way down gave
                assert _same(out, seen[T][0]) and (hits, b.band_cells) == seen[T][1:], T
            seen[T] = (out, hits, b.band_cells)
        b.set_cutoff(INF)
        b.run()
        assert _same(b.results(), want) and b.cutoff_hits() == packed.npairs and b.band_cells == nominal
    for T in Ts:
        if T != np.floor(T) and T < cc.KEY_MAX:  # a fractional cutoff is its floor
            assert _same(seen[T][0], seen[float(np.floor(T))][0]) and seen[T][1:] == seen[float(np.floor(T))][1:], T
        if T >= cc.KEY_MAX:  # the clamp: every integer distance is within
            assert _same(seen[T][0], want) and seen[T][1] == packed.npairs, T
    cells = [seen[T][2] for T in Ts]
    assert cells == sorted(cells)  # monotone in T
    if check_cells:
        dmin = float(ref[0].min())
        assert seen[dmin][2] < nominal and seen[dmin][1] >= 1  # the related pairs at T = D: pruned, and within
    print("%s / %s, R = %d, %d pairs, %d cutoffs x %d, nominal %.0f, %.2f s; T: cells  %s" % (
        name, family, R, packed.npairs, len(Ts), 2 * times, nominal, time.perf_counter() - t0,
        "  ".join("%g: %.0f" % (T, c) for T, c in zip(Ts, cells))))
    return ref, Ts, seen, nominal


@pytest.mark.parametrize("name", list(bc.TABLES))
def test_tables_by_families_r4(gpu, name):
    """Every table against the random, the low-complexity and the rearranged family: three stripes of 256 rows (`heavy`
    with m - n within cut_cases.DELTA)."""
    for family in ("random", "low_complexity", "rearranged"):
        _envelope(gpu, name, family, 4)


@pytest.mark.parametrize("name, R", [("user_costs.json", 4), ("tight", 4), ("user_costs.json", 8)])
@pytest.mark.parametrize("family", ["edges", "short_m"])
def test_stripe_and_chunk_borders(gpu, family, name, R):
    """Last stripes of one row and of ROWS rows against m = 1, 63, 64, 65, 64 c, 64 c + 1 and 5 n (edges), and
    n = 2 ROWS + 1 against m = 33, 34, 63 (short_m)."""
    _envelope(gpu, name, family, R)


@pytest.mark.parametrize("name", ["user_costs.json", "gui_int"])
def test_ten_stripes_of_drift(gpu, name):
    """Eleven stripes whose window starts and ends a chunk further at each; the whole list of cutoffs twice over."""
    _envelope(gpu, name, "drift", 4, times=2)


@pytest.mark.parametrize("family", ["low_complexity", "rearranged"])
def test_r16(gpu, family):
    """R = 16: three stripes of 1024 rows (n = 2100) under user_costs.json."""
    _envelope(gpu, "user_costs.json", family, 16, n=2100)


def test_empty_sides(gpu):
    """(0, 0), (0, 300) and (300, 0) in the cutoff's pair list between wave pairs: (0, 300) is within exactly when
    300 insert <= T, (300, 0) when 300 delete <= T, (0, 0) always, and the other pairs are what the oracle says."""
    _, ins, dele = bc.costs("user_costs.json")
    edge = [300 * ins - 1, 300 * ins, 300 * dele - 1, 300 * dele]
    ref, Ts, seen, _ = _envelope(gpu, "user_costs.json", "empty_sides", 4, extra=edge)
    p0, pi, pd = (cc.EMPTY_PAIRS[k] for k in ("none", "insert", "delete"))
    assert ref[0][p0] == 0 and ref[0][pi] == 300 * ins and ref[0][pd] == 300 * dele
    for T in Ts:
        d = seen[T][0][0]
        assert d[p0] == 0
        assert d[pi] == (300 * ins if 300 * ins <= T else INF), T
        assert d[pd] == (300 * dele if 300 * dele <= T else INF), T


@pytest.mark.parametrize("name, kind", [("sum", "related"), ("fact", "related"), ("sum", "independent")])
def test_default_option_route(gpu, name, kind):
    """1536 x 1536 pairs under default options.  40 run SPLIT, which no cutoff moves: the filter only.  260 start two per
    wave under `fact` and on the plain stripe kernel under `sum` (a mismatch that costs delete + insert does not pack);
    a cutoff moves them to the window exactly when the host's restatement keeps less than the share of their cells
    (2/3 from two pairs per wave, any saving from the plain kernel), +inf moves them back, and the contract holds on
    either side.  Independent pairs under `sum` prune nothing under their own diagonal's bound and stay."""
    t0 = time.perf_counter()
    sub, ins, dele = bc.costs(name)
    plan = sedcost.build_plan(bc.TABLES[name], [S], [S])
    gpu.set_costs(plan)
    A, B = cc.route_pairs(kind, cc.ROUTE_MANY)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    med = float(np.sort(ref[0])[len(A) // 2])
    # the 40: SPLIT before and after
    few = sedgpu.PackedPairs(A[:cc.ROUTE_FEW], B[:cc.ROUTE_FEW])
    ref_few = tuple(x[:cc.ROUTE_FEW] for x in ref)
    with _Batch(gpu, few) as b:
        tasks = b.split_tasks
        assert b.mode == "i32" and tasks > 0 and b.packed_pairs == b.chains == 0
        for T in (med, 100.0, INF):
            b.set_cutoff(T)
            assert b.split_tasks == tasks and b.band_cells == b.work()[0]
            b.run()
            assert b.cutoff_hits() == _contract(b.results(), ref_few, T)
    # the 260
    with _Batch(gpu, packed) as fresh:
        fresh.run()
        want = fresh.results()
    start = cc.ROUTE_MANY if name == "fact" else 0
    line, windowed = [], set()
    with _Batch(gpu, packed) as b:
        nominal, R = b.work()[0], b.rows_per_lane
        assert b.mode == "i32" and R == 16 and b.packed_pairs == start and b.chains == b.split_tasks == b.lane_pairs == 0
        share = 2 / 3 if start else 1.0
        for T in (med, 100.0, 300.0, 600.0, 1000.0, 60000.0, INF, med - 1):
            cells, host_nominal = cc.batch_cells(sub, ins, dele, A, B, R, T)
            assert host_nominal == nominal
            if T == 60000.0:  # no tighter than any pair's diagonal bound: the band cells of SED_OPT_BAND
                assert cells == sum(sedgpu.band_cells(sub, ins, dele, a, b_, R) for a, b_ in zip(A, B))
            win = T != INF and cells < share * nominal
            b.set_cutoff(T)
            assert b.packed_pairs == (0 if win else start) and b.chains == b.split_tasks == 0, (T, cells / nominal)
            assert b.band_cells == (cells if win else nominal), (T, b.band_cells, cells)
            b.run()
            out = b.results()
            assert b.cutoff_hits() == _contract(out, ref, T)
            if T == INF:
                assert _same(out, want)
            windowed.add(win)
            line.append("%g: %.3f%s" % (T, cells / nominal, " win" if win else ""))
        assert True in windowed and False in windowed
    if (name, kind) == ("sum", "independent"):
        assert "60000: 1.000" in line  # nothing pruned: they stayed
    print("%s / %s 1536 x 1536, default options, R = %d, %d pairs start %s, %.2f s; T: share  %s" % (
        name, kind, R, len(A), "two per wave" if start else "on the plain stripe kernel", time.perf_counter() - t0,
        "  ".join(line)))


def test_cut_option_1_and_2_agree(gpu):
    """SED_OPT_CUT = 1 (always the window) and 2 (never) on one batch: the same result arrays and hit counts for every
    cutoff; 2 runs every cell."""
    ran = {}
    for v in (1, 2):
        _, Ts, seen, nominal = _envelope(gpu, "user_costs.json", "rearranged", 4, opts=((O.SED_OPT_CUT, v),),
                                         check_cells=v == 1)
        ran[v] = (Ts, seen)
        assert v == 1 or all(seen[T][2] == nominal for T in Ts)
    assert ran[1][0] == ran[2][0]
    for T in ran[1][0]:
        assert _same(ran[1][1][T][0], ran[2][1][T][0]) and ran[1][1][T][1] == ran[2][1][T][1], T
    assert any(ran[1][1][T][2] < nominal for T in ran[1][0])


@pytest.mark.parametrize("name", sorted(cc.F64_ROUTES))
def test_filter_only_fp64(gpu, name):
    """costs.json with IUPAC symbols on one wave per pair, 16-lane segments, forced SPLIT and the fp64 lane kernels
    (scaled-integer and bit-parallel pairs): the filter compares the fp64 value itself, so the median pair is within at
    T = D and one ulp above, and beyond one ulp below."""
    t0 = time.perf_counter()
    _, _, opts, pos, zero, want_len = cc.f64_route(name)
    plan, packed = cc.f64_plan(name)
    gpu.set_costs(plan)
    ref = _oracle(plan, packed)
    p = int(np.argsort(ref[0], kind="stable")[packed.npairs // 2])
    D = float(ref[0][p])
    with _Batch(gpu, packed, tuple(opts.items())) as b:
        assert b.mode != "i32" and all(getattr(b, k) > 0 for k in pos) and all(getattr(b, k) == 0 for k in zero)
        b.run()
        want = b.results()
        assert _contract(want, ref, INF, want_len=want_len) == packed.npairs
        line = []
        for T, keeps in ((D, True), (float(np.nextafter(D, 0)), False), (float(np.nextafter(D, INF)), True),
                         (0.0, None), (1e300, None), (D, True)):
            b.set_cutoff(T)
            assert b.band_cells == b.work()[0]
            b.run()
            out = b.results()
            hits = _contract(out, ref, T, want_len=want_len)
            assert b.cutoff_hits() == hits
            if keeps is not None:
                assert out[0][p] == (D if keeps else INF), (T, D, out[0][p])
            line.append("%r: %d" % (T, hits))
        assert 0 < int((ref[0] <= D).sum()) < packed.npairs
        b.set_cutoff(INF)
        b.run()
        assert _same(b.results(), want)
    print("costs.json / fp64 %s, %d pairs, median D = %r, %.2f s; T: hits  %s" % (
        name, packed.npairs, D, time.perf_counter() - t0, "  ".join(line)))


def test_pipelined_batch_counts_hits_in_its_current_slot(gpu, tables):
    """2000 lane pairs, distance only, created with SED_PIPELINE: three runs under one cutoff without reading any, then
    results and hits; two more under another, so that the batch has met its odd and its even slot."""
    t0 = time.perf_counter()
    A, B = cc.lane_pairs()
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    d = np.sort(ref[0])
    b = sedgpu.Batch(gpu, packed, False, pipeline=True, no_len=True)
    try:
        assert b.mode == "i32" and b.lane_pairs == packed.npairs
        line = []
        for T, runs in ((float(d[len(d) // 2]), 3), (float(d[len(d) // 4]) + 0.5, 2), (INF, 1), (float(d[0]), 1)):
            b.set_cutoff(T)
            for _ in range(runs):
                b.run()
            hits = _contract(b.results(), ref, T)
            assert b.cutoff_hits() == hits and (T == INF or 0 < hits < packed.npairs)
            line.append("%g x %d: %d" % (T, runs, hits))
    finally:
        b.close()
    print("user_costs.json / pipelined lane pairs, %d pairs, %.2f s; T x runs: hits  %s" % (
        packed.npairs, time.perf_counter() - t0, "  ".join(line)))
