"""CPU: bounded search (sed_batch_set_cutoff) across the envelope of tests/cut_cases.py, without a
device.

Window property.  Under a cutoff T the windowed kernel runs the band of ub = min(T, the diagonal's bound UB).  "<= T"
stays exact as long as every cell some path of cost <= ub passes through lies inside the window of diagonals
(sedgpu.band_bounds) and inside the chunk range its stripe runs (sedgpu.band_chunk_range, cell (i, j) of lane
t = (i - 1) % (64 R) / R at step j - 1 + t, chunk (j - 1 + t) >> 6).  Checked against a forward plus backward DP in
numpy for T = D, D + 1, D + insert + delete and min(UB, 2 D + 3); tests/test_band_bound.py does it for ub = UB and
optimal cells only, and T = D, the narrowest window that still has to hold a path, is not implied by it.

The inputs bite.  At T = D there are stripes whose leftmost chunk, and others whose rightmost chunk, holds such a cell,
so a range one chunk narrower on either side would lose it; stripes that start at a later chunk than the stripe above
(the forward's `clo > clo_prev` load), and stripes that run past the last chunk of the stripe above (whose words of the
in-place bottom-row buffer past top_hi are stale).  sed_band_chunks makes both ends nondecreasing in the stripe
(tests/test_band_bound.py asserts it), so a stripe never ends below the one above: the count of that is printed too,
and is 0.

Host arithmetic.  Every batch tests/test_gpu_cut_envelope.py runs plans as the integer stripe route its window replaces,
its schedule has a WIN step exactly under cut_win and ends its DP phase with FILTER, the default-option and fp64 batches
take the routes the GPU test asserts, and the restatement of the kept cells (cut_cases.window_cells) is
sedgpu.band_cells where the cutoff is no tighter than the diagonal's bound."""
import functools

import numpy as np
import pytest

import band_cases as bc
import cut_cases as cc
import sedgpu

O = sedgpu
COUNTS = ("stripes", "left", "left_inside", "right", "right_inside", "clo_moves", "chi_moves", "chi_falls", "cutoffs")


def _extremes(mask):
    """Per row of a boolean matrix: whether it has a true cell, its first and its last true column."""
    return mask.any(axis=1), mask.argmax(axis=1), mask.shape[1] - 1 - mask[:, ::-1].argmax(axis=1)


def _check_pair(sub, ins, dele, a, b, R, counts):
    n, m, rows = len(a), len(b), 64 * R
    F = bc.dp(sub, ins, dele, a, b)
    through = F + bc.dp(sub, ins, dele, a[::-1], b[::-1])[::-1, ::-1]  # the cheapest path through each cell
    D = float(F[n, m])
    gap, ub = cc.gap_cost(n, m, ins, dele), cc.diag_bound(sub, ins, dele, a, b)
    assert gap <= D <= ub
    i = np.arange(n + 1)
    stripe, lane = (i - 1) // rows, ((i - 1) % rows) // R  # (row 0 is the border: never read below)
    for T in sorted({D, D + 1, D + ins + dele, min(ub, 2 * D + 3)}):
        assert T >= gap
        w = min(T, ub)
        elo, ehi = sedgpu.band_bounds(n, m, ins, dele, w)
        assert elo <= min(0, m - n) and ehi >= max(0, m - n)
        mask = through <= w
        has, jmin, jmax = _extremes(mask)
        assert has.all()  # a path of cost D <= w crosses every row
        assert (jmin - i).min() >= elo and (jmax - i).max() <= ehi, (n, m, T, elo, ehi)  # (a)
        # (b) the cells the kernel computes: rows and columns >= 1
        has, jmin, jmax = _extremes(mask[:, 1:])
        jmin, jmax = jmin + 1, jmax + 1
        has[0] = False
        first, last = (jmin - 1 + lane) >> 6, (jmax - 1 + lane) >> 6
        prev = None
        for k in range((n + rows - 1) // rows):
            clo, chi, nchunks = sedgpu.band_chunk_range(n, m, R, elo, ehi, k)
            sel = has & (stripe == k)
            if sel.any():
                assert first[sel].min() >= clo and last[sel].max() <= chi, (n, m, T, k, clo, chi)
            if T == D:
                counts["stripes"] += 1
                if sel.any():
                    left, right = first[sel].min() == clo, last[sel].max() == chi
                    counts["left"] += left
                    counts["left_inside"] += left and clo > 0
                    counts["right"] += right
                    counts["right_inside"] += right and chi < nchunks - 1
                if prev is not None:
                    counts["clo_moves"] += clo > prev[0]
                    counts["chi_moves"] += chi > prev[1]
                    counts["chi_falls"] += chi < prev[1]
            prev = (clo, chi)
        counts["cutoffs"] += 1
    if gap >= 1:  # one below the length difference's cost: no path at all, and the engine runs no stripe
        assert not (through <= gap - 1).any()


@functools.lru_cache(maxsize=None)
def _check_case(name, family, R, n):
    """The window property over one batch's non-empty pairs; its bites at T = D (computed once per session)."""
    sub, ins, dele = bc.costs(name)
    A, B = cc.pairs(name, family, R, n)
    counts = dict.fromkeys(COUNTS, 0)
    for a, b in zip(A, B):
        if len(a) and len(b):
            _check_pair(sub, ins, dele, a, b, R, counts)
    return counts


@pytest.mark.parametrize("name, family, R, n", cc.MODEL_CASES)
def test_window_holds_every_path_within_the_cutoff(name, family, R, n):
    assert _check_case(name, family, R, n)["cutoffs"] > 0


@pytest.mark.parametrize("name, family, R", [("user_costs.json", "short_m", 4), ("tight", "short_m", 4),
                                             ("user_costs.json", "short_m", 8), ("user_costs.json", "empty_sides", 4)])
def test_window_of_the_families_of_this_module(name, family, R):
    """short_m and empty_sides' real pairs, as above (their bites are not counted: the evidence is asked of the
    families the band tests share)."""
    assert _check_case(name, family, R, None)["cutoffs"] > 0


def test_the_inputs_bite():
    """Over the whole set at T = D (the counts of the window tests above, which a session computes once)."""
    total = dict.fromkeys(COUNTS, 0)
    for case in cc.MODEL_CASES:
        for key, v in _check_case(*case).items():
            total[key] += int(v)
    print("cut envelope, T = D: " + ", ".join("%s %d" % kv for kv in total.items()))
    for key in ("left", "left_inside", "right", "right_inside", "clo_moves", "chi_moves"):
        assert total[key] > 0, key
    assert total["chi_falls"] == 0


# ---- host arithmetic ----
def test_cutoffs():
    T = cc.cutoffs(np.array([40.0, np.inf, 7.0, 90.0, 12.0]), 2.0, 3.0, [(5, 5), (0, 300), (30, 20), (20, 40)])
    want = {0, 65535, 65536.5, 1e300, 30, 29}  # (30, 20): ten deletes
    for D in (7, 40, 90):
        want |= {D - 1, D - 0.5, D, D + 0.5, D + 1}
    assert T == sorted(want)
    assert cc.cutoffs([0.0, 0.0], 1.0, 1.0, [(3, 3), (3, 3)]) == [0, 0.5, 1, 65535, 65536.5, 1e300]  # none below 0
    assert [cc.cut_key(t) for t in (0, 6.5, 65535, 65536.5, 1e300)] == [0, 6, 65535, 65535, 65535]


def test_heavy_is_trimmed_until_it_fits():
    """`heavy` (insert 20, delete 60) keeps every family of the GPU test on the 16-bit keys only with m - n within
    cut_cases.DELTA: the first of HEAVY_STEPS at which all of HEAVY_FAMILIES plan as i32."""
    saved = cc.DELTA["heavy"]
    try:
        fits = {}
        for d in cc.HEAVY_STEPS:
            cc.DELTA["heavy"] = d
            fits[d] = all(cc.distance_fits("heavy", *cc.pairs("heavy", f, 4), 4) for f in cc.HEAVY_FAMILIES)
    finally:
        cc.DELTA["heavy"] = saved
    assert next(d for d in cc.HEAVY_STEPS if fits[d]) == saved and not fits[cc.HEAVY_STEPS[0]]
    assert {t: d for t, d in cc.DELTA.items() if t != "heavy"} == {t: d for t, d in bc.DELTA.items() if t != "heavy"}


def test_every_gpu_case_runs_the_integer_windowed_route():
    """No case dropped for not fitting: every table x family the GPU test lists is here, plans as i32 at its R with one
    wave per pair, has a WIN step exactly under cut_win, and ends its DP phase with FILTER under a cutoff."""
    listed = {(t, f, 4) for t in bc.TABLES for f in ("random", "low_complexity", "rearranged")}
    listed |= {(t, f, R) for f in ("edges", "short_m") for t, R in (("user_costs.json", 4), ("tight", 4),
                                                                    ("user_costs.json", 8))}
    listed |= {("user_costs.json", "drift", 4), ("gui_int", "drift", 4), ("user_costs.json", "low_complexity", 16),
               ("user_costs.json", "rearranged", 16), ("user_costs.json", "empty_sides", 4)}
    assert {c[:3] for c in cc.GPU_CASES} == listed and len(cc.GPU_CASES) == len(listed) == 35
    for name, family, R, n in cc.GPU_CASES:
        A, B = cc.pairs(name, family, R, n)
        where = (name, family, R)
        assert cc.distance_fits(name, A, B, R), where
        packed, costs, opts = sedgpu.PackedPairs(A, B), cc.plan_costs(name), cc.stripe_options(R)
        assert sedgpu.plan_routes(costs, opts, packed, O.SED_NO_LEN)["lane_pairs"] == 0, where
        for cut_on, cut_win in ((False, False), (True, False), (True, True)):
            s = sedgpu.plan_schedule(costs, opts, packed, O.SED_NO_LEN, cut_on, cut_win)
            kinds = [st.launcher for st in s]
            assert all(st.phase == "dp" for st in s), where
            assert kinds == (["win"] if cut_win else ["i32"]) + ["filter"] * cut_on, (where, kinds)
            assert s[-1].end and not any(st.end for st in s[:-1]), where
        # SED_OPT_CUT = 2 never windows
        with pytest.raises(sedgpu.SedError) as ex:
            sedgpu.plan_schedule(costs, {**opts, O.SED_OPT_CUT: 2}, packed, O.SED_NO_LEN, True, True)
        assert ex.value.code == sedgpu.SED_E_ARG
    # the shapes the issue names
    A, B = cc.pairs("user_costs.json", "drift", 4)
    assert len(A) == 6 and len(A[0]) == 2600 and {len(b) for b in B} >= {2200, 3000}
    A, B = cc.pairs("user_costs.json", "short_m", 8)
    assert {len(a) for a in A} == {1025} and sorted({len(b) for b in B}) == [33, 34, 63]
    A, B = cc.pairs("user_costs.json", "empty_sides", 4)
    assert [(len(A[p]), len(B[p])) for p in cc.EMPTY_PAIRS.values()] == [(0, 0), (0, 300), (300, 0)]
    assert sum(len(a) > 0 and len(b) > 0 for a, b in zip(A, B)) == 4


def test_kept_cells_restate_the_band_cells():
    """cut_cases.window_cells under the diagonal's own bound is sedgpu.band_cells, pair by pair; under a cutoff no
    tighter than any pair's bound batch_cells is their sum, under a cutoff below a pair's length difference that pair
    counts nothing, and the count is monotone in the cutoff."""
    for name, family, R, n in cc.GPU_CASES[::4] + cc.GPU_CASES[-6:]:
        sub, ins, dele = bc.costs(name)
        A, B = cc.pairs(name, family, R, n)
        total = 0
        for a, b in zip(A, B):
            if len(a) and len(b):
                ub = cc.diag_bound(sub, ins, dele, a, b)
                assert ub <= cc.KEY_MAX
                cells = cc.window_cells(len(a), len(b), R, ins, dele, ub)
                assert cells == sedgpu.band_cells(sub, ins, dele, a, b, R) and 0 < cells <= len(a) * len(b)
                total += cells
        cells, nominal = cc.batch_cells(sub, ins, dele, A, B, R, 1e300)
        assert cells == total and nominal == sum(len(a) * len(b) for a, b in zip(A, B))
        seq = [cc.batch_cells(sub, ins, dele, A, B, R, T)[0] for T in (0, 10, 100.5, 1000, 65535)]
        assert seq == sorted(seq) and seq[-1] == total
    sub, ins, dele = bc.costs("user_costs.json")
    a, b = np.zeros(700, np.uint8), np.zeros(600, np.uint8)
    assert cc.batch_cells(sub, ins, dele, [a], [b], 4, 100 * dele - 1) == (0.0, 420000.0)
    assert cc.batch_cells(sub, ins, dele, [a], [b], 4, 100 * dele)[0] > 0


def test_default_option_batches_start_where_the_gpu_test_says():
    """1536 x 1536 pairs under default options: 40 run SPLIT, which takes no window; 260 run two per wave under `fact`
    and one per wave on the plain stripe kernel under `sum`, whose mismatches cost what delete + insert do and do not
    pack.  Neither CHAINs (pairs of three stripes)."""
    for name in ("sum", "fact"):
        for kind in ("related", "independent"):
            few = cc.route_pairs(kind, cc.ROUTE_FEW)
            many = cc.route_pairs(kind, cc.ROUTE_MANY)
            assert all(np.array_equal(x, y) for x, y in zip(few[0] + few[1], many[0][:40] + many[1][:40]))
            r = sedgpu.plan_routes(cc.plan_costs(name), {}, sedgpu.PackedPairs(*few), O.SED_NO_LEN)
            assert r["mode"] == 1 and r["split_tasks"] > 0 and r["packed_pairs"] == r["chains"] == 0
            with pytest.raises(sedgpu.SedError):
                sedgpu.plan_schedule(cc.plan_costs(name), {}, sedgpu.PackedPairs(*few), O.SED_NO_LEN, True, True)
            packed = sedgpu.PackedPairs(*many)
            r = sedgpu.plan_routes(cc.plan_costs(name), {}, packed, O.SED_NO_LEN)
            assert r["mode"] == 1 and r["split_tasks"] == r["chains"] == r["lane_pairs"] == 0
            assert r["packed_pairs"] == (cc.ROUTE_MANY if name == "fact" else 0), (name, kind)
            assert r["rows_per_lane"] in (4, 8, 16)
            first = {"fact": "x2", "sum": "i32"}[name]
            assert [st.launcher for st in sedgpu.plan_schedule(cc.plan_costs(name), {}, packed, O.SED_NO_LEN, True)] == \
                [first, "filter"]
            assert [st.launcher for st in sedgpu.plan_schedule(cc.plan_costs(name), {}, packed, O.SED_NO_LEN, True, True)] \
                == ["win", "filter"]
            assert r["rows_per_lane"] == 16
    # independent pairs under `sum`: the diagonal's bound prunes nothing at the planner's R, a small cutoff does
    sub, ins, dele = bc.costs("sum")
    A, B = cc.route_pairs("independent", cc.ROUTE_MANY)
    assert cc.batch_cells(sub, ins, dele, A, B, 16, 1e300) == (260.0 * 1536 ** 2, 260.0 * 1536 ** 2)
    assert cc.batch_cells(sub, ins, dele, A, B, 16, 100)[0] < 0.6 * 260 * 1536 ** 2


@pytest.mark.parametrize("name", sorted(cc.F64_ROUTES))
def test_fp64_batches_take_their_routes(name):
    a, b, opts, pos, zero, want_len = cc.f64_route(name)
    plan, packed = cc.f64_plan(name)
    r = sedgpu.plan_routes(cc.costs_of(plan), opts, packed, O.SED_NO_LEN)
    assert r["mode"] != 1 and all(r[k] > 0 for k in pos) and all(r[k] == 0 for k in zero), r
    kinds = [st.launcher for st in sedgpu.plan_schedule(cc.costs_of(plan), opts, packed, O.SED_NO_LEN, True)]
    assert kinds[-1] == "filter" and "win" not in kinds
    assert kinds[:-1] == {"wave": ["f64"], "segments": ["f64_seg"], "split": ["f64"], "lane": ["lane"]}[name]
    with pytest.raises(sedgpu.SedError):
        sedgpu.plan_schedule(cc.costs_of(plan), opts, packed, O.SED_NO_LEN, True, True)
    assert want_len == (name != "lane")  # (the wave kernels report lengths regardless, the lane kernels never)
    if name == "lane":
        assert r["lane_pairs"] == packed.npairs == r["scaled_pairs"] + r["bitpar_pairs"]
        assert any("N" in s for s in a + b)
    if name == "wave":
        assert packed.npairs == 64
    if name == "segments":
        assert r["segment_pairs"] == packed.npairs == 300


def test_pipelined_lane_batch():
    A, B = cc.lane_pairs()
    packed, costs = sedgpu.PackedPairs(A, B), cc.plan_costs("user_costs.json")
    r = sedgpu.plan_routes(costs, {}, packed, O.SED_NO_LEN | O.SED_PIPELINE)
    assert r["mode"] == 1 and r["lane_pairs"] == packed.npairs == 2000
    s = sedgpu.plan_schedule(costs, {}, packed, O.SED_NO_LEN | O.SED_PIPELINE, True)
    assert [st.launcher for st in s] == ["lane", "filter"]
