"""The envelope of bounded search (sed_batch_set_cutoff), shared by the CPU model test
(tests/test_cut_envelope.py) and the GPU test (tests/test_gpu_cut_envelope.py): the cost tables and sequence families of
tests/band_cases.py, two families of its own (empty sides in the cutoff's pair list, wave pairs of m = 33, 34, 63), the
cutoffs a batch is run under, the planner's word that a batch stays on the integer windowed route, and the host's
restatement of the cells a cutoff keeps.  Everything is seeded and device-free."""
import json
import os

import numpy as np

import band_cases as bc
import sedcost
import sedgpu

S = bc.S
O = sedgpu
INF = float("inf")
# one wave per pair on the plain stripe kernel (tests/test_gpu_cutoff.py: STRIPE), as plan_routes takes options
STRIPE = {O.SED_OPT_CHAIN: 2, O.SED_OPT_SPLIT: 2, O.SED_OPT_PACK: 2}
KEY_MAX = 65535  # the integer scale's clamp of a cutoff (sed_batch_set_cutoff: every integer distance is below 2^16)

# The largest m - n a family gives a table.  band_cases.DELTA, with `heavy` trimmed from 300 in steps of 50 until every
# batch of HEAVY_FAMILIES plans as i32 on the distance-only stripe kernel at R = 4 (distance_fits; the CPU test repeats
# the search and asserts that it ends here).
HEAVY_STEPS = (300, 250, 200, 150, 100, 50)
HEAVY_FAMILIES = ("random", "low_complexity", "rearranged")
DELTA = dict(bc.DELTA)
DELTA["heavy"] = 150


def plan_costs(name):
    """A table as sed_set_costs, plan_routes and plan_schedule take it."""
    p = sedcost.build_plan(bc.TABLES[name], [S], [S])
    return (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
            float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))


def stripe_options(R):
    return {**STRIPE, O.SED_OPT_ROWS_PER_LANE: R}


def distance_fits(name, A, B, R):
    """Whether the batch plans as the integer stripe route the cutoff windows: mode i32 at the forced R, one wave per
    pair (no CHAIN, SPLIT or packing), distance only."""
    try:
        r = sedgpu.plan_routes(plan_costs(name), stripe_options(R), sedgpu.PackedPairs(list(A), list(B)), O.SED_NO_LEN)
    except sedgpu.SedError:
        return False
    return (r["mode"] == 1 and r["rows_per_lane"] == R and r["traceback_mode"] == 0 and
            r["chains"] == r["packed_pairs"] == r["split_tasks"] == 0)


# ---- families ----
def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def empty_sides(rng, n, R, delta=300):
    """(0, 0), (0, 300) and (300, 0) among real pairs: a 10 % mutated n x n pair, an independent one, one of
    (n, n - delta) and an identical one, so that the cutoff's pair list holds the empty sides between wave pairs."""
    r = lambda k: rng.integers(0, 4, size=k).astype(np.uint8)  # noqa: E731
    a, z = r(n), np.zeros(0, np.uint8)
    A = [a, z, a, z, a, r(300), a]
    B = [bc.mut(rng, a), z, r(n), r(300), bc.mut(rng, a)[:n - delta], z, a.copy()]
    return A, B


EMPTY_PAIRS = {"none": 1, "insert": 3, "delete": 5}  # empty_sides: the pairs (0, 0), (0, 300), (300, 0)


def short_m(rng, n, R, delta=300):
    """n = 2 ROWS + 1 (n is not read) against m = 33, 34 and 63: the shortest str2 that still runs on a wave, one chunk
    or two under three stripes, the last of one row.  str2 is a 10 % mutated stretch of str1 from its start, its middle
    and its end, and an independent one."""
    nn = 128 * R + 1
    a = rng.integers(0, 4, size=nn).astype(np.uint8)
    A, B = [], []
    for m in (33, 34, 63):
        for at in (0, nn // 2, nn - m):
            A.append(a)
            B.append(bc.mut(rng, a[at:at + m]))
        A.append(a)
        B.append(rng.integers(0, 4, size=m).astype(np.uint8))
    return A, B


FAMILIES = dict(bc.FAMILIES, empty_sides=empty_sides, short_m=short_m)
FAMILY_N = dict(bc.FAMILY_N, empty_sides=600, short_m=0)


def pairs(table, family, R, n=None):
    """(A, B) of one family under one table: band_cases.family_pairs, with this module's DELTA and families."""
    return bc.family_pairs(table, family, R, n, FAMILIES, FAMILY_N, DELTA)


# (table, family, R, n): the batches tests/test_gpu_cut_envelope.py runs on the windowed kernel under stripe_options(R)
GPU_CASES = [(t, f, 4, None) for t in bc.TABLES for f in ("random", "low_complexity", "rearranged")]
GPU_CASES += [(t, f, R, None) for f in ("edges", "short_m") for t, R in (("user_costs.json", 4), ("tight", 4),
                                                                        ("user_costs.json", 8))]
GPU_CASES += [("user_costs.json", "drift", 4, None), ("gui_int", "drift", 4, None)]
GPU_CASES += [("user_costs.json", "low_complexity", 16, 2100), ("user_costs.json", "rearranged", 16, 2100)]
GPU_CASES += [("user_costs.json", "empty_sides", 4, None)]
# (table, family, R, n): what the window property is checked on (the CPU model needs no route)
MODEL_CASES = [(t, f, 4, None) for t in bc.TABLES for f in ("random", "low_complexity", "rearranged", "edges", "drift")]
MODEL_CASES += [("user_costs.json", "edges", 8, None), ("user_costs.json", "low_complexity", 16, 2100)]


# ---- cutoffs ----
def gap_cost(n, m, ins, dele):
    return ins * (m - n) if m > n else dele * (n - m)


def cutoffs(ref_dists, ins, dele, lens):
    """The cutoffs a batch runs under, from its oracle distances and its (n, m): both sides and the exact "<=" edge of
    the smallest, the median and the largest finite distance (with halves: a fractional cutoff counts as its floor), 0,
    the clamp of the integer scale (65535, 65536.5, 1e300), and for the first pair of unequal non-empty lengths the cost
    of its length difference and one below it, which leaves that pair no path at all.  Sorted, without repeats."""
    d = np.sort(np.asarray(ref_dists, np.float64)[np.isfinite(ref_dists)])
    T = {0.0, float(KEY_MAX), KEY_MAX + 1.5, 1e300}
    for D in (d[0], d[len(d) // 2], d[-1]):
        T |= {float(D) + x for x in (-1, -0.5, 0, 0.5, 1)}
    for n, m in lens:
        if n != m and n > 0 and m > 0:
            gap = float(gap_cost(n, m, ins, dele))
            T |= {gap, gap - 1}
            break
    return sorted(t for t in T if t >= 0)


def cut_key(T):
    """A cutoff on the integer scale."""
    return int(np.floor(min(T, float(KEY_MAX))))


# ---- the host's restatement of a cutoff's windows (sed_batch_set_cutoff, sed_band_pair_cells) ----
def diag_bound(sub, ins, dele, a, b):
    k = min(len(a), len(b))
    return float(sub[a[:k], b[:k]].sum()) + gap_cost(len(a), len(b), ins, dele)


def window_cells(n, m, R, ins, dele, ub):
    """Cells of an n x m pair inside its stripes' chunk ranges under the window of ub: per stripe its rows times the
    columns 64 clo + 1 .. 64 chi (up to m where the range holds the last chunk or passes m)."""
    elo, ehi = sedgpu.band_bounds(n, m, ins, dele, ub)
    rows, cells = 64 * R, 0
    for k in range((n + rows - 1) // rows):
        clo, chi, nchunks = sedgpu.band_chunk_range(n, m, R, elo, ehi, k)
        jend = m if (chi >= nchunks - 1 or 64 * chi > m) else 64 * chi
        cells += min(rows, n - k * rows) * (jend - 64 * clo)
    return cells


def batch_cells(sub, ins, dele, A, B, R, T):
    """(cells the windowed kernel runs under cutoff T, n m summed) over a batch of wave pairs: a pair with an empty
    side or whose length difference alone costs more than T runs no stripe."""
    key, cells, nominal = cut_key(T), 0, 0
    for a, b in zip(A, B):
        n, m = len(a), len(b)
        if n == 0 or m == 0:
            continue
        nominal += n * m
        if gap_cost(n, m, ins, dele) <= key:
            cells += window_cells(n, m, R, ins, dele, min(key, diag_bound(sub, ins, dele, a, b)))
    return float(cells), float(nominal)


# ---- the default-option route: pairs of 1536 x 1536 ----
# Under default options a batch of at most 256 pairs longer than 256 runs SPLIT (sed_plan.cpp: i32_split), which takes no
# window, and CHAIN takes one-stripe pairs only: 1536 x 1536 pairs reach a route a cutoff can leave from 257 pairs on.
# ROUTE_FEW is the batch that stays SPLIT, ROUTE_MANY the same 40 pairs followed by 220 more.
ROUTE_N, ROUTE_FEW, ROUTE_MANY = 1536, 40, 260


def route_pairs(kind, count):
    """"related": low_complexity's nine pairs of equal lengths, then copies mutated at 1 .. 10 % (the rate cycles every
    31 pairs); "independent": uniform random pairs.  The first pairs of a longer batch are the shorter batch."""
    rng = np.random.default_rng(bc.seed("route", kind))
    r = lambda: rng.integers(0, 4, size=ROUTE_N).astype(np.uint8)  # noqa: E731
    if kind == "independent":
        A = [(r(), r()) for _ in range(count)]
        return [a for a, _ in A], [b for _, b in A]
    A, B = bc.low_complexity(rng, ROUTE_N, 16)
    A, B = [_u8(a) for a, b in zip(A, B) if len(b) == ROUTE_N], [_u8(b) for b in B if len(b) == ROUTE_N]
    assert len(A) == 9
    for i in range(count - len(A)):
        a = r()
        A.append(a)
        B.append(bc.mut(rng, a, 0.01 + 0.09 * (i % 31) / 30))
    return A, B


# ---- the filter-only fp64 routes: costs.json with IUPAC symbols ----
IUPAC = "AGCUYRWSKMDVHBN"


def _iupac(rng, count, lo, hi):
    lut = np.array(list(IUPAC))
    seq = lambda: "".join(lut[rng.integers(0, len(IUPAC), size=int(rng.integers(lo, hi + 1)))])  # noqa: E731
    return [seq() for _ in range(count)], [seq() for _ in range(count)]


def _with_n(rng, count):
    """~28-nt ACGU strings with N at 1 % (config 5's lengths): most pairs lie inside the unit-cost subset ACGU."""
    lut = np.array(list("ACGUN"))
    seq = lambda: "".join(lut[rng.choice(5, p=[0.2475] * 4 + [0.01], size=int(rng.integers(24, 33)))])  # noqa: E731
    return [seq() for _ in range(count)], [seq() for _ in range(count)]


# name: (strings, options, the getters that must be > 0, those that must be 0, whether the route reports lengths).  The
# fp64 wave kernels (whole waves, 16-lane segments, SPLIT) carry the op count in their keys and report it whatever
# SED_NO_LEN says (sed_f64.hip; tests/test_gpu_cutoff.py::test_filter_only_fp64); the lane kernels report -1 (sed_lane.hip).
F64_ROUTES = {
    "wave": (lambda rng: _iupac(rng, 64, 100, 300), {O.SED_OPT_SEG: 2, O.SED_OPT_SPLIT: 2},
             (), ("lane_pairs", "segment_pairs", "split_tasks"), True),
    "segments": (lambda rng: _iupac(rng, 300, 100, 300), {}, ("segment_pairs",), ("lane_pairs", "split_tasks"), True),
    "split": (lambda rng: _iupac(rng, 6, 300, 600), {O.SED_OPT_SPLIT: 1}, ("split_tasks",), ("lane_pairs",), True),
    "lane": (lambda rng: _with_n(rng, 2000), {}, ("lane_pairs", "scaled_pairs", "bitpar_pairs"),
             ("segment_pairs", "split_tasks"), False),
}


def f64_route(name):
    """(strings a, strings b, options, getters > 0, getters == 0, reports lengths) of one fp64 route."""
    make, opts, pos, zero, want_len = F64_ROUTES[name]
    a, b = make(np.random.default_rng(bc.seed("f64", name)))
    return a, b, dict(opts), pos, zero, want_len


def f64_plan(name):
    """(cost plan, packed pairs) of an fp64 route's batch under costs.json."""
    a, b = f64_route(name)[:2]
    with open(os.path.join(bc.GOLDEN, "costs.json")) as f:
        plan = sedcost.build_plan(json.load(f), a, b)
    return plan, sedgpu.PackedPairs([plan.encode(s) for s in a], [plan.encode(s) for s in b])


def costs_of(plan):
    return (plan.K, np.ascontiguousarray(plan.sub, np.float64).ravel(), np.ascontiguousarray(plan.sub_int, np.uint8).ravel(),
            float(plan.ins), int(plan.ins_int), float(plan.dele), int(plan.del_int))


# ---- the pipelined batch: 2000 lane pairs ----
def lane_pairs(count=2000):
    rng = np.random.default_rng(bc.seed("pipelined", count))
    A = [rng.integers(0, 4, size=int(rng.integers(20, 37))).astype(np.uint8) for _ in range(count)]
    B = [bc.mut(rng, np.resize(a, int(rng.integers(20, 33))), 0.2) for a in A]
    return A, B
