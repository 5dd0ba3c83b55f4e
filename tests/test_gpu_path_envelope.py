"""GPU: every route to an edit script on paths built to cross its seams (tests/path_cases.py): insert runs of three
chunks inside one tile, delete runs through band, tile and stripe borders in one column, turns on and beside tile and
stripe corners, scripts that end in hundreds of border ops, staircases of period 63, 64 and 65, homopolymers whose
path the tie order alone decides, and pairs one symbol thin.  tests/test_path_cases.py proves without a device that the
oracle's canonical path does what each pair claims, and that each batch here is planned onto the route it names.

Every test first asserts its route from the batch's own attributes (mode, traceback_mode, rows_per_lane, chains,
split_tasks, segment_pairs, lane_pairs), then compares every pair with the C oracle through test_gpu_parity's
_oracle_check: distance bits, typing, length and the script op by op.  A wrong script or a nonzero err fails here; it
faults nothing.  Pair counts and largest shapes are printed per case and listed in profiles/path_envelope/README.md."""
import pytest

import path_cases as pc
import sedcost
import sedgpu
from test_gpu_parity import OPCH, _oracle_check

pytestmark = pytest.mark.gpu
INT = list(pc.INT_TABLES)
F64 = list(pc.F64_TABLES)
OPTS = {"R": sedgpu.SED_OPT_ROWS_PER_LANE, "split": sedgpu.SED_OPT_SPLIT, "lane": sedgpu.SED_OPT_LANE,
        "chain": sedgpu.SED_OPT_CHAIN, "tb": sedgpu.SED_OPT_TB, "seg": sedgpu.SED_OPT_SEG, "band": sedgpu.SED_OPT_BAND,
        "pack": sedgpu.SED_OPT_PACK}


def _run(gpu, table, pairs, route, times=1, mode=0, script=True, no_len=False, **opts):
    """One Batch of the pairs under the options: asserts `route` (attribute: value or predicate) before it runs, runs it
    `times` times reading the results after each run (results() raises when any pair reports err), and returns the runs
    as gpu_run does, [(dist, is_int, len, script)] each, and the batch's band_chunks_run()."""
    plan = sedcost.build_plan(table, [a for a, _ in pairs], [b for _, b in pairs])
    gpu.set_mode(mode)
    for k, v in opts.items():
        gpu.set_option(OPTS[k], v)
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs([plan.encode(a) for a, _ in pairs], [plan.encode(b) for _, b in pairs])
    try:
        b = sedgpu.Batch(gpu, packed, script, no_len=no_len)
        try:
            got = {k: getattr(b, k) for k in route}
            miss = {k: got[k] for k, v in route.items() if not (v(got[k]) if callable(v) else got[k] == v)}
            assert not miss, (miss, got)
            outs = []
            for _ in range(times):
                b.run()
                d, ii, ln, ops = b.results()
                outs.append([(float(d[p]), bool(ii[p]), int(ln[p]),
                              "".join(OPCH[c] for c in sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p])))
                              if script else None) for p in range(len(pairs))])
            return outs, b.band_chunks_run()
        finally:
            b.close()
    finally:
        gpu.set_mode(0)
        for k in opts:
            gpu.set_option(OPTS[k], 0)


def _shape(what, pairs, nfam):
    print("%s: %d pairs (%d built), n <= %d, m <= %d" % (what, len(pairs), nfam, max(len(a) for a, _ in pairs),
                                                         max(len(b) for _, b in pairs)))


def _positive(v):
    return v > 0


@pytest.mark.parametrize("R", [4, 8, 16])
@pytest.mark.parametrize("name", INT)
def test_codes_and_checkpoints(gpu, name, R):
    """Every family at R: 38 built pairs (costs.json, user_costs.json), 41 (gui_int) or 51 (sum), the largest
    585 x 779 at R = 4, 1097 x 1291 at R = 8 and 2121 x 2315 at R = 16, filled to 260 pairs so that the per-cell codes run sed_traceback_kernel (one lane per pair; 256 pairs and fewer run the window kernel).  Per-cell
    codes (tb = 1); then checkpoints on the stripe kernel (tb = 2, CHAIN off) with band pruning off, two runs of one
    Batch (the second reads topb and selb after a first use), and one run each with the refined and the static windows:
    all equal to the codes' scripts and to the oracle's, no err."""
    table = pc.INT_TABLES[name]
    built = pc.pairs_of(pc.batch(name, R))
    pairs = built + pc.pad_pairs(260 - len(built), "codes %s %d" % (name, R))
    _shape("%s R=%d" % (name, R), pairs, len(built))
    base = {"mode": "i32", "rows_per_lane": R, "split_tasks": 0, "lane_pairs": 0}
    (codes,), _ = _run(gpu, table, pairs, {**base, "traceback_mode": 1}, tb=1, split=2, lane=2, R=R)
    _oracle_check(table, pairs, codes)
    ck = {**base, "traceback_mode": 2, "chains": 0}
    (run1, run2), chunks = _run(gpu, table, pairs, ck, times=2, tb=2, split=2, lane=2, chain=2, R=R, band=2)
    assert chunks is None
    assert run1 == codes and run2 == codes
    for band in (0, 3):
        (pruned,), chunks = _run(gpu, table, pairs, ck, tb=2, split=2, lane=2, chain=2, R=R, band=band)
        assert chunks is not None and chunks[0] <= chunks[1], (band, chunks)
        assert pruned == codes, band


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", INT)
def test_checkpoints_on_chain(gpu, name, R):
    """The one-stripe members of every family (path_cases.chain_batch) through CHAIN with checkpoints, two runs of one
    Batch, and with per-cell codes.  R = 4: 30 pairs (45 under sum), n <= 256, m <= 395; R = 8: 34 pairs (37 gui_int,
    52 sum), n <= 512, m <= 552."""
    table = pc.INT_TABLES[name]
    pairs = pc.pairs_of(pc.chain_batch(name, R))
    _shape("chain %s R=%d" % (name, R), pairs, len(pairs))
    base = {"mode": "i32", "rows_per_lane": R, "split_tasks": 0, "lane_pairs": 0, "chains": _positive}
    (run1, run2), _ = _run(gpu, table, pairs, {**base, "traceback_mode": 2}, times=2, tb=2, chain=1, lane=2, split=2, R=R)
    _oracle_check(table, pairs, run1)
    assert run2 == run1
    (codes,), _ = _run(gpu, table, pairs, {**base, "traceback_mode": 1}, tb=1, chain=1, lane=2, split=2, R=R)
    assert codes == run1


@pytest.mark.parametrize("name", ["costs.json", "user_costs.json"])
def test_two_pairs_per_wave(gpu, name):
    """sed_wf_i32x2_kernel is distance only and needs every mismatch below insert + delete, so it runs the two shipped
    tables: every family at R = 4, each pair twice (a partner of equal n and m; 76 pairs, the largest 585 x 779),
    distances against the oracle and against the run with packing off."""
    table = pc.INT_TABLES[name]
    pairs = [p for p in pc.pairs_of(pc.batch(name, 4)) for _ in (0, 1)]
    _shape("x2 %s" % name, pairs, len(pairs))
    route = {"mode": "i32", "rows_per_lane": 4, "split_tasks": 0, "traceback_mode": 0}
    (got,), _ = _run(gpu, table, pairs, {**route, "packed_pairs": lambda v: v >= len(pairs) // 2}, script=False,
                     no_len=True, R=4, split=2, lane=2)
    _oracle_check(table, pairs, got, no_len=True)
    (plain,), _ = _run(gpu, table, pairs, {**route, "packed_pairs": 0}, script=False, no_len=True, R=4, split=2, lane=2,
                       pack=2)
    assert [g[:2] for g in got] == [g[:2] for g in plain]


@pytest.mark.parametrize("name", INT)
def test_window_traceback(gpu, name):
    """One member of each family (5; 6 under gui_int, 7 under sum; the largest 577 x 524) and short random pairs, 70 pairs on the
    automatic route: past the 64 of the
    stripe-parallel walk and within the window kernel's 256 (tests/test_path_cases.py: the schedule's tb_codes step)."""
    table = pc.INT_TABLES[name]
    pairs = pc.window_batch(name)
    _shape("window %s" % name, pairs, sum(bool(pc.members(fam, name, 4)) for fam in pc.FAMILIES))
    (got,), _ = _run(gpu, table, pairs, {"mode": "i32", "traceback_mode": lambda v: v in (1, 4), "chains": 0})
    _oracle_check(table, pairs, got)


@pytest.mark.parametrize("name", INT)
def test_integer_split_band_maps(gpu, name):
    """Integer SPLIT forced at R = 4: long_delete at columns 64 and 65, the staircases and the corners, every pair of
    three stripes (17 pairs, 20 under sum and gui_int; 714 x 713 the largest; delete runs of 579 rows across both stripe
    borders), so each goes through sed_tb_bandmap, bandcompose and bandemit (traceback mode 4: code tiles recomputed
    from checkpoints, then the stripe-parallel walk); two runs of one Batch."""
    table = pc.INT_TABLES[name]
    pairs = pc.pairs_of(pc.split_batch(name))
    _shape("split %s" % name, pairs, len(pairs))
    route = {"mode": "i32", "rows_per_lane": 4, "split_tasks": _positive, "traceback_mode": 4, "lane_pairs": 0, "chains": 0}
    (run1, run2), _ = _run(gpu, table, pairs, route, times=2, split=1, R=4)
    _oracle_check(table, pairs, run1)
    assert run2 == run1


@pytest.mark.parametrize("mode, count", [(2, 260), (3, 100)])
@pytest.mark.parametrize("name", F64)
def test_fp64_one_wave(gpu, name, mode, count):
    """fp64, one wave per pair (SPLIT and segments off) over IUPAC symbols.  These batches get R = 4 from the cost model
    (asserted), so the families built for stripes of 256 rows cross its seams; those built for 512 rows ride along as
    longer paths.  76 built pairs (82 under frac_indel), the largest 1097 x 1291, filled to 260 pairs (mode 2: one lane
    per pair walks the codes) and to 100 (mode 3, typed: the window kernel of 65..256 pairs)."""
    table = pc.F64_TABLES[name]
    built = pc.pairs_of(pc.batch(name, 4, f64=True) + pc.batch(name, 8, f64=True))
    pairs = built + pc.pad_pairs(count - len(built), "f64 %s" % name, pc.IUPAC)
    _shape("fp64 %s mode %d" % (name, mode), pairs, len(built))
    route = {"mode": lambda v: v in ("f64", "f64-typed"), "rows_per_lane": 4, "split_tasks": 0,
             "segment_pairs": 0, "lane_pairs": 0, "traceback_mode": 1}
    (got,), _ = _run(gpu, table, pairs, route, mode=mode, split=2, seg=2)
    _oracle_check(table, pairs, got)


@pytest.mark.parametrize("name", F64)
def test_fp64_segments(gpu, name):
    """fp64 in 16-lane segments (SED_OPT_SEG = 1, 300 pairs, R = 4 from the cost model, asserted): every family at
    SW = 16 built for stripes of 64 rows, and for 128 rows as longer paths; chunks of 16 columns, insert runs of 53.
    76 built pairs (82 under frac_indel), n <= 406, m <= 379 (390 under frac_indel)."""
    table = pc.F64_TABLES[name]
    built = pc.pairs_of(pc.batch(name, 4, SW=16, f64=True) + pc.batch(name, 8, SW=16, f64=True))
    pairs = built + pc.pad_pairs(300 - len(built), "seg %s" % name, pc.IUPAC)
    _shape("segments %s" % name, pairs, len(built))
    route = {"mode": lambda v: v in ("f64", "f64-typed"), "rows_per_lane": 4, "split_tasks": 0,
             "segment_pairs": len(pairs), "lane_pairs": 0, "traceback_mode": 1}
    (got,), _ = _run(gpu, table, pairs, route, seg=1)
    _oracle_check(table, pairs, got)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("name", F64)
def test_fp64_split_stripes(gpu, name, R):
    """fp64 SPLIT forced (stripes of 64 R rows; 41 pairs, 44 under frac_indel; the largest 454 x 523 at R = 2 and
    585 x 779 at R = 4): every family, long_delete at column 257 (past the ring of
    256) and in the last column of m = 255, 256, 257, through the stripe-parallel walk (tb_stripes), two runs of one
    Batch (the hand-off words' epochs)."""
    table = pc.F64_TABLES[name]
    pairs = pc.pairs_of(pc.f64_split_batch(name, R))
    assert len(pairs) <= 64
    _shape("fp64 split %s R=%d" % (name, R), pairs, len(pairs))
    route = {"mode": lambda v: v in ("f64", "f64-typed"), "rows_per_lane": R, "split_tasks": _positive,
             "segment_pairs": 0, "lane_pairs": 0, "traceback_mode": 3}
    (run1, run2), _ = _run(gpu, table, pairs, route, times=2, split=1, R=0 if R == 2 else R)
    _oracle_check(table, pairs, run1)
    assert run2 == run1


@pytest.mark.parametrize("name", INT)
def test_lane_scripts(gpu, name):
    """The thin and ell members of m <= 32 (built at a stripe of 64 rows: 4 pairs, 7 under sum, n <= 83, m <= 30) with
    short random lane pairs, 40 pairs on the automatic route: every pair on sed_lane.hip's script kernels."""
    table = pc.INT_TABLES[name]
    built = pc.pairs_of(pc.lane_batch(name))
    pairs = built + pc.pad_pairs(40 - len(built), "lane " + name, lo=1, hi=33)
    _shape("lane %s" % name, pairs, len(built))
    (got,), _ = _run(gpu, table, pairs, {"mode": "i32", "lane_pairs": len(pairs), "split_tasks": 0})
    _oracle_check(table, pairs, got)
