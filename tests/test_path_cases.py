"""CPU: the path families of tests/path_cases.py, without a device.

a. Claims.  For every family, table and layout tests/test_gpu_path_envelope.py uses, the C oracle's canonical script does
   literally what the pair claims: each run's length and the cells where it starts and ends, the cells passed and
   avoided, the whole script of the homopolymers.  A combination whose claim does not hold is in path_cases.DROPPED by
   name, at most one in eight.
b. The oracle against oracle/pyref.py on the small members (n m <= 40 000): the two restatements of the reference
   agree where the tie order decides everything.
c. The entry arithmetic of ck_traceback_pair (csrc/sed_cktb.hip) restated for every cell of every canonical path of the
   checkpoint batches: both sides of the window choice and its equality, chunk 0, and the first and last tile row occur
   at every R.  This treats every path cell as a possible entry of a tile visit; it does not model where the walk
   leaves a tile, so the kernel enters at a subset of these cells.
d. Routes.  Every batch of the GPU file goes through the planner (sedgpu.plan_routes, plan_schedule) and lands on the
   route it is meant for."""
import functools

import numpy as np
import pytest

import oracle
import path_cases as pc
import pyref
import sedcost
import sedgpu

INT = list(pc.INT_TABLES)
F64 = list(pc.F64_TABLES)
# (R, SW, f64) of every layout the GPU file builds families for
INT_LAYOUTS = [(4, 64), (8, 64), (16, 64), (4, 16), (1, 64)]
F64_LAYOUTS = [(2, 64), (4, 64), (8, 64), (4, 16), (8, 16)]


@functools.lru_cache(maxsize=None)
def scripts(name, R, SW, f64):
    """((a, b, claim, the oracle's script), ...) of every family under a table and layout, computed once."""
    items = pc.batch(name, R, SW, f64)
    table = (pc.F64_TABLES if f64 else pc.INT_TABLES)[name]
    plan = sedcost.build_plan(table, [a for a, _, _ in items], [b for _, b, _ in items])
    cs = oracle.Costs.from_plan(plan)
    return tuple((a, b, c, oracle.ops_to_str(oracle.pair(cs, plan.encode(a), plan.encode(b))["ops"])) for a, b, c in items)


# ---- a. claims ----
@pytest.mark.parametrize("name, f64", [(t, False) for t in INT] + [(t, True) for t in F64])
def test_every_claim_holds_on_the_oracles_script(name, f64):
    seen = set()
    for R, SW in (F64_LAYOUTS if f64 else INT_LAYOUTS):
        for a, b, claim, script in scripts(name, R, SW, f64):
            assert script.count("i") + script.count("u") == len(b) and script.count("d") + script.count("u") == len(a)
            assert not pc.claim_errors(script, claim), (name, R, SW, claim["family"], claim["what"],
                                                        pc.claim_errors(script, claim))
            assert claim["runs"] or claim["script"] is not None
            seen.add(claim["family"])
    want = {fam for fam, t, f in pc.combinations() if t == name and f == f64 and (fam, t) not in pc.DROPPED}
    assert seen == want


def _oracle_scripts(table, items):
    plan = sedcost.build_plan(table, [a for a, _, _ in items], [b for _, b, _ in items])
    cs = oracle.Costs.from_plan(plan)
    return [oracle.ops_to_str(oracle.pair(cs, plan.encode(a), plan.encode(b))["ops"]) for a, b, _ in items]


@pytest.mark.parametrize("name", INT)
def test_integer_split_members_hold_and_have_three_stripes(name):
    """The band map and compose kernels return for pairs of fewer than three stripes (sed_tb.hip: K < 3), so every
    member of the integer SPLIT batch has three at its R = 4; the delete runs at columns 64 and 65 cross both stripe
    borders and the stairs the second."""
    items = pc.split_batch(name)
    assert {c["family"] for _, _, c in items} == {"long_delete", "corner"} | ({"staircase"} - {
        f for f, t in pc.DROPPED if t == name})
    for (a, b, claim), script in zip(items, _oracle_scripts(pc.INT_TABLES[name], items)):
        assert -(-len(a) // 256) >= 3, (claim["what"], len(a))
        assert not pc.claim_errors(script, claim), (name, claim["family"], claim["what"])
    for _, _, c in items:
        if c["family"] == "long_delete":
            (r,) = c["runs"]
            assert r["start"][1] in (64, 65) and r["start"][0] < 256 and r["end"][0] > 512 and r["run"] == 579
        if c["family"] == "staircase":
            assert c["runs"][0]["start"][0] < 512 < c["runs"][-1]["end"][0]


@pytest.mark.parametrize("name", F64)
def test_fp64_ring_members_hold(name):
    """long_delete in the last column of m = 255, 256, 257 (path_cases.f64_split_batch) at R = 2 and 4."""
    for R in (2, 4):
        items = [x for x in pc.f64_split_batch(name, R) if x[2]["what"].startswith("the last column, 25")]
        assert [len(b) for _, b, _ in items] == [255, 256, 257]
        for (a, b, claim), script in zip(items, _oracle_scripts(pc.F64_TABLES[name], items)):
            assert not pc.claim_errors(script, claim), (name, R, claim["what"])


def test_claims_are_literal():
    """claim_errors refuses a script that is off by one op anywhere a claim looks."""
    a, b, claim, script = next(x for x in scripts("sum", 4, 64, False) if x[2]["family"] == "long_insert")
    k = script.index("i")
    assert pc.claim_errors(script[:k] + "u" + script[k + 1:], claim)           # a run one short
    assert pc.claim_errors(script[:k] + "i" + script[k:], claim)               # one long
    assert pc.claim_errors(script[:k - 1] + "iu" + script[k + 1:], claim)      # moved by one cell
    a, b, claim, script = next(x for x in scripts("sum", 4, 64, False) if x[2]["avoid"])
    assert pc.claim_errors(script, dict(claim, avoid=claim["through"]))


def test_dropped_combinations_are_few_and_named():
    combos = pc.combinations()
    assert all((fam, t) in {(f, n) for f, n, _ in combos} for fam, t in pc.DROPPED)
    dropped = [c for c in combos if (c[0], c[1]) in pc.DROPPED]
    assert 8 * len(dropped) <= len(combos), (len(dropped), len(combos))
    for fam in ("corner", "long_insert", "border_finish"):  # under dot keys and under distance keys
        live = {t for f, t, f64 in combos if f == fam and not f64 and (f, t) not in pc.DROPPED}
        assert live & set(pc.FACTORS) and live - set(pc.FACTORS)
    for t in pc.INT_TABLES:
        assert pc.INT_TABLES[t] is __import__("band_cases").TABLES[t]


def test_families_reach_their_seams():
    """The geometry the families promise, read off the claims at R = 8: rows on both sides of a stripe and a tile border,
    columns 1, 63, 64, 65 and 257, runs of 3 chunks + 5 and of a stripe + a tile + 3, six turns per staircase."""
    items = {fam: pc.members(fam, "sum", 8) for fam in pc.FAMILIES}
    rows = {c["runs"][0]["start"][0] for _, _, c in items["long_insert"]}
    assert rows >= {512, 513, 1024, 576, 577} and all(c["runs"][0]["run"] == 197 for _, _, c in items["long_insert"])
    cols = {c["runs"][0]["start"][1] for _, _, c in items["long_delete"]}
    assert cols == {1, 63, 64, 65, 100, 257} and all(c["runs"][0]["run"] == 579 for _, _, c in items["long_delete"])
    assert all(len(c["runs"]) == 3 and {r["run"] for r in c["runs"]} <= {63, 64, 65} for _, _, c in items["staircase"])
    thr = {tuple(c["through"][0]) for _, _, c in items["corner"]}
    assert {(576, 640), (512, 448), (1024, 1024)} <= thr and sum(i % 64 == 0 and j % 64 == 0 for i, j in thr) == 3
    assert {len(b) for _, b, _ in items["thin"]} >= {1, 2, 7, 8} and {len(a) for a, _, _ in items["thin"]} >= {1, 8, 9}
    assert {(len(a) > len(b)) - (len(a) < len(b)) for a, b, _ in items["ell"]} == {-1, 0, 1}
    assert max(c["runs"][0]["run"] for _, _, c in items["border_finish"]) == 1029


# ---- b. the oracle against pyref ----
@pytest.mark.parametrize("name, f64", [(t, False) for t in INT] + [(t, True) for t in F64])
def test_oracle_agrees_with_pyref_on_the_small_members(name, f64):
    """Every member of n m <= 40 000 built at stripes of 64 rows and chunks of 16 columns (R = 4, SW = 16: the smallest
    layout, whose members are the families' small ones), under every table: oracle/pyref.py rebuilds the reference's
    node graph and walks create_paths(dp)[0].  About 35 pairs and 4 s per table, pyref being pure Python."""
    table = (pc.F64_TABLES if f64 else pc.INT_TABLES)[name]
    small = [x for x in scripts(name, 4, 16, f64) if len(x[0]) * len(x[1]) <= 40000]
    for a, b, claim, script in small:
        assert pyref.run_pair(a, b, table)[1] == script, (name, claim["family"], claim["what"])
    fams = {x[2]["family"] for x in scripts(name, 4, 16, f64)} - {"staircase"}  # (315 x 378 and more: not small)
    assert {x[2]["family"] for x in small} == fams and len(small) >= 25, (len(small), fams)


# ---- c. the checkpoint traceback's entry arithmetic ----
def entry_classes(script, R):
    """The classes of tile entries among the cells of one path (sed_cktb.hip: ck_traceback_pair, band pruning off so
    clo = 0): k, t, Q, ce, re as there, x = (j - 1 + t) & 63 the entry step inside its chunk; a window of two chunks
    when ce > clo and x < re."""
    ROWS, G, out = 64 * R, 64 // R, set()
    for i, j in pc.path_cells(script):
        if i < 1 or j < 1:
            continue
        k, t = (i - 1) // ROWS, ((i - 1) % ROWS) // R
        Q = t // G
        ce, x = (j - 1 + t) >> 6, (j - 1 + t) & 63
        re = i - (k * ROWS + 64 * Q) - 1
        assert 0 <= re <= 63
        out.add("x < re" if x < re else "x == re" if x == re else "x > re")
        out.add("two chunks" if ce > 0 and x < re else "one chunk")
        if ce == 0:
            out.add("ce == 0")
            if x < re:
                out.add("ce == 0 and x < re")  # (the window choice's `ce > clo` alone keeps one chunk)
        if re in (0, 63):
            out.add("re == %d" % re)
    return out


@pytest.mark.parametrize("R", [4, 8, 16])
@pytest.mark.parametrize("name", INT)
def test_checkpoint_batches_hold_every_entry_class(name, R):
    have = set()
    for a, b, claim, script in scripts(name, R, 64, False):
        have |= entry_classes(script, R)
    assert have >= {"x < re", "x == re", "x > re", "two chunks", "one chunk", "ce == 0", "ce == 0 and x < re",
                    "re == 0", "re == 63"}, (name, R, have)


# ---- d. routes ----
O = {"mode": sedgpu.SED_OPT_MODE, "R": sedgpu.SED_OPT_ROWS_PER_LANE, "split": sedgpu.SED_OPT_SPLIT,
     "lane": sedgpu.SED_OPT_LANE, "chain": sedgpu.SED_OPT_CHAIN, "tb": sedgpu.SED_OPT_TB, "seg": sedgpu.SED_OPT_SEG,
     "band": sedgpu.SED_OPT_BAND, "pack": sedgpu.SED_OPT_PACK}
I32, SCRIPT, NO_LEN = 1, 1, 4


def planned(table, pairs, flags=SCRIPT, schedule=False, **opts):
    p = sedcost.build_plan(table, [a for a, _ in pairs], [b for _, b in pairs])
    costs = (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
             float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))
    packed = sedgpu.PackedPairs([p.encode(a) for a, _ in pairs], [p.encode(b) for _, b in pairs])
    options = {O[k]: v for k, v in opts.items()}
    got = sedgpu.plan_routes(costs, options, packed, flags)
    if schedule:
        got["steps"] = [s.launcher for s in sedgpu.plan_schedule(costs, options, packed, flags)]
    return got


def has(got, **want):
    miss = {k: got[k] for k, v in want.items() if not (v(got[k]) if callable(v) else got[k] == v)}
    assert not miss, (miss, got)


@pytest.mark.parametrize("name", INT)
def test_integer_batches_take_their_routes(name):
    table = pc.INT_TABLES[name]
    for R in (4, 8, 16):
        built = pc.pairs_of(pc.batch(name, R))
        assert 30 <= len(built) <= 64
        pairs = built + pc.pad_pairs(260 - len(built), "codes %s %d" % (name, R))
        got = planned(table, pairs, schedule=True, tb=1, split=2, lane=2, R=R)
        has(got, mode=I32, rows_per_lane=R, traceback_mode=1, split_tasks=0, lane_pairs=0)
        assert "tb_codes" in got["steps"] and len(pairs) > 256  # (past 256 pairs: sed_traceback_kernel)
        for band in (2, 0, 3):
            got = planned(table, pairs, schedule=True, tb=2, split=2, lane=2, chain=2, R=R, band=band)
            has(got, mode=I32, rows_per_lane=R, traceback_mode=2, chains=0, split_tasks=0, lane_pairs=0,
                dot_keys=lambda v: (v & 1) == (name in pc.FACTORS))
            assert "tb_ck" in got["steps"]
            assert (got["band_cells"] < got["cells"]) == (band != 2)
    for R in (4, 8):
        pairs = pc.pairs_of(pc.chain_batch(name, R))
        assert len(pairs) >= 12 and {c["family"] for _, _, c in pc.chain_batch(name, R)} == {
            fam for fam, t, f64 in pc.combinations() if t == name and not f64 and (fam, t) not in pc.DROPPED
            and (fam != "staircase" or R == 8)}  # (a staircase has 5 p = 315 rows and more: past one stripe at R = 4)
        for tb in (2, 1):
            got = planned(table, pairs, schedule=True, tb=tb, chain=1, lane=2, split=2, R=R)
            has(got, mode=I32, rows_per_lane=R, traceback_mode=tb, chains=lambda v: v > 0, split_tasks=0, lane_pairs=0)
            assert "chain" in got["steps"]
    pairs = pc.window_batch(name)
    got = planned(table, pairs, schedule=True)
    assert len(pairs) == 70 and "tb_codes" in got["steps"] and "tb_stripes" not in got["steps"]
    has(got, mode=I32, traceback_mode=lambda v: v in (1, 4), chains=0)
    pairs = pc.pairs_of(pc.split_batch(name))
    got = planned(table, pairs, schedule=True, split=1, R=4)
    has(got, mode=I32, rows_per_lane=4, traceback_mode=4, split_tasks=lambda v: v > 0, lane_pairs=0, chains=0)
    assert "tb_stripes" in got["steps"] and "codes" in got["steps"]
    built = pc.pairs_of(pc.lane_batch(name))
    pairs = built + pc.pad_pairs(40 - len(built), "lane " + name, lo=1, hi=33)
    assert len(built) >= 4
    got = planned(table, pairs, schedule=True)
    has(got, mode=I32, lane_pairs=40, split_tasks=0)
    assert got["steps"].count("lane") >= 1 and "tb_codes" not in got["steps"]


@pytest.mark.parametrize("name", ["costs.json", "user_costs.json"])
def test_two_pairs_per_wave_is_planned(name):
    pairs = [p for p in pc.pairs_of(pc.batch(name, 4)) for _ in (0, 1)]
    got = planned(pc.INT_TABLES[name], pairs, flags=NO_LEN, schedule=True, R=4, split=2, lane=2)
    has(got, mode=I32, rows_per_lane=4, split_tasks=0, packed_pairs=lambda v: v >= len(pairs) // 2)
    assert "x2" in got["steps"]
    for other in ("sum", "gui_int"):  # a mismatch of insert + delete: the 16-bit halves cannot hold it
        both = [p for p in pc.pairs_of(pc.batch(other, 4)) for _ in (0, 1)]
        assert planned(pc.INT_TABLES[other], both, flags=NO_LEN, R=4, split=2, lane=2)["packed_pairs"] == 0


@pytest.mark.parametrize("name", F64)
def test_fp64_batches_take_their_routes(name):
    table = pc.F64_TABLES[name]
    f64 = lambda v: v in (2, 3)  # noqa: E731  (sed.h: SED_MODE_F64, SED_MODE_F64_TYPED)
    built = pc.pairs_of(pc.batch(name, 4, f64=True) + pc.batch(name, 8, f64=True))
    for mode, count in ((2, 260), (3, 100)):
        pairs = built + pc.pad_pairs(count - len(built), "f64 %s" % name, pc.IUPAC)
        got = planned(table, pairs, schedule=True, mode=mode, split=2, seg=2)
        has(got, mode=f64, rows_per_lane=4, split_tasks=0, segment_pairs=0, lane_pairs=0, traceback_mode=1)
        assert "f64" in got["steps"] and "tb_codes" in got["steps"]
    built = pc.pairs_of(pc.batch(name, 4, SW=16, f64=True) + pc.batch(name, 8, SW=16, f64=True))
    pairs = built + pc.pad_pairs(300 - len(built), "seg %s" % name, pc.IUPAC)
    got = planned(table, pairs, schedule=True, seg=1)
    has(got, mode=f64, rows_per_lane=4, split_tasks=0, segment_pairs=300, traceback_mode=1)
    assert "f64_seg" in got["steps"] and "tb_seg" in got["steps"]
    for R in (2, 4):
        pairs = pc.pairs_of(pc.f64_split_batch(name, R))
        got = planned(table, pairs, schedule=True, split=1, R=0 if R == 2 else R)
        has(got, mode=f64, rows_per_lane=R, split_tasks=lambda v: v > 0, segment_pairs=0, traceback_mode=3)
        assert "tb_stripes" in got["steps"] and {255, 256, 257} <= {len(b) for _, b in pairs}
