"""CPU: the similarity join across its numeric envelope (tests/join_envelope.py): the planner at and one step past each
of its borders, the case builders judged by the C oracle alone, the plan of the split-wave case, and the two integer
kernels' lanes restated word for word (the scaled DP with its cost bytes, perm selectors, offset keys and decode; the
bit-parallel recurrence under the planner's 2-bit code map) against the oracle on the integer scale.

The DP model also measures the envelope's margin: over the limit tables the smallest key a lane meets is
KB - 32 (255 << 16) - 32 = 0xE01FFFDC (32 free substitutions under insert + delete = 255), far above the 0 an unsigned
minimum would wrap at; a key's low half-word sinks by at most 32 below KB's 0xFFFC, so it never borrows from the
distance; the largest decoded distance is 32 * 255 = 8160, far below the cutoff clamp 65535."""
import math
import re

import numpy as np
import pytest

import join_cases as jc
import join_envelope as je
import join_f64_cases as jf
import sedgpu

INF = math.inf
_REF = {}  # computed once, shared, never changed


def limit_ref(name):
    """(plan, S, rows, columns, oracle D) of a limit table over max_pairs, zero_pairs and one length grid."""
    if name not in _REF:
        plan, S = je.limit_tables()[name]
        pairs = je.max_pairs(plan) + je.zero_pairs(plan)
        seqs = je.length_grid(je.ALPHA[0] + je.ALPHA[1], 2)
        rows, cols = [a for a, _ in pairs] + seqs, [b for _, b in pairs] + seqs
        D = jc.oracle_matrix(plan, rows, cols)
        D.setflags(write=False)
        _REF[name] = (plan, S, rows, cols, D)
    return _REF[name]


def int_plan(plan, rows, cols, T, self_join=False, options=None):
    return sedgpu.join_plan(jc.costs_of(plan), options or {}, [len(s) for s in rows], [len(s) for s in cols], self_join,
                            jc.codes_mask(plan, rows), jc.codes_mask(plan, cols), T)


# ---- the planner's borders ----

@pytest.mark.parametrize("name", list(je.LIMITS))
def test_planner_accepts_every_limit_table(name):
    plan, S = je.limit_tables()[name]
    _, i, d, K = je.LIMITS[name]
    assert (plan.K, plan.ins * S, plan.dele * S) == (K, i, d) and je.scale_of(plan) == S
    sub = np.asarray(plan.sub) * S
    assert (sub[je.ZERO_CELL], sub[je.UNIT_CELL], sub[je.FULL_CELL], sub[je.BELOW_CELL]) == (0, 1, i + d, i + d - 1)
    assert (sub <= i + d).all() and (sub != sub.T).any()
    full = (1 << K) - 1
    p = sedgpu.join_plan(jc.costs_of(plan), {}, [5], [7], False, full, full, 1.0)
    assert (p["scale"], p["kernel"]) == (S, 1)
    assert sedgpu.join_route(jc.costs_of(plan), {}, [5], [7], False, full, full, 1.0) == ("int", "")


def test_a_nonzero_diagonal_plans_the_dp():
    """i127_d128 charges C -> C 3; the oracle honours it, and over A and C alone, with insert = delete = 1 and every
    other cell unit, only that entry keeps the bit-parallel kernel out."""
    plan, _ = je.limit_tables()["i127_d128"]
    assert plan.sub[1, 1] * 1 == 3
    assert jc.oracle_matrix(plan, ["CC"], ["CC"])[0, 0] == 6.0
    sub = 1.0 - np.eye(4)
    unit = je.CodePlan(sub, 1.0, 1.0)
    assert sedgpu.join_plan(jc.costs_of(unit), {}, [5], [7], False, 15, 15, 1.0)["kernel"] == 2
    sub[1, 1] = 0.5
    diag = je.CodePlan(sub, 1.0, 1.0)
    assert sedgpu.join_plan(jc.costs_of(diag), {}, [5], [7], False, 15, 15, 1.0)["kernel"] == 1
    assert sedgpu.join_plan(jc.costs_of(diag), {}, [5], [7], False, 0b1101, 0b1101, 1.0)["kernel"] == 2  # C is not met
    assert je.unit_map(diag, 15, 15) is None and je.unit_map(diag, 0b1101, 0b1101) == 0b10_01_00_00


@pytest.mark.parametrize("name", list(je.refused_neighbours()))
def test_first_refused_neighbour_of_each_rule(name):
    plan, why = je.refused_neighbours()[name]
    full = (1 << plan.K) - 1
    with pytest.raises(sedgpu.SedError) as ei:
        sedgpu.join_plan(jc.costs_of(plan), {}, [5], [7], False, full, full, 1.0)
    assert ei.value.code == sedgpu.SED_E_RANGE
    route, text = sedgpu.join_route(jc.costs_of(plan), {}, [5], [7], False, full, full, 1.0)
    assert route == "f64" and re.search(why, text), (name, text)
    assert sedgpu.join_f64_plan(jc.costs_of(plan), {}, [5], [7], False, full, full, 1.0)["kernel"] == 3


def test_bitpar_tables_plan_the_bit_parallel_kernel():
    for name, (plan, S, symbols) in je.bitpar_tables().items():
        rows, cols = (["AC", "CA"], ["YS", "SSY"]) if symbols is None else ([symbols], [symbols[::-1]])
        p = int_plan(plan, rows, cols, 1.0)
        assert (p["scale"], p["kernel"]) == (S, 2), name
        assert int_plan(plan, rows, cols, 1.0, options={sedgpu.SED_OPT_JOIN_DP: 2})["kernel"] == 1
        assert je.unit_map(plan, jc.codes_mask(plan, rows), jc.codes_mask(plan, cols)) is not None
    plan = je.one_way_table()
    assert int_plan(plan, ["YS"], ["AC"], 1.0)["kernel"] == 1           # the other way costs 0.5
    assert int_plan(plan, ["AC", "ACG"], ["YS"], 1.0)["kernel"] == 1    # a fifth code
    assert je.unit_map(plan, 0b11000000, 0b11) is None and je.unit_map(plan, 0b111, 0b11000000) is None
    assert je.unit_map(plan, 0b11, 0b11000000) == (1 << 2) | (2 << 12) | (3 << 14)
    assert je.unit_map(je.unit_block_table(), 0b11001010, 0b11001010) == (1 << 6) | (2 << 12) | (3 << 14)


# ---- the builders, judged by the oracle alone ----

def test_length_grids_cover_every_class():
    seqs = je.length_grids("AC")
    assert len(seqs) == 99 and set("".join(seqs)) == {"A", "C"}
    lens = [len(s) for s in seqs]
    assert sorted(lens) == sorted(list(range(33)) * 3) and lens[:33] != sorted(lens[:33])
    self_classes = {(lens[i], lens[j]) for i in range(99) for j in range(99) if i != j}
    assert len(self_classes) == 33 * 33 and len({(n, n) for n in lens}) == 33  # the search's n = m, identical pairs included
    plan = jc.plan_for(jc.served_tables()["costs ACGU"][0], "ACGU")
    D = jc.oracle_matrix(plan, seqs, seqs)
    assert 10 <= len(np.unique(D)) <= 33  # two symbols: small distances, which many cutoffs split


def test_max_pairs_reach_the_largest_distances():
    for name, want in (("i127_d128", {8160, 32 * 127, 32 * 128}), ("i1_d254", {32 * 254, 32 * 255, 32}),
                       ("i254_d1", {32 * 254, 32 * 255, 32}), ("s256", {8160}), ("s256_i1", {8160, 32 * 254})):
        plan, S = je.limit_tables()[name]
        got = {int(jc.oracle_matrix(plan, [a], [b])[0, 0] * S) for a, b in je.max_pairs(plan)}
        assert want <= got and max(got) == 32 * 255, (name, got)
        zero = [jc.oracle_matrix(plan, [a], [b])[0, 0] * S for a, b in je.zero_pairs(plan)]
        assert zero[0] == 0 and len(je.limit_set(plan)) == 100


def test_lane_position_and_identical_sets():
    seqs = je.lane_position_set()
    assert len(seqs) == len(set(seqs)) == 257 and {len(s) for s in seqs} == {17} and set("".join(seqs)) == set("ACGU")
    plan = jc.plan_for(jc.served_tables()["costs ACGU"][0], "ACGU")
    D = jc.oracle_matrix(plan, [seqs[p] for p in je.LANE_QUERIES], seqs)
    for q, p in enumerate(je.LANE_QUERIES):
        assert np.nonzero(D[q] == 0)[0].tolist() == [p]
    same = je.identical_set()
    assert len(same) == 130 and len(set(same)) == 1 and len(same[0]) == 17


def test_split_wave_set_geometry():
    seqs = je.split_wave_set()
    lens = [len(s) for s in seqs]
    assert len(seqs) == 65 and set(lens) == {10, 11, 12, 13, 14} and lens[:5] == [10, 11, 12, 13, 14]
    col = je.sorted_lengths(seqs)
    assert len(set(col[:64])) >= 2 and col[63] != col[64]
    assert [p for p in range(1, 65) if col[p] != col[p - 1]] == [13, 30, 45, 64]


@pytest.mark.parametrize("T", [0.0, 1.0, 2.0, INF])
def test_split_wave_plan_integer(T):
    """insert = delete = 1: at T = 1 a row of 12 symbols is in scope for columns of 11..13 only."""
    seqs = je.split_wave_set()
    lens = [len(s) for s in seqs]
    for name in ("costs ACGU", "costs ACGUN"):
        table, al, S = jc.served_tables()[name]
        plan = jc.plan_for(table, al)
        p = int_plan(plan, seqs, seqs, T, True)
        assert (p["run"], p["cells"]) == jc.lower_bound_count(lens, lens, 1.0, 1.0, T, S, list(range(65))), (name, T)
        q = int_plan(plan, seqs[:7], seqs, T)
        assert (q["run"], q["cells"]) == jc.lower_bound_count(lens[:7], lens, 1.0, 1.0, T, S)
    if T == 1.0:
        assert int_plan(plan, [seqs[lens.index(12)]], seqs, T)["run"] == sum(11 <= m <= 13 for m in lens)


def test_split_wave_plan_f64():
    """The rounding table (insert 0.1, delete 0.2): just above one insert a row of 12 is in scope for 12 and 13."""
    table, al = jf.rounding_table()
    plan = jc.plan_for(table, al)
    seqs = je.split_wave_set()
    lens = [len(s) for s in seqs]
    mask = jc.codes_mask(plan, seqs)
    for T in (float(np.nextafter(0.1, INF)), float(np.nextafter(0.2, INF)), 0.1, INF):
        keep = jf.keep_rule(plan.ins, plan.dele, T)
        p = sedgpu.join_f64_plan(jc.costs_of(plan), {}, lens, lens, True, mask, mask, T)
        assert (p["run"], p["cells"]) == jf.keep_count(lens, lens, keep, list(range(65))), T
    keep = jf.keep_rule(plan.ins, plan.dele, float(np.nextafter(0.1, INF)))
    assert [m for m in range(10, 15) if keep[12, m]] == [12, 13]


# ---- one lane of the DP variant ----

@pytest.mark.parametrize("name", list(je.LIMITS))
def test_dp_lane_model_on_the_limit_tables(name):
    plan, S, rows, cols, D = limit_ref(name)
    DS, lo_key, hi_low = je.dp_lane_matrix(plan, S, rows, cols)
    want = D * S
    assert np.array_equal(want, np.floor(want)) and np.array_equal(DS, want.astype(np.int64)), name
    ins_del = int((plan.ins + plan.dele) * S)
    assert ins_del == 255 and DS.max() == 32 * 255 and DS.min() == 0
    # the margin: 32 free substitutions give the smallest key there is, and it is the bound of the design
    assert lo_key == je.KB - 32 * (ins_del << 16) - 32 == 0xE01FFFDC and lo_key > 0
    assert hi_low == 32  # (<= 0xFFFC: the low half-word never borrows)
    # the cutoffs through the planner's clamp, against the oracle's matrix cut on the host
    sq = len(rows) - 33  # the grid's own square block: a self join
    for T in je.cutoffs(plan, D[sq:, sq:], S):
        got = je.hits_of_scaled(DS[sq:, sq:], je.planner_cut(T, S), S, True)
        assert jc.same_hits(got, je.expected_hits(D[sq:, sq:], T, S, True)), (name, T)
    assert [je.planner_cut(T / S, S) for T in je.CLAMP_CUTOFFS] == [65535] * 5 and je.CUT_ALL > 32 * 255


def test_dp_lane_model_cost_bytes():
    """Both ends of the addend byte occur, and the selectors pick byte b of the row."""
    plan, S = je.limit_tables()["i127_d128"]
    row = je.cost_rows(plan, S)
    byte = lambda a, b: (int(row[a, b >> 2]) >> (8 * (b & 3))) & 0xFF
    assert byte(*je.ZERO_CELL) == 0x00 and byte(*je.FULL_CELL) == 0xFF and byte(*je.BELOW_CELL) == 0xFE
    assert byte(1, 1) == 3 and byte(0, 0) == 0
    for b in range(8):
        w = int(je.perm(np.int64(row[1, 1]), np.int64(row[1, 0]), np.array([je.scaled_sel(b)], np.int64))[0])
        assert w == 0xFF00FFFF | (byte(1, b) << 16)


# ---- the bit-parallel lane under the 2-bit code map ----

@pytest.mark.parametrize("name", list(je.bitpar_tables()))
def test_bitpar_model_under_the_code_map(name):
    plan, S, symbols = je.bitpar_tables()[name]
    if symbols is None:  # the search whose query codes are disjoint from the index's
        rows, cols = je.near_set(11, je.ALPHA[0:2], 40), je.near_set(12, je.ALPHA[6:8], 60)
    else:
        rows = cols = je.length_grid(symbols[1] + symbols[3], 4) + je.near_set(13, symbols, 30)
    D = jc.oracle_matrix(plan, rows, cols)
    DS = je.bitpar_matrix(plan, S, rows, cols)
    assert np.array_equal(DS, (D * S).astype(np.int64)) and np.array_equal(D * S, np.floor(D * S)), name
    for T in je.BITPAR_CUTOFFS:
        got = je.hits_of_scaled(DS, je.planner_cut(T, S), S)
        assert jc.same_hits(got, je.expected_hits(D, T, S)), (name, T)
    if symbols is None:
        assert not np.array_equal(D, jc.oracle_matrix(plan, cols, rows).T)  # the other way costs 0.5
