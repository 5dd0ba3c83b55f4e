"""CPU: the cases of tests/f64_pair_cases.py hit what they claim, without a device.

a. Route placement.  Every case tests/test_gpu_f64_pair_envelope.py runs goes through the planner (sedgpu.plan_routes)
and lands where it claims to: fp64 with simple typing or typed as the table says, never the integer or the scaled
route; the rows per lane; the lane, segment, bit-parallel and SPLIT counts.  The planner exports no unit-cost mask, so
k32_unit_high's is read off one-symbol pairs: code c is in the mask exactly when ([c], [c]) is planned bit-parallel.

b. The tables.  Every mismatch entry of the K-tables is live in their sweep; near_tie's cells tie and nearly tie by the
thousand, and a DP that reassociates the update candidate, or sums a path's costs exactly, writes another script than the
oracle; huge, huge_mixed and subnormal reach the values they are named for."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden
import f64_pair_cases as fc
import oracle
import sedcost
import sedgpu


def build(name):
    return sedcost.build_plan(fc.table(name), [fc.alphabet(name)], [fc.alphabet(name)])


def plan_costs(name):
    p = build(name)
    return (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
            float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))


def planned(case):
    return sedgpu.plan_routes(plan_costs(case.name), case.plan_opts, sedgpu.PackedPairs(case.A, case.B), case.flags)


def oracle_batch(name, A, B, want_ops=False):
    p = sedgpu.PackedPairs(A, B)
    return oracle.batch(oracle.Costs.from_plan(build(name)), p.codes_a, p.off_a, p.len_a, p.codes_b, p.off_b, p.len_b,
                        p.npairs, want_ops=want_ops)


# ---- a. route placement ----
def test_tables_are_what_they_claim():
    for name, (t, al, mode) in fc.TABLES.items():
        p = build(name)
        assert p.K == len(al) and list(p.alphabet) == list(al), name
        off = ~np.eye(p.K, dtype=bool)
        folds = np.array([[a.lower() == b.lower() for b in al] for a in al])
        assert np.isfinite(p.sub).all() and np.isfinite([p.ins, p.dele]).all(), name
        assert (p.sub[folds] == 0).all() and p.sub_int[folds].all(), name  # the planner's int 0
        assert (p.sub[~folds] != 0).all(), name
        simple = not p.ins_int and not p.del_int and p.ins > 0 and p.dele > 0 and \
            (p.sub[~folds] > 0).all() and not p.sub_int[~folds].any()
        assert simple == (mode == fc.F64), name
        assert (folds & off).sum() == {17: 4, 31: 30, 32: 30}.get(p.K, 0), name
    k32 = build("k32")
    folds = np.array([[a.lower() == b.lower() for b in fc.SYMS32] for a in fc.SYMS32])
    v = k32.sub[~folds]
    assert len(v) == 962 == len(set(v.tolist())) and (v > 0.55).all() and (v < 0.95).all()
    assert (np.ldexp(v, 30) != np.floor(np.ldexp(v, 30))).all()  # not dyadic: no scaled-integer route
    assert (k32.sub != k32.sub.T)[~folds].all()
    for name in ("k17", "k31"):
        K = len(fc.alphabet(name))
        assert np.array_equal(build(name).sub, k32.sub[:K, :K]), name
    assert np.array_equal(build("huge").sub, k32.sub * 1e308) and build("huge").dele == 1.1 * 1e308
    typed = build("k32_typed")
    assert typed.ins_int and not typed.del_int and (typed.ins, typed.dele) == (2.0, 3.0)
    assert typed.sub_int[~folds].sum() == -(-962 // 3) and set(typed.sub[typed.sub_int.astype(bool)]) == {0.0, 1.0, 2.0}
    near = build("near_tie")
    assert {0.3, 0.30000000000000004} <= set(near.sub.ravel()) <= set(fc.NEAR_VALUES) | {0.0}
    mixed = build("huge_mixed")
    assert set(mixed.sub.ravel()) == set(fc.HUGE_MIXED_VALUES) | {0.0} and mixed.ins == mixed.dele == 1e308
    sub = build("subnormal")
    stored = np.array([sub.ins, sub.dele] + sub.sub.ravel().tolist())
    assert (stored.view(np.uint64) >> np.uint64(32) == 0).all()  # a zero high word
    assert set((sub.sub / fc.TINY).ravel()) == set(range(8)) and (sub.ins, sub.dele) == (3 * fc.TINY, 5 * fc.TINY)
    inf_low = np.array([np.inf]).view(np.uint64)[0] & np.uint64(0xFFFFFFFF)
    assert inf_low == 0  # +inf: a zero low word


def test_every_case_is_planned_where_it_claims():
    seen = set()
    for case in fc.all_cases():
        got = planned(case)
        assert not fc.misses(case.expect, got), (case.label, fc.misses(case.expect, got))
        seen.add((case.label.split()[0], got["mode"]))
    assert seen == {(kind, mode) for kind in ("wave", "seg", "split") for mode in (fc.F64, fc.TYPED)} | \
        {("lane", fc.F64), ("full", fc.F64)}


def test_shapes_cross_the_seams_they_name():
    for name in fc.WAVE_TABLES:
        for R in fc.WAVE_R:
            A, B = fc.wave_batch(name, R)
            assert {(64 * R + d, m) for d in (-1, 0, 1) for m in fc.WAVE_M} | {(1, 1)} <= {(len(a), len(b)) for a, b in zip(A, B)}
            A, B = fc.seg_batch(name, R)
            assert len(A) == fc.SEG_PAIRS and max(map(len, A)) == 32 * R + 1
            assert {(16 * R + d, m) for d in (-1, 0, 1) for m in fc.SEG_M} <= {(len(a), len(b)) for a, b in zip(A, B)}
        for R in fc.SPLIT_R:
            A, B = fc.split_batch(name, R)
            assert len(A) <= 16 and {len(a) for a in A} == {64 * R + 1, 128 * R + 1}
            assert {(n, m) for n in (64 * R + 1, 128 * R + 1) for m in fc.SPLIT_M} <= {(len(a), len(b)) for a, b in zip(A, B)}
    for name in fc.LANE_TABLES:
        A, B = fc.lane_batch(name)
        assert {(n, m) for n in fc.LANE_N for m in fc.LANE_M} <= {(len(a), len(b)) for a, b in zip(A, B)}


def test_unit_high_mask_is_the_last_four_codes():
    for name, want in (("k32_unit_high", fc.UNIT_HIGH_MASK), ("n_first", fc.N_FIRST_MASK)):
        costs = plan_costs(name)
        mask = 0
        for c in range(costs[0]):
            one = sedgpu.PackedPairs([np.array([c], np.uint8)], [np.array([c], np.uint8)])
            got = sedgpu.plan_routes(costs, {}, one, 4)  # SED_NO_LEN
            assert got["mode"] == fc.F64 and got["lane_pairs"] == 1
            mask |= got["bitpar_pairs"] << c
        assert mask == want, name
    # the subset does not hang on which symbol a batch meets first: costs.json's ACGU, with N before or after them
    # (a pass of unit_subset that began at N, which costs 0.75 against the others, used to end with N alone)
    for al in ("ACGUN", "NACGU", "ANCGU"):
        p = sedcost.build_plan(load_golden("costs.json"), [al], [al])
        got = ""
        for c in range(5):
            one = sedgpu.PackedPairs([np.array([c], np.uint8)], [np.array([c], np.uint8)])
            r = sedgpu.plan_routes((5, p.sub.ravel(), p.sub_int.ravel(), p.ins, p.ins_int, p.dele, p.del_int), {}, one, 4)
            got += al[c] * r["bitpar_pairs"]
        assert got == al.replace("N", ""), (al, got)
    A, B = fc.lane_batch("k32_unit_high")
    inside = fc.in_unit_subset("k32_unit_high", A, B)
    assert len(inside) == 12 and {(len(A[p]), len(B[p])) for p in inside} == {(n, m) for n in fc.LANE_N for m in fc.LANE_M}
    # the subset is worth running: a pair inside it has a distance above 0 unless it is one symbol repeated
    d = oracle_batch("k32_unit_high", [A[p] for p in inside], [B[p] for p in inside])[0]
    assert (d == np.floor(d)).all() and (d > 0).sum() >= 10


# ---- b. the tables ----
@pytest.mark.parametrize("name", fc.K_TABLES)
def test_every_mismatch_entry_is_live_in_the_sweep(name):
    """Entry (a, b) times 1.5 changes the distance or the script of the sweep's pair (a^(K - 1), the other symbols):
    every column of that pair is paid by an update or by an insert and a delete, which cost more than any mismatch,
    perturbed or not.  No entry is left out."""
    p = build(name)
    K = p.K
    A, B = fc.sweep(name)
    assert len(A) == 2 * K and all(len(a) == len(b) == K - 1 for a, b in zip(A, B))
    for side in (A, B):  # symbol K - 1 stands first and last on both sides
        assert any(s[0] == K - 1 for s in side) and any(s[-1] == K - 1 for s in side)
        assert {int(s[0]) for s in side} == {int(s[-1]) for s in side} == set(range(K))
    base = [oracle.pair(oracle.Costs.from_plan(p), a, b) for a, b in zip(A[:K], B[:K])]
    dead = []
    for a in range(K):
        for b in range(K):
            if fc.alphabet(name)[a].lower() == fc.alphabet(name)[b].lower():
                continue
            sub = p.sub.copy()
            sub[a, b] *= 1.5
            o = oracle.pair(oracle.Costs(sub, p.sub_int, p.ins, p.ins_int, p.dele, p.del_int), A[a], B[a])
            if o["dist"] == base[a]["dist"] and np.array_equal(o["ops"], base[a]["ops"]):
                dead.append((a, b))
    assert not dead, dead[:10]


def _candidates(name, a, b):
    """(insert, delete, update) candidates of every interior cell, recomputed from the oracle's matrix."""
    p = build(name)
    D = oracle.pair(oracle.Costs.from_plan(p), a, b, want_ops=False, full=True)["D"]
    cand = np.stack([D[1:, :-1] + p.ins, D[:-1, 1:] + p.dele, D[:-1, :-1] + p.sub[np.ix_(a, b)]])
    assert np.array_equal(cand.min(0), D[1:, 1:])
    return cand


def py_dp(p, a, b, update, value=float):
    """The oracle's recurrence in Python with the update candidate and the cell value to choose: returns the script.
    update(diag, cost, ins) -> candidate; value: what a candidate is compared and stored as."""
    n, m = len(a), len(b)
    ins, dele = value(p.ins), value(p.dele)
    D = [[value(0)] * (m + 1) for _ in range(n + 1)]
    L = [[0] * (m + 1) for _ in range(n + 1)]
    ch = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(1, m + 1):
        D[0][j], L[0][j] = value(j * p.ins), j
    for i in range(1, n + 1):
        D[i][0], L[i][0], ch[i][0] = value(i * p.dele), i, 1
        for j in range(1, m + 1):
            cand = (D[i][j - 1] + ins, D[i - 1][j] + dele, update(D[i - 1][j - 1], value(p.sub[a[i - 1], b[j - 1]]), ins))
            key = [float(c) for c in cand]  # (an exact sum is compared as the double it rounds to)
            v = min(key)
            lp = (L[i][j - 1], L[i - 1][j], L[i - 1][j - 1])
            k = min((lp[q], q) for q in range(3) if key[q] == v)[1]
            D[i][j], L[i][j], ch[i][j] = cand[key.index(v)], lp[k] + 1, k
    ops, i, j = [], n, m
    while i or j:
        op = ch[i][j] if i and j else (0 if not i else 1)
        ops.append(op)
        i, j = i - (op != 0), j - (op != 1)
    return ops[::-1]


def test_near_tie_cells_tie_and_nearly_tie_and_the_case_bites():
    A, B = fc.wave_batch("near_tie", 4)
    ties = near = cells = 0
    for a, b in zip(A, B):
        cand = _candidates("near_tie", a, b)
        mn = cand.min(0)
        ties += int(((cand == mn).sum(0) >= 2).sum())
        near += int(((cand != mn) & (cand - mn <= 2 * np.spacing(mn))).any(0).sum())
        cells += mn.size
    print("near_tie: %d cells, %d with an exact tie, %d with a loser within 2 ulp" % (cells, ties, near))
    assert ties >= 1000 and near >= 300
    # two DPs that are each right in exact arithmetic, on the 40 x 40 pairs of the same batch: one reassociates the
    # update candidate as a fused or reordered add would; the other stands in for a DP on an FMA-free fsum: a cell is
    # the exact sum of its path's costs (Fractions) and is compared as the double that sum rounds to, which is what
    # math.fsum over the path's costs returns
    p = build("near_tie")
    A, B = fc.probe("near_tie")
    want = [oracle.pair(oracle.Costs.from_plan(p), a, b)["ops"].tolist() for a, b in zip(A, B)]
    same = [py_dp(p, a, b, lambda d, c, ins: d + c) for a, b in zip(A, B)]
    assert same == want  # (the Python DP itself is the oracle's)
    reassoc = [py_dp(p, a, b, lambda d, c, ins: (d + ins) + (c - ins)) for a, b in zip(A, B)]
    exact = [py_dp(p, a, b, lambda d, c, ins: d + c, value=Fraction) for a, b in zip(A, B)]
    print("near_tie: %d of %d scripts differ under a reassociated update, %d under exact path sums" % (
        sum(x != y for x, y in zip(reassoc, want)), len(want), sum(x != y for x, y in zip(exact, want))))
    assert reassoc != want and exact != want


def test_huge_sinks():
    for A, B in (fc.wave_batch("huge", 4), fc.wave_batch("huge", 8), fc.split_batch("huge", 2), fc.split_batch("huge", 4)):
        d = oracle_batch("huge", A, B)[0]
        assert not np.isnan(d).any() and (d == np.inf).sum() * 2 >= len(d)
        assert (np.isfinite(d) & (d > 0)).any()  # one_mismatch: a finite sink that is not the empty script's 0


def test_huge_mixed_sinks():
    A, B = fc.wave_batch("huge_mixed", 4)
    d = oracle_batch("huge_mixed", A, B)[0]
    assert (d == np.inf).any() and (d == -np.inf).any() and not np.isnan(d).any()
    for a, b in zip(A[:6], B[:6]):  # no cell of a matrix either
        D = oracle.pair(oracle.Costs.from_plan(build("huge_mixed")), a, b, want_ops=False, full=True)["D"]
        assert not np.isnan(D).any()


def test_subnormal_sinks():
    for A, B in (fc.wave_batch("subnormal", 4), fc.lane_batch("subnormal")):
        d = oracle_batch("subnormal", A, B)[0]
        assert (d >= 0).all() and (d < np.finfo(np.float64).tiny).all() and (d > 0).any()
