"""CPU: the envelope of the fp64 k-nearest calls, proved before tests/test_gpu_join_knn_f64_envelope.py runs it on a
device.  On every call of join_knn_f64_envelope.envelope_calls() the two passes restated word for word
(join_knn_f64_cases.bound_pass_model, emit_pass_model) end at the bounds and the list of the definition in every
schedule; the ladders' distances are the chosen doubles bit for bit; the bisection takes and leaves every bit 62..0 in a
wave that sets a final bound; and restatements that are subtly wrong - a bisection that skips one round, starts or ends
a bit late, compares <=, asks for k - 1, orders keys by (low word, high word), a bound whose low word is sign-extended,
no self rule, codes masked with 0x07 - disagree with the definition on some call."""
import math

import numpy as np
import pytest

import join_cases as jc
import join_knn_cases as kc
import join_knn_f64_cases as kf
import join_knn_f64_envelope as ke
import sedgpu

INF = math.inf
U64 = np.uint64


def distinct(calls):
    """One call per model input (the options change the launches, never the result)."""
    seen = {}
    for c in calls:
        seen.setdefault(c.key(), c)
    return list(seen.values())


def by_definition(c):
    s, cols, _, D, self_join, lo = ke.call_inputs(c)
    return kf.pass1_by_definition(D, [len(x) for x in cols], c.k, c.T, self_join, lo)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(U64), np.ascontiguousarray(b, np.float64).view(U64))


def trimmed(c, mask):
    """The candidates of a mask as records, shuffled, through the library's trim."""
    _, _, _, D, _, lo = ke.call_inputs(c)
    r, col = np.nonzero(mask)
    hits = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
    hits["row"], hits["col"], hits["dist"] = r + lo, col, D[r, col]
    return sedgpu.join_knn_trim(hits[np.random.default_rng(2).permutation(len(hits))], c.k)


# ---- the oracle is the reference for D ----

@pytest.mark.parametrize("name", ke.LADDERS)
def test_ladder_distances_are_the_chosen_doubles(name):
    """D(BASE, column) is the table entry bit for bit (top: or +inf, the sum of two 2^1023-scale costs); the columns of
    a wave are pairwise different doubles (top: but for its two at +inf)."""
    table, cols, want = ke.ladder(name)
    s = ke.envelope_set(("ladder", name))
    assert s.cols == cols and s.queries == [ke.BASE] and s.plan.K == 16 and all(len(x) == 32 for x in cols + [ke.BASE])
    assert len(cols) == (128 if name == "two waves" else 64)
    assert same_bits(s.Dq[0], want)
    indel = 2.0 ** (1023 if name == "top" else 1000)
    assert s.plan.ins == s.plan.dele == indel and not np.diag(s.plan.sub).any()
    finite = [v for v in want if v != INF]
    assert max(finite) < (INF if name == "top" else indel) and min(finite) >= 0
    for w in range(0, len(cols), 64):
        wave = [ke.key_of(v) for v in want[w:w + 64] if v != INF]
        assert len(set(wave)) == len(wave) == (62 if name == "top" else 64)
    if name == "top":
        assert want.count(INF) == 2 and ke.MAX_DOUBLE in want
        for i, j in ke.TOP_PAIRS:
            assert ke.top_values()[i] + ke.top_values()[j] == INF and min(ke.top_values()[i], ke.top_values()[j]) >= 2.0 ** 1022


def test_ladder_values_are_what_the_issue_lists():
    ev = [ke.key_of(v) for v in ke.exponent_values()]
    for e in (-1074, -1060, -1023, -1022, -500, 0, 500, 999):
        assert ke.key_of(2.0 ** e) in ev
    for e0 in ke.EXPONENT_BASES:  # pairs that differ in one exponent bit, each of the 11
        for j in range(11):
            assert e0 << 52 in ev and (e0 ^ 1 << j) << 52 in ev
    lo, hi = ke.fraction_low_pairs(), ke.fraction_high_pairs()
    assert [t for t, _, _ in lo + hi] == list(range(52))
    fv = {ke.key_of(v) for v in ke.fraction_low_values() + ke.fraction_high_values()}
    for t, a, b in lo + hi:  # pairs that differ in fraction bit t alone, neighbours in their wave's order
        assert a ^ b == 1 << t and {a, b} <= fv
        assert not [k for k in fv if min(a, b) < k < max(a, b)]
    edge = ke.word_edge_keys()
    assert any(k & 0xFFFFFFFF == 0x80000000 and k >> 32 not in (0, 0x7FF00000) for k in edge)
    assert any(k & 0xFFFFFFFF == 0 for k in edge) and any(k & 0xFFFFFFFF == 0xFFFFFFFF for k in edge)
    # as (low, high) pairs the seam's keys order otherwise
    swap = lambda k: (k & 0xFFFFFFFF) << 32 | k >> 32
    assert sorted(edge) != sorted(edge, key=swap)
    assert len(ke.wide_values()) == 192 <= 240 and len({ke.entry(i) for i in range(240)}) == 240
    assert all(a != b for a, b in map(ke.entry, range(240)))


# ---- the passes on every call ----

def test_the_envelope_is_the_issues():
    calls = ke.envelope_calls()
    assert {c.group for c in calls} == {"ladders", "columns", "k", "rows", "cutoffs", "rerun", "cross"}
    assert {(c.case, c.k) for c in ke.envelope_calls("ladders")} == {(n, k) for n in ke.LADDERS for k in range(1, 65)}
    cols = ke.envelope_calls("columns")
    assert {c.ncols for c in cols} == {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300}
    assert {(c.k, c.queries is None) for c in cols} == {(k, q) for k in (1, 2, 8) for q in (True, False)}
    assert {c.rows for c in ke.envelope_calls("rows", "self")} == {(1, 2), (3, 9), (5, 6), (139, 140)}
    assert len(ke.envelope_set(("rows",) * 2).cols) == 140
    assert {len(c.queries) for c in ke.envelope_calls("rows", "search")} == {1, 4, 5, 9}
    assert {dict(c.options)[sedgpu.SED_OPT_JOIN_ROWS] for c in ke.envelope_calls("rows")} == {1, 3, 4, 5}
    assert {c.k for c in ke.envelope_calls("k")} == {1, 2, 63, 64}
    assert all(len(ke.call_inputs(c)[1]) <= 300 and max(map(len, ke.call_inputs(c)[1])) <= 32 for c in calls)


def test_bounds_are_the_same_in_every_schedule():
    """On every call the bound pass ends at the definition's bounds bit for bit under the sequential, reversed,
    all-stale and shuffled-with-stale-reads orders; the emit pass appends the definition's candidates, and their trim
    is the expected list."""
    calls = distinct(ke.envelope_calls())
    assert len(calls) > 450
    for c in calls:
        want, cand = by_definition(c)
        ran = []
        for order in kc.ORDERS:
            bound, pairs = ke.call_model(c, order)
            assert same_bits(bound, want), (c, order)
            ran.append(pairs)
        mask, p2, _ = ke.call_emit(c)
        assert int(mask.sum()) == cand, c
        assert p2 <= min(ran) and max(ran) == ran[kc.ORDERS.index("stale")], c
        assert jc.same_hits(trimmed(c, mask), ke.call_expected(c)), c


def test_conditions_that_keep_the_device_tests_honest():
    # every ladder call: a wave with k candidates for the base row; the bound is that k-th distance, below max_dist (but
    # where the k-th distance is +inf itself: the last two ranks of `top`)
    at_inf = []
    for c in ke.envelope_calls("ladders"):
        s, cols, _, D, _, _ = ke.call_inputs(c)
        assert c.T == INF and D.shape[0] == 1
        kth = min(float(np.sort(D[0, w:w + 64])[c.k - 1]) for w in range(0, len(cols), 64))
        bound = ke.call_model(c)[0]
        assert same_bits(bound, [kth]), c
        if kth == INF:
            at_inf.append((c.case, c.k))
        else:
            assert bound[0] < c.T, c
    assert at_inf == [("top", 63), ("top", 64)]
    # the two-wave ladder's bound comes from either wave
    two = ke.envelope_set(("ladder", "two waves")).Dq[0]
    first = [float(np.sort(two[:64])[k - 1]) < float(np.sort(two[64:])[k - 1]) for k in range(1, 65)]
    assert 8 <= sum(first) <= 56
    # a third of all (call, row) bounds end strictly below max_dist
    below = total = 0
    for c in distinct(ke.envelope_calls()):
        bound = ke.call_model(c)[0]
        below += int((bound < c.T + 0.0).sum())
        total += len(bound)
    assert 3 * below >= total, (below, total)
    # rows: a call of three or more launches; a ragged last group; ranges off the multiples of the group
    assert sedgpu.join_rows_per_group() == 4
    assert max(ke.launches(c) for c in ke.envelope_calls("rows")) >= 3
    assert any(ke.launches(c) >= 3 and len(ke.call_inputs(c)[2]) % 4 for c in ke.envelope_calls("rows"))
    # rows: some bounds below a finite cap, some at it, and pass 2 leaves whole (wave, row)s out
    capped = [c for c in distinct(ke.envelope_calls("rows")) if c.T != INF]
    assert any((ke.call_model(c)[0] < c.T).any() for c in capped) and any((ke.call_model(c)[0] == c.T).any() for c in capped)
    assert any(ke.call_emit(c)[2] > 0 for c in distinct(ke.envelope_calls("rows")))
    # rerun: the candidates exceed the room a first small call leaves, over more than one launch
    small, grows = ke.envelope_calls("rerun")
    assert (small.note, grows.note) == ("small", "grows") and ke.launches(grows) > 3
    rows = len(ke.call_inputs(grows)[2])
    assert int(ke.call_emit(grows)[0].sum()) > 2 * rows * grows.k + 1024 > 2 * 4 * small.k + 1024
    _, p2, _ = ke.call_emit(grows)
    assert ke.call_model(grows, "stale")[1] == p2  # one length: the skip removes nothing, so the sandwich is 2 p2 exactly


def test_the_sixteenth_symbol_is_in_rows_and_columns():
    s = ke.envelope_set(("columns",) * 2)
    assert s.plan.K == 16 and s.cols[0][0] == s.cols[0][31] == "X" == ke.AL16[15]
    for c in ke.envelope_calls("columns"):
        _, cols, rows, _, _, _ = ke.call_inputs(c)
        for side in (cols, rows):
            assert any(len(x) == 32 and x[0] == x[31] == "X" for x in side), c
    assert bin(jc.codes_mask(s.plan, s.cols)).count("1") == 16
    assert ke.fold8("AX") == ke.AL16[0] + ke.AL16[7] and all(ke.AL16.index(ch) < 8 for ch in ke.fold8(ke.AL16))


def test_k_against_the_lanes_in_scope():
    """130 columns of one length: waves of 64, 64 and 2.  A row of the first wave sees 63, 64 and 2 columns in scope, one
    of the last 64, 64 and 1; with 127 columns no wave has 64 in scope for a row of the first and its bound stays at max_dist.  k
    = 65 and k = the 129 columns in scope are outside 1..64, which the planner refuses before anything runs: that no
    wave can hold 65 candidates is the model's statement alone."""
    s = ke.envelope_set(("same length",) * 2)
    assert len(s.cols) == 130 and {len(x) for x in s.cols} == {28}
    for c in ke.envelope_calls("k", "one row"):
        _, cols, _, D, _, lo = ke.call_inputs(c)
        ok = kc.in_scope(D.shape, True, lo)[0]
        assert [int(ok[w:w + 64].sum()) for w in (0, 64, 128)] == ([63, 64, 2] if lo == 5 else [64, 64, 1])
        bound = ke.call_model(c)[0]
        assert bound[0] < INF, c
        if c.k == 2:  # the last wave counts for row 5 and not for row 129
            last = float(np.sort(D[0, 128:][ok[128:]])[-1])
            assert (bound[0] <= last) if lo == 5 else ok[128:].sum() < c.k
    (none,) = [c for c in ke.envelope_calls("k", "none") if c.note == "none"]
    assert (none.k, none.rows, none.ncols) == (64, (0, 64), 127)
    assert (ke.call_model(none)[0] == INF).all() and (np.bincount(ke.call_expected(none)["row"]) == 64).all()
    assert int(ke.call_emit(none)[0].sum()) == 64 * 126  # pass 2 is the join at max_dist; the trim keeps 64 of a row's 126
    (whole,) = [c for c in ke.envelope_calls("k", "none") if c.k == 64 and c.rows is None]
    bound = ke.call_model(whole)[0]
    assert (bound[:64] == INF).all() and (bound[64:] < INF).all()  # a row of the second wave sees all 64 of the first
    lens = [28] * 130
    mask = jc.codes_mask(s.plan, s.cols)
    whole = next(c for c in ke.envelope_calls("k", "whole") if c.queries is None)
    for k in ke.REFUSED_K:
        with pytest.raises(sedgpu.SedError, match=r"\(-1\).*k = %d .*1\.\.64" % k):
            sedgpu.join_knn_f64_plan(jc.costs_of(s.plan), {}, lens, lens, True, mask, mask, k, INF)
        D, ok, len_rows, len_cols, low, _, T = ke.model_inputs(whole)
        assert (kf.bound_pass_model(D, ok, len_rows, len_cols, low, k, T)[0] == INF).all()


def test_cutoffs_are_adjacent_bit_patterns():
    for case in ("fraction high", "exponents", "same length"):
        calls = {c.note: c for c in ke.envelope_calls("cutoffs", case)}
        assert set(calls) == set(ke.CUTOFF_NOTES)
        d, k = calls["at d"].T, calls["at d"].k
        assert d > 0 and ke.key_of(calls["below d"].T) + 1 == ke.key_of(d) == ke.key_of(calls["above d"].T) - 1
        assert ke.key_of(calls["tiny"].T) == 1 and ke.key_of(calls["zero"].T) == 0 and ke.key_of(calls["minus zero"].T) == 1 << 63
        n = {note: len(ke.call_expected(c)) for note, c in calls.items()}
        assert n["at d"] == n["above d"] == n["largest"] == k and n["below d"] == k - 1, (case, n)
        assert n["zero"] == n["minus zero"] <= n["tiny"] < k
        assert jc.same_hits(ke.call_expected(calls["zero"]), ke.call_expected(calls["minus zero"]))
        if case == "fraction high":  # the bound pass 2 reads: bit 31 of the low word alone, a high word that is no trivial one
            assert ke.key_of(d) == 0x3FF1234580000000 and same_bits(ke.call_model(calls["at d"])[0], [d])
        if case == "same length":  # a cutoff of 0 with hits: the row's duplicates
            assert n["zero"] >= 2
        if case == "exponents":
            assert n["zero"] == 1 and n["tiny"] == 2
    (top,) = ke.envelope_calls("cutoffs", "top")
    assert top.T == ke.MAX_DOUBLE and len(ke.call_expected(top)) == 62 and same_bits(ke.call_model(top)[0], [ke.MAX_DOUBLE])


# ---- the bisection's rounds ----

def traced_bisection(trace):
    """kf.kth_by_bisection's loop with every round's outcome recorded: trace gets (x of every row, [bit -> took, per row])."""
    def kth(key_lane, cand, k):
        key_lane, cand = np.asarray(key_lane, U64), np.asarray(cand, bool)
        x = np.zeros(key_lane.shape[:-1], U64)
        took = {}
        for bit in range(62, -1, -1):
            c = x | U64(1 << bit)
            took[bit] = (cand & (key_lane < c[..., None])).sum(-1) < k
            x = np.where(took[bit], c, x)
        assert np.array_equal(x, kf.kth_by_bisection(key_lane, cand, k))
        trace.append((x, took, cand.sum(-1) >= k))
        return x
    return kth


def test_every_round_of_the_bisection_goes_both_ways():
    """Over the ladders' calls, in a (wave, row) with k candidates whose result is the row's final bound: for every bit
    62..0 some such bisection takes the bit and some leaves it."""
    taken, left = set(), set()
    for c in ke.envelope_calls("ladders"):
        trace = []
        bound, _ = kf.bound_pass_model(*ke.model_inputs(c), kth=traced_bisection(trace))
        assert same_bits(bound, ke.call_model(c)[0])
        final = bound.view(U64)
        for x, took, enough in trace:
            if enough[0] and x[0] == final[0]:
                for bit in range(63):
                    (taken if took[bit][0] else left).add(bit)
    assert taken == left == set(range(63))


# ---- mutants: a restatement that is subtly wrong must disagree on some call ----

def swap_words(key):
    key = np.asarray(key, U64)
    return (key << U64(32)) | (key >> U64(32))


def bisection(key_lane, cand, k, bits=range(62, -1, -1), below=np.less, need=0):
    """kf.kth_by_bisection with its choices open: the rounds, the compare, the count asked for."""
    key_lane, cand = np.asarray(key_lane, U64), np.asarray(cand, bool)
    x = np.zeros(key_lane.shape[:-1], U64)
    for bit in bits:
        c = x | U64(1 << bit)
        x = np.where((cand & below(key_lane, c[..., None])).sum(-1) < k + need, c, x)
    return x


def sign_extended(b):
    """A bound rebuilt from its two words with the low word taken as a signed int: bit 31 floods the high word."""
    b = np.asarray(b, U64)
    return np.where((b >> U64(31)) & U64(1) == 1, b | U64(0xFFFFFFFF00000000), b)


def skip(t):
    return dict(kth=lambda K, cand, k: bisection(K, cand, k, bits=[b for b in range(62, -1, -1) if b != t]))


MUTANTS = {"as written": dict(kth=bisection),
           "from bit 61": dict(kth=lambda K, cand, k: bisection(K, cand, k, bits=range(61, -1, -1))),
           "to bit 1": dict(kth=lambda K, cand, k: bisection(K, cand, k, bits=range(62, 0, -1))),
           "key <= c": dict(kth=lambda K, cand, k: bisection(K, cand, k, below=np.less_equal)),
           "k - 1": dict(kth=lambda K, cand, k: bisection(K, cand, k, need=-1)),
           "low word first": dict(kth=lambda K, cand, k: bisection(K, cand, k, below=lambda a, b: swap_words(a) < swap_words(b))),
           "low word sign-extended": dict(read=sign_extended)}


def mutant_result(c, how):
    """(the final bounds, the trimmed list) of the two passes with the mutation in them."""
    D, ok, len_rows, len_cols, low, k, T = ke.model_inputs(c)
    bound, _ = kf.bound_pass_model(D, ok, len_rows, len_cols, low, k, T, **how)
    mask, _, _ = kf.emit_pass_model(D, ok, len_rows, len_cols, low, bound, read=how.get("read"))
    return bound, trimmed(c, mask)


def kills(c, how):
    bound, hits = mutant_result(c, how)
    return not same_bits(bound, by_definition(c)[0]) or not jc.same_hits(hits, ke.call_expected(c))


def test_the_open_bisection_is_the_model():
    assert not any(kills(c, MUTANTS["as written"]) for c in ke.envelope_calls("ladders")[::5])


@pytest.mark.parametrize("t", range(62, -1, -1))
def test_a_bisection_that_skips_a_round_is_caught(t):
    assert any(kills(c, skip(t)) for c in ke.envelope_calls("ladders")), t


@pytest.mark.parametrize("mutant", [m for m in MUTANTS if m != "as written"])
def test_mutants_of_the_bound_pass_are_caught(mutant):
    dead = [c for c in ke.envelope_calls("ladders") if kills(c, MUTANTS[mutant])]
    assert dead, mutant
    if mutant == "low word sign-extended":  # in pass 1 (a later wave reads a bound an earlier one wrote) and in pass 2
        assert {"two waves", "fraction high"} <= {c.case for c in dead}
        assert any(not same_bits(mutant_result(c, MUTANTS[mutant])[0], by_definition(c)[0]) for c in dead)


def test_mutants_of_scope_and_codes_are_caught_by_the_columns_group():
    """No self rule: every pair in scope.  Codes masked with 0x07: the distances of the folded sequences."""
    calls = distinct(ke.envelope_calls("columns"))
    selfs = [c for c in calls if c.queries is None and c.ncols > c.k]  # (a wave with k columns once the row's own counts)
    assert len(selfs) >= 30
    for c in selfs:
        D, _, len_rows, len_cols, low, k, T = ke.model_inputs(c)
        bound, _ = kf.bound_pass_model(D, np.ones(D.shape, bool), len_rows, len_cols, low, k, T)
        assert not same_bits(bound, by_definition(c)[0]), c
    folded = ke.envelope_set(("folded",) * 2)
    dead = 0
    for c in calls:
        D, ok, len_rows, len_cols, low, k, T = ke.model_inputs(c)
        _, _, _, _, self_join, lo = ke.call_inputs(c)
        Df = folded.D[lo:lo + D.shape[0], :D.shape[1]] if self_join else folded.D[list(c.queries)][:, :D.shape[1]]
        bound, _ = kf.bound_pass_model(Df, ok, len_rows, len_cols, low, k, T)
        mask, _, _ = kf.emit_pass_model(Df, ok, len_rows, len_cols, low, bound)
        r, col = np.nonzero(mask)
        hits = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
        hits["row"], hits["col"], hits["dist"] = r + lo, col, Df[r, col]
        dead += int(not same_bits(bound, by_definition(c)[0]) or not jc.same_hits(sedgpu.join_knn_trim(hits, k), ke.call_expected(c)))
    assert dead >= len(calls) - 6, (dead, len(calls))  # (all but the prefixes of one and two columns, at the least)
