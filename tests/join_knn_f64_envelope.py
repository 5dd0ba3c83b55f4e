"""The envelope of the fp64 k-nearest calls (sed_join_knn_self_f64 / sed_join_knn_search_f64): the sets
and the list of every call tests/test_gpu_join_knn_f64_envelope.py makes (envelope_calls), which
tests/test_join_knn_f64_envelope.py proves on the CPU first.  The models are join_knn_f64_cases' (bound_pass_model,
emit_pass_model, expected_knn), the call record and the scope rule join_knn_cases' (Call, in_scope, call_inputs); every
distance comes from the C oracle's fp64 matrix.  No device is needed here.

The ladders.  A 16-symbol table with a zero diagonal and insert = delete = 2^1000; the query is BASE (every symbol
twice, 32 symbols); a column is BASE with the first a replaced by b.  The diagonal path costs 0 + ... + sub[a][b] + 0 +
... = sub[a][b] exactly (adding zeros changes nothing, subnormals included), and every path that leaves the diagonal
holds an insert and a delete: 2^1001 at least, above every cost of the table (all < 2^1000).  So D(BASE, column) =
sub[a][b] bit for bit, and the 240 free entries of the table are 240 doubles chosen at will: one wave of 64 columns
per ladder, every k = 1..64, so every chosen double is some call's k-th smallest and the row's final bound.  The `top`
ladder has a table of its own with insert = delete = 2^1023: a path off the diagonal costs fl(2^1024) = +inf there, so
one substitution is again exact for every finite cost up to the largest double, and a column with two substitutions of
2^1023-scale costs lies at +inf: the last two ranks of that ladder reach +inf through the bisection."""
import math
import sys

import numpy as np

import join_cases as jc
import join_f64_cases as jf
import join_knn_cases as kc
import join_knn_f64_cases as kf
import sedgpu

INF = math.inf
WAVE = kf.WAVE
AL16 = jf.AL16
BASE = AL16 * 2
MAX_DOUBLE = sys.float_info.max
Call = kc.Call


def dbl(key):
    """The double whose bit pattern is `key`."""
    return float(np.array([key], np.uint64).view(np.float64)[0])


def key_of(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


# ---- the ladders' doubles ----

def _fill(v, n, rng, exp_lo, exp_hi):
    """v, then random keys (biased exponent exp_lo..exp_hi, any fraction) up to n distinct values."""
    seen = {key_of(x) for x in v}
    assert len(seen) == len(v)
    while len(v) < n:
        key = (int(rng.integers(exp_lo, exp_hi + 1)) << 52) | int(rng.integers(1 << 52))
        if key not in seen:
            seen.add(key)
            v.append(dbl(key))
    return v


EXPONENT_BASES = (0b01010101010, 0b10101010101)  # biased exponents; with one bit flipped they stay below 2022 (2^999)


def exponent_values():
    """Powers of two from the smallest subnormal to 2^999; two biased exponents and each with one of its 11 bits
    flipped (pairs that differ in a single exponent bit); 0; all-ones fractions beside powers of two (2 and the double
    below it differ in every bit 62..0); random keys over the whole exponent range."""
    v = [0.0] + [2.0 ** e for e in (-1074, -1073, -1060, -1023, -1022, -500, 0, 1, 500, 999)]
    for e0 in EXPONENT_BASES:
        v += [dbl(e << 52) for e in [e0] + [e0 ^ (1 << j) for j in range(11)]]
    v += [dbl(k) for k in (3, 0x000FFFFFFFFFFFFF, 0x3FEFFFFFFFFFFFFF, 0x3FF0000000000001, 0x3FFFFFFFFFFFFFFF,
                           0x7E5FFFFFFFFFFFFF, 0x7E6FFFFFFFFFFFFF)]
    return _fill(v, WAVE, np.random.default_rng(1074), 0, 2021)


def fraction_pairs(ts, exp_of, seed):
    """Per t a random key (biased exponent exp_of(t), so no two pairs interleave) and the key with fraction bit t
    flipped: [(t, key, key ^ 1 << t)]."""
    rng = np.random.default_rng(seed)
    out = []
    for t in ts:
        key = (exp_of(t) << 52) | int(rng.integers(1 << 52))
        out.append((t, key, key ^ (1 << t)))
    return out


def fraction_low_pairs():
    return fraction_pairs(range(32), lambda t: 63 * t, 31)  # (t = 0: a pair of subnormals)


def fraction_high_pairs():
    return fraction_pairs(range(32, 52), lambda t: 40 + 97 * (t - 32), 51)


WORD_EDGE_HIGH = (0x3FF12345, 0x00012345, 0x7E5ABCDE, 0x000FFFFF)  # (the last: H + 1 is the smallest normal's)


def word_edge_keys():
    """Around the seam of a key's two 32-bit words, for high words that are not trivial: low word 0, 0x7FFFFFFF,
    0x80000000 (bit 31 alone), 0xFFFFFFFF, then the next high word with low words 0 and 0x80000000.  As (low, high) pairs
    they order otherwise than as keys."""
    out = []
    for h in WORD_EDGE_HIGH:
        out += [h << 32, h << 32 | 0x7FFFFFFF, h << 32 | 0x80000000, h << 32 | 0xFFFFFFFF, (h + 1) << 32,
                (h + 1) << 32 | 0x80000000]
    return out


def fraction_low_values():
    return [dbl(k) for _, a, b in fraction_low_pairs() for k in (a, b)]


def fraction_high_values():
    v = [dbl(k) for _, a, b in fraction_high_pairs() for k in (a, b)] + [dbl(k) for k in word_edge_keys()]
    assert len(v) == WAVE and len({key_of(x) for x in v}) == WAVE
    return v


TOP_PAIRS = ((0, 1), (0, 2))  # the `top` ladder's two columns at +inf: the entries whose costs each one adds


def top_values():
    """62 finite costs up to the largest double (a table with insert = delete = 2^1023 holds them exactly): the first
    three are 2^1023-scale, and any two of them sum to +inf."""
    v = [MAX_DOUBLE, 2.0 ** 1023, dbl(0x7FDFFFFFFFFFFFFF), 2.0 ** 1022, 2.0 ** 1001, 2.0 ** 1000, 1.0, 5e-324, 0.0,
         dbl(0x7FE0000080000000), dbl(0x7FE00000FFFFFFFF), dbl(0x7FE0000100000000), dbl(0x7FEFFFFF80000000)]
    return _fill(v, WAVE - len(TOP_PAIRS), np.random.default_rng(1023), 2022, 2046)


# ---- a ladder's table and columns ----

def entry(i):
    """The i-th free entry of a 16 x 16 table, i = 0..239: (a, b), a != b, consecutive entries in different rows."""
    a = i % 16
    return AL16[a], AL16[(a + 1 + i // 16) % 16]


def ladder_table(values, indel):
    """The table whose i-th free entry is values[i] (1 where none is given), zero diagonal, insert = delete = indel."""
    assert len(values) <= 240
    upd = {a: {b: (0.0 if a == b else 1.0) for b in AL16} for a in AL16}
    for i, v in enumerate(values):
        a, b = entry(i)
        upd[a][b] = float(v)
    return {"insert": indel, "delete": indel, "update": upd}


def column(*entries):
    """BASE with, per entry, the first a replaced by b (entries of different rows: different places)."""
    s = list(BASE)
    assert len({entry(i)[0] for i in entries}) == len(entries)
    for i in entries:
        a, b = entry(i)
        s[BASE.index(a)] = b
    return "".join(s)


WIDE = ("exponents", "fraction low", "fraction high")  # the ladders of the 2^1000 table, 64 entries each, in this order


def wide_values():
    return exponent_values() + fraction_low_values() + fraction_high_values()


def ladder(name):
    """(the table, the columns in a shuffled order, the double each column lies at from BASE)."""
    if name == "top":
        v = top_values()
        table = ladder_table(v, 2.0 ** 1023)
        cols = [column(i) for i in range(len(v))] + [column(i, j) for i, j in TOP_PAIRS]
        want = v + [INF] * len(TOP_PAIRS)
    else:
        table = ladder_table(wide_values(), 2.0 ** 1000)
        parts = ("fraction high", "exponents") if name == "two waves" else (name,)
        at = [WAVE * WIDE.index(p) + i for p in parts for i in range(WAVE)]
        cols, want = [column(i) for i in at], [wide_values()[i] for i in at]
    order = np.concatenate([w + np.random.default_rng(len(name)).permutation(WAVE) for w in range(0, len(cols), WAVE)])
    return table, [cols[i] for i in order], [want[i] for i in order]


LADDERS = WIDE + ("top", "two waves")


# ---- the other sets ----

def code15_set(seed=1615, count=300):
    """Sequences of 20..32 symbols over all 16 symbols with near-duplicates; one in four has 32 symbols with the 16th
    symbol (code 15) first and last, the first sequence among them."""
    rng = np.random.default_rng(seed)
    ends = lambda: "X" + jc.random_seq(rng, AL16, 30) + "X"
    seqs = [ends()]
    while len(seqs) < count:
        s = ends() if rng.random() < 0.25 else jc.random_seq(rng, AL16, int(rng.integers(20, 33)))
        seqs.append(s)
        if rng.random() < 0.3 and len(seqs) < count:
            p = int(rng.integers(len(s)))
            seqs.append(s[:p] + jc.random_seq(rng, AL16, 1) + s[p + 1:])
    return seqs


def fold8(s):
    """What a kernel that masked codes with 0x07 would read: symbols 8..15 as 0..7."""
    return "".join(AL16[AL16.index(c) & 7] for c in s)


def same_length_set(seed=130, count=130, bases=6):
    """`count` sequences of 28 symbols, each one of a few bases with 0..3 substitutions: duplicates and near
    neighbours, and the index's order is the list's (three waves of 64, 64 and 2 columns)."""
    rng = np.random.default_rng(seed)
    base = [jc.random_seq(rng, AL16, 28) for _ in range(bases)]
    seqs = []
    for _ in range(count):
        s = list(base[int(rng.integers(bases))])
        for _ in range(int(rng.integers(0, 4))):
            s[int(rng.integers(28))] = AL16[int(rng.integers(16))]
        seqs.append("".join(s))
    return seqs


class Set(kc.EnvelopeSet):
    """join_knn_cases.EnvelopeSet (no scale on this route: S = 1) with the plan's lower-bound table."""

    def __init__(self, table, alphabet, cols, queries=None):
        super().__init__(jc.plan_for(table, alphabet), 1, cols, queries)
        self.low = kf.lower_table(self.plan)


def _make_set(what, arg=None):
    if what == "ladder":
        table, cols, _ = ladder(arg)
        return Set(table, AL16, cols, [BASE])
    r16 = jf.random16_table()[0]
    if what == "columns":
        return Set(r16, AL16, code15_set())
    if what == "folded":  # the columns set as a kernel that masked codes with 0x07 would see it
        return Set(r16, AL16, [fold8(s) for s in code15_set()])
    if what == "same length":
        return Set(r16, AL16, same_length_set())
    if what == "rows":  # lengths 0..32 under insert != delete: the length skip works launch by launch
        return Set(r16, AL16, jc.mixed_set(1604, AL16, 140))
    if what == "ties":
        return Set(jc.load_golden("costs.json"), "ACGUN", kc.tie_set()[0])
    if what == "cross":  # the table and alphabet both routes serve
        return Set(jc.load_golden("user_costs.json"), "ACGUN", kc.random_set())
    raise KeyError(what)


_SETS = {}  # computed once, shared, never changed


def envelope_set(name):
    if name not in _SETS:
        _SETS[name] = _make_set(*name)
    return _SETS[name]


# ---- the envelope's calls ----

COLUMN_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
LAUNCH_ROWS = (1, 3, 4, 5)  # SED_OPT_JOIN_ROWS: launches of part of a row group, of one, and of one and a ragged second
ROW_RANGES = ((1, 2), (3, 9), (5, 6), (139, 140))
QUERY_COUNTS = (1, 4, 5, 9)
CUTOFF_NOTES = ("at d", "below d", "above d", "tiny", "zero", "minus zero", "largest")
REFUSED_K = (65, 129)  # k = 65 and k = the 129 columns in scope of the 130-column set: outside 1..64


def kth_distance(D, k, self_col=None):
    """The k-th smallest of one row of the oracle's matrix, its own column left out."""
    v = np.delete(D, self_col) if self_col is not None else np.asarray(D)
    return float(np.sort(v)[k - 1])


def cutoffs_at(d):
    return list(zip(CUTOFF_NOTES, (d, float(np.nextafter(d, 0.0)), float(np.nextafter(d, INF)), 5e-324, 0.0, -0.0, MAX_DOUBLE)))


def word_edge_rank():
    """k for which the `fraction high` ladder's k-th distance is 0x3FF12345_80000000: the low word's bit 31 alone."""
    v = sorted(key_of(x) for x in fraction_high_values())
    return v.index(WORD_EDGE_HIGH[0] << 32 | 0x80000000) + 1


def _build_calls():
    out = []
    add = lambda *a, **kw: out.append(Call(*a, **kw))
    rows_opt = lambda step: ((sedgpu.SED_OPT_JOIN_ROWS, step),)
    # 1. ladders: one query, every k
    for name in LADDERS:
        for k in range(1, WAVE + 1):
            add("ladders", name, ("ladder", name), k, queries=[0])
    # 2. column counts on and beside the wave and the block, the 16th symbol in rows and columns
    for N in COLUMN_COUNTS:
        for k in (1, 2, 8):
            add("columns", N, ("columns",) * 2, k, ncols=N)
            add("columns", N, ("columns",) * 2, k, ncols=N, queries=sorted({3 % N, 0, N - 1, 299}))
    # 3. k against the lanes in scope: 130 columns of one length, waves of 64, 64 and 2
    s = ("same length",) * 2
    for k in (1, 2, 63, 64):
        add("k", "whole", s, k)
        add("k", "whole", s, k, queries=[0, 64, 129])
        for rows in ((5, 6), (129, 130)):  # the row's own column in the first wave, in the last
            add("k", "one row", s, k, rows=rows)
        add("k", "none", s, k, ncols=127)
    add("k", "none", s, 64, ncols=127, rows=(0, 64), note="none")  # waves of 64 and 63: neither has 64 in scope for a row of the first
    # 4. row ranges off the multiples of the row group, under forced launch rows
    s = ("rows",) * 2
    cap = float(np.median([kth_distance(envelope_set(s).D[r], 3, r) for r in range(140)]))
    for step in LAUNCH_ROWS:
        for k, T in ((2, INF), (3, cap)):
            for rows in ROW_RANGES:
                add("rows", "self", s, k, T, rows=rows, options=rows_opt(step))
            for n in QUERY_COUNTS:
                add("rows", "search", s, k, T, queries=list(range(n)), options=rows_opt(step))
    # 5. cutoffs on and beside a k-th distance: adjacent bit patterns
    for name, k in (("fraction high", word_edge_rank()), ("exponents", 8)):
        s = ("ladder", name)
        for note, T in cutoffs_at(kth_distance(envelope_set(s).Dq[0], k)):
            add("cutoffs", name, s, k, T, queries=[0], note=note)
    add("cutoffs", "top", ("ladder", "top"), WAVE, MAX_DOUBLE, queries=[0], note="largest")
    s = ("same length",) * 2
    D = envelope_set(s).D
    r = next(r for r in range(len(D)) if (np.delete(D[r], r) == 0).sum() >= 2)  # a row with duplicates
    for note, T in cutoffs_at(kth_distance(D[r], 8, r)):
        add("cutoffs", "same length", s, 8, T, rows=(r, r + 1), note=note)
    # 6. the overflow rerun across launches
    add("rerun", None, ("ties",) * 2, 1, rows=(0, 4), options=rows_opt(5), note="small")
    add("rerun", None, ("ties",) * 2, 1, options=rows_opt(5), note="grows")
    # 7. both routes on a table both serve
    add("cross", None, ("cross",) * 2, 8)
    return out


_CALLS = []


def envelope_calls(group=None, case=None):
    """Every call of the GPU envelope tests, in the order they are made (those of one group and case)."""
    if not _CALLS:
        _CALLS.extend(_build_calls())
    return [c for c in _CALLS if (group is None or c.group == group) and (case is None or c.case == case)]


def call_inputs(call):
    return kc.call_inputs(call, envelope_set)


def model_inputs(call):
    """bound_pass_model's arguments up to T."""
    s, cols, rows, D, self_join, lo = call_inputs(call)
    return D, kc.in_scope(D.shape, self_join, lo), [len(x) for x in rows], [len(x) for x in cols], s.low, call.k, call.T


_MODELS = {}


def call_model(call, order="sequential"):
    """(the final bounds, the pairs pass 1 ran) of the call under `order`, computed once."""
    key = call.key() + (order,)
    if key not in _MODELS:
        _MODELS[key] = kf.bound_pass_model(*model_inputs(call), order)
    return _MODELS[key]


def call_emit(call):
    """emit_pass_model on the bounds of call_model: (the candidates' mask, the pairs pass 2 runs, the (wave, row) left out)."""
    D, ok, len_rows, len_cols, low, _, _ = model_inputs(call)
    return kf.emit_pass_model(D, ok, len_rows, len_cols, low, call_model(call)[0])


def call_expected(call):
    _, _, _, D, self_join, lo = call_inputs(call)
    return kf.expected_knn(D, call.k, call.T, self_join, lo)


def launches(call):
    """The launches one pass of the call makes under its forced launch rows."""
    step = dict(call.options).get(sedgpu.SED_OPT_JOIN_ROWS, 0)
    nrows = len(call_inputs(call)[2])
    return -(-nrows // step) if step else 1
