"""The key-range envelope of the integer and lane kernels as data, shared by the CPU tests (tests/test_key_envelope.py)
and the GPU tests (tests/test_gpu_key_envelope.py, test_fuzz_gpu.py::test_route_fuzz_drawn_tables).  A handful of
inequalities in csrc/sed_plan.cpp decide which key format a batch gets and whether it stays off fp64:

  i32_fits      npad delete + cols insert <= 65533 and npad + cols < 16384, npad = n rounded up to 64 R,
                cols = max(m + 64 + 64 / R, 32);
  i32_eligible  1 <= mismatch <= insert + delete <= 255;
  x2_costs_ok   every mismatch < insert + delete (the 16-bit halves);
  scaled_costs  512 delete S + 33 insert S <= 65533, (insert + delete) S <= 255, K <= 8.

The tables here sit on them: the steepest delete the lane block takes, insert + delete = 255 three ways, both i32_fits
limits at once, and on the scaled grid the last accepted and the first refused (insert, delete).  `fits` restates
i32_fits and `border` derives from it the last str2 length that fits and the first that does not, so tests run the two
side by side.  Everything is seeded and device-free."""
import numpy as np

from band_cases import TABLES as BAND_TABLES, _table, mut

S = "ACGU"
S8 = "ACGUYRWS"  # the scaled tables' alphabets are its first K symbols


# ---- integer tables: ACGU, every one i32_eligible ----
def _int_table(seed, ins, dele, variant):
    """Mismatches uniform in 1 .. insert + delete - 1 from a fixed seed, with 1 and insert + delete - 1 forced in (`lt`:
    the 16-bit halves may pack); `eq`: the same draw with one mismatch at insert + delete (no packing, and the update
    ties insert + delete wherever those two symbols meet)."""
    hi = ins + dele - 1
    sub = np.random.default_rng(seed).integers(1, hi + 1, size=(4, 4))
    sub[0, 1], sub[1, 0] = 1, hi
    if variant == "eq":
        sub[2, 3] = ins + dele
    np.fill_diagonal(sub, 0)
    return _table(ins, dele, sub.tolist())


# name: (insert, delete).  i1_d127: the steepest delete whose 512-row lane block fits (512 x 127 = 65024, against 65536
# at delete 128); i1_d254, i254_d1, i127_d128: insert + delete = 255 with rows dominating, columns dominating, neither;
# i4_d4 (mismatches to 8): both i32_fits limits at once, 4 (8192 + 8191) = 65532.
INT_BASES = {"i1_d127": (1, 127), "i1_d254": (1, 254), "i254_d1": (254, 1), "i127_d128": (127, 128), "i4_d4": (4, 4)}
VARIANTS = ("lt", "eq")
INT_TABLES = {"%s/%s" % (base, v): _int_table(11 + k, ins, dele, v)
              for k, (base, (ins, dele)) in enumerate(INT_BASES.items()) for v in VARIANTS}
INT_NAMES = tuple(INT_TABLES)
TABLES = dict(INT_TABLES)
TABLES["user_costs.json"] = BAND_TABLES["user_costs.json"]


def packs(name):
    """Whether x2_costs_ok lets the table's distance-only pairs run two per lane or wave."""
    sub, ins, dele = costs(name)
    return bool((sub[~np.eye(4, dtype=bool)] < ins + dele).all())


def costs(name):
    """(sub 4 x 4, insert, delete) of an integer table."""
    t = TABLES[name]
    sub = np.array([[0.0 if a == b else t["update"][a][b] for b in S] for a in S])
    return sub, float(t["insert"]), float(t["delete"])


# ---- scaled tables: dyadic and fp64 (K = 5..8 symbols, or a scale S >= 2), distance-only lane pairs ----
def _scaled_table(seed, ins, dele, scale, K):
    """insert / S and delete / S over the first K symbols of S8; scaled mismatches uniform in 1 .. insert + delete with
    1 (the smallest above a match) and insert + delete forced in.  Insert and delete are not 1.0, so no symbol lies in a
    unit-cost subset (sed_plan.cpp: unit_subset) and no pair runs bit-parallel."""
    sub = np.random.default_rng(seed).integers(1, ins + dele + 1, size=(K, K))
    sub[0, 1], sub[1, 0], sub[K - 1, 0] = 1, ins + dele, ins + dele
    al = S8[:K]
    return {"insert": ins / scale, "delete": dele / scale,
            "update": {a: {b: float(sub[i][j]) / scale for j, b in enumerate(al) if b != a} for i, a in enumerate(al)}}


# name: (scaled insert, scaled delete, S, K, accepted).  (15, 127): 512 x 127 + 33 x 15 = 65519 is accepted; (16, 127):
# 65552 is refused and must run the fp64 lane kernel; (254, 1): (insert + delete) S = 255.
SCALED_BASES = {"s15_d127_k8": (15, 127, 1, 8, True), "s15_d127_s8_k5": (15, 127, 8, 5, True),
                "s16_d127_k8": (16, 127, 1, 8, False), "s16_d127_s8_k5": (16, 127, 8, 5, False),
                "s254_d1_k8": (254, 1, 1, 8, True)}
SCALED_TABLES = {name: _scaled_table(31 + k, ins, dele, scale, K)
                 for k, (name, (ins, dele, scale, K, _)) in enumerate(SCALED_BASES.items())}
SCALED_NAMES = tuple(SCALED_TABLES)


def scaled_alphabet(name):
    return S8[:SCALED_BASES[name][3]]


def scaled_sub(name):
    """The K x K costs of a scaled table (matches 0)."""
    al, t = scaled_alphabet(name), SCALED_TABLES[name]
    return np.array([[0.0 if a == b else t["update"][a][b] for b in al] for a in al])


# ---- the i32_fits inequality ----
def auto_R(max_n):
    """The rows per lane an integer batch gets from its longest str1 (sed_plan.cpp: choose_R)."""
    want = 1
    while want < max(1, (max_n + 63) // 64):
        want *= 2
    return min(16, max(4, want))


def _npad(n, R):
    return (n + 64 * R - 1) // (64 * R) * (64 * R)


def _indel(name):
    return costs(name)[1:] if isinstance(name, str) else name


def fits(name, n, m, R):
    """i32_fits for one pair (n, m) of a batch at R rows per lane; name: a table of TABLES, or (insert, delete)."""
    ins, dele = _indel(name)
    npad, cols = _npad(n, R), max(m + 64 + 64 // R, 32)
    return npad * dele + cols * ins <= 65533 and npad + cols < 16384


def border(name, n, R):
    """(the largest m >= 1 that fits for n and R, that m + 1), or None when no m does: cols = m + 64 + 64 / R is bounded
    by (65533 - npad delete) / insert and by 16383 - npad."""
    ins, dele = _indel(name)
    npad = _npad(n, R)
    cols = min(int((65533 - npad * dele) // ins), 16383 - npad)
    m = cols - 64 - 64 // R
    if m < 1:
        return None
    assert fits(name, n, m, R) and not fits(name, n, m + 1, R)
    return m, m + 1


def lane_max_n(name):
    """The largest n <= 512 whose lane pairs (m <= 32) fit at the R their batch gets when n is its longest str1."""
    return max(n for n in range(1, 513) if fits(name, n, 32, auto_R(n)))


def split_shape(name, R):
    """The largest multi-stripe shape that fits at R: the most full stripes k >= 2 with a border, and that border's m."""
    k = 2
    if border(name, k * 64 * R, R) is None:
        return None
    while border(name, (k + 1) * 64 * R, R) is not None:
        k += 1
    return k * 64 * R, border(name, k * 64 * R, R)[0]


# ---- sequence builders: lists of uint8 code arrays ----
def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def max_pair(sub, n, m):
    """One symbol against another whose mismatch is the table's largest."""
    off = np.where(np.eye(len(sub), dtype=bool), -1.0, sub)
    x, y = np.unravel_index(int(off.argmax()), off.shape)
    return _u8(np.full(n, x)), _u8(np.full(m, y))


def mutated_pair(rng, n, m, K=4):
    a = rng.integers(0, K, size=n)
    return _u8(a), mut(rng, np.resize(a, m))


KINDS = ("max", "identical", "mutated", "random", "shifted", "acca")


def pairs(sub, rng, n, m, K=4, kinds=KINDS):
    """The pairs of one shape: max-distance, identical (str2 = str1 resized to m), 10 % mutated, random, a shifted copy,
    (AC)^k against (CA)^k."""
    a = rng.integers(0, K, size=n)
    out = {"max": max_pair(sub, n, m),
           "identical": (a, np.resize(a, m)),
           "mutated": (a, np.where(rng.random(m) < 0.1, rng.integers(0, K, size=m), np.resize(a, m))),
           "random": (a, rng.integers(0, K, size=m)),
           "shifted": (a, np.resize(np.roll(a, -3), m)),
           "acca": (np.resize([0, 1], n), np.resize([1, 0], m))}
    return [_u8(out[k][0]) for k in kinds], [_u8(out[k][1]) for k in kinds]


def seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(map(str, parts))))


# ---- the cases of tests/test_gpu_key_envelope.py, device-free so that tests/test_key_envelope.py can place them ----
LANE_M = (1, 16, 17, 31, 32)
BIG = 2_000_000  # shapes past this many cells run the max-distance and the mutated pair only


def lane_n(name):
    return (1, 16, 17, 255, 256, lane_max_n(name))


def lane_block(name, sub=None, K=4, nmax=None):
    """Every builder at every lane shape of a table: n in {1, 16, 17, 255, 256, the largest that fits}, m in LANE_M."""
    sub = costs(name)[0] if sub is None else sub
    ns = lane_n(name) if nmax is None else (1, 16, 17, 255, 256, nmax)
    rng = np.random.default_rng(seed("lane", name))
    A, B = [], []
    for n in sorted(set(ns)):
        for m in LANE_M:
            a, b = pairs(sub, rng, n, m, K)
            A, B = A + a, B + b
    return A, B


def border_ns(name, R):
    """n in {1, 64 R, 64 R + 1} while some m fits."""
    return [n for n in (1, 64 * R, 64 * R + 1) if border(name, n, R) is not None]


def border_batch(name, R, n):
    """(A, B) at the last m that fits, and one pair (a, b) at the first that does not."""
    m0, m1 = border(name, n, R)
    sub = costs(name)[0]
    rng = np.random.default_rng(seed("border", name, R, n))
    A, B = pairs(sub, rng, n, m0, kinds=KINDS if n * m0 <= BIG else ("max", "mutated"))
    a, b = mutated_pair(rng, n, m1)
    return A, B, a, b


L_SHAPES = ((8192, 8123), (8192, 8124), (15360, 955), (1, 16251))


def l_batch(name, n, m):
    """One max-distance and one mutated pair of a shape of the L-limit cases."""
    a, b = max_pair(costs(name)[0], n, m)
    a2, b2 = mutated_pair(np.random.default_rng(seed("L", name, n, m)), n, m)
    return [a, a2], [b, b2]


def chain_batch(name, R):
    """Single-stripe pairs for CHAIN: n in {1, 17, 64 R - 1, 64 R} against m in {1, 33, 64, 65} with every builder, and
    against the last m that fits with the max-distance and the mutated pair."""
    sub = costs(name)[0]
    rng = np.random.default_rng(seed("chain", name, R))
    A, B = [], []
    if border(name, 64 * R, R) is None:  # (one stripe's padded rows alone pass the D field: no pair fits at this R)
        return A, B
    for n in (1, 17, 64 * R - 1, 64 * R):
        m0 = border(name, n, R)[0]
        for m in (1, 33, 64, 65):
            if m <= m0:
                a, b = pairs(sub, rng, n, m)
                A, B = A + a, B + b
        a, b = pairs(sub, rng, n, m0, kinds=("max", "mutated"))
        A, B = A + a, B + b
    return A, B


# ---- cases: one batch under one set of options, with the route it must take ----
class Case:
    """table: a name of TABLES or SCALED_TABLES; flags as Batch takes them (script, no_len); opts: {SED_OPT_*: value};
    expect: {a field of sedgpu.PLAN_ROUTE_FIELDS: its value, or a predicate of it}; ref: the key under which the batch's
    oracle results may be shared (same table, same pairs)."""

    def __init__(self, label, table, A, B, script, no_len, opts, expect, ref=None):
        self.label, self.name, self.A, self.B, self.script, self.no_len = label, table, A, B, script, no_len
        self.opts, self.expect, self.ref = dict(opts), dict(expect), ref or label
        self.alphabet = scaled_alphabet(table) if table in SCALED_TABLES else S
        self.table = SCALED_TABLES[table] if table in SCALED_TABLES else TABLES[table]

    @property
    def flags(self):
        return 1 if self.script else (4 if self.no_len else 0)  # SED_WANT_SCRIPT, SED_NO_LEN

    def shape(self):
        return "%d pairs, n <= %d, m <= %d" % (len(self.A), max(map(len, self.A)), max(map(len, self.B)))


def misses(expect, got):
    """The expected fields `got` ({field: number}) does not meet."""
    return {k: (got[k], "expected" if callable(v) else v) for k, v in expect.items()
            if not (v(got[k]) if callable(v) else got[k] == v)}


def _positive(v):
    return v > 0


FLAGSETS = (("script", True, False), ("dist+len", False, False), ("dist", False, True))
I32, F64 = 1, 2  # sed.h: SED_MODE_I32, SED_MODE_F64 (every table here has simple typing)
O_R, O_SPLIT, O_LANE, O_CHAIN, O_PACK, O_TB, O_DOT, O_BITPAR, O_SCALED = 2, 3, 4, 5, 6, 7, 10, 11, 12  # SED_OPT_*


def lane_cases(name):
    """Block 1: the lane block under script, distance + length, distance only and distance only unpacked, on the lane
    kernels and (SED_OPT_LANE = 2) on the wave kernels.  SPLIT is off: a batch of <= 256 pairs past 256 rows would
    take it."""
    A, B = lane_block(name)
    out = []
    for lane in (0, 2):
        for what, script, no_len in FLAGSETS + (("dist, pack off", False, True),):
            pack = 2 if what.endswith("off") else 0
            exp = {"mode": I32, "lane_pairs": 0 if lane else len(A), "traceback_mode": 1 if script else 0,
                   "chains": 0, "split_tasks": 0}
            if what == "dist" and packs(name):
                exp["packed_pairs"] = _positive if lane else len(A)
            else:
                exp["packed_pairs"] = 0
            out.append(Case("lane %s, %s, lane=%d" % (name, what, lane), name, A, B, script, no_len,
                            {O_SPLIT: 2, O_LANE: lane, O_PACK: pack}, exp, ref="lane " + name))
    return out


def border_cases(name, R, n):
    """Block 2: wave kernels at a forced R, a batch at the last m that fits (integer) and the same batch with one pair
    at the first that does not (fp64)."""
    A, B, a, b = border_batch(name, R, n)
    opts = {O_R: R, O_SPLIT: 2, O_LANE: 2, O_CHAIN: 2}
    tag = "border %s R=%d n=%d m=%d" % (name, R, n, len(B[0]))
    base = {"mode": I32, "rows_per_lane": R, "lane_pairs": 0, "chains": 0, "split_tasks": 0, "packed_pairs": 0}
    out = [Case(tag + ", script tb=1", name, A, B, True, False, {**opts, O_TB: 1}, {**base, "traceback_mode": 1}, tag),
           Case(tag + ", script tb=2", name, A, B, True, False, {**opts, O_TB: 2}, {**base, "traceback_mode": 2}, tag),
           Case(tag + ", dist+len", name, A, B, False, False, opts, {**base, "traceback_mode": 0}, tag)]
    # distance only: the batch's pairs share n and m, so they pack two per wave where the table allows it; a partner
    # of two thirds the columns (3 m' > m) still does
    rng = np.random.default_rng(seed("partner", name, R, n))
    m2 = max(1, 2 * len(B[0]) // 3 + 1)
    a2, b2 = mutated_pair(rng, n, m2)
    packed = (lambda v: v >= 2) if packs(name) else 0
    out.append(Case(tag + ", dist", name, A, B, False, True, opts, {**base, "packed_pairs": packed}, tag))
    out.append(Case(tag + ", dist with partner", name, A[:1] + [a2], B[:1] + [b2], False, True, opts,
                    {**base, "packed_pairs": packed}))
    past = "border %s R=%d n=%d m=%d" % (name, R, n, len(b))
    out.append(Case(past + ", script", name, A + [a], B + [b], True, False, opts, {"mode": F64, "lane_pairs": 0}, past))
    out.append(Case(past + ", dist", name, A + [a], B + [b], False, True, opts, {"mode": F64, "lane_pairs": 0}, past))
    return out


L_TABLES = ("i4_d4/lt", "i4_d4/eq", "user_costs.json")


def l_cases(name):
    """Block 3: the L limit at the automatic R.  Each shape is a batch of its own (one pair that does not fit takes
    its whole batch to fp64); its mode is what `fits` says at the R the planner derives from n.  (1, 16251) does not
    fit: a single row still pads to 64 R rows, 256 at the R = 4 such a batch gets, so the last m that fits is
    border(name, 1, 4)[0] = 16047, which runs beside it."""
    out = []
    for n, m in L_SHAPES + ((1, border(name, 1, auto_R(1))[0]),):
        A, B = l_batch(name, n, m)
        exp = {"mode": I32 if fits(name, n, m, auto_R(n)) else F64, "lane_pairs": 0}
        tag = "L %s %d x %d" % (name, n, m)
        out.append(Case(tag + ", script", name, A, B, True, False, {}, exp, tag))
        out.append(Case(tag + ", dist", name, A, B, False, True, {}, exp, tag))
        # two long pairs go SPLIT at R = 4 (checkpoints, no L field); with SPLIT off they run the stripe kernel at the
        # automatic R with per-cell codes: the ladder keys whose L field runs into the D field by design
        stripe = dict(exp, split_tasks=0, chains=0)
        if exp["mode"] == I32:
            stripe.update(rows_per_lane=auto_R(n), traceback_mode=1)
        out.append(Case(tag + ", script, SPLIT off", name, A, B, True, False, {O_SPLIT: 2}, stripe, tag))
    return out


L_FITS = {(8192, 8123): True, (8192, 8124): False, (15360, 955): True, (1, 16251): False}

CHAIN_CASES = [(name, R) for name in INT_NAMES for R in (4, 8) if border(name, 64 * R, R) is not None]


def chain_cases(name, R):
    """Block 4: CHAIN forced, dynamic (1) and static chains of 3, on the wide-ladder dot keys where the table factors
    (SED_OPT_DOT 0), on the perm ladder (2) and on the 3-bit ladder's dot keys (3)."""
    A, B = chain_batch(name, R)
    out = []
    for chain in (1, 3):
        for dot in (0, 2, 3):
            opts = {O_R: R, O_CHAIN: chain, O_LANE: 2, O_SPLIT: 2, O_DOT: dot}
            exp = {"mode": I32, "rows_per_lane": R, "lane_pairs": 0, "chains": _positive, "split_tasks": 0,
                   "traceback_mode": 1}
            if dot == 2:
                exp["dot_keys"] = 0
            tag = "chain %s R=%d" % (name, R)
            out.append(Case("%s chain=%d dot=%d, script" % (tag, chain, dot), name, A, B, True, False, opts, exp, tag))
            if dot == 0:
                out.append(Case("%s chain=%d dot=0, dist+len" % (tag, chain), name, A, B, False, False, opts,
                                {**exp, "traceback_mode": 0}, tag))
    return out


SPLIT_CASES = [(name, R) for name in INT_NAMES for R in (4, 8, 16) if split_shape(name, R) is not None]


def split_cases(name, R):
    """Block 4: integer SPLIT forced on one mutated pair at the largest multi-stripe shape that fits."""
    n, m = split_shape(name, R)
    a, b = mutated_pair(np.random.default_rng(seed("split", name, R)), n, m)
    exp = {"mode": I32, "rows_per_lane": R, "lane_pairs": 0, "chains": 0, "split_tasks": n // (64 * R)}
    tag = "split %s R=%d %d x %d" % (name, R, n, m)
    return [Case(tag + ", script", name, [a], [b], True, False, {O_R: R, O_SPLIT: 1},
                 {**exp, "traceback_mode": 4 if R == 4 else 1}, tag),
            Case(tag + ", dist+len", name, [a], [b], False, False, {O_R: R, O_SPLIT: 1}, {**exp, "traceback_mode": 0}, tag)]


def scaled_cases(name):
    """Block 5: the lane shapes with n up to 512 under a scaled table, distance only: as planned, with the scaled
    kernel off and with the bit-parallel one off."""
    accepted = SCALED_BASES[name][4]
    A, B = lane_block(name, scaled_sub(name), SCALED_BASES[name][3], 512)
    out = []
    for what, opts in (("", {}), (", scaled off", {O_SCALED: 2}), (", bitpar off", {O_BITPAR: 2})):
        exp = {"mode": F64, "lane_pairs": len(A), "bitpar_pairs": 0,
               "scaled_pairs": len(A) if accepted and O_SCALED not in opts else 0}
        out.append(Case("scaled %s%s" % (name, what), name, A, B, False, True, {O_SPLIT: 2, **opts}, exp,
                        "scaled " + name))
    return out


def all_cases():
    for name in INT_NAMES:
        yield from lane_cases(name)
        for R in (4, 8, 16):
            for n in border_ns(name, R):
                yield from border_cases(name, R, n)
    for name in L_TABLES:
        yield from l_cases(name)
    for name, R in CHAIN_CASES:
        yield from chain_cases(name, R)
    for name, R in SPLIT_CASES:
        yield from split_cases(name, R)
    for name in SCALED_NAMES:
        yield from scaled_cases(name)
