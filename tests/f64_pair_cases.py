"""The alphabet and numeric envelope of the fp64 pair kernels as data, shared by the CPU tests
(tests/test_f64_pair_cases.py) and the GPU tests (tests/test_gpu_f64_pair_envelope.py).  csrc/sed_f64.hip and
csrc/sed_lane.hip promise every alphabet of 1 .. SED_MAX_K = 32 symbols and every finite double; the tables here sit on
what that takes:

  k17, k31, k32   one past a 4-bit code, an odd stride, the full LDS table (`a * K + b` into SED_MAX_K^2 entries): the
                  15 IUPAC letters, their lowercase forms, X and -; 962 non-dyadic mismatches, none symmetric, and the
                  planner's int 0 for the 30 case-folded entries off the diagonal;
  k32_typed       the same with Python ints among the costs: the table's typing plane (e.y) is live;
  k32_unit_high   the unit-cost subset is the last four codes: the mask's bit 31, unit_code's shift by 31 (lane only);
  near_tie        0.1, 0.2, 0.3 and 0.1 + 0.2: sums equal in exact arithmetic sit 1 ulp apart or tie;
  huge            k32 times 1e308: values reach +inf, the script is decided by the L keys alone;
  huge_mixed      +-1e308 and +-0.5: typed, values reach both infinities, never NaN;
  subnormal       multiples of 2^-1074: every stored double has a zero high word;
  n_first         costs.json's ACGU and N with N as code 0: the unit-cost subset starts at code 1 (lane only).

`sweep` makes every entry of a K-table live; `shapes` are random pairs, half of them related, at the smallest sizes that
cross each kernel's seams.  A Case is one batch under one set of options with the route it must take.  Everything is
seeded and device-free."""
import itertools
import math

import numpy as np

from key_cases import O_BITPAR, O_LANE, O_R, O_SCALED, O_SPLIT, misses, seed  # noqa: F401  (misses: for the tests)

O_MODE, O_SEG = 1, 13  # SED_OPT_MODE, SED_OPT_SEG
F64, TYPED = 2, 3      # sed.h: SED_MODE_F64 (simple typing), SED_MODE_F64_TYPED

SYMS32 = "AGCUYRWSKMDVHBN" + "agcuyrwskmdvhbn" + "X-"
SYMS6 = "ACGUYR"
assert len(set(SYMS32)) == 32


def _folds(a, b):
    return a.lower() == b.lower()


def _entries(syms):
    """(a, b) of every mismatch entry in table order: the case-folded ones are the planner's int 0, never looked up."""
    return [(a, b) for a in syms for b in syms if not _folds(a, b)]


def _fill(syms, value):
    out = {a: {} for a in syms}
    for k, (a, b) in enumerate(_entries(syms)):
        out[a][b] = value(k, a, b)
    return out


# ---- the K-tables ----
_rng32 = np.random.default_rng(3232)
_K32 = _fill(SYMS32, lambda k, a, b: float(_rng32.uniform(0.55, 0.95)))


def _k_table(K, scale=1.0):
    syms = SYMS32[:K]
    return {"insert": 1.0 * scale, "delete": 1.1 * scale, "update": _fill(syms, lambda k, a, b: _K32[a][b] * scale)}


def _typed_table():
    """k32 with insert the int 2, delete 3.0 and every third mismatch the int 1 or 2."""
    return {"insert": 2, "delete": 3.0,
            "update": _fill(SYMS32, lambda k, a, b: 1 + (k // 3) % 2 if k % 3 == 0 else _K32[a][b])}


UNIT_FIRST = 28  # k32_unit_high: the codes from here on cost 1.0 among themselves


def _unit_high_table():
    """Every code below UNIT_FIRST costs 0.75 against every other symbol, both ways, so none of them has a unit-cost
    partner; the last four cost 1.0 among themselves."""
    at = {c: i for i, c in enumerate(SYMS32)}
    return {"insert": 1.0, "delete": 1.0,
            "update": _fill(SYMS32, lambda k, a, b: 1.0 if min(at[a], at[b]) >= UNIT_FIRST else 0.75)}


UNIT_HIGH_MASK = 0xF0000000

N_FIRST = "NACGU"


def _n_first_table():
    """costs.json's ACGU and N (every cost 1.0 but N's 0.75) with N as code 0: dyadic over 5 symbols, so the lane pairs
    with an N run the scaled-integer kernel and the others bit-parallel through its 2-bit map of the subset's codes."""
    return {"insert": 1.0, "delete": 1.0, "update": _fill(N_FIRST, lambda k, a, b: 0.75 if "N" in (a, b) else 1.0)}


N_FIRST_MASK = 0x1E

NEAR_VALUES = (0.3, 0.1 + 0.2, 0.1, 0.2, 0.6, 0.7)
assert NEAR_VALUES[0] != NEAR_VALUES[1]


def _near_tie_table():
    rng = np.random.default_rng(1020)
    t = _fill("ACGU", lambda k, a, b: NEAR_VALUES[int(rng.integers(0, len(NEAR_VALUES)))])
    t["A"]["C"], t["C"]["A"] = NEAR_VALUES[0], NEAR_VALUES[1]
    return {"insert": 0.1, "delete": 0.2, "update": t}


HUGE_MIXED_VALUES = (-1e308, 1e308, 0.5, -0.5)


def _huge_mixed_table():
    rng = np.random.default_rng(308)
    t = _fill(SYMS6, lambda k, a, b: HUGE_MIXED_VALUES[k % 4 if k < 4 else int(rng.integers(0, 4))])
    return {"insert": 1e308, "delete": 1e308, "update": t}


TINY = math.ldexp(1.0, -1074)  # the smallest subnormal


def _subnormal_table():
    rng = np.random.default_rng(1074)
    return {"insert": 3 * TINY, "delete": 5 * TINY,
            "update": _fill(SYMS6, lambda k, a, b: (k % 7 + 1 if k < 7 else int(rng.integers(1, 8))) * TINY)}


# name: (table, alphabet, the mode the planner must choose by itself)
TABLES = {
    "k17": (_k_table(17), SYMS32[:17], F64),
    "k31": (_k_table(31), SYMS32[:31], F64),
    "k32": (_k_table(32), SYMS32, F64),
    "k32_typed": (_typed_table(), SYMS32, TYPED),
    "k32_unit_high": (_unit_high_table(), SYMS32, F64),
    "near_tie": (_near_tie_table(), "ACGU", F64),
    "huge": (_k_table(32, 1e308), SYMS32, F64),
    "huge_mixed": (_huge_mixed_table(), SYMS6, TYPED),
    "subnormal": (_subnormal_table(), SYMS6, F64),
    "n_first": (_n_first_table(), N_FIRST, F64),
}
UNIT_LO = {"k32_unit_high": UNIT_FIRST, "n_first": 1}  # lane only: the unit-cost subset is the codes from here on
K_TABLES = ("k17", "k31", "k32", "k32_typed")   # their sweeps must make every entry live
SWEEP_TABLES = K_TABLES + ("huge", "k32_unit_high")  # every table of more than 16 symbols runs its sweep
WAVE_TABLES = tuple(n for n in TABLES if n not in UNIT_LO)
LANE_TABLES = tuple(n for n, (_, _, mode) in TABLES.items() if mode == F64)  # the lane kernel: simple typing only
FULL_TABLES = ("k32", "near_tie", "huge")


def table(name):
    return TABLES[name][0]


def alphabet(name):
    return TABLES[name][1]


# ---- pairs: lists of uint8 code arrays ----
def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def rand_pair(rng, K, n, m, related, lo=0):
    """Codes lo .. K - 1; related: str2 is str1 (resized to m) with one symbol in ten redrawn, as
    test_gpu_parity._random_pairs builds its related pairs."""
    a = rng.integers(lo, K, size=n)
    b = rng.integers(lo, K, size=m)
    if related:
        b = np.where(rng.random(m) < 0.1, b, np.resize(a, m))
    return _u8(a), _u8(b)


def sweep(name):
    """For each symbol a, (a * (K - 1), the K - 1 other symbols in table order), then the transposes: every mismatch
    entry is the only way to pay for its column, and every symbol stands as a row and as a column symbol."""
    K = len(alphabet(name))
    A = [_u8(np.full(K - 1, a)) for a in range(K)]
    B = [_u8([b for b in range(K) if b != a]) for a in range(K)]
    return A + B, B + A


def shapes(name, ns, ms, tag, per_shape=1, lo_half=None):
    """per_shape random pairs of every (n, m), every other shape's related.  lo_half: the first pair of every shape lies
    wholly in the codes from lo_half on (k32_unit_high's unit-cost subset)."""
    K = len(alphabet(name))
    rng = np.random.default_rng(seed("f64 shapes", name, tag))
    A, B = [], []
    for k, (n, m) in enumerate(itertools.product(ns, ms)):
        for q in range(per_shape):
            lo = lo_half if lo_half is not None and q == 0 else 0
            a, b = rand_pair(rng, K, n, m, related=k % 2 == 0, lo=lo)
            A.append(a)
            B.append(b)
    return A, B


def probe(name, count=20, size=40):
    """count pairs of size x size, half of them related: small enough for a DP written in Python."""
    K = len(alphabet(name))
    rng = np.random.default_rng(seed("f64 probe", name))
    got = [rand_pair(rng, K, size, size, related=i % 2 == 0) for i in range(count)]
    return [a for a, _ in got], [b for _, b in got]


def pad(name, count, tag):
    """count pairs of at most 12 x 12."""
    K = len(alphabet(name))
    rng = np.random.default_rng(seed("f64 pad", name, tag))
    got = [rand_pair(rng, K, int(rng.integers(1, 13)), int(rng.integers(1, 13)), related=i % 2 == 0)
           for i in range(count)]
    return [a for a, _ in got], [b for _, b in got]


def one_mismatch(name, n, tag):
    """A pair of n x n that differs in one symbol past the middle: under `huge` its sink is that one mismatch, finite
    and not 0, while the cells a few steps off the diagonal are +inf."""
    K = len(alphabet(name))
    rng = np.random.default_rng(seed("f64 one mismatch", name, tag))
    a = rng.integers(0, K, size=n)
    b = a.copy()
    at = 2 * n // 3
    b[at] = (a[at] + 1) % K
    assert not _folds(alphabet(name)[a[at]], alphabet(name)[b[at]])
    return _u8(a), _u8(b)


WAVE_M = (1, 63, 64, 65, 130)
SEG_M = (1, 15, 16, 17, 40)
SPLIT_M = (1, 63, 64, 65, 255, 256, 257)  # the ring of 256
LANE_N, LANE_M = (1, 2, 255, 512), (1, 31, 32)
SEG_PAIRS = 300


def wave_batch(name, R):
    """One wave per pair at R rows per lane: a stripe is 64 R rows, a chunk 64 columns.  n x WAVE_M, the sweep of the
    tables past 16 symbols, near_tie's 40 x 40 probe, and under `huge` one square pair of (64 R + 1)^2, whose m is not
    one of WAVE_M: the only way to a finite sink other than 0 past a stripe border under that table."""
    A, B = shapes(name, (1, 64 * R - 1, 64 * R, 64 * R + 1), WAVE_M, "wave %d" % R)
    if name in SWEEP_TABLES:
        a, b = sweep(name)
        A, B = A + a, B + b
    if name == "near_tie":
        a, b = probe(name)
        A, B = A + a, B + b
    if name == "huge":
        a, b = one_mismatch(name, 64 * R + 1, "wave %d" % R)  # (past WAVE_M: 257 or 513 columns, this table only)
        A, B = A + [a], B + [b]
    return A, B


def seg_batch(name, R):
    """16-lane segments: a stripe is 16 R rows, a chunk 16 columns; filled to SEG_PAIRS (past the 256 wave pairs the
    segments need)."""
    A, B = shapes(name, (1, 16 * R - 1, 16 * R, 16 * R + 1, 32 * R + 1), SEG_M, "seg %d" % R)
    if name in SWEEP_TABLES:
        a, b = sweep(name)
        A, B = A + a, B + b
    a, b = pad(name, SEG_PAIRS - len(A), "seg %d" % R)
    return A + a, B + b


def split_batch(name, R):
    """SPLIT: two and three stripes of 64 R rows, m around a chunk and around the ring of 256 steps; 14 pairs, and
    under `huge` one with a finite sink."""
    A, B = shapes(name, (64 * R + 1, 128 * R + 1), SPLIT_M, "split %d" % R)
    if name == "huge":
        a, b = one_mismatch(name, 64 * R + 1, "split %d" % R)
        A, B = A + [a], B + [b]
    return A, B


def lane_batch(name):
    """The lane kernel's block of 512 x 32, two pairs a shape; under k32_unit_high and n_first the first of the two lies
    wholly in the unit-cost subset."""
    A, B = shapes(name, LANE_N, LANE_M, "lane", per_shape=2, lo_half=UNIT_LO.get(name))
    if name in SWEEP_TABLES:
        a, b = sweep(name)
        A, B = A + a, B + b
    return A, B


def in_unit_subset(name, A, B):
    """The pairs of a batch under a table of UNIT_LO whose symbols all lie in its unit-cost subset."""
    return [p for p, (a, b) in enumerate(zip(A, B)) if min(int(a.min()), int(b.min())) >= UNIT_LO[name]]


FULL_SHAPES = {"one wave": (70, 70), "split": (300, 90)}


def full_pair(name, route):
    """The pair of a full-matrix case: 70 x 70 on the one-wave kernel (two chunks), 300 x 90 on SPLIT (two stripes at
    the R = 4 the full matrix runs)."""
    n, m = FULL_SHAPES[route]
    rng = np.random.default_rng(seed("f64 full", name, route))
    return rand_pair(rng, len(alphabet(name)), n, m, related=True)


# ---- cases ----
class Case:
    """name: a table of TABLES; flags as Batch takes them (script, no_len); mode: SED_OPT_MODE (0: the planner's own
    choice); opts: {SED_OPT_*: value}; expect: {a field of sedgpu.PLAN_ROUTE_FIELDS: its value}; ref: the key under
    which the batch's oracle results may be shared (same table, same pairs)."""

    def __init__(self, label, name, A, B, script, no_len, mode, opts, expect, ref):
        self.label, self.name, self.A, self.B, self.script, self.no_len = label, name, A, B, script, no_len
        self.mode, self.opts, self.expect, self.ref = mode, dict(opts), dict(expect), ref
        self.table, self.alphabet = table(name), alphabet(name)

    @property
    def flags(self):
        return 1 if self.script else (4 if self.no_len else 0)  # SED_WANT_SCRIPT, SED_NO_LEN

    @property
    def plan_opts(self):
        return {**self.opts, **({O_MODE: self.mode} if self.mode else {})}

    def shape(self):
        return "%d pairs, n <= %d, m <= %d" % (len(self.A), max(map(len, self.A)), max(map(len, self.B)))


FLAGSETS = (("script", True, False), ("dist+len", False, False), ("dist", False, True))


def modes(name):
    """(SED_OPT_MODE, the mode the batch must report): the planner's own choice, and for a simple-typing table the
    typed kernels forced as well."""
    own = TABLES[name][2]
    return ((0, own),) + (((3, TYPED),) if own == F64 else ())


def _wave_cases(kind, name, R, A, B, opts, route):
    out = []
    for mode, got in modes(name):
        for what, script, no_len in FLAGSETS:
            out.append(Case("%s %s R=%d, mode %d, %s" % (kind, name, R, mode, what), name, A, B, script, no_len, mode,
                            opts, {"mode": got, "rows_per_lane": R, "lane_pairs": 0, "bitpar_pairs": 0,
                                   "scaled_pairs": 0, **route}, "%s %s %d" % (kind, name, R)))
    return out


def wave_cases(name, R):
    """sed_wf_f64_kernel, SW = 64: SPLIT, the segments and the lane kernel off."""
    A, B = wave_batch(name, R)
    return _wave_cases("wave", name, R, A, B, {O_R: R, O_SPLIT: 2, O_LANE: 2, O_SEG: 2},
                       {"segment_pairs": 0, "split_tasks": 0})


def seg_cases(name, R):
    """sed_wf_f64_kernel, SW = 16: every pair in a segment."""
    A, B = seg_batch(name, R)
    return _wave_cases("seg", name, R, A, B, {O_R: R, O_SPLIT: 2, O_LANE: 2, O_SEG: 1},
                       {"segment_pairs": len(A), "split_tasks": 0})


def split_cases(name, R):
    """sed_wf_f64_split_kernel forced: a task per pair and stripe.  R = 2 is SPLIT's own default (SED_OPT_ROWS_PER_LANE
    0).  The tables of more than 16 symbols run their sweep as a batch of one-stripe tasks too (script only)."""
    A, B = split_batch(name, R)
    opts = {O_SPLIT: 1, O_R: 0 if R == 2 else R}
    tasks = sum(-(-len(a) // (64 * R)) for a in A)
    out = _wave_cases("split", name, R, A, B, opts, {"segment_pairs": 0, "split_tasks": tasks})
    if name in SWEEP_TABLES:
        A, B = sweep(name)
        out += [c for c in _wave_cases("split sweep", name, R, A, B, opts, {"segment_pairs": 0, "split_tasks": len(A)})
                if c.script]
    return out


def lane_cases(name):
    """sed_lane_f64_kernel: distance only, every pair on a lane (SED_OPT_LANE = 1: also in a batch of few pairs); under
    the tables of UNIT_LO the pairs inside the subset run bit-parallel, and the same batch runs with that switched off.
    n_first is dyadic over 5 symbols: its other pairs run sed_lane_scaled_kernel, whose bit-parallel branch reads the
    subset through a 2-bit map, and with the scaled kernel off the batch runs the fp64 lane kernel as the rest do."""
    A, B = lane_batch(name)
    unit = len(in_unit_subset(name, A, B)) if name in UNIT_LO else 0
    scaled = len(A) - unit if name == "n_first" else 0
    base = {"mode": F64, "lane_pairs": len(A), "segment_pairs": 0, "split_tasks": 0}
    opts = {O_SPLIT: 2, O_LANE: 1}
    ref = "lane " + name
    out = [Case("lane %s" % name, name, A, B, False, True, 0, opts,
                {**base, "bitpar_pairs": unit, "scaled_pairs": scaled}, ref)]
    if unit:
        out.append(Case("lane %s, bitpar off" % name, name, A, B, False, True, 0, {**opts, O_BITPAR: 2},
                        {**base, "bitpar_pairs": 0, "scaled_pairs": scaled and len(A)}, ref))
    if scaled:
        out.append(Case("lane %s, scaled off" % name, name, A, B, False, True, 0, {**opts, O_SCALED: 2},
                        {**base, "bitpar_pairs": unit, "scaled_pairs": 0}, ref))
    return out


def full_case(name, route):
    """What sed_full_matrix plans for its pair (fp64 at R = 4, the lengths wanted), as a Case for the planner: the
    one-wave kernel needs SPLIT switched off, as every single pair with cells goes SPLIT otherwise."""
    a, b = full_pair(name, route)
    opts = {O_R: 4, **({O_SPLIT: 2} if route == "one wave" else {})}
    tasks = 0 if route == "one wave" else -(-len(a) // 256)
    return Case("full %s, %s" % (name, route), name, [a], [b], False, False, 2, opts,
                {"mode": F64, "rows_per_lane": 4, "lane_pairs": 0, "segment_pairs": 0, "split_tasks": tasks},
                "full %s %s" % (name, route))


WAVE_R, SPLIT_R = (4, 8), (2, 4)


def all_cases():
    for name in WAVE_TABLES:
        for R in WAVE_R:
            yield from wave_cases(name, R)
            yield from seg_cases(name, R)
        for R in SPLIT_R:
            yield from split_cases(name, R)
    for name in LANE_TABLES:
        yield from lane_cases(name)
    for name in FULL_TABLES:
        for route in FULL_SHAPES:
            yield full_case(name, route)
