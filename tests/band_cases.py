"""The envelope of band pruning (SED_OPT_BAND) as cost tables and sequence families, shared by the CPU
model tests (tests/test_band_bound.py, tests/test_band_refine.py) and the GPU tests (tests/test_gpu_band_refine.py,
tests/test_gpu_band_envelope.py).  Any table i32_eligible accepts (sed_plan.cpp: 1 <= mismatch <= insert + delete <=
255, insert and delete >= 1) reaches the pruned route, in dot keys where it factors over signed bytes and in distance
keys where it does not; the tables here cover both, mismatches that tie with delete + insert, lopsided indels and
distances next to the 16-bit key limit.  The families put co-optimal paths on the window's edges (homopolymers, short
and chunk-length periods), move the path by hundreds of columns inside a stripe, and sit on the stripe and chunk
borders.  Everything is seeded and device-free."""
import functools
import json
import os

import numpy as np

import sedgpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = "ACGU"


# ---- cost tables (the reference's JSON shape, ACGU only) ----
def _table(ins, dele, sub):
    return {"insert": float(ins), "delete": float(dele),
            "update": {a: {b: float(sub[i][j]) for j, b in enumerate(S) if b != a} for i, a in enumerate(S)}}


def _golden(name, key=None):
    with open(os.path.join(GOLDEN, name)) as f:
        t = json.load(f)
    t = t["tables"][key] if key else t
    return _table(t["insert"], t["delete"], [[0 if a == b else t["update"][a][b] for b in S] for a in S])


def _drawn(seed, ins, dele, hi):
    """Mismatches uniform in 1..hi from a fixed seed, with 1, hi and insert + delete forced in."""
    rng = np.random.default_rng(seed)
    sub = rng.integers(1, hi + 1, size=(4, 4))
    sub[0, 1], sub[1, 0], sub[2, 3] = 1, hi, ins + dele
    return _table(ins, dele, sub.tolist())


# name: table.  The two shipped tables and `fact` (insert 3, delete 1, mismatches 1..2: a draw of test_gpu_routes'
# _factorable_tables) factor for dot keys at every shape used here; the other five do not (sed_dot_factor refuses them:
# tests/test_band_bound.py::test_case_tables_are_what_they_claim), `tight` and `heavy` included, so their three-stripe
# batches run the distance-key decode of the refinement.  `unfactorable` is the first refused draw of insert, delete
# 1..3, mismatches 1..4 from seed 768.
TABLES = {
    "costs.json": _golden("costs.json"),
    "user_costs.json": _golden("user_costs.json"),
    "fact": _table(3, 1, [[0, 2, 1, 2], [2, 0, 1, 2], [2, 2, 0, 2], [1, 2, 1, 0]]),
    "sum": _table(1, 2, [[0 if i == j else 3 for j in range(4)] for i in range(4)]),  # every mismatch = insert + delete
    "gui_int": _golden("g8_cost_tables.json", "gui_int"),  # insert 3, delete 1, mismatches 1..4
    "tight": _drawn(2, 2, 5, 7),
    "heavy": _drawn(3, 20, 60, 80),
    "unfactorable": _table(3, 3, [[0, 3, 1, 4], [1, 0, 4, 1], [4, 3, 0, 1], [4, 3, 1, 0]]),
}
FACTORABLE = ("costs.json", "user_costs.json", "fact")
NEW_TABLES = tuple(t for t in TABLES if not t.endswith(".json"))
# the largest m - n a family gives a table: `heavy` must keep npad delete + (m + 64 + 64 / R) insert <= 65533
# (sed_plan.cpp), which at R = 4 and n <= 768 is m <= 892
DELTA = {name: 150 if name == "heavy" else 300 for name in TABLES}


def costs(name):
    """(sub 4 x 4, insert, delete) of a table, as the device-free entry points of sedgpu take them."""
    t = TABLES[name]
    sub = np.array([[0.0 if a == b else t["update"][a][b] for b in S] for a in S])
    return sub, float(t["insert"]), float(t["delete"])


def factors(name, maxmin):
    """Whether a checkpoint batch whose largest min(n, m) is maxmin runs dot keys under the table."""
    return sedgpu.dot_factor(*costs(name), maxmin, 0) is not None


def i32_fits(name, A, B, R):
    """The planner's bound on the 16-bit distance field for every pair of a batch (sed_plan.cpp: dsum <= 65533)."""
    _, ins, dele = costs(name)
    rows = 64 * R
    return all((len(a) + rows - 1) // rows * rows * dele + max(len(b) + 64 + 64 // R, 32) * ins <= 65533
               for a, b in zip(A, B))


# ---- sequence families: (rng, n, R, delta) -> (A, B), lists of uint8 code arrays ----
def mut(rng, x, rate=0.1):
    return np.where(rng.random(len(x)) < rate, rng.integers(0, 4, size=len(x)), x).astype(np.uint8)


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def random_family(rng, n, R, delta=300):
    """Random, identical, mutated; a last stripe below 64 rows; m - n = +-delta; shifted copies (a path off the
    diagonal)."""
    rows = 64 * R
    r = lambda k: rng.integers(0, 4, size=k).astype(np.uint8)  # noqa: E731
    a, s = r(n), r(2 * rows + 40)
    A = [a, a, a, s, s, a, a, a[:n - delta], a, a[37:]]
    B = [r(n), a.copy(), mut(rng, a), mut(rng, s), r(len(s)), np.concatenate([mut(rng, a), r(delta)]),
         mut(rng, a)[delta:], r(n), np.concatenate([r(37), mut(rng, a)[:n - 37]]), mut(rng, a)]
    return A, B


RANDOM_RELATED = (1, 2)  # random_family's identical and mutated pairs: the narrowest windows


def low_complexity(rng, n, R, delta=300):
    """Inputs whose co-optimal paths fan out to the window's edges: homopolymers against themselves and against another
    symbol, (AC)^k against (CA)^k, (ACGU)^k against its rotations (5 % mutated), and random units of period 63, 64
    and 65 (the chunk length and its neighbours) against themselves shifted by half a period; m - n over 0, +-1, +-37
    and +-delta."""
    A, B = [], []
    deltas = (0, 1, -1, 37, -37, delta, -delta)
    for d in deltas:
        A += [np.zeros(n), np.zeros(n), np.resize([0, 1], n)]
        B += [np.zeros(n + d), np.ones(n + d), np.resize([1, 0], n + d)]
    for rot, ds in ((1, (0, 1, -37, delta)), (2, (0, -1, 37, -delta)), (3, (0, 37, -delta, delta))):
        for d in ds:
            A.append(np.resize([0, 1, 2, 3], n))
            B.append(mut(rng, np.resize(np.roll([0, 1, 2, 3], -rot), n + d), 0.05))
    for period, ds in ((63, (0, 1, -delta)), (64, (0, -1, delta)), (65, (0, 37, -37))):
        unit = rng.integers(0, 4, size=period)
        for d in ds:
            A.append(np.resize(unit, n))
            B.append(np.resize(np.roll(unit, -(period // 2)), n + d))
    return [_u8(a) for a in A], [_u8(b) for b in B]


def rearranged(rng, n, R, delta=300):
    """Paths that leave the diagonal by hundreds of columns inside one stripe: a block swap (|X| = 200), one deletion of
    delta symbols (b = a[:200] + a[200 + delta:]) and its mirror, delta random symbols inserted; two deletions and two
    insertions of delta / 2 that start inside stripe 1 (the insertions, 20 rows apart, lie inside it at every R; the
    deletions do where 64 R >= delta + 30).  Each also 5 % mutated."""
    rows = 64 * R
    r = lambda k: rng.integers(0, 4, size=k).astype(np.uint8)  # noqa: E731
    a, h, p = r(n), delta // 2, rows + 10
    assert n >= max(200 + delta, p + 2 * h + 20) + 20
    bs = [np.concatenate([a[200:], a[:200]]),
          np.concatenate([a[:200], a[200 + delta:]]),
          np.concatenate([a[:200], r(delta), a[200:]]),
          np.concatenate([a[:p], a[p + h:p + h + 20], a[p + 2 * h + 20:]]),
          np.concatenate([a[:p], r(h), a[p:p + 20], r(h), a[p + 20:]])]
    bs += [mut(rng, b, 0.05) for b in bs]
    return [a] * len(bs), [_u8(b) for b in bs]


def edges(rng, n, R, delta=300):
    """Stripe and chunk borders (n is not read): n = 2 ROWS + 1 (a last stripe of one row), 3 ROWS (a full one) and
    3 ROWS + 1, each against m = 1, 63, 64, 65 and 64 c, 64 c + 1 with 64 c next to n (the rounding of
    sed_band_chunks); one pair with m = 5 n.  str2 is a 10 % mutation of str1, truncated or extended with random
    symbols."""
    rows = 64 * R
    A, B = [], []
    for nn in (2 * rows + 1, 3 * rows, 3 * rows + 1):
        a = rng.integers(0, 4, size=nn).astype(np.uint8)
        c = (nn + 32) // 64
        for m in (1, 63, 64, 65, 64 * c, 64 * c + 1) + ((5 * nn,) if nn == 2 * rows + 1 else ()):
            A.append(a)
            B.append(np.concatenate([mut(rng, a), rng.integers(0, 4, size=max(m - nn, 0)).astype(np.uint8)])[:m])
    return A, B


def drift(rng, n, R, delta=300):
    """Ten stripes and a last one of 40 rows (n = 10 ROWS + 40, n is not read) with a path that moves 40 columns per
    stripe: 40 symbols deleted after every ROWS rows, 40 random ones inserted there, and the two alternating; then the
    same 5 % mutated.  Every stripe starts and ends at another chunk than the one above (the `clo > clo_prev` load of
    the forward, the stale words of the in-place bottom-row buffer)."""
    rows = 64 * R
    a = rng.integers(0, 4, size=10 * rows + 40).astype(np.uint8)
    blocks = [a[k * rows:(k + 1) * rows] for k in range(11)]
    ins40 = lambda: rng.integers(0, 4, size=40).astype(np.uint8)  # noqa: E731
    deleted = np.concatenate([blocks[0]] + [blk[40:] for blk in blocks[1:]])
    inserted = np.concatenate([blocks[0]] + [x for blk in blocks[1:] for x in (ins40(), blk)])
    mixed = np.concatenate([blocks[0]] + [x for k, blk in enumerate(blocks[1:])
                                          for x in ((blk[40:],) if k % 2 else (ins40(), blk))])
    bs = [deleted, inserted, mixed]
    bs += [mut(rng, b, 0.05) for b in bs]
    return [a] * len(bs), bs


FAMILIES = {"random": random_family, "low_complexity": low_complexity, "rearranged": rearranged, "edges": edges,
            "drift": drift}
# the shapes the tables x families tests run at R = 4: three stripes, the last of 88, 107 and 188 rows
FAMILY_N = {"random": 600, "low_complexity": 619, "rearranged": 700, "edges": 0, "drift": 0}


def seed(*parts):
    """A seed of its own for every named input (shared with tests/cut_cases.py)."""
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(map(str, parts))))


def family_pairs(table, family, R, n=None, families=None, family_n=None, delta=None):
    """(A, B) of one family under one table's delta, from a seed of its own.  families, family_n and delta stand in for
    FAMILIES, FAMILY_N and DELTA (tests/cut_cases.py adds families of its own)."""
    n = (family_n or FAMILY_N)[family] if n is None else n
    return (families or FAMILIES)[family](np.random.default_rng(seed(table, family, R, n)), n, R,
                                          (delta or DELTA)[table])


# ---- the reference of the CPU model tests: forward + backward DP in numpy (integer costs: exact in float64) ----
def dp(sub, ins, dele, a, b):
    """F[i, j] = the cost of the cheapest path (0, 0) -> (i, j)."""
    n, m = len(a), len(b)
    F = np.zeros((n + 1, m + 1))
    ramp = ins * np.arange(m + 1)
    F[0, :] = ramp
    for i in range(1, n + 1):
        cand = np.empty(m + 1)
        cand[0] = dele * i
        cand[1:] = np.minimum(F[i - 1, 1:] + dele, F[i - 1, :-1] + sub[a[i - 1], b])  # delete, update
        F[i] = np.minimum.accumulate(cand - ramp) + ramp  # the insert chain along the row
    return F


class Ref:
    """What the model tests read of one pair's DP: the distance, the plain diagonal's cost and its suffixes, the
    extreme diagonals and, row by row, the extreme columns >= 1 of the cells on a distance-optimal path, and the rows
    at the stripe boundaries (values and which cells are optimal)."""

    def __init__(self, sub, ins, dele, a, b, R):
        n, m, rows = len(a), len(b), 64 * R
        F = dp(sub, ins, dele, a, b)
        Bk = dp(sub, ins, dele, a[::-1], b[::-1])[::-1, ::-1]  # the cheapest path (i, j) -> (n, m)
        self.a, self.b, self.n, self.m, self.dist = a, b, n, m, F[n, m]
        opt = F + Bk == self.dist
        ii, jj = np.nonzero(opt)
        self.emin, self.emax = int((jj - ii).min()), int((jj - ii).max())
        inner = opt[:, 1:]
        self.has = inner.any(axis=1)  # (a row whose only optimal cell is column 0 has none to check)
        self.jmin = inner.argmax(axis=1) + 1
        self.jmax = m - inner[:, ::-1].argmax(axis=1)
        k_ = min(n, m)
        self.diag = sub[a[:k_], b[:k_]]
        self.gap = ins * (m - n) if m > n else dele * (n - m)
        self.ub = float(self.diag.sum()) + self.gap
        self.rows = {r0: (F[r0].copy(), opt[r0].copy()) for r0 in range(rows, n, rows)}


@functools.lru_cache(maxsize=None)
def refs(table, family, R):
    """The Refs of family_pairs(table, family, R): computed once per session, shared by both model tests."""
    sub, ins, dele = costs(table)
    A, B = family_pairs(table, family, R)
    return [Ref(sub, ins, dele, a, b, R) for a, b in zip(A, B)]
