"""The fp64 route of the similarity join (sed_join_self_f64, sed_join_search_f64) as cost tables,
sequence sets and references, shared by the CPU tests (tests/test_join_f64_host.py) and the GPU tests
(tests/test_gpu_join_f64.py).  No device is needed here.

Tables: costs.json over its 15 IUPAC symbols, the rounding table of fit_f64_cases (0.1 / 0.2 / 0.3 / 0.7), a random
asymmetric table over 16 symbols, user_costs.json (which both routes serve), and a table of subnormal costs.
References: the C oracle over the full cross product (join_cases.oracle_matrix) cut with D <= T; lane_matrix is the
word-for-word model of the kernel's lane and keep_rule that of the planner's length skip."""
import math

import numpy as np

import fit_f64_cases as ff
import join_cases as jc
import oracle
import sedgpu
from conftest import load_golden

INF = math.inf
IUPAC = ff.IUPAC
AL16 = IUPAC + "X"
MAXK = 16   # SED_JOIN_F64_MAXK
MAXLEN = 32


def rounding_table():
    """fit_f64_cases.rounding_table as a table over ACGUN: 0.1 + 0.2 != 0.3 in fp64, so a kernel that reassociates,
    rebases or fuses shows."""
    al = "ACGUN"
    p = ff.rounding_table(len(al))
    return {"insert": 0.1, "delete": 0.2,
            "update": {a: {b: float(p.sub[i, j]) for j, b in enumerate(al)} for i, a in enumerate(al)}}, al


def random16_table():
    """16 symbols, insert != delete, sub[a][b] != sub[b][a], nothing dyadic."""
    rng = np.random.default_rng(1616)
    sub = rng.uniform(0.05, 1.5, size=(16, 16))
    return {"insert": 0.37, "delete": 0.83,
            "update": {a: {b: (0.0 if a == b else float(sub[i, j])) for j, b in enumerate(AL16)}
                       for i, a in enumerate(AL16)}}, AL16


def subnormal_table():
    """Every cost a small multiple of the smallest subnormal: sums and border products stay subnormal and exact."""
    al = "ACGU"
    q = 5e-324
    rng = np.random.default_rng(5)
    return {"insert": 3 * q, "delete": 7 * q,
            "update": {a: {b: (0.0 if a == b else float(rng.integers(1, 12)) * q) for b in al} for a in al}}, al


def tables():
    """name -> (table, alphabet); only user_costs is served by the integer route too."""
    return {"costs15": (load_golden("costs.json"), IUPAC),
            "rounding": rounding_table(),
            "random16": random16_table(),
            "user_costs": (load_golden("user_costs.json"), "ACGUN")}


def f64_only():
    return [n for n in tables() if n != "user_costs"]


def mixed_set(name, count=130, seed=None):
    table, al = tables()[name] if name in tables() else subnormal_table()
    return jc.mixed_set(2000 + len(name) + count if seed is None else seed, al, count, 0.05 if "N" in al else 0.0)


def edge_length_set(name, count=97):
    return jc.edge_length_set(3000 + len(name) + count, tables()[name][1], count)


def expected_hits_f64(D, T, self_join=False, row_lo=0):
    """The oracle's matrix cut with a plain D <= T; JOIN_HIT_DTYPE records sorted by (row, col); a self join leaves
    (i, i) out.  D's row r is row row_lo + r."""
    keep = D <= T
    if self_join:
        for r in range(D.shape[0]):
            keep[r, row_lo + r] = False
    r, c = np.nonzero(keep)
    out = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
    out["row"], out["col"], out["dist"] = r + row_lo, c, D[r, c]
    return out


def lane_matrix(plan, rows, cols):
    """sed_join_f64.hip's lane, word for word, every (row, column) pair side by side in numpy: the table as 16 x 16
    doubles with zeros past K, the column's codes zero padded to 32, row 0 = (double)j * insert, column 0 of row i =
    (double)i * delete, a cell = min(left + insert, min(up + delete, diagonal + tab[16 a + b_j])) over all 32 columns,
    the sink the register at the column's length m."""
    R, Cn = len(rows), len(cols)
    ins, dele = np.float64(plan.ins) + 0.0, np.float64(plan.dele) + 0.0
    tab = np.zeros((MAXK, MAXK))
    tab[:plan.K, :plan.K] = np.asarray(plan.sub, np.float64) + 0.0
    a = np.zeros((R, MAXLEN), np.int64)
    b = np.zeros((Cn, MAXLEN), np.int64)
    for i, s in enumerate(rows):
        a[i, :len(s)] = plan.encode(s)
    for j, s in enumerate(cols):
        b[j, :len(s)] = plan.encode(s)
    n = np.array([len(s) for s in rows], np.int64)
    m = np.array([len(s) for s in cols], np.int64)
    V = np.broadcast_to((np.arange(MAXLEN + 1, dtype=np.float64) * ins)[None, None, :], (R, Cn, MAXLEN + 1)).copy()
    for i in range(MAXLEN):
        live = (i < n)[:, None]
        ai = a[:, i]
        dg = V[:, :, 0].copy()
        V[:, :, 0] = np.where(live, np.float64(i + 1) * dele, V[:, :, 0])
        for j in range(1, MAXLEN + 1):
            cost = tab[ai[:, None], b[None, :, j - 1]]
            up = V[:, :, j].copy()
            v = np.minimum(V[:, :, j - 1] + ins, np.minimum(up + dele, dg + cost))
            V[:, :, j] = np.where(live, v, up)
            dg = up
    return np.take_along_axis(V, np.broadcast_to(m[None, :, None], (R, Cn, 1)), axis=2)[:, :, 0]


def keep_rule(ins, dele, T):
    """sed_join_plan.cpp: sed_join_f64_keep_rule, word for word: [n, m] true when a row of n and a column of m symbols
    are computed."""
    ins, dele = float(ins) + 0.0, float(dele) + 0.0
    keep = np.ones((MAXLEN + 1, MAXLEN + 1), bool)
    for n in range(MAXLEN + 1):
        for m in range(MAXLEN + 1):
            if n == 0 or m == 0:
                keep[n, m] = (float(m) * ins if n == 0 else float(n) * dele) <= T
            elif n != m and math.isfinite(T):
                p = float(m - n) * ins if m > n else float(n - m) * dele
                if math.isfinite(p) and p >= 2.0 ** -900:
                    keep[n, m] = not (p - p * 2.0 ** -40 > T)
    return keep


def keep_count(len_rows, len_cols, keep, self_rows=None):
    """Brute force: the pairs in scope the rule computes, and their cells; self_rows = the columns the rows are."""
    run = cells = 0
    for i, n in enumerate(len_rows):
        for j, m in enumerate(len_cols):
            if self_rows is not None and self_rows[i] == j:
                continue
            if keep[n, m]:
                run += 1
                cells += n * m
    return run, cells


def adversarial_min(plan, per_class=200, seed=9):
    """minD[n, m] = the oracle's smallest D over pairs of a row of n and a column of m symbols built to lie as close
    above the length bound as pairs can: the column is the row with |m - n| random symbols inserted at random places
    (m > n) or removed (n > m), so the indels cost nothing beyond the bound; plus, per class, the row followed by the
    extra symbols (matches, then inserts: the sequentially rounded sum), the extra symbols followed by the row (the
    border product, then matches) and their delete-side mirrors.  n = m is never skipped and stays +inf."""
    rng = np.random.default_rng(seed)
    K = plan.K
    ca, la, cb, lb, cls = [], [], [], [], []
    for n in range(MAXLEN + 1):
        for m in range(MAXLEN + 1):
            if n == m:
                continue
            lo, hi = min(n, m), max(n, m)
            short = rng.integers(0, K, size=(per_class + 2, lo))
            order = np.argsort(rng.random((per_class + 2, hi)), axis=1)
            extra = np.zeros((per_class + 2, hi), bool)
            np.put_along_axis(extra, order[:, :hi - lo], True, axis=1)
            extra[per_class] = np.arange(hi) >= lo        # the short one, then the extra symbols
            extra[per_class + 1] = np.arange(hi) < hi - lo  # the extra symbols, then the short one
            long_ = rng.integers(0, K, size=(per_class + 2, hi))
            long_[~extra] = short.ravel()
            a, b = (short, long_) if m > n else (long_, short)
            ca.append(a.ravel()), cb.append(b.ravel())
            la.append(np.full(per_class + 2, n)), lb.append(np.full(per_class + 2, m))
            cls.append(np.full(per_class + 2, n * (MAXLEN + 1) + m))
    ca, cb = np.concatenate(ca).astype(np.uint8), np.concatenate(cb).astype(np.uint8)
    la, lb, cls = (np.concatenate(x) for x in (la, lb, cls))
    oa = np.concatenate([[0], np.cumsum(la[:-1])]).astype(np.int64)
    ob = np.concatenate([[0], np.cumsum(lb[:-1])]).astype(np.int64)
    one = lambda x: x if len(x) else np.zeros(1, np.uint8)
    d = oracle.batch(oracle.Costs.from_plan(plan), one(ca), oa, la.astype(np.int32), one(cb), ob, lb.astype(np.int32),
                     len(la), nthreads=8)[0]
    out = np.full((MAXLEN + 1) ** 2, INF)
    np.minimum.at(out, cls, d)
    return out.reshape(MAXLEN + 1, MAXLEN + 1)


def cutoffs(table, D):
    """0, each cost, three occurring distances, the fp64 neighbours of all of them, +inf."""
    base = {0.0, float(table["insert"]), float(table["delete"])}
    base |= {float(v) for row in table["update"].values() for v in row.values()}
    occ = np.unique(D[np.isfinite(D)])
    base |= {float(occ[i]) for i in (1, len(occ) // 3, len(occ) // 2) if i < len(occ)}
    out = set()
    for t in base:
        out |= {t, float(np.nextafter(t, INF))} | ({float(np.nextafter(t, 0.0))} if t > 0 else set())
    return sorted(out) + [INF]


class DefinitionEngineF64(jc.DefinitionEngine):
    """join_cases.DefinitionEngine with the fp64 calls, for wfsearch's and sedshard's index_fn: it records how it was
    built and which calls served."""

    def __init__(self, seqs, user_cost=False, **kw):
        super().__init__(seqs, user_cost)
        self.kw = kw
        self.calls = []

    def self_join(self, max_dist, rows=None):
        self.calls.append("self_join")
        return super().self_join(max_dist, rows)

    def search(self, queries, max_dist):
        self.calls.append("search")
        return super().search(queries, max_dist)

    def self_join_f64(self, max_dist, rows=None):
        self.calls.append("self_join_f64")
        return super().self_join(max_dist, rows)

    def search_f64(self, queries, max_dist):
        self.calls.append("search_f64")
        return super().search(queries, max_dist)
