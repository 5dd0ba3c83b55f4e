"""Shared builders of the similarity join's tests (test_join_host.py, test_gpu_join.py): the cost tables, the sequence
sets and the reference - the C oracle over the full row x column cross product, cut at T on the host."""
import importlib
import json
import math
import os

import numpy as np

import oracle
import sedcost
import sedgpu
from conftest import GOLDEN, load_golden

INF = math.inf


def import_shim(name):
    """A module of the drop-in package, which reads its cost tables from the working directory when it is imported."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        return importlib.import_module(name)
    finally:
        os.chdir(cwd)


def eighths_table():
    """8 symbols in eighths, insert != delete, sub[a][b] != sub[b][a]: a swapped direction changes the distances."""
    al = "ACGUNRYS"
    rng = np.random.default_rng(4242)
    t = {"insert": 0.625, "delete": 1.25, "update": {}}
    for a in al:
        t["update"][a] = {b: (0.0 if a == b else float(rng.integers(1, 15)) / 8.0) for b in al}
    t["update"]["A"]["C"], t["update"]["C"]["A"] = 0.25, 1.75
    return t, al


def served_tables():
    """name -> (table, alphabet, S)"""
    e, al = eighths_table()
    return {"costs ACGU": (load_golden("costs.json"), "ACGU", 1),
            "costs ACGUN": (load_golden("costs.json"), "ACGUN", 4),
            "user_costs": (load_golden("user_costs.json"), "ACGUN", 4),
            "eighths": (e, al, 8)}


def refused_tables():
    """name -> (table, alphabet, regex of the refusal's text): test_lane_scaled_dyadic_vs_oracle's three."""
    costs = load_golden("costs.json")
    t2 = json.loads(json.dumps(costs))
    for a in "ACGU":
        t2["update"][a]["N"] = 0.66
    t3 = json.loads(json.dumps(costs))
    t3["update"]["A"]["N"] = 2.5
    al9 = "ACGUNRYSK"
    rng = np.random.default_rng(77)
    t4 = {"insert": 0.625, "delete": 1.25, "update": {}}
    for a in al9:
        t4["update"][a] = {b: (0.0 if a == b else float(rng.integers(1, 15)) / 8.0) for b in al9}
    return {"N at 0.66": (t2, "ACGUN", r"multiples of 2\^-k"),
            "A->N 2.5": (t3, "ACGUN", r"exceeds insert \+ delete"),
            "9 symbols": (t4, al9, r"9 symbols")}


def plan_for(table, alphabet):
    """The CostPlan over the whole alphabet, in its order (code c = alphabet[c])."""
    return sedcost.plan_over(table, list(alphabet), set(alphabet), set(alphabet))


def costs_of(plan):
    return (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)


def random_seq(rng, alphabet, n, pn=0.0):
    base = [c for c in alphabet if c != "N"] if pn else list(alphabet)
    return "".join("N" if pn and rng.random() < pn else base[int(rng.integers(len(base)))] for _ in range(n))


def mixed_set(seed, alphabet, count, pn=0.0):
    """Lengths from {0, 1, 2, 31, 32} and U[20, 32], planted duplicates, and near-duplicates one substitution and one
    indel away."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < count:
        n = int(rng.choice([0, 1, 2, 31, 32])) if rng.random() < 0.3 else int(rng.integers(20, 33))
        s = random_seq(rng, alphabet, n, pn)
        seqs.append(s)
        r = rng.random()
        if len(s) >= 2 and len(seqs) < count:
            p = int(rng.integers(len(s)))
            if r < 0.12:
                seqs.append(s)  # a duplicate
            elif r < 0.24:
                c = random_seq(rng, alphabet.replace(s[p], "") or alphabet, 1)
                seqs.append(s[:p] + c + s[p + 1:])  # one substitution
            elif r < 0.36:
                seqs.append(s[:p] + s[p + 1:])  # one deletion
    order = rng.permutation(count)
    return [seqs[i] for i in order]


def edge_length_set(seed, alphabet, count):
    """Only the lengths 0, 1, 31 and 32; the last sequence has 32 symbols."""
    rng = np.random.default_rng(seed)
    seqs = [random_seq(rng, alphabet, int(rng.choice([0, 1, 31, 32]))) for _ in range(count - 1)]
    return seqs + [random_seq(rng, alphabet, 32)]


def encode(plan, seqs):
    return [plan.encode(s) for s in seqs]


def packed_queries(plan, seqs):
    ca, la = plan.encode_many(seqs)
    return sedgpu.PackedPairs.from_concat(ca, la, np.zeros(0, np.uint8), np.zeros(len(la), np.int32))


def codes_mask(plan, seqs):
    m = 0
    for s in seqs:
        m |= sedgpu.codes_seen(plan.encode(s)) if len(s) else 0
    return m


def oracle_matrix(plan, rows, cols):
    """D[r, c] = the C oracle's dp[n][m].value for (str1 = rows[r], str2 = cols[c]), the full cross product."""
    if not rows or not cols:
        return np.zeros((len(rows), len(cols)))
    pp = sedgpu.PackedPairs([plan.encode(a) for a in rows for _ in cols], [plan.encode(b) for _ in rows for b in cols])
    d = oracle.batch(oracle.Costs.from_plan(plan), pp.codes_a, pp.off_a, pp.len_a, pp.codes_b, pp.off_b, pp.len_b,
                     pp.npairs, nthreads=4)[0]
    return d.reshape(len(rows), len(cols)).copy()


def expected_hits(D, T, S, self_join=False, row_lo=0):
    """The oracle's matrix cut at T: a pair is within T exactly when D * S <= floor(T * S) (D * S is an exact integer);
    JOIN_HIT_DTYPE records sorted by (row, col); a self join leaves (i, i) out.  D's row r is row row_lo + r."""
    cut = INF if T == INF else math.floor(T * S)
    keep = (D * S) <= cut
    if self_join:
        for r in range(D.shape[0]):
            keep[r, row_lo + r] = False
    r, c = np.nonzero(keep)
    out = np.zeros(len(r), sedgpu.JOIN_HIT_DTYPE)
    out["row"], out["col"], out["dist"] = r + row_lo, c, D[r, c]
    return out


def same_hits(got, want):
    """The same (row, col) and dist bit for bit."""
    return len(got) == len(want) and np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]) \
        and np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64))


def lower_bound_count(len_rows, len_cols, ins, dele, T, S, self_rows=None):
    """Brute force: the pairs in scope with lb * S <= floor(T * S), lb = insert (m - n)+ + delete (n - m)+, and their
    cells; self_rows = the columns the rows are (a self join leaves those pairs out)."""
    cut = INF if T == INF else math.floor(T * S)
    run = cells = 0
    for i, n in enumerate(len_rows):
        for j, m in enumerate(len_cols):
            if self_rows is not None and self_rows[i] == j:
                continue
            if (ins * max(m - n, 0) + dele * max(n - m, 0)) * S <= cut:
                run += 1
                cells += n * m
    return run, cells


class DefinitionEngine:
    """A pure-Python JoinIndex engine for wfsearch's and sedshard's index_fn: wagnerFisher's recurrence over the
    golden tables, cut at T."""

    def __init__(self, seqs, user_cost=False):
        self.seqs = list(seqs)
        self.table = load_golden("user_costs.json" if user_cost else "costs.json")
        self.closed = False

    def dist(self, a, b):
        t = self.table
        ins, dele, upd = t["insert"], t["delete"], t["update"]
        prev = [j * ins for j in range(len(b) + 1)]
        for i, x in enumerate(a, 1):
            cur = [i * dele]
            for j, y in enumerate(b, 1):
                c = 0 if x.lower() == y.lower() else upd[x][y]
                cur.append(min(cur[j - 1] + ins, prev[j] + dele, prev[j - 1] + c))
            prev = cur
        return float(prev[len(b)])

    def self_join(self, max_dist, rows=None):
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        return [(i, j, d) for i in range(lo, hi) for j, b in enumerate(self.seqs)
                if i != j for d in [self.dist(self.seqs[i], b)] if d <= max_dist]

    def search(self, queries, max_dist):
        return [(q, j, d) for q, a in enumerate(queries) for j, b in enumerate(self.seqs)
                for d in [self.dist(a, b)] if d <= max_dist]

    def close(self):
        self.closed = True
