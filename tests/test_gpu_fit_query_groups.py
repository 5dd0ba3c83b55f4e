"""GPU: more than 65 535 queries in one index call, so that every fit launcher runs a second query group
(sed_internal.h: sed_fit_each_query_group): the group's first query reaches the kernel, the grid's y is the group's
size, the events sit on the right kernels, and queries 65 535 and 65 536 get what every other query gets.

One index over a single text of 12 symbols (one chunk record, so the grid's x extent is 1) and 65 537 queries that cycle
through 61 distinct patterns (61 is prime: the boundary at 65 535 falls mid-cycle), through the four routes, search and
hits.  Patterns: 1..8 symbols on the short routes, 65..72 on the long ones (all in the R = 2 group, which so crosses the
limit): a piece of the text, or one with a symbol changed, behind 64 copies of one code on the long routes.

Expected values are the C oracle's on the 61 patterns, tiled.  The best hit is oracle.fit's.  The hits come from
oracle.batch: E(e), S(e) = the lexicographic minimum over s of (D(pattern, text[s:e]), -s), which is the cell the fit DP
keeps in the last row at column e when sums of costs are exact, as they are here (every cost among the codes that occur
is a multiple of 1/4; asserted).  Before anything runs on a device the module checks that reference against oracle.fit:
the row's first strict minimum is the best hit.  Which 61 of the candidate patterns a case takes, and its max_dist, are
chosen from the oracle's rows: the smallest max_dist at which 61 candidates of all eight lengths have one to four hits."""
import types

import numpy as np
import pytest

import fit_envelope
import fit_f64_cases as fc
import oracle
import sedgpu
from test_gpu_fit import _golden_plan

NQ, NPAT, NTEXT = 65537, 61, 12
EDGE = (65534, 65535, 65536)
# route: (search call, hits call, symbols in front of the piece, the device-free plan export)
ROUTES = {
    "i32": ("search", "hits", 0, sedgpu.fit_index_plan),
    "f64": ("search_f64", "hits_f64", 0, sedgpu.fit_index_f64_plan),
    "long": ("search_long", "hits_long", 64, sedgpu.fit_index_long_plan),
    "long_f64": ("search_long_f64", "hits_long_f64", 64, sedgpu.fit_index_long_f64_plan),
}


def _plan(route):
    """The table the route's own GPU tests run under."""
    if route.endswith("f64"):
        return fc.golden15("costs.json")
    g = _golden_plan("user_costs.json", "ACGU")
    return fit_envelope.Plan(g.sub, g.ins, g.dele)


def _ncodes(route):
    """The codes a case draws from, 0 .. n - 1: all four of the integer table, the ten of the fp64 table whose mutual
    costs are multiples of 1/4."""
    return 10 if route.endswith("f64") else 4


def _candidates(front, text, ncodes):
    """Distinct patterns: `front` copies of a code (each of 0..3 in turn, if any), then a piece of the text of 1..8
    symbols, as it is or with one symbol changed (to one of the next three codes)."""
    pieces = [text[b - L:b] for L in range(1, 9) for b in range(L, NTEXT + 1)]
    for p in list(pieces):
        for i in range(len(p)):
            for c in range(1, 4):
                q = p.copy()
                q[i] = (p[i] + c) % ncodes
                pieces.append(q)
    out, seen = [], set()
    for f in (range(4) if front else [0]):
        for p in pieces:
            pat = np.concatenate([np.full(front, f, np.uint8), p]).astype(np.uint8)
            if pat.tobytes() not in seen:
                seen.add(pat.tobytes())
                out.append(pat)
    return out


def _last_rows(plan, pats, text):
    """(E, S), each [pattern, e] for e = 0 .. len(text): the last row of every pattern's fit matrix, from oracle.batch."""
    n = len(text)
    se = np.array([(s, e) for e in range(n + 1) for s in range(e, -1, -1)], np.int64)  # (per e: the largest s first)
    lens = np.array([len(p) for p in pats], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    npairs = len(pats) * len(se)
    d = oracle.batch(oracle.Costs.from_plan(plan), np.concatenate(pats), np.repeat(offs, len(se)), np.repeat(lens, len(se)),
                     np.concatenate([text, np.zeros(1, np.uint8)]), np.tile(se[:, 0], len(pats)).copy(),
                     np.tile((se[:, 1] - se[:, 0]).astype(np.int32), len(pats)).copy(), npairs, nthreads=4)[0]
    d = d.reshape(len(pats), len(se))
    E = np.zeros((len(pats), n + 1))
    S = np.zeros((len(pats), n + 1), np.int64)
    for e in range(n + 1):
        cols = np.flatnonzero(se[:, 1] == e)
        k = np.argmin(d[:, cols], axis=1)  # (the first minimum = the one of the largest s)
        E[:, e] = d[np.arange(len(pats)), cols[k]]
        S[:, e] = se[cols[k], 0]
    return E, S


class Case:
    """A route's inputs and the oracle's answers, built once."""

    def __init__(self, route):
        self.route = route
        self.plan = plan = _plan(route)
        nc = _ncodes(route)
        for v in (plan.sub[:nc, :nc].ravel().tolist() + [plan.ins, plan.dele]):
            assert v >= 0 and float(4 * v).is_integer(), "sums of these costs are exact in fp64"
        self.text = text = np.random.default_rng(12).integers(0, nc, size=NTEXT).astype(np.uint8)
        cand = _candidates(ROUTES[route][2], text, nc)
        E, S = _last_rows(plan, cand, text)
        lens = np.array([len(p) for p in cand])
        # the smallest cutoff at which 61 candidates of all eight lengths have one to four hits, and those candidates:
        # the lengths in turn, each length's in the order they were built
        self.max_dist, pick = None, None
        for T in np.unique(E).tolist():
            n = (E <= T).sum(axis=1)
            ok = [list(np.flatnonzero((n >= 1) & (n <= 4) & (lens == L))) for L in sorted(set(lens.tolist()))]
            if all(ok) and sum(len(x) for x in ok) >= NPAT:
                self.max_dist, pick = T, []
                while len(pick) < NPAT:
                    for x in ok:
                        if x and len(pick) < NPAT:
                            pick.append(int(x.pop(0)))
                break
        assert pick is not None, "no cutoff gives 61 patterns of every length one to four hits"
        self.pats = pats = [cand[i] for i in pick]
        assert len({p.tobytes() for p in pats}) == NPAT and len({len(p) for p in pats}) == 8
        self.best = fit_envelope.oracle_fit(plan, pats, [text] * NPAT)
        self.hits = []
        for k, i in enumerate(pick):
            e = min(range(NTEXT + 1), key=lambda j: (E[i, j], j))  # the row's first strict minimum is the best hit
            assert (float(E[i, e]), int(S[i, e]), e) == self.best[k], (route, k)
            self.hits.append([(int(S[i, j]), j, float(E[i, j])) for j in range(NTEXT + 1) if E[i, j] <= self.max_dist])
        assert all(1 <= len(h) <= 4 for h in self.hits)
        self.qi = qi = np.arange(NQ) % NPAT
        off = np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.int64)
        self.queries = types.SimpleNamespace(
            npairs=NQ, codes_a=np.concatenate(pats + [np.zeros(1, np.uint8)]), off_a=off[qi].copy(),
            len_a=np.array([len(p) for p in pats], np.int32)[qi].copy())


_cases = {}


def case(route):
    if route not in _cases:
        _cases[route] = Case(route)
    return _cases[route]


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_planner_serves_65537_queries(route):
    """Without a device: the case exists (one to four hits per pattern at its cutoff) and the route's planner takes it."""
    c = case(route)
    plan = ROUTES[route][3](c.plan.costs(), {}, c.queries.len_a, [NTEXT])
    if "rows" in plan:
        assert set(np.asarray(plan["rows"]).tolist()) == {2}


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_search_past_one_query_group(gpu, route):
    c = case(route)
    gpu.set_costs(c.plan)
    ix = sedgpu.FitIndex.from_texts(gpu, [c.text])
    try:
        d, s, e = getattr(ix, ROUTES[route][0])(c.queries)
        assert ix.last_ms() > 0  # (the events of the first and of the last group)
    finally:
        ix.close()
    got = list(zip(d.ravel().tolist(), s.ravel().tolist(), e.ravel().tolist()))
    want = [c.best[k] for k in c.qi.tolist()]
    bad = [q for q in range(NQ) if got[q] != want[q]]
    assert not bad, (len(bad), bad[:3], bad[-3:], "queries 65534, 65535, 65536 (got, oracle):",
                     {q: (got[q], want[q]) for q in EDGE})


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_hits_past_one_query_group(gpu, route):
    c = case(route)
    want = [(q, 0, s, e, D) for q, k in enumerate(c.qi.tolist()) for s, e, D in c.hits[k]]
    gpu.set_costs(c.plan)
    ix = sedgpu.FitIndex.from_texts(gpu, [c.text])
    try:
        h = getattr(ix, ROUTES[route][1])(c.queries, c.max_dist, cap=len(want))
        assert ix.hits_last_ms() > 0
    finally:
        ix.close()
    got = sorted(zip(h["query"].tolist(), h["text"].tolist(), h["start"].tolist(), h["end"].tolist(), h["dist"].tolist()))
    by_q = lambda recs: {q: [r for r in recs if r[0] == q] for q in EDGE}
    assert got == sorted(want), (len(got), len(want), "queries 65534, 65535, 65536 (got, oracle):", by_q(got), by_q(want))
