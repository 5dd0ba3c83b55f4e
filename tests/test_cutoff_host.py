"""CPU: the host side of bounded search (sed_batch_set_cutoff).  The windowed distance-only kernel runs
the band of SED_OPT_BAND under ub = min(cutoff, diagonal bound); results stay exact for every pair within the cutoff as
long as every cell of every path of cost <= cutoff lies inside the window of that cutoff, which is checked here on small
pairs against a forward plus backward DP in numpy (tests/test_band_bound.py does it for the diagonal bound).  Then
wfsearch.nearest's deepening loop against brute force, with the C oracle standing in for the engine, and the untouched
default path of distance_batch."""
import importlib
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import oracle
import sedcost
import sedgpu

S = "ACGU"


@pytest.fixture(scope="module")
def wfsearch():
    """wfsearch and the drop-in module it scores with (wfsearch.SED), which reads its cost tables from the working
    directory when it is imported, as the reference does."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        return importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)


def _table(name):
    t = load_golden(name)
    sub = np.array([[0.0 if a == b else t["update"][a][b] for b in S] for a in S])
    return sub, float(t["insert"]), float(t["delete"])


def _dp(sub, ins, dele, a, b):
    """F[i, j] = the cost of the cheapest path (0, 0) -> (i, j)."""
    n, m = len(a), len(b)
    F = np.zeros((n + 1, m + 1))
    F[0, :] = ins * np.arange(m + 1)
    F[:, 0] = dele * np.arange(n + 1)
    for i in range(1, n + 1):
        up = np.minimum(F[i - 1, 1:] + dele, F[i - 1, :-1] + sub[a[i - 1], b])
        row = F[i]
        for j in range(1, m + 1):
            v = row[j - 1] + ins
            row[j] = v if v < up[j - 1] else up[j - 1]
    return F


@pytest.mark.parametrize("name", ["user_costs.json", "costs.json"])
def test_every_path_within_the_cutoff_lies_inside_its_window(name):
    sub, ins, dele = _table(name)
    rng = np.random.default_rng(31337 + len(name))
    checked = nonempty = 0
    for it in range(300):
        n, m = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if it % 3 == 0:
            m = n
        a = rng.integers(0, 4, size=n)
        if it % 2:  # related: a shifted, mutated copy; else independent
            src = np.resize(np.roll(a, -int(rng.integers(0, 4))), m)
            b = np.where(rng.random(m) < 0.15, rng.integers(0, 4, size=m), src)
        else:
            b = rng.integers(0, 4, size=m)
        F = _dp(sub, ins, dele, a, b)
        Bk = _dp(sub, ins, dele, a[::-1], b[::-1])[::-1, ::-1]  # the cheapest path (i, j) -> (n, m)
        through = F + Bk  # the cheapest path through each cell
        D = F[-1, -1]
        gap = ins * max(m - n, 0) + dele * max(n - m, 0)
        for T in (D - 1, D, D + 1, D + ins + dele, 2 * D + 3, float(int(rng.integers(0, 60)))):
            if T < gap:  # no path at all: the engine runs no stripe for such a pair
                assert not (through <= T).any()
                continue
            elo, ehi = sedgpu.band_bounds(n, m, ins, dele, T)
            assert elo <= min(0, m - n) and ehi >= max(0, m - n)
            ii, jj = np.nonzero(through <= T)
            checked += 1
            if len(ii):
                nonempty += 1
                e = jj - ii
                assert e.min() >= elo and e.max() <= ehi, (n, m, T, elo, ehi, int(e.min()), int(e.max()))
    assert checked > 900 and nonempty > 600


def _oracle_distances(table, queries, seqs):
    plan = sedcost.build_plan(table, queries, seqs)
    packed = sedgpu.PackedPairs([plan.encode(q) for q in queries], [plan.encode(s) for s in seqs])
    d, is_int, _, _, _ = oracle.batch(oracle.Costs.from_plan(plan), packed.codes_a, packed.off_a, packed.len_a,
                                      packed.codes_b, packed.off_b, packed.len_b, packed.npairs)
    return [int(v) if t else float(v) for v, t in zip(d.tolist(), is_int.tolist())]


@pytest.mark.parametrize("user", [False, True])
def test_nearest_against_brute_force(user, wfsearch, monkeypatch):
    table = load_golden("user_costs.json" if user else "costs.json")
    monkeypatch.setattr(wfsearch.SED, "user_costs" if user else "default_costs", table)
    rng = np.random.default_rng(5150 + user)
    rounds = []
    for it in range(100):  # (x 2 cost tables: 200 document sets)
        q = "".join(rng.choice(list(S), size=int(rng.integers(1, 16))))
        nd = int(rng.integers(1, 14))
        if it % 10 == 0:  # all documents identical
            docs = ["".join(rng.choice(list(S), size=int(rng.integers(1, 16))))] * nd
        else:
            docs = []
            for _ in range(nd):
                if rng.random() < 0.4:  # a mutated copy of the query, or a copy of an earlier document (ties)
                    src = list(q if not docs or rng.random() < 0.6 else docs[int(rng.integers(0, len(docs)))])
                    for _m in range(int(rng.integers(0, 3))):
                        src[int(rng.integers(0, len(src)))] = str(rng.choice(list(S)))
                    docs.append("".join(src))
                else:
                    docs.append("".join(rng.choice(list(S), size=int(rng.integers(1, 20)))))
        k = [1, nd, nd + 3, int(rng.integers(1, nd + 1))][it % 4]
        cuts = []

        def fake(queries, seqs, max_dist):
            cuts.append(max_dist)
            return [v if v <= max_dist else math.inf for v in _oracle_distances(table, queries, seqs)]

        got = wfsearch.nearest(q, docs, k, user_cost=user, distance_fn=fake)
        full = _oracle_distances(table, [q] * nd, docs)
        want = sorted(range(nd), key=lambda i: (full[i], i))[:k]  # ties by collection order
        assert got == [(docs[i], 1 / (1 + full[i])) for i in want], (q, docs, k)
        assert cuts and cuts == sorted(cuts) and len(set(cuts)) == len(cuts)  # the cutoff only grows
        rounds.append(len(cuts))
    assert max(rounds) > 1  # (the loop did deepen somewhere)
    assert wfsearch.nearest("ACGU", [], 3, distance_fn=lambda *a: []) == []
    assert wfsearch.nearest("ACGU", ["ACGU"], 0, distance_fn=lambda *a: [0]) == []


class _FakeContext:
    def __init__(self):
        self.calls = []

    def set_costs(self, plan):
        pass

    def run(self, packed, want_script, no_len=False):
        self.calls.append(("run", want_script, no_len))
        P = packed.npairs
        return np.arange(P, dtype=np.float64), np.ones(P, np.uint8), np.full(P, -1, np.int32), None

    def run_cutoff(self, packed, max_dist, no_len=True):
        self.calls.append(("run_cutoff", max_dist, no_len))
        P = packed.npairs
        d = np.arange(P, dtype=np.float64)
        far = d > max_dist
        return np.where(far, np.inf, d), (~far).astype(np.uint8), np.full(P, -1, np.int32), int((~far).sum())


def test_distance_batch_without_a_cutoff_keeps_its_path(wfsearch, monkeypatch):
    SED = wfsearch.SED
    fake = _FakeContext()
    monkeypatch.setattr(sedgpu, "context", lambda: fake)
    a, b = ["ACGU", "AC", "G"], ["ACGA", "UC", "GG"]
    assert SED.distance_batch(a, b) == [0, 1, 2]
    assert SED.distance_batch(a, b, max_dist=None) == [0, 1, 2]
    assert fake.calls == [("run", False, True)] * 2  # the one engine call of the default path, nothing else
    out = SED.distance_batch(a, b, max_dist=1)
    assert out == [0, 1, math.inf] and [type(v) for v in out] == [int, int, float]
    assert fake.calls[-1] == ("run_cutoff", 1, True)
    # the search cache serves wf_scores only
    wfsearch.clear_cache()
    assert wfsearch.search_within("ACGU", b, 1) == [("ACGA", 1.0), ("UC", 0.5)]
    assert not wfsearch._CACHE


class _ServedContext:
    """Stands in for sedgpu.Context behind sedgpu._serve."""
    seen = []

    def __init__(self, device=0):
        self.device = device

    def run_cutoff(self, packed, max_dist, no_len=True):
        _ServedContext.seen.append(("run_cutoff", packed.npairs, max_dist, no_len))
        return np.array([1.0, np.inf]), np.array([1, 0], np.uint8), np.array([-1, -1], np.int32), 1

    def deepen(self, packed, k, first, last, no_len=True):
        _ServedContext.seen.append(("deepen", packed.npairs, k, first, last, no_len))
        return np.array([1.0, 4.0]), np.array([1, 1], np.uint8), np.array([-1, -1], np.int32), 2, [first, 2 * first]

    def close(self):
        pass


def test_engine_client_forwards_the_cutoff_calls(monkeypatch):
    """EngineClient.run_cutoff / deepen reach the serving process's Context (a forked child served by its parent, or a
    worker) and bring its arrays back."""
    import threading
    from multiprocessing import Pipe
    monkeypatch.setattr(sedgpu, "Context", _ServedContext)
    _ServedContext.seen = []
    c2s_r, c2s_w = Pipe(duplex=False)
    s2c_r, s2c_w = Pipe(duplex=False)
    th = threading.Thread(target=sedgpu._serve, args=(c2s_r, s2c_w, 0), daemon=True)
    th.start()
    client = sedgpu.EngineClient(0)
    client._tx, client._rx = c2s_w, s2c_r
    packed = sedgpu.PackedPairs([np.zeros(3, np.uint8)] * 2, [np.ones(4, np.uint8)] * 2)
    d, ii, ln, hits = client.run_cutoff(packed, 2.5)
    assert d.tolist() == [1.0, math.inf] and ii.tolist() == [1, 0] and ln.tolist() == [-1, -1] and hits == 1
    d, ii, ln, hits, cuts = client.deepen(packed, 2, 3.0, 50.0)
    assert d.tolist() == [1.0, 4.0] and hits == 2 and cuts == [3.0, 6.0]
    assert _ServedContext.seen == [("run_cutoff", 2, 2.5, True), ("deepen", 2, 2, 3.0, 50.0, True)]
    with pytest.raises(sedgpu.SedError, match="unknown engine request"):
        client._call("no_such_call")
    c2s_w.close()  # the client's end closes: the serving loop ends
    th.join(5)
    assert not th.is_alive()
    client._tx = client._rx = None
