"""CPU: the host side of fit search (sed_fit_search): the planner through sed_fit_plan (scale, window,
lanes, the cost models it refuses), the definition of a hit restated in pure Python and checked against brute force
over every substring with the C oracle as G, wfsearch.fit_search with that restatement standing in for the engine, and
the forked-client request against a fake context."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import oracle
import sedcost
import sedgpu

E_RANGE = -4


def fit_definition(sub, ins, dele, p, t):
    """(dist, start, end) of pattern codes p in text codes t under sub[a][b] = cost(a -> b): the DP of sed.h, rows =
    the pattern, D[0][j] = 0, D[i][0] = i delete, every cell the lexicographic minimum of (D, -start) over insert
    (left), delete (up) and update (diagonal), then the first strict minimum of the last row."""
    n = len(t)
    row = [(0.0, -j) for j in range(n + 1)]
    for i, a in enumerate(p, 1):
        cost = sub[a]
        cur = [(i * dele, 0)]
        for j in range(1, n + 1):
            up, dg, left = row[j], row[j - 1], cur[j - 1]
            cur.append(min((left[0] + ins, left[1]), (up[0] + dele, up[1]), (dg[0] + cost[t[j - 1]], dg[1])))
        row = cur
    end = min(range(n + 1), key=lambda j: (row[j][0], j))
    return row[end][0], -row[end][1], end


def fit_definition_str(table, pattern, text):
    """fit_definition over strings under a cost table of the golden files' form."""
    plan = sedcost.build_plan(table, [pattern], [text])
    return fit_definition(plan.sub.tolist(), plan.ins, plan.dele, plan.encode(pattern).tolist(), plan.encode(text).tolist())


def costs_of(table, alphabet):
    """The sed_set_costs arguments of `table` over `alphabet`."""
    plan = sedcost.build_plan(table, [alphabet], [alphabet])
    return (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)


def unit_costs(K, ins, dele, sub=1.0):
    return (K, np.where(np.eye(K) > 0, 0.0, sub), np.eye(K, dtype=np.uint8), float(ins), 0, float(dele), 0)


@pytest.fixture(scope="module")
def wfsearch():
    cwd = os.getcwd()
    os.chdir(GOLDEN)  # the drop-in module reads its cost tables from the working directory when it is imported
    try:
        return importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("name", ["costs.json", "user_costs.json"])
def test_scale_of_the_golden_tables(name):
    t = load_golden(name)
    assert sedgpu.fit_plan(costs_of(t, "ACGU"), {}, [28], [100])["scale"] == 1
    assert sedgpu.fit_plan(costs_of(t, "ACGUN"), {}, [28], [100])["scale"] == 4


def test_window():
    for P in (1, 7, 32):
        assert sedgpu.fit_plan(unit_costs(4, 1, 1), {}, [P, 1], [50, 9])["W"] == 2 * P
        got = sedgpu.fit_plan(costs_of(load_golden("user_costs.json"), "ACGU"), {}, [P], [50])
        assert got["W"] == P + (3 * P) // 2  # insert 2, delete 3
    assert sedgpu.fit_plan(unit_costs(4, 0, 1), {}, [5], [50])["W"] == -1


def _refused(costs, len_p, len_t=(10,)):
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.fit_plan(costs, {}, list(len_p), list(len_t))
    return ex.value.code


def test_refused_cost_models():
    t = load_golden("costs.json")
    assert t["update"]["R"]["D"] == 0.66
    assert _refused(costs_of(t, "ARD"), [5]) == E_RANGE          # not dyadic
    assert sedgpu.fit_plan(costs_of(t, "ARG"), {}, [5], [10])["scale"] == 2  # (R -> A, G: 0.5)
    assert _refused(unit_costs(9, 1, 1), [5]) == E_RANGE         # 9 symbols
    assert _refused(unit_costs(4, 1, 1), [33]) == E_RANGE        # P = 33
    assert _refused(unit_costs(4, 1, 1), [4, 33], [10, 10]) == E_RANGE
    assert _refused(unit_costs(4, 1, 3000), [32]) == E_RANGE     # P * delete * S = 96000 > 65535
    assert _refused(unit_costs(4, 1, 2100.25), [32]) == E_RANGE   # S = 4: 32 * 8401 > 65535
    assert _refused(unit_costs(4, 1, 1), [5], [-1]) == -1        # (a bad argument is not a range error)


def test_lane_count_under_a_chunk_override():
    rng = np.random.default_rng(7)
    lt = rng.integers(0, 900, size=40).tolist() + [0, 1, 63, 64, 65]
    lp = rng.integers(1, 33, size=len(lt)).tolist()
    for c in (1, 7, 64, 65, 200, 5000):
        got = sedgpu.fit_plan(unit_costs(4, 1, 1), {sedgpu.SED_OPT_FIT_CHUNK: c}, lp, lt)
        assert got["lanes"] == sum(-(-(n + 1) // c) for n in lt) and got["chunk"] == c
        assert got["nominal_cells"] == sum(p * n for p, n in zip(lp, lt))
        assert got["cells"] >= got["nominal_cells"]
    one = sedgpu.fit_plan(unit_costs(4, 1, 1), {sedgpu.SED_OPT_FIT_CHUNK: 5000}, lp, lt)
    assert one["cells"] == one["nominal_cells"]  # one lane per text: no warm-up


def test_lane_records_tile_every_text():
    """sed_fit_lanes: a pair's lanes own [0, n + 1) without gap or overlap, start min(c0, W) columns early rounded to
    a 4-symbol word of the text, and run to their last owned column."""
    rng = np.random.default_rng(11)
    lt = rng.integers(0, 900, size=40).tolist() + [0, 1, 63, 64, 65]
    lp = rng.integers(1, 33, size=len(lt)).tolist()
    costs = costs_of(load_golden("user_costs.json"), "ACGU")
    for c in (0, 1, 7, 64, 200, 5000):
        opts = {sedgpu.SED_OPT_FIT_CHUNK: c}
        plan = sedgpu.fit_plan(costs, opts, lp, lt)
        lanes, par = sedgpu.fit_lanes(costs, opts, lp, lt)
        assert len(lanes["pair"]) == plan["lanes"] and (par["ins"], par["del"]) == (2, 3)
        W = plan["W"]
        for q, n in enumerate(lt):
            at = np.flatnonzero(lanes["pair"] == q)
            c0, cnt, lead = lanes["c0"][at], lanes["cnt"][at], lanes["lead"][at]
            assert c0[0] == 0 and (c0[1:] == c0[:-1] + cnt[:-1]).all() and c0[-1] + cnt[-1] == n + 1
            assert (lanes["plen"][at] == lp[q]).all() and not lanes["pat"][at].any()
            assert (4 * lanes["tw"][at] == c0 - lead).all() and (lanes["nsteps"][at] == lead + cnt - 1).all()
            assert ((lead >= np.minimum(c0, W)) & (lead < np.minimum(c0, W) + 4) & (lead <= c0)).all()
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.fit_lanes(unit_costs(9, 1, 1), {}, [5], [10])
    assert ex.value.code == E_RANGE


def test_insert_zero_runs_one_lane_per_pair():
    lt = [0, 5, 3000, 40000]
    for opts in ({}, {sedgpu.SED_OPT_FIT_CHUNK: 16}):
        got = sedgpu.fit_plan(unit_costs(4, 0, 1), opts, [8] * len(lt), lt)
        assert got["lanes"] == len(lt) and got["cells"] == got["nominal_cells"]


def test_auto_chunk_rule():
    """Few long texts are split, never into chunks shorter than W; many texts are not split at all."""
    few = sedgpu.fit_plan(costs_of(load_golden("user_costs.json"), "ACGU"), {}, [28] * 8192, [4096] * 8192)
    assert few["W"] == 70 and few["chunk"] >= few["W"] and few["lanes"] > 8192
    assert few["cells"] <= 2.1 * few["nominal_cells"]
    tiny = sedgpu.fit_plan(unit_costs(4, 1, 1), {}, [32] * 16, [200] * 16)
    assert tiny["chunk"] >= tiny["W"] == 64
    many = sedgpu.fit_plan(unit_costs(4, 1, 1), {}, [28] * 200000, [30] * 200000)
    assert many["lanes"] == 200000 and many["chunk"] == 0


def _brute(costs, p, t):
    """The definition by brute force: G(s, e) of every substring from the C oracle."""
    n = len(t)
    spans = [(s, e) for e in range(n + 1) for s in range(e + 1)]
    packed = sedgpu.PackedPairs([p] * len(spans), [t[s:e] for s, e in spans])
    d = oracle.batch(costs, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b, packed.off_b, packed.len_b,
                     packed.npairs)[0]
    best = min(d)
    end = min(e for (s, e), v in zip(spans, d) if v == best)
    start = max(s for (s, e), v in zip(spans, d) if v == best and e == end)
    return float(best), start, end


def _brute_cases():
    """The 120 small cases of test_definition_against_brute_force: (it, sub, insert, delete, pattern, text)."""
    rng = np.random.default_rng(2024)
    for it in range(120):
        K = int(rng.integers(2, 5))
        ins, dele = (float(rng.integers(0 if it % 7 == 0 else 1, 5)) / 2, float(rng.integers(0, 7)) / 2)
        sub = rng.integers(0, 9, size=(K, K)) / 4.0
        sub[np.eye(K) > 0] = 0
        p = rng.integers(0, K, size=int(rng.integers(1, 7))).astype(np.uint8)
        t = rng.integers(0, K, size=int(rng.integers(0, 25))).astype(np.uint8)
        if it % 3 == 0 and len(t) >= len(p):  # a planted copy
            at = int(rng.integers(0, len(t) - len(p) + 1))
            t[at:at + len(p)] = p
        yield it, sub, ins, dele, p, t


def test_definition_against_brute_force():
    for it, sub, ins, dele, p, t in _brute_cases():
        K = len(sub)
        costs = oracle.Costs(sub, np.zeros((K, K), np.uint8), ins, 0, dele, 0)
        assert fit_definition(sub.tolist(), ins, dele, p.tolist(), t.tolist()) == _brute(costs, p, t), (it, p, t)


def oracle_fit(sub, ins, dele, pats, texts, nthreads=1):
    """oracle.fit over lists of code arrays: [(dist, start, end)]."""
    K = len(sub)
    costs = oracle.Costs(sub, np.zeros((K, K), np.uint8), ins, 0, dele, 0)
    pk = sedgpu.PackedPairs(pats, texts)
    d, s, e = oracle.fit(costs, pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b, pk.npairs, nthreads)
    return list(zip(d.tolist(), s.tolist(), e.tolist()))


def test_oracle_fit_on_the_brute_force_cases():
    """The compiled oracle equals the pure-Python definition and the brute force over every substring, exactly."""
    for it, sub, ins, dele, p, t in _brute_cases():
        K = len(sub)
        costs = oracle.Costs(sub, np.zeros((K, K), np.uint8), ins, 0, dele, 0)
        got = oracle_fit(sub, ins, dele, [p], [t])[0]
        assert got == fit_definition(sub.tolist(), ins, dele, p.tolist(), t.tolist()), (it, p, t)
        assert got == _brute(costs, p, t), (it, p, t)


def test_oracle_fit_against_the_definition_on_random_pairs():
    """3000 pairs in 60 cost models: K 2..8, P 1..40 (past the kernel's 32 on purpose), texts 0..200, costs multiples of
    1/4 with insert = 0, delete = 0, nonzero diagonals and substitutions dearer than insert + delete among them.  Every
    sum of such costs is exact in fp64, so equality is exact.  Two oracle threads: the batch driver's split."""
    rng = np.random.default_rng(4040)
    seen = {"ins0": 0, "del0": 0, "diag": 0, "dear": 0, "P>32": 0}
    for model in range(60):
        K = 2 + model % 7
        ins = 0.0 if model % 6 == 0 else float(rng.integers(1, 9)) / 4
        dele = 0.0 if model % 6 == 1 else float(rng.integers(1, 13)) / 4
        sub = rng.integers(0, 4 * int(ins + dele + 2) + 1, size=(K, K)) / 4.0  # up to about insert + delete + 2
        if model % 3:
            sub[np.eye(K) > 0] = 0
        seen["ins0"] += ins == 0
        seen["del0"] += dele == 0
        seen["diag"] += bool(np.diag(sub).any())
        seen["dear"] += bool((sub > ins + dele).any())
        pats, texts = [], []
        for it in range(50):
            P = (1, 32, 33, 40)[it] if it < 4 else int(rng.integers(1, 41))
            n = (0, 1, 200)[it] if it < 3 else int(rng.integers(0, 201))
            p = rng.integers(0, K, size=P).astype(np.uint8)
            t = rng.integers(0, K, size=n).astype(np.uint8)
            if it % 2 and n >= P:  # a planted copy, some of them with a symbol changed
                at = int(rng.integers(0, n - P + 1))
                t[at:at + P] = p
                if it % 4 == 1:
                    t[at + int(rng.integers(0, P))] = rng.integers(0, K)
            seen["P>32"] += P > 32
            pats.append(p)
            texts.append(t)
        got = oracle_fit(sub, ins, dele, pats, texts, nthreads=2)
        subl = sub.tolist()
        want = [fit_definition(subl, ins, dele, p.tolist(), t.tolist()) for p, t in zip(pats, texts)]
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (model, bad[:3])
    assert all(v >= 5 for v in seen.values()), seen


def test_fit_search_module(wfsearch):
    table = load_golden("costs.json")
    seen = []

    def fit_fn(patterns, texts, user_cost):
        seen.append((list(patterns), list(texts), user_cost))
        return [fit_definition_str(table, a, b) for a, b in zip(patterns, texts)]

    docs = ["GGGACGUACGG", "UUUU", "", "ACGAACGU", "CCACGUA"]
    got = wfsearch.fit_search("ACGUA", docs, fit_fn=fit_fn)
    assert seen == [(["ACGUA"] * 5, docs, False)]
    assert got == [("GGGACGUACGG", 1.0, 3, 8), ("UUUU", 1 / 5, 0, 1), ("", 1 / 6, 0, 0), ("ACGAACGU", 1 / 2, 0, 4),
                   ("CCACGUA", 1.0, 2, 7)]
    assert all(len(h) == 4 for h in got)  # scripts=False: (sequence, score, start, end)
    assert wfsearch.fit_search("ACGUA", docs, max_dist=1, fit_fn=fit_fn) == [got[0], got[3], got[4]]
    assert wfsearch.fit_search("ACGUA", docs, max_dist=0, fit_fn=fit_fn) == [got[0], got[4]]
    assert wfsearch.fit_search("ACGUA", [], fit_fn=fit_fn) == []
    assert wfsearch.fit_search("ACGUA", docs, max_dist=-1, scripts=True, fit_fn=fit_fn) == []

    class Collection:
        def find(self, query):
            return [{"sequence": s} for s in docs]

    assert wfsearch.fit_search("ACGUA", Collection(), fit_fn=fit_fn) == got


class _ServedContext:
    """Stands in for sedgpu.Context behind sedgpu._serve."""
    seen = []

    def __init__(self, device=0):
        self.device = device

    def fit(self, packed):
        _ServedContext.seen.append(("fit", packed.npairs, packed.len_a.tolist(), packed.len_b.tolist()))
        return np.array([0.0, 1.5]), np.array([2, 0], np.int32), np.array([5, 4], np.int32)

    def close(self):
        pass


def test_engine_client_forwards_fit(monkeypatch):
    """EngineClient.fit reaches the serving process's Context (a forked child served by its parent, or a worker) and
    brings its arrays back."""
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
    packed = sedgpu.PackedPairs([np.zeros(3, np.uint8)] * 2, [np.ones(9, np.uint8), np.ones(4, np.uint8)])
    d, s, e = client.fit(packed)
    assert d.tolist() == [0.0, 1.5] and s.tolist() == [2, 0] and e.tolist() == [5, 4]
    assert _ServedContext.seen == [("fit", 2, [3, 3], [9, 4])]
    c2s_w.close()  # the client's end closes: the serving loop ends
    th.join(5)
    assert not th.is_alive()
    client._tx = client._rx = None


def test_fit_batch_goes_through_the_context(wfsearch, monkeypatch):
    SED = wfsearch.SED

    class Fake:
        def set_costs(self, plan):
            self.K = plan.K

        def fit(self, packed):
            self.lens = (packed.len_a.tolist(), packed.len_b.tolist())
            return np.array([0.0, 2.0]), np.array([1, 0], np.int32), np.array([4, 0], np.int32)

    fake = Fake()
    monkeypatch.setattr(sedgpu, "context", lambda: fake)
    assert SED.fit_batch(["ACG", "UU"], ["AACGA", ""]) == [(0.0, 1, 4), (2.0, 0, 0)]
    assert fake.lens == ([3, 2], [5, 0]) and fake.K == 4
    assert SED.fit_batch([], []) == []
    with pytest.raises(KeyError):
        SED.fit_batch(["AC!"], ["ACGU"])  # the reference's KeyError for a symbol the table does not know
