"""CPU: the host side of fit search's fp64 route (sed_fit_search_f64): what the planner serves and
refuses and which route sed_fit_route names; the lane records under forced, automatic and one-lane chunking; the
word-for-word model of the kernel's lane (fit_f64_cases.run_lanes) run over the planner's own lane records and reduced
as the runtime reduces, equal to oracle.fit to the bit, which is the test of the window argument; the hits reference
pinned against oracle.fit and the pure-Python row; wfsearch's route keyword over index_fn / fit_fn engines; the ABI."""
import ctypes

import numpy as np
import pytest

import oracle  # noqa: F401
import sedgpu
import fit_f64_cases as fc
from test_fit_host import E_RANGE, fit_definition_str, unit_costs, wfsearch  # noqa: F401  (a fixture)
from test_fit_hits_host import hits_row
from conftest import load_golden

CHUNK = sedgpu.SED_OPT_FIT_CHUNK
OPTIONS = [("c8", {CHUNK: 8}), ("c72", {CHUNK: 72}), ("auto", {}), ("one", {CHUNK: 1 << 30})]


def _code(fn, *args):
    with pytest.raises(sedgpu.SedError) as ex:
        fn(*args)
    return ex.value.code


@pytest.mark.parametrize("name,plan", fc.f64_only_tables(), ids=[n for n, _ in fc.f64_only_tables()])
def test_integer_refusals_are_served(name, plan):
    lp, lt = [32, 5], [100, 40]
    assert _code(sedgpu.fit_plan, plan.costs(), {}, lp, lt) == E_RANGE
    got = sedgpu.fit_f64_plan(plan.costs(), {}, lp, lt)
    assert got["scale"] == 0 and got["lanes"] >= 2 and got["nominal_cells"] == 32 * 100 + 5 * 40
    route, why = sedgpu.fit_route(plan.costs(), {}, lp, lt)
    assert route == "f64" and why.startswith("fit search: ")
    words = {n: w for n, _, w in fc.integer_limit_tables()}
    words.update(costs15="15 symbols (at most 8)", user15="15 symbols (at most 8)", unit9="9 symbols (at most 8)",
                 unit16="16 symbols (at most 8)", rounding="not all multiples", sub_0="not all multiples")
    assert words[name] in why, why


@pytest.mark.parametrize("name,alphabet", [("costs.json", "ACGU"), ("user_costs.json", "ACGU"), ("costs.json", "ACGUN")])
def test_route_prefers_the_integer_kernels(name, alphabet):
    plan = fc.golden_dyadic(name, alphabet)
    assert sedgpu.fit_route(plan.costs(), {}, [28, 5], [4096, 0]) == ("int", "")
    assert sedgpu.fit_f64_plan(plan.costs(), {}, [28], [4096])["scale"] == 0  # (the fp64 route serves them too)


def test_refused_by_both():
    for costs, lp, both in ((unit_costs(17, 1, 1), [5], ("17 symbols (at most 8)", "17 symbols (at most 16)")),
                            (unit_costs(4, -1.0, 1), [5], ("not all multiples", "insert = -1 is not a finite cost >= 0")),
                            (unit_costs(4, 1, 1), [0], ("pattern length 0 outside 1..32",) * 2),
                            (unit_costs(4, 1, 1), [33], ("pattern length 33 outside 1..32",) * 2)):
        assert _code(sedgpu.fit_plan, costs, {}, lp, [10]) == E_RANGE
        assert _code(sedgpu.fit_f64_plan, costs, {}, lp, [10]) == E_RANGE
        assert _code(sedgpu.fit_f64_lanes, costs, {}, lp, [10]) == E_RANGE
        assert _code(sedgpu.fit_index_f64_plan, costs, {}, lp, [10]) == E_RANGE
        route, why = sedgpu.fit_route(costs, {}, lp, [10])
        assert route is None and both[0] in why.split("; ")[0], why
        assert both[1] in why.split("; ")[1], why
    neg = fc.unit(4)
    neg.sub[1, 2] = -0.5
    assert "cost(1 -> 2) = -0.5" in sedgpu.fit_route(neg.costs(), {}, [5], [10])[1]
    nz = fc.unit(9)
    nz.sub[0, 0] = -0.0  # -0.0 is a cost: normalised, not refused
    assert sedgpu.fit_route(nz.costs(), {}, [5], [10])[0] == "f64"


def test_window_and_one_lane_rule():
    r = fc.rounding_table()  # P delete / insert = 2 P exactly: W = P + 2 P + 2
    for P in (1, 8, 32):
        got = sedgpu.fit_f64_plan(r.costs(), {CHUNK: 8}, [P], [300])
        assert (got["W"], got["one_lane"], got["chunk"]) == (3 * P + 2, 0, 8)
    u = fc.unit(9, 1.0, 0.0)  # delete = 0: W = P + 2
    assert sedgpu.fit_f64_plan(u.costs(), {CHUNK: 8}, [5], [300])["W"] == 7
    for plan, why in ((fc.unit(9, 0.0, 1.0), 1), (fc.unit(9, 1e-300, 1.0), 2), (fc.unit(9, 1.0, 1e300), 2),
                      (fc.unit(9, 1e-7, 1.0), 2)):  # (32 / 1e-7 > 2^20)
        got = sedgpu.fit_f64_plan(plan.costs(), {CHUNK: 8}, [32, 3], [300, 70000])
        assert (got["W"], got["one_lane"], got["chunk"], got["lanes"]) == (-1, why, 0, 2)


def _check_lanes(lanes, plan_out, len_p, len_t):
    W = plan_out["W"]
    pairs = lanes["pair"].tolist()
    assert pairs == sorted(pairs) and len(pairs) == plan_out["lanes"]
    first = [pairs.index(p) for p in range(len(len_t))] + [len(pairs)]  # first[] of the plan
    for p, n in enumerate(len_t):
        sl = slice(first[p], first[p + 1])
        c0, cnt, lead, nsteps, tw = (lanes[k][sl] for k in ("c0", "cnt", "lead", "nsteps", "tw"))
        assert c0[0] == 0 and (c0[1:] == c0[:-1] + cnt[:-1]).all() and c0[-1] + cnt[-1] == n + 1  # tiles 0..n once
        assert (cnt >= 1).all() and (lanes["plen"][sl] == len_p[p]).all()
        if W >= 0:  # a lane starts at the text's border column or warms up over at least the documented window
            assert (lead[c0 <= W] == c0[c0 <= W]).all() and (lead[c0 > W] >= W).all() and (lead <= W + 3).all()
        else:
            assert len(c0) == 1 and lead[0] == 0
        assert ((c0 - lead) % 4 == 0).all() and (tw == (c0 - lead) // 4).all()
        assert (nsteps == c0 + cnt - 1 - (c0 - lead)).all()
    return first


@pytest.mark.parametrize("oname,options", OPTIONS, ids=[n for n, _ in OPTIONS])
def test_lane_records(oname, options):
    plan = fc.rounding_table()
    len_p, len_t = [5, 32, 1, 8], [0, 300, 129, 64]
    out = sedgpu.fit_f64_plan(plan.costs(), options, len_p, len_t)
    lanes = sedgpu.fit_f64_lanes(plan.costs(), options, len_p, len_t)
    _check_lanes(lanes, out, len_p, len_t)
    assert out["W"] == 32 * 3 + 2
    if oname == "auto":  # four pairs are far from filling the device: the chunk is the target's, but never below W
        assert (out["chunk"], out["lanes"]) == (98, 1 + 4 + 2 + 1)
    if oname == "one":
        assert out["lanes"] == 4
    # the index's lanes equal the per-call lanes of the cross product, query-major
    qs, ts = [5, 32], [0, 300, 129]
    il = sedgpu.fit_index_f64_lanes(plan.costs(), options, qs, ts)
    pl = sedgpu.fit_f64_lanes(plan.costs(), options, [q for q in qs for _ in ts], ts * len(qs))
    for k in sedgpu.FIT_LANE_FIELDS:
        assert (il[k] == pl[k]).all(), k
    ip = sedgpu.fit_index_f64_plan(plan.costs(), options, qs, ts)
    pp = sedgpu.fit_f64_plan(plan.costs(), options, [q for q in qs for _ in ts], ts * len(qs))
    assert ip == pp


def test_insert_zero_runs_one_lane_whatever_the_length():
    plan = fc.unit(4, 0.0, 1.0)
    assert _code(sedgpu.fit_plan, plan.costs(), {}, [8], [70000]) == E_RANGE  # the 16-bit start field
    route, why = sedgpu.fit_route(plan.costs(), {}, [8], [70000])
    assert route == "f64" and "span more than 65535" in why
    for options in ({}, {CHUNK: 8}):
        lanes = sedgpu.fit_f64_lanes(plan.costs(), options, [8, 3], [70000, 10])
        assert lanes["cnt"].tolist() == [70001, 11] and lanes["lead"].tolist() == [0, 0]
        assert sedgpu.fit_f64_plan(plan.costs(), options, [8, 3], [70000, 10])["one_lane"] == 1


def _model_cases(plan, options, rng, P):
    """Texts of every length 0..200 (random), and for lengths 100 and 200 copies planted to end on every seam of the
    planner's own lanes, on column n and (the empty match) column 0."""
    K = plan.K
    p = rng.integers(0, K, size=P).astype(np.uint8)
    texts = [rng.integers(0, K, size=n).astype(np.uint8) for n in range(201)]
    for n in (100, 200):
        seams = fc.seam_columns(sedgpu.fit_f64_lanes(plan.costs(), options, [P], [n]))
        for e in seams + [n]:
            texts.append(fc.plant(rng, K, p, n, [e]))
        texts.append(fc.plant(rng, K, p, n, seams))
    texts.append(np.full(150, p[0], np.uint8))  # ties: equal D at many starts
    return [p] * len(texts), texts


@pytest.mark.parametrize("tname", ["rounding", "costs15"])
@pytest.mark.parametrize("chunk", [8, 72])
def test_lane_model_equals_the_oracle(tname, chunk):
    """The window argument, tested: the kernel's lane, run over the planner's lane records (synthetic border column,
    warm-up over `lead` columns, owned columns, first strict minimum) and reduced in chunk order, gives oracle.fit's
    (dist, start, end) exactly, dist compared as float64 with ==."""
    plan = dict(fc.f64_only_tables())[tname]
    options = {CHUNK: chunk}
    rng = np.random.default_rng(chunk)
    for P in (1, 3, 8, 32):
        pats, texts = _model_cases(plan, options, rng, P)
        len_p, len_t = [len(p) for p in pats], [len(t) for t in texts]
        out = sedgpu.fit_f64_plan(plan.costs(), options, len_p, len_t)
        lanes = sedgpu.fit_f64_lanes(plan.costs(), options, len_p, len_t)
        assert out["chunk"] == chunk and out["lanes"] > len(texts)
        best, _ = fc.run_lanes(plan, lanes, pats, texts)
        got = fc.reduce_lanes(best, lanes, len(texts))
        want = fc.oracle_fit(plan, pats, texts)
        assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)


def test_hits_reference_is_the_definition():
    rng = np.random.default_rng(3)
    for tname in ("rounding", "costs15", "sub_0"):
        plan = dict(fc.f64_only_tables())[tname]
        pats = [rng.integers(0, plan.K, size=P).astype(np.uint8) for P in (1, 4, 9, 32)]
        texts = [fc.plant(rng, plan.K, p, n, [n // 2, n]) for p, n in zip(pats, (0, 7, 40, 90))]
        every = fc.rows_reference(plan, pats, texts, np.inf)
        assert len(every) == sum(len(t) + 1 for t in texts)
        want = fc.oracle_fit(plan, pats, texts)
        for k, (p, t) in enumerate(zip(pats, texts)):
            row = [(d, s) for q, s, e, d in every if q == k]
            assert row == hits_row(plan.sub.tolist(), plan.ins, plan.dele, p.tolist(), t.tolist())
            d = min(v for v, _ in row)
            e = next(j for j, (v, _) in enumerate(row) if v == d)  # the first strict minimum
            assert (d, row[e][1], e) == want[k]
        T = sorted(d for _, _, _, d in every)[len(every) // 3]
        assert fc.rows_reference(plan, pats, texts, T) == [h for h in every if h[3] <= T]


class _OracleIndex:
    """An index_fn engine that serves the definition through the C oracle and records which calls it got."""

    def __init__(self, table, seqs, user_cost, f64=False):
        self.table, self.seqs, self.f64, self.calls = table, list(seqs), f64, []

    def _search(self, patterns):
        return [[fit_definition_str(self.table, p, t) for t in self.seqs] for p in patterns]

    def search(self, patterns):
        self.calls.append("search")
        if len(set("".join(self.seqs) + "".join(patterns))) > 8:
            raise sedgpu.SedError("fit index: the texts and these patterns have 9 symbols (fit search serves at most 8)")
        return self._search(patterns)

    def search_f64(self, patterns):
        self.calls.append("search_f64")
        return self._search(patterns)

    def _hits(self, patterns, max_dist):
        import sedcost
        out = []
        for q, p in enumerate(patterns):
            for d, t in enumerate(self.seqs):
                pl = sedcost.build_plan(self.table, [p], [t])
                row = hits_row(pl.sub.tolist(), pl.ins, pl.dele, pl.encode(p).tolist(), pl.encode(t).tolist())
                out += [(q, d, s, e, v) for e, (v, s) in enumerate(row) if v <= max_dist]
        return out

    def hits(self, patterns, max_dist):
        self.calls.append("hits")
        return self._hits(patterns, max_dist)

    def hits_f64(self, patterns, max_dist):
        self.calls.append("hits_f64")
        return self._hits(patterns, max_dist)

    def close(self):
        pass


def test_wfsearch_routes(wfsearch):
    table = load_golden("costs.json")
    seen = []

    def fit_fn(patterns, texts, user_cost, f64=False):
        seen.append("f64" if f64 else "int")
        return [fit_definition_str(table, a, b) for a, b in zip(patterns, texts)]

    acgu = ["GGGACGUACGG", "UUUU", "", "ACGAACGU"]
    iupac = acgu + ["ACGDACGU", "RYKMSWBVHN"]
    want = {tuple(d): [(s,) + (1 / (1 + v), a, b) for s, (v, a, b) in
                       zip(d, (fit_definition_str(table, "ACGUA", s) for s in d))] for d in (acgu, iupac)}
    assert wfsearch.fit_search("ACGUA", acgu, fit_fn=fit_fn) == want[tuple(acgu)] and seen == ["int"]
    assert wfsearch.fit_search("ACGUA", acgu, fit_fn=fit_fn, route="auto") == want[tuple(acgu)] and seen[-1] == "int"
    assert wfsearch.fit_search("ACGUA", acgu, fit_fn=fit_fn, route="f64") == want[tuple(acgu)] and seen[-1] == "f64"
    assert wfsearch.fit_search("ACGUA", iupac, fit_fn=fit_fn, route="auto") == want[tuple(iupac)] and seen[-1] == "f64"
    assert wfsearch.fit_search("ACGUA", acgu + ["ACGDA"], fit_fn=fit_fn, route="auto")[-1][0] == "ACGDA" and seen[-1] == "f64"
    assert wfsearch.fit_route(["ACGUA"], acgu) == "int" and wfsearch.fit_route(["ACGUA"], acgu + ["D"]) == "f64"
    with pytest.raises(ValueError):
        wfsearch.fit_search("ACGUA", acgu, fit_fn=fit_fn, route="fp64")
    # the pre-route three-argument engines keep working with the default
    assert wfsearch.fit_search("ACGUA", acgu, fit_fn=lambda p, t, u: [fit_definition_str(table, a, b) for a, b in zip(p, t)]) \
        == want[tuple(acgu)]

    made = []

    def index_fn(seqs, user_cost, f64=False):
        made.append(_OracleIndex(table, seqs, user_cost, f64))
        return made[-1]

    for docs in (acgu, iupac):
        ix = wfsearch.FitIndex(docs, index_fn=index_fn, route="auto")
        assert made[-1].f64 and ix.search("ACGUA") == want[tuple(docs)]
        assert made[-1].calls == ["search" if docs is acgu else "search_f64"]
        occ = ix.occurrences("ACGUA", 1.0, all_ends=True)
        assert made[-1].calls[-1] == ("hits" if docs is acgu else "hits_f64")
        assert ix.occurrences("ACGUA", 1.0, all_ends=True, route="f64") == occ and made[-1].calls[-1] == "hits_f64"
        assert wfsearch.fit_occurrences("ACGUA", docs, 1.0, all_ends=True, index_fn=index_fn, route="auto") == occ
        assert ix.search_many(["ACGUA", "GG"], route="f64")[0] == want[tuple(docs)]
    # the default route: a pre-route two-argument index_fn, and the refusal on the ninth symbol
    ix = wfsearch.FitIndex(iupac, index_fn=lambda seqs, user_cost: _OracleIndex(table, seqs, user_cost))
    with pytest.raises(sedgpu.SedError, match="9 symbols"):
        ix.search("ACGUA")


def test_string_edit_distance_index_over_15_symbols(wfsearch, monkeypatch):
    import StringEditDistance as SED
    monkeypatch.setattr(SED, "default_costs", load_golden("costs.json"))
    texts = ["ACGDACGU", "RYKMSWBVHN", "AGCUYRWSKMDVHBN"]
    seen = []

    class Engine:
        def __init__(self, codes, off, lens):
            seen.append(("built", int(codes.max()), lens.tolist()))

        def search_f64(self, plan, packed):
            seen.append(("search_f64", plan.K, packed.len_a.tolist()))
            z = np.zeros((packed.npairs, 3))
            return z, z.astype(np.int32), z.astype(np.int32)

        def hits_f64(self, plan, packed, max_dist):
            seen.append(("hits_f64", plan.K, max_dist))
            return np.zeros(0, sedgpu.FIT_HIT_DTYPE)

        def close(self):
            pass

    with pytest.raises(sedgpu.SedError, match="15 symbols"):
        SED.FitIndex(texts, engine=Engine)
    ix = SED.FitIndex(texts, engine=Engine, f64=True)
    assert seen == [("built", 14, [8, 10, 15])] and len(ix.symbols) == 15
    assert ix.plan(["ACGUA"]).K == 15
    assert ix.search_f64(["ACGUA", "DD"]) == [[(0.0, 0, 0)] * 3] * 2 and seen[-1] == ("search_f64", 15, [5, 2])
    assert ix.hits_f64(["ACGUA"], 1.5) == [] and seen[-1] == ("hits_f64", 15, 1.5)
    with pytest.raises(KeyError):  # the reference's KeyError for a symbol the table does not know
        ix.search_f64(["ACGZ"])
    with pytest.raises(sedgpu.SedError, match="17 symbols .*at most 16"):
        SED.FitIndex(texts, alphabet="12", engine=Engine, f64=True)


def test_abi_exports_and_binds_the_new_calls():
    names = {"sed_fit_search_f64", "sed_fit_index_search_f64", "sed_fit_index_hits_f64", "sed_fit_f64_plan", "sed_fit_f64_lanes",
             "sed_fit_index_f64_plan", "sed_fit_index_f64_lanes", "sed_fit_route"}
    lib = ctypes.CDLL(sedgpu.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert names <= {n for n, _, _ in sedgpu.SIGNATURES}
    for attr in ("fit_f64",):
        assert hasattr(sedgpu.Context, attr)
    assert hasattr(sedgpu.FitIndex, "search_f64") and hasattr(sedgpu.FitIndex, "hits_f64")
