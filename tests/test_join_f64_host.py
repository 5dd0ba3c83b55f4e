"""CPU: the fp64 route of the similarity join: its planner (sed_join_f64_plan, sed_join_f64_keep, sed_join_route), the
length skip against adversarial pairs through the C oracle, the kernel's lane restated in numpy, and the Python layers
over injected engines (StringEditDistance.JoinIndex, wfsearch.JoinIndex, wfsearch.neighbors, sedshard.neighbors)."""
import math
import re

import numpy as np
import pytest

import join_cases as jc
import join_f64_cases as jf
import sedgpu
import sedshard

INF = math.inf
NAMES = list(jf.tables()) + ["subnormal"]
_ADV = {}


def table_of(name):
    return jf.subnormal_table() if name == "subnormal" else jf.tables()[name]


def plan_of(name):
    return jc.plan_for(*table_of(name))


def adversarial(name):
    if name not in _ADV:
        _ADV[name] = jf.adversarial_min(plan_of(name))
        _ADV[name].setflags(write=False)
    return _ADV[name]


def f64_plan(plan, len_rows, len_cols, T, self_join=False, row_mask=None, col_mask=None, options=None):
    full = (1 << plan.K) - 1
    return sedgpu.join_f64_plan(jc.costs_of(plan), options or {}, len_rows, len_cols, self_join,
                                full if row_mask is None else row_mask, full if col_mask is None else col_mask, T)


@pytest.fixture(scope="module")
def wfsearch():
    return jc.import_shim("wfsearch")


# ---- the planner ----

def _edited(name, edit):
    plan = plan_of(name)
    edit(plan)
    return plan


def _set(plan, **kw):
    for k, v in kw.items():
        setattr(plan, k, v)


def test_envelope_and_refusal_texts():
    al17 = jf.AL16 + "Z"
    t17 = {"insert": 1.0, "delete": 1.0, "update": {a: {b: float(a != b) for b in al17} for a in al17}}
    cases = [(jc.plan_for(t17, al17), r"17 symbols \(at most 16\)"),
             (_edited("random16", lambda p: p.sub.__setitem__((2, 3), -0.5)), r"cost\(2 -> 3\) = -0\.5"),
             (_edited("random16", lambda p: p.sub.__setitem__((4, 1), math.nan)), r"cost\(4 -> 1\) = nan"),
             (_edited("random16", lambda p: p.sub.__setitem__((0, 9), INF)), r"cost\(0 -> 9\) = inf"),
             (_edited("random16", lambda p: _set(p, ins=-1.0)), r"insert = -1 "),
             (_edited("random16", lambda p: _set(p, dele=INF)), r"delete = inf ")]
    for plan, why in cases:
        with pytest.raises(sedgpu.SedError) as ei:
            f64_plan(plan, [5], [7], 1.0, row_mask=1, col_mask=1)
        assert ei.value.code == sedgpu.SED_E_RANGE, why
        route, text = sedgpu.join_route(jc.costs_of(plan), {}, [5], [7], False, 1, 1, 1.0)
        assert route is None and "; join (fp64): " in text
        assert re.search(why, text), (why, text)


@pytest.mark.parametrize("T", [math.nan, -1.0, -0.0001])
def test_bad_cutoff_is_arg_error(T):
    with pytest.raises(sedgpu.SedError) as ei:
        f64_plan(plan_of("costs15"), [5], [7], T)
    assert ei.value.code == sedgpu.SED_E_ARG
    with pytest.raises(sedgpu.SedError) as ei:
        sedgpu.join_f64_keep(1.0, 1.0, T)
    assert ei.value.code == sedgpu.SED_E_ARG


def test_code_outside_alphabet_and_length_over_32_are_arg_errors():
    plan = plan_of("costs15")
    for rm, cm in ((1 << 15, 1), (1, 1 << 20), (1 << 31, 1)):
        with pytest.raises(sedgpu.SedError) as ei:
            f64_plan(plan, [5], [7], 1.0, row_mask=rm, col_mask=cm)
        assert ei.value.code == sedgpu.SED_E_ARG
    for lr, lc in (([33], [5]), ([5], [33]), ([-1], [5])):
        with pytest.raises(sedgpu.SedError) as ei:
            f64_plan(plan, lr, lc, 1.0)
        assert ei.value.code == sedgpu.SED_E_ARG
    p16 = plan_of("random16")  # K = 16: every 4-bit code is inside
    assert f64_plan(p16, [5], [7], 1.0)["kernel"] == 3


def test_route_on_every_table():
    for name, (table, al, _) in jc.served_tables().items():
        plan = jc.plan_for(table, al)
        assert sedgpu.join_route(jc.costs_of(plan), {}, [5, 0], [7, 32], False, 1, 1, 1.0) == ("int", ""), name
    for name, (table, al, why) in jc.refused_tables().items():
        plan = jc.plan_for(table, al)
        route, text = sedgpu.join_route(jc.costs_of(plan), {}, [5], [7], False, 1, 1, 1.0)
        assert route == "f64" and re.search(why, text), name
    for name in NAMES:
        route, text = sedgpu.join_route(jc.costs_of(plan_of(name)), {}, [5], [7], True, 1, 1, INF)
        assert (route, text == "") == (("int", True) if name == "user_costs" else ("f64", False)), name
    # bad arguments are bad for both routes
    with pytest.raises(sedgpu.SedError) as ei:
        sedgpu.join_route(jc.costs_of(plan_of("costs15")), {}, [33], [7], False, 1, 1, 1.0)
    assert ei.value.code == sedgpu.SED_E_ARG


def test_waves_follow_the_launches():
    G = sedgpu.join_rows_per_group()
    plan = plan_of("costs15")
    assert f64_plan(plan, [5] * (2 * G + 2), [5] * 257, 1.0)["waves"] == 2 * 4 * 3
    assert f64_plan(plan, [5] * (2 * G + 2), [5] * 257, 1.0, options={sedgpu.SED_OPT_JOIN_ROWS: G + 1})["waves"] == 2 * 4 * 4
    assert f64_plan(plan, [5] * 3, [], 1.0) == {"scale": 0.0, "kernel": 3, "waves": 0, "scope": 0, "run": 0, "cells": 0.0}


# ---- the length skip ----

@pytest.mark.parametrize("name", NAMES)
def test_skip_never_drops_a_pair_the_oracle_keeps(name):
    """Exhaustively over n, m in 0..32: at every cutoff, every (n, m) the plan skips has oracle D > T for the pure-indel
    pairs, the match-then-inserts pairs and 200 random minimal-cost pairs of that class; the C rule is its Python
    restatement; run and cells are the brute-force count under the rule."""
    table, al = table_of(name)
    plan = plan_of(name)
    minD = adversarial(name)
    seqs = jf.mixed_set(name, 130)
    lens = [len(s) for s in seqs]
    skipped_somewhere = False
    for T in jf.cutoffs(table, minD):
        keep = sedgpu.join_f64_keep(plan.ins, plan.dele, T)
        assert np.array_equal(keep, jf.keep_rule(plan.ins, plan.dele, T)), T
        assert keep.diagonal().all()
        assert (minD[~keep] > T).all(), (name, T, np.argwhere(~keep & ~(minD > T))[:3])
        skipped_somewhere |= bool((~keep).any())
        if T == INF:
            assert keep.all()
        for self_join in (False, True):
            p = f64_plan(plan, lens[:40] if self_join else lens[40:], lens, T, self_join)
            want = jf.keep_count(lens[:40] if self_join else lens[40:], lens, keep, list(range(40)) if self_join else None)
            assert (p["run"], p["cells"]) == want, (name, T, self_join)
            assert p["scope"] == (40 * 130 - 40 if self_join else 90 * 130)
    assert skipped_somewhere


def test_the_rule_skips_no_less_than_a_wide_margin_allows():
    """The deflation is 2^-40: a bound a part in 10^9 above the cutoff is skipped, one below it is kept."""
    keep = sedgpu.join_f64_keep(1.0, 1.0, 2.0)
    assert keep[5, 7] and keep[7, 5] and not keep[5, 8] and not keep[8, 5]
    keep = sedgpu.join_f64_keep(0.66, 0.66, 3 * 0.66)
    assert keep[4, 7] and not keep[4, 8]
    keep = sedgpu.join_f64_keep(0.66, 0.66, 3 * 0.66 * (1 - 1e-9))
    assert not keep[4, 7]


def test_the_rounded_sum_below_the_product():
    """insert = 0.1: "A" against "A" + ten other symbols is 0.9999999999999999 although fl(10 * 0.1) = 1.0.  The pair's
    class (1, 11) is computed at nextafter(1.0, 0), where the pair is a hit, and one step further down, where it is
    none; a product bound would have skipped it at both."""
    table, al = jf.rounding_table()
    plan = jc.plan_for(table, al)
    D = jc.oracle_matrix(plan, ["A"], ["A" + "CGUCGUCGUC"])
    below = float(np.nextafter(1.0, 0.0))
    assert 10 * 0.1 == 1.0 and D[0, 0] == below
    assert jf.lane_matrix(plan, ["A"], ["A" + "CGUCGUCGUC"])[0, 0] == below
    lower = float(np.nextafter(below, 0.0))
    for T, hit in ((below, True), (lower, False)):
        assert sedgpu.join_f64_keep(0.1, 0.2, T)[1, 11]
        assert f64_plan(plan, [1], [11], T)["run"] == 1
        assert len(jf.expected_hits_f64(D, T)) == int(hit)
    assert not sedgpu.join_f64_keep(0.1, 0.2, 0.99)[1, 11]


def test_skip_hypotheses():
    """Never on a path the argument does not cover: n = 0 or m = 0 use the exact product, subnormal and overflowing
    products and max_dist = +inf are never skipped."""
    tiny = 5e-324
    keep = sedgpu.join_f64_keep(3 * tiny, 7 * tiny, 10 * tiny)
    assert keep[1:, 1:].all()  # every bound is subnormal
    assert keep[0, :4].tolist() == [True, True, True, True] and not keep[0, 4]  # 4 * 3 q > 10 q, exactly
    assert keep[1, 0] and not keep[2, 0]
    keep = sedgpu.join_f64_keep(1e308, 1e308, 1.1e308)
    assert keep[1, 2] and keep[1, 3] and keep[1, 11]  # 2 * 1e308 and 10 * 1e308 overflow: never skipped
    keep = sedgpu.join_f64_keep(1e307, 1e307, 1.1e307)
    assert keep[1, 2] and not keep[1, 3]
    assert sedgpu.join_f64_keep(1.0, 1.0, INF).all()
    assert sedgpu.join_f64_keep(0.0, 0.0, 0.0).all()
    assert sedgpu.join_f64_keep(-0.0, 1.0, 0.0)[0].all()


# ---- the kernel's lane, restated ----

@pytest.mark.parametrize("name", NAMES)
def test_lane_restatement_equals_the_oracle(name):
    plan = plan_of(name)
    seqs = jf.mixed_set(name, 130)
    D = jc.oracle_matrix(plan, seqs, seqs)
    L = jf.lane_matrix(plan, seqs, seqs)
    assert np.array_equal(L.view(np.uint64), D.view(np.uint64))
    edge = jf.edge_length_set("costs15", 40) if name == "costs15" else seqs[:10] + ["", seqs[0][:1]]
    assert np.array_equal(jf.lane_matrix(plan, edge, seqs).view(np.uint64), jc.oracle_matrix(plan, edge, seqs).view(np.uint64))


# ---- the Python layers over injected engines ----

class FakeDevice:
    """The device half of StringEditDistance.JoinIndex: records the calls, returns no hits."""
    made = []

    def __init__(self, codes, off, lens):
        self.codes, self.calls = codes, []
        FakeDevice.made.append(self)

    def _call(self, name, plan):
        self.calls.append((name, plan.K))
        return np.zeros(0, sedgpu.JOIN_HIT_DTYPE)

    def self_join(self, plan, max_dist, rows):
        return self._call("self_join", plan)

    def search(self, plan, packed, max_dist):
        return self._call("search", plan)

    def self_join_f64(self, plan, max_dist, rows):
        return self._call("self_join_f64", plan)

    def search_f64(self, plan, packed, max_dist):
        return self._call("search_f64", plan)

    def close(self):
        pass


def test_package_join_index_symbol_bounds(wfsearch):
    SED = wfsearch.SED
    iupac = ["".join(jf.IUPAC), "ACGU"]
    # the default and f64=False: the 8-symbol bound and its texts, as before
    for kw in ({}, {"f64": False}):
        with pytest.raises(sedgpu.SedError, match=r"the sequences have 15 symbols \(the join serves at most 8\)$"):
            SED.join_index(iupac, engine=FakeDevice, **kw)
        ix = SED.join_index(["ACGU", "ACGUN"], engine=FakeDevice, **kw)
        with pytest.raises(sedgpu.SedError, match=r"these rows have 9 symbols \(the join serves at most 8\)$"):
            ix.search(["RYSK"], 1.0)
        assert ix.self_join(1.0) == [] and ix.search(["AC"], 1.0) == []
        assert [c[0] for c in FakeDevice.made[-1].calls] == ["self_join", "search"]
    # f64=True lifts it to 16 and says so
    ix = SED.join_index(iupac, engine=FakeDevice, f64=True)
    assert ix.self_join_f64(1.5) == [] and ix.search_f64(["NNA"], 1.5) == [] and ix.self_join(1.5) == []
    assert FakeDevice.made[-1].calls == [("self_join_f64", 15), ("search_f64", 15), ("self_join", 15)]
    with pytest.raises(sedgpu.SedError, match=r"at most 16\)$"):
        SED.join_index(iupac, alphabet="abcdefghijklmnopq", engine=FakeDevice, f64=True)
    ix.close()


def test_package_join_route(wfsearch):
    SED = wfsearch.SED
    short = ["ACGU", "ACGUN", "", "GGGA"]
    assert SED.join_route(short, short, 2.0, True) == "int"     # user_costs: both serve it, the integer call is taken
    assert SED.join_route(short, short, 2.0, False) == "int"    # costs.json over ACGUN is dyadic
    assert SED.join_route(short + ["ACD"], short, 2.0) == "f64"  # a D at 0.66
    assert SED.join_route(["".join(jf.IUPAC)], short, 2.0) == "f64"  # 15 symbols
    assert SED.join_route(["ACGZ"], short, 2.0) == "int"        # the table does not resolve Z: the integer call raises
    assert SED.join_route(["A" * 33], short, 2.0) == "int"      # bad arguments stay the integer call's to report
    assert SED.join_route([], short, 2.0) == "int"


def test_wfsearch_routes_over_the_engine(wfsearch):
    made = []

    def index_fn(seqs, user_cost, **kw):
        made.append(jf.DefinitionEngineF64(seqs, user_cost, **kw))
        return made[-1]
    seqs = jc.mixed_set(5, "ACGUN", 30, pn=0.05)
    with_d = seqs[:29] + ["ACGUDACGU"]
    # the default route: the index is built and called exactly as before
    ix = wfsearch.JoinIndex(seqs, True, index_fn=index_fn)
    base = ix.neighbors(2)
    assert made[-1].kw == {} and made[-1].calls == ["self_join"] and ix.search("ACGU", 2) == ix.search("ACGU", 2, route="int")
    assert wfsearch.neighbors(seqs, 2, True, index_fn=index_fn) == base and made[-1].kw == {} and made[-1].closed
    # auto: the integer call on user_costs, fp64 under costs.json with a D in the collection
    ix = wfsearch.JoinIndex(seqs, True, index_fn=index_fn, route="auto")
    assert ix.neighbors(2) == base and made[-1].kw == {"f64": True} and made[-1].calls == ["self_join"]
    assert ix.search_many(["ACGU", ""], 2) and made[-1].calls == ["self_join", "search"]
    ix = wfsearch.JoinIndex(with_d, False, index_fn=index_fn, route="auto")
    want = [(i, j, 1 / (1 + d)) for i, j, d in jc.DefinitionEngine(with_d).self_join(2)]
    assert ix.neighbors(2) == want and made[-1].calls == ["self_join_f64"]
    assert ix.neighbors(2, rows=(0, 5)) == [h for h in want if h[0] < 5] and made[-1].calls[-1] == "self_join_f64"
    assert ix.search("ACGUD", 5) and made[-1].calls[-1] == "search_f64"
    assert ix.search("ACGU", 2, route="int") == ix.search("ACGU", 2) and made[-1].calls[-2:] == ["search", "search_f64"]
    # f64: always the new calls
    assert wfsearch.neighbors(seqs, 2, True, index_fn=index_fn, route="f64") == base
    assert made[-1].kw == {"f64": True} and made[-1].calls == ["self_join_f64"] and made[-1].closed
    with pytest.raises(ValueError, match="route must be one of"):
        wfsearch.JoinIndex(seqs, index_fn=index_fn, route="fp64")
    with pytest.raises(ValueError, match="route must be one of"):
        ix.neighbors(2, route="double")
    assert wfsearch.neighbors([], 2, index_fn=index_fn, route="auto") == []


def test_sedshard_routes():
    calls = []

    def join_fn(seqs, lo, hi, max_dist, user, **kw):
        calls.append(kw)
        return jc.DefinitionEngine(seqs, user).self_join(max_dist, (lo, hi))
    seqs = jc.mixed_set(72, "ACGUN", 9, pn=0.05)
    one = sedshard.neighbors(seqs, 12.0, True, join_fn=join_fn)
    jc.import_shim("StringEditDistance")
    for route, kw in (("int", {}), ("auto", {}), ("f64", {"f64": True})):
        got = sedshard.neighbors(seqs, 12.0, True, join_fn=join_fn, route=route)
        assert calls[-1] == kw and np.array_equal(got, one), route
    got = sedshard.neighbors(seqs + ["ACD"], 1.0, False, join_fn=join_fn, route="auto")
    assert calls[-1] == {"f64": True} and len(got) >= 0
    assert calls[0] == {}
    with pytest.raises(ValueError, match="route must be one of"):
        sedshard.neighbors(seqs, 1.0, route="x", join_fn=join_fn)


def test_binding_is_complete():
    names = {s[0] for s in sedgpu.SIGNATURES}
    assert {"sed_join_self_f64", "sed_join_search_f64", "sed_join_f64_plan", "sed_join_f64_keep", "sed_join_route"} <= names
    lib = sedgpu.load()
    for n in names:
        assert getattr(lib, n) is not None
    assert sedgpu.JOIN_KERNELS[3] == "f64" and sedgpu.JOIN_ROUTES == {0: "int", 1: "f64"}
