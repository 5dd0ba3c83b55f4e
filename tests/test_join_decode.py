"""CPU: sed_join_decode, what every join call does with the records it downloads (sedgpu.join_decode): validate, convert,
order.  No kernel emits a record it refuses, so only this test reaches the refusals.  Both routes ("int": w0 = D on the
scale; "f64": (w0, w1) = the double's words) and both forms (k = 0: a join; k >= 1: the k nearest, under its rows'
bounds).  The call below is rows 10..13 of a 20-column index unless a case says otherwise."""
import math
import struct

import numpy as np
import pytest

import sedgpu

E_ARG, E_DEVICE = -1, -2
CUT_ALL = 65535  # SED_JOIN_CUT_ALL
ROWS, NCOLS = (10, 4), 20


def f64(row, col, dist):
    """An fp64 route's record: the double's low and high words."""
    lo, hi = struct.unpack("<II", struct.pack("<d", dist) if isinstance(dist, float) else struct.pack("<Q", dist))
    return (row, col, lo, hi)


def bits(records):
    return [struct.unpack("<Q", struct.pack("<d", float(d)))[0] for d in records["dist"]]


def decode(records, route="int", cap=None, rows=ROWS, ncols=NCOLS, self_join=False, **kw):
    cap = (CUT_ALL if route == "int" else math.inf) if cap is None else cap
    return sedgpu.join_decode(np.array(records, np.uint32).reshape(-1, 4), route, cap, rows, ncols, self_join, **kw)


def refused(records, **kw):
    with pytest.raises(sedgpu.SedError) as e:
        decode(records, **kw)
    return e.value.code, str(e.value)


def triples(hits):
    return [(int(h["row"]), int(h["col"]), float(h["dist"])) for h in hits]


@pytest.mark.parametrize("route", ["int", "f64"])
@pytest.mark.parametrize("k", [0, 1, 64])
def test_no_record_is_no_hit(route, k):
    bounds = ([5] * 4 if route == "int" else [5.0] * 4) if k else None
    assert len(decode([], route=route, k=k, bounds=bounds)) == 0
    assert len(decode([], route=route, rows=(0, 0), ncols=0, k=k)) == 0


def test_a_join_comes_back_sorted_by_row_and_column():
    rec = [(12, 3, 7, 0), (10, 19, 0, 0), (12, 0, 2, 0), (13, 13, 1, 0), (10, 2, 9, 0)]
    assert triples(decode(rec)) == [(10, 2, 9.0), (10, 19, 0.0), (12, 0, 2.0), (12, 3, 7.0), (13, 13, 1.0)]
    got = decode([f64(r, c, float(d)) for r, c, d, _ in rec], route="f64")
    assert triples(got) == [(10, 2, 9.0), (10, 19, 0.0), (12, 0, 2.0), (12, 3, 7.0), (13, 13, 1.0)]


@pytest.mark.parametrize("route", ["int", "f64"])
def test_the_k_nearest_come_back_by_distance_then_column_trimmed_to_k(route):
    """Row 10 has four candidates with a tie at distance 2 (columns 7 and 4), row 12 one, row 13 two."""
    rec = [(10, 7, 2), (12, 1, 5), (10, 9, 1), (13, 0, 3), (10, 4, 2), (10, 0, 6), (13, 2, 3)]
    as_route = (lambda r: [(a, b, d, 0) for a, b, d in r]) if route == "int" else (lambda r: [f64(a, b, float(d)) for a, b, d in r])
    bounds = [6, 0, 5, 3] if route == "int" else [6.0, 0.0, 5.0, 3.0]
    ordered = [(10, 9, 1.0), (10, 4, 2.0), (10, 7, 2.0), (10, 0, 6.0), (12, 1, 5.0), (13, 0, 3.0), (13, 2, 3.0)]
    want = {1: [ordered[0], ordered[4], ordered[5]], 2: ordered[:2] + ordered[4:], 64: ordered}  # (64: fewer than k present)
    for k in (1, 2, 64):
        assert triples(decode(as_route(rec), route=route, k=k, bounds=bounds)) == want[k], k


@pytest.mark.parametrize("scale_log2", [0, 8])
def test_integer_distances_are_exact(scale_log2):
    ds = [0, 1, 255, 256, 257, 32640, CUT_ALL]
    got = decode([(10, c, d, 0) for c, d in enumerate(ds)], scale_log2=scale_log2)
    assert [float(x) for x in got["dist"]] == [d / 2.0 ** scale_log2 for d in ds]   # (a power of two: exact)
    got = decode([(11, 5, CUT_ALL, 0)], scale_log2=scale_log2, k=1, bounds=[0, CUT_ALL, 0, 0])
    assert triples(got) == [(11, 5, CUT_ALL / 2.0 ** scale_log2)]


def test_fp64_distances_are_the_words_bit_for_bit():
    ds = [0.0, 5e-324, 2.2250738585072009e-308, 0.1 + 0.2, 1e308, math.inf]
    got = decode([f64(10, c, d) for c, d in enumerate(ds)], route="f64", cap=math.inf)
    assert bits(got) == [struct.unpack("<Q", struct.pack("<d", d))[0] for d in ds]
    got = decode([f64(13, c, d) for c, d in enumerate(ds)], route="f64", cap=math.inf, k=64, bounds=[0.0, 0.0, 0.0, math.inf])
    assert bits(got) == [struct.unpack("<Q", struct.pack("<d", d))[0] for d in ds]
    assert triples(decode([f64(10, 1, -0.0)], route="f64", cap=0.0)) == [(10, 1, 0.0)]  # (-0.0 >= 0: as before)


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("route", ["int", "f64"])
def test_a_record_outside_the_call_is_refused(route, k):
    mk = (lambda r, c: (r, c, 1, 0)) if route == "int" else (lambda r, c: f64(r, c, 1.0))
    kw = dict(route=route, k=k, bounds=([3] * 4 if route == "int" else [3.0] * 4) if k else None)
    good = [mk(10, 0), mk(13, 19)]
    assert len(decode(good, **kw)) == 2
    for bad in (mk(9, 0), mk(14, 0), mk(10, 20), mk(0xFFFFFFFF, 0), mk(10, 0xFFFFFFFF)):
        code, text = refused(good + [bad], **kw)
        assert code == E_DEVICE and "record 2" in text and "row %d, column %d" % (bad[0], bad[1]) in text, (bad, text)


@pytest.mark.parametrize("k", [0, 1])
def test_a_distance_above_the_cap_is_refused(k):
    kw = dict(k=k, bounds=[CUT_ALL] * 4 if k else None)
    assert len(decode([(10, 1, 40, 0)], cap=40, **kw)) == 1
    assert refused([(10, 1, 41, 0)], cap=40, **kw)[0] == E_DEVICE
    assert refused([(10, 1, 0x10000, 0)], cap=CUT_ALL, **kw)[0] == E_DEVICE
    kw = dict(route="f64", k=k, bounds=[math.inf] * 4 if k else None)
    t = 0.1 + 0.2
    assert len(decode([f64(10, 1, t)], cap=t, **kw)) == 1
    assert refused([f64(10, 1, np.nextafter(t, math.inf).item())], cap=t, **kw)[0] == E_DEVICE   # one ulp above max_dist
    assert refused([f64(10, 1, math.inf)], cap=1e308, **kw)[0] == E_DEVICE


def test_a_k_nearest_record_above_its_rows_bound_is_refused_within_the_cap():
    bounds = [7, 3, 0, 9]
    assert len(decode([(10, 1, 7, 0), (11, 1, 3, 0), (12, 1, 0, 0)], cap=40, k=1, bounds=bounds)) == 3
    assert refused([(10, 1, 7, 0), (11, 1, 4, 0)], cap=40, k=1, bounds=bounds)[0] == E_DEVICE   # row 11's bound is 3
    assert len(decode([(11, 1, 4, 0)], cap=40)) == 1                                              # (a join has no bounds)
    fb = [0.5, 0.25, 0.0, math.inf]
    assert len(decode([f64(11, 1, 0.25)], route="f64", cap=2.0, k=1, bounds=fb)) == 1
    assert refused([f64(11, 1, np.nextafter(0.25, 1.0).item())], route="f64", cap=2.0, k=1, bounds=fb)[0] == E_DEVICE
    assert refused([f64(13, 1, 2.5)], route="f64", cap=2.0, k=1, bounds=fb)[0] == E_DEVICE       # within the bound, above the cap


@pytest.mark.parametrize("k", [0, 3])
def test_nan_is_refused(k):
    kw = dict(route="f64", cap=math.inf, k=k, bounds=[math.inf] * 4 if k else None)
    for nan in (0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000):
        assert refused([f64(10, 1, 1.0), f64(10, 2, nan)], **kw)[0] == E_DEVICE


@pytest.mark.parametrize("route", ["int", "f64"])
def test_a_pair_reported_twice_is_refused(route):
    mk = (lambda r, c, d: (r, c, d, 0)) if route == "int" else (lambda r, c, d: f64(r, c, float(d)))
    adjacent = [mk(10, 1, 2), mk(11, 4, 1), mk(11, 4, 1), mk(12, 0, 0)]
    apart = [mk(11, 4, 1), mk(10, 1, 2), mk(12, 0, 0), mk(13, 5, 1), mk(11, 4, 1)]   # adjacent only after the sort
    for rec in (adjacent, apart):
        code, text = refused(rec, route=route)
        assert code == E_DEVICE and "row 11, column 4" in text, text
        bounds = [9] * 4 if route == "int" else [9.0] * 4
        code, text = refused(rec, route=route, k=2, bounds=bounds)
        assert code == E_DEVICE and "row 11 reports column 4 twice" in text, text
    # the k-nearest calls look for the pair among the hits the trim leaves, as they always did: with k = 1 the second
    # report of (11, 4) is trimmed away before the check
    assert triples(decode(adjacent, route=route, k=1, bounds=[9] * 4 if route == "int" else [9.0] * 4)) == \
        [(10, 1, 2.0), (11, 4, 1.0), (12, 0, 0.0)]


@pytest.mark.parametrize("route", ["int", "f64"])
def test_a_rows_own_column_is_refused_in_a_self_join_alone(route):
    mk = (lambda r, c: (r, c, 0, 0)) if route == "int" else (lambda r, c: f64(r, c, 0.0))
    bounds = [1] * 4 if route == "int" else [1.0] * 4
    rec = [mk(10, 11), mk(12, 12)]
    assert triples(decode(rec, route=route, k=1, bounds=bounds)) == [(10, 11, 0.0), (12, 12, 0.0)]
    assert triples(decode(rec, route=route)) == [(10, 11, 0.0), (12, 12, 0.0)]
    code, text = refused(rec, route=route, self_join=True, k=1, bounds=bounds)
    assert code == E_DEVICE and "row 12, column 12" in text


# ---- where the one list of checks is stricter than one of the two copies it replaces ----
@pytest.mark.parametrize("route", ["int", "f64"])
def test_stricter_a_join_refuses_a_rows_own_column_in_a_self_join(route):
    """The join's copy of the checks let (i, i) of a self join through; the k-nearest copy refused it.  No kernel emits it:
    both skip a row's own column."""
    rec = [(12, 12, 0, 0)] if route == "int" else [f64(12, 12, 0.0)]
    code, text = refused(rec, route=route, self_join=True)
    assert code == E_DEVICE and "row 12, column 12" in text


def test_stricter_a_join_refuses_a_negative_fp64_distance():
    """The join's copy compared an fp64 distance with max_dist alone; the k-nearest copy also refused dist < 0.  No kernel
    emits one: every cost is >= +0."""
    for d in (-5e-324, -1.0, -math.inf):
        assert refused([f64(10, 1, d)], route="f64", cap=math.inf)[0] == E_DEVICE
        assert refused([f64(10, 1, d)], route="f64", cap=math.inf, k=1, bounds=[math.inf] * 4)[0] == E_DEVICE


def test_bad_arguments():
    assert refused([(10, 1, 0, 0)], k=65, bounds=[1] * 4)[0] == E_ARG
    assert refused([(10, 1, 0, 0)], k=-1, bounds=[1] * 4)[0] == E_ARG
    assert refused([(10, 1, 0, 0)], k=1)[0] == E_ARG                    # a k-nearest call without its bounds
    assert refused([(10, 1, 0, 0)], scale_log2=9)[0] == E_ARG
    assert refused([(10, 1, 0, 0)], cap=math.nan)[0] == E_ARG
    assert refused([(10, 1, 0, 0)], rows=(-1, 4))[0] == E_ARG
