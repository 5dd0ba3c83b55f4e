"""GPU: bounded search (sed_batch_set_cutoff).  Under a cutoff T every pair is checked against the C
oracle: distance D <= T gives the same value and int flag as without a cutoff, D > T gives (inf, flag 0, len -1).  The
windowed distance-only stripe kernel (R = 4, 8, 16) is reached by batches of a few long pairs with the two-pairs-per-wave
packing, CHAIN and SPLIT off, and under default options by a batch that leaves the two-pairs-per-wave route for it; the
other routes (fp64, two pairs per wave, lane kernels, SPLIT) only compare.  tests/test_gpu_cut_envelope.py runs the same
contract over the tables, families and cutoffs of tests/cut_cases.py."""
import importlib
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
import oracle
import sedcost
import sedgpu
import synth

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
S = "ACGU"
INF = float("inf")
STRIPE = ((sedgpu.SED_OPT_CHAIN, 2), (sedgpu.SED_OPT_SPLIT, 2), (sedgpu.SED_OPT_PACK, 2))  # one wave per pair


def _oracle(plan, packed, want_len=False):
    d, i, ln, _, _ = oracle.batch(oracle.Costs.from_plan(plan), packed.codes_a, packed.off_a, packed.len_a,
                                  packed.codes_b, packed.off_b, packed.len_b, packed.npairs, nthreads=THREADS)
    return d, i.astype(bool), ln


def _contract(out, ref, T, want_len=False):
    """sed.h's result contract of sed_batch_set_cutoff for one run under cutoff T."""
    (d, ii, ln, _), (od, oi, ol) = out, ref
    within = od <= T
    assert np.array_equal(d[within], od[within]), np.flatnonzero(within & (d != od))[:10]
    assert np.array_equal(ii[within].astype(bool), oi[within])
    assert np.all(d[~within] == INF), np.flatnonzero(~within & (d != INF))[:10]
    assert not ii[~within].any() and np.all(ln[~within] == -1)
    if want_len:
        assert np.array_equal(ln[within], ol[within])
    else:
        assert np.all(ln == -1)
    return int(within.sum())


class _Batch:
    """A distance-only batch under the given options (put back on exit)."""

    def __init__(self, gpu, packed, opts=(), R=0, no_len=True):
        self.gpu, self.opts = gpu, tuple(opts) + ((sedgpu.SED_OPT_ROWS_PER_LANE, R),)
        self.packed, self.no_len = packed, no_len

    def __enter__(self):
        for k, v in self.opts:
            self.gpu.set_option(k, v)
        try:
            self.b = sedgpu.Batch(self.gpu, self.packed, False, no_len=self.no_len)
        except BaseException:
            self.__exit__()
            raise
        return self.b

    def __exit__(self, *exc):
        if getattr(self, "b", None) is not None:
            self.b.close()
        for k, _ in self.opts:
            self.gpu.set_option(k, 0)


def _windowed(gpu, table, A, B, R, cutoffs, want_pruned=True, lane_pairs=0):
    """Every cutoff on one resident batch of the windowed stripe route, each run against the oracle."""
    plan = sedcost.build_plan(table, [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    with _Batch(gpu, packed, STRIPE, R) as b:
        assert b.mode == "i32" and b.traceback_mode == 0 and b.rows_per_lane == R and b.split_tasks == 0
        assert b.lane_pairs == lane_pairs
        nominal = b.work()[0]
        cells = []
        for T in cutoffs:
            b.set_cutoff(T)
            assert b.chains == 0 and b.packed_pairs == 0
            b.run()
            hits = _contract(b.results(), ref, T)
            assert b.cutoff_hits() == hits
            assert b.work()[0] == nominal
            cells.append(b.band_cells)
            if want_pruned:
                assert b.band_cells < nominal, (T, b.band_cells, nominal)
    return ref, cells, nominal


@pytest.mark.parametrize("n, R", [(768, 4), (768, 8), (1536, 16)])
def test_stripe_and_chunk_geometry(gpu, tables, n, R):
    """10 % mutated copies: three stripes at (768, 4), two at (768, 8) and (1536, 16); the cutoffs sit on the exact
    "<=" edge of pair 3's distance."""
    a, b = synth.related_codes(np.arange(6), n)
    plan = sedcost.build_plan(tables[True], [S], [S])
    dstar = float(_oracle(plan, sedgpu.PackedPairs(list(a), list(b)))[0][3])
    (od, _, _), cells, nominal = _windowed(gpu, tables[True], list(a), list(b), R, [dstar - 1, dstar, dstar + 1])
    assert (od < dstar).any() and (od > dstar).any()  # the cutoffs split the batch
    assert cells[0] <= cells[1] <= cells[2] < nominal


@pytest.mark.parametrize("user", [True, False])
def test_path_next_to_the_window_edge(gpu, tables, user):
    """b = a without its first s symbols, s random ones appended (tests/test_gpu_band.py's construction); with the
    cutoff at that pair's distance the optimal path runs s columns off the diagonal, along the edge the cutoff sets."""
    t = tables[user]
    rng = np.random.default_rng(99 + user)
    n = 1536
    a = rng.integers(0, 4, size=n).astype(np.uint8)
    tail = rng.integers(0, 4, size=n).astype(np.uint8)
    sub = np.array([[0.0 if x == y else t["update"][x][y] for y in S] for x in S])
    step = t["insert"] + t["delete"]
    for s in range(n // 2, 0, -1):  # the largest s whose shift costs less than its own diagonal
        b = np.concatenate([a[s:], tail[:s]])
        if step * s < float(sub[a, b].sum()):
            break
    assert s > 64
    A = [a, a, a]
    B = [np.concatenate([a[s - ds:], tail[:s - ds]]) for ds in (0, 1, 7)]
    plan = sedcost.build_plan(t, [S], [S])
    od = _oracle(plan, sedgpu.PackedPairs(A, B))[0]
    assert od[0] <= step * s  # (the shifted path, or better)
    _windowed(gpu, t, A, B, 16, [float(od[0]), float(od.min()), float(od.max())])


def _unequal(rng):
    def mut(x):
        return np.where(rng.random(len(x)) < 0.1, rng.integers(0, 4, size=len(x)), x).astype(np.uint8)

    a = rng.integers(0, 4, size=1536).astype(np.uint8)
    A = [a, a, a, mut(a[:1100]), mut(a[436:]), rng.integers(0, 4, size=1100).astype(np.uint8)]
    B = [mut(a[:1100]), mut(a[436:]), rng.integers(0, 4, size=1100).astype(np.uint8), a, a, a]
    return a, mut, A, B


def test_unequal_lengths(gpu, tables):
    """(1536, 1100) and (1100, 1536) under insert 2, delete 3: the length difference alone costs 1308 / 872, so a
    cutoff of 800 runs no stripe at all (every pair inf), 1000 only the (1100, 1536) pairs, 1400 and 2000 all."""
    t = tables[True]
    assert t["insert"] * 436 == 872 and t["delete"] * 436 == 1308
    _, _, A, B = _unequal(np.random.default_rng(4096))
    (od, _, _), cells, nominal = _windowed(gpu, t, A, B, 16, [800, 1000, 1400, 2000])
    assert cells[0] == 0 and 0 < cells[1] < cells[2] <= cells[3]
    assert (od <= 1400).any() and (od > 1400).any() and (od <= 1000).any()


NLANE = 8  # lane pairs of the mixed batch (17 pairs in all: past the 16 below which short pairs stay on the wave kernels)


def _mixed(rng):
    """Pairs 0..5 unequal lengths, 6 and 7 identical, 8 independent random 1024 x 1024, 9.. lane pairs (40 x 28: 10 %
    mutated prefixes, the last one an identical 28 x 28)."""
    a, mut, A, B = _unequal(rng)
    r = synth.pair_codes([7], 1024, 0)[0], synth.pair_codes([7], 1024, 1)[0]
    A = A + [a, a[:1100], r[0]] + [a[40 * i:40 * i + 40] for i in range(NLANE - 1)] + [a[:28]]
    B = B + [a.copy(), a[:1100].copy(), r[1]] + [mut(a[40 * i:40 * i + 28]) for i in range(NLANE - 1)] + [a[:28].copy()]
    return A, B


def test_mixed_batch(gpu, tables):
    """The unequal pairs plus eight 40 x 28 pairs on a lane kernel in the same run, two identical pairs (D = 0, within
    T = 0, the narrowest window) and an independent random 1024 x 1024 pair (D = 797 under user_costs.json, 550 under costs.json).  The second cutoff
    is below the length difference's cost (872 / 1308, and 436 under costs.json's unit indels) and the random pair's
    distance, the third lets the first unequal pairs in."""
    A, B = _mixed(np.random.default_rng(4097))
    for user, R, cuts in ((True, 16, [0, 700, 1000, 1400]), (False, 8, [0, 400, 520, 600])):
        (od, _, _), cells, _ = _windowed(gpu, tables[user], A, B, R, cuts, lane_pairs=NLANE)
        assert od[6] == 0 and od[7] == 0 and od[8] > cuts[1] and (od[:6] > cuts[1]).all() and (od[:6] <= cuts[2]).any()
        assert od[-1] == 0 and (od[9:-1] > 0).all() and (od[9:] < cuts[1]).all()  # lane pairs on both sides of T = 0
        # (the identical pairs' bound stays 0 and the one-stripe pairs have nothing to skip, so the first two cutoffs
        # may run the same chunks; the unequal pairs join later)
        assert cells == sorted(cells) and cells[0] < cells[3]


def test_rerunning_a_resident_batch(gpu, tables):
    """Cutoffs T1, a larger T2, a smaller T3, then +inf on one batch: each run obeys its own cutoff, and the last equals
    a batch that never had one, as whole arrays."""
    A, B = _mixed(np.random.default_rng(4098))
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    with _Batch(gpu, packed, STRIPE, 16) as fresh:
        fresh.run()
        want = fresh.results()
        nominal = fresh.band_cells
        assert fresh.cutoff_hits() == packed.npairs
    with _Batch(gpu, packed, STRIPE, 16) as b:
        assert b.lane_pairs == NLANE
        for T in (1000, 1600, 300, INF):
            b.set_cutoff(T)
            b.run()
            out = b.results()
            assert b.cutoff_hits() == int(np.isfinite(out[0]).sum()) == _contract(out, ref, T)
            assert (b.band_cells < nominal) == (T != INF)
        for x, y in zip(out[:3], want[:3]):
            assert np.array_equal(x, y)
        assert b.cutoff_hits() == packed.npairs


def test_filter_only_fp64(gpu, tables):
    """64 pairs of 64 x 64 with 1 % N under costs.json: the fp64 kernels, compared on the fp64 value."""
    rng = np.random.default_rng(64)
    strs = [["".join(np.where(rng.random(64) < 0.01, "N", rng.choice(list(S), size=64))) for _ in range(64)]
            for _side in range(2)]
    assert any("N" in s for s in strs[0] + strs[1])
    plan = sedcost.build_plan(tables[False], strs[0], strs[1])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs([plan.encode(s) for s in strs[0]], [plan.encode(s) for s in strs[1]])
    ref = _oracle(plan, packed)
    T = float(np.median(ref[0]))
    with _Batch(gpu, packed) as b:
        assert b.mode != "i32"
        b.set_cutoff(T)
        b.run()
        hits = _contract(b.results(), ref, T, want_len=True)  # (the fp64 wave kernels report lengths regardless)
        assert 0 < hits < 64 and b.cutoff_hits() == hits and b.band_cells == b.work()[0]


def test_filter_only_two_pairs_per_wave(gpu, tables):
    """512 independent 300 x 300 pairs: a cutoff at the median distance keeps every cell inside the window, so the 2/3
    rule leaves the pairs on the two-pairs-per-wave kernel."""
    ids = np.arange(512)
    A, B = synth.pair_codes(ids, 300, 0), synth.pair_codes(ids, 300, 1)
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(list(A), list(B))
    ref = _oracle(plan, packed)
    T = float(np.median(ref[0]))
    with _Batch(gpu, packed) as b:
        b.set_cutoff(T)
        assert b.packed_pairs > 0 and b.band_cells == b.work()[0]
        b.run()
        hits = _contract(b.results(), ref, T)
        assert 0 < hits < 512 and b.cutoff_hits() == hits


def test_filter_only_lane_pairs(gpu, tables):
    """2000 pairs of ~28 nt on the lane kernels, with lengths (len -1 beyond the cutoff) and without."""
    ids = np.arange(2000)
    la, lb = synth.lengths(ids, 20, 36, 2), synth.lengths(ids, 20, 32, 3)
    A = [synth.pair_codes([i], int(n), 0)[0] for i, n in zip(ids, la)]
    B = [synth.pair_codes([i], int(m), 1)[0] for i, m in zip(ids, lb)]
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(A, B)
    ref = _oracle(plan, packed)
    T = float(np.median(ref[0]))
    for no_len in (True, False):
        with _Batch(gpu, packed, no_len=no_len) as b:
            assert b.lane_pairs == 2000
            b.set_cutoff(T)
            b.run()
            hits = _contract(b.results(), ref, T, want_len=not no_len)
            assert 0 < hits < 2000 and b.cutoff_hits() == hits


def test_nearest_and_search_within(tables):
    """wfsearch.nearest / search_within through the module: 64 documents of 300 nt, 8 of them copies of the query mutated
    at 2 - 20 %, the rest random; k = 5."""
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        wfsearch = importlib.import_module("wfsearch")
    finally:
        os.chdir(cwd)
    rng = np.random.default_rng(300)
    lut = np.array(list(S))
    q = rng.integers(0, 4, size=300)
    docs = []
    for i in range(64):
        if i % 8 == 3:
            rate = 0.02 + 0.18 * (i // 8) / 7
            docs.append(np.where(rng.random(300) < rate, rng.integers(0, 4, size=300), q))
        else:
            docs.append(rng.integers(0, 4, size=300))
    query, docs = "".join(lut[q]), ["".join(lut[d]) for d in docs]
    plan = sedcost.build_plan(tables[False], [query], docs)
    packed = sedgpu.PackedPairs([plan.encode(query)] * 64, [plan.encode(d) for d in docs])
    od = _oracle(plan, packed)[0]
    order = sorted(range(64), key=lambda i: (od[i], i))
    got = wfsearch.nearest(query, docs, 5)
    assert got == [(docs[i], 1 / (1 + int(od[i]))) for i in order[:5]]
    assert all(i % 8 == 3 for i in order[:5])
    T = float(od[order[5]])
    within = wfsearch.search_within(query, docs, T)
    assert within == [(docs[i], 1 / (1 + int(od[i]))) for i in range(64) if od[i] <= T] and len(within) >= 6
    assert wfsearch.search_within(query, docs, 0) == []
    assert len(wfsearch.nearest(query, docs, 100)) == 64


def test_error_paths(gpu, tables):
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    a, b = synth.related_codes(np.arange(2), 100)
    packed = sedgpu.PackedPairs(list(a), list(b))
    script = sedgpu.Batch(gpu, packed, True)
    try:
        with pytest.raises(sedgpu.SedError, match=r"\(-1\)"):  # SED_E_ARG
            script.set_cutoff(10)
    finally:
        script.close()
    with _Batch(gpu, packed) as d:
        for bad in (math.nan, -1.0, -INF):
            with pytest.raises(sedgpu.SedError, match=r"\(-1\)"):
                d.set_cutoff(bad)
        d.set_cutoff(0)  # valid: only identical pairs are within
        d.run()
        assert d.cutoff_hits() == 0 and np.all(d.results()[0] == INF)


def test_two_pairs_per_wave_batch_moves_to_the_window_and_back(gpu, tables):
    """Default options: 260 related pairs of 1536 x 1536 (two stripes at R = 16) run two per wave without a cutoff.  A
    cutoff at the median distance keeps ~0.6 of their cells (below the 2/3 share), so the wave pairs move to the windowed
    kernel; +inf moves them back and gives the results of a batch that never had a cutoff; then the cutoff again."""
    a, b = synth.related_codes(np.arange(260), 1536)
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(list(a), list(b))
    ref = _oracle(plan, packed)
    T = float(np.median(ref[0]))
    with _Batch(gpu, packed) as fresh:
        fresh.run()
        want = fresh.results()
    with _Batch(gpu, packed) as bt:
        nominal = bt.work()[0]
        assert bt.rows_per_lane == 16 and bt.packed_pairs == 260 and bt.split_tasks == 0 and bt.chains == 0
        for cut in (T, INF, T - 1):
            bt.set_cutoff(cut)
            if cut == INF:
                assert bt.packed_pairs == 260 and bt.band_cells == nominal
            else:
                assert bt.packed_pairs == 0 and bt.band_cells < 2 / 3 * nominal
            bt.run()
            out = bt.results()
            hits = _contract(out, ref, cut)
            assert bt.cutoff_hits() == hits and (cut == INF or 0 < hits < 260)
            if cut == INF:
                for x, y in zip(out[:3], want[:3]):
                    assert np.array_equal(x, y)


def test_costs_set_after_the_fill_do_not_reach_the_windows(gpu, tables):
    """The windows use the costs of the batch's fill, as its kernels do, whatever the context's table is by the first
    set_cutoff."""
    a, b = synth.related_codes(np.arange(6), 1536)
    plan = sedcost.build_plan(tables[True], [S], [S])
    gpu.set_costs(plan)
    packed = sedgpu.PackedPairs(list(a), list(b))
    ref = _oracle(plan, packed)
    T = float(np.sort(ref[0])[3])
    with _Batch(gpu, packed, STRIPE, 16) as bt:
        try:
            gpu.set_costs(sedcost.build_plan(tables[False], [S], [S]))  # insert = delete = 1: other windows, other keys
            bt.set_cutoff(T)
            bt.run()
            assert _contract(bt.results(), ref, T) == 4 and bt.band_cells < bt.work()[0]
        finally:
            gpu.set_costs(plan)
