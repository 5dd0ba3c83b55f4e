"""CPU: the band-pruning bound (SED_OPT_BAND; sed_internal.h: sed_band_window, sed_band_chunks, through the
device-free entry points of libsed.so).  The checkpoint forward skips the cells outside a window of diagonals
derived from the cost of the plain diagonal path; the results stay exact as long as every cell of every
distance-optimal path lies inside the window.  Checked here on a few hundred small pairs against a forward plus
backward DP in numpy, with the chunk ranges' monotonicity, clipping and coverage, and the cell count of the
flagship shape (config 4's pairs: 0.531 of n*m); then on the tables and families of tests/band_cases.py at the sizes
the GPU tests run them."""
import numpy as np
import pytest

import band_cases
from conftest import load_golden
import sedgpu
import synth

S = "ACGU"


def _table(name):
    t = load_golden(name)
    sub = np.array([[0.0 if a == b else t["update"][a][b] for b in S] for a in S])
    return sub, float(t["insert"]), float(t["delete"])


def _diag_ub(sub, ins, dele, a, b):
    k = min(len(a), len(b))
    return float(sub[a[:k], b[:k]].sum()) + (ins * (len(b) - len(a)) if len(b) > len(a) else dele * (len(a) - len(b)))


def _dp(sub, ins, dele, a, b):
    """F[i, j] = the cost of the cheapest path (0, 0) -> (i, j)."""
    n, m = len(a), len(b)
    F = np.zeros((n + 1, m + 1))
    F[0, :] = ins * np.arange(m + 1)
    F[:, 0] = dele * np.arange(n + 1)
    for i in range(1, n + 1):
        up = np.minimum(F[i - 1, 1:] + dele, F[i - 1, :-1] + sub[a[i - 1], b])  # delete, update
        row = F[i]
        for j in range(1, m + 1):
            v = row[j - 1] + ins
            row[j] = v if v < up[j - 1] else up[j - 1]
    return F


def _optimal_cells(sub, ins, dele, a, b):
    """Boolean (n + 1) x (m + 1): the cells on at least one distance-optimal path."""
    F = _dp(sub, ins, dele, a, b)
    Bk = _dp(sub, ins, dele, a[::-1], b[::-1])[::-1, ::-1]  # the cheapest path (i, j) -> (n, m)
    return F + Bk == F[-1, -1]


@pytest.mark.parametrize("name", ["user_costs.json", "costs.json"] + list(band_cases.NEW_TABLES))
def test_every_optimal_path_lies_inside_the_window(name):
    sub, ins, dele = band_cases.costs(name)
    rng = np.random.default_rng(20260 + len(name))
    seen = set()
    for it in range(240):
        n, m = int(rng.integers(1, 49)), int(rng.integers(1, 49))
        if it % 3 == 0:
            m = n
        a = rng.integers(0, 4, size=n)
        if it % 2:  # related: a shifted, mutated copy (a drifting path); else independent
            s = int(rng.integers(0, 6))
            src = np.resize(np.roll(a, -s), m)
            b = np.where(rng.random(m) < 0.15, rng.integers(0, 4, size=m), src)
        else:
            b = rng.integers(0, 4, size=m)
        seen.add(int(np.sign(m - n)))
        elo, ehi = sedgpu.band_bounds(n, m, ins, dele, _diag_ub(sub, ins, dele, a, b))
        assert elo <= min(0, m - n) and ehi >= max(0, m - n)
        ii, jj = np.nonzero(_optimal_cells(sub, ins, dele, a, b))
        e = jj - ii
        assert e.min() >= elo and e.max() <= ehi, (n, m, elo, ehi, int(e.min()), int(e.max()))
    assert seen == {-1, 0, 1}


# (table, family, R): the batches tests/test_gpu_band_envelope.py runs (R only sets the families' stripe height here)
ENVELOPE = [(t, f, 4) for t in band_cases.TABLES for f in ("random", "low_complexity", "rearranged")]
ENVELOPE += [("user_costs.json", "edges", 4), ("tight", "edges", 4), ("user_costs.json", "edges", 8),
             ("user_costs.json", "drift", 4), ("gui_int", "drift", 4)]


@pytest.mark.parametrize("name, family, R", ENVELOPE)
def test_every_optimal_path_of_the_envelope_lies_inside_the_window(name, family, R):
    """The same over band_cases' tables and families (homopolymers and short periods: co-optimal paths out to the
    window's edges; block swaps and long indels: paths far off the diagonal), against the shared numpy DP."""
    _, ins, dele = band_cases.costs(name)
    for ref in band_cases.refs(name, family, R):
        elo, ehi = sedgpu.band_bounds(ref.n, ref.m, ins, dele, ref.ub)
        assert elo <= min(0, ref.m - ref.n) and ehi >= max(0, ref.m - ref.n)
        assert ref.emin >= elo and ref.emax <= ehi, (ref.n, ref.m, elo, ehi, ref.emin, ref.emax)


def test_case_tables_are_what_they_claim():
    """band_cases.TABLES: every one eligible for the integer kernel (1 <= mismatch <= insert + delete <= 255), the
    factorable ones accepted by sed_dot_factor at every min(n, m) the batches reach and the others refused, the classes
    the envelope names present, and every batch within the 16-bit distance field."""
    for name in band_cases.TABLES:
        sub, ins, dele = band_cases.costs(name)
        off = sub[~np.eye(4, dtype=bool)]
        assert ins >= 1 and dele >= 1 and ins + dele <= 255 and off.min() >= 1 and off.max() <= ins + dele
        assert np.all(sub == np.floor(sub)) and not np.diag(sub).any()
        for maxmin in (552, 768, 769, 1537, 2100, 2600):
            assert band_cases.factors(name, maxmin) == (name in band_cases.FACTORABLE), (name, maxmin)
    for name in ("sum", "gui_int", "tight", "heavy"):  # a mismatch that ties with delete + insert
        sub, ins, dele = band_cases.costs(name)
        assert (sub == ins + dele).any()
    assert band_cases.costs("sum")[0].max() == 3 and band_cases.costs("sum")[1:] == (1.0, 2.0)
    assert band_cases.costs("gui_int")[1:] == (3.0, 1.0) and band_cases.costs("tight")[1:] == (2.0, 5.0)
    assert band_cases.costs("heavy")[1:] == (20.0, 60.0)
    for name, family, R in ENVELOPE:
        A, B = band_cases.family_pairs(name, family, R)
        assert band_cases.i32_fits(name, A, B, R), (name, family, R)
    # `heavy` sits next to the limit: its widest pair is within 5 % of 65533, and m = n + 300 would pass it
    A, B = band_cases.family_pairs("heavy", "rearranged", 4)
    assert max(768 * 60 + (len(b) + 80) * 20 for b in B) > 0.95 * 65533
    assert not band_cases.i32_fits("heavy", [A[0]], [np.zeros(len(A[0]) + 300, np.uint8)], 4)


def test_bounds_formula():
    # config 4's bound: n = m, insert 2, delete 3, UB 3814 .. 3843 -> half-width 762 .. 768
    assert sedgpu.band_bounds(4096, 4096, 2, 3, 3814) == (-762, 762)
    assert sedgpu.band_bounds(4096, 4096, 2, 3, 3843) == (-768, 768)
    # identical strings: only the diagonal (and the corner's indels when the lengths differ)
    assert sedgpu.band_bounds(100, 100, 2, 3, 0) == (0, 0)
    assert sedgpu.band_bounds(100, 130, 2, 3, 60) == (0, 30)
    assert sedgpu.band_bounds(130, 100, 2, 3, 90) == (-30, 0)
    # never wider than the matrix
    assert sedgpu.band_bounds(10, 20, 1, 1, 10 ** 6) == (-10, 20)
    with pytest.raises(sedgpu.SedError):
        sedgpu.band_bounds(10, 20, 0, 0, 5)


@pytest.mark.parametrize("R", [4, 8, 16])
def test_chunk_ranges_are_monotone_clipped_and_cover_the_window(R):
    rng = np.random.default_rng(77 + R)
    rows = 64 * R
    for it in range(300):
        n, m = int(rng.integers(1, 5 * rows)), int(rng.integers(1, 5000))
        d = m - n
        elo = min(0, d) - int(rng.integers(0, 1500)) * int(it % 4 != 0)
        ehi = max(0, d) + int(rng.integers(0, 1500)) * int(it % 4 != 1)
        nstripes = (n + rows - 1) // rows
        prev = (0, 0)
        for k in range(nstripes):
            clo, chi, nchunks = sedgpu.band_chunk_range(n, m, R, elo, ehi, k)
            G = 64 // R
            assert nchunks == ((m + 63 + G - 1) // G * G + 63) // 64
            assert 0 <= clo <= chi <= nchunks - 1
            assert clo >= prev[0] and chi >= prev[1]  # monotone in the stripe
            prev = (clo, chi)
            r0, r1 = k * rows, min(n, (k + 1) * rows)
            i = np.arange(r0 + 1, r1 + 1)
            need_lo, need_hi = np.maximum(1, i + elo), np.minimum(m, i + ehi)
            t = (i - 1 - r0) // R  # the row's lane: it runs columns 64 clo + 1 .. 64 chi + 64 - t
            assert np.all(need_lo >= 64 * clo + 1) and np.all(need_hi <= 64 * chi + 64 - t), (n, m, elo, ehi, k)
            # whole chunks, no wider than needed: one chunk less on either side would cut the window
            assert 64 * (clo + 1) + 1 > need_lo.min()
            assert chi == nchunks - 1 or np.any(need_hi > 64 * (chi - 1) + 64 - t)
        if k == nstripes - 1:  # the sink's chunk runs
            cap_lane = ((n - 1) % rows) // R
            assert clo <= (m - 1 + cap_lane) // 64 <= chi
    # an open window: every chunk
    clo, chi, nchunks = sedgpu.band_chunk_range(3000, 4096, R, -(1 << 29), 1 << 29, 0)
    assert (clo, chi) == (0, nchunks - 1)
    with pytest.raises(sedgpu.SedError):
        sedgpu.band_chunk_range(3000, 4096, R, -5, 5, 99)


def test_band_cells_of_the_flagship_shape():
    """Config 4's pairs (synth.pair_codes, ids 0..2, 4096 x 4096, user_costs.json): half-width k = 762 .. 768, and the
    1024-row stripes keep (1792 + 2560 + 2560 + 1792) * 1024 cells, 0.531 of n * m."""
    sub, ins, dele = _table("user_costs.json")
    ids = np.arange(3)
    A, B = synth.pair_codes(ids, 4096, 0), synth.pair_codes(ids, 4096, 1)
    for a, b in zip(A, B):
        ub = _diag_ub(sub, ins, dele, a, b)
        elo, ehi = sedgpu.band_bounds(4096, 4096, ins, dele, ub)
        assert -elo == ehi and 762 <= ehi <= 768, (ub, elo, ehi)
        cells = sedgpu.band_cells(sub, ins, dele, a, b, 16)
        assert cells == (1792 + 2560 + 2560 + 1792) * 1024
        assert abs(cells / 4096 ** 2 - 0.531) < 5e-4
    # the 10 % mutated related pairs keep 0.297
    a, b = synth.related_codes([0], 4096)
    assert abs(sedgpu.band_cells(sub, ins, dele, a[0], b[0], 16) / 4096 ** 2 - 0.297) < 2e-3
    # identical strings: the narrowest window still holds the diagonal's chunks; a short pair is never cut
    a = synth.pair_codes([5], 2048, 0)[0]
    assert 0 < sedgpu.band_cells(sub, ins, dele, a, a, 16) <= 2 * 1024 * (1024 + 128)
    assert sedgpu.band_cells(sub, ins, dele, a[:40], a[:33], 4) == 40 * 33
