"""GPU: band pruning (SED_OPT_BAND) across its envelope: the cost tables and sequence families of
tests/band_cases.py.  Two shipped tables, both factorable, and uniform random sequences leave most of it unvisited: the
refinement's distance-key decode below a refined stripe, mismatches that tie with delete + insert on every cell,
distances next to the 16-bit limit, co-optimal paths that fan out to the window's edges (homopolymers, periods of 2, 4
and the chunk length), paths that jump by hundreds of columns inside one stripe, stripes of one row, m of 1 and of
64 c +- 1, and ten stripes whose window moves at every one.  A window one chunk too narrow faults nothing: it gives a
valid script that is not the reference's, which only a comparison on such inputs sees.

Every batch goes through test_gpu_band_refine's _check: SED_OPT_BAND 0, 3 and 2 give the same whole `ops` buffers,
distances, typing and lengths, every pair equals the C oracle op by op, the padding is zero, err == 0 on every pair and
the chunks run are refined <= static <= unpruned.  On top of that each batch proves its route: the integer kernel (an
ineligible table would otherwise quietly run fp64), checkpoints (traceback mode 2) at the R asked for, stored windows
under 0 and 3 and none under 2, and dot keys exactly where sed_dot_factor accepts the table.  Every comparison is for
bit equality; tests/test_band_bound.py and tests/test_band_refine.py check the same inputs against the window model."""
import numpy as np
import pytest

import band_cases
import sedgpu
from test_gpu_band_refine import _check

pytestmark = pytest.mark.gpu
TABLES = list(band_cases.TABLES)


def _lane(a, b):  # (sed_internal.h: SED_LANE_MAXN, SED_LANE_MAXM; the lane-per-pair kernel's pairs)
    return len(a) <= 512 and len(b) <= 32


def _envelope(gpu, name, A, B, R, times=1, dot=0, label=""):
    maxmin = max(min(len(a), len(b)) for a, b in zip(A, B) if not _lane(a, b))
    want_dot = dot != 2 and band_cases.factors(name, maxmin)

    def route(b, band):
        assert b.mode == "i32", (name, b.mode)
        assert b.traceback_mode == 2 and b.rows_per_lane == R
        assert b.dot_keys == want_dot, (name, maxmin)
        assert (b.band_chunks_run() is None) == (band == 2)

    print("%s / %s, %s keys, %d pairs, " % (name, label, "dot" if want_dot else "distance", len(A)), end="")
    return _check(gpu, band_cases.TABLES[name], A, B, R, times, dot, route)


@pytest.mark.parametrize("name", TABLES)
def test_tables_by_families_r4(gpu, name):
    """Every table against the random, the low-complexity and the rearranged family: three stripes of 256 rows, the
    second and third refined (n = 600, 619, 700; `heavy` with m - n within +-150, which keeps its distances under
    65533)."""
    for family in ("random", "low_complexity", "rearranged"):
        A, B = band_cases.family_pairs(name, family, 4)
        _envelope(gpu, name, A, B, 4, label=family)


@pytest.mark.parametrize("name", band_cases.FACTORABLE)
def test_both_key_formats(gpu, name):
    """The factorable tables again with SED_OPT_DOT = 2: the same three families as one batch on distance keys (the
    non-dot ck_key_dist decode through three stripes) must give the dot-key run's buffers, and the oracle's."""
    A, B = [], []
    for family in ("random", "low_complexity", "rearranged"):
        a, b = band_cases.family_pairs(name, family, 4)
        A, B = A + a, B + b
    (d, ii, ln, ops), chunks, chunks3 = _envelope(gpu, name, A, B, 4, label="three families")
    (d2, ii2, ln2, ops2), chunks_2, chunks3_2 = _envelope(gpu, name, A, B, 4, dot=2, label="three families")
    assert np.array_equal(ops, ops2), np.flatnonzero(ops != ops2)[:10]
    assert np.array_equal(d, d2) and np.array_equal(ln, ln2) and np.array_equal(ii, ii2)
    assert chunks == chunks_2 and chunks3 == chunks3_2  # the windows come from distances: the same in either format


@pytest.mark.parametrize("name, R", [("user_costs.json", 4), ("tight", 4), ("user_costs.json", 8)])
def test_stripe_and_chunk_borders(gpu, name, R):
    """band_cases.edges: last stripes of one row and of ROWS rows, m = 1, 63, 64, 65, 64 c and 64 c + 1 under three
    stripes, and m = 5 n."""
    A, B = band_cases.family_pairs(name, "edges", R)
    assert {len(a) for a in A} == {128 * R + 1, 192 * R, 192 * R + 1} and 5 * (128 * R + 1) in {len(b) for b in B}
    _envelope(gpu, name, A, B, R, label="edges")


@pytest.mark.parametrize("name", ["user_costs.json", "gui_int"])
def test_ten_stripes_of_drift(gpu, name):
    """band_cases.drift at R = 4: eleven stripes, the path 40 columns further left, right or alternating at each, three
    runs of one batch (run k + 1 meets the words run k left in the in-place bottom-row buffer)."""
    A, B = band_cases.family_pairs(name, "drift", 4)
    assert len(A[0]) == 2600 and {len(b) for b in B} >= {2200, 3000}
    _envelope(gpu, name, A, B, 4, times=3, label="drift")


def test_low_complexity_and_rearranged_r16(gpu):
    """R = 16 once: three stripes of 1024 rows (n = 2100) under user_costs.json."""
    for family in ("low_complexity", "rearranged"):
        A, B = band_cases.family_pairs("user_costs.json", family, 16, n=2100)
        _envelope(gpu, "user_costs.json", A, B, 16, label=family)


@pytest.mark.parametrize("name", TABLES)
def test_related_pairs_are_pruned(gpu, name):
    """Non-vacuity: the identical and the mutated pair of the random family, alone as one batch, run fewer chunks than
    unpruned under every table.  The host's restatement of the static window (sedgpu.band_cells) says so before the GPU
    does.  (Independent random pairs are not asserted: under `sum`, where a mismatch costs what delete + insert do, the
    diagonal's bound is loose and nothing of them is pruned.)"""
    A, B = band_cases.family_pairs(name, "random", 4)
    A, B = [A[p] for p in band_cases.RANDOM_RELATED], [B[p] for p in band_cases.RANDOM_RELATED]
    sub, ins, dele = band_cases.costs(name)
    for a, b in zip(A, B):
        assert sedgpu.band_cells(sub, ins, dele, a, b, 4) < len(a) * len(b)
    _, chunks, chunks3 = _envelope(gpu, name, A, B, 4, label="identical and mutated")
    assert chunks[0] < chunks[1] and chunks3[0] < chunks3[1]
