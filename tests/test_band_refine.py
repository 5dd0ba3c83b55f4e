"""CPU: the per-stripe refinement of the band windows (sed_internal.h: sed_refine_cell, sed_refine_chunks, through
sed_band_refine_row of libsed.so).  Before stripe k the checkpoint forward scans the row the stripe above left behind:
a smaller upper bound from the diagonal cell, then every computed cell's slack under it, give the stripe's chunk
range.  The results stay exact as long as every cell of every distance-optimal path lies inside its stripe's range.
Checked against a forward plus backward DP in numpy, stripe after stripe as the kernel chains them (each stripe reads
only the columns the one above computed), with true row values and with off-path values inflated (the kernel's values
off the optimal paths are >= the true ones).  The envelope test repeats it over the cost tables and sequence families of
tests/band_cases.py, the inputs tests/test_gpu_band_envelope.py runs on the device."""
import functools

import numpy as np
import pytest

import band_cases
from band_cases import Ref
import sedgpu


def _mut(rng, x, rate=0.1):
    return np.where(rng.random(len(x)) < rate, rng.integers(0, 4, size=len(x)), x)


def _pairs(rng):
    """(a, b, R, kind): two and three stripes of 256 rows at R = 4, one 1100-symbol pair at R = 8."""
    out = []
    for n in (300, 600, 700):
        a = rng.integers(0, 4, size=n)
        out += [(a, rng.integers(0, 4, size=n), 4, "random"), (a, a.copy(), 4, "identical"), (a, _mut(rng, a), 4, "mutated")]
    for d in (1, 63, 64, 300):
        a = rng.integers(0, 4, size=600)
        tail = rng.integers(0, 4, size=d)
        out += [(a, np.concatenate([_mut(rng, a), tail]), 4, "n<m by %d" % d),       # 600 x (600 + d)
                (a, _mut(rng, a)[d:], 4, "n>m by %d" % d),                            # 600 x (600 - d)
                (a[:450], rng.integers(0, 4, size=450 - min(d, 300)), 4, "random n>m by %d" % d),
                (a[:300 + d // 2], np.concatenate([tail, _mut(rng, a[:300 + d // 2])]), 4, "shifted n<m by %d" % d)]
    a = rng.integers(0, 4, size=1100)
    out.append((a, _mut(rng, a), 8, "mutated 1100"))
    return out


@functools.lru_cache(maxsize=None)
def _pair_refs(name):
    """(Ref, R, kind) of _pairs under one table, for the true and the inflated walk."""
    sub, ins, dele = band_cases.costs(name)
    # (`heavy`, m = 900: the planner would not run the pair on 16-bit keys)
    return [(Ref(sub, ins, dele, a, b, R), R, kind) for a, b, R, kind in _pairs(np.random.default_rng(31 + len(name)))
            if band_cases.i32_fits(name, [a], [b], R)]


def _walk(ref, ins, dele, R, inflate_rng=None):
    """Chains the stripes' ranges as the forward does and checks each; returns the refined and the static ranges."""
    n, m, rows = ref.n, ref.m, 64 * R
    dist, diag, gap, ub = ref.dist, ref.diag, ref.gap, ref.ub
    k_ = min(n, m)
    elo, ehi = sedgpu.band_bounds(n, m, ins, dele, ub)
    nstripes = (n + rows - 1) // rows
    refined, static = [], []
    for k in range(nstripes):
        s_lo, s_hi, nchunks = sedgpu.band_chunk_range(n, m, R, elo, ehi, k)
        static.append((s_lo, s_hi))
        if k == 0:
            clo, chi = s_lo, s_hi
        else:
            r0 = k * rows
            row, opt0 = ref.rows[r0]
            row = row.copy()
            if inflate_rng is not None:
                row += np.where(opt0, 0, inflate_rng.integers(0, 51, size=m + 1))
            suf = float(diag[r0:].sum()) + gap if r0 <= k_ else None
            clo, chi, ub_new, any_ = sedgpu.band_refine_row(n, m, R, ins, dele, k, ub, suf, row.astype(np.int32),
                                                            refined[-1][0], refined[-1][1])
            assert any_
            assert dist <= ub_new <= ub
            ub = float(ub_new)
            assert clo >= refined[-1][0] and chi >= refined[-1][1]  # nondecreasing
            assert s_lo <= clo <= chi <= s_hi  # never wider than the static range
        refined.append((clo, chi))
        r1 = min(n, (k + 1) * rows)
        i = np.arange(k * rows + 1, r1 + 1)
        i = i[ref.has[i]]  # every optimal cell of the row lies between the row's extreme ones
        t = (i - k * rows - 1) // R  # the row's lane: it runs columns 64 clo + 1 .. 64 chi + 64 - t
        assert np.all(ref.jmin[i] >= 64 * clo + 1) and np.all(ref.jmax[i] <= 64 * chi + 64 - t), (n, m, R, k, clo, chi)
    return refined, static


@pytest.mark.parametrize("name", ["user_costs.json", "costs.json"] + list(band_cases.NEW_TABLES))
@pytest.mark.parametrize("inflated", [False, True])
def test_every_optimal_path_lies_inside_the_refined_ranges(name, inflated):
    sub, ins, dele = band_cases.costs(name)
    narrower = 0
    for ref, R, kind in _pair_refs(name):
        refined, static = _walk(ref, ins, dele, R, np.random.default_rng(7) if inflated else None)
        assert len(refined) >= 2, kind
        narrower += sum(r[1] - r[0] < s[1] - s[0] for r, s in zip(refined, static))
    assert narrower > 0  # the refinement does narrow some stripe


# (table, family, R): every table against the random, low-complexity and rearranged families at R = 4, the stripe and
# chunk borders, and the ten-stripe drift (R = 4 only)
ENVELOPE = [(t, f, 4) for t in band_cases.TABLES for f in ("random", "low_complexity", "rearranged")]
ENVELOPE += [("user_costs.json", "edges", 4), ("tight", "edges", 4), ("user_costs.json", "edges", 8),
             ("user_costs.json", "drift", 4), ("gui_int", "drift", 4)]
# (the model narrows some stripe below its static range in every one of these, with true and with inflated values, so
# narrower > 0 is asserted of all: none is left out)


@pytest.mark.parametrize("name, family, R", ENVELOPE)
@pytest.mark.parametrize("inflated", [False, True])
def test_every_optimal_path_of_the_envelope_lies_inside_the_refined_ranges(name, family, R, inflated):
    """test_every_optimal_path_lies_inside_the_refined_ranges over band_cases' tables and families: the inputs the GPU
    tests run (tests/test_gpu_band_envelope.py) keep the model's invariants."""
    sub, ins, dele = band_cases.costs(name)
    narrower = 0
    for ref in band_cases.refs(name, family, R):
        assert band_cases.i32_fits(name, [ref.a], [ref.b], R)
        refined, static = _walk(ref, ins, dele, R, np.random.default_rng(7) if inflated else None)
        assert len(refined) >= 2, (ref.n, ref.m)
        narrower += sum(r[1] - r[0] < s[1] - s[0] for r, s in zip(refined, static))
    print("%s / %s, R = %d: %d stripes narrower than their static range" % (name, family, R, narrower))
    assert narrower > 0


def test_refine_row_arguments():
    row = np.zeros(601, np.int32)
    with pytest.raises(sedgpu.SedError):
        sedgpu.band_refine_row(600, 600, 4, 2, 3, 0, 100, 100, row, 0, 1)  # stripe 0 is never refined
    with pytest.raises(sedgpu.SedError):
        sedgpu.band_refine_row(600, 600, 4, 2, 3, 3, 100, 100, row, 0, 1)  # no such stripe
    with pytest.raises(sedgpu.SedError):
        sedgpu.band_refine_row(600, 600, 4, 2, 3, 1, 100, 100, row, 2, 1)  # clo_prev > chi_prev
    # no surviving cell (every value above the bound): the static range of the bound, and the flag says so
    row[:] = 10 ** 6
    clo, chi, ub, any_ = sedgpu.band_refine_row(600, 600, 4, 2, 3, 1, 500, None, row, 0, 9)
    assert not any_ and ub == 500
    assert (clo, chi) == sedgpu.band_chunk_range(600, 600, 4, *sedgpu.band_bounds(600, 600, 2, 3, 500), 1)[:2]
