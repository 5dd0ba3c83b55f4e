"""CPU: the rows-per-lane rule of banded checkpoint batches (csrc/sed_plan.cpp: band_rows_rule; DESIGN.md 3.6c, "Rows per
lane") through sed_plan_routes.  The rule moves the automatic R of an integer batch from 16 to 8 or 4 by a modelled
forward cost, only where the batch runs the checkpoint route on the stripe kernel with band pruning and every wave pair
has at least 2048 rows; everything else plans as before (tests/test_plan_routes.py holds the recorded fills)."""
import functools

import numpy as np
import pytest

import band_cases as bc
import plan_route_cases as pc
import sedcost
import sedgpu
import synth

O = sedgpu
SCRIPT = sedgpu.SED_WANT_SCRIPT
PAIRS = 300
# what the fitted model picks for config-4-shaped fills (unrelated synthetic ACGU pairs under user_costs.json)
PICK = {4096: 8, 2048: 8}


@functools.lru_cache(maxsize=None)
def user_costs():
    return pc._costs(True, "ACGU")


def table_costs(name):
    p = sedcost.build_plan(bc.TABLES[name], ["ACGU"], ["ACGU"])
    return (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
            float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))


@functools.lru_cache(maxsize=None)
def synth_pairs(n, count=PAIRS):
    ids = np.arange(count, dtype=np.uint64)
    return list(synth.pair_codes(ids, n, 0)), list(synth.pair_codes(ids, n, 1))


def plan(A, B, options=None, flags=SCRIPT, costs=None):
    return sedgpu.plan_routes(costs or user_costs(), options or {}, sedgpu.PackedPairs(list(A), list(B)), flags)


@pytest.mark.parametrize("n", sorted(PICK))
def test_config4_shaped_fills_take_the_models_choice(n):
    r = plan(*synth_pairs(n))
    assert (r["mode"], r["traceback_mode"], r["rows_per_lane"]) == (1, 2, PICK[n])
    assert r["band_cells"] < r["cells"] and r["dot_keys"] == 1


@pytest.mark.parametrize("n", sorted(PICK))
def test_batches_off_the_banded_checkpoint_route_keep_r16(n):
    A, B = synth_pairs(n)
    for options in ({O.SED_OPT_BAND: 2}, {O.SED_PLAN_ENV_BAND: 0}, {O.SED_OPT_TB: 1}):
        assert plan(A, B, options)["rows_per_lane"] == 16, options
    r = plan(A, B, flags=0)
    assert (r["rows_per_lane"], r["traceback_mode"]) == (16, 0)


@pytest.mark.parametrize("n", sorted(PICK))
def test_a_forced_r_is_honoured(n):
    A, B = synth_pairs(n)
    for R in (4, 8, 16):
        r = plan(A, B, {O.SED_OPT_ROWS_PER_LANE: R})
        assert (r["rows_per_lane"], r["traceback_mode"]) == (R, 2)


@pytest.mark.parametrize("n", sorted(PICK))
def test_static_windows_still_take_the_rule(n):
    A, B = synth_pairs(n)
    auto = plan(A, B)
    for options in ({O.SED_PLAN_ENV_BAND: 3}, {O.SED_OPT_BAND: 3}):
        assert plan(A, B, options) == auto  # (the model and the reported cells are on the static windows)


def test_the_gate_is_two_full_r16_stripes_for_every_wave_pair():
    A, B = synth_pairs(2048)
    assert plan(A, B)["rows_per_lane"] == PICK[2048]
    short = synth.pair_codes([7], 2047, 0)[0]
    r = plan(A + [short], B + [B[0]])
    assert (r["rows_per_lane"], r["traceback_mode"]) == (16, 2)
    # a lane pair is no wave pair: the rule stays on
    r = plan(A + [A[0][:40]], B + [B[0][:20]])
    assert (r["rows_per_lane"], r["lane_pairs"], r["traceback_mode"]) == (PICK[2048], 1, 2)
    # ... unless the lane kernel is off, which makes it a short wave pair
    assert plan(A + [A[0][:40]], B + [B[0][:20]], {O.SED_OPT_LANE: 2})["rows_per_lane"] == 16
    # an empty pair is neither
    z = np.zeros(0, np.uint8)
    assert plan(A + [z], B + [z])["rows_per_lane"] == PICK[2048]


@pytest.mark.parametrize("n", sorted(PICK))
def test_band_cells_are_those_of_the_chosen_r(n):
    A, B = synth_pairs(n)
    r = plan(A, B)
    K, sub, _, ins, _, dele, _ = user_costs()
    want = sum(sedgpu.band_cells(sub.reshape(4, 4), ins, dele, a, b, r["rows_per_lane"]) for a, b in zip(A, B))
    assert r["band_cells"] == want
    assert want < sum(sedgpu.band_cells(sub.reshape(4, 4), ins, dele, a, b, 16) for a, b in zip(A, B))


def _mutated(A, rate, seed):
    rng = np.random.default_rng(seed)
    return [bc.mut(rng, a, rate) for a in A]


def test_a_wider_band_never_picks_a_smaller_r():
    """str2 = str1 with a growing share of positions redrawn: the diagonal bound, and with it every pair's window,
    grows with the share, and the choice must not shrink.  Identical and 10 % mutated pairs must not pick a larger R
    than unrelated ones."""
    A, B = synth_pairs(2048)
    picks = [plan(A, [a.copy() for a in A])["rows_per_lane"]]
    for rate in (0.02, 0.05, 0.1, 0.2, 0.4, 0.7, 1.0):
        r = plan(A, _mutated(A, rate, 2048))
        assert r["traceback_mode"] == 2
        picks.append(r["rows_per_lane"])
    unrelated = plan(A, B)["rows_per_lane"]
    print("identical, 2 .. 100 %% redrawn: R = %s; unrelated: R = %d" % (picks, unrelated))
    assert picks == sorted(picks), picks
    assert picks[0] <= unrelated and picks[3] <= unrelated  # identical, 10 %
    assert set(picks) <= {4, 8, 16}


def test_pairs_past_the_dot_key_bound_and_unfactorable_tables_plan_at_the_chosen_r():
    # two pairs with min(n, m) >= 4320 move the batch to distance keys (tests/test_dot_factor.py)
    A, B = synth_pairs(4096)
    long_a, long_b = synth.pair_codes([1, 2], 4350, 0), synth.pair_codes([1, 2], 4330, 1)
    r = plan(A + list(long_a), B + list(long_b))
    assert (r["traceback_mode"], r["dot_keys"]) == (2, 0) and r["rows_per_lane"] in (4, 8, 16)
    assert r["rows_per_lane"] == plan(A + list(long_a), B + list(long_b), {O.SED_OPT_DOT: 2})["rows_per_lane"]
    # a table sed_dot_factor refuses
    sub, ins, dele = bc.costs("unfactorable")
    assert sedgpu.dot_factor(sub, ins, dele, 2048, 0) is None
    A, B = synth_pairs(2048)
    Bm = _mutated(A, 0.1, 7)
    r = plan(A, Bm, costs=table_costs("unfactorable"))
    assert (r["mode"], r["traceback_mode"], r["dot_keys"]) == (1, 2, 0) and r["rows_per_lane"] in (4, 8, 16)
    assert r["band_cells"] == sum(sedgpu.band_cells(sub, ins, dele, a, b, r["rows_per_lane"]) for a, b in zip(A, Bm))
