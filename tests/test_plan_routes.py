"""CPU: the planner (csrc/sed_plan.cpp) through sed_plan_routes.  Every fill of plan_route_cases.py must give the route
numbers tests/golden/plan_routes.json holds, which were read from the getters of real batches (sed_batch_*) on an
MI355X before the planner was split from the runtime: the planner decides what that runtime decided, with no device."""
import itertools

import pytest

from conftest import load_golden
import plan_route_cases as pc
import sedgpu

GOLD = load_golden("plan_routes.json")
KNOB_KEYS = {"SED_TBPAR": sedgpu.SED_PLAN_ENV_TBPAR, "SED_BAND": sedgpu.SED_PLAN_ENV_BAND,
             "SED_ALT_DP": sedgpu.SED_PLAN_ENV_ALT_DP, "SED_CK_HALVES": sedgpu.SED_PLAN_ENV_CK_HALVES}


def plan(case):
    opts = dict(case.options)
    opts.update({KNOB_KEYS[k]: v for k, v in case.knobs.items()})
    return sedgpu.plan_routes(case.costs, opts, case.packed, case.flags)


def test_table_covers_the_golden_file():
    assert set(GOLD) == set(pc.NAMES) and tuple(pc.FIELDS) == sedgpu.PLAN_ROUTE_FIELDS


@pytest.mark.parametrize("name", pc.NAMES)
def test_routes_match_the_recorded_getters(name):
    want = GOLD[name]
    case = pc.Case(name)
    if "error" in want:
        with pytest.raises(sedgpu.SedError) as ex:
            plan(case)
        assert ex.value.code == want["error"]
    else:
        assert plan(case) == want  # (band_cells, cells and algo_bytes bit for bit: JSON round-trips doubles)


def test_the_table_reaches_every_route():
    """The recorded numbers themselves: each route the table is there for was taken on the GPU."""
    g = GOLD
    assert g["split_script_4096"]["split_tasks"] == 16 and g["split_script_4096"]["traceback_mode"] == 4
    assert g["split_dist_4096"]["split_tasks"] == 16 and g["split_dist_4096"]["traceback_mode"] == 0
    ck = g["ck_2048"]
    assert (ck["traceback_mode"], ck["dot_keys"], ck["dp_launches"]) == (2, 1, 2) and ck["band_cells"] < ck["cells"]
    assert g["ck_2048_band_off"]["band_cells"] == ck["cells"] and g["ck_2048_dot_off"]["dot_keys"] == 0
    assert g["ck_2048_codes"]["traceback_mode"] == 1 and g["ck_2048_codes"]["dp_launches"] == 1
    assert g["chain_dynamic"]["chains"] == 5120 and g["chain_dynamic"]["dot_keys"] & 2
    assert g["chain_dynamic_capped"]["chains"] == 300 and g["chain_static"]["chains"] == 134
    assert g["lane_bitpar"]["bitpar_pairs"] == 1000 and g["lane_x2"]["packed_pairs"] == 1000
    assert g["lane_scaled"]["scaled_pairs"] > 0 and g["lane_scaled"]["bitpar_pairs"] > 0
    assert g["wave_x2"]["packed_pairs"] == 300 and g["f64_segments"]["segment_pairs"] == 300
    assert g["f64_split"]["rows_per_lane"] == 2 and g["f64_split"]["split_tasks"] > 0
    assert g["i32_overflow"]["mode"] == 2 and g["i32_overflow_forced"]["error"] == -4
    assert g["wide_alphabet"]["error"] == -5 and g["negative_length"]["error"] == g["bad_code"]["error"] == -1
    assert g["no_pairs"]["cells"] == 0 and g["empty_sides"]["split_tasks"] == 10
    assert g["env_tbpar_on"]["traceback_mode"] == 3 and g["env_band_off"]["band_cells"] == ck["cells"]
    assert g["env_ck_one_part"]["dp_launches"] == 1 and g["env_ck_four_parts"]["dp_launches"] == 4


def test_environment_knobs_are_plain_options_of_a_plan():
    """The knobs the runtime reads from the environment once are fields of the planner's options: one process plans
    the same fill under each value (the recorded numbers needed a process per value)."""
    ck = pc.Case("ck_2048")
    assert plan(ck)["dp_launches"] == 2
    # 2048 wave pairs: at most 2 parts of 1024
    got = {v: sedgpu.plan_routes(ck.costs, {sedgpu.SED_PLAN_ENV_CK_HALVES: v}, ck.packed, ck.flags)["dp_launches"]
           for v in (0, 1, 2, 3, 4, 9)}
    assert got == {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 9: 2}
    assert sedgpu.plan_routes(ck.costs, {sedgpu.SED_PLAN_ENV_BAND: 0}, ck.packed, ck.flags) == GOLD["env_band_off"]
    assert sedgpu.plan_routes(ck.costs, {sedgpu.SED_PLAN_ENV_BAND: 1}, ck.packed, ck.flags) == GOLD["ck_2048"]
    sp = pc.Case("split_script_4096")
    for v in (0, 1):  # a SPLIT checkpoint batch reports mode 4 whichever walk follows
        assert sedgpu.plan_routes(sp.costs, {sedgpu.SED_PLAN_ENV_TBPAR: v}, sp.packed, sp.flags) == GOLD["env_tbpar_off"]
    tb = pc.Case("env_tbpar_on")
    modes = {v: sedgpu.plan_routes(tb.costs, {**tb.options, sedgpu.SED_PLAN_ENV_TBPAR: v}, tb.packed,
                                   tb.flags)["traceback_mode"] for v in (-1, 0, 1)}
    assert modes == {-1: 1, 0: 1, 1: 3}  # 100 pairs: past the automatic rule's 64
    lane = pc.Case("lane_pipelined")  # SED_ALT_DP moves launches between streams: no reported number changes
    for v in (0, 1):
        assert sedgpu.plan_routes(lane.costs, {sedgpu.SED_PLAN_ENV_ALT_DP: v}, lane.packed, lane.flags) == \
            GOLD["env_alt_dp_off"]


# every value sed_set_option takes per key (include/sed.h), and one it refuses
ACCEPTED = {
    sedgpu.SED_OPT_MODE: (0, 1, 2, 3), sedgpu.SED_OPT_SPLIT: (0, 1, 2), sedgpu.SED_OPT_LANE: (0, 1, 2),
    sedgpu.SED_OPT_TB: (0, 1, 2), sedgpu.SED_OPT_PACK: (0, 2), sedgpu.SED_OPT_BITPAR: (0, 2),
    sedgpu.SED_OPT_SEG: (0, 1, 2), sedgpu.SED_OPT_SPLITCK: (0, 2), sedgpu.SED_OPT_ZEROCOPY: (0, 2),
    sedgpu.SED_OPT_SCALED: (0, 2), sedgpu.SED_OPT_DOT: (0, 2, 3), sedgpu.SED_OPT_CHAIN_WAVES: (0, 1, 300, 2 ** 31 - 1),
    sedgpu.SED_OPT_CUT: (0, 1, 2), sedgpu.SED_OPT_BAND: (0, 2), sedgpu.SED_OPT_DEBUG_CORRUPT: (0, 1, 2 ** 31 - 1),
    sedgpu.SED_OPT_CHAIN: (0, 1, 2, 3, 1024), sedgpu.SED_OPT_ROWS_PER_LANE: (0, 1, 2, 4, 8, 16, 32),
}
REJECTED = {
    sedgpu.SED_OPT_MODE: 4, sedgpu.SED_OPT_SPLIT: 3, sedgpu.SED_OPT_LANE: 3, sedgpu.SED_OPT_TB: 3,
    sedgpu.SED_OPT_PACK: 1, sedgpu.SED_OPT_BITPAR: 1, sedgpu.SED_OPT_SEG: 3, sedgpu.SED_OPT_SPLITCK: 1,
    sedgpu.SED_OPT_ZEROCOPY: 1, sedgpu.SED_OPT_SCALED: 1, sedgpu.SED_OPT_DOT: 1, sedgpu.SED_OPT_CHAIN_WAVES: -1,
    sedgpu.SED_OPT_CUT: 3, sedgpu.SED_OPT_BAND: 1, sedgpu.SED_OPT_DEBUG_CORRUPT: -1, sedgpu.SED_OPT_CHAIN: 1025,
    sedgpu.SED_OPT_ROWS_PER_LANE: 3,
}


def _takes(key, value):
    """Whether the option table takes (key, value).  A refused option fails the plan with SED_E_ARG before anything
    else is looked at.  Under 40 symbols every plan with accepted options fails later and otherwise: forced integer
    mode with SED_E_RANGE, every other with SED_E_ALPHABET, both before the planner looks at the rows per lane (whose
    own check is SED_E_ARG again)."""
    case = _takes.case
    with pytest.raises(sedgpu.SedError) as ex:
        sedgpu.plan_routes(case.costs, {key: value}, case.packed, case.flags)
    assert ex.value.code in (-1, -4, -5)
    return ex.value.code != -1


def test_option_table_accepts_exactly_the_documented_values():
    _takes.case = pc.Case("wide_alphabet")
    assert set(ACCEPTED) == set(REJECTED) == set(range(1, 18))
    for key, values in ACCEPTED.items():
        for v in values:
            assert _takes(key, v), (key, v)
        assert not _takes(key, REJECTED[key]), (key, REJECTED[key])
        assert not _takes(key, -1), key
    # the irregular ones in full: every value 0..40 of the small sets
    for key in (sedgpu.SED_OPT_DOT, sedgpu.SED_OPT_ROWS_PER_LANE, sedgpu.SED_OPT_PACK):
        assert tuple(v for v in range(41) if _takes(key, v)) == ACCEPTED[key], key
    assert _takes(sedgpu.SED_OPT_ROWS_PER_LANE, 64) is False and _takes(sedgpu.SED_OPT_CHAIN, 1024)
    for key, v in itertools.product((0, 18, 100, 105), (0, 1)):
        assert not _takes(key, v), key  # unknown keys
