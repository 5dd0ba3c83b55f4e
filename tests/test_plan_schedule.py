"""CPU: what a run launches (csrc/sed_plan.cpp: sed_plan_run) through sed_plan_schedule.

(a) The expected sequences below were written by reading the launch code this schedule replaced (run_batch and
run_batch_parts of sed_runtime.cpp before the schedule existed), together with the routes tests/golden/plan_routes.json
records for each fill; none comes from calling the planner.  A row is (launcher, phase, stream, part, carries the start
event, carries the end event).

(b) The properties the old hand-kept launch counter could silently break hold for every fill and every cutoff state."""
import pytest

from conftest import load_golden
import plan_route_cases as pc
import schedule_cases as sc
import sedgpu
from test_plan_routes import KNOB_KEYS

GOLD = load_golden("plan_routes.json")
T, F = True, False
SCRIPT, PIPELINE = pc.SCRIPT, pc.PIPELINE


def schedule(case, cut_on=False, cut_win=False, flags=None, options=None):
    opts = dict(case.options)
    opts.update({KNOB_KEYS[k]: v for k, v in getattr(case, "knobs", {}).items()})
    opts.update(options or {})
    return sedgpu.plan_schedule(case.costs, opts, case.packed, case.flags if flags is None else flags, cut_on, cut_win)


def rows(s):
    return [tuple(st) for st in s]


def parts(n, lane=False):
    """A checkpoint batch in n parts: every part's forward, the lane kernel inside part 0's DP window (part 0's forward
    then drops its end event to it), every part's traceback, all on the parts' own streams."""
    fwd = [("i32", "dp", "part", i, T, not (lane and i == 0)) for i in range(n)]
    return fwd + [("lane", "dp", "part", 0, F, T)] * lane + [("tb_ck", "tb", "part", i, T, T) for i in range(n)]


# fill of plan_route_cases.py: (expected rows, need_ev, reuse_wait)
EXPECTED = {
    "ck_2048": (parts(2), F, None),
    "env_ck_one_part": ([("i32", "dp", "dp", 0, T, T), ("tb_ck", "tb", "tb", 0, T, T)], F, None),
    "env_ck_four_parts": (parts(GOLD["env_ck_four_parts"]["dp_launches"]), F, None),
    # one stream: the codes kernel closes the DP phase; one pair walks its stripes in parallel (SED_TBPAR unset)
    "split_script_4096": ([("i32", "dp", "dp", 0, T, F), ("codes", "dp", "dp", 0, F, T),
                              ("tb_stripes", "tb", "tb", 0, T, T)], F, None),
    "env_tbpar_off": ([("i32", "dp", "dp", 0, T, F), ("codes", "dp", "dp", 0, F, T),
                          ("tb_codes", "tb", "tb", 0, T, T)], F, None),
    "split_dist_4096": ([("i32", "dp", "dp", 0, T, T)], F, None),
    "chain_dynamic": ([("chain", "dp", "dp", 0, T, T), ("tb_codes", "tb", "tb", 0, T, T)], F, None),
    "lane_bitpar": ([("lane", "dp", "dp", 0, T, T)], F, None),
    "wave_x2": ([("x2", "dp", "dp", 0, T, T)], F, None),
    "f64_segments": ([("f64_seg", "dp", "dp", 0, T, T), ("tb_seg", "tb", "tb", 0, T, T)], F, None),
    "f64_split": ([("f64", "dp", "dp", 0, T, T), ("tb_stripes", "tb", "tb", 0, T, T)], F, None),
    # two result slots on two DP streams, ordered by stream: no events unless timed, no wait
    "lane_pipelined": ([("lane", "dp", "dp", 0, T, T)], F, None),
    # SED_ALT_DP=0: three slots on one stream, whose events every run records
    "env_alt_dp_off": ([("lane", "dp", "dp", 0, T, T)], T, None),
    "no_pairs": ([], F, None),
}
# the same fills pipelined: the traceback on its own stream, a slot's next user waiting for its traceback's end
EXPECTED_PIPELINED = {
    # (dynamic CHAIN script batches: odd runs' DP on the second DP stream)
    "chain_dynamic": [("chain", "dp", "dp", 0, T, T), ("tb_codes", "tb", "tb", 0, T, T)],
    # the codes kernel opens the traceback phase on the traceback stream
    "split_script_4096": [("i32", "dp", "dp", 0, T, T), ("codes", "tb", "tb", 0, T, F), ("tb_stripes", "tb", "tb", 0, F, T)],
    "env_tbpar_off": [("i32", "dp", "dp", 0, T, T), ("codes", "tb", "tb", 0, T, F), ("tb_codes", "tb", "tb", 0, F, T)],
    "f64_segments": [("f64_seg", "dp", "dp", 0, T, T), ("tb_seg", "tb", "tb", 0, T, T)],
    # a checkpoint batch takes SED_PIPELINE as a hint only: one buffer, its parts as without it
    "ck_2048": parts(2),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_recorded_fills_launch_what_the_runtime_launched(name):
    want, need_ev, reuse = EXPECTED[name]
    s = schedule(pc.Case(name))
    assert rows(s) == want
    assert (s.need_ev, s.reuse_wait) == (need_ev, reuse)
    assert s.parts == GOLD[name]["dp_launches"]


@pytest.mark.parametrize("name", sorted(EXPECTED_PIPELINED))
def test_pipelined_script_fills(name):
    case = pc.Case(name)
    s = schedule(case, flags=case.flags | PIPELINE)
    assert rows(s) == EXPECTED_PIPELINED[name]
    ck = name == "ck_2048"
    assert (s.need_ev, s.reuse_wait) == ((F, None) if ck else (T, "tb_end"))


def test_split_checkpoint_walk_follows_the_traceback_mode():
    """SPLIT with checkpoints reports traceback mode 4 whichever walk follows; SED_TBPAR picks it."""
    case = pc.Case("split_script_4096")
    assert GOLD["split_script_4096"]["traceback_mode"] == GOLD["env_tbpar_off"]["traceback_mode"] == 4
    walk = {v: rows(schedule(case, options={sedgpu.SED_PLAN_ENV_TBPAR: v}))[-1][0] for v in (-1, 0, 1)}
    assert walk == {-1: "tb_stripes", 0: "tb_codes", 1: "tb_stripes"}


def test_distance_batch_three_ways():
    """Wave pairs on the plain stripe kernel and lane pairs: without a cutoff, with the filter only, and with the wave
    pairs on the windowed kernel."""
    shape = sc.Shape("cut_windowed")
    r = sedgpu.plan_routes(shape.costs, shape.options, shape.packed, shape.flags)
    assert r["lane_pairs"] == 12 and r["packed_pairs"] == r["chains"] == r["split_tasks"] == 0 and r["mode"] == 1
    assert rows(schedule(shape)) == [("i32", "dp", "dp", 0, T, F), ("lane", "dp", "dp", 0, F, T)]
    assert rows(schedule(shape, True)) == [("i32", "dp", "dp", 0, T, F), ("lane", "dp", "dp", 0, F, F),
                                           ("filter", "dp", "dp", 0, F, T)]
    assert rows(schedule(shape, True, True)) == [("win", "dp", "dp", 0, T, F), ("lane", "dp", "dp", 0, F, F),
                                                 ("filter", "dp", "dp", 0, F, T)]
    # the two-pairs-per-wave fill: the windowed launch replaces the packed forward
    x2 = pc.Case("wave_x2")
    assert rows(schedule(x2, True)) == [("x2", "dp", "dp", 0, T, F), ("filter", "dp", "dp", 0, F, T)]
    assert rows(schedule(x2, True, True)) == [("win", "dp", "dp", 0, T, F), ("filter", "dp", "dp", 0, F, T)]
    # lane pairs only: nothing for the window to take, and SED_OPT_CUT = 2 never windows
    assert rows(schedule(sc.Shape("cut_filter"), True)) == [("lane", "dp", "dp", 0, T, F), ("filter", "dp", "dp", 0, F, T)]
    for bad in ((sc.Shape("cut_filter"), True, True, None), (shape, False, True, None),
                (shape, True, True, {sedgpu.SED_OPT_CUT: 2}), (pc.Case("ck_2048"), True, False, None)):
        with pytest.raises(sedgpu.SedError) as ex:
            schedule(bad[0], bad[1], bad[2], options=bad[3])
        assert ex.value.code == sedgpu.SED_E_ARG


def test_schedule_shapes_take_their_routes():
    """tests/schedule_cases.py: each small batch the GPU test runs plans the shape it is there for."""
    got = {n: rows(schedule(sc.Shape(n), sc.SHAPES[n][4] is not None, n == "cut_windowed")) for n in sc.NAMES}
    assert got["one_part_script"] == [("i32", "dp", "dp", 0, T, T), ("tb_ck", "tb", "tb", 0, T, T)]
    assert got["two_parts"] == parts(2, lane=True)
    assert got["split_ck"] == EXPECTED["split_script_4096"][0]
    assert got["pipelined_codes"] == [("i32", "dp", "dp", 0, T, T), ("tb_codes", "tb", "tb", 0, T, T)]
    assert schedule(sc.Shape("pipelined_codes")).reuse_wait == "tb_end"
    assert got["lane_only"] == [("lane", "dp", "dp", 0, T, T)]
    assert got["cut_filter"] == [("lane", "dp", "dp", 0, T, F), ("filter", "dp", "dp", 0, F, T)]
    assert got["cut_windowed"][0][0] == "win"
    # the whole waves' traceback before the segments', the end event on the last
    assert got["f64_segments"] == [("f64", "dp", "dp", 0, T, F), ("f64_seg", "dp", "dp", 0, F, T),
                                   ("tb_codes", "tb", "tb", 0, T, F), ("tb_seg", "tb", "tb", 0, F, T)]


def _fills():
    for name in pc.NAMES:
        if "error" not in GOLD[name]:
            yield name, pc.Case(name)
    for name in sc.NAMES:
        yield "shape_" + name, sc.Shape(name)


def _opts(case):
    return {**case.options, **{KNOB_KEYS[k]: v for k, v in getattr(case, "knobs", {}).items()}}


@pytest.mark.parametrize("pipeline", [0, PIPELINE])
def test_properties_of_every_schedule(pipeline):
    seen = set()
    for name, case in _fills():
        flags = case.flags | pipeline
        for cut_on, cut_win in ((F, F), (T, F), (T, T)):
            try:
                s = schedule(case, cut_on, cut_win, flags=flags)
            except sedgpu.SedError as ex:  # a cutoff state the batch cannot be in
                assert ex.code == sedgpu.SED_E_ARG and cut_on
                assert (flags & SCRIPT) or cut_win
                continue
            where = (name, pipeline, cut_on, cut_win)
            assert len(s) <= s.capacity, where
            # every non-empty (phase, part): one start carrier, its first step; one end carrier, its last step
            groups = {}
            for st in s:
                groups.setdefault((st.phase, st.part), []).append(st)
            for g in groups.values():
                assert [st.start for st in g] == [T] + [F] * (len(g) - 1), where
                assert [st.end for st in g] == [F] * (len(g) - 1) + [T], where
            # the DP phase comes first, and a distance batch has no traceback phase
            assert [st.phase for st in s] == sorted((st.phase for st in s), key=("dp", "tb").index), where
            assert (flags & SCRIPT) or all(st.phase == "dp" for st in s), where
            assert all(st.part < s.parts for st in s) and all((st.stream == "part") == (s.parts > 1) for st in s), where
            # no step for a count the plan reports as zero
            r = sedgpu.plan_routes(case.costs, _opts(case), case.packed, flags)
            kinds = {st.launcher for st in s}
            seen |= kinds
            assert ("lane" in kinds) == (r["lane_pairs"] > 0), where
            assert ("chain" in kinds) == (r["chains"] > 0 and not cut_win), where
            assert ("f64_seg" in kinds) == (r["segment_pairs"] > 0), where
            assert ("tb_seg" in kinds) == (r["segment_pairs"] > 0 and bool(flags & SCRIPT)), where
            assert ("x2" in kinds) <= (r["packed_pairs"] > 0 and not cut_win), where
            assert ("filter" in kinds) == cut_on and ("win" in kinds) == cut_win, where
            assert ("tb_ck" in kinds) == (r["traceback_mode"] == 2), where
            assert ("codes" in kinds) <= (r["traceback_mode"] == 4), where
            assert not ({"tb_codes", "tb_stripes"} & kinds) or r["traceback_mode"] in (1, 3, 4), where
            assert ("tb_stripes" in kinds) <= (r["traceback_mode"] in (3, 4)), where
            if case.packed.npairs == 0:
                assert not s, where
            if r["mode"] != 1:
                assert not ({"i32", "chain", "x2", "win", "codes", "tb_ck"} & kinds), where
            else:
                assert not ({"f64", "f64_seg", "tb_seg"} & kinds), where
    assert seen == set(sedgpu.STEP_LAUNCHERS)  # the fills reach every launcher
