"""CPU: the device-free fit and join exports answer what tests/golden/plan_snapshot.json records (plan fields, rows,
lane records, params, route and `why` text, or the refusal's code), case by case.  The file was recorded by
tools/plan_snapshot.py before the planners' routes became a parameter; the arithmetic is the same, so the compare is
exact: doubles round-trip through JSON's repr."""
import pytest

import plan_snapshot_cases as cases
from conftest import load_golden


@pytest.fixture(scope="module")
def snaps():
    return cases.snapshot(), load_golden("plan_snapshot.json")


def test_the_case_list_is_the_recorded_one(snaps):
    got, want = snaps
    assert sorted(got) == sorted(want)


def test_every_export_answers_as_recorded(snaps):
    got, want = snaps
    differ = {name: [call for call in want[name] if got[name].get(call) != want[name][call]]
              for name in want if got.get(name) != want[name]}
    assert not differ, differ


def test_the_cases_reach_what_they_are_for(snaps):
    """The list's own coverage, read off the recorded answers: every export both serves and refuses, each route function
    has its three outcomes, and the three one_lane reasons and both join kernels occur."""
    want = snaps[1]
    calls = {}
    for entry in want.values():
        for call, r in (entry.items() if "ok" not in entry and "code" not in entry else [("join_f64_keep", entry)]):
            calls.setdefault(call, set()).add("ok" if "ok" in r else r["code"])
    every = set(cases.PAIR_CALLS) | set(cases.INDEX_CALLS) | set(cases.JOIN_CALLS) | {"fit_cutoff_scaled", "join_f64_keep"}
    assert set(calls) == every
    plans = every - {"fit_route", "fit_long_route", "join_route", "join_f64_keep"}
    assert all({"ok", -1, -4} <= calls[c] for c in plans), calls
    assert {"ok", -1} <= calls["join_f64_keep"]
    for route in ("fit_route", "fit_long_route", "join_route"):
        seen = {e[route]["ok"][0] for e in want.values() if route in e and "ok" in e[route]}
        assert seen == {"int", "f64", None}, (route, seen)
    one_lane = {e[c]["ok"]["one_lane"] for e in want.values() for c in ("fit_f64_plan", "fit_index_long_f64_plan")
                if c in e and "ok" in e[c]}
    assert one_lane == {0, 1, 2}
    assert {e["join_plan"]["ok"]["kernel"] for e in want.values() if "join_plan" in e and "ok" in e["join_plan"]} == {1, 2}
