"""CPU: join_long_plan, join_knn_plan (both index types), join_knn_f64_plan and join_f64_lower answer what
tests/golden/join_plan_snapshot.json records (plan fields, or the refusal's code and text), case by case.  The file was
recorded by tools/join_plan_snapshot.py from the commit before the five plan exports got one body; the arithmetic is
the same, so the compare is exact.  One record is that change's own: join_snapshot_cases.REORDERED."""
import pytest

import join_snapshot_cases as cases
from conftest import load_golden


@pytest.fixture(scope="module")
def snaps():
    return cases.snapshot(), load_golden("join_plan_snapshot.json")


def test_the_case_list_is_the_recorded_one(snaps):
    got, want = snaps
    assert sorted(got) == sorted(want)


def test_every_export_answers_as_recorded(snaps):
    got, want = snaps
    differ = {name: [call for call in want[name] if got[name].get(call) != want[name][call]]
              for name in want if got.get(name) != want[name]}
    assert not differ, differ


def test_the_reordered_refusal_names_k(snaps):
    """k out of range and a NULL out at once: k is refused first, by every k-nearest plan export."""
    r = snaps[1][cases.REORDERED]["sed_join_knn_plan"]
    assert r["code"] == -1 and r["text"].startswith("join: k = 0 neighbours")
    assert snaps[1]["raw/knn_plan_k1_null_out"]["sed_join_knn_plan"] == {"code": -1, "text": "bad join arguments"}


def test_the_cases_reach_what_they_are_for(snaps):
    """The list's own coverage, read off the recorded answers: every export both serves and refuses (an argument and a
    range refusal each, but for join_f64_lower, which has arguments alone), every k of K_EDGES is recorded on a call
    that is otherwise served, the long plans serve 128 symbols and refuse 129, and the short ones refuse 33."""
    want = snaps[1]
    seen = {}
    for entry in want.values():
        for call, r in entry.items():
            seen.setdefault(call, set()).add("ok" if "ok" in r else r["code"])
    assert set(seen) == set(cases.CALLS) | {"join_f64_lower", "sed_join_knn_plan"}
    assert all({"ok", -1, -4} <= seen[c] for c in cases.CALLS), seen
    assert {"ok", -1} <= seen["join_f64_lower"]
    for k in cases.K_EDGES:
        e = want["join/search_user_k%d" % k]
        for c in cases.CALLS[1:]:
            assert ("ok" in e[c]) == (1 <= k <= 64), (k, c)
            assert "ok" in e[c] or "k = %d" % k in e[c]["text"]
    for c, longest in (("join_long_plan", 128), ("join_knn_plan_long", 128), ("join_knn_plan", 32), ("join_knn_f64_plan", 32)):
        for n in (33, 127, 128, 129):
            assert ("ok" in want["join/long_rows_%d" % n][c]) == (n <= longest), (c, n)
    assert "lane_cells" in want["join/long_rows_128"]["join_knn_plan_long"]["ok"]
    assert "lane_cells" not in want["join/search_user"]["join_knn_plan"]["ok"]
