#!/usr/bin/env python3
"""Record tests/golden/join_plan_snapshot.json: what the join's device-free exports answer over the cases of
tests/join_snapshot_cases.py (no device needed).  The library is sedgpu's: libsed.so beside it, or the one SED_LIBRARY
names, which is how the file is recorded from another build than the tree's.

    SED_LIBRARY=/path/to/parent/libsed.so python tools/join_plan_snapshot.py   # write the file, from the parent's build
    python tools/join_plan_snapshot.py --reordered                             # rewrite the one record that changed
    python tools/join_plan_snapshot.py --check                                 # compare, write nothing

--reordered replaces join_snapshot_cases.REORDERED alone, from the tree's library: the one input whose refusal text the
single plan body changed on purpose.  No other record is ever taken from the tree under test."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("rna-sequence-diff-patch_amd", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
OUT = os.path.join(REPO, "tests", "golden", "join_plan_snapshot.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the recorded file instead of writing it")
    ap.add_argument("--reordered", action="store_true", help="rewrite the one re-ordered record alone")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import join_snapshot_cases as cases
    import sedgpu
    from plan_snapshot import dumps
    snap = cases.snapshot()
    if args.check or args.reordered:
        with open(args.out) as f:
            want = json.load(f)
    if args.check:
        bad = sorted(k for k in set(snap) | set(want) if snap.get(k) != want.get(k))
        print("%s: %d cases, %d differ%s" % (sedgpu.LIB_PATH, len(snap), len(bad), ": " + ", ".join(bad[:10]) if bad else ""))
        return 1 if bad else 0
    if args.reordered:
        want[cases.REORDERED] = snap[cases.REORDERED]
        snap = want
    text = dumps(snap)
    with open(args.out, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes -> %s" % (sedgpu.LIB_PATH, len(snap), len(text), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
