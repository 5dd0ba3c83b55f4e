#!/usr/bin/env python3
"""Record tests/golden/plan_snapshot.json: what every device-free fit and join export answers over the cases of
tests/plan_snapshot_cases.py (no device needed).  The library is sedgpu's: libsed.so beside it, or the one SED_LIBRARY
names, which is how the file is recorded from another build than the tree's.

    SED_LIBRARY=/path/to/libsed.so python tools/plan_snapshot.py            # write the file
    python tools/plan_snapshot.py --check                                   # compare, write nothing

The file pins behaviour across a refactor: it is recorded before the change and the change must reproduce it, so it
is regenerated only by a change that means to alter what a planner answers."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("rna-sequence-diff-patch_amd", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
OUT = os.path.join(REPO, "tests", "golden", "plan_snapshot.json")


def dumps(snap):
    """One case per line, so that a changed answer is a one-line diff."""
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in snap.items()) + "\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the recorded file instead of writing it")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import plan_snapshot_cases
    import sedgpu
    snap = plan_snapshot_cases.snapshot()
    if args.check:
        with open(args.out) as f:
            want = json.load(f)
        bad = sorted(k for k in set(snap) | set(want) if snap.get(k) != want.get(k))
        print("%s: %d cases, %d differ%s" % (sedgpu.LIB_PATH, len(snap), len(bad), ": " + ", ".join(bad[:10]) if bad else ""))
        return 1 if bad else 0
    text = dumps(snap)
    with open(args.out, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes -> %s" % (sedgpu.LIB_PATH, len(snap), len(text), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
