#!/usr/bin/env python3
"""What the planner decides for every bench.py workload, without a device: one JSON line per workload with the fields
of sedgpu.plan_routes for the fill bench.py makes (same pairs, costs and flags).  Two libraries plan alike when their
outputs are equal byte for byte:

    SED_LIBRARY=/path/to/other/libsed.so python3 tools/plan_workloads.py > a.jsonl
    python3 tools/plan_workloads.py > b.jsonl && cmp a.jsonl b.jsonl
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (puts the package on sys.path)
import sedcost  # noqa: E402
import sedgpu  # noqa: E402
import synth  # noqa: E402


def main():
    names = sys.argv[1:] or ["c4", "c3", "c2", "c5", "c5n", "iupac", "timing"]
    for w in names:
        P, n, m, costs_file, _ = bench.WORKLOADS[w]
        with open(os.path.join(REPO, "tests", "golden", costs_file)) as f:
            table = json.load(f)
        iupac = w in ("iupac", "timing")
        alpha = synth.IUPAC if iupac else (synth.ALPHABET + "N" if w == "c5n" else synth.ALPHABET)
        p = sedcost.build_plan(table, [alpha], [alpha])
        costs = (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
                 float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))
        A, B, qa, qb = bench.shard_inputs(w, P, n, m, 1, 0)
        packed = sedgpu.PackedPairs.from_arrays(A, B) if A is not None else sedgpu.PackedPairs(qa, qb)
        script = w not in ("c5", "c5n")
        flags = (sedgpu.SED_WANT_SCRIPT if script else sedgpu.SED_NO_LEN) | sedgpu.SED_PIPELINE
        print(json.dumps({"workload": w, **sedgpu.plan_routes(costs, {}, packed, flags)}), flush=True)


if __name__ == "__main__":
    main()
