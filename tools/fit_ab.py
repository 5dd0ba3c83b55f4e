"""Fit search (sed_fit_search): one 28-nt query against 8192 texts of 4096 nt under user_costs.json, with
the automatic chunk length against one lane per text (and any --chunk lengths), interleaved run by run; kernel time from
the engine's HIP events and the wall time of the whole blocking call (packing, upload, kernel, download).  Then the
distance-only lane kernel (sed_lane_i32_kernel, the same 3-VALU cell) on 262144 pairs of 28 x 28 as a per-cell yardstick.

    python tools/fit_ab.py [--texts 8192] [--length 4096] [--runs 7] [--chunk C ...] [--out profiles/fit/ab.jsonl]

One JSON line per variant; every variant must return the same hits."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import sedcost
    import sedgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=8192)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--pattern", type=int, default=28)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--chunk", type=int, action="append", default=[])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "user_costs.json")) as f:
        table = json.load(f)
    plan = sedcost.build_plan(table, ["ACGU"], ["ACGU"])
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    rng = np.random.default_rng(28)
    q = rng.integers(0, 4, size=a.pattern).astype(np.uint8)
    docs = rng.integers(0, 4, size=(a.texts, a.length)).astype(np.uint8)
    for d in range(0, a.texts, 100):  # 1 % of the texts hold a copy of the query with 10 % substitutions
        m = np.where(rng.random(a.pattern) < 0.1, rng.integers(0, 4, size=a.pattern), q)
        at = int(rng.integers(0, a.length - a.pattern + 1))
        docs[d, at:at + a.pattern] = m
    packed = sedgpu.PackedPairs.from_concat(np.tile(q, a.texts), np.full(a.texts, a.pattern, np.int32), docs.ravel(),
                                            np.full(a.texts, a.length, np.int32))
    ctx = sedgpu.Context(int(os.environ.get("SED_DEVICE", "0")))
    ctx.set_costs(plan)
    variants = [("auto", 0), ("one_lane_per_text", a.length + 1)] + [("chunk_%d" % c, c) for c in a.chunk]
    kernel = {name: [] for name, _ in variants}
    wall = {name: [] for name, _ in variants}
    first = None
    for run in range(a.runs + 1):  # (run 0 warms every variant up)
        for name, c in variants:
            ctx.set_option(sedgpu.SED_OPT_FIT_CHUNK, c)
            t0 = time.perf_counter()
            got = ctx.fit(packed)
            t1 = time.perf_counter()
            if first is None:
                first = [x.copy() for x in got]
            assert all(np.array_equal(x, y) for x, y in zip(got, first)), name
            if run:
                kernel[name].append(ctx.fit_last_ms())
                wall[name].append(1e3 * (t1 - t0))
    ctx.set_option(sedgpu.SED_OPT_FIT_CHUNK, 0)
    lines = []
    nominal = float(a.pattern) * a.length * a.texts
    for name, c in variants:
        fp = sedgpu.fit_plan(costs, {sedgpu.SED_OPT_FIT_CHUNK: c}, packed.len_a, packed.len_b)
        k = np.array(kernel[name])
        lines.append({"variant": name, "texts": a.texts, "length": a.length, "pattern": a.pattern, "W": fp["W"],
                      "chunk": fp["chunk"], "lanes": fp["lanes"], "cells_over_nominal": fp["cells"] / nominal,
                      "kernel_ms_median": round(float(np.median(k)), 4), "kernel_ms_min": round(float(k.min()), 4),
                      "kernel_ms_max": round(float(k.max()), 4),
                      "nominal_gcells_per_s": round(nominal / float(np.median(k)) / 1e6, 1),
                      "call_ms_median": round(float(np.median(wall[name])), 2),
                      "hits_within_6": int((first[0] <= 6).sum())})
    # the yardstick: the distance-only lane kernel, one pair per lane (no packing, no bit-parallel route)
    npairs = 262144
    A = rng.integers(0, 4, size=(npairs, 28)).astype(np.uint8)
    B = rng.integers(0, 4, size=(npairs, 28)).astype(np.uint8)
    ctx.set_option(sedgpu.SED_OPT_PACK, 2)
    ctx.set_option(sedgpu.SED_OPT_BITPAR, 2)
    b = sedgpu.Batch(ctx, sedgpu.PackedPairs.from_arrays(A, B), False, no_len=True)
    b.run()
    b.sync()
    b.reset_times()
    for _ in range(a.runs):
        b.run()
    ms = b.times()[0]
    lines.append({"variant": "lane_i32_distance_only_28x28", "pairs": npairs, "lane_pairs": b.lane_pairs,
                  "packed_pairs": b.packed_pairs, "kernel_ms_median": round(float(np.median(ms)), 4),
                  "kernel_ms_min": round(float(ms.min()), 4),
                  "nominal_gcells_per_s": round(b.work()[0] / float(np.median(ms)) / 1e6, 1)})
    b.close()
    ctx.close()
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    sys.exit(main())
