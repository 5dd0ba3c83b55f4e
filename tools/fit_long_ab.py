"""Long fit search (sed_fit_index_search_long): one query of P = 76, 256 and 1024 against 8192 texts of
4096 nt under user_costs.json.  After one warm-up of every variant the variants run interleaved, --runs times each, on
one otherwise idle GPU; kernel times are the engine's HIP events.

  per P: the automatic chunk against forced chunks either side of it (half, double, one chunk per text);
  P = 32 through the long kernel at R = 2 against sed_fit_index_kernel on the same lanes (the same forced chunk);
  the 16-thread C oracle on a sample of the texts, as the CPU baseline.

Cell updates are counted with the skew and the warm-up columns: a wave of R rows a lane updates 64 R cells in each of
its steps.  The expectation is stated before the run: the short kernel's measured 9.3e12 cell updates/s scaled by
3 R / (3 R + HANDOVER) instructions a step, HANDOVER = the step's instructions beside its 3 R cell instructions.

    python tools/fit_long_ab.py [--texts 8192] [--length 4096] [--runs 7] [--out profiles/fit_long]

Writes ab.json and README.md into --out; every chunking of a P must return the same hits, which the oracle's sample
must equal."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHORT_RATE = 9.3e12  # sed_fit_kernel's measured cell updates/s
HANDOVER = 24        # instructions a step beside the cells': two DPP moves, inj, the report, the rebase test, the loop


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "spread_pct": round(100 * float(x.max() - x.min()) / float(np.median(x)), 2)}


def counted_cells(sedgpu, costs, opts, P, lens, R):
    """64 R cells in every step of every wave: nsteps + 63 steps, rounded up to a text word's four."""
    lanes, _ = sedgpu.fit_index_long_lanes(costs, opts, [P], lens)
    ns = lanes["nsteps"]
    steps = (ns > 0) * ((ns + 63 + 3) // 4 * 4)
    return float(64 * R * steps.sum()), int(len(ns))


def main():
    import numpy as np
    import oracle
    import sedcost
    import sedgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=8192)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_long"))
    a = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "user_costs.json")) as f:
        table = json.load(f)
    plan = sedcost.build_plan(table, ["ACGU"], ["ACGU"])
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    rng = np.random.default_rng(76)
    docs = rng.integers(0, 4, size=(a.texts, a.length)).astype(np.uint8)
    lens = [a.length] * a.texts
    ctx = sedgpu.context()
    ctx.set_costs(plan)
    ix = sedgpu.FitIndex.from_texts(ctx, list(docs))
    CH, RW = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS
    res = {"texts": a.texts, "length": a.length, "runs": a.runs, "device": _device_name(), "patterns": {}}

    def run(call, q, chunk, rows=0):
        ctx.set_option(CH, chunk)
        ctx.set_option(RW, rows)
        out = call(q)
        ctx.set_option(CH, 0)
        ctx.set_option(RW, 0)
        return out

    for P in (76, 256, 1024):
        pat = rng.integers(0, 4, size=P).astype(np.uint8)
        for d in range(0, a.texts, 100):  # 1 % of the texts hold a copy with 10 % substitutions
            m = np.where(rng.random(P) < 0.1, rng.integers(0, 4, size=P), pat).astype(np.uint8)
            at = int(rng.integers(0, a.length - P + 1))
            docs[d, at:at + P] = m
        ix.close()
        ix = sedgpu.FitIndex.from_texts(ctx, list(docs))
        q = sedgpu.PackedPairs([pat], [np.zeros(0, np.uint8)])
        auto = sedgpu.fit_index_long_plan(costs, {}, [P], lens)
        R = int(auto["rows"][0])
        ac = auto["chunk"] or a.length + 1
        chunks = {"auto": 0, "half": max(ac // 2 // 4 * 4, 4), "double": min(2 * ac, a.length + 1), "one_per_text": a.length + 1}
        times = {k: [] for k in chunks}
        want = None
        for it in range(a.runs + 1):  # (run 0 warms every variant up)
            for k, c in chunks.items():
                got = run(ix.search_long, q, c)
                want = want or [x.copy() for x in got]
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), (P, k)
                if it:
                    times[k].append(ix.last_ms())
        ns = min(a.sample, a.texts)
        pk = sedgpu.PackedPairs([pat] * ns, list(docs[:ns]))
        t0 = time.perf_counter()
        od, os_, oe = oracle.fit(oracle.Costs.from_plan(plan), pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b,
                                 ns, 16)
        cpu_s = time.perf_counter() - t0
        assert np.array_equal(od, want[0][0, :ns]) and np.array_equal(os_, want[1][0, :ns]) and np.array_equal(oe, want[2][0, :ns])
        entry = {"rows": R, "W": auto["W"], "auto_chunk": auto["chunk"], "expected_counted_cells_per_s":
                 SHORT_RATE * 3 * R / (3 * R + HANDOVER), "variants": {},
                 "oracle_16_threads": {"texts": ns, "seconds": round(cpu_s, 4), "nominal_cells_per_s": P * a.length * ns / cpu_s}}
        for k, c in chunks.items():
            cells, waves = counted_cells(sedgpu, costs, {CH: c}, P, lens, R)
            st = stats(times[k])
            st.update({"chunk": c, "waves": waves, "counted_cells": cells,
                       "counted_cells_per_s": cells / (st["median"] * 1e-3),
                       "nominal_cells_per_s": P * a.length * a.texts / (st["median"] * 1e-3)})
            entry["variants"][k] = st
        res["patterns"][str(P)] = entry
        print(json.dumps({str(P): entry}), flush=True)

    # the price of the wave layout: P = 32 at R = 2 against the short index kernel on the same lanes
    pat = rng.integers(0, 4, size=32).astype(np.uint8)
    q = sedgpu.PackedPairs([pat], [np.zeros(0, np.uint8)])
    chunk = sedgpu.fit_index_long_plan(costs, {}, [32], lens)["chunk"] or a.length + 1
    tl, ts = [], []
    for it in range(a.runs + 1):
        gl = run(ix.search_long, q, chunk, 2)
        ml = ix.last_ms()
        gs = run(ix.search, q, chunk)
        ms = ix.last_ms()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(gl, gs))
        if it:
            tl.append(ml)
            ts.append(ms)
    res["p32"] = {"chunk": chunk, "long_r2_ms": stats(tl), "short_index_ms": stats(ts),
                  "ratio": round(stats(tl)["median"] / stats(ts)["median"], 3)}
    ix.close()
    print(json.dumps({"p32": res["p32"]}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))


def _device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        return "unknown"


def readme(r):
    out = ["# Long fit search: measurements (DESIGN.md 3.6h)", "",
           "Written by `tools/fit_long_ab.py`; the raw numbers are in `ab.json`.", "",
           "Workload: one query of P symbols against %d texts of %d nt, `user_costs.json`; device %s; %d runs of every"
           " variant after one warm-up, variants interleaved run by run, one process, nothing else on the GPU.  Kernel ms"
           " are HIP events around the launches.  Counted cells = 64 R cells for every step of every wave (skew and warm-up"
           " columns included); nominal cells = P x text symbols." % (r["texts"], r["length"], r["device"], r["runs"]), "",
           "Expectation, stated before the run: %.1e cell updates/s (the short kernel, measured) x 3 R / (3 R + %d)"
           " instructions a step." % (SHORT_RATE, HANDOVER), "",
           "| P | R | chunk | waves | median ms | min | max | spread | counted cells/s | expected | nominal cells/s |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for P, e in r["patterns"].items():
        for k, v in e["variants"].items():
            out.append("| %s | %d | %s (%d) | %d | %s | %s | %s | %s %% | %.3g | %.3g | %.3g |"
                       % (P, e["rows"], k, v["chunk"], v["waves"], v["median"], v["min"], v["max"], v["spread_pct"],
                          v["counted_cells_per_s"], e["expected_counted_cells_per_s"], v["nominal_cells_per_s"]))
    out += ["", "| P | 16-thread C oracle, nominal cells/s (sample of texts) | GPU automatic chunk, nominal cells/s |", "|---|---|---|"]
    for P, e in r["patterns"].items():
        out.append("| %s | %.3g (%d texts, %s s) | %.3g |" % (P, e["oracle_16_threads"]["nominal_cells_per_s"],
                                                               e["oracle_16_threads"]["texts"], e["oracle_16_threads"]["seconds"],
                                                               e["variants"]["auto"]["nominal_cells_per_s"]))
    p = r["p32"]
    out += ["", "The price of the wave layout: P = 32, chunk %d, the long kernel at R = 2: %s ms (spread %s %%);"
            " `sed_fit_index_kernel` on the same lanes: %s ms (spread %s %%); ratio %s."
            % (p["chunk"], p["long_r2_ms"]["median"], p["long_r2_ms"]["spread_pct"], p["short_index_ms"]["median"],
               p["short_index_ms"]["spread_pct"], p["ratio"]), "",
            "Not measured: other text lengths and counts, several queries a call, other cost tables, more than one GPU.", ""]
    return "\n".join(out)


if __name__ == "__main__":
    sys.exit(main())
