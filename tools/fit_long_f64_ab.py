"""Long fit search in fp64 (sed_fit_index_search_long_f64): one query of P = 76, 256 and 1024 against
8192 texts of 4096 nt.  After one warm-up of every variant the variants run interleaved, --runs times each, on one
otherwise idle GPU; kernel times are the engine's HIP events (the fp64 search's include its reduce kernel).

  (a) user_costs.json over ACGU: sed_fit_index_search_long_f64 interleaved with sed_fit_index_search_long on the same
      waves (the automatic chunk of the integer plan, forced for both); the integer kernel is the yardstick, the
      results must be equal bit for bit, and the ratio is expected near the ratio of VALU instructions a cell.
  (b) costs.json over the 15 IUPAC symbols, 1 % ambiguity codes in the texts: only this route serves it; against the
      16-thread C oracle on a sample of the texts, whose hits it must equal.

Cell updates are counted with the skew and the warm-up columns: a wave of R rows a lane updates 64 R cells in each of
its steps.  The expectation is stated before the run: sed_fit_index_f64_kernel's measured 9.1e11 cells/s at 19 VALU
instructions a cell, scaled by 19 / the VALU instructions a cell counted in this kernel's disassembly
at each R (VALU_PER_CELL below).

    python tools/fit_long_f64_ab.py [--texts 8192] [--length 4096] [--runs 7] [--out profiles/fit_long_f64]

Writes ab.json and README.md into --out."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHORT_F64_RATE = 9.1e11   # sed_fit_index_f64_kernel, nominal cells/s, measured
SHORT_F64_VALU = 19       # its VALU instructions a cell
# VALU instructions of sed_fit_index_long_f64_kernel<R> over (columns unrolled x R): an upper bound of the step's
# instructions a cell (the prologue is in the count)
VALU_PER_CELL = {2: 38.0, 4: 30.8, 8: 27.1, 16: 25.8, 32: 32.8}
INT_PER_CELL = {R: (3 * R + 24) / R for R in VALU_PER_CELL}  # sed_fit_index_long_kernel
IUPAC = "AGCUYRWSKMDVHBN"


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "spread_pct": round(100 * float(x.max() - x.min()) / float(np.median(x)), 2)}


def counted_cells(sedgpu, costs, opts, P, lens, R):
    """64 R cells in every step of every wave: nsteps + 63 steps, rounded up to a text word's four."""
    ns = sedgpu.fit_index_long_f64_lanes(costs, opts, [P], lens)["nsteps"]
    steps = (ns > 0) * ((ns + 63 + 3) // 4 * 4)
    return float(64 * R * steps.sum()), int(len(ns))


def _device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        return "unknown"


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_long_f64"))
    a = ap.parse_args()
    golden = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(golden, "user_costs.json")) as f:
        user = sedcost.build_plan(json.load(f), ["ACGU"], ["ACGU"])
    with open(os.path.join(golden, "costs.json")) as f:
        iupac = sedcost.build_plan(json.load(f), [IUPAC], [IUPAC])
    costs_of = lambda p: (p.K, p.sub, p.sub_int, p.ins, p.ins_int, p.dele, p.del_int)
    lens = [a.length] * a.texts
    ctx = sedgpu.context()
    CH = sedgpu.SED_OPT_FIT_CHUNK
    res = {"texts": a.texts, "length": a.length, "runs": a.runs, "device": _device_name(), "a_user_costs": {}, "b_costs15": {}}

    def run(call, q, chunk):
        ctx.set_option(CH, chunk)
        out = call(q)
        ctx.set_option(CH, 0)
        return out

    for P in (76, 256, 1024):
        for key, plan, K in (("a_user_costs", user, 4), ("b_costs15", iupac, 4)):
            rng = np.random.default_rng(P)
            pat = rng.integers(0, K, size=P).astype(np.uint8)
            docs = rng.integers(0, 4, size=(a.texts, a.length)).astype(np.uint8)
            if key == "b_costs15":  # 1 % ambiguity codes (codes 4..14 of the 15-symbol plan)
                amb = rng.random(docs.shape) < 0.01
                docs[amb] = rng.integers(4, 15, size=int(amb.sum())).astype(np.uint8)
            for d in range(0, a.texts, 100):  # 1 % of the texts hold a copy with 10 % substitutions
                m = np.where(rng.random(P) < 0.1, rng.integers(0, K, size=P), pat).astype(np.uint8)
                at = int(rng.integers(0, a.length - P + 1))
                docs[d, at:at + P] = m
            ctx.set_costs(plan)
            ix = sedgpu.FitIndex.from_texts(ctx, list(docs))
            q = sedgpu.PackedPairs([pat], [np.zeros(0, np.uint8)])
            costs = costs_of(plan)
            auto = sedgpu.fit_index_long_f64_plan(costs, {}, [P], lens)
            R = int(auto["rows"][0])
            chunk = auto["chunk"] or a.length + 1
            variants = {"long_f64": ix.search_long_f64}
            if key == "a_user_costs":
                variants["long_int"] = ix.search_long
            times = {k: [] for k in variants}
            want = None
            for it in range(a.runs + 1):  # (run 0 warms every variant up)
                for k, call in variants.items():
                    got = run(call, q, chunk)
                    want = want or [x.copy() for x in got]
                    assert all(np.array_equal(x, y) for x, y in zip(got, want)), (P, k)
                    if it:
                        times[k].append(ix.last_ms())
            ix.close()
            cells, waves = counted_cells(sedgpu, costs, {CH: chunk}, P, lens, R)
            entry = {"rows": R, "W": auto["W"], "chunk": chunk, "waves": waves, "counted_cells": cells,
                     "expected_counted_cells_per_s": SHORT_F64_RATE * SHORT_F64_VALU / VALU_PER_CELL[R], "variants": {}}
            for k in variants:
                st = stats(times[k])
                st.update({"counted_cells_per_s": cells / (st["median"] * 1e-3),
                           "nominal_cells_per_s": P * a.length * a.texts / (st["median"] * 1e-3)})
                entry["variants"][k] = st
            if key == "a_user_costs":
                entry["ratio_f64_over_int"] = round(entry["variants"]["long_f64"]["median"] / entry["variants"]["long_int"]["median"], 3)
                entry["expected_ratio"] = round(VALU_PER_CELL[R] / INT_PER_CELL[R], 2)
            else:
                ns = min(a.sample, a.texts)
                pk = sedgpu.PackedPairs([pat] * ns, list(docs[:ns]))
                t0 = time.perf_counter()
                od, os_, oe = oracle.fit(oracle.Costs.from_plan(plan), pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b,
                                         pk.len_b, ns, 16)
                cpu_s = time.perf_counter() - t0
                assert np.array_equal(od, want[0][0, :ns]) and np.array_equal(os_, want[1][0, :ns]) and np.array_equal(oe, want[2][0, :ns])
                entry["oracle_16_threads"] = {"texts": ns, "seconds": round(cpu_s, 4), "nominal_cells_per_s": P * a.length * ns / cpu_s}
            res[key][str(P)] = entry
            print(json.dumps({key: {str(P): entry}}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))


def readme(r):
    out = ["# Long fit search in fp64: measurements (DESIGN.md 3.6j)", "",
           "Written by `tools/fit_long_f64_ab.py`; the raw numbers are in `ab.json`.", "",
           "Workload: one query of P symbols against %d texts of %d nt; device %s; %d runs of every variant after one"
           " warm-up, variants interleaved run by run, one process, nothing else on the GPU.  Kernel ms are HIP events around"
           " the launches (the fp64 search's include its reduce kernel).  Counted cells = 64 R cells for every step of every"
           " wave (skew and warm-up columns included); nominal cells = P x text symbols." % (r["texts"], r["length"], r["device"], r["runs"]),
           "", "Expectation, stated before the run: %.1e cells/s (`sed_fit_index_f64_kernel`, measured, %d VALU instructions a"
           " cell) x %d / the VALU instructions a cell of this kernel's disassembly (%s).  A prediction only." % (
               SHORT_F64_RATE, SHORT_F64_VALU, SHORT_F64_VALU, ", ".join("R = %d: %.1f" % kv for kv in VALU_PER_CELL.items())),
           "", "## (a) `user_costs.json` over ACGU, against `sed_fit_index_search_long` on the same waves", "",
           "| P | R | chunk | waves | kernel | median ms | min | max | spread | counted cells/s | expected | nominal cells/s |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def rows(sec):
        for P, e in r[sec].items():
            for k, v in e["variants"].items():
                out.append("| %s | %d | %d | %d | %s | %s | %s | %s | %s %% | %.3g | %s | %.3g |"
                           % (P, e["rows"], e["chunk"], e["waves"], k, v["median"], v["min"], v["max"], v["spread_pct"],
                              v["counted_cells_per_s"], "%.3g" % e["expected_counted_cells_per_s"] if k == "long_f64" else "",
                              v["nominal_cells_per_s"]))
    rows("a_user_costs")
    out += ["", "| P | fp64 / integer, measured | expected from the instruction counts |", "|---|---|---|"]
    for P, e in r["a_user_costs"].items():
        out.append("| %s | %s | %s |" % (P, e["ratio_f64_over_int"], e["expected_ratio"]))
    out += ["", "## (b) `costs.json` over 15 IUPAC symbols, 1 % ambiguity codes: only this route serves it", "",
            "| P | R | chunk | waves | kernel | median ms | min | max | spread | counted cells/s | expected | nominal cells/s |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rows("b_costs15")
    out += ["", "| P | 16-thread C oracle, nominal cells/s (sample of texts) | GPU, nominal cells/s |", "|---|---|---|"]
    for P, e in r["b_costs15"].items():
        o = e["oracle_16_threads"]
        out.append("| %s | %.3g (%d texts, %s s) | %.3g |" % (P, o["nominal_cells_per_s"], o["texts"], o["seconds"],
                                                               e["variants"]["long_f64"]["nominal_cells_per_s"]))
    out += ["", "Not measured: the hits kernel, several queries a call, R = 8 and 32, forced chunks, other text counts and"
            " lengths, other cost tables, more than one GPU.", ""]
    return "\n".join(out)


if __name__ == "__main__":
    sys.exit(main())
