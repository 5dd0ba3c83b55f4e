"""Fit search's fp64 route (sed_fit_index_search_f64) on 3.6f's workload: one 28-nt query against 8192
texts of 4096 nt.  After one warm-up of every variant the variants run interleaved, --runs times each, on one otherwise
idle GPU; kernel times are the engine's HIP events (the fp64 time includes its per-pair reduce kernel).

  (a) user_costs.json over ACGU, a table both routes serve: sed_fit_index_search_f64 against sed_fit_index_kernel on
      the same lanes (the same forced chunk; the fp64 window is 2 columns longer).  The results must be equal.
  (b) costs.json over all 15 IUPAC symbols, 1 % of the text symbols ambiguity codes (D, V, H among them), which only
      the fp64 route serves: the kernel against the 16-thread C oracle on a sample of the texts.  Equal results.

The expectation for (a) is stated before the run, from instruction counts (EXPECTATION below).

    python tools/fit_f64_ab.py [--texts 8192] [--length 4096] [--runs 7] [--out profiles/fit_f64]

Writes ab.json into --out; profiles/fit_f64/README.md holds the expectation and the reading of the numbers."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

IUPAC = "AGCUYRWSKMDVHBN"
# Per cell, from the disassembly of the two loops (tools/kernel_resources.py counts; llvm-objdump for the mix):
#   integer (sed_fit_index_kernel): v_perm_b32 + v_sub_u32 + v_min3_u32 = 3 VALU, no memory access;
#   fp64 (sed_fit_index_f64_kernel): 3 v_add_f64, 2 x (v_cmp_lt_f64, v_cmp_eq_f64, v_cmp_gt_i32), 9 v_cndmask_b32
#   (two 3-register selects of (D, start) and the front-row overwrite), 1 address add = 19 VALU, plus 4 scalar mask
#   operations and one ds_read_b64 of the cost table, about 1.6 v_readlane/v_writelane of spilled masks.
# Assumed: v_add_f64 and the fp64 compares issue at the rate of 32-bit VALU on CDNA4's vector unit (4 cycles a wave64),
# so the ratio of VALU instructions is the ratio of times at equal occupancy: 19 / 3 = 6.3.  The fp64 kernel holds 2 to 3
# waves a SIMD against the integer kernel's 4 and waits on an LDS read per cell (lanes of a wave read different
# entries: bank conflicts), neither of which the count covers: expected 6.3x at best, up to about 10x.
EXPECTATION = {"valu_per_cell_f64": 19, "valu_per_cell_int": 3, "ratio_from_valu": round(19 / 3, 2), "ratio_upper": 10.0,
               "assumed_fp64_issue": "v_add_f64 / v_cmp_*_f64 at the 32-bit VALU rate (4 cycles per wave64)"}


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "spread_pct": round(100 * float(x.max() - x.min()) / float(np.median(x)), 2)}


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_f64"))
    a = ap.parse_args()
    golden = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(golden, "user_costs.json")) as f:
        user = json.load(f)
    with open(os.path.join(golden, "costs.json")) as f:
        default = json.load(f)
    P = 28
    rng = np.random.default_rng(28)
    ctx = sedgpu.context()
    CH = sedgpu.SED_OPT_FIT_CHUNK
    lens = [a.length] * a.texts
    res = {"texts": a.texts, "length": a.length, "runs": a.runs, "P": P, "device": _device_name(), "expectation": EXPECTATION}

    # (a) the dyadic 4-symbol table, both routes on the same lanes
    plan = sedcost.build_plan(user, ["ACGU"], ["ACGU"])
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    pat = rng.integers(0, 4, size=P).astype(np.uint8)
    docs = rng.integers(0, 4, size=(a.texts, a.length)).astype(np.uint8)
    for d in range(0, a.texts, 100):  # 1 % of the texts hold a copy with 10 % substitutions
        m = np.where(rng.random(P) < 0.1, rng.integers(0, 4, size=P), pat).astype(np.uint8)
        at = int(rng.integers(0, a.length - P + 1))
        docs[d, at:at + P] = m
    ctx.set_costs(plan)
    ix = sedgpu.FitIndex.from_texts(ctx, list(docs))
    q = sedgpu.PackedPairs([pat], [np.zeros(0, np.uint8)])
    pi, pf = sedgpu.fit_index_plan(costs, {}, [P], lens), sedgpu.fit_index_f64_plan(costs, {}, [P], lens)
    chunk = pf["chunk"] or a.length + 1
    ti, tf = [], []
    for it in range(a.runs + 1):  # (run 0 warms both up)
        ctx.set_option(CH, chunk)
        gi = ix.search(q)
        mi = ix.last_ms()
        gf = ix.search_f64(q)
        mf = ix.last_ms()
        ctx.set_option(CH, 0)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(gi, gf))
        if it:
            ti.append(mi)
            tf.append(mf)
    ix.close()
    nominal = float(P) * a.length * a.texts
    fl = sedgpu.fit_index_f64_plan(costs, {CH: chunk}, [P], lens)
    il = sedgpu.fit_index_plan(costs, {CH: chunk}, [P], lens)
    res["a"] = {"table": "user_costs.json over ACGU", "chunk": chunk, "auto_chunk_int": pi["chunk"], "W_int": il["W"],
                "W_f64": fl["W"], "lanes": fl["lanes"], "int_ms": stats(ti), "f64_ms": stats(tf),
                "ratio": round(stats(tf)["median"] / stats(ti)["median"], 3),
                "f64_cells_per_s": 32 * fl["cells"] / P / (stats(tf)["median"] * 1e-3),
                "int_cells_per_s": 32 * il["cells"] / P / (stats(ti)["median"] * 1e-3),
                "f64_nominal_cells_per_s": nominal / (stats(tf)["median"] * 1e-3)}
    print(json.dumps({"a": res["a"]}), flush=True)

    # (b) the 15-symbol table, 1 % ambiguity codes
    plan = sedcost.build_plan(default, [IUPAC], [IUPAC])
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    code = {c: k for k, c in enumerate(plan.alphabet)}
    acgu = np.array([code[c] for c in "ACGU"], np.uint8)
    amb = np.array([code[c] for c in IUPAC if c not in "ACGU"], np.uint8)
    docs = acgu[rng.integers(0, 4, size=(a.texts, a.length))]
    mask = rng.random(docs.shape) < 0.01
    docs[mask] = amb[rng.integers(0, len(amb), size=int(mask.sum()))]
    pat = acgu[rng.integers(0, 4, size=P)]
    pat[5] = code["D"]
    ctx.set_costs(plan)
    assert sedgpu.fit_route(costs, {}, [P], [a.length])[0] == "f64"
    ix = sedgpu.FitIndex.from_texts(ctx, list(docs))
    q = sedgpu.PackedPairs([pat], [np.zeros(0, np.uint8)])
    tb, got = [], None
    for it in range(a.runs + 1):
        got = ix.search_f64(q)
        if it:
            tb.append(ix.last_ms())
    ix.close()
    ns = min(a.sample, a.texts)
    pk = sedgpu.PackedPairs([pat] * ns, list(docs[:ns]))
    t0 = time.perf_counter()
    od, os_, oe = oracle.fit(oracle.Costs.from_plan(plan), pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b, ns, 16)
    cpu_s = time.perf_counter() - t0
    assert od.tobytes() == got[0][0, :ns].tobytes() and np.array_equal(os_, got[1][0, :ns]) and np.array_equal(oe, got[2][0, :ns])
    pb = sedgpu.fit_index_f64_plan(costs, {}, [P], lens)
    res["b"] = {"table": "costs.json over %s, 1 %% ambiguity codes" % IUPAC, "chunk": pb["chunk"], "W": pb["W"],
                "lanes": pb["lanes"], "f64_ms": stats(tb), "f64_nominal_cells_per_s": nominal / (stats(tb)["median"] * 1e-3),
                "oracle_16_threads": {"texts": ns, "seconds": round(cpu_s, 4), "nominal_cells_per_s": P * a.length * ns / cpu_s}}
    res["b"]["speedup_over_oracle"] = round(res["b"]["f64_nominal_cells_per_s"] /
                                            res["b"]["oracle_16_threads"]["nominal_cells_per_s"], 1)
    print(json.dumps({"b": res["b"]}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def _device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        return "unknown"


if __name__ == "__main__":
    sys.exit(main())
