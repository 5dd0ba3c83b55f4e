"""The fp64 route of the similarity join (sed_join_self_f64) in one process, the arms interleaved, --runs
rounds each after one warm-up, the spread reported:

  both     user_costs.json over ACGUN, which both routes serve: kernel ms (HIP events) of sed_join_self_f64 against
           sed_join_self with the DP variant forced (SED_OPT_JOIN_DP = 2), as count queries, on the 500 sequences of
           bench.gen_all_vs_all(500, n_rate=0.01) at T = +inf and on --scale sequences of U[24, 32] at T = 2;
  iupac    costs.json over its 15 symbols with 1 % ambiguity codes, which only this route serves: the same two sizes,
           kernel ms, pairs run against pairs in scope, cells per second;
  calls    the 500-sequence IUPAC set as whole calls: wfsearch.neighbors(seqs, 2, route="f64") against filtering
           sedshard.all_vs_all(seqs);
  oracle   the C oracle (16 threads) on a sample of --oracle-pairs pairs of the IUPAC set.

Expected ratio of the two row loops, from the compiled code (one trip = one DP row of 32 cells):
  integer DP   98 VALU: 32 v_perm_b32, 32 v_add_u32, 32 v_min3_u32, 2 v_mov
  fp64        225 VALU: 96 v_add_f64, 64 v_min_f64, 32 v_add_u32_sdwa (the table address), 31 v_mov_b64 (the diagonal's
              copies), 1 v_cvt + 1 v_mul_f64 (column 0); and 32 ds_read_b64
so 2.3x by instruction count.  By issue rate (profiles/r04/s7/ubench_valu_f64.txt: v_add_f64 4.67, v_min_f64 4.59,
v_min3_u32 4.59, v_add_u32 2.63 cycles; v_perm_b32, the sdwa add and v_mov_b64 taken at 4.5, not measured) a row is about
1040 against 380 cycles: 2.7x.  The sink adds 66 v_cndmask_b32 per (row, wave) against 35, row 0 adds 29 v_mul_f64.

    python tools/join_f64_ab.py [--runs 5] [--scale 8192] [--out profiles/join_f64]

Writes ab.jsonl (one raw line per measurement) into --out."""
import argparse
import importlib
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

IUPAC = "AGCUYRWSKMDVHBN"


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 5), "min": round(float(x.min()), 5), "max": round(float(x.max()), 5),
            "spread_pct": round(100 * float(x.max() - x.min()) / max(float(np.median(x)), 1e-12), 2), "runs": len(x)}


def count_query(call):
    import sedgpu
    try:
        call()
    except sedgpu.SedError:
        pass  # the count query's refusal for lack of room: found has the total


def main():
    import numpy as np
    import bench
    import oracle
    import sedcost
    import sedgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=int, default=8192)
    ap.add_argument("--oracle-pairs", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "join_f64"))
    a = ap.parse_args()
    golden = os.path.join(REPO, "tests", "golden")
    cwd = os.getcwd()
    os.chdir(golden)  # the drop-in module reads its cost tables from the working directory when it is imported
    try:
        wfsearch = importlib.import_module("wfsearch")
        sedshard = importlib.import_module("sedshard")
    finally:
        os.chdir(cwd)
    tables = {}
    for name in ("costs.json", "user_costs.json"):
        with open(os.path.join(golden, name)) as f:
            tables[name] = json.load(f)
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kv):
        lines.append(kv)
        print(json.dumps(kv), flush=True)

    def costs_of(plan):
        return (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)

    def ambiguous(seqs, rng, rate=0.01):
        """ACGU codes (0..3 = AGCU of IUPAC's order) with `rate` of the symbols replaced by ambiguity codes 4..14"""
        out = []
        for s in seqs:
            s = np.asarray(s, np.uint8) % 4
            hit = rng.random(len(s)) < rate
            s = np.where(hit, rng.integers(4, 15, size=len(s)), s).astype(np.uint8)
            out.append(s)
        return out

    ctx = sedgpu.context()
    uplan = sedcost.plan_over(tables["user_costs.json"], list("ACGUN"), set("ACGUN"), set("ACGUN"))
    iplan = sedcost.plan_over(tables["costs.json"], list(IUPAC), set(IUPAC), set(IUPAC))
    rng = np.random.default_rng(a.scale)
    small = bench.gen_all_vs_all(500, n_rate=0.01)[1][:500]
    big = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(24, 33, size=a.scale)]
    sets = (("config5_500", small, math.inf), ("u24_32_%d" % a.scale, big, 2.0))
    # ---- both routes on a table both serve ----
    ctx.set_costs(uplan)
    for label, seqs, T in sets:
        ix = sedgpu.JoinIndex.from_seqs(ctx, seqs)
        lens = [len(s) for s in seqs]
        mask = sedgpu.codes_seen(np.concatenate(seqs))
        f64_ms, int_ms = [], []
        for r in range(a.runs + 1):  # (round 0 warms both arms up)
            count_query(lambda: ix.self_join_f64(T, cap=0))
            f_found, f_run, f_t = ix.found, ix.pairs_run(), ix.last_ms()
            ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 2)
            count_query(lambda: ix.self_join(T, cap=0))
            ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
            assert ix.found == f_found
            if r:
                f64_ms.append(f_t)
                int_ms.append(ix.last_ms())
        pf = sedgpu.join_f64_plan(costs_of(uplan), {}, lens, lens, True, mask, mask, T)
        pi = sedgpu.join_plan(costs_of(uplan), {sedgpu.SED_OPT_JOIN_DP: 2}, lens, lens, True, mask, mask, T)
        fs, is_ = stats(f64_ms), stats(int_ms)
        emit(part="both", table="user_costs", set=label, T=str(T), hits=int(f_found), f64_pairs_run=f_run,
             int_pairs_run=pi["run"], pairs_in_scope=pf["scope"], f64_kernel_ms=fs, int_dp_kernel_ms=is_,
             ratio_of_medians=round(fs["median"] / is_["median"], 3), predicted_by_count=2.3, predicted_by_rate=2.7)
        ix.close()
    # ---- the IUPAC table, which only the fp64 route serves ----
    ctx.set_costs(iplan)
    for label, seqs, T in sets:
        seqs = ambiguous(seqs, np.random.default_rng(len(seqs)))
        ix = sedgpu.JoinIndex.from_seqs(ctx, seqs)
        lens = [len(s) for s in seqs]
        mask = sedgpu.codes_seen(np.concatenate(seqs))
        ms = []
        for r in range(a.runs + 1):
            count_query(lambda: ix.self_join_f64(T, cap=0))
            if r:
                ms.append(ix.last_ms())
        p = sedgpu.join_f64_plan(costs_of(iplan), {}, lens, lens, True, mask, mask, T)
        st = stats(ms)
        emit(part="iupac", table="costs", set=label, T=str(T), symbols=bin(mask).count("1"), hits=int(ix.found),
             pairs_run=ix.pairs_run(), pairs_in_scope=p["scope"], cells=p["cells"], kernel_ms=st,
             cells_per_s=round(p["cells"] / (st["median"] * 1e-3), 1),
             lane_cells_per_s=round(ix.pairs_run() * 32.0 * float(np.mean(lens)) / (st["median"] * 1e-3), 1))
        ix.close()
        if len(seqs) == 500:
            strs = ["".join(IUPAC[c] for c in s) for s in seqs]
            new_s, old_s = [], []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                nb = wfsearch.neighbors(strs, 2, route="f64")
                t1 = time.perf_counter()
                M = sedshard.all_vs_all(strs)
                old = [(i, j, 1 / (1 + M[i, j])) for i in range(len(strs)) for j in range(len(strs))
                       if i != j and M[i, j] <= 2]
                t2 = time.perf_counter()
                same = nb == old
                if r:
                    new_s.append(t1 - t0)
                    old_s.append(t2 - t1)
            emit(part="calls", table="costs", set=label, T=2, hits=len(nb), equal=same, neighbors_f64_s=stats(new_s),
                 all_vs_all_filter_s=stats(old_s))
            # the C oracle, 16 threads, on a sample of the pairs
            n = min(a.oracle_pairs, 500 * 499)
            pr = np.random.default_rng(1)
            ii, jj = pr.integers(0, 500, size=n), pr.integers(0, 500, size=n)
            pp = sedgpu.PackedPairs([seqs[i] for i in ii], [seqs[j] for j in jj])
            cs = oracle.Costs.from_plan(iplan)
            secs = []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                oracle.batch(cs, pp.codes_a, pp.off_a, pp.len_a, pp.codes_b, pp.off_b, pp.len_b, pp.npairs, nthreads=16)
                if r:
                    secs.append(time.perf_counter() - t0)
            st = stats(secs)
            cells = float(np.sum(pp.len_a.astype(np.float64) * pp.len_b))
            emit(part="oracle", table="costs", set=label, pairs=n, threads=16, seconds=st,
                 pairs_per_s=round(n / st["median"], 1), cells_per_s=round(cells / st["median"], 1))
    with open(os.path.join(a.out, "ab.jsonl"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
