"""The k nearest neighbours of every sequence (sed_join_knn_self) against the two ways to get them from
the join itself, on one index in one process, the arms interleaved, --runs rounds each after one warm-up, the spread
reported.  Kernel ms from HIP events, every call a count query (cap = 0), so no hit list is stored or sorted:

  knn      self_knn(k): both passes; pass 1's share (knn_bound_ms), the candidates pass 2 appends, the pairs run;
  join_T   self_join(T_k), T_k = the smallest T at which every row has k hits (the largest k-th distance of the
           k-nearest result): what a caller who guessed T perfectly pays, before trimming `hits` records on the host;
  join_inf self_join(+inf): the dense matrix as a hit list.

Workloads: --short sequences of U[24, 32] on the short index, --long sequences of U[60, 90] on the long index, over
ACGU under costs.json; each with the variant the planner picks (bit-parallel) and with the scaled DP forced.

    python tools/join_knn_ab.py [--runs 3] [--k 8] [--short 8192,65536] [--long 8192] [--out profiles/join_knn]

Writes ab.jsonl (one raw line per measurement) into --out."""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from join_ab import stats  # noqa: E402


def main():
    import numpy as np
    import sedcost
    import sedgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--short", default="8192,65536")
    ap.add_argument("--long", default="8192")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "join_knn"))
    a = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "costs.json")) as f:
        table = json.load(f)
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kv):
        lines.append(kv)
        print(json.dumps(kv), flush=True)

    def count(call):
        try:
            call()
        except sedgpu.SedError:
            pass  # the count query's refusal for lack of room: found has the total

    ctx = sedgpu.context()
    plan = sedcost.plan_over(table, list("ACGU"), set("ACGU"), set("ACGU"))
    ctx.set_costs(plan)
    work = [("short", int(x), 24, 32) for x in a.short.split(",") if x] + [("long", int(x), 60, 90) for x in a.long.split(",") if x]
    for kind, N, lo, hi in work:
        rng = np.random.default_rng(N + hi)
        seqs = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(lo, hi + 1, size=N)]
        ix = (sedgpu.LongJoinIndex if kind == "long" else sedgpu.JoinIndex).from_seqs(ctx, seqs)
        scope = N * (N - 1)
        for forced in (False, True):
            ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
            full = ix.self_knn(a.k)  # (also sizes the device list: no timed call repeats its second pass)
            assert len(full) == N * a.k
            T = float(full["dist"].max())
            bounds = ix.knn_bounds()
            kth = full["dist"][a.k - 1::a.k]
            ms = {"knn": [], "knn_pass1": [], "join_T": [], "join_inf": []}
            seen = {}
            for r in range(a.runs + 1):  # (round 0 warms every arm up)
                count(lambda: ix.self_knn(a.k, cap=0))
                t, t1 = ix.last_ms(), ix.knn_bound_ms()
                seen["knn"] = (ix.knn_candidates, ix.pairs_run())
                count(lambda: ix.self_join(T, cap=0))
                tj = ix.last_ms()
                seen["join_T"] = (int(ix.found), ix.pairs_run())
                count(lambda: ix.self_join(math.inf, cap=0))
                ti = ix.last_ms()
                seen["join_inf"] = (int(ix.found), ix.pairs_run())
                if r:
                    ms["knn"].append(t)
                    ms["knn_pass1"].append(t1)
                    ms["join_T"].append(tj)
                    ms["join_inf"].append(ti)
            knn, p1 = stats(ms["knn"]), stats(ms["knn_pass1"])
            emit(index=kind, seqs=N, lengths=[lo, hi], k=a.k, kernel="dp" if forced else "bitpar", pairs_in_scope=scope,
                 knn_kernel_ms=knn, knn_pass1_ms=p1, pass1_share=round(p1["median"] / knn["median"], 3),
                 knn_candidates=seen["knn"][0], candidates_per_row=round(seen["knn"][0] / N, 2), knn_pairs_run=seen["knn"][1],
                 bound_mean=round(float(bounds.mean()), 2), kth_dist_mean=round(float(kth.mean()), 2), T_k=T,
                 join_T_kernel_ms=stats(ms["join_T"]), join_T_hits=seen["join_T"][0], join_T_pairs_run=seen["join_T"][1],
                 join_inf_kernel_ms=stats(ms["join_inf"]), join_inf_hits=seen["join_inf"][0])
        ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
        ix.close()
    with open(os.path.join(a.out, "ab.jsonl"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
