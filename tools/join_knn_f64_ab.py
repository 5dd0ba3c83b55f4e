"""The k nearest neighbours on the fp64 route (sed_join_knn_self_f64) against the two ways to get them
from the fp64 join itself, on one index in one process, the arms interleaved, --runs rounds each after one warm-up, the
spread reported.  Kernel ms from HIP events, every call a count query (cap = 0), so no hit list is stored or sorted:

  knn      self_knn_f64(k): both passes; pass 1's share (knn_bound_ms), the candidates pass 2 appends, the pairs run;
  join_T   self_join_f64(T_k), T_k = the smallest T at which every row has k hits (the largest k-th distance of the
           k-nearest result): what a caller who guessed T perfectly pays, before trimming the hits on the host;
  join_inf self_join_f64(+inf): the dense matrix as a hit list.

Workloads: --seqs sequences of U[24, 32] symbols, ACGU with 1 % ambiguity codes, under two tables: user_costs.json (over
ACGUN, 1 % N) and the 15-symbol costs.json (1 % drawn from its eleven ambiguity codes).

    python tools/join_knn_f64_ab.py [--runs 3] [--k 8] [--seqs 8192] [--out profiles/join_knn_f64]

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

IUPAC = "AGCUYRWSKMDVHBN"


def main():
    import numpy as np
    import sedcost
    import sedgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--seqs", default="8192")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "join_knn_f64"))
    a = ap.parse_args()
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
    for name, alphabet in (("user_costs.json", "ACGUN"), ("costs.json", IUPAC)):
        with open(os.path.join(REPO, "tests", "golden", name)) as f:
            table = json.load(f)
        plan = sedcost.plan_over(table, list(alphabet), set(alphabet), set(alphabet))
        ctx.set_costs(plan)
        base = [alphabet.index(c) for c in "ACGU"]
        amb = [i for i in range(len(alphabet)) if i not in base]
        for N in [int(x) for x in a.seqs.split(",") if x]:
            rng = np.random.default_rng(N + len(alphabet))
            seqs = []
            for n in rng.integers(24, 33, size=N):
                s = rng.choice(base, size=int(n))
                s[rng.random(int(n)) < 0.01] = rng.choice(amb)
                seqs.append(s.astype(np.uint8))
            ix = sedgpu.JoinIndex.from_seqs(ctx, seqs)
            full = ix.self_knn_f64(a.k)  # (also sizes the device list: no timed call repeats its second pass)
            assert len(full) == N * a.k
            T = float(full["dist"].max())
            bounds = ix.knn_bounds_f64()
            kth = full["dist"][a.k - 1::a.k]
            ms = {"knn": [], "knn_pass1": [], "join_T": [], "join_inf": []}
            seen = {}
            for r in range(a.runs + 1):  # (round 0 warms every arm up)
                count(lambda: ix.self_knn_f64(a.k, cap=0))
                t, t1 = ix.last_ms(), ix.knn_bound_ms()
                seen["knn"] = (ix.knn_candidates, ix.pairs_run())
                count(lambda: ix.self_join_f64(T, cap=0))
                tj = ix.last_ms()
                seen["join_T"] = (int(ix.found), ix.pairs_run())
                count(lambda: ix.self_join_f64(math.inf, cap=0))
                ti = ix.last_ms()
                seen["join_inf"] = (int(ix.found), ix.pairs_run())
                if r:
                    ms["knn"].append(t)
                    ms["knn_pass1"].append(t1)
                    ms["join_T"].append(tj)
                    ms["join_inf"].append(ti)
            knn, p1, jT, ji = (stats(ms[x]) for x in ("knn", "knn_pass1", "join_T", "join_inf"))
            emit(table=name, symbols=len(alphabet), seqs=N, lengths=[24, 32], k=a.k, pairs_in_scope=N * (N - 1),
                 knn_kernel_ms=knn, knn_pass1_ms=p1, pass1_share=round(p1["median"] / knn["median"], 3),
                 knn_candidates=seen["knn"][0], candidates_per_row=round(seen["knn"][0] / N, 2), knn_pairs_run=seen["knn"][1],
                 bound_mean=round(float(bounds.mean()), 3), kth_dist_mean=round(float(kth.mean()), 3), T_k=T,
                 join_T_kernel_ms=jT, join_T_hits=seen["join_T"][0], join_T_pairs_run=seen["join_T"][1],
                 join_inf_kernel_ms=ji, join_inf_hits=seen["join_inf"][0],
                 knn_over_join_T=round(knn["median"] / jT["median"], 3), knn_over_join_inf=round(knn["median"] / ji["median"], 3))
            ix.close()
    with open(os.path.join(a.out, "ab.jsonl"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
