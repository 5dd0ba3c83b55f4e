"""The long similarity join (sed_join_long_self) measured: kernel times by HIP events, the arms of a
part interleaved, --runs rounds each after one warm-up, the spread reported:

  kernels    --seqs sequences of U[60, 90] symbols at T = 2 and T = 8 as count queries, under user_costs.json (the scaled
             DP) and under the unit table over ACGU (bit-parallel): kernel ms, pairs run against pairs in scope, the
             plan's cells n m and lane cells, nominal cells / s;
  calls      the first --calls of those sequences as whole calls: wfsearch.neighbors(seqs, T, long_sequences=True)
             against the only route there was before, filtering sedshard.all_vs_all(seqs) (the dense matrix); the ratio;
  selectors  the DP launch of `kernels` at T = 8 through this library and through one built with the other selector
             layout (--selregs-lib; make -C rna-sequence-diff-patch_amd/csrc OBJDIR=../../tools/ab_libs/obj_selregs
             OUT=../../tools/ab_libs/libsed_selregs.so EXTRA=-DSED_JOIN_LONG_SELREGS), each arm a child process per
             round, the rounds alternating;
  short      --seqs sequences of U[24, 32] through the long and the short index, bit-parallel and DP forced.

    python tools/join_long_ab.py [--runs 5] [--seqs 8192] [--calls 1000] [--out profiles/join_long]

Writes ab.jsonl (one raw line per measurement) into --out."""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN = os.path.join(REPO, "tests", "golden")


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 5), "min": round(float(x.min()), 5), "max": round(float(x.max()), 5),
            "spread_pct": round(100 * float(x.max() - x.min()) / max(float(np.median(x)), 1e-12), 2), "runs": len(x)}


def collection(n, lo, hi, n_rate):
    """n code arrays of U[lo, hi] symbols over ACGU, n_rate of them N (code 4)."""
    import numpy as np
    rng = np.random.default_rng(n + lo)
    out = []
    for ln in rng.integers(lo, hi + 1, size=n):
        s = rng.integers(0, 4, size=int(ln)).astype(np.uint8)
        s[rng.random(int(ln)) < n_rate] = 4
        out.append(s)
    return out


def plans():
    import sedcost
    with open(os.path.join(GOLDEN, "user_costs.json")) as f:
        user = json.load(f)
    with open(os.path.join(GOLDEN, "costs.json")) as f:
        costs = json.load(f)
    return {"user_costs": sedcost.plan_over(user, list("ACGUN"), set("ACGUN"), set("ACGUN")),
            "unit": sedcost.plan_over(costs, list("ACGU"), set("ACGU"), set("ACGU"))}


def count_query(ix, T):
    import sedgpu
    try:
        ix.self_join(T, cap=0)
    except sedgpu.SedError:
        pass  # the count query's refusal for lack of room: found has the total
    return ix.last_ms()


def timed(ixs, T, runs):
    """{label: [ms]} of count queries on several indexes, interleaved, after one warm-up round."""
    ms = {k: [] for k in ixs}
    for r in range(runs + 1):
        for k, ix in ixs.items():
            t = count_query(ix, T)
            if r:
                ms[k].append(t)
    return ms


def child(a):
    """One arm of `selectors`: the DP launch at T = 8 under whatever library SED_LIBRARY names."""
    import sedgpu
    ctx = sedgpu.context()
    ctx.set_costs(plans()["user_costs"])
    ix = sedgpu.LongJoinIndex.from_seqs(ctx, collection(a.seqs, 60, 90, 0.01))
    ms = timed({"x": ix}, 8, a.runs)["x"]
    print(json.dumps({"ms": ms, "hits": int(ix.found), "pairs_run": ix.pairs_run()}))
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seqs", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--selregs-lib", default=os.path.join(REPO, "tools", "ab_libs", "libsed_selregs.so"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "join_long"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import sedgpu
    cwd = os.getcwd()
    os.chdir(GOLDEN)  # the drop-in module reads its cost tables from the working directory when it is imported
    try:
        wfsearch = importlib.import_module("wfsearch")
        sedshard = importlib.import_module("sedshard")
    finally:
        os.chdir(cwd)
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kv):
        lines.append(kv)
        print(json.dumps(kv), flush=True)

    ctx = sedgpu.context()
    P = plans()
    costs_of = lambda p: (p.K, p.sub, p.sub_int, p.ins, p.ins_int, p.dele, p.del_int)
    # ---- kernels ----
    for table, n_rate in (("user_costs", 0.01), ("unit", 0.0)):
        plan = P[table]
        ctx.set_costs(plan)
        seqs = collection(a.seqs, 60, 90, n_rate)
        lens = [len(s) for s in seqs]
        mask = sedgpu.codes_seen(__import__("numpy").concatenate(seqs))
        ix = sedgpu.LongJoinIndex.from_seqs(ctx, seqs)
        for T in (2, 8):
            ms = timed({"long": ix}, T, a.runs)["long"]
            p = sedgpu.join_long_plan(costs_of(plan), {}, lens, lens, True, mask, mask, T)
            med = stats(ms)["median"]
            emit(part="kernels", table=table, seqs=a.seqs, lengths="60..90", T=T, kernel=sedgpu.JOIN_KERNELS[p["kernel"]],
                 hits=int(ix.found), pairs_run=ix.pairs_run(), pairs_in_scope=p["scope"], cells=p["cells"],
                 lane_cells=p["lane_cells"], kernel_ms=stats(ms), nominal_cells_per_s=p["cells"] / (med * 1e-3))
        ix.close()
        # ---- the same collection's head as whole calls, against the dense route ----
        strs = ["".join("ACGUN"[c] for c in s) for s in seqs[:a.calls]]
        user = table == "user_costs"
        for T in (2, 8):
            new_s, old_s = [], []
            for r in range(min(a.runs, 3) + 1):
                t0 = time.perf_counter()
                nb = wfsearch.neighbors(strs, T, user, long_sequences=True)
                t1 = time.perf_counter()
                M = sedshard.all_vs_all(strs, user)
                old = [(i, j, 1 / (1 + M[i, j])) for i in range(len(strs)) for j in range(len(strs)) if i != j and M[i, j] <= T]
                t2 = time.perf_counter()
                assert nb == old
                if r:
                    new_s.append(t1 - t0)
                    old_s.append(t2 - t1)
            emit(part="calls", table=table, seqs=len(strs), T=T, hits=len(nb), neighbors_long_s=stats(new_s),
                 all_vs_all_filter_s=stats(old_s), ratio=stats(old_s)["median"] / stats(new_s)["median"])
    # ---- short sequences through both indexes ----
    for table, forced in (("unit", False), ("unit", True)):
        plan = P[table]
        ctx.set_costs(plan)
        ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 2 if forced else 0)
        seqs = collection(a.seqs, 24, 32, 0.0)
        ixs = {"long": sedgpu.LongJoinIndex.from_seqs(ctx, seqs), "short": sedgpu.JoinIndex.from_seqs(ctx, seqs)}
        for T in (2, math.inf):
            ms = timed(ixs, T, a.runs)
            assert ixs["long"].found == ixs["short"].found and ixs["long"].pairs_run() == ixs["short"].pairs_run()
            emit(part="short", seqs=a.seqs, lengths="24..32", T=str(T), kernel="dp" if forced else "bitpar",
                 hits=int(ixs["long"].found), pairs_run=ixs["long"].pairs_run(), long_ms=stats(ms["long"]),
                 short_ms=stats(ms["short"]), long_over_short=stats(ms["long"])["median"] / stats(ms["short"])["median"])
        for ix in ixs.values():
            ix.close()
    ctx.set_option(sedgpu.SED_OPT_JOIN_DP, 0)
    ctx.close()
    # ---- the two selector layouts, a child process per arm and round ----
    if os.path.exists(a.selregs_lib):
        arms = {"code_words": sedgpu.LIB_PATH, "selector_registers": a.selregs_lib}
        ms = {k: [] for k in arms}
        seen = {}
        for _ in range(a.rounds):
            for k, lib in arms.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(a.runs), "--seqs",
                                      str(a.seqs)], env=dict(os.environ, SED_LIBRARY=lib), capture_output=True, text=True,
                                     timeout=300, check=True).stdout
                got = json.loads(out.strip().splitlines()[-1])
                ms[k] += got["ms"]
                seen.setdefault("hits", got["hits"])
                assert seen["hits"] == got["hits"]
        emit(part="selectors", seqs=a.seqs, T=8, hits=seen["hits"], code_words_ms=stats(ms["code_words"]),
             selector_registers_ms=stats(ms["selector_registers"]),
             selector_registers_over_code_words=stats(ms["selector_registers"])["median"] / stats(ms["code_words"])["median"])
    else:
        emit(part="selectors", measured=False, why="no library at %s" % a.selregs_lib)
    with open(os.path.join(a.out, "ab.jsonl"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
