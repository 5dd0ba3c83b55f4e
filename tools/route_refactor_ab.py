"""Host time per call of the fit and join entry points, one library against another (SED_LIBRARY), for a change that
must leave it alone: the eight index calls (search / hits x short / long x integer / fp64), the two pair calls and ten
join calls (self / search x integer / fp64; the k-nearest self and search calls, the fp64 k-nearest self call; the long
index's self, search and k-nearest self calls), each on the smallest workload of its own tools/fit_*_ab.py or
tools/join*_ab.py.

A library is a process (sedgpu binds one per process), so the two alternate as processes, --rounds of each: every
process builds the same seeded inputs, warms every call up once and then times --runs calls of each with a host clock
around the call, which ends in the stream's synchronise.  Reported per entry point: the median over all timed calls of
each library, the base library's spread (the least and the largest of its own timed calls, all rounds), and whether the
other library's median lies within it.  Kernel ms (HIP events) ride along to show what share of the call is host time.

    python tools/route_refactor_ab.py --base tools/ab_libs/parent.so [--new rna-sequence-diff-patch_amd/libsed.so]
                                      [--base-package DIR] [--rounds 3] [--runs 7] [--out profiles/route_refactor]

Writes ab.json and README.md into --out."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SED_AB_PACKAGE: the folder of the sedgpu.py a worker imports (--base-package sets it for the base library's workers)
for p in (os.environ.get("SED_AB_PACKAGE") or os.path.join(REPO, "rna-sequence-diff-patch_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
IUPAC = "AGCUYRWSKMDVHBN"
KNN_K = 8  # tools/join_knn_ab.py, join_knn_f64_ab.py


def worker(a):
    """One library's process: {entry point: {"wall_ms": [...], "kernel_ms": [...]}} as one JSON line."""
    import numpy as np
    import sedcost
    import sedgpu
    golden = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(golden, "user_costs.json")) as f:
        user = sedcost.build_plan(json.load(f), ["ACGU"], ["ACGU"])
    with open(os.path.join(golden, "costs.json")) as f:
        iupac = sedcost.build_plan(json.load(f), [IUPAC], [IUPAC])
    rng = np.random.default_rng(2024)
    docs = list(rng.integers(0, 4, size=(a.texts, a.length)).astype(np.uint8))
    short = rng.integers(0, 4, size=28).astype(np.uint8)   # tools/fit_index_ab.py, fit_hits_ab.py, fit_f64_ab.py
    long_ = rng.integers(0, 4, size=76).astype(np.uint8)   # tools/fit_long_ab.py, fit_long_f64_ab.py: their smallest P
    for d in range(0, a.texts, 100):                       # 1 % of the texts hold a copy of each
        docs[d][100:128], docs[d][300:376] = short, long_
    seqs = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(24, 33, size=a.seqs)]
    q_short = sedgpu.PackedPairs([short], [np.zeros(0, np.uint8)])
    q_long = sedgpu.PackedPairs([long_], [np.zeros(0, np.uint8)])
    pairs = sedgpu.PackedPairs([short] * a.texts, docs)
    q_join = sedgpu.PackedPairs(seqs[:64], [np.zeros(0, np.uint8)] * len(seqs[:64]))
    rng_long = np.random.default_rng(a.seqs + 60)          # tools/join_long_ab.py, join_knn_ab.py: 60..90 symbols
    seqs_long = [rng_long.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng_long.integers(60, 91, size=a.seqs)]
    q_join_long = sedgpu.PackedPairs(seqs_long[:64], [np.zeros(0, np.uint8)] * 64)
    ctx = sedgpu.context()
    out = {}

    def measure(name, call, kernel_ms):
        call()  # warm-up; a hits call also learns the room its records need
        wall, kern = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(kernel_ms())
        out[name] = {"wall_ms": wall, "kernel_ms": kern}

    for plan, f64 in ((user, False), (iupac, True)):  # the integer routes under the dyadic table, fp64 under costs.json
        ctx.set_costs(plan)
        sfx = "_f64" if f64 else ""
        ix = sedgpu.FitIndex.from_texts(ctx, docs)
        measure("fit_index_search" + sfx, lambda: getattr(ix, "search" + sfx)(q_short), ix.last_ms)
        measure("fit_index_search_long" + sfx, lambda: getattr(ix, "search_long" + sfx)(q_long), ix.last_ms)
        measure("fit_index_hits" + sfx, lambda: getattr(ix, "hits" + sfx)(q_short, 3.0), ix.hits_last_ms)
        measure("fit_index_hits_long" + sfx, lambda: getattr(ix, "hits_long" + sfx)(q_long, 6.0), ix.hits_last_ms)
        ix.close()
        measure("fit_search" + sfx, lambda: getattr(ctx, "fit" + sfx)(pairs), ctx.fit_last_ms)
        jx = sedgpu.JoinIndex.from_seqs(ctx, seqs)
        measure("join_self" + sfx, lambda: getattr(jx, "self_join" + sfx)(2.0), jx.last_ms)
        measure("join_search" + sfx, lambda: getattr(jx, "search" + sfx)(q_join, 2.0), jx.last_ms)
        measure("join_knn_self" + sfx, lambda: getattr(jx, "self_knn" + sfx)(KNN_K), jx.last_ms)
        if not f64:
            measure("join_knn_search", lambda: jx.search_knn(q_join, KNN_K), jx.last_ms)
        jx.close()
        if not f64:  # (the long index has the integer route alone)
            lx = sedgpu.LongJoinIndex.from_seqs(ctx, seqs_long)
            measure("join_long_self", lambda: lx.self_join(8.0), lx.last_ms)
            measure("join_long_search", lambda: lx.search(q_join_long, 8.0), lx.last_ms)
            measure("join_long_knn_self", lambda: lx.self_knn(KNN_K), lx.last_ms)
            lx.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def stats(xs):
    import numpy as np
    x = np.asarray(xs, float)
    return {"median": round(float(np.median(x)), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=os.path.join(REPO, "tools", "ab_libs", "parent.so"))
    ap.add_argument("--new", default=os.path.join(REPO, "rna-sequence-diff-patch_amd", "libsed.so"))
    ap.add_argument("--base-package", default=None, help="the folder of the base commit's own sedgpu.py, when the base "
                    "library lacks an export this tree's sedgpu.py binds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--texts", type=int, default=8192)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--seqs", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "route_refactor"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    libs = {"base": os.path.abspath(a.base), "new": os.path.abspath(a.new)}
    raw = {k: [] for k in libs}
    for r in range(a.rounds):
        for k, path in libs.items():  # a fresh child per library and round, one at a time
            env = dict(os.environ, SED_LIBRARY=path)
            if k == "base" and a.base_package:
                env["SED_AB_PACKAGE"] = os.path.abspath(a.base_package)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--runs", str(a.runs), "--texts", str(a.texts),
                   "--length", str(a.length), "--seqs", str(a.seqs)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("round %d, %s: the worker ended with status %d" % (r, k, p.returncode))
            raw[k].append(json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
            print("round %d %s done" % (r, k), flush=True)
    res = {"texts": a.texts, "length": a.length, "seqs": a.seqs, "rounds": a.rounds, "runs": a.runs, "entries": {}}
    for name in raw["base"][0]:
        e = {}
        for k in libs:
            wall = [x for proc in raw[k] for x in proc[name]["wall_ms"]]
            e[k] = {"wall_ms": stats(wall), "round_medians": [stats(proc[name]["wall_ms"])["median"] for proc in raw[k]],
                    "kernel_ms": stats([x for proc in raw[k] for x in proc[name]["kernel_ms"]])}
        lo, hi, m = e["base"]["wall_ms"]["min"], e["base"]["wall_ms"]["max"], e["new"]["wall_ms"]["median"]
        e["new_median_vs_base_spread"] = "within" if lo <= m <= hi else "below" if m < lo else "above"
        res["entries"][name] = e
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(readme(res))
    return 0


def readme(r):
    out = ["# Host time per call, one library against another", "",
           "Written by `tools/route_refactor_ab.py`; the raw numbers are in `ab.json`.", "",
           "base = the parent commit's library, new = this tree's; the kernels are the same objects, so only the host code"
           " around them differs.  Each library ran in %d processes of its own, alternating with the other's; every process"
           " built the same seeded inputs, warmed each call up once and timed %d calls of it: wall ms of the whole call"
           " (a host clock around a call that ends in the stream's synchronise).  Spread = the least and the largest of base's"
           " own %d timed calls.  Kernel ms are the engine's HIP events for the same calls." % (r["rounds"], r["runs"], r["rounds"] * r["runs"]),
           "", "Workloads: the fit calls, one query (28 symbols; long: 76) against %d texts of %d nt, the pair calls the same"
           " %d pairs; the join calls, %d sequences of 24..32 symbols at T = 2 (search: 64 query rows), the k-nearest calls"
           " on the same at k = %d, the long index's calls on as many sequences of 60..90 symbols at T = 8 and k = %d.  Integer"
           " routes under `user_costs.json` over ACGU, fp64 routes under `costs.json` over the 15 IUPAC symbols."
           % (r["texts"], r["length"], r["texts"], r["seqs"], KNN_K, KNN_K),
           "", "| entry point | base median ms | base spread (min .. max) | new median ms | new median against base's spread |"
           " base / new round medians | kernel ms base / new |", "|---|---|---|---|---|---|---|"]
    for name, e in r["entries"].items():
        b, n = e["base"], e["new"]
        out.append("| sed_%s | %s | %s .. %s | %s | %s | %s / %s | %s / %s |" % (
            name, b["wall_ms"]["median"], b["wall_ms"]["min"], b["wall_ms"]["max"], n["wall_ms"]["median"],
            e["new_median_vs_base_spread"], b["round_medians"], n["round_medians"], b["kernel_ms"]["median"], n["kernel_ms"]["median"]))
    out += ["", "Not measured: more than one query a call, other text counts and lengths, forced options, more than one GPU.", ""]
    return "\n".join(out)


if __name__ == "__main__":
    sys.exit(main())
