"""bench.py's --dump-outputs and --full.  CPU: the dump's arrays, types, byte budget and seeded sample.  GPU: one
small plain run with --dump-outputs, its result line, and the dumped results against the C oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_whole(tmp_path):
    d = str(tmp_path / "out")
    dist = np.array([3.0, 2.5, 0.0])
    ln = np.array([7, 5, -1], np.int32)
    ops = np.array([0xFFFFFFFF, 0, 0x9E3779B9, 1], np.uint32)
    assert bench.dump_outputs(d, dist, ln, ops) == {"dist": 3, "len": 3, "ops": 4}
    assert sorted(os.listdir(d)) == ["dist.npy", "len.npy", "ops.npy"]
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in ("dist", "len", "ops")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["dist"], dist) and np.array_equal(got["len"], ln)
    assert np.array_equal(got["ops"].astype(np.uint32), ops)  # every 32-bit word is exact in a double
    d2 = str(tmp_path / "dist_only")
    assert bench.dump_outputs(d2, dist, ln, None) == {"dist": 3, "len": 3}
    assert sorted(os.listdir(d2)) == ["dist.npy", "len.npy"]


def test_dump_outputs_budget_and_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 16)  # the same code path as 64 MB, at a size a test can write
    dist = np.arange(100, dtype=np.float64)
    ln = np.arange(100, dtype=np.int32)
    ops = (np.arange(50000, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    na = bench.dump_outputs(a, dist, ln, ops)
    bench.dump_outputs(b, dist, ln, ops)
    assert _dir_bytes(a) <= 1 << 16
    assert (1 << 16) // 8 // 2 < na["ops"] < len(ops)  # a sample, and most of the budget used
    sa, sb = np.load(os.path.join(a, "ops.npy")), np.load(os.path.join(b, "ops.npy"))
    assert np.array_equal(sa, sb)  # the same word indices in every run
    room = ((1 << 16) - 2 * 100 * 8) // 8 - 64  # the budget less dist and len, in words, less the file headers
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, len(ops), size=room))
    assert np.array_equal(sa.astype(np.uint32), ops[idx])
    # one word changed in the source shows in the sample if it was drawn
    ops2 = ops.copy()
    ops2[idx[5]] ^= 1
    bench.dump_outputs(b, dist, ln, ops2)
    assert not np.array_equal(np.load(os.path.join(b, "ops.npy")), sa)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_results(tmp_path):
    import oracle
    import sedcost
    import sedgpu
    P, n, m, steps = 40, 150, 131, 3
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--pairs", str(P), "--shape", "%dx%d" % (n, m), "--dump-outputs", d],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["full"] is False and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(P * n * m / (line["ms_per_step"] * 1e-3))
    assert line["unit"] == "cells/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    # nothing that takes work of its own
    assert line["cpu_baseline"] is None and line["issue"] is None and line["roofline"]["traffic"] is None
    assert "script_valid_rate" not in line and "script_exact_rate" not in line
    # the dumped arrays are the results of these inputs: every pair against the C oracle
    with open(os.path.join(GOLDEN, "user_costs.json")) as f:
        plan = sedcost.build_plan(json.load(f), ["ACGU"], ["ACGU"])
    A, B, _, _ = bench.shard_inputs("c4", P, n, m, 1, 0)
    packed = sedgpu.PackedPairs.from_arrays(A, B)
    cs = oracle.Costs.from_plan(plan)
    dist, ln, ops = (np.load(os.path.join(d, x + ".npy")) for x in ("dist", "len", "ops"))
    assert dist.shape == (P,) and ln.shape == (P,) and ops.shape == (int(packed.ops_off[P]),)
    words = ops.astype(np.uint32)
    for p in range(P):
        o = oracle.pair(cs, A[p], B[p])
        assert dist[p] == o["dist"] and ln[p] == o["len"], p
        assert np.array_equal(sedgpu.unpack_ops(words, packed.ops_off, p, int(ln[p])), o["ops"]), p
