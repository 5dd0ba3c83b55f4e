"""GPU: one small batch per shape of a run's schedule (tests/schedule_cases.py; csrc/sed_plan.cpp: sed_plan_run) runs
twice.  The second run's events must all have been recorded (last_times reads the four of every part: an event no launch
carried fails it) and its results equal the C oracle's.  That each batch plans the shape it is named for is
tests/test_plan_schedule.py's business, on the CPU."""
import os

import numpy as np
import pytest

from conftest import padding_errors
import oracle
import schedule_cases as sc
import sedgpu

pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
INF = float("inf")


@pytest.mark.parametrize("name", sc.NAMES)
def test_two_runs_are_timed_and_match_the_oracle(gpu, name):
    shape = sc.Shape(name)
    K, sub, sub_int, ins, ins_int, dele, del_int = shape.costs
    p, P = shape.packed, shape.packed.npairs
    script = bool(shape.flags & sedgpu.SED_WANT_SCRIPT)
    no_len = bool(shape.flags & sedgpu.SED_NO_LEN)
    cs = oracle.Costs(np.reshape(sub, (K, K)), np.reshape(sub_int, (K, K)), ins, ins_int, dele, del_int)
    od, oi, ol, oops, ooff = oracle.batch(cs, p.codes_a, p.off_a, p.len_a, p.codes_b, p.off_b, p.len_b, P,
                                          want_ops=script, nthreads=THREADS)
    cut = INF if shape.cut is None else float(np.quantile(od, shape.cut))
    want = sedgpu.plan_schedule(shape.costs, shape.options, p, shape.flags, shape.cut is not None, name == "cut_windowed")
    gpu.invalidate_costs()  # (set below past the Context's cache)
    assert gpu._lib.sed_set_costs(gpu.ptr, K, sub, sub_int, ins, ins_int, dele, del_int) == 0
    for k, v in shape.options.items():
        gpu.set_option(k, v)
    try:
        b = sedgpu.Batch(gpu, p, script, pipeline=bool(shape.flags & sedgpu.SED_PIPELINE), no_len=no_len)
        try:
            if shape.cut is not None:
                b.set_cutoff(cut)
                # (the windowed kernel took the wave pairs exactly when the planned schedule says so)
                assert (b.band_cells < b.work()[0]) == (want[0].launcher == "win")
            assert b.dp_launches == want.parts
            b.run()
            b.run()
            d, ii, ln, ops = b.results()
            dp_ms, tb_ms = b.last_times()
        finally:
            b.close()
    finally:
        for k in shape.options:
            gpu.set_option(k, 0)
        gpu.invalidate_costs()
    print("%s: dp %.4f ms, traceback %.4f ms" % (name, dp_ms, tb_ms))
    assert np.isfinite(dp_ms) and np.isfinite(tb_ms) and dp_ms >= 0 and tb_ms >= 0
    within = od <= cut
    assert 0 < within.sum() and (shape.cut is None) == bool(within.all())
    assert np.array_equal(d[within], od[within]), np.flatnonzero(within & (d != od))[:10]
    assert np.array_equal(ii[within].astype(bool), oi[within].astype(bool))
    assert np.all(d[~within] == INF) and not ii[~within].any() and np.all(ln[~within] == -1)
    if no_len:
        assert np.all((ln == -1) | (ln == ol))
    else:
        assert np.array_equal(ln, ol), np.flatnonzero(ln != ol)[:10]
    if script:
        bad = [q for q in range(P)
               if not np.array_equal(sedgpu.unpack_ops(ops, p.ops_off, q, int(ln[q])), oops[ooff[q]:ooff[q] + ol[q]])]
        assert not bad, bad[:10]
        assert not padding_errors(ops, p.ops_off, p.len_a, p.len_b, ln)
