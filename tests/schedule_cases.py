"""Small batches, one per shape of a run's schedule (csrc/sed_plan.cpp: sed_plan_run), for the CPU test that reads the
schedule (test_plan_schedule.py) and the GPU test that runs it (test_gpu_schedule.py).  Each is the smallest fill for
which the planner takes the route: the CPU test asserts that through sedgpu.plan_routes / plan_schedule."""
import numpy as np

import plan_route_cases as pc
import sedgpu

O = sedgpu
SCRIPT, PIPELINE, NO_LEN = pc.SCRIPT, pc.PIPELINE, pc.NO_LEN
# one wave per pair on the plain stripe kernel (tests/test_gpu_cutoff.py: STRIPE)
STRIPE = {O.SED_OPT_CHAIN: 2, O.SED_OPT_SPLIT: 2, O.SED_OPT_PACK: 2}


def _related(seed, count, n, m=None):
    """count pairs: str2 = str1 resized to m with 10 % point mutations."""
    rng = np.random.default_rng(seed)
    A = [rng.integers(0, 4, size=n).astype(np.uint8) for _ in range(count)]
    B = [np.where(rng.random(m or n) < 0.1, rng.integers(0, 4, size=m or n), np.resize(a, m or n)).astype(np.uint8)
         for a in A]
    return A, B


def _two_parts():
    """2048 wave pairs (the fewest two parts take: 1024 each) of 65..130 x 65..130, so stripes of one and two chunks,
    and 24 pairs of 40 x 28 on the lane kernel, which runs inside part 0's DP window."""
    A, B = pc._pairs(21, 2048, 65, 130, 65, 130)
    la, lb = _related(22, 24, 40, 28)
    return A + la, B + lb


def _windowed():
    """Six 10 % mutated 768 x 768 pairs (two stripes at R = 8) and 12 pairs of 40 x 28 on the lane kernel: 18 pairs, past
    the 16 below which short pairs stay on the wave kernels."""
    A, B = _related(23, 6, 768)
    la, lb = _related(24, 12, 40, 28)
    return A + la, B + lb


# name: (costs, options, flags, pairs, the cutoff's quantile of the batch's distances or None)
SHAPES = {
    # checkpoint traceback in one part: forward, traceback
    "one_part_script": (lambda: pc._costs(True, "ACGU"), {O.SED_OPT_TB: 2, **STRIPE}, SCRIPT,
                        lambda: pc._pairs(20, 12, 100, 300, 100, 300), None),
    "two_parts": (lambda: pc._costs(True, "ACGU"), {O.SED_OPT_TB: 2, **STRIPE}, SCRIPT, _two_parts, None),
    # SPLIT with checkpoints: forward, tile codes, stripe-parallel walk
    "split_ck": (lambda: pc._costs(False, "ACGU"), {O.SED_OPT_SPLIT: 1}, SCRIPT,
                 lambda: pc._pairs(25, 2, 500, 700, 500, 700), None),
    # three rotating buffers, the traceback on its own stream
    "pipelined_codes": (lambda: pc._costs(True, "ACGU"), dict(STRIPE), SCRIPT | PIPELINE,
                        lambda: pc._pairs(26, 80, 100, 300, 100, 300), None),
    "lane_only": (lambda: pc._costs(False, "ACGU"), {}, NO_LEN, lambda: pc._pairs(27, 200, 24, 32, 24, 32), None),
    "cut_filter": (lambda: pc._costs(False, "ACGU"), {}, NO_LEN, lambda: pc._pairs(27, 200, 24, 32, 24, 32), 0.5),
    "cut_windowed": (lambda: pc._costs(True, "ACGU"), {O.SED_OPT_ROWS_PER_LANE: 8, **STRIPE}, NO_LEN, _windowed, 0.85),
    # fp64: 300 pairs the cost model runs in 16-lane segments and 6 it keeps on whole waves (256 rows are one stripe
    # of a wave at R = 4 and four of a segment, which pays only below ~945 columns: sed_plan.cpp, f64_cost)
    "f64_segments": (lambda: pc._costs(False, pc.IUPAC), {}, SCRIPT,
                     lambda: tuple(x + y for x, y in zip(pc._pairs(28, 300, 10, 120, 10, 120, K=15),
                                                         pc._pairs(29, 6, 256, 256, 1000, 1100, K=15))), None),
}
NAMES = tuple(SHAPES)


class Shape:
    def __init__(self, name):
        costs, opts, flags, pairs, cut = SHAPES[name]
        self.name, self.costs, self.options, self.flags, self.cut = name, costs(), dict(opts), flags, cut
        A, B = pairs()
        self.packed = sedgpu.PackedPairs(list(A), list(B))
