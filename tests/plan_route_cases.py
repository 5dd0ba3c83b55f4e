"""The fills behind tests/golden/plan_routes.json: small batches, one per route the planner can pick (csrc/sed_plan.cpp).
Each case is the raw input of a fill (cost table, options, environment knobs, flags, pairs), built from seeds, so the
CPU test (test_plan_routes.py), the GPU consistency test (test_gpu_routes.py) and whoever records the golden numbers
from a library's getters all see the same bytes."""
import json
import os

import numpy as np

import sedcost
import sedgpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IUPAC = "AGCUYRWSKMDVHBN"
SCRIPT, PIPELINE, NO_LEN = sedgpu.SED_WANT_SCRIPT, sedgpu.SED_PIPELINE, sedgpu.SED_NO_LEN
# sed_plan_routes' output order (include/sed.h)
FIELDS = ("mode", "rows_per_lane", "lane_pairs", "chains", "traceback_mode", "dot_keys", "bitpar_pairs",
          "segment_pairs", "split_tasks", "scaled_pairs", "packed_pairs", "dp_launches", "band_cells", "cells",
          "algo_bytes")


def _table(user):
    with open(os.path.join(GOLDEN, "user_costs.json" if user else "costs.json")) as f:
        return json.load(f)


def _costs(user, alphabet):
    p = sedcost.build_plan(_table(user), [alphabet], [alphabet])
    return (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
            float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))


def _wide_costs(K):
    """K symbols at fractional costs: no integer table, so fp64 whatever the size."""
    sub = np.full((K, K), 0.7)
    np.fill_diagonal(sub, 0.0)
    return K, sub.ravel(), np.zeros(K * K, np.uint8), 0.9, 0, 0.8, 0


def _pairs(seed, count, nlo, nhi, mlo, mhi, K=4, related=0.5):
    """count pairs of codes < K, lengths uniform in [nlo, nhi] x [mlo, mhi]; `related` of them are str1 resized with
    12 % point mutations (so band pruning has something to prune)."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    for _ in range(count):
        n, m = int(rng.integers(nlo, nhi + 1)), int(rng.integers(mlo, mhi + 1))
        a = rng.integers(0, K, size=n).astype(np.uint8)
        if n and rng.random() < related:
            b = np.where(rng.random(m) < 0.12, rng.integers(0, K, size=m), np.resize(a, m)).astype(np.uint8)
        else:
            b = rng.integers(0, K, size=m).astype(np.uint8)
        A.append(a)
        B.append(b)
    return A, B


def _with_n(seed, count):
    """~28-nt ACGUN pairs, N at 1 %: most pairs lie inside the unit-cost subset ACGU."""
    rng = np.random.default_rng(seed)
    seq = lambda: rng.choice(5, p=[0.2475] * 4 + [0.01], size=int(rng.integers(24, 33))).astype(np.uint8)
    return [seq() for _ in range(count)], [seq() for _ in range(count)]


def _empty_sides():
    A, B = _pairs(77, 6, 1, 300, 1, 300)
    z = np.zeros(0, np.uint8)
    return A + [z, A[0], z], B + [B[1], z, z]


O = sedgpu
# name: (costs, {option: value}, {environment knob: value}, flags, pairs)
_CASES = {
    "split_script_4096": (lambda: _costs(False, "ACGU"), {}, {}, SCRIPT, lambda: _pairs(1, 1, 4096, 4096, 4096, 4096)),
    "split_dist_4096": (lambda: _costs(False, "ACGU"), {}, {}, 0, lambda: _pairs(1, 1, 4096, 4096, 4096, 4096)),
    "ck_2048": (lambda: _costs(True, "ACGU"), {}, {}, SCRIPT, lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "ck_2048_band_off": (lambda: _costs(True, "ACGU"), {O.SED_OPT_BAND: 2}, {}, SCRIPT,
                         lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "ck_2048_dot_off": (lambda: _costs(True, "ACGU"), {O.SED_OPT_DOT: 2}, {}, SCRIPT,
                        lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "ck_2048_codes": (lambda: _costs(True, "ACGU"), {O.SED_OPT_TB: 1}, {}, SCRIPT,
                      lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "chain_dynamic": (lambda: _costs(False, "ACGU"), {}, {}, SCRIPT, lambda: _pairs(3, 12000, 200, 200, 200, 200)),
    "chain_dynamic_capped": (lambda: _costs(False, "ACGU"), {O.SED_OPT_CHAIN_WAVES: 300}, {}, SCRIPT,
                             lambda: _pairs(3, 12000, 200, 200, 200, 200)),
    "chain_static": (lambda: _costs(True, "ACGU"), {O.SED_OPT_CHAIN: 3}, {}, SCRIPT,
                     lambda: _pairs(4, 400, 1, 256, 33, 500)),
    "lane_bitpar": (lambda: _costs(False, "ACGU"), {}, {}, NO_LEN, lambda: _pairs(5, 1000, 24, 32, 24, 32)),
    "lane_x2": (lambda: _costs(True, "ACGU"), {}, {}, NO_LEN, lambda: _pairs(5, 1000, 24, 32, 24, 32)),
    "lane_scaled": (lambda: _costs(False, "ACGUN"), {}, {}, NO_LEN, lambda: _with_n(6, 1000)),
    "lane_pipelined": (lambda: _costs(False, "ACGU"), {}, {}, NO_LEN | PIPELINE,
                       lambda: _pairs(5, 1000, 24, 32, 24, 32)),
    "wave_x2": (lambda: _costs(True, "ACGU"), {}, {}, NO_LEN, lambda: _pairs(7, 300, 300, 300, 100, 250)),
    "f64_segments": (lambda: _costs(False, IUPAC), {}, {}, SCRIPT, lambda: _pairs(8, 300, 10, 500, 10, 500, K=15)),
    "f64_split": (lambda: _costs(False, IUPAC), {}, {}, SCRIPT, lambda: _pairs(8, 4, 10, 500, 10, 500, K=15)),
    "i32_overflow": (lambda: _costs(True, "ACGU"), {}, {}, 0, lambda: _pairs(9, 1, 14000, 14000, 14000, 14000)),
    "i32_overflow_forced": (lambda: _costs(True, "ACGU"), {O.SED_OPT_MODE: 1}, {}, 0,
                            lambda: _pairs(9, 1, 14000, 14000, 14000, 14000)),
    "wide_alphabet": (lambda: _wide_costs(40), {}, {}, 0, lambda: _pairs(10, 8, 1, 100, 1, 100, K=40)),
    "no_pairs": (lambda: _costs(True, "ACGU"), {}, {}, SCRIPT, lambda: ([], [])),
    "empty_sides": (lambda: _costs(True, "ACGU"), {}, {}, SCRIPT, _empty_sides),
    "negative_length": (lambda: _costs(True, "ACGU"), {}, {}, SCRIPT, _empty_sides),  # (Case: len_b[3] = -1)
    "bad_code": (lambda: _costs(True, "ACGU"), {}, {}, SCRIPT, _empty_sides),  # (Case: one code 4 in pair 2)
    # the environment knobs (sed_opts; the runtime reads them once per process)
    "env_tbpar_off": (lambda: _costs(False, "ACGU"), {}, {"SED_TBPAR": 0}, SCRIPT,
                      lambda: _pairs(1, 1, 4096, 4096, 4096, 4096)),
    "env_tbpar_on": (lambda: _costs(True, "ACGU"), {O.SED_OPT_SPLIT: 2, O.SED_OPT_ROWS_PER_LANE: 4}, {"SED_TBPAR": 1},
                     SCRIPT, lambda: _pairs(11, 100, 100, 900, 100, 900)),
    "env_band_off": (lambda: _costs(True, "ACGU"), {}, {"SED_BAND": 0}, SCRIPT,
                     lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "env_ck_one_part": (lambda: _costs(True, "ACGU"), {}, {"SED_CK_HALVES": 1}, SCRIPT,
                        lambda: _pairs(2, 2048, 1100, 1100, 1100, 1100)),
    "env_ck_four_parts": (lambda: _costs(True, "ACGU"), {O.SED_OPT_TB: 2}, {"SED_CK_HALVES": 4}, SCRIPT,
                          lambda: _pairs(12, 4200, 100, 300, 100, 300)),
    "env_alt_dp_off": (lambda: _costs(False, "ACGU"), {}, {"SED_ALT_DP": 0}, NO_LEN | PIPELINE,
                       lambda: _pairs(5, 1000, 24, 32, 24, 32)),
}
NAMES = tuple(_CASES)
# the fills the GPU consistency test repeats against a real batch's getters: one per family of routes
GPU_NAMES = ("split_script_4096", "ck_2048", "chain_dynamic_capped", "chain_static", "lane_scaled", "wave_x2",
             "f64_segments", "f64_split", "empty_sides")


class Case:
    def __init__(self, name):
        costs, opts, knobs, flags, pairs = _CASES[name]
        self.name, self.costs, self.options, self.knobs, self.flags = name, costs(), dict(opts), dict(knobs), flags
        A, B = pairs()
        self.packed = sedgpu.PackedPairs(A, B)
        if name == "negative_length":
            self.packed.len_b[3] = -1
        if name == "bad_code":
            self.packed.codes_a[self.packed.off_a[2]] = 4

    def arrays(self):
        p = self.packed
        return p.codes_a, p.off_a, p.len_a, p.codes_b, p.off_b, p.len_b, p.npairs
