"""CPU: the key-range envelope of tests/key_cases.py, without a device.

a. Route placement.  Every case tests/test_gpu_key_envelope.py runs goes through the planner (sedgpu.plan_routes) and
lands where it claims to: integer mode at `border` and fp64 one symbol past it, at R = 4, 8, 16 and the automatic R;
packed pairs under `lt` tables and none under `eq`; the scaled lane kernel for (15, 127) and not for (16, 127); and the
traceback mode, chains, SPLIT tasks and dot keys the GPU tests assert from the Batch getters.  This is the proof that
the inputs sit on the inequalities of csrc/sed_plan.cpp.

b. Key model.  The lane kernels' recurrences (csrc/sed_lane.hip) and the stripe kernel's ladder keys
(csrc/sed_i32_keys.h) restated in numpy at the kernels' word width, with the same key carried alongside with its
fields 2^32 apart (int64), where no field can reach another.  At every cell of a column <= m the narrow key must be
the wide one packed, every field within its 16 bits: no borrow and no carry across a field.  The decoded (D, L) must be
the C oracle's.  (Rows are a loop; a row's insert chain is a running minimum over its columns, which is what the
kernels' left-to-right min3 computes: the insert candidate is the left cell itself, and clearing the op bits of a
minimum that the left cell lost cannot lift it past the left cell, whose op bits are clear.)"""
import numpy as np
import pytest

import key_cases as kc
import oracle
import sedcost
import sedgpu


def plan_costs(case):
    p = sedcost.build_plan(case.table, [case.alphabet], [case.alphabet])
    return (p.K, np.ascontiguousarray(p.sub, np.float64).ravel(), np.ascontiguousarray(p.sub_int, np.uint8).ravel(),
            float(p.ins), int(p.ins_int), float(p.dele), int(p.del_int))


def planned(case):
    return sedgpu.plan_routes(plan_costs(case), case.opts, sedgpu.PackedPairs(case.A, case.B), case.flags)


# ---- a. route placement ----
def test_tables_are_what_they_claim():
    for name in kc.INT_NAMES:
        sub, ins, dele = kc.costs(name)
        off = sub[~np.eye(4, dtype=bool)]
        assert off.min() == 1 and ins + dele <= 255 and (off == ins + dele - 1).any()
        assert off.max() == (ins + dele if name.endswith("eq") else ins + dele - 1)
        assert kc.packs(name) == name.endswith("lt")
    assert sum(kc.costs(n)[1] + kc.costs(n)[2] == 255 for n in kc.INT_NAMES) == 6
    assert kc.lane_max_n("i1_d127/lt") == 512 and kc.lane_max_n("i1_d254/eq") == 256
    for name, (ins, dele, scale, K, accepted) in kc.SCALED_BASES.items():
        sub = kc.scaled_sub(name) * scale
        assert (sub == np.floor(sub)).all() and sub.max() == ins + dele and sub[0, 1] == 1
        assert (512 * dele + 33 * ins <= 65533) == accepted and (K > 4 or scale > 1)


def test_border_is_the_inequality():
    """`border` against a brute-force scan of `fits`, and the issue's own figures."""
    for name in kc.INT_NAMES + ("user_costs.json",):
        for R in (4, 8, 16):
            for n in (1, 64 * R, 64 * R + 1, 8192, 15360):
                ms = [m for m in range(1, 16400, 1 if (n, R) == (256, 4) else 7) if kc.fits(name, n, m, R)]
                got = kc.border(name, n, R)
                assert (got is None) == (not ms) and (not ms or got[0] - 7 < ms[-1] <= got[0]), (name, R, n)
                assert got is None or (kc.fits(name, n, got[0], R) and not kc.fits(name, n, got[1], R))
    for name in kc.L_TABLES:
        assert kc.border(name, 8192, 16) == (8123, 8124) and kc.border(name, 15360, 16)[0] == 955
        for (n, m), fit in kc.L_FITS.items():
            assert kc.fits(name, n, m, kc.auto_R(n)) == fit, (name, n, m)
    assert kc.costs("i4_d4/eq")[0].max() * 8123 + 4 * (8192 - 8123) == 65260  # the D of the max-distance L-limit pair


def test_every_case_is_planned_where_it_claims():
    seen = set()
    for case in kc.all_cases():
        got = planned(case)
        assert not kc.misses(case.expect, got), (case.label, kc.misses(case.expect, got))
        seen.add((case.label.split()[0], got["mode"]))
    assert seen == {("lane", 1), ("border", 1), ("border", 2), ("L", 1), ("L", 2), ("chain", 1), ("split", 1),
                    ("scaled", 2)}


def test_an_integer_only_r_does_not_fail_the_fp64_fallback():
    """A batch forced to R = 16 whose keys do not fit runs fp64 at that mode's own R, as it does unforced."""
    for case in kc.border_cases("i4_d4/lt", 16, 1025):
        if case.expect["mode"] == kc.F64:
            assert planned(case)["rows_per_lane"] in (2, 4, 8)


# ---- b. key model ----
KB, KB3 = 0xFFFFFFFC, 0xFFFFFE00  # sed_internal.h: SED_KB; sed_i32_keys.h: SED_KB3
LADDER = {4: (4, 0x1230), 8: (8, 0x10123450), 16: (16, 0x1234501230123450)}  # sed_i32_keys.h: Ladder<R>::P, pat


def rung(R, i):
    P, pat = LADDER[R]
    return (pat >> (4 * (i & (P - 1)))) & 0xF


class Format:
    """One key format: the word's bits, its bias, the low field's part of the update addend and of the delete addend
    per row, and the rung and the mask of the bits cleared after the min (0: none)."""

    def __init__(self, bits, bias, upd_lo, del_lo=lambda i: 0, rung=lambda i: 0, clear=0):
        self.bits, self.bias, self.upd_lo, self.del_lo, self.rung, self.clear = bits, bias, upd_lo, del_lo, rung, clear


LANE_DIST = Format(32, KB, lambda i: -1)                              # sed_lane_i32_kernel<false, false>
LANE_LEN = Format(32, KB, lambda i: -2, lambda i: 1, clear=3)         # sed_lane_i32_kernel<true, *>
HALF = Format(16, 0xFFFF, lambda i: 0)                                # sed_lane_i32x2_kernel, one 16-bit half


def ladder_len(R):                                                    # i32_step<R, *, LEN = true>, the perm ladder
    d = lambda i: rung(R, i) - rung(R, i - 1)  # noqa: E731
    return Format(32, KB3, lambda i: d(i) - 6, lambda i: d(i) + 1, lambda i: rung(R, i), 7)


def sweep(fmt, sub, ins, dele, A, B):
    """The recurrence of one format over a batch, row by row: returns every pair's sink word.  Alongside the narrow
    words (uint64 masked to the format's bits, as the kernel's registers hold them) runs the wide key, the same sums
    in int64 with the distance field at bit 32; `same` asserts after every addition and every min that a narrow
    word is its wide key packed, each field within its own 16 bits, on the cells of rows <= n and columns <= m."""
    P, N, M = len(A), max(map(len, A)), max(map(len, B))
    n, m = np.array([len(a) for a in A]), np.array([len(b) for b in B])
    a = np.zeros((P, N), np.int64)
    b = np.zeros((P, M), np.int64)  # (columns past m: whatever follows in memory; nothing flows back from them)
    for p in range(P):
        a[p, :n[p]], b[p, :m[p]] = A[p], B[p]
    mask = (1 << fmt.bits) - 1
    cols = np.arange(M + 1)[None, :] <= m[:, None]
    kappa = (sub - ins - dele).astype(np.int64)  # cost - insert - delete <= 0

    def same(nar, wide, live, what):
        if fmt.bits == 16:
            hi, lo, packed = fmt.bias + wide, np.zeros_like(wide), fmt.bias + wide
        else:
            h = (wide + (1 << 31)) >> 32
            hi, lo = (fmt.bias >> 16) + h, (fmt.bias & 0xFFFF) + (wide - (h << 32))
            packed = (hi << 16) + lo
        ok = (hi >= 0) & (hi <= 0xFFFF) & (lo >= 0) & (lo <= 0xFFFF) & (nar.astype(np.int64) == packed)
        assert ok[live].all(), (what, np.argwhere(~ok & live)[:5])

    nar = np.full((P, M + 1), fmt.bias, np.uint64)
    wide = np.zeros((P, M + 1), np.int64)
    sink_n, sink_w = np.zeros(P, np.uint64), np.zeros(P, np.int64)
    for i in range(1, N + 1):
        live = cols & (i <= n)[:, None]
        k = kappa[a[:, i - 1][:, None], b]  # (P, M): the update's distance part of columns 1..M
        lo, dl, c = fmt.upd_lo(i), fmt.del_lo(i), fmt.rung(i)
        if fmt.bits == 16:  # costrow16's byte under 0xFF: needs cost < insert + delete (x2_costs_ok)
            add_n, add_w = (0xFF00 | (k & 0xFF)).astype(np.uint64), k
        else:  # v_perm: byte 3 0xFF, byte 2 the costrow byte cost - insert - delete - 1, bytes 1:0 the constant
            add_n = ((0xFF << 24) | (((k - 1) & 0xFF) << 16) | (lo & 0xFFFF)).astype(np.uint64)
            add_w = (k << 32) + lo
        dg_n, dg_w = (nar[:, :-1] + add_n) & mask, wide[:, :-1] + add_w
        up_n, up_w = (nar[:, 1:] + np.uint64(dl)) & mask, wide[:, 1:] + dl
        same(dg_n, dg_w, live[:, 1:], "update candidate, row %d" % i)
        same(up_n, up_w, live[:, 1:], "delete candidate, row %d" % i)
        mm_n, mm_w = np.minimum(up_n, dg_n), np.minimum(up_w, dg_w)
        if fmt.clear:
            mm_n, mm_w = (mm_n & np.uint64(mask & ~fmt.clear)) | np.uint64(c), (mm_w & ~fmt.clear) | c
        nar = np.minimum.accumulate(np.concatenate([np.full((P, 1), fmt.bias + c, np.uint64), mm_n], 1), 1)
        wide = np.minimum.accumulate(np.concatenate([np.full((P, 1), c, np.int64), mm_w], 1), 1)
        same(nar, wide, live, "cell, row %d" % i)
        done = np.flatnonzero(n == i)
        sink_n[done], sink_w[done] = nar[done, m[done]], wide[done, m[done]]
    return [int(x) for x in sink_n]


M32 = 0xFFFFFFFF


def decode_dist(w, n, m, ins, dele):   # sed_lane_i32_kernel, !LEN
    return ((w - KB + ((n * dele + m * ins) << 16) + 0xFFFF) & M32) >> 16, None


def decode_len(w, n, m, ins, dele):    # sed_lane_i32_kernel, LEN: kins = (insert << 16) + 4, kdel - 1 = (delete << 16) + 4
    v = (w - KB + n * ((dele << 16) + 4) + m * ((ins << 16) + 4)) & M32
    return v >> 16, (v >> 2) & 0x3FFF


def decode_half(w, n, m, ins, dele):   # sed_lane_i32x2_kernel
    return (w + 1 + n * dele + m * ins) & 0xFFFF, None


def decode_ladder(R):                  # i32_decode<R, LEN = true>: L inside the window [max(n, m), n + m]
    def decode(w, n, m, ins, dele):
        v = (w - KB3 - rung(R, n) + n * ((dele << 16) + 8) + m * ((ins << 16) + 8)) & M32
        lo = max(n, m)
        L = lo + ((((v >> 3) & 0x1FFF) - lo) & 0x1FFF)
        return ((v - 8 * L) & M32) >> 16, L
    return decode


def model_check(name, fmt, decode, A, B):
    sub, ins, dele = kc.costs(name)
    ins, dele = int(ins), int(dele)
    sinks = sweep(fmt, sub, ins, dele, A, B)
    plan = sedcost.build_plan(kc.TABLES[name], [kc.S], [kc.S])
    cs = oracle.Costs.from_plan(plan)
    for w, a, b in zip(sinks, A, B):
        D, L = decode(w, len(a), len(b), ins, dele)
        o = oracle.pair(cs, a, b, want_ops=False)
        assert D == o["dist"] and (L is None or L == o["len"]), (name, len(a), len(b), D, L, o)


@pytest.mark.parametrize("name", kc.INT_NAMES)
def test_lane_key_models(name):
    """The lane block under the distance keys, the length keys and (`lt` tables) the 16-bit halves."""
    A, B = kc.lane_block(name)
    model_check(name, LANE_DIST, decode_dist, A, B)
    model_check(name, LANE_LEN, decode_len, A, B)
    if kc.packs(name):
        model_check(name, HALF, decode_half, A, B)


@pytest.mark.parametrize("R", [4, 8, 16])
def test_stripe_ladder_key_model(R):
    """The stripe kernel's ladder keys on single-stripe pairs under every table that has one at R: the small CHAIN
    shapes (n in {1, 17, 64 R}, m in {1, 33, 65}, max-distance and mutated), and the max-distance pair of 64 R rows at
    the last m that fits."""
    ran = 0
    for name in kc.INT_NAMES:
        if kc.border(name, 64 * R, R) is None:
            continue
        sub = kc.costs(name)[0]
        rng = np.random.default_rng(kc.seed("ladder", name, R))
        A, B = [], []
        for n in (1, 17, 64 * R):
            for m in (1, 33, 65):
                a, b = kc.pairs(sub, rng, n, m, kinds=("max", "mutated"))
                A, B = A + a, B + b
        model_check(name, ladder_len(R), decode_ladder(R), A, B)
        a, b = kc.max_pair(sub, 64 * R, kc.border(name, 64 * R, R)[0])
        model_check(name, ladder_len(R), decode_ladder(R), [a], [b])
        ran += 1
    assert ran == {4: 10, 8: 6, 16: 4}[R]
