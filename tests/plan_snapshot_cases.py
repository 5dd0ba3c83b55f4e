"""The cases behind tests/golden/plan_snapshot.json: every device-free fit and join export of sedgpu over small fixed
arguments, served and refused, with what each call returns (plan fields, rows, lane records, params, the route and its
`why` text) or the SedError code it raises.  tools/plan_snapshot.py records them, tests/test_plan_snapshot.py recomputes
them; both go through snapshot() below, so the file and the test cannot disagree about a case.

A fit case runs every export of its form on the same arguments: a refusal therefore shows on each route that has it,
and a route that lacks it shows what it answers instead.  The route functions carry the refusal texts (a SedError
carries the code alone), the integer route's first: where two refusals apply to one call, the text names the one that
wins, which is how the order between them is pinned."""
import json
import math
import os

import numpy as np

import sedcost
import sedgpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK, ROWS = sedgpu.SED_OPT_FIT_CHUNK, sedgpu.SED_OPT_FIT_ROWS
JOIN_DP, JOIN_ROWS = sedgpu.SED_OPT_JOIN_DP, sedgpu.SED_OPT_JOIN_ROWS

PAIR_CALLS = ("fit_plan", "fit_lanes", "fit_f64_plan", "fit_f64_lanes", "fit_route")
INDEX_CALLS = ("fit_index_plan", "fit_index_lanes", "fit_index_f64_plan", "fit_index_f64_lanes", "fit_index_long_plan",
               "fit_index_long_lanes", "fit_index_long_f64_plan", "fit_index_long_f64_lanes", "fit_long_route")
JOIN_CALLS = ("join_plan", "join_f64_plan", "join_route")


def unit(K, ins=1.0, dele=1.0, sub=1.0, cell=None):
    """sed_set_costs' arguments of a table with `sub` off a zero diagonal; cell = ((a, b), cost) overrides one entry."""
    t = np.where(np.eye(K) > 0, 0.0, float(sub))
    if cell:
        t[cell[0]] = cell[1]
    return (K, t, np.eye(K, dtype=np.uint8), float(ins), 0, float(dele), 0)


def user(alphabet="ACGU"):
    with open(os.path.join(GOLDEN, "user_costs.json")) as f:
        p = sedcost.build_plan(json.load(f), [alphabet], [alphabet])
    return (p.K, p.sub, p.sub_int, p.ins, p.ins_int, p.dele, p.del_int)


def fit_tables():
    return {"unit": unit(4),                         # S = 1, W = 2 P
            "user": user(),                          # insert 2, delete 3: W = P + floor(3 P / 2)
            "s256": unit(4, 0.25, 0.5, 1.0 / 256),   # needs S = 2^8: W = 3 P
            "third": unit(4, cell=((0, 1), 1.0 / 3)),  # no multiple of 2^-8: the fp64 routes alone
            "k16": unit(16)}                         # 16 symbols: the fp64 routes alone


def fit_cases():
    """[(name, form, costs, options, len_p, len_t, max_dist or None)]; form "pair" runs PAIR_CALLS (and
    fit_cutoff_scaled when max_dist is given), "index" runs INDEX_CALLS."""
    out = []
    add = lambda name, form, costs, options, lp, lt, md=None: out.append((name, form, costs, options, lp, lt, md))
    T = fit_tables()
    # served: every table without options; a chunk below W and a multiple of 4 above it
    for tn, costs in T.items():
        add("pair_%s" % tn, "pair", costs, {}, [7, 32, 1, 12], [0, 5, 70, 150], 1.5)
        add("index_%s" % tn, "index", costs, {}, [7, 32, 1], [0, 5, 70, 150])
    for tn in ("unit", "user", "k16"):
        for c in (16, 100):
            add("pair_%s_chunk%d" % (tn, c), "pair", T[tn], {CHUNK: c}, [7, 32, 1, 12], [0, 5, 70, 150], 0.25)
            add("index_%s_chunk%d" % (tn, c), "index", T[tn], {CHUNK: c}, [7, 32], [0, 5, 70, 150])
    # the long routes: P = 33, 129, 2048, with the rows option at 2 and at a value too small for a query
    for tn in ("unit", "user", "third"):
        add("long33_%s" % tn, "index", T[tn], {}, [33, 5], [0, 150, 300])
        add("long33_%s_chunk16" % tn, "index", T[tn], {CHUNK: 16}, [33], [0, 150, 300])
        add("long33_%s_chunk200" % tn, "index", T[tn], {CHUNK: 200}, [33], [0, 150, 300])
    add("long129_unit", "index", T["unit"], {}, [129, 128], [0, 150, 300])
    add("long129_unit_rows2", "index", T["unit"], {ROWS: 2}, [128, 129], [150])   # 129 > 64 * 2
    add("long128_unit_rows2", "index", T["unit"], {ROWS: 2}, [128, 5], [150, 300])
    add("long33_k16_rows2", "index", T["k16"], {ROWS: 2}, [33], [150])
    add("long33_unit_rows32_chunk16", "index", T["unit"], {ROWS: 32, CHUNK: 16}, [33], [150])
    add("long2048_unit", "index", T["unit"], {}, [2048], [0, 150, 300])
    add("long2048_user_chunk16", "index", T["user"], {CHUNK: 16}, [2048], [300])
    add("long2048_k16_chunk5000", "index", T["k16"], {CHUNK: 5000}, [2048, 40], [300])
    add("pair_unit_cut_all", "pair", T["unit"], {}, [5], [10], math.inf)
    add("pair_s256_cut", "pair", T["s256"], {}, [5], [10], 255.999)
    add("pair_unit_cut_nan", "pair", T["unit"], {}, [5], [10], math.nan)
    add("pair_unit_cut_negative", "pair", T["unit"], {}, [5], [10], -0.5)
    # K = 9 and K = 17 against a pattern of length 0 and of length pmax + 1: which refusal comes first
    for K in (9, 17):
        add("pair_k%d" % K, "pair", unit(K), {}, [5], [10], 1.0)
        add("index_k%d" % K, "index", unit(K), {}, [5, 40], [10])
        for P in (0, 33):
            add("pair_k%d_p%d" % (K, P), "pair", unit(K), {}, [5, P], [10, 10])
        for P in (0, 33, 2049):
            add("index_k%d_p%d" % (K, P), "index", unit(K), {}, [5, P], [10])
    for P in (0, 33):
        add("pair_unit_p%d" % P, "pair", T["unit"], {}, [P], [10])
    for P in (0, 33, 2049):
        add("index_unit_p%d" % P, "index", T["unit"], {}, [5, P], [10])
    # a negative text length at index 0 and at index 1, with 1 query and with 2, and against a bad pattern
    for lt in ([-1, 5], [5, -1]):
        tag = "neg%d" % lt.index(-1)
        add("pair_%s" % tag, "pair", T["unit"], {}, [5, 6], lt)
        add("pair_%s_p0" % tag, "pair", T["unit"], {}, [0, 33], lt)
        add("index_%s_q1" % tag, "index", T["unit"], {}, [5], lt)
        add("index_%s_q2" % tag, "index", T["unit"], {}, [5, 6], lt)
        add("index_%s_q2_p0_first" % tag, "index", T["unit"], {}, [0, 5], lt)
        add("index_%s_q2_p0_second" % tag, "index", T["unit"], {}, [5, 0], lt)
        add("index_%s_k17" % tag, "index", unit(17), {}, [5, 6], lt)
    # the integer envelope
    add("pair_insert0", "pair", unit(4, 0.0, 1.0), {CHUNK: 16}, [5, 32], [10, 300], 2.0)
    add("index_insert0", "index", unit(4, 0.0, 1.0), {CHUNK: 16}, [5, 32], [10, 300])
    add("pair_p_delete", "pair", unit(4, 1.0, 3000.0), {}, [32], [10])            # 32 * 3000 > 65535
    add("pair_p_delete_s4", "pair", unit(4, 1.0, 2100.25), {}, [32], [10])        # S = 4: 32 * 8401 > 65535
    add("index_p_delete", "index", unit(4, 1.0, 3000.0), {}, [32], [10])
    add("index_long_d_field", "index", unit(4, 16.0, 31.0), {}, [2048], [100])   # 2048 * 31 + 128 * 16 = 65536
    add("index_long_d_field_fits", "index", unit(4, 16.0, 31.0), {}, [2047], [100])
    add("pair_delete_byte", "pair", unit(4, 1.0, 300.0), {}, [5], [10])           # delete * S > 255
    add("pair_addend_byte", "pair", unit(4, 100.0, 200.0), {}, [5], [10])         # (insert + delete) * S > 255
    add("index_addend_byte", "index", unit(4, 100.0, 200.0), {}, [5], [10])
    add("index_addend_byte_p40", "index", unit(4, 100.0, 200.0), {}, [5, 40], [10])  # (the short routes: the length first)
    # the span of a lane's 16-bit start field: 65535 columns and more, without a chunk and under one that fails
    for n in (65534, 65535):
        add("pair_insert0_n%d" % n, "pair", unit(4, 0.0, 1.0), {}, [5, 5], [10, n])
        add("index_insert0_n%d" % n, "index", unit(4, 0.0, 1.0), {}, [5, 32], [10, n])
    wide = unit(4, 1.0, 200.0)  # W = 201 P: few lanes over a long text
    add("pair_span_auto", "pair", wide, {}, [32, 3], [70000, 9])
    add("index_span_auto", "index", wide, {}, [32], [9, 70000])
    add("index_span_clamped", "index", unit(4, 1.0, 250.0), {}, [200], [70000])   # W = 50200: chunk = 65535 - W - 3
    add("pair_span_chunk_ok", "pair", T["unit"], {CHUNK: 40000}, [32], [70000])
    add("index_span_chunk_ok", "index", T["unit"], {CHUNK: 40000}, [32, 5], [70000])
    add("pair_span_chunk_fails", "pair", T["unit"], {CHUNK: 65535}, [32, 5], [9, 70000])
    add("index_span_chunk_fails", "index", T["unit"], {CHUNK: 65535}, [32, 5], [9, 70000])
    add("index_span_chunk_edge", "index", T["unit"], {CHUNK: 65468}, [32], [70000])  # 65468 + 64 + 3 = 65535
    # costs the fp64 routes refuse, and ones no route takes as arguments
    add("pair_insert_negative", "pair", unit(4, -1.0, 1.0), {}, [5], [10])
    add("index_delete_negative", "index", unit(4, 1.0, -2.0), {}, [5, 32], [10])
    add("pair_cell_negative", "pair", unit(4, cell=((1, 2), -0.5)), {}, [5], [10])
    add("index_cell_negative", "index", unit(4, cell=((1, 2), -0.5)), {}, [5, 32], [10])
    add("pair_insert_nan", "pair", unit(4, math.nan, 1.0), {}, [5], [10])
    add("index_delete_inf", "index", unit(4, 1.0, math.inf), {}, [5], [10])
    add("pair_cell_inf", "pair", unit(4, cell=((3, 0), math.inf)), {}, [5], [10])
    add("index_cell_nan", "index", unit(4, cell=((3, 0), math.nan)), {}, [5], [10])
    # one_lane: chunked, insert = 0 (above), and no window (a cost below 2^-900; P delete / insert above 2^20)
    add("pair_no_window_tiny", "pair", unit(4, 1e-300, 1.0), {CHUNK: 8}, [5], [300])
    add("index_no_window_tiny", "index", unit(9, 1e-300, 1.0), {CHUNK: 8}, [76, 3], [300])
    add("index_no_window_ratio", "index", unit(9, 1e-3, 1.0), {CHUNK: 8}, [2048], [300])
    add("index_window_ratio_fits", "index", unit(9, 1e-3, 1.0), {CHUNK: 2000000}, [1000], [300])
    # empty cross products, and an option no plan takes
    add("pair_empty", "pair", T["unit"], {}, [], [], 1.0)
    add("index_no_queries", "index", T["unit"], {}, [], [10, 20])
    add("index_no_texts", "index", T["unit"], {}, [5, 40], [])
    add("index_no_texts_p0", "index", T["unit"], {}, [0], [])
    add("index_empty", "index", T["unit"], {}, [], [])
    add("pair_bad_option", "pair", T["unit"], {ROWS: 3}, [5], [10])
    add("index_bad_option", "index", T["unit"], {CHUNK: -1}, [5], [10])
    return out


def join_cases():
    """[(name, costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist)] for JOIN_CALLS."""
    out = []
    rows, cols = [0, 1, 9, 20, 32, 20, 31], [0, 1, 9, 20, 32, 20, 31, 5, 5, 18]
    u4, u5 = unit(4), unit(5)
    add = lambda name, costs, o, lr, lc, s, rc, cc, md: out.append((name, costs, o, lr, lc, s, rc, cc, md))
    for md in (0.0, 1.5, 4.0, math.inf, math.nan, -1.0):
        add("self_unit4_md%r" % md, u4, {}, cols, cols, True, 0xF, 0xF, md)
        add("search_unit5_md%r" % md, u5, {}, rows, cols, False, 0x1F, 0xF, md)
    add("search_unit5_four_codes", u5, {}, rows, cols, False, 0x1B, 0x12, 2.0)   # K = 5, four codes seen
    add("search_unit4_dp", u4, {JOIN_DP: 2}, rows, cols, False, 0xF, 0xF, 2.0)
    add("self_unit4_rows3", u4, {JOIN_ROWS: 3}, cols, cols, True, 0xF, 0xF, 2.0)
    add("search_unit4_rows3", u4, {JOIN_ROWS: 3}, rows, cols, False, 0xF, 0xF, 2.0)
    add("self_prefix", u4, {}, rows, cols, True, 0xF, 0xF, 2.0)                  # the rows: the first 7 columns
    add("self_more_rows_than_columns", u4, {}, cols, rows, True, 0xF, 0xF, 2.0)
    add("search_user", user(), {}, rows, cols, False, 0xF, 0x7, 4.5)
    add("self_user_k5", user("ACGUN"), {}, cols, cols, True, 0x1F, 0x1F, 2.25)   # S = 4
    add("search_third", unit(4, cell=((0, 1), 1.0 / 3)), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("search_k16", unit(16), {}, rows, cols, False, 0xFFFF, 0xF0F0, 3.0)
    add("search_off_unit_cell", unit(4, cell=((2, 3), 0.5)), {}, rows, cols, False, 0x3, 0x3, 2.0)  # not a cell met
    add("search_off_unit_cell_met", unit(4, cell=((2, 3), 0.5)), {}, rows, cols, False, 0x4, 0x8, 2.0)
    add("search_empty_rows", u4, {}, [], cols, False, 0, 0xF, 1.0)
    add("search_empty_cols", u4, {}, rows, [], False, 0xF, 0, 1.0)
    add("self_empty", u4, {}, [], [], True, 0, 0, 1.0)
    # refusals, alone and in pairs that show their order: arguments, max_dist, the costs rule, codes, rows, columns
    add("row_code_outside", u4, {}, rows, cols, False, 0x10, 0xF, 1.0)
    add("col_code_outside", u4, {}, rows, cols, False, 0xF, 0x10, 1.0)
    add("both_codes_outside", u4, {}, rows, cols, False, 0x20, 0x80000000, 1.0)
    add("col_code_outside_k16", unit(16), {}, rows, cols, False, 0xFFFF, 0x10000, 1.0)
    for bad in (65, -1):
        add("row_len_%d" % bad, u4, {}, [3, bad], cols, False, 0xF, 0xF, 1.0)
        add("col_len_%d" % bad, u4, {}, rows, [3, bad], False, 0xF, 0xF, 1.0)
        add("row_and_col_len_%d" % bad, u4, {}, [bad], [bad], False, 0xF, 0xF, 1.0)
    add("row_len_33", u4, {}, [33], cols, False, 0xF, 0xF, 1.0)
    add("code_before_length", u4, {}, [65], cols, False, 0x10, 0xF, 1.0)
    for K in (9, 17):
        add("k%d" % K, unit(K), {}, rows, cols, False, 0xF, 0xF, 1.0)
        add("k%d_before_code_and_length" % K, unit(K), {}, [65], cols, False, 1 << 20, 0xF, 1.0)
        add("k%d_after_max_dist" % K, unit(K), {}, rows, cols, False, 0xF, 0xF, math.nan)
    add("insert_below_one", unit(4, 0.0, 1.0), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("delete_below_one", unit(4, 1.0, 0.0), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("cell_above_insert_delete", unit(4, sub=3.0), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("addend_byte", unit(4, 100.0, 200.0), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("insert_negative", unit(4, -1.0, 1.0), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("cell_nan", unit(4, cell=((1, 2), math.nan)), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("delete_inf", unit(4, 1.0, math.inf), {}, rows, cols, False, 0xF, 0xF, 1.0)
    add("bad_option", u4, {JOIN_DP: 1}, rows, cols, False, 0xF, 0xF, 1.0)
    return out


KEEP_CASES = [(1.0, 1.0, 0.0), (1.0, 1.0, 1.5), (1.0, 1.0, math.inf), (2.0, 3.0, 4.0), (0.0, 0.0, 0.0), (0.1, 0.2, 0.3),
              (1e-300, 1.0, 1.0), (-0.0, 1.0, 2.0), (1.0, 1.0, math.nan), (1.0, 1.0, -1.0), (-1.0, 1.0, 1.0),
              (1.0, math.inf, 1.0)]


def _plain(v):
    """What a call returned, as JSON holds it: arrays as lists, numpy scalars as Python's."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def _call(fn, *args):
    try:
        return {"ok": _plain(fn(*args))}
    except sedgpu.SedError as e:
        return {"code": e.code}


def snapshot():
    """{case name: {export: {"ok": what it returned} or {"code": the SedError's}}}, through a JSON round trip so that
    a recomputed snapshot and a loaded one compare equal (NaN never appears in a result)."""
    snap = {}
    for name, form, costs, options, lp, lt, md in fit_cases():
        entry = {c: _call(getattr(sedgpu, c), costs, options, lp, lt) for c in (PAIR_CALLS if form == "pair" else INDEX_CALLS)}
        if md is not None:
            entry["fit_cutoff_scaled"] = _call(sedgpu.fit_cutoff_scaled, costs, options, lp, lt, md)
        snap["fit/" + name] = entry
    for name, *args in join_cases():
        snap["join/" + name] = {c: _call(getattr(sedgpu, c), *args) for c in JOIN_CALLS}
    for ins, dele, md in KEEP_CASES:
        got = _call(sedgpu.join_f64_keep, ins, dele, md)
        if "ok" in got:  # the 33 x 33 bools as each row's mask
            got["ok"] = [sum(1 << m for m, bit in enumerate(row) if bit) for row in got["ok"]]
        snap["keep/%r_%r_%r" % (ins, dele, md)] = got
    assert len(snap) == len(fit_cases()) + len(join_cases()) + len(KEEP_CASES), "two cases share a name"
    return json.loads(json.dumps(snap))
