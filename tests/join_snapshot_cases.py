"""The cases behind tests/golden/join_plan_snapshot.json: the device-free join exports tests/golden/plan_snapshot.json
does not pin - join_long_plan, join_knn_plan (short and long_index=True), join_knn_f64_plan and join_f64_lower - over
join_cases() of plan_snapshot_cases.py, a few long-length cases and k in {0, 1, 64, 65}, with what each call returns
or the SedError's code and text (the text only where the export has a channel for it).  tools/join_plan_snapshot.py
records them, tests/test_join_plan_snapshot.py recomputes them; both go through snapshot() below.

The file was recorded from the library of the commit before the five plan exports got their one body.  One answer of
it is that change's own (REORDERED below); every other record predates it."""
import ctypes as C
import hashlib
import json
import math

import numpy as np

import plan_snapshot_cases as base
import sedgpu

CALLS = ("join_long_plan", "join_knn_plan", "join_knn_plan_long", "join_knn_f64_plan")
K_EDGES = (0, 1, 64, 65)
# join_cases() whose every k of K_EDGES is recorded (the others run k = 1): a call every export serves, one the costs
# rule of the integer routes refuses, one both routes' argument checks refuse
K_CASES = ("search_user", "search_k16", "row_len_65")
LOWER_CASES = [(1.0, 1.0), (2.0, 3.0), (0.1, 0.2), (1e-300, 1.0), (-0.0, 1.0), (0.0, 0.0), (-1.0, 1.0), (1.0, math.inf),
               (math.nan, 1.0)]
# The one input whose answer is the tree's own, not the recording's: k out of range AND out = NULL with nout > 0.  Both
# are SED_E_ARG; sed_join_knn_plan used to name the arguments first, and now names k first as sed_join_knn_f64_plan did.
REORDERED = "raw/knn_plan_k0_null_out"


def long_cases():
    """join_cases()' tuples for lengths around the two index types' edges: 33, 127, 128, 129."""
    u4 = base.unit(4)
    out = []
    for n in (33, 127, 128, 129):
        out.append(("long_rows_%d" % n, u4, {}, [0, 5, n], [1, 40, 128, 64, 64], False, 0xF, 0xF, 3.0))
        out.append(("long_self_%d" % n, u4, {base.JOIN_ROWS: 2}, [n, 2, 100], [n, 2, 100], True, 0xF, 0xF, math.inf))
    out.append(("long_user_128", base.user(), {}, [128, 90], [128, 100, 7], False, 0xF, 0x7, 12.5))
    out.append(("long_key_room", base.unit(4, 100.0, 155.0), {}, [128], [128], False, 0xF, 0xF, 1.0))  # 255 * 128 <= 65535
    return out


def _call(fn, *args, **kw):
    try:
        return {"ok": base._plain(fn(*args, **kw))}
    except sedgpu.SedError as e:
        return {"code": e.code, "text": str(e)}


def _calls(args, k):
    *head, max_dist = args
    return {"join_long_plan": _call(sedgpu.join_long_plan, *args),
            "join_knn_plan": _call(sedgpu.join_knn_plan, *head, k, max_dist),
            "join_knn_plan_long": _call(sedgpu.join_knn_plan, *head, k, max_dist, long_index=True),
            "join_knn_f64_plan": _call(sedgpu.join_knn_f64_plan, *head, k, max_dist)}


def _lower(ins, dele):
    """join_f64_lower's 33 x 33 table as its two border rows, the two next to them and a digest of all of it."""
    try:
        low = sedgpu.join_f64_lower(ins, dele)
    except sedgpu.SedError as e:
        return {"code": e.code}
    return {"ok": {"row0": low[0].tolist(), "col0": low[:, 0].tolist(), "row1": low[1].tolist(), "col1": low[:, 1].tolist(),
                   "sha256": hashlib.sha256(np.ascontiguousarray(low).tobytes()).hexdigest()}}


def _raw_knn_plan(k, null_out):
    """sed_join_knn_plan called past the wrapper, which cannot pass a NULL out: (code, text)."""
    lib = C.CDLL(sedgpu.LIB_PATH)
    lib.sed_join_knn_plan_error.restype = C.c_char_p
    sub = (C.c_double * 16)(*base.unit(4)[1].ravel())
    sub_int = (C.c_uint8 * 16)(*base.unit(4)[2].ravel())
    lens = (C.c_int32 * 2)(3, 4)
    out = (C.c_double * 6)()
    rc = lib.sed_join_knn_plan(0, C.c_int32(k), 4, sub, sub_int, C.c_double(1.0), 0, C.c_double(1.0), 0, None, 0, lens, 2, lens,
                               2, 0, C.c_uint32(0xF), C.c_uint32(0xF), C.c_double(1.0), None if null_out else out, 6)
    return {"code": rc, "text": lib.sed_join_knn_plan_error().decode()}


def snapshot():
    """{case name: {call: {"ok": fields} or {"code": c, "text": t}}}, through a JSON round trip."""
    snap = {}
    for name, *args in base.join_cases() + long_cases():
        snap["join/" + name] = _calls(args, 1)
        if name in K_CASES:
            for k in K_EDGES:
                snap["join/%s_k%d" % (name, k)] = _calls(args, k)
    for ins, dele in LOWER_CASES:
        snap["lower/%r_%r" % (ins, dele)] = {"join_f64_lower": _lower(ins, dele)}
    snap["raw/knn_plan_k1_null_out"] = {"sed_join_knn_plan": _raw_knn_plan(1, True)}
    snap[REORDERED] = {"sed_join_knn_plan": _raw_knn_plan(0, True)}
    return json.loads(json.dumps(snap))
