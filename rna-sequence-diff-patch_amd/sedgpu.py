"""ctypes binding of libsed.so (include/sed.h) — the only way the Python side
reaches the GPU engine.  There is deliberately no CPU fallback: if the library
or a HIP device is missing, every entry point raises.

Process model.  The reference's callers parallelise by forking: gui.py runs
wagnerFisher in the GUI process (gui.py:360), then IRMethods.create_search_threads
forks a multiprocessing.Process per similarity method and again for wf_score
(IRMethods.py:487-491, 511-514).  HIP cannot be used in a child forked after the
parent initialised it.  context() therefore returns, in such a child, an
EngineClient that sends every call to an engine that owns a HIP context:
  - by default the parent itself: every fork of a process that holds a Context
    gets a socket pair.  One selector thread of the parent watches the pairs;
    a child's first request starts a thread that serves it on a Context of its
    own (from a pool of two, else a new one), and children that never call the
    engine cost only their socket.  A child pays no start-up beyond that
    sed_create, which is what create_search_threads' two Process rounds need.
    Served children need the parent alive: when it exits, their calls raise;
  - otherwise (SED_FORK_ENGINE=worker, a grandchild, or a fork taken while no
    Context existed) the child starts one engine worker, a fresh interpreter
    running this file, and talks to it over a pipe pair.
Processes that never inherited a HIP context use the GPU directly.
SED_ENGINE=worker keeps HIP out of the calling process always; SED_ENGINE=inproc
forbids both (a forked child then raises SedError).  An inherited Context is
never touched by the child (not even by __del__).
"""
import collections
import ctypes as C
import math
import os
import pickle
import socket
import subprocess
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SED_LIBRARY", os.path.join(HERE, "libsed.so"))

SED_WANT_SCRIPT = 1
SED_PIPELINE = 2
SED_NO_LEN = 4
SED_OPT_MODE = 1
SED_OPT_ROWS_PER_LANE = 2
SED_OPT_SPLIT = 3
SED_OPT_LANE = 4
SED_OPT_CHAIN = 5
SED_OPT_PACK = 6
SED_OPT_TB = 7
SED_OPT_CHAIN_WAVES = 8
SED_OPT_DEBUG_CORRUPT = 9
SED_OPT_DOT = 10
SED_OPT_BITPAR = 11
SED_OPT_SCALED = 12
SED_OPT_SEG = 13
SED_OPT_SPLITCK = 14
SED_OPT_ZEROCOPY = 15
SED_OPT_BAND = 16
SED_OPT_CUT = 17
SED_OPT_FIT_CHUNK = 18
SED_OPT_FIT_ROWS = 19
SED_OPT_JOIN_DP = 20
SED_OPT_JOIN_ROWS = 21
# sed_plan_routes only: the environment knobs the runtime reads once per process, as options of a plan
SED_PLAN_ENV_TBPAR = 101
SED_PLAN_ENV_BAND = 102
SED_PLAN_ENV_ALT_DP = 103
SED_PLAN_ENV_CK_HALVES = 104
MODE_NAMES = {1: "i32", 2: "f64", 3: "f64-typed"}
SED_E_ARG = -1
SED_E_RANGE = -4

_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")

# (name, restype, argtypes) — every symbol include/sed.h declares
SIGNATURES = [
    ("sed_version", C.c_char_p, []),
    ("sed_create", C.c_void_p, [C.c_int]),
    ("sed_destroy", None, [C.c_void_p]),
    ("sed_last_error", C.c_char_p, [C.c_void_p]),
    ("sed_set_option", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("sed_set_costs", C.c_int, [C.c_void_p, C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int]),
    ("sed_run_batch", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, C.c_uint32,
                                _f64p, _u8p, _i32p, C.c_void_p, C.c_void_p]),
    ("sed_batch_create", C.c_void_p, [C.c_void_p, _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, C.c_uint32]),
    ("sed_batch_destroy", None, [C.c_void_p]),
    ("sed_batch_mode", C.c_int, [C.c_void_p]),
    ("sed_batch_rows_per_lane", C.c_int, [C.c_void_p]),
    ("sed_batch_lane_pairs", C.c_int, [C.c_void_p]),
    ("sed_batch_chains", C.c_int, [C.c_void_p]),
    ("sed_batch_dot_keys", C.c_int, [C.c_void_p]),
    ("sed_plan_routes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                  _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, C.c_uint32, _f64p, C.c_int]),
    ("sed_plan_schedule", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                    _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, C.c_uint32, C.c_int, C.c_int,
                                    _i32p, C.c_int, _i32p]),
    ("sed_dot_factor", C.c_int, [_f64p, C.c_double, C.c_double, C.c_int, C.c_int, _u32p]),
    ("sed_band_bounds", C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, _i32p]),
    ("sed_band_chunk_range", C.c_int, [C.c_int32] * 6 + [_i32p]),
    ("sed_band_cells", C.c_double, [_f64p, C.c_double, C.c_double, _u8p, C.c_int32, _u8p, C.c_int32, C.c_int32]),
    ("sed_batch_band_cells", C.c_double, [C.c_void_p]),
    ("sed_batch_band_chunks_run", C.c_double, [C.c_void_p, _f64p]),
    ("sed_band_refine_row", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double,
                                      C.c_double, _i32p, C.c_int32, C.c_int32, _i32p]),
    ("sed_batch_set_cutoff", C.c_int, [C.c_void_p, C.c_double]),
    ("sed_batch_cutoff_hits", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    ("sed_batch_packed_pairs", C.c_int, [C.c_void_p]),
    ("sed_batch_bitpar_pairs", C.c_int, [C.c_void_p]),
    ("sed_batch_scaled_pairs", C.c_int, [C.c_void_p]),
    ("sed_batch_segment_pairs", C.c_int, [C.c_void_p]),
    ("sed_batch_split_tasks", C.c_int, [C.c_void_p]),
    ("sed_batch_traceback_mode", C.c_int, [C.c_void_p]),
    ("sed_batch_chain_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("sed_batch_run", C.c_int, [C.c_void_p]),
    ("sed_batch_sync", C.c_int, [C.c_void_p]),
    ("sed_batch_last_times", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("sed_batch_times", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int]),
    ("sed_batch_spans", C.c_int, [C.c_void_p, _f32p, C.c_int]),
    ("sed_batch_reset_times", C.c_int, [C.c_void_p]),
    ("sed_batch_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("sed_run_pair", C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sed_pair_submit", C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_uint32]),
    ("sed_pair_wait", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sed_batch_results", C.c_int, [C.c_void_p, _f64p, _u8p, _i32p, C.c_void_p, C.c_void_p]),
    ("sed_batch_dp_launches", C.c_int, [C.c_void_p]),
    ("sed_batch_device_results", C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 5),
    ("sed_batch_export", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]),
    ("sed_batch_work", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("sed_fit_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                               _i32p, _i32p, C.c_int32, _f64p, C.c_int]),
    ("sed_fit_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                _i32p, _i32p, C.c_int32, _i32p, C.c_int64, _u32p]),
    ("sed_fit_last_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_fit_index_create", C.c_void_p, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32]),
    ("sed_fit_index_destroy", None, [C.c_void_p]),
    ("sed_fit_index_texts", C.c_int32, [C.c_void_p]),
    ("sed_fit_index_symbols", C.c_int64, [C.c_void_p]),
    ("sed_fit_index_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_index_last_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_fit_index_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                     _i32p, C.c_int32, _i32p, C.c_int32, _f64p, C.c_int]),
    ("sed_fit_index_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                      _i32p, C.c_int32, _i32p, C.c_int32, _i32p, C.c_int64, _u32p]),
    ("sed_fit_index_hits", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    ("sed_fit_index_hits_last_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_fit_cutoff_scaled", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                        _i32p, _i32p, C.c_int32, C.c_double, C.POINTER(C.c_int64)]),
    ("sed_fit_index_search_long", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_index_hits_long", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                          C.POINTER(C.c_int64)]),
    ("sed_fit_index_long_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                          _i32p, C.c_int32, _i32p, C.c_int32, _f64p, C.c_int, _i32p]),
    ("sed_fit_index_long_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                           _i32p, C.c_int32, _i32p, C.c_int32, _i32p, C.c_int64, _u32p]),
    ("sed_fit_search_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_index_search_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_index_hits_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_int64)]),
    ("sed_fit_f64_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                   _i32p, _i32p, C.c_int32, _f64p, C.c_int]),
    ("sed_fit_f64_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                    _i32p, _i32p, C.c_int32, _i32p, C.c_int64]),
    ("sed_fit_index_f64_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                         _i32p, C.c_int32, _i32p, C.c_int32, _f64p, C.c_int]),
    ("sed_fit_index_f64_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                          _i32p, C.c_int32, _i32p, C.c_int32, _i32p, C.c_int64]),
    ("sed_fit_route", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                _i32p, _i32p, C.c_int32, C.c_char_p, C.c_int]),
    ("sed_fit_index_search_long_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, _f64p, _i32p, _i32p]),
    ("sed_fit_index_hits_long_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                              C.POINTER(C.c_int64)]),
    ("sed_fit_index_long_f64_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                              _i32p, C.c_int32, _i32p, C.c_int32, _f64p, C.c_int, _i32p]),
    ("sed_fit_index_long_f64_lanes", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                               _i32p, C.c_int32, _i32p, C.c_int32, _i32p, C.c_int64]),
    ("sed_fit_long_route", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                     _i32p, C.c_int32, _i32p, C.c_int32, C.c_char_p, C.c_int]),
    ("sed_join_index_create", C.c_void_p, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32]),
    ("sed_join_index_destroy", None, [C.c_void_p]),
    ("sed_join_index_seqs", C.c_int32, [C.c_void_p]),
    ("sed_join_self", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int64)]),
    ("sed_join_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64)]),
    ("sed_join_last_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_join_pairs_run", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("sed_join_rows_per_group", C.c_int32, []),
    ("sed_join_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32, C.c_double,
                                _f64p, C.c_int]),
    ("sed_join_knn_self", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64)]),
    ("sed_join_knn_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                      C.c_int64, C.POINTER(C.c_int64)]),
    ("sed_join_knn_bounds", C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    ("sed_join_knn_candidates", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("sed_join_knn_bound_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_join_knn_trim", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    ("sed_join_decode", C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_char_p, C.c_int]),
    ("sed_join_knn_plan", C.c_int, [C.c_int, C.c_int32, C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int,
                                    _i32p, C.c_int, _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32,
                                    C.c_double, _f64p, C.c_int]),
    ("sed_join_knn_plan_error", C.c_char_p, []),
    ("sed_join_self_f64", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64)]),
    ("sed_join_search_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                      C.POINTER(C.c_int64)]),
    ("sed_join_f64_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                    _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32, C.c_double,
                                    _f64p, C.c_int]),
    ("sed_join_f64_keep", C.c_int, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint64)]),
    ("sed_join_knn_self_f64", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64)]),
    ("sed_join_knn_search_f64", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                          C.c_int64, C.POINTER(C.c_int64)]),
    ("sed_join_knn_bounds_f64", C.c_int, [C.c_void_p, _f64p, C.c_int32]),
    ("sed_join_knn_f64_plan", C.c_int, [C.c_int32, C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p,
                                        C.c_int, _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32,
                                        C.c_double, _f64p, C.c_int]),
    ("sed_join_f64_lower", C.c_int, [C.c_double, C.c_double, _f64p]),
    ("sed_join_route", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                 _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32, C.c_double,
                                 C.c_char_p, C.c_int]),
    ("sed_join_long_index_create", C.c_void_p, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32]),
    ("sed_join_long_index_destroy", None, [C.c_void_p]),
    ("sed_join_long_index_seqs", C.c_int32, [C.c_void_p]),
    ("sed_join_long_self", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    ("sed_join_long_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                       C.POINTER(C.c_int64)]),
    ("sed_join_long_last_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_join_long_pairs_run", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("sed_join_long_knn_self", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_int64)]),
    ("sed_join_long_knn_search", C.c_int, [C.c_void_p, _u8p, _i64p, _i32p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                           C.c_int64, C.POINTER(C.c_int64)]),
    ("sed_join_long_knn_bounds", C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    ("sed_join_long_knn_candidates", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("sed_join_long_knn_bound_time", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("sed_join_long_max_len", C.c_int32, []),
    ("sed_join_long_plan", C.c_int, [C.c_int, _f64p, _u8p, C.c_double, C.c_int, C.c_double, C.c_int, _i32p, C.c_int,
                                     _i32p, C.c_int32, _i32p, C.c_int32, C.c_int, C.c_uint32, C.c_uint32, C.c_double,
                                     _f64p, C.c_int]),
    ("sed_join_long_plan_error", C.c_char_p, []),
    ("sed_selftest", C.c_int, [C.c_void_p]),
    ("sed_full_matrix", C.c_int, [C.c_void_p, _u8p, C.c_int32, _u8p, C.c_int32, _f64p, _u8p]),
]

_lib = None
_lock = threading.Lock()


class SedError(RuntimeError):
    pass


def load():
    """Load libsed.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SedError("libsed.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                       % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


_hip_pid = None  # pid of the process whose HIP context this module created (inherited by forked children)


class Context:
    """One sed_ctx (device + stream + cost table), owned by the process that created it."""

    def __init__(self, device=0):
        global _hip_pid
        if _hip_pid is not None and _hip_pid != os.getpid():
            raise SedError("HIP was initialised by process %d and this process is a fork of it: use "
                           "sedgpu.context(), which runs the engine in a worker process" % _hip_pid)
        lib = load()
        self._lib = lib
        self._pid = os.getpid()
        self.device = device
        self.ptr = lib.sed_create(device)
        _hip_pid = self._pid
        if not self.ptr:
            raise SedError("sed_create(%d) failed: no usable HIP device" % device)
        self._cost_key = None
        self._cost_plan = None
        self._pair_out = None
        self._pending = None  # (want_script, script words) of a submit_pair not yet waited for

    def close(self):
        # a forked child must not call into the parent's HIP context (it would destroy or hang on it)
        if self.ptr and self._pid == os.getpid():
            self._lib.sed_destroy(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if self._pid != os.getpid():
            raise SedError("%s: this Context belongs to process %d (fork); use sedgpu.context()" % (what, self._pid))
        if rc != 0:
            msg = self._lib.sed_last_error(self.ptr)
            raise SedError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def set_option(self, key, value):
        self._check(self._lib.sed_set_option(self.ptr, key, value), "sed_set_option")

    def set_mode(self, mode):
        """0 auto, 1 integer, 2 fp64, 3 fp64 with int typing."""
        self.set_option(SED_OPT_MODE, mode)
        self.invalidate_costs()

    def invalidate_costs(self):
        """Forget the cached cost plan: the next set_costs() uploads its table.  Call it after any direct
        lib.sed_set_costs / mode change that bypasses set_costs()."""
        self._cost_key = None
        self._cost_plan = None

    def set_costs(self, plan):
        if plan is self._cost_plan:  # (sedcost.pair_plan hands out the same plan object for the same costs)
            return
        key = plan.key()
        if key == self._cost_key:
            self._cost_plan = plan
            return
        self._cost_plan = None
        sub = np.ascontiguousarray(plan.sub, dtype=np.float64).ravel()
        sub_int = np.ascontiguousarray(plan.sub_int, dtype=np.uint8).ravel()
        self._check(self._lib.sed_set_costs(self.ptr, plan.K, sub, sub_int, plan.ins, plan.ins_int,
                                            plan.dele, plan.del_int), "sed_set_costs")
        self._cost_key = key
        self._cost_plan = plan

    def selftest(self):
        return self._lib.sed_selftest(self.ptr)

    def run(self, packed, want_script, no_len=False):
        """packed: PackedPairs.  Returns (dist f64[], is_int u8[], len i32[], ops u32[] | None).
        no_len (distance only): lengths are not computed (-1), the integer kernels run 3 ops/cell."""
        np_ = packed.npairs
        dist = np.zeros(max(np_, 1), np.float64)
        is_int = np.zeros(max(np_, 1), np.uint8)
        ln = np.zeros(max(np_, 1), np.int32)
        ops = None
        ops_ptr = ops_off_ptr = None
        if want_script:
            ops = np.zeros(max(int(packed.ops_off[-1]), 1), np.uint32)
            ops_ptr = ops.ctypes.data_as(C.c_void_p)
            ops_off_ptr = packed.ops_off.ctypes.data_as(C.c_void_p)
        rc = self._lib.sed_run_batch(self.ptr, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b,
                                     packed.off_b, packed.len_b, np_,
                                     SED_WANT_SCRIPT if want_script else (SED_NO_LEN if no_len else 0),
                                     dist, is_int, ln, ops_ptr, ops_off_ptr)
        self._check(rc, "sed_run_batch")
        return dist[:np_], is_int[:np_], ln[:np_], ops

    def run_cutoff(self, packed, max_dist, no_len=True):
        """Distances of packed's pairs under a cutoff, one launch: (dist, is_int, len, hits); pairs beyond max_dist
        come back as (inf, 0, -1)."""
        return self.deepen(packed, 0, max_dist, max_dist, no_len)[:4]

    def deepen(self, packed, k, first, last, no_len=True):
        """One resident batch run under the cutoff `first`, doubled until at least k pairs are within it or it has
        reached `last` (the deepening loop of wfsearch.nearest; no input is uploaded twice).
        Returns (dist, is_int, len, hits, cutoffs tried)."""
        batch = Batch(self, packed, False, no_len=no_len)
        try:
            cut, cuts = float(first), []
            while True:
                batch.set_cutoff(cut)
                batch.run()
                cuts.append(cut)
                hits = batch.cutoff_hits()
                if hits >= k or cut >= last:
                    break
                cut = min(2.0 * cut, float(last))
            dist, is_int, ln, _ = batch.results()
            return dist, is_int, ln, hits, cuts
        finally:
            batch.close()

    def fit(self, packed, _call="sed_fit_search"):
        """Fit search (sed_fit_search): packed = PackedPairs with the patterns (1..32 symbols) as side a and the texts
        as side b.  Returns (dist f64[], start i32[], end i32[]): for each pair the smallest distance of the pattern to
        any substring text[start:end], the occurrence ending earliest and, among those, the shortest.  Serves dyadic
        tables over at most 8 symbols; fit_f64 serves the rest, and fit_route says which a search needs."""
        np_ = packed.npairs
        dist = np.zeros(max(np_, 1), np.float64)
        start = np.zeros(max(np_, 1), np.int32)
        end = np.zeros(max(np_, 1), np.int32)
        rc = getattr(self._lib, _call)(self.ptr, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b,
                                       packed.off_b, packed.len_b, np_, dist, start, end)
        self._check(rc, _call)
        return dist[:np_], start[:np_], end[:np_]

    def fit_f64(self, packed):
        """fit() through the fp64 kernels (sed_fit_search_f64): any table of finite costs >= 0 over at most 16 symbols;
        dist is the fp64 value of the definition's own order of additions."""
        return self.fit(packed, "sed_fit_search_f64")

    def fit_last_ms(self):
        """Device time of the last fit()'s kernel (ms, HIP events)."""
        ms = C.c_float()
        self._check(self._lib.sed_fit_last_time(self.ptr, C.byref(ms)), "sed_fit_last_time")
        return ms.value

    def fit_index(self, codes, off, lens):
        """A resident text index for fit search (sed_fit_index_create): text d = codes[off[d] : off[d] + lens[d]],
        uploaded once.  FitIndex.search then sends only the queries."""
        return FitIndex(self, codes, off, lens)

    def join_index(self, codes, off, lens):
        """A resident index of short sequences for the similarity join (sed_join_index_create): sequence i =
        codes[off[i] : off[i] + lens[i]], 0..32 symbols, uploaded once."""
        return JoinIndex(self, codes, off, lens)

    def join_long_index(self, codes, off, lens):
        """join_index for sequences of 0..128 symbols (sed_join_long_index_create): the integer route only."""
        return LongJoinIndex(self, codes, off, lens)

    def run_pair(self, codes_a, codes_b, want_script, no_len=False):
        """One pair (codes as bytes): (dist, is_int, len, ops u32[] | None) through sed_run_pair, the per-call path of
        the drop-in module (no numpy arrays on the way in, preallocated result cells on the way out)."""
        if self._pid != os.getpid():
            self._check(0, "sed_run_pair")
        r = self._pair_out
        if r is None:
            r = self._pair_out = (C.c_double(), C.c_uint8(), C.c_int32())
        ops = None
        ops_ptr = None
        if want_script:
            ops = np.zeros(max(1, (len(codes_a) + len(codes_b) + 15) // 16), np.uint32)
            ops_ptr = ops.ctypes.data
        flags = SED_WANT_SCRIPT if want_script else (SED_NO_LEN if no_len else 0)
        rc = self._lib.sed_run_pair(self.ptr, codes_a, len(codes_a), codes_b, len(codes_b), flags, C.addressof(r[0]),
                                    C.addressof(r[1]), C.addressof(r[2]), ops_ptr)
        if rc != 0:
            self._check(rc, "sed_run_pair")
        return r[0].value, r[1].value, r[2].value, ops

    def submit_pair(self, codes_a, codes_b, want_script, no_len=False):
        """run_pair's first half (sed_pair_submit): the pair's kernels are enqueued and this returns at once;
        wait_pair() returns what run_pair would have."""
        if self._pid != os.getpid():
            self._check(0, "sed_pair_submit")
        flags = SED_WANT_SCRIPT if want_script else (SED_NO_LEN if no_len else 0)
        rc = self._lib.sed_pair_submit(self.ptr, codes_a, len(codes_a), codes_b, len(codes_b), flags)
        if rc != 0:
            self._check(rc, "sed_pair_submit")
        self._pending = (want_script, (len(codes_a) + len(codes_b) + 15) // 16)

    def wait_pair(self):
        """(dist, is_int, len, ops u32[] | None) of the pair submit_pair enqueued (sed_pair_wait)."""
        want_script, words = self._pending
        self._pending = None
        r = self._pair_out
        if r is None:
            r = self._pair_out = (C.c_double(), C.c_uint8(), C.c_int32())
        ops = np.zeros(max(1, words), np.uint32) if want_script else None
        rc = self._lib.sed_pair_wait(self.ptr, C.addressof(r[0]), C.addressof(r[1]), C.addressof(r[2]),
                                     ops.ctypes.data if want_script else None)
        if rc != 0:
            self._check(rc, "sed_pair_wait")
        return r[0].value, r[1].value, r[2].value, ops

    def full_matrix(self, codes_a, codes_b):
        n, m = len(codes_a), len(codes_b)
        D = np.zeros((n + 1) * (m + 1), np.float64)
        M = np.zeros((n + 1) * (m + 1), np.uint8)
        rc = self._lib.sed_full_matrix(self.ptr, np.ascontiguousarray(codes_a, np.uint8) if n else np.zeros(1, np.uint8),
                                       n, np.ascontiguousarray(codes_b, np.uint8) if m else np.zeros(1, np.uint8),
                                       m, D, M)
        self._check(rc, "sed_full_matrix")
        return D.reshape(n + 1, m + 1), M.reshape(n + 1, m + 1)


class PackedPairs:
    """Concatenated codes + offsets for a list of (codes_a, codes_b) pairs."""

    def __init__(self, pairs_a, pairs_b):
        self.npairs = len(pairs_a)
        self.len_a = np.array([len(x) for x in pairs_a] or [0], dtype=np.int32)
        self.len_b = np.array([len(x) for x in pairs_b] or [0], dtype=np.int32)
        self.off_a = np.zeros(max(self.npairs, 1), np.int64)
        self.off_b = np.zeros(max(self.npairs, 1), np.int64)
        if self.npairs:
            self.off_a[1:] = np.cumsum(self.len_a[:-1])
            self.off_b[1:] = np.cumsum(self.len_b[:-1])
        self.codes_a = np.concatenate([np.asarray(x, np.uint8) for x in pairs_a] + [np.zeros(1, np.uint8)])
        self.codes_b = np.concatenate([np.asarray(x, np.uint8) for x in pairs_b] + [np.zeros(1, np.uint8)])
        words = (self.len_a.astype(np.int64) + self.len_b + 15) // 16
        self.ops_off = np.zeros(max(self.npairs, 1) + 1, np.int64)
        if self.npairs:
            self.ops_off[1:self.npairs + 1] = np.cumsum(words[:self.npairs])

    @classmethod
    def from_concat(cls, codes_a, len_a, codes_b, len_b):
        """Pairs from concatenated codes and per-pair lengths (CostPlan.encode_many)."""
        self = cls.__new__(cls)
        P = len(len_a)
        self.npairs = P
        self.len_a = np.asarray(len_a, np.int32) if P else np.zeros(1, np.int32)
        self.len_b = np.asarray(len_b, np.int32) if P else np.zeros(1, np.int32)
        self.off_a = np.zeros(max(P, 1), np.int64)
        self.off_b = np.zeros(max(P, 1), np.int64)
        if P:
            self.off_a[1:] = np.cumsum(self.len_a[:-1])
            self.off_b[1:] = np.cumsum(self.len_b[:-1])
        self.codes_a = np.concatenate([np.asarray(codes_a, np.uint8), np.zeros(1, np.uint8)])
        self.codes_b = np.concatenate([np.asarray(codes_b, np.uint8), np.zeros(1, np.uint8)])
        words = (self.len_a.astype(np.int64) + self.len_b + 15) // 16
        self.ops_off = np.zeros(max(P, 1) + 1, np.int64)
        if P:
            self.ops_off[1:P + 1] = np.cumsum(words[:P])
        return self

    @classmethod
    def from_arrays(cls, A, B):
        """Fixed-length pairs from 2-D uint8 arrays (npairs x n), (npairs x m)."""
        self = cls.__new__(cls)
        P, n = A.shape
        m = B.shape[1]
        self.npairs = P
        self.len_a = np.full(max(P, 1), n, np.int32)
        self.len_b = np.full(max(P, 1), m, np.int32)
        self.off_a = (np.arange(max(P, 1), dtype=np.int64) * n)
        self.off_b = (np.arange(max(P, 1), dtype=np.int64) * m)
        self.codes_a = np.ascontiguousarray(np.concatenate([A.ravel(), np.zeros(1, np.uint8)]), np.uint8)
        self.codes_b = np.ascontiguousarray(np.concatenate([B.ravel(), np.zeros(1, np.uint8)]), np.uint8)
        w = (n + m + 15) // 16
        self.ops_off = np.arange(max(P, 1) + 1, dtype=np.int64) * w
        return self


# one sed_fit_hit (include/sed.h)
FIT_HIT_DTYPE = np.dtype([("query", np.int32), ("text", np.int32), ("start", np.int32), ("end", np.int32),
                          ("dist", np.float64)], align=True)


class FitIndex:
    """Device-resident texts for fit search (sed_fit_index_*): upload once, search many times.  search() and hits() run
    under the context's costs and options of that moment."""

    def __init__(self, ctx, codes, off, lens):
        self.ctx = ctx
        self.found = 0       # the last hits()' total count
        self._hit_room = 0   # records the last hits(cap=None) made room for: the next one starts there
        self._lib = ctx._lib
        lens = np.ascontiguousarray(lens, np.int32)
        off = np.ascontiguousarray(off, np.int64)
        self.ntexts = len(lens)
        codes = np.ascontiguousarray(codes, np.uint8)
        one = lambda a, t: a if len(a) else np.zeros(1, t)
        self.ptr = self._lib.sed_fit_index_create(ctx.ptr, one(codes, np.uint8), one(off, np.int64), one(lens, np.int32),
                                                  self.ntexts)
        if not self.ptr:
            msg = self._lib.sed_last_error(ctx.ptr)
            raise SedError("sed_fit_index_create failed: %s" % (msg.decode() if msg else ""))

    @classmethod
    def from_texts(cls, ctx, texts):
        """From a list of uint8 code arrays."""
        lens = np.array([len(t) for t in texts], np.int32)
        off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64) if len(texts) else np.zeros(0, np.int64)
        codes = np.concatenate([np.asarray(t, np.uint8) for t in texts]) if len(texts) else np.zeros(0, np.uint8)
        return cls(ctx, codes, off, lens)

    def close(self):
        if self.ptr and self.ctx.ptr and self.ctx._pid == os.getpid():
            self._lib.sed_fit_index_destroy(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def symbols(self):
        return int(self._lib.sed_fit_index_symbols(self.ptr))

    def search(self, packed, _call="sed_fit_index_search"):
        """packed: the queries as side a of a PackedPairs (codes_a, off_a, len_a, npairs; side b is not read).  Returns
        (dist f64, start i32, end i32), each shaped (queries, texts): the hits Context.fit gives for every (query,
        text), from one launch."""
        if not self.ptr:
            raise SedError("%s: the index is closed" % _call)
        Q, D = packed.npairs, self.ntexts
        dist = np.zeros(max(Q * D, 1), np.float64)
        start = np.zeros(max(Q * D, 1), np.int32)
        end = np.zeros(max(Q * D, 1), np.int32)
        rc = getattr(self._lib, _call)(self.ptr, packed.codes_a, packed.off_a, packed.len_a, Q, dist, start, end)
        self.ctx._check(rc, _call)
        return dist[:Q * D].reshape(Q, D), start[:Q * D].reshape(Q, D), end[:Q * D].reshape(Q, D)

    def search_long(self, packed):
        """search() for queries of 1..2048 symbols (sed_fit_index_search_long): one wave per (query, chunk of a text).
        The same results, bit for bit, where search() serves the queries."""
        return self.search(packed, "sed_fit_index_search_long")

    def hits_long(self, packed, max_dist, cap=None):
        """hits() for queries of 1..2048 symbols (sed_fit_index_hits_long)."""
        return self.hits(packed, max_dist, cap, "sed_fit_index_hits_long")

    def search_long_f64(self, packed):
        """search_long() through the fp64 kernels (sed_fit_index_search_long_f64): queries of 1..2048 symbols under the
        tables and alphabets (up to 16 symbols) search_long refuses; the values are the oracle's, bit for bit."""
        return self.search(packed, "sed_fit_index_search_long_f64")

    def hits_long_f64(self, packed, max_dist, cap=None):
        """hits_long() through the fp64 kernels (sed_fit_index_hits_long_f64)."""
        return self.hits(packed, max_dist, cap, "sed_fit_index_hits_long_f64")

    def search_f64(self, packed):
        """search() through the fp64 kernels (sed_fit_index_search_f64): the tables and alphabets (up to 16 symbols)
        search() refuses, on the same resident texts."""
        return self.search(packed, "sed_fit_index_search_f64")

    def hits_f64(self, packed, max_dist, cap=None):
        """hits() through the fp64 kernels (sed_fit_index_hits_f64): a hit is a column whose fp64 value is <= max_dist."""
        return self.hits(packed, max_dist, cap, "sed_fit_index_hits_f64")

    @staticmethod
    def long_plan(costs, options, len_p, len_t):
        """What search_long / hits_long would decide, without a device: fit_index_long_plan."""
        return fit_index_long_plan(costs, options, len_p, len_t)

    @staticmethod
    def long_lanes(costs, options, len_p, len_t):
        """The wave records search_long / hits_long would run, without a device: fit_index_long_lanes."""
        return fit_index_long_lanes(costs, options, len_p, len_t)

    def last_ms(self):
        """Device time of the last search's kernel (ms, HIP events)."""
        ms = C.c_float()
        self.ctx._check(self._lib.sed_fit_index_last_time(self.ptr, C.byref(ms)), "sed_fit_index_last_time")
        return ms.value

    def hits(self, packed, max_dist, cap=None, _call="sed_fit_index_hits"):
        """Every hit within max_dist (sed_fit_index_hits): packed as for search().  Returns a structured array over
        FIT_HIT_DTYPE (query, text, start, end, dist), one record per (query, text, end column) whose best distance is
        <= max_dist, sorted by (query, text, end).  cap = the records to make room for: more hits than that raise
        SedError (the index stays usable; FitIndex.found has the count).  cap=None asks for the count first when nothing
        is known and retries with room, so it always returns every hit."""
        if not self.ptr:
            raise SedError("%s: the index is closed" % _call)
        Q = packed.npairs
        found = C.c_int64(0)
        room = self._hit_room if cap is None else int(cap)
        while True:
            out = np.zeros(max(room, 1), FIT_HIT_DTYPE)
            rc = getattr(self._lib, _call)(self.ptr, packed.codes_a, packed.off_a, packed.len_a, Q, float(max_dist),
                                           out.ctypes.data if room > 0 else None, room, C.byref(found))
            self.found = int(found.value)
            if rc == SED_E_RANGE and cap is None and self.found > room:
                room = self.found  # (a refusal of the plan leaves found at 0 <= room)
                continue
            self.ctx._check(rc, _call)
            if cap is None:
                self._hit_room = max(self._hit_room, room)
            return out[:self.found]

    def hits_last_ms(self):
        """Device time of the last hits()' kernel (ms, HIP events)."""
        ms = C.c_float()
        self.ctx._check(self._lib.sed_fit_index_hits_last_time(self.ptr, C.byref(ms)), "sed_fit_index_hits_last_time")
        return ms.value


# one sed_join_hit (include/sed.h)
JOIN_HIT_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("dist", np.float64)], align=True)


def join_rows_per_group():
    """The rows a block of the join kernel runs against its columns (sed_join_rows_per_group)."""
    return int(load().sed_join_rows_per_group())


class JoinIndex:
    """Device-resident short sequences (0..32 symbols each) for the similarity join (sed_join_*): upload once, then
    self_join() / search() return every (row, col) pair within a distance as a JOIN_HIT_DTYPE array sorted by (row, col),
    under the context's costs and options of that moment.  Rows are str1, columns str2."""

    _PREFIX = "sed_join_"  # the entry points' names: _PREFIX + index_create, self, search, last_time, pairs_run, ...

    def __init__(self, ctx, codes, off, lens):
        self.ctx = ctx
        self.found = 0       # the last call's total count
        self._hit_room = 0   # records the last cap=None call made room for: the next one starts there
        self._knn_rows = 0   # the rows of the last self_knn / search_knn call
        self._lib = ctx._lib
        lens = np.ascontiguousarray(lens, np.int32)
        off = np.ascontiguousarray(off, np.int64)
        self.nseqs = len(lens)
        codes = np.ascontiguousarray(codes, np.uint8)
        one = lambda a, t: a if len(a) else np.zeros(1, t)
        create = self._PREFIX + "index_create"
        self.ptr = getattr(self._lib, create)(ctx.ptr, one(codes, np.uint8), one(off, np.int64), one(lens, np.int32),
                                              self.nseqs)
        if not self.ptr:
            msg = self._lib.sed_last_error(ctx.ptr)
            raise SedError("%s failed: %s" % (create, msg.decode() if msg else ""))

    @classmethod
    def from_seqs(cls, ctx, seqs):
        """From a list of uint8 code arrays."""
        lens = np.array([len(t) for t in seqs], np.int32)
        off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64) if len(seqs) else np.zeros(0, np.int64)
        codes = np.concatenate([np.asarray(t, np.uint8) for t in seqs]) if len(seqs) else np.zeros(0, np.uint8)
        return cls(ctx, codes, off, lens)

    def close(self):
        if self.ptr and self.ctx.ptr and self.ctx._pid == os.getpid():
            getattr(self._lib, self._PREFIX + "index_destroy")(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _hits(self, what, call, cap):
        if not self.ptr:
            raise SedError("%s: the index is closed" % what)
        found = C.c_int64(0)
        room = self._hit_room if cap is None else int(cap)
        while True:
            out = np.zeros(max(room, 1), JOIN_HIT_DTYPE)
            rc = call(out.ctypes.data if room > 0 else None, room, C.byref(found))
            self.found = int(found.value)
            if rc == SED_E_RANGE and cap is None and self.found > room:
                room = self.found  # (a refusal of the plan leaves found at 0 <= room)
                continue
            self.ctx._check(rc, what)
            if cap is None:
                self._hit_room = max(self._hit_room, room)
            return out[:self.found]

    def self_join(self, max_dist, rows=None, cap=None, _call=None):
        """Every (i, j), i != j, i in rows = (lo, hi) (default: every sequence), with distance(seq i -> seq j) <=
        max_dist (sed_join_self).  cap = the records to make room for: more hits raise SedError (the index stays
        usable; found has the count; cap=0 is a count query).  cap=None retries once with room, so it returns every hit."""
        lo, hi = (0, self.nseqs) if rows is None else rows
        _call = _call or self._PREFIX + "self"
        fn = getattr(self._lib, _call)
        return self._hits(_call, lambda out, room, found: fn(
            self.ptr, int(lo), int(hi), float(max_dist), out, room, found), cap)

    def search(self, packed, max_dist, cap=None, _call=None):
        """Every (q, j) with distance(query q -> seq j) <= max_dist (sed_join_search); packed: the queries as side a of
        a PackedPairs, 0..32 symbols each.  cap as for self_join."""
        _call = _call or self._PREFIX + "search"
        fn = getattr(self._lib, _call)
        return self._hits(_call, lambda out, room, found: fn(
            self.ptr, packed.codes_a, packed.off_a, packed.len_a, packed.npairs, float(max_dist), out, room, found), cap)

    def self_join_f64(self, max_dist, rows=None, cap=None):
        """self_join() through the fp64 kernel (sed_join_self_f64): the tables and alphabets (up to 16 symbols)
        self_join() refuses, on the same resident sequences; dist is the oracle's double, bit for bit."""
        return self.self_join(max_dist, rows, cap, "sed_join_self_f64")

    def search_f64(self, packed, max_dist, cap=None):
        """search() through the fp64 kernel (sed_join_search_f64)."""
        return self.search(packed, max_dist, cap, "sed_join_search_f64")

    def self_knn(self, k, max_dist=math.inf, rows=None, cap=None, _call=None):
        """For every i in rows = (lo, hi) (default: every sequence), the k sequences j != i of smallest distance(seq i ->
        seq j) among those within max_dist (sed_join_knn_self): JOIN_HIT_DTYPE records sorted by (row, dist, col), ties
        going to the lower column.  k = 1..64; exact.  cap as for self_join (None: room for k a row, which suffices)."""
        lo, hi = (0, self.nseqs) if rows is None else rows
        _call = _call or self._PREFIX + "knn_self"
        fn = getattr(self._lib, _call)
        self._knn_rows = max(int(hi) - int(lo), 0)
        return self._hits(_call, lambda out, room, found: fn(
            self.ptr, int(lo), int(hi), int(k), float(max_dist), out, room, found),
            self._knn_rows * min(max(int(k), 0), 64) if cap is None else cap)

    def search_knn(self, packed, k, max_dist=math.inf, cap=None, _call=None):
        """For every query q, the k sequences of smallest distance(query q -> seq j) among those within max_dist
        (sed_join_knn_search); packed and cap as for search and self_knn."""
        _call = _call or self._PREFIX + "knn_search"
        fn = getattr(self._lib, _call)
        self._knn_rows = packed.npairs
        return self._hits(_call, lambda out, room, found: fn(
            self.ptr, packed.codes_a, packed.off_a, packed.len_a, packed.npairs, int(k), float(max_dist), out, room, found),
            self._knn_rows * min(max(int(k), 0), 64) if cap is None else cap)

    def self_knn_f64(self, k, max_dist=math.inf, rows=None, cap=None):
        """self_knn() through the fp64 kernel (sed_join_knn_self_f64): the tables and alphabets (up to 16 symbols)
        self_knn() refuses; the order is by (the oracle's double, col) and dist is that double, bit for bit."""
        return self.self_knn(k, max_dist, rows, cap, "sed_join_knn_self_f64")

    def search_knn_f64(self, packed, k, max_dist=math.inf, cap=None):
        """search_knn() through the fp64 kernel (sed_join_knn_search_f64)."""
        return self.search_knn(packed, k, max_dist, cap, "sed_join_knn_search_f64")

    def knn_bounds_f64(self):
        """The last self_knn_f64 / search_knn_f64 call's bound of every row after its first pass, as doubles, one per row
        of the call (sed_join_knn_bounds_f64)."""
        out = np.zeros(max(self._knn_rows, 1), np.float64)
        self.ctx._check(self._lib.sed_join_knn_bounds_f64(self.ptr, out, self._knn_rows), "sed_join_knn_bounds_f64")
        return out[:self._knn_rows]

    def knn_bounds(self):
        """The last self_knn / search_knn call's bound of every row after its first pass, on the integer scale (D * S),
        one per row of the call (sed_join_knn_bounds)."""
        out = np.zeros(max(self._knn_rows, 1), np.int32)
        name = self._PREFIX + "knn_bounds"
        self.ctx._check(getattr(self._lib, name)(self.ptr, out, self._knn_rows), name)
        return out[:self._knn_rows]

    @property
    def knn_candidates(self):
        """The hits the last self_knn / search_knn call's second pass appended, before the trim (sed_join_knn_candidates)."""
        n = C.c_int64()
        name = self._PREFIX + "knn_candidates"
        self.ctx._check(getattr(self._lib, name)(self.ptr, C.byref(n)), name)
        return int(n.value)

    def knn_bound_ms(self):
        """Device time of the first pass of the last self_knn / search_knn call's first launch (ms, HIP events): with one
        launch, last_ms() less this is the second pass."""
        ms = C.c_float()
        name = self._PREFIX + "knn_bound_time"
        self.ctx._check(getattr(self._lib, name)(self.ptr, C.byref(ms)), name)
        return ms.value

    def last_ms(self):
        """Device time of the last join's kernel(s) (ms, HIP events)."""
        ms = C.c_float()
        self.ctx._check(getattr(self._lib, self._PREFIX + "last_time")(self.ptr, C.byref(ms)), self._PREFIX + "last_time")
        return ms.value

    def pairs_run(self):
        """The pairs the last join's waves ran, counted on the device (sed_join_pairs_run): join_plan's "run"."""
        n = C.c_int64()
        self.ctx._check(getattr(self._lib, self._PREFIX + "pairs_run")(self.ptr, C.byref(n)), self._PREFIX + "pairs_run")
        return int(n.value)


def join_long_max_len():
    """The longest sequence a LongJoinIndex holds (sed_join_long_max_len): 128."""
    return int(load().sed_join_long_max_len())


class LongJoinIndex(JoinIndex):
    """JoinIndex for sequences of 0..128 symbols each (sed_join_long_*): the same calls, records, sort and cap protocol
    through the integer route's long kernel; the queries of search() have 0..128 symbols too.  There is no fp64 route
    for it yet."""

    _PREFIX = "sed_join_long_"

    def self_join_f64(self, max_dist, rows=None, cap=None):
        raise SedError("the long join has no fp64 route yet (sed_join_long_self serves the integer route's tables)")

    def search_f64(self, packed, max_dist, cap=None):
        raise SedError("the long join has no fp64 route yet (sed_join_long_search serves the integer route's tables)")

    def self_knn_f64(self, k, max_dist=math.inf, rows=None, cap=None):
        raise SedError("the long join has no fp64 route yet (sed_join_long_knn_self serves the integer route's tables)")

    def search_knn_f64(self, packed, k, max_dist=math.inf, cap=None):
        raise SedError("the long join has no fp64 route yet (sed_join_long_knn_search serves the integer route's tables)")

    def knn_bounds_f64(self):
        raise SedError("the long join has no fp64 route yet (sed_join_long_knn_bounds serves the integer route's calls)")


JOIN_PLAN_FIELDS = ("scale", "kernel", "waves", "scope", "run", "cells")
JOIN_KERNELS = {1: "dp", 2: "bitpar", 3: "f64"}
JOIN_ROUTES = {0: "int", 1: "f64"}  # SED_JOIN_ROUTE_*


def codes_seen(codes):
    """The mask sed_join_plan takes: bit c set when code c occurs (bit 31: any code >= 31)."""
    mask = 0
    for c in np.unique(np.asarray(codes, np.uint8)).tolist():
        mask |= 1 << min(c, 31)
    return mask


def _join_args(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist):
    return _plan_args(costs, options) + (_lengths(len_rows), len(len_rows), _lengths(len_cols), len(len_cols),
                                         int(bool(self_join)), int(row_codes), int(col_codes), float(max_dist))


def _join_plan_call(name, head, args, error=None, lane_cells=False):
    """The plan dict of one join _plan export: head = what it takes before _join_args' arguments (args), error = the
    export that holds a refusal's text (None: it has no such channel), lane_cells: it fills the seventh slot."""
    fields = JOIN_PLAN_FIELDS + (("lane_cells",) if lane_cells else ())
    out = np.zeros(len(fields), np.float64)
    rc = getattr(load(), name)(*head, *_join_args(*args), out, len(out))
    if rc != 0:
        if error is None:
            raise _fit_fail(name, rc)
        err = SedError("%s failed (%d): %s" % (name, rc, getattr(load(), error)().decode()))
        err.code = rc
        raise err
    return {f: (float(v) if f in ("scale", "cells", "lane_cells") else int(v)) for f, v in zip(fields, out)}


def join_plan(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist):
    """What JoinIndex.self_join / search would decide, without a device (sed_join_plan): {field: number} over
    JOIN_PLAN_FIELDS.  costs and options as plan_routes takes them; row_codes / col_codes from codes_seen.  Raises
    SedError carrying the SED_E_* code (.code) the join would fail with."""
    return _join_plan_call("sed_join_plan", (), (costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist))


def join_long_plan(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist):
    """What LongJoinIndex.self_join / search would decide, without a device (sed_join_long_plan): join_plan's fields for
    lengths 0..128, and "lane_cells", the cells the waves execute with their blocks of 32 columns and their spare lanes.
    Arguments and errors as join_plan; the SedError also carries the refusal's text (sed_join_long_plan_error)."""
    return _join_plan_call("sed_join_long_plan", (), (costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist),
                           "sed_join_long_plan_error", True)


def join_knn_trim(hits, k):
    """The k-nearest calls' trim alone, without a device (sed_join_knn_trim): JOIN_HIT_DTYPE records in any order -> a
    new array sorted by (row, dist, col) with each row's first k."""
    out = np.array(hits, JOIN_HIT_DTYPE)
    kept = C.c_int64()
    rc = load().sed_join_knn_trim(out.ctypes.data if len(out) else None, len(out), int(k), C.byref(kept))
    if rc != 0:
        raise _fit_fail("sed_join_knn_trim", rc)
    return out[:kept.value]


def join_decode(records, route, cap, rows, ncols, self_join, scale_log2=0, k=0, bounds=None):
    """What every join call does with the records it downloads, without a device (sed_join_decode): records = an (n, 4)
    uint32 array of (row, col, w0, w1); route = "int" (dist = w0 * 2^-scale_log2, cap = the cutoff on that scale) or
    "f64" ((w0, w1) = the double's low and high words, cap = max_dist); rows = (first, nrows) of the call.  k = 0: a
    join's hits sorted by (row, col); k >= 1: a k-nearest call's, trimmed, under bounds (one per row: integers on the
    "int" route, doubles on "f64").  Returns JOIN_HIT_DTYPE records; a record no kernel emits raises SedError (.code =
    SED_E_DEVICE, the text names it), bad arguments SedError with .code = SED_E_ARG."""
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 4)
    first, nrows = rows
    out = np.zeros(max(len(rec), 1), JOIN_HIT_DTYPE)
    kept = C.c_int64()
    why = C.create_string_buffer(256)
    b = None if bounds is None else np.ascontiguousarray(bounds, np.float64 if route == "f64" else np.uint32)
    rc = load().sed_join_decode(rec.ctypes.data if len(rec) else None, len(rec), {v: r for r, v in JOIN_ROUTES.items()}[route],
                                int(scale_log2), float(cap), int(first), int(nrows), int(ncols), int(bool(self_join)), int(k),
                                None if b is None or not len(b) else b.ctypes.data, out.ctypes.data, C.byref(kept), why, len(why))
    if rc != 0:
        err = SedError("sed_join_decode failed (%d): %s" % (rc, why.value.decode()))
        err.code = rc
        raise err
    return out[:kept.value]


def join_knn_plan(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, k, max_dist, long_index=False):
    """What JoinIndex.self_knn / search_knn (long_index: LongJoinIndex's) would decide, without a device
    (sed_join_knn_plan): k outside 1..64 raises SedError (.code = SED_E_ARG, the text names k), then join_plan's (or
    join_long_plan's) refusals; the fields are those of the join at max_dist, which bound each pass from above."""
    return _join_plan_call("sed_join_knn_plan", (int(bool(long_index)), int(k)),
                           (costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist),
                           "sed_join_knn_plan_error", bool(long_index))


def join_f64_plan(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist):
    """What JoinIndex.self_join_f64 / search_f64 would decide, without a device (sed_join_f64_plan): join_plan's fields
    with scale = 0 (fp64 has none) and kernel = 3.  Arguments and errors as join_plan."""
    return _join_plan_call("sed_join_f64_plan", (), (costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist))


def join_knn_f64_plan(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, k, max_dist):
    """What JoinIndex.self_knn_f64 / search_knn_f64 would decide, without a device (sed_join_knn_f64_plan): k outside
    1..64 raises SedError (.code = SED_E_ARG, the text names k), then join_f64_plan's refusals, with their text; the
    fields are those of the fp64 join at max_dist, which bound each pass from above."""
    return _join_plan_call("sed_join_knn_f64_plan", (int(k),),
                           (costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist),
                           "sed_join_knn_plan_error")


def join_f64_lower(ins, dele):
    """The table behind the fp64 route's length skip (sed_join_f64_lower): a 33 x 33 float64 array, [n, m] a value <=
    every distance of a row of n and a column of m symbols under these costs; join_f64_keep(ins, dele, T) is
    join_f64_lower(ins, dele) <= T."""
    low = np.zeros(33 * 33, np.float64)
    rc = load().sed_join_f64_lower(float(ins), float(dele), low)
    if rc != 0:
        raise _fit_fail("sed_join_f64_lower", rc)
    return low.reshape(33, 33)


def join_f64_keep(ins, dele, max_dist):
    """The fp64 route's length skip (sed_join_f64_keep): a 33 x 33 bool array, [n, m] true when a row of n and a column
    of m symbols are computed under these costs and cutoff."""
    keep = (C.c_uint64 * 33)()
    rc = load().sed_join_f64_keep(float(ins), float(dele), float(max_dist), keep)
    if rc != 0:
        raise _fit_fail("sed_join_f64_keep", rc)
    return np.array([[(int(keep[n]) >> m) & 1 for m in range(33)] for n in range(33)], bool)


def join_route(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist):
    """Which route serves the join join_plan's arguments describe, without a device (sed_join_route): (route, why).
    route = "int" (self_join / search serve it), "f64" (only self_join_f64 / search_f64 do; why = the integer route's
    refusal) or None (neither; why = both refusals).  Bad arguments raise SedError as join_plan does."""
    return _route_call("sed_join_route", _join_args(costs, options, len_rows, len_cols, self_join, row_codes, col_codes, max_dist),
                       JOIN_ROUTES)


def unpack_ops(ops_words, ops_off, p, length):
    """Op codes (uint8 0 ins, 1 del, 2 upd) of pair p from the packed script buffer."""
    w = ops_words[ops_off[p]: ops_off[p] + (length + 15) // 16]
    codes = (w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3
    return codes.ravel()[:length].astype(np.uint8)


class Batch:
    """Device-resident batch (sed_batch_*): upload once, run many times."""

    def __init__(self, ctx, packed, want_script, pipeline=False, no_len=False):
        self.ctx = ctx
        self._lib = ctx._lib
        self.packed = packed
        self.want_script = want_script
        flags = (SED_WANT_SCRIPT if want_script else (SED_NO_LEN if no_len else 0)) | \
            (SED_PIPELINE if pipeline else 0)
        self.ptr = self._lib.sed_batch_create(ctx.ptr, packed.codes_a, packed.off_a, packed.len_a, packed.codes_b,
                                              packed.off_b, packed.len_b, packed.npairs, flags)
        if not self.ptr:
            msg = self._lib.sed_last_error(ctx.ptr)
            raise SedError("sed_batch_create failed: %s" % (msg.decode() if msg else ""))

    def close(self):
        if self.ptr and self.ctx._pid == os.getpid():
            self._lib.sed_batch_destroy(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def mode(self):
        return MODE_NAMES.get(self._lib.sed_batch_mode(self.ptr), "?")

    @property
    def rows_per_lane(self):
        return self._lib.sed_batch_rows_per_lane(self.ptr)

    @property
    def lane_pairs(self):
        return self._lib.sed_batch_lane_pairs(self.ptr)

    @property
    def chains(self):
        return self._lib.sed_batch_chains(self.ptr)

    @property
    def dot_keys(self):
        """True when the checkpoint forward kernel runs dot keys (v_dot4 + v_max3 per cell, SED_OPT_DOT)."""
        return (self._lib.sed_batch_dot_keys(self.ptr) & 1) == 1

    @property
    def band_cells(self):
        """Cells the forward computes per run: below sum n*m when the batch is band-pruned (SED_OPT_BAND)."""
        return float(self._lib.sed_batch_band_cells(self.ptr))

    def band_chunks_run(self):
        """(chunks the forward ran, chunks of the same stripes unpruned) of the last run of a band-pruned batch, summed
        from the ranges the kernel stored per stripe; None when the batch is not band-pruned or has not run."""
        total = np.zeros(1, np.float64)
        run = float(self._lib.sed_batch_band_chunks_run(self.ptr, total))
        return None if run < 0 else (run, float(total[0]))

    @property
    def ladder_dot_keys(self):
        """True when the CHAIN kernel runs ladder keys with the update addend as one v_dot4 (SED_OPT_DOT)."""
        return (self._lib.sed_batch_dot_keys(self.ptr) & 2) == 2

    @property
    def ladder_wide(self):
        """True when those ladder dot keys run over the wide ladder (V = D*A + 16L, one jump row in 8)."""
        return (self._lib.sed_batch_dot_keys(self.ptr) & 4) == 4

    @property
    def traceback_mode(self):
        """0 distance only, 1 per-cell traceback codes, 2 checkpoints + recompute (SED_OPT_TB), 3 per-cell codes walked
        stripe-parallel, 4 SPLIT checkpoints recomputed into per-cell codes (SED_OPT_SPLITCK)."""
        return self._lib.sed_batch_traceback_mode(self.ptr)

    def chain_stats(self):
        """(pairs handed out by the dynamic-CHAIN counter, most pairs one wave computed) of the last run."""
        f, mx = C.c_int32(), C.c_int32()
        self.ctx._check(self._lib.sed_batch_chain_stats(self.ptr, C.byref(f), C.byref(mx)), "sed_batch_chain_stats")
        return f.value, mx.value

    @property
    def packed_pairs(self):
        """Pairs computed two per lane / per wave in packed 16-bit cells (distance-only batches)."""
        return self._lib.sed_batch_packed_pairs(self.ptr)

    @property
    def bitpar_pairs(self):
        """Lane pairs computed bit-parallel (unit costs, distance only; SED_OPT_BITPAR)."""
        return self._lib.sed_batch_bitpar_pairs(self.ptr)

    @property
    def scaled_pairs(self):
        """fp64 lane pairs computed as an exact integer DP of costs scaled by 2^k (dyadic tables, SED_OPT_SCALED)."""
        return self._lib.sed_batch_scaled_pairs(self.ptr)

    @property
    def segment_pairs(self):
        """fp64 wave pairs computed in 16-lane segments, four per wave (SED_OPT_SEG)."""
        return self._lib.sed_batch_segment_pairs(self.ptr)

    @property
    def split_tasks(self):
        """SPLIT batches: the (pair, stripe) workgroups of a run, 0 otherwise (SED_OPT_SPLIT)."""
        return self._lib.sed_batch_split_tasks(self.ptr)

    def set_cutoff(self, max_dist):
        """Bound the distances of the runs that follow (distance-only batches): a pair beyond max_dist comes back as
        (inf, is_int 0, len -1), the others as without a cutoff; float('inf') turns it off (sed_batch_set_cutoff)."""
        self.ctx._check(self._lib.sed_batch_set_cutoff(self.ptr, float(max_dist)), "sed_batch_set_cutoff")

    def cutoff_hits(self):
        """Pairs within the cutoff in the last run (waits for it), without downloading the distances."""
        h = C.c_int32()
        self.ctx._check(self._lib.sed_batch_cutoff_hits(self.ptr, C.byref(h)), "sed_batch_cutoff_hits")
        return h.value

    def run(self):
        self.ctx._check(self._lib.sed_batch_run(self.ptr), "sed_batch_run")

    def sync(self):
        self.ctx._check(self._lib.sed_batch_sync(self.ptr), "sed_batch_sync")

    def last_times(self):
        a, b = C.c_float(), C.c_float()
        self.ctx._check(self._lib.sed_batch_last_times(self.ptr, C.byref(a), C.byref(b)), "sed_batch_last_times")
        return a.value, b.value

    def times(self, max_runs=4096):
        """(dp_ms[], traceback_ms[]) of every run since reset_times(), from HIP events."""
        a = np.zeros(max_runs, np.float32)
        b = np.zeros(max_runs, np.float32)
        cnt = self._lib.sed_batch_times(self.ptr, a, b, max_runs)
        if cnt < 0:
            self.ctx._check(cnt, "sed_batch_times")
        return a[:cnt].astype(np.float64), b[:cnt].astype(np.float64)

    def spans(self, max_runs=4096):
        """Every run since reset_times() as intervals: array [runs, parts, 4] of {DP start, DP end, traceback start,
        traceback end} in ms from the first run's DP start (HIP events on the launching streams)."""
        P = max(1, self.dp_launches)
        out = np.zeros(max_runs * P * 4, np.float32)
        cnt = self._lib.sed_batch_spans(self.ptr, out, max_runs)
        if cnt < 0:
            self.ctx._check(cnt, "sed_batch_spans")
        return out[:cnt * P * 4].reshape(cnt, P, 4).astype(np.float64)

    def reset_times(self):
        self._lib.sed_batch_reset_times(self.ptr)

    def set_timing(self, every):
        """Timing events on every run (1), every k-th run (k), or none (0)."""
        self.ctx._check(self._lib.sed_batch_set_timing(self.ptr, int(every)), "sed_batch_set_timing")

    def work(self):
        a, b = C.c_double(), C.c_double()
        self._lib.sed_batch_work(self.ptr, C.byref(a), C.byref(b))
        return a.value, b.value

    @property
    def dp_launches(self):
        """Forward launches per run: a checkpoint batch of >= 2048 wave pairs runs in parts on as many streams
        (SED_CK_HALVES, default 2), else 1.  With parts, times() and last_times() are the mean launch over the parts
        (which overlap each other's kernels); spans() gives every part's intervals."""
        return self._lib.sed_batch_dp_launches(self.ptr)

    def device_results(self):
        vals = [C.c_uint64() for _ in range(5)]
        self._lib.sed_batch_device_results(self.ptr, *[C.byref(v) for v in vals])
        return [v.value for v in vals]

    def export(self, d_dist=0, d_len=0, d_ops=0):
        """Device-to-device copy of the results into caller memory (raw device pointers)."""
        self.ctx._check(self._lib.sed_batch_export(self.ptr, d_dist, d_len, d_ops), "sed_batch_export")

    def results(self):
        P = self.packed.npairs
        dist = np.zeros(max(P, 1), np.float64)
        is_int = np.zeros(max(P, 1), np.uint8)
        ln = np.zeros(max(P, 1), np.int32)
        ops = None
        ops_ptr = off_ptr = None
        if self.want_script:
            ops = np.zeros(max(int(self.packed.ops_off[P]), 1), np.uint32)
            ops_ptr = ops.ctypes.data_as(C.c_void_p)
            off_ptr = self.packed.ops_off.ctypes.data_as(C.c_void_p)
        self.ctx._check(self._lib.sed_batch_results(self.ptr, dist, is_int, ln, ops_ptr, off_ptr), "sed_batch_results")
        return dist[:P], is_int[:P], ln[:P], ops


class EngineClient:
    """The Context interface (set_costs, set_option, set_mode, run, full_matrix, selftest) served by an
    engine worker process: a fresh interpreter running this file, started on first use, that owns its
    own HIP context.  One request at a time over a pipe pair; the worker exits when the pipe closes."""

    def __init__(self, device=0, channel=None):
        self.device = device
        self._proc = None
        self._tx = self._rx = None
        self._cost_key = None
        self._pid = os.getpid()
        self._channel = channel  # this process's socket to its parent's engine thread (None: start a worker)
        self.served_by = None

    def _start(self):
        from multiprocessing.connection import Connection
        if self._channel is not None:  # the parent serves this child (see the module docstring)
            sock, self._channel = self._channel, None
            self._tx = self._rx = Connection(sock.detach())
            self.served_by = "parent"
            self._tx.send_bytes(pickle.dumps(("open", self.device), protocol=pickle.HIGHEST_PROTOCOL))
            status, val = pickle.loads(self._rx.recv_bytes())
            if status != "ok":
                raise SedError(val)
            return
        self.served_by = "worker"
        c2w_r, c2w_w = os.pipe()
        w2c_r, w2c_w = os.pipe()
        env = dict(os.environ)
        env["SED_ENGINE"] = "inproc"
        try:
            self._proc = subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), "--engine-worker",
                                           str(self.device), str(c2w_r), str(w2c_w)],
                                          pass_fds=(c2w_r, w2c_w), close_fds=True, env=env)
        finally:
            os.close(c2w_r)
            os.close(w2c_w)
        self._tx = Connection(c2w_w, readable=False)
        self._rx = Connection(w2c_r, writable=False)

    def _call(self, *req):
        if self._pid != os.getpid():  # a fork of a process with a client: start its own worker
            self.__init__(self.device)
        if self._tx is None:
            self._start()
        try:
            self._tx.send_bytes(pickle.dumps(req, protocol=pickle.HIGHEST_PROTOCOL))
            status, val = pickle.loads(self._rx.recv_bytes())
        except (EOFError, OSError) as ex:
            raise SedError("engine worker (pid %s) is gone: %s" % (self._proc.pid if self._proc else "?", ex))
        if status != "ok":
            raise SedError(val)
        return val

    def close(self):
        if self._tx is not None and self._pid == os.getpid():
            for f in {id(self._tx): self._tx, id(self._rx): self._rx}.values():
                try:
                    f.close()
                except OSError:
                    pass
            if self._proc is not None:
                try:
                    self._proc.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    self._proc.kill()
        self._proc = None
        self._tx = self._rx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._call("set_option", key, value)

    def set_mode(self, mode):
        self.set_option(SED_OPT_MODE, mode)
        self.invalidate_costs()

    def invalidate_costs(self):
        self._cost_key = None

    def set_costs(self, plan):
        key = plan.key()
        if key == self._cost_key:
            return
        self._call("set_costs", plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
        self._cost_key = key

    def selftest(self):
        return self._call("selftest")

    def run(self, packed, want_script, no_len=False):
        return self._call("run", packed, want_script, no_len)

    def run_pair(self, codes_a, codes_b, want_script, no_len=False):
        return self._call("run_pair", codes_a, codes_b, want_script, no_len)

    def run_cutoff(self, packed, max_dist, no_len=True):
        return self._call("run_cutoff", packed, max_dist, no_len)

    def deepen(self, packed, k, first, last, no_len=True):
        return self._call("deepen", packed, k, first, last, no_len)

    def fit(self, packed):
        return self._call("fit", packed)

    def fit_f64(self, packed):
        return self._call("fit_f64", packed)

    def full_matrix(self, codes_a, codes_b):
        return self._call("full_matrix", np.asarray(codes_a, np.uint8), np.asarray(codes_b, np.uint8))

    def fit_index(self, codes, off, lens):
        raise SedError("fit_index: a forked child's engine proxy does not serve resident indexes (its texts would live "
                       "in the serving process); use fit() here, or build the index in the process that owns the device")

    def join_index(self, codes, off, lens):
        raise SedError("join_index: a forked child's engine proxy does not serve resident indexes (its sequences would "
                       "live in the serving process); build the index in the process that owns the device")

    def join_long_index(self, codes, off, lens):
        raise SedError("join_long_index: a forked child's engine proxy does not serve resident indexes (its sequences "
                       "would live in the serving process); build the index in the process that owns the device")


class _PlanArgs:
    """The fields Context.set_costs reads from a sedcost.CostPlan."""

    def __init__(self, K, sub, sub_int, ins, ins_int, dele, del_int):
        self.K, self.sub, self.sub_int = K, sub, sub_int
        self.ins, self.ins_int, self.dele, self.del_int = ins, ins_int, dele, del_int

    def key(self):
        return (self.K, self.sub.tobytes(), self.sub_int.tobytes(), self.ins, self.ins_int, self.dele, self.del_int)


_serve_pool = []  # idle serving Contexts of this process (parent-served children): the next child reuses one
_serve_pool_lock = threading.Lock()


def _serve(rx, tx, device, pooled=False):
    """Serve EngineClient requests on one Context until the client closes its end.  pooled: the Context comes from
    and returns to _serve_pool (a parent serving its forked children: create_search_threads' second Process then
    starts without a sed_create), with the options the client set put back to their defaults."""
    ctx = None
    touched = set()
    while True:
        try:
            req = pickle.loads(rx.recv_bytes())
        except (EOFError, OSError):
            break
        try:
            op, args = req[0], req[1:]
            if op == "open":  # (a parent-served child names its device first)
                device = args[0]
            if ctx is None:
                if pooled:
                    with _serve_pool_lock:
                        for x in _serve_pool:
                            if x.device == device:
                                _serve_pool.remove(x)
                                ctx = x
                                break
                if ctx is None:
                    ctx = Context(device)
            if op == "open":
                val = None
            elif op == "set_costs":
                ctx.set_costs(_PlanArgs(*args))
                val = None
            elif op == "set_option":
                ctx.set_option(*args)
                touched.add(args[0])
                val = None
            elif op == "selftest":
                val = ctx.selftest()
            elif op == "run":
                val = ctx.run(*args)
            elif op == "run_pair":
                val = ctx.run_pair(*args)
            elif op == "run_cutoff":
                val = ctx.run_cutoff(*args)
            elif op == "deepen":
                val = ctx.deepen(*args)
            elif op == "fit":
                val = ctx.fit(*args)
            elif op == "fit_f64":
                val = ctx.fit_f64(*args)
            elif op == "full_matrix":
                val = ctx.full_matrix(*args)
            else:
                raise SedError("unknown engine request %r" % (op,))
            out = ("ok", val)
        except Exception as ex:  # reported to the client as SedError
            out = ("err", "%s: %s" % (type(ex).__name__, ex))
        try:
            tx.send_bytes(pickle.dumps(out, protocol=pickle.HIGHEST_PROTOCOL))
        except OSError:
            break
    if ctx is not None and pooled:
        try:
            for key in touched:
                ctx.set_option(key, 0)
            if touched:
                ctx.invalidate_costs()
            with _serve_pool_lock:
                if len(_serve_pool) < 2:
                    _serve_pool.append(ctx)
                    ctx = None
        except SedError:
            pass
    if ctx is not None:
        ctx.close()


def _engine_worker(device, rfd, wfd):
    """The worker process's main loop."""
    from multiprocessing.connection import Connection
    _serve(Connection(rfd, writable=False), Connection(wfd, readable=False), device)


def _serve_child(sock):
    """Thread of a HIP process serving one forked child over its socket pair."""
    from multiprocessing.connection import Connection
    conn = Connection(sock.detach())
    try:
        _serve(conn, conn, 0, pooled=True)
    finally:
        conn.close()


# fork hooks: a process holding a HIP Context gives each fork a socket pair.  The parent's ends are watched by one
# selector thread (started at the first fork); a child's first request starts a thread serving that child, and a child
# that exits without using the engine (a Manager server, a helper) only has its socket closed.  Served children depend
# on this process: when it exits, their channels close and their next engine call raises SedError.
_fork_pair = None
_child_channel = None  # (socket, pid) in a child forked from a HIP process
_sel_state = None  # parent: (selector, wake read end, wake write end, channels to register)
_sel_lock = threading.Lock()


def _watch_channel(sock):
    """Hand the parent's end of a new child's socket pair to the selector thread."""
    global _sel_state
    with _sel_lock:
        if _sel_state is None:
            import selectors
            sel = selectors.DefaultSelector()
            wr, ww = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
            wr.setblocking(False)
            sel.register(wr, selectors.EVENT_READ)
            _sel_state = (sel, wr, ww, [])
            threading.Thread(target=_channel_selector, args=(_sel_state,), daemon=True,
                             name="sed-engine-channels").start()
        _sel_state[3].append(sock)
        ww = _sel_state[2]
    ww.send(b"\0")


def _channel_selector(state):
    """The selector thread: waits on every child's channel until its first request (or its end)."""
    import selectors
    sel, wake, _, pending = state
    while True:
        for key, _ in sel.select():
            s = key.fileobj
            if s is wake:
                try:
                    wake.recv(4096)
                except BlockingIOError:
                    pass
                with _sel_lock:
                    new, pending[:] = list(pending), []
                for x in new:
                    sel.register(x, selectors.EVENT_READ)
                continue
            sel.unregister(s)
            try:
                first = s.recv(1, socket.MSG_PEEK)
            except OSError:
                first = b""
            if first:
                threading.Thread(target=_serve_child, args=(s,), daemon=True, name="sed-engine-fork").start()
            else:
                s.close()  # the child closed its end without a request


def _before_fork():
    global _fork_pair
    _fork_pair = None
    if _hip_pid == os.getpid() and os.environ.get("SED_FORK_ENGINE", "parent") == "parent":
        try:
            _fork_pair = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
        except OSError:
            _fork_pair = None


def _after_fork_in_parent():
    global _fork_pair
    pair, _fork_pair = _fork_pair, None
    if pair is not None:
        pair[1].close()
        _watch_channel(pair[0])


_ctx = None
_ctx_pid = None


def _reset_lock_in_child():
    global _lock, _fork_pair, _child_channel, _sel_state, _sel_lock
    _lock = threading.Lock()  # a fork taken while another thread held it must not deadlock the child
    _sel_lock = threading.Lock()
    st, _sel_state = _sel_state, None  # (the parent's selector thread does not exist here: drop its copies)
    if st is not None:
        for x in (st[0], st[1], st[2]):
            try:
                x.close()
            except OSError:
                pass
    if _child_channel is not None and _child_channel[1] != os.getpid():
        # a channel this process's parent got but never used: a grandchild must not hold it open
        try:
            _child_channel[0].close()
        except OSError:
            pass
    pair, _fork_pair = _fork_pair, None
    if pair is not None:
        pair[0].close()
        _child_channel = (pair[1], os.getpid())
    else:
        _child_channel = None


if hasattr(os, "register_at_fork"):
    os.register_at_fork(before=_before_fork, after_in_parent=_after_fork_in_parent, after_in_child=_reset_lock_in_child)


def context(device=None):
    """Process-wide default engine (device from SED_DEVICE / LOCAL_RANK, else 0): an in-process Context,
    or an EngineClient in a child forked after its parent initialised HIP (or with SED_ENGINE=worker)."""
    global _ctx, _ctx_pid, _child_channel
    with _lock:
        pid = os.getpid()
        if _ctx is None or _ctx_pid != pid:
            if device is None:
                device = int(os.environ.get("SED_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            mode = os.environ.get("SED_ENGINE", "auto")
            inherited = _hip_pid is not None and _hip_pid != pid
            if mode == "worker" or (inherited and mode != "inproc"):
                ch = _child_channel[0] if (_child_channel and _child_channel[1] == pid and mode != "worker") else None
                _child_channel = None  # (one client per channel)
                _ctx = EngineClient(device, ch)
            else:
                _ctx = Context(device)  # raises SedError in a fork of a HIP process (SED_ENGINE=inproc)
            _ctx_pid = pid
        return _ctx


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "--engine-worker":
    _engine_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))


def dot_factor(sub, ins, dele, maxmin=0, ladder_maxsum=0):
    """The byte factorisation behind SED_OPT_DOT (no device needed): (A, rows, cols, aux) or None.
    sub: 4 x 4 costs (row symbol -> column symbol); rows/cols: 4 x 4 signed bytes; aux = (decode shift, multiplier),
    or for the ladder keys (ladder_maxsum > 0) (sentinel byte, L unit: 16 on the wide ladder, else 8)."""
    out = np.zeros(10, np.uint32)
    A = load().sed_dot_factor(np.ascontiguousarray(sub, np.float64).ravel(), float(ins), float(dele), int(maxmin),
                              int(ladder_maxsum), out)
    if A < 0:
        raise SedError("sed_dot_factor: bad arguments")
    if A == 0:
        return None
    to_bytes = lambda w: np.frombuffer(np.asarray(w, np.uint32).tobytes(), np.int8).reshape(4, 4).astype(np.int64)
    return A, to_bytes(out[0:4]), to_bytes(out[4:8]), (int(out[8]), int(out[9]))


PLAN_ROUTE_FIELDS = ("mode", "rows_per_lane", "lane_pairs", "chains", "traceback_mode", "dot_keys", "bitpar_pairs",
                     "segment_pairs", "split_tasks", "scaled_pairs", "packed_pairs", "dp_launches", "band_cells", "cells",
                     "algo_bytes")


def plan_routes(costs, options, packed, flags):
    """The planner without a device (sed_plan_routes): what a Batch of `packed` created under these costs and options
    would report, as {field: number} over PLAN_ROUTE_FIELDS (counts as ints).  costs = (K, sub, sub_int, ins, ins_int,
    dele, del_int) as sed_set_costs takes them; options = {SED_OPT_* or SED_PLAN_ENV_*: value}.  Raises SedError
    carrying the SED_E_* code (.code) batch creation would fail with."""
    K, sub, sub_int, ins, ins_int, dele, del_int = costs
    opts = np.array([x for kv in options.items() for x in kv] or [0, 0], np.int32)
    out = np.zeros(len(PLAN_ROUTE_FIELDS), np.float64)
    rc = load().sed_plan_routes(int(K), np.ascontiguousarray(sub, np.float64).ravel(),
                                np.ascontiguousarray(sub_int, np.uint8).ravel(), float(ins), int(ins_int), float(dele),
                                int(del_int), opts, len(options), packed.codes_a, packed.off_a, packed.len_a,
                                packed.codes_b, packed.off_b, packed.len_b, packed.npairs, flags, out, len(out))
    if rc != 0:
        err = SedError("sed_plan_routes failed (%d)" % rc)
        err.code = rc
        raise err
    return {k: (float(v) if k in ("band_cells", "cells", "algo_bytes") else int(v))
            for k, v in zip(PLAN_ROUTE_FIELDS, out)}


STEP_LAUNCHERS = ("win", "x2", "chain", "i32", "codes", "f64", "f64_seg", "lane", "filter", "tb_ck", "tb_codes",
                  "tb_stripes", "tb_seg")
STEP_PHASES = ("dp", "tb")
STEP_STREAMS = ("dp", "tb", "part")
Step = collections.namedtuple("Step", "launcher phase stream part start end")


class Schedule(list):
    """The Steps of one run, with need_ev (untimed runs record events too), reuse_wait (None, "dp_end" or "tb_end": what
    a rotating buffer's next user waits for), parts and capacity (the most steps a schedule holds)."""


def plan_schedule(costs, options, packed, flags, cut_on=False, cut_win=False):
    """The launches of one run, without a device (sed_plan_schedule): the Schedule a Batch of `packed` created under
    these costs and options (as plan_routes takes them) executes per run in the cutoff state (cut_on, cut_win).  Raises
    SedError carrying the SED_E_* code (.code): batch creation's, or SED_E_ARG for a cutoff state the batch cannot be
    in."""
    K, sub, sub_int, ins, ins_int, dele, del_int = costs
    opts = np.array([x for kv in options.items() for x in kv] or [0, 0], np.int32)
    rows, info = np.zeros((64, 6), np.int32), np.zeros(4, np.int32)
    n = load().sed_plan_schedule(int(K), np.ascontiguousarray(sub, np.float64).ravel(),
                                 np.ascontiguousarray(sub_int, np.uint8).ravel(), float(ins), int(ins_int), float(dele),
                                 int(del_int), opts, len(options), packed.codes_a, packed.off_a, packed.len_a,
                                 packed.codes_b, packed.off_b, packed.len_b, packed.npairs, flags, int(bool(cut_on)),
                                 int(bool(cut_win)), rows, len(rows), info)
    if n < 0:
        err = SedError("sed_plan_schedule failed (%d)" % n)
        err.code = n
        raise err
    s = Schedule(Step(STEP_LAUNCHERS[k], STEP_PHASES[ph], STEP_STREAMS[on], int(part), bool(a), bool(z))
                 for k, ph, on, part, a, z in rows[:n].tolist())
    s.need_ev, s.reuse_wait = bool(info[0]), {0: None, 1: "dp_end", 3: "tb_end"}[int(info[1])]
    s.parts, s.capacity = int(info[2]), int(info[3])
    return s


FIT_PLAN_FIELDS = ("scale", "W", "chunk", "lanes", "cells", "nominal_cells")
FIT_F64_PLAN_FIELDS = FIT_PLAN_FIELDS + ("one_lane",)
FIT_LANE_FIELDS = ("tw", "pair", "pat", "plen", "nsteps", "lead", "cnt", "c0")
FIT_ROUTES = {0: "int", 1: "f64"}


def _plan_args(costs, options):
    """The cost model and the options as every device-free export takes them."""
    K, sub, sub_int, ins, ins_int, dele, del_int = costs
    opts = np.array([x for kv in options.items() for x in kv] or [0, 0], np.int32)
    return (int(K), np.ascontiguousarray(sub, np.float64).ravel(), np.ascontiguousarray(sub_int, np.uint8).ravel(),
            float(ins), int(ins_int), float(dele), int(del_int), opts, len(options))


def _lengths(lens):
    return np.ascontiguousarray(lens if len(lens) else [0], np.int32)


def _fit_pair_args(costs, options, len_p, len_t):
    return _plan_args(costs, options) + (_lengths(len_p), _lengths(len_t), len(len_p))


def _fit_index_args(costs, options, len_p, len_t):
    return _plan_args(costs, options) + (_lengths(len_p), len(len_p), _lengths(len_t), len(len_t))


def _fit_fail(name, rc):
    err = SedError("%s failed (%d)" % (name, rc))
    err.code = rc
    return err


def _fit_plan_call(name, args, fields=FIT_PLAN_FIELDS, nrows=None):
    """The plan dict of one _plan export over `fields`; nrows = the queries of a long plan, which adds "rows"."""
    out = np.zeros(len(fields), np.float64)
    rows = () if nrows is None else (np.zeros(max(nrows, 1), np.int32),)
    rc = getattr(load(), name)(*args, out, len(out), *rows)
    if rc != 0:
        raise _fit_fail(name, rc)
    plan = {k: (float(v) if k in ("scale", "cells", "nominal_cells") else int(v)) for k, v in zip(fields, out)}
    if rows:
        plan["rows"] = rows[0][:nrows]
    return plan


def _fit_lanes_call(name, args, nl, params):
    """The lane dict of one _lanes export of nl records; params: the integer routes' (lanes, params), else lanes alone."""
    rec = np.zeros((max(nl, 1), len(FIT_LANE_FIELDS)), np.int32)
    par = (np.zeros(18, np.uint32),) if params else ()
    rc = getattr(load(), name)(*args, rec.ravel(), nl, *par)
    if rc != 0:
        raise _fit_fail(name, rc)
    lanes = {k: rec[:nl, i].astype(np.int64) for i, k in enumerate(FIT_LANE_FIELDS)}
    lanes["tw"] &= 0xFFFFFFFF
    if not params:
        return lanes
    return lanes, {"row": par[0][:16].reshape(8, 2).copy(), "ins": int(par[0][16]), "del": int(par[0][17])}


def _route_call(name, args, routes):
    """(route, why) of one _route export: a name of `routes`, or None when the refusal is both routes'."""
    why = C.create_string_buffer(1024)
    rc = getattr(load(), name)(*args, why, len(why))
    text = why.value.decode()
    if rc in routes:
        return routes[rc], text
    if rc == SED_E_RANGE:
        return None, text
    raise _fit_fail(name, rc)


def fit_plan(costs, options, len_p, len_t):
    """What Context.fit would decide, without a device (sed_fit_plan): {field: number} over FIT_PLAN_FIELDS.  costs and
    options as plan_routes takes them; len_p / len_t = the pairs' pattern and text lengths.  Raises SedError carrying
    the SED_E_* code (.code) the search would fail with."""
    return _fit_plan_call("sed_fit_plan", _fit_pair_args(costs, options, len_p, len_t))


def fit_cutoff_scaled(costs, options, len_p, len_t, max_dist):
    """The cutoff FitIndex.hits hands its kernel, without a device (sed_fit_cutoff_scaled): min(floor(max_dist * S),
    65535) under the scale S of fit_plan's plan for the same arguments.  Raises SedError carrying the code (.code):
    fit_plan's for these arguments, else SED_E_ARG for a NaN or negative max_dist."""
    out = C.c_int64(0)
    rc = load().sed_fit_cutoff_scaled(*_fit_pair_args(costs, options, len_p, len_t), float(max_dist), C.byref(out))
    if rc != 0:
        raise _fit_fail("sed_fit_cutoff_scaled", rc)
    return int(out.value)


def fit_lanes(costs, options, len_p, len_t):
    """The lane records Context.fit would run, without a device (sed_fit_lanes): (lanes, params).  lanes = {field:
    int64[nlanes]} over FIT_LANE_FIELDS, tw in 4-symbol words from the pair's own text start; params = {"row":
    u32[8][2] update addend bytes, "ins", "del": the scaled insert and delete}.  Arguments and errors as fit_plan."""
    nl = fit_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_lanes", _fit_pair_args(costs, options, len_p, len_t), nl, True)


def fit_f64_plan(costs, options, len_p, len_t):
    """What Context.fit_f64 would decide, without a device (sed_fit_f64_plan): fit_plan's fields with scale = 0 (fp64)
    and "one_lane": 0, or why every text runs as one lane (1 insert = 0, 2 the window argument's conditions fail).
    Arguments and errors as fit_plan."""
    return _fit_plan_call("sed_fit_f64_plan", _fit_pair_args(costs, options, len_p, len_t), FIT_F64_PLAN_FIELDS)


def fit_f64_lanes(costs, options, len_p, len_t):
    """The lane records Context.fit_f64 would run, without a device (sed_fit_f64_lanes): {field: int64[nlanes]} over
    FIT_LANE_FIELDS, as fit_lanes' first result."""
    nl = fit_f64_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_f64_lanes", _fit_pair_args(costs, options, len_p, len_t), nl, False)


def fit_index_f64_plan(costs, options, len_p, len_t):
    """What FitIndex.search_f64 would decide, without a device (sed_fit_index_f64_plan): fit_f64_plan's fields for the
    queries x texts cross product."""
    return _fit_plan_call("sed_fit_index_f64_plan", _fit_index_args(costs, options, len_p, len_t), FIT_F64_PLAN_FIELDS)


def fit_index_f64_lanes(costs, options, len_p, len_t):
    """The lane records FitIndex.search_f64 / hits_f64 would run, without a device (sed_fit_index_f64_lanes), query-major,
    pair = query * len(len_t) + text."""
    nl = fit_index_f64_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_index_f64_lanes", _fit_index_args(costs, options, len_p, len_t), nl, False)


def fit_route(costs, options, len_p, len_t):
    """Which route serves the search fit_plan's arguments describe, without a device (sed_fit_route): (route, why).
    route = "int" (Context.fit serves it), "f64" (only Context.fit_f64 does; why = the integer route's refusal) or
    None (neither; why = both refusals).  Bad arguments raise SedError as fit_plan does."""
    return _route_call("sed_fit_route", _fit_pair_args(costs, options, len_p, len_t), FIT_ROUTES)


def fit_index_plan(costs, options, len_p, len_t):
    """What FitIndex.search would decide for queries of lengths len_p against texts of lengths len_t, without a device
    (sed_fit_index_plan): fit_plan's fields for the queries x texts cross product.  Errors as fit_plan."""
    return _fit_plan_call("sed_fit_index_plan", _fit_index_args(costs, options, len_p, len_t))


def fit_index_lanes(costs, options, len_p, len_t):
    """The lane records FitIndex.search would run, without a device (sed_fit_index_lanes): (lanes, params) as fit_lanes
    returns them, query-major, pair = query * len(len_t) + text."""
    nl = fit_index_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_index_lanes", _fit_index_args(costs, options, len_p, len_t), nl, True)


def fit_index_long_plan(costs, options, len_p, len_t):
    """What FitIndex.search_long would decide, without a device (sed_fit_index_long_plan): fit_index_plan's fields
    (lanes = the waves) and "rows": int32[queries], the pattern rows per lane each query runs with.  Errors as
    fit_plan."""
    return _fit_plan_call("sed_fit_index_long_plan", _fit_index_args(costs, options, len_p, len_t), nrows=len(len_p))


def fit_index_long_lanes(costs, options, len_p, len_t):
    """The wave records FitIndex.search_long would run, without a device (sed_fit_index_long_lanes): (lanes, params) as
    fit_index_lanes returns them, one record per (query, chunk record), query-major."""
    nl = fit_index_long_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_index_long_lanes", _fit_index_args(costs, options, len_p, len_t), nl, True)


def fit_index_long_f64_plan(costs, options, len_p, len_t):
    """What FitIndex.search_long_f64 would decide, without a device (sed_fit_index_long_f64_plan): fit_index_f64_plan's
    fields (lanes = the waves) and "rows": int32[queries], as fit_index_long_plan."""
    return _fit_plan_call("sed_fit_index_long_f64_plan", _fit_index_args(costs, options, len_p, len_t), FIT_F64_PLAN_FIELDS,
                          nrows=len(len_p))


def fit_index_long_f64_lanes(costs, options, len_p, len_t):
    """The wave records FitIndex.search_long_f64 / hits_long_f64 would run, without a device
    (sed_fit_index_long_f64_lanes): as fit_index_f64_lanes, one record per (query, chunk record), query-major."""
    nl = fit_index_long_f64_plan(costs, options, len_p, len_t)["lanes"]
    return _fit_lanes_call("sed_fit_index_long_f64_lanes", _fit_index_args(costs, options, len_p, len_t), nl, False)


def fit_long_route(costs, options, len_p, len_t):
    """fit_route for the long calls, over fit_index_long_plan's arguments (sed_fit_long_route): (route, why).  route =
    "int" whenever FitIndex.search_long serves the search, "f64" when only search_long_f64 does (why = the integer
    route's refusal), None when neither does (why = both refusals)."""
    return _route_call("sed_fit_long_route", _fit_index_args(costs, options, len_p, len_t), FIT_ROUTES)


def band_bounds(n, m, ins, dele, ub):
    """Band pruning (SED_OPT_BAND, no device needed): (e_lo, e_hi), the diagonals e = j - i an optimal path of an
    n x m pair can touch when some path costs ub."""
    out = np.zeros(2, np.int32)
    if load().sed_band_bounds(int(n), int(m), float(ins), float(dele), float(ub), out) != 0:
        raise SedError("sed_band_bounds: bad arguments")
    return int(out[0]), int(out[1])


def band_chunk_range(n, m, rows_per_lane, e_lo, e_hi, stripe):
    """(c_lo, c_hi, nchunks): the 64-step chunks stripe `stripe` of an n x m pair runs for the window (e_lo, e_hi)."""
    out = np.zeros(3, np.int32)
    if load().sed_band_chunk_range(int(n), int(m), int(rows_per_lane), int(e_lo), int(e_hi), int(stripe), out) != 0:
        raise SedError("sed_band_chunk_range: bad arguments")
    return int(out[0]), int(out[1]), int(out[2])


def band_refine_row(n, m, rows_per_lane, ins, dele, stripe, ub_prev, suf, drow, clo_prev, chi_prev):
    """One stripe's refined chunk range from the row above it, as the forward kernel computes it (sed.h:
    sed_band_refine_row): (clo, chi, the new upper bound, whether a cell survived).  suf = None where the stripe
    boundary lies past the diagonal's end."""
    out = np.zeros(4, np.int32)
    row = np.ascontiguousarray(drow, np.int32)
    if len(row) != m + 1:
        raise SedError("band_refine_row: drow must hold m + 1 values")
    if load().sed_band_refine_row(int(n), int(m), int(rows_per_lane), float(ins), float(dele), int(stripe), float(ub_prev),
                                  -1.0 if suf is None else float(suf), row, int(clo_prev), int(chi_prev), out) != 0:
        raise SedError("sed_band_refine_row: bad arguments")
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def band_cells(sub, ins, dele, codes_a, codes_b, rows_per_lane=16):
    """Cells the pruned forward computes for one pair of codes 0..3 under the 4 x 4 table sub, with the plain
    diagonal's cost as the bound."""
    a, b = np.ascontiguousarray(codes_a, np.uint8), np.ascontiguousarray(codes_b, np.uint8)
    r = load().sed_band_cells(np.ascontiguousarray(sub, np.float64).ravel(), float(ins), float(dele), a, len(a), b, len(b),
                              int(rows_per_lane))
    if r < 0:
        raise SedError("sed_band_cells: bad arguments")
    return float(r)
