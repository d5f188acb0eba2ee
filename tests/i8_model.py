"""The CPU model of the int8 shadow tier (tests/cpp/knn_i8_quant_cpu.cc: reindexer_amd/csrc/knn_i8_quant.h compiled for the host) through
ctypes, shared by tests/test_knn_i8_quant.py (the arithmetic against float64) and tests/test_gpu_pruned_internals.py (the device against
the model)."""
import ctypes as C
from pathlib import Path

import numpy as np

LIB = Path(__file__).resolve().parent / "cpp" / "libknn_i8_quant_cpu.so"
F, I8, I32, U32, U64 = C.c_float, C.c_int8, C.c_int32, C.c_uint32, C.c_uint64
PF, PI8, PI32 = C.POINTER(F), C.POINTER(I8), C.POINTER(I32)
L2, IP, COS = 0, 1, 2


def load():
    assert LIB.exists(), f"{LIB} is missing: run `python -m reindexer_amd.build`"
    so = C.CDLL(str(LIB))
    so.i8_cpu_quantize_row.argtypes = [PF, U32, PI8, PF, PF]
    so.i8_cpu_quantize_rows.argtypes = [PF, U64, U32, PI8, PF, PF]
    so.i8_cpu_quantize_query.argtypes = [PF, U32, PI8, PI8, PI32, PF]
    so.i8_cpu_dot.argtypes = [PI8, PI8, PI8, U32, C.POINTER(C.c_int)]
    so.i8_cpu_dot.restype = I32
    so.i8_cpu_bounds_many.argtypes = [C.c_int, U64, PF, PF, PI32, PF, PF, PF, PF, PF]
    so.i8_cpu_margin.argtypes = [C.c_int, F, U32, F, F, F, F, F, F, PF]
    so.i8_cpu_f32_margin.argtypes = [C.c_int, C.c_int, F, U32, F, F]
    so.i8_cpu_f32_margin.restype = F
    so.i8_cpu_ld.argtypes = [U32]
    so.i8_cpu_ld.restype = U32
    so.i8_cpu_dim_supported.argtypes = [U32]
    return so


def _p(a, t):
    return a.ctypes.data_as(t)


def quantize_rows(lib, rows):
    rows = np.ascontiguousarray(rows, np.float32)
    n, d = rows.shape
    ld8 = lib.i8_cpu_ld(d)
    codes = np.zeros((n, ld8), np.int8)
    scale, resid = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib.i8_cpu_quantize_rows(_p(rows, PF), n, d, _p(codes, PI8), _p(scale, PF), _p(resid, PF))
    return codes, scale, resid


def quantize_queries(lib, queries):
    n, d = queries.shape
    ld8 = lib.i8_cpu_ld(d)
    h, l, t = np.zeros((n, ld8), np.int8), np.zeros((n, ld8), np.int8), np.zeros((n, ld8), np.int32)
    info = np.zeros((n, 4), np.float32)
    for q in range(n):
        row = np.ascontiguousarray(queries[q])
        lib.i8_cpu_quantize_query(_p(row, PF), d, _p(h[q], PI8), _p(l[q], PI8), _p(t[q], PI32), _p(info[q], PF))
    return h, l, t, info
