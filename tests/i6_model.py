"""The CPU model of the 6-bit shadow (tests/cpp/knn_i6_quant_cpu.cc: reindexer_amd/csrc/knn_i6_quant.h compiled for the host) through ctypes,
shared by tests/test_knn_i6_quant.py and tests/test_gpu_scan_i6.py.  Everything behind the integer sum is the int8 tier's model (i8_model)."""
import ctypes as C
from pathlib import Path

import numpy as np

from .i8_model import PF, PI8, _p

LIB = Path(__file__).resolve().parent / "cpp" / "libknn_i6_quant_cpu.so"
PU8 = C.POINTER(C.c_uint8)
BIAS, CODE_MAX = 32, 31


def load():
    assert LIB.exists(), f"{LIB} is missing: run `python -m reindexer_amd.build`"
    so = C.CDLL(str(LIB))
    so.i6_cpu_ld.argtypes = [C.c_uint32]
    so.i6_cpu_ld.restype = C.c_uint32
    so.i6_cpu_shadow_bytes.argtypes = [C.c_uint64, C.c_uint32]
    so.i6_cpu_shadow_bytes.restype = C.c_uint64
    so.i6_cpu_quantize_rows.argtypes = [PF, C.c_uint64, C.c_uint32, PU8, PF, PF]
    so.i6_cpu_pack.argtypes = [PU8, C.c_uint64, C.c_uint32, PU8]
    so.i6_cpu_unpack.argtypes = [PU8, C.c_uint64, C.c_uint32, PU8]
    so.i6_cpu_sum.argtypes = [PI8, PI8, PU8, C.c_uint64, C.c_uint32, C.POINTER(C.c_int)]
    so.i6_cpu_sum.restype = C.c_int32
    return so


def quantize_rows(lib, rows):
    """-> (u [n][ld6] uint8 with a zero pad, s_r, e_r) as knn_i6_build forms them"""
    rows = np.ascontiguousarray(rows, np.float32)
    n, d = rows.shape
    u = np.zeros((n, lib.i6_cpu_ld(d)), np.uint8)
    scale, resid = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib.i6_cpu_quantize_rows(_p(rows, PF), n, d, _p(u, PU8), _p(scale, PF), _p(resid, PF))
    return u, scale, resid


def pack(lib, u):
    u = np.ascontiguousarray(u, np.uint8)
    n, ld6 = u.shape
    shadow = np.full(lib.i6_cpu_shadow_bytes(n, ld6), 0xAA, np.uint8)
    lib.i6_cpu_pack(_p(u, PU8), n, ld6, _p(shadow, PU8))
    return shadow


def unpack(lib, shadow, n, ld6):
    u = np.zeros((n, ld6), np.uint8)
    lib.i6_cpu_unpack(_p(shadow, PU8), n, ld6, _p(u, PU8))
    return u
