"""The decisions of level 1 of the batched HNSW build on the device (reindexer_amd/csrc/hnsw_build_plan.h), compiled for the host
(tests/cpp/hnsw_build_upper_plan_cpu.cc) and pinned on the CPU: when a batch's level 1 goes to the device, how RXGPU_HNSW_BUILD_UPPER is
read, the size of the dense level-1 view and the scratch of the step.  Every expectation is a restatement of the rule written here; the
header's own output is never read as its expectation."""
import ctypes as C
from pathlib import Path

import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_build_upper_plan_cpu.so"
P, U32, U64, I32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
DEVICE, HOST_DELETED, HOST_M, HOST_EFC, HOST_SHARDED = range(5)   # HnswBuildPath


@pytest.fixture(scope="module")
def lib():
    from reindexer_amd import build
    build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    for name, res, args in [
        ("hnsw_build_upper_plan_variable", I32, []), ("hnsw_build_upper_plan_on_device", I32, [I32, I32, I32, U64]),
        ("hnsw_build_upper_plan_view_bytes", U64, [U64, U32]), ("hnsw_build_upper_plan_scratch", None, [U64, U32, U32, U32, U64, P]),
    ]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def test_the_variable_is_read_per_call(lib, monkeypatch):
    monkeypatch.delenv("RXGPU_HNSW_BUILD_UPPER", raising=False)
    assert lib.hnsw_build_upper_plan_variable() == 0                      # unset means host
    for value, want in [("device", 1), ("host", 0), ("", 0), ("Device", 0), ("device ", 0), ("1", 0), ("devices", 0)]:
        monkeypatch.setenv("RXGPU_HNSW_BUILD_UPPER", value)
        assert lib.hnsw_build_upper_plan_variable() == want, value         # read again: the value set a line ago holds
    monkeypatch.delenv("RXGPU_HNSW_BUILD_UPPER")
    assert lib.hnsw_build_upper_plan_variable() == 0


def test_device_or_host(lib):
    on = lib.hnsw_build_upper_plan_on_device
    assert on(1, DEVICE, 1, 1) == 1 and on(1, DEVICE, 5, 900) == 1
    assert on(0, DEVICE, 1, 1) == 0                                       # the variable says host
    for path in (HOST_DELETED, HOST_M, HOST_EFC, HOST_SHARDED):           # level 0 of the batch stays on the host: so does level 1
        assert on(1, path, 3, 10) == 0
    assert on(1, DEVICE, 0, 10) == 0 and on(1, DEVICE, -1, 10) == 0       # no level-1 node in front of the batch to start from
    assert on(1, DEVICE, 2, 0) == 0                                       # no row of level >= 1 in the batch
    # the top level only grows: once a batch of a flush is taken, every later batch with a row of level >= 1 is
    tops = [0, 0, 1, 1, 2, 2, 3]
    taken = [on(1, DEVICE, t, 4) for t in tops]
    assert taken == sorted(taken)


def test_view_bytes(lib):
    assert lib.hnsw_build_upper_plan_view_bytes(1_000_000, 16) == 68 * 1_000_000      # 68 B a node at M = 16: 2.2 % of a 768-float row
    assert 68 / (768 * 4) < 0.0222
    assert lib.hnsw_build_upper_plan_view_bytes(0, 16) == 0 and lib.hnsw_build_upper_plan_view_bytes(7, 64) == 7 * 65 * 4
    assert lib.hnsw_build_upper_plan_view_bytes(1 << 32, 64) == (1 << 32) * 260       # no 32-bit wrap


@pytest.mark.parametrize("up_rows,M,k,dim,cap", [(1, 4, 8, 50, 1000), (47, 4, 40, 48, 3000), (1024, 16, 200, 768, 1_000_000), (65536, 64, 256, 1024, 5_000_000)])
def test_scratch_layout(lib, up_rows, M, k, dim, cap):
    out = (U64 * 20)()
    lib.hnsw_build_upper_plan_scratch(up_rows, M, k, dim, cap, out)
    (pairs, o_cd, o_cr, o_q, o_pt, o_inc, o_t, o_tc, o_ts, over_cap, big_cap, o_over, o_bi, o_bd, o_bp, o_cnt, bytes0, node_bytes, o_ids, total) = out
    # the batch scratch of up_rows rows whose lists hold M entries (max_m0 = M), queries always packed
    assert pairs == up_rows * M
    assert over_cap == pairs // (256 - M) + 1 and big_cap == pairs + over_cap * M
    sizes = [up_rows * k * 4, up_rows * k * 4, up_rows * dim * 4, pairs * 4, pairs * 4, pairs * 4, pairs * 4, pairs * 4, over_cap * 8, big_cap * 4,
             big_cap * 4, big_cap * 4, 32]
    offs = [o_cd, o_cr, o_q, o_pt, o_inc, o_t, o_tc, o_ts, o_over, o_bi, o_bd, o_bp, o_cnt]
    at = 0
    for o, size in zip(offs, sizes):
        assert o == at and o % 256 == 0, (o, at)
        at = (at + size + 255) // 256 * 256
    assert bytes0 == at and node_bytes == cap * 8
    # the ids of U behind it
    assert o_ids == bytes0 and o_ids % 256 == 0
    assert total == (o_ids + up_rows * 4 + 255) // 256 * 256 and total % 256 == 0
    assert total < 1 << 40
