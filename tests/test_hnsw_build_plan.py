"""The decisions of the batched HNSW build on the device (reindexer_amd/csrc/hnsw_build_plan.h), compiled for the host
(tests/cpp/hnsw_build_plan_cpu.cc) and pinned on the CPU: the batch schedule and its environment hooks, which builds take the device path,
what the selection kernel keeps in LDS, and the scratch layout of the pair grouping.  Every expectation is a restatement of the rule written
here; the header's own output is never read as its expectation."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_build_plan_cpu.so"
P, U32, U64, I32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
HOOKS = ("RXGPU_HNSW_BUILD_SEED", "RXGPU_HNSW_BUILD_RATIO", "RXGPU_HNSW_BUILD_BATCH")


@pytest.fixture(scope="module")
def lib():
    from reindexer_amd import build
    build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    for name, res, args in [
        ("hnsw_build_plan_knobs", None, [P]), ("hnsw_build_plan_seed_rows", U64, [U64, U64]), ("hnsw_build_plan_batch_rows", U64, [U64, U64]),
        ("hnsw_build_plan_path", I32, [U64, U32, U32, I32]), ("hnsw_build_plan_lds", None, [U32, U32, P]),
        ("hnsw_build_plan_scratch", None, [U64, U32, U32, U32, U32, I32, U64, P]),
    ]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture()
def env(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    return monkeypatch


def schedule(lib, n):
    """(seed rows, [batch sizes]) of a build from empty, as the Map drives the header."""
    seed = lib.hnsw_build_plan_seed_rows(0, n)
    a, out = seed, []
    while True:
        b = lib.hnsw_build_plan_batch_rows(a, n)
        if b == 0:
            return seed, out
        out.append(b)
        a += b


def test_default_schedule(lib, env):
    knobs = (U64 * 3)()
    lib.hnsw_build_plan_knobs(knobs)
    assert list(knobs) == [1024, 16, 16384]
    # n below the seed: everything goes through the sequential builder, no batch
    assert schedule(lib, 0) == (0, []) and schedule(lib, 1) == (1, []) and schedule(lib, 1024) == (1024, [])
    # the first batch is the floor of 64, a last batch is cut short
    assert schedule(lib, 1025) == (1024, [1]) and schedule(lib, 1100) == (1024, [64, 12])
    seed, batches = schedule(lib, 1_000_000)
    a = seed
    for b in batches[:-1]:
        assert b == min(max(a // 16, 64), 16384)
        a += b
    assert a + batches[-1] == 1_000_000 and 0 < batches[-1] <= min(max(a // 16, 64), 16384)
    assert max(batches) == 16384                              # the cap is reached (at a = 262144) and holds from there on
    # resuming: rows linked past the seed take no seed rows; a graph that is further than n has nothing to do
    assert lib.hnsw_build_plan_seed_rows(5000, 9000) == 0 and lib.hnsw_build_plan_seed_rows(100, 600) == 500
    assert lib.hnsw_build_plan_batch_rows(9000, 9000) == 0 and lib.hnsw_build_plan_batch_rows(9001, 9000) == 0


def test_schedule_follows_the_environment(lib, env):
    env.setenv("RXGPU_HNSW_BUILD_SEED", "64")
    env.setenv("RXGPU_HNSW_BUILD_RATIO", "2")
    env.setenv("RXGPU_HNSW_BUILD_BATCH", "300")
    seed, batches = schedule(lib, 1000)
    assert seed == 64 and batches == [64, 64, 96, 144, 216, 300, 52]   # a / 2 with the floor of 64, then the cap, then what is left
    env.setenv("RXGPU_HNSW_BUILD_SEED", "0")      # zero or junk: the default stays
    env.setenv("RXGPU_HNSW_BUILD_RATIO", "x3")
    env.setenv("RXGPU_HNSW_BUILD_BATCH", "")
    knobs = (U64 * 3)()
    lib.hnsw_build_plan_knobs(knobs)
    assert list(knobs) == [1024, 16, 16384]


def test_eligibility(lib):
    assert lib.hnsw_build_plan_path(0, 16, 200, 0) == 0 and lib.hnsw_build_plan_path(0, 64, 256, 0) == 0
    assert lib.hnsw_build_plan_path(1, 16, 200, 0) == 1       # a deleted node: its slot would be recycled
    assert lib.hnsw_build_plan_path(0, 65, 200, 0) == 2
    assert lib.hnsw_build_plan_path(0, 16, 257, 0) == 3
    assert lib.hnsw_build_plan_path(0, 16, 200, 1) == 4       # a Map over a device list
    assert lib.hnsw_build_plan_path(0, 0, 200, 0) == 2 and lib.hnsw_build_plan_path(0, 16, 0, 0) == 3


FIXED = (3 * 256 + 4 * 128) * 4   # candidate ids / distances / order; kept and heap ids / distances


@pytest.mark.parametrize("dim,M,kept", [(48, 12, True), (768, 16, True), (1536, 16, False), (768, 64, False), (50, 4, True)])
def test_lds_decision(lib, dim, M, kept):
    stride = (dim + 3) // 4 * 4
    out = (U32 * 3)()
    lib.hnsw_build_plan_lds(stride, M, out)
    rows = (M + 1) * stride * 4
    assert (FIXED + rows <= 64 * 1024) == kept                # the rule: the new row and M kept rows beside the fixed arrays, within 64 KB
    assert list(out) == [FIXED, rows if kept else 0, int(kept)]


@pytest.mark.parametrize("rows,M,k,dim,pack", [(64, 4, 8, 50, 1), (16384, 16, 200, 768, 0), (1, 64, 1, 3, 1), (1000, 12, 100, 48, 0)])
def test_scratch_areas_do_not_overlap_and_hold_the_worst_case(lib, rows, M, k, dim, pack):
    out = (U64 * 18)()
    nodes_cap = 12345
    lib.hnsw_build_plan_scratch(rows, M, 2 * M, k, dim, pack, nodes_cap, out)
    (pairs, o_cd, o_cr, o_q, o_pt, o_inc, o_touched, o_tcnt, o_tseg, over_cap, big_cap, o_over, o_bid, o_bdist, o_bpos, o_cnt, total, node_bytes) = list(out)
    assert pairs == rows * M and node_bytes == nodes_cap * 8
    # a node past the cap of 256 entries holds more than 256 - maxM0 incoming rows; all of them together hold at most `pairs`
    assert over_cap >= pairs // (256 - 2 * M + 1) + (1 if pairs else 0) and big_cap >= pairs + over_cap * 2 * M
    areas = [(o_cd, rows * k * 4), (o_cr, rows * k * 4), (o_q, rows * dim * 4 if pack else 0), (o_pt, pairs * 4), (o_inc, pairs * 4), (o_touched, pairs * 4),
             (o_tcnt, pairs * 4), (o_tseg, pairs * 4), (o_over, over_cap * 8), (o_bid, big_cap * 4), (o_bdist, big_cap * 4), (o_bpos, big_cap * 4), (o_cnt, 32)]
    end = 0
    for off, size in areas:
        assert off % 256 == 0 and off >= end, (off, end)
        end = off + size
    assert total >= end
