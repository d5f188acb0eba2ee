"""The launch policy of an HNSW search (reindexer_amd/csrc/hnsw_launch_plan.h: plan_hnsw_search, read_hnsw_knobs), compiled for the host
(tests/cpp/hnsw_launch_plan_cpu.cc) and pinned on the CPU: what a call of a given shape stages, splits, zeroes and launches, and what every
RXGPU_HNSW_* hook does to that.  The expected values are those of the rules as they stood inside hnsw_search_impl before the plan was
split out of it."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_launch_plan_cpu.so"

# the order in which hnsw_plan_cpu writes the plan
FIELDS = ["big_ef", "words", "max_slots", "vis_hash_log2", "vis_lds_log2", "vis_words", "vis_slots", "first_zero_bytes", "split_upload", "split_parts",
          "part_q", "o_qcorr", "o_qnorm", "staged", "zero_copy", "st_corr", "st_norm", "st_count", "st_dist", "st_row", "st_end", "prefetch_links", "team",
          "team_max", "nbl", "spec", "lds_cand_cap", "ef_cap", "use_sorted", "sorted_mode", "sorted_restart_cap", "helper_wanted", "tier_cap0", "tier_cap1",
          "force_global_tiers"]
HOOKS = ["VISITED", "VISITED_LOG2", "VISITED_LDS", "SPLIT_UPLOAD", "PREFETCH", "LDS_CAND_CAP", "HELPER", "RESTART_CAND", "SORTED", "GCAND_CAP", "TEAM",
         "TEAM_MAX", "ZERO_COPY", "NBL", "SPEC", "SERVER", "SERVER_SLOTS", "SERVER_IDLE_US", "SERVER_LIFE_MS"]
# hooks that leave the kernel form alone: the resident kernel keeps serving single queries while they are set
KEEP_SERVER = {"SERVER", "SERVER_SLOTS", "SERVER_IDLE_US", "SERVER_LIFE_MS", "SPLIT_UPLOAD", "HELPER", "SPEC", "NBL"}
M1, M10 = 1_000_000, 10_000_000
GIB = 1 << 30


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.hnsw_plan_cpu.restype = None
    L.hnsw_plan_cpu.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    L.hnsw_plan_filtered_cpu.restype = None
    L.hnsw_plan_filtered_cpu.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    L.hnsw_knobs_names_a_kernel.restype = C.c_int
    L.hnsw_plan_constants.argtypes = [C.c_void_p]
    return L


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    import os
    for name in list(os.environ):
        if name.startswith("RXGPU_HNSW_"):
            monkeypatch.delenv(name)


class Plan:
    def __init__(self, values):
        for name, v in zip(FIELDS, values):
            setattr(self, name, int(v))


def plan(L, n=M1, nq=1, dim=768, k=10, ef=128, bare=True, sq8=False, to_host=True, avail=0, filtered=None):
    out = np.full(len(FIELDS) + 1, 0xDEAD, np.uint64)
    if filtered is None:
        L.hnsw_plan_cpu(n, dim, int(bare), nq, k, ef, int(sq8), int(to_host), avail, out.ctypes.data)
    else:   # the entry point that names the argument
        L.hnsw_plan_filtered_cpu(n, dim, int(bare), nq, k, ef, int(sq8), int(to_host), avail, int(filtered), out.ctypes.data)
    assert out[-1] == 0xDEAD   # the shim wrote exactly the fields named here
    return Plan(out[:-1])


def test_constants_shared_with_the_kernels(lib):
    c = np.zeros(5, np.int32)
    lib.hnsw_plan_constants(c.ctypes.data)
    assert list(c) == [4096, 1024, 2048, 256, 224]   # kHnswMaxEf, kHnswLdsCandEf, kHnswCandLds, kHnswSortedMaxEf, kHnswSortedMaxEfDel


def test_single_query_1m(lib):
    p = plan(lib)
    assert p.words == 31250 and not p.big_ef
    assert p.vis_hash_log2 == 0 and p.vis_words == 31250 and p.vis_lds_log2 == 13   # bitset in HBM; a handful of searches: the hash set in LDS
    assert p.max_slots == p.vis_slots == 17179
    assert not p.split_upload and p.part_q == 1 and p.first_zero_bytes == 0
    assert (p.st_corr, p.st_norm, p.st_count, p.st_dist, p.st_row, p.st_end) == (3072, 3076, 3080, 3084, 3124, 3164)
    assert p.staged and p.zero_copy
    assert p.use_sorted and p.sorted_mode == 1 and p.sorted_restart_cap == 600 and not p.helper_wanted
    assert p.lds_cand_cap == 1024 and p.ef_cap == 128 and not p.force_global_tiers
    assert (p.tier_cap0, p.tier_cap1) == (65536, 1000001)
    assert (p.prefetch_links, p.team, p.team_max, p.nbl, p.spec) == (1, 4, 256, 0, 0)


def test_single_query_10m_takes_the_hash_set(lib):
    p = plan(lib, n=M10)
    assert p.words == 312500
    assert p.vis_hash_log2 == 14 and p.vis_words == 16384   # 2^13 words >= 64 ef, twice that in HBM
    assert p.max_slots == 1717 and p.vis_slots == 32768


def test_batch_10m_budget_split_helpers(lib):
    p = plan(lib, n=M10, nq=16384, avail=200 * GIB)
    assert p.max_slots == 13743 and p.vis_slots == 32768   # an eighth of what is free, capped at 16 GiB
    assert p.split_upload and p.split_parts == 4 and p.part_q == 4096
    assert not p.staged and not p.zero_copy
    assert p.helper_wanted and p.sorted_restart_cap == 256
    assert p.first_zero_bytes == 0   # nothing to zero: hash set


def test_batch_1m_bitset(lib):
    p = plan(lib, nq=16384)
    assert p.vis_hash_log2 == 0 and p.vis_slots == 17179
    assert p.split_upload and p.split_parts == 4 and p.part_q == 4096   # nq <= vis_slots
    assert p.helper_wanted and p.sorted_restart_cap == 600              # the bitset is the smaller set: the restart area stays
    assert p.first_zero_bytes == 16384 * 31250 * 4                      # zeroed beside the upload
    q = plan(lib, nq=2047)
    assert not q.split_upload and q.part_q == 2047 and not q.helper_wanted
    assert plan(lib, nq=64).first_zero_bytes == 0 and plan(lib, nq=68).first_zero_bytes == 68 * 31250 * 4   # from 8 MiB on


def test_batch_larger_than_a_launch_is_not_split(lib):
    p = plan(lib, nq=20000)
    assert p.vis_slots == 17179 and not p.split_upload and p.part_q == 20000 and p.helper_wanted


def test_staging_and_zero_copy_limits(lib):
    a, b = plan(lib, nq=64), plan(lib, nq=65)
    assert a.staged and a.zero_copy and b.staged and not b.zero_copy
    c, d = plan(lib, nq=256), plan(lib, nq=512)
    assert c.staged and c.st_end == 809984 and not d.staged and not d.zero_copy


def test_sq8_and_sink_calls_copy(lib):
    p = plan(lib, sq8=True)
    assert p.staged and not p.zero_copy
    assert (p.o_qcorr, p.o_qnorm) == (768, 1024) and p.o_qcorr % 256 == 0 and p.o_qnorm % 256 == 0
    assert (p.st_corr, p.st_norm, p.st_count) == (768, 772, 776)
    q = plan(lib, sq8=True, nq=3, dim=100)
    assert (q.o_qcorr, q.o_qnorm) == (512, 768) and q.st_corr == 304
    s = plan(lib, to_host=False)
    assert s.staged and not s.zero_copy


def test_sorted_list_limits(lib):
    a, b = plan(lib, ef=256, k=10), plan(lib, ef=257, k=10)
    assert a.use_sorted and a.lds_cand_cap == 1024 and a.ef_cap == 256
    assert not b.use_sorted and b.lds_cand_cap == 2048 and b.ef_cap == 320
    c, d = plan(lib, ef=224, bare=False), plan(lib, ef=225, bare=False)
    assert c.use_sorted and not d.use_sorted


def test_big_ef_goes_to_the_tiers(lib):
    p = plan(lib, ef=1025, nq=16384)
    assert p.big_ef and not p.split_upload and not p.helper_wanted and p.first_zero_bytes == 0 and not p.use_sorted
    assert (p.tier_cap0, p.tier_cap1) == (65536, 1000001)
    assert not plan(lib, ef=1024).big_ef
    assert plan(lib, n=1000, k=10, ef=100).tier_cap0 == 1001   # a small graph: one tier


def test_filtered_plan_differs_in_the_helpers_only(lib, monkeypatch):
    # a call under an allowed-rows bitmap plans as the same call on a graph with deleted nodes (bare = false), minus the helper workgroups:
    # the filtered family has none.  Only helper_wanted differs — and, at the one shape where the plan shrinks the restart area BECAUSE helpers
    # run beside the batch (ef <= 128, a bitset of 2^17 words or more: 10M rows), the restart area, which keeps its 600 entries.
    shapes = [dict(), dict(nq=64), dict(nq=2047), dict(nq=2048), dict(nq=16384), dict(n=M10, nq=16384, avail=200 * GIB), dict(n=M10, nq=16384, ef=129),
              dict(nq=20000), dict(sq8=True, nq=4096), dict(ef=224, nq=4096), dict(ef=225, nq=4096), dict(ef=1025, nq=16384), dict(to_host=False, nq=4096)]
    shrunk = 0
    for shape in shapes:
        plain, filt = plan(lib, bare=False, **shape), plan(lib, bare=False, filtered=True, **shape)
        assert vars(plan(lib, bare=False, filtered=False, **shape)) == vars(plain), shape
        differ = {f for f in FIELDS if getattr(plain, f) != getattr(filt, f)}
        assert not filt.helper_wanted, shape
        if plain.helper_wanted and plain.sorted_restart_cap == 256:
            shrunk += 1
            assert shape.get("n") == M10 and shape.get("ef", 128) <= 128
            assert differ == {"helper_wanted", "sorted_restart_cap"} and filt.sorted_restart_cap == 600, shape
        else:
            assert differ == ({"helper_wanted"} if plain.helper_wanted else set()), shape
        # all of it at once: the plan of the same call with the helpers switched off
        monkeypatch.setenv("RXGPU_HNSW_HELPER", "0")
        assert vars(plan(lib, bare=False, **shape)) == vars(filt), shape
        monkeypatch.delenv("RXGPU_HNSW_HELPER")
    assert shrunk == 1
    assert plan(lib, bare=False, nq=16384).helper_wanted and not plan(lib, bare=False, nq=2047).helper_wanted   # (both sides of the rule are among the shapes)


def test_hook_visited(lib, monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_VISITED", "bitset")
    p = plan(lib, n=M10)
    assert p.vis_hash_log2 == 0 and p.vis_words == 312500 and p.vis_lds_log2 == 0 and p.vis_slots == p.max_slots == 1717
    monkeypatch.setenv("RXGPU_HNSW_VISITED", "hash")
    p = plan(lib)
    assert p.vis_hash_log2 == 14 and p.vis_words == 16384 and p.vis_lds_log2 == 0
    monkeypatch.delenv("RXGPU_HNSW_VISITED")
    monkeypatch.setenv("RXGPU_HNSW_VISITED_LDS", "0")
    p = plan(lib)
    assert p.vis_lds_log2 == 0 and p.vis_hash_log2 == 0


def test_hook_visited_log2(lib, monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_VISITED_LOG2", "8")
    for n in (M1, M10):   # 16 * 2^8 words is below either bitset: the hash set, as small as asked for — no doubling
        p = plan(lib, n=n)
        assert p.vis_hash_log2 == 8 and p.vis_words == 256 and p.vis_lds_log2 == 8
    assert plan(lib, n=100_000).vis_hash_log2 == 0   # 3125 words: the bitset is the smaller set
    monkeypatch.setenv("RXGPU_HNSW_VISITED_LOG2", "2")
    assert plan(lib, n=M10).vis_hash_log2 == 6
    monkeypatch.setenv("RXGPU_HNSW_VISITED_LOG2", "30")
    assert plan(lib, n=1_000_000_000).vis_hash_log2 == 20


def test_hook_split_upload(lib, monkeypatch):
    for v, parts, part_q in (("0", None, 16384), ("1", None, 16384), ("8", 8, 2048), ("3", 3, 5462), ("99", 16, 1024)):
        monkeypatch.setenv("RXGPU_HNSW_SPLIT_UPLOAD", v)
        p = plan(lib, nq=16384)
        assert p.split_upload == (parts is not None) and p.part_q == part_q
        if parts:
            assert p.split_parts == parts


def test_hooks_of_the_kernel_form(lib, monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_SORTED", "0")
    assert not plan(lib).use_sorted
    monkeypatch.setenv("RXGPU_HNSW_SORTED", "2")
    p = plan(lib)
    assert p.use_sorted and p.sorted_mode == 2
    assert not plan(lib, ef=300).use_sorted
    monkeypatch.delenv("RXGPU_HNSW_SORTED")
    monkeypatch.setenv("RXGPU_HNSW_RESTART_CAND", "6")
    assert plan(lib).sorted_restart_cap == 6 and plan(lib, n=M10, nq=16384).sorted_restart_cap == 6
    monkeypatch.setenv("RXGPU_HNSW_RESTART_CAND", "5000")
    assert plan(lib).sorted_restart_cap == 2048
    monkeypatch.delenv("RXGPU_HNSW_RESTART_CAND")
    monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "8")
    p = plan(lib)
    assert p.lds_cand_cap == 8 and p.force_global_tiers   # the LDS re-run tier is skipped
    monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "0")
    assert plan(lib).lds_cand_cap == 1
    monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "9999")
    assert plan(lib).lds_cand_cap == 2048
    monkeypatch.delenv("RXGPU_HNSW_LDS_CAND_CAP")
    monkeypatch.setenv("RXGPU_HNSW_GCAND_CAP", "64")
    p = plan(lib)
    assert (p.tier_cap0, p.tier_cap1) == (64, 1000001)
    monkeypatch.delenv("RXGPU_HNSW_GCAND_CAP")
    monkeypatch.setenv("RXGPU_HNSW_HELPER", "0")
    p = plan(lib, n=M10, nq=16384)
    assert not p.helper_wanted and p.sorted_restart_cap == 600 and p.split_upload
    monkeypatch.delenv("RXGPU_HNSW_HELPER")
    monkeypatch.setenv("RXGPU_HNSW_ZERO_COPY", "0")
    p = plan(lib)
    assert p.staged and not p.zero_copy
    monkeypatch.delenv("RXGPU_HNSW_ZERO_COPY")
    for name, field, value, want in (("PREFETCH", "prefetch_links", "0", 0), ("TEAM", "team", "1", 1), ("TEAM_MAX", "team_max", "16", 16), ("NBL", "nbl", "1", 1),
                                     ("SPEC", "spec", "1", 1)):
        monkeypatch.setenv("RXGPU_HNSW_" + name, value)
        assert getattr(plan(lib), field) == want
        monkeypatch.delenv("RXGPU_HNSW_" + name)


def test_which_hooks_name_a_kernel(lib, monkeypatch):
    assert lib.hnsw_knobs_names_a_kernel() == 0
    for name in HOOKS:
        monkeypatch.setenv("RXGPU_HNSW_" + name, "hash" if name == "VISITED" else "1")
        assert lib.hnsw_knobs_names_a_kernel() == (0 if name in KEEP_SERVER else 1), name
        monkeypatch.delenv("RXGPU_HNSW_" + name)
    monkeypatch.setenv("RXGPU_HNSW_NO_SUCH_HOOK", "1")     # not a hook: ignored
    monkeypatch.setenv("RXGPU_HNSW_STREAM_GLOBAL", "1")    # read by the streaming sessions, not a search hook
    assert lib.hnsw_knobs_names_a_kernel() == 0
    monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")
    monkeypatch.setenv("RXGPU_HNSW_TEAM", "1")             # one of several is enough
    assert lib.hnsw_knobs_names_a_kernel() == 1
