"""The decisions of a batched IVF list search (reindexer_amd/csrc/ivf_batch_plan.h), compiled for the host (tests/cpp/ivf_batch_plan_cpu.cc)
and pinned on the CPU: the envelope of the device train, the cut of a call into trains against a scratch budget, gridx, the rule that maps a
64-entry chunk of a query's concatenated probed lists to (probe slot, offset) and the scratch layout.  Every expectation is a restatement of
the rule written here, or a property stated in the test; the header's own output is never read as its expectation."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libivf_batch_plan_cpu.so"
P = C.c_void_p
U32, U64, I32 = C.c_uint32, C.c_uint64, C.c_int
CHUNK = 64          # kIvfBatchChunk: list entries per chunk = lanes of a wavefront
MAX_PROBE = 128     # what the coarse search leaves in HBM (the widest fused top list)
MAX_KK = 128        # entries a wavefront's list holds (two per lane)
MAX_GRID_X = 256    # the plan's stated cap on workgroups per query
WAVES = 4
MAX_TRAIN_QUERIES = 32768


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    for name, res, args in [
        ("ivfb_on_device", I32, [U32, U32]), ("ivfb_wide_list", I32, [U32]), ("ivfb_default_on_device", I32, [U32, U32, U32]),
        ("ivfb_list_chunks", U32, [U64]), ("ivfb_chunk_at", None, [P, U32, U32, P]), ("ivfb_grid_x", U32, [U32, U32, U32, U64, U64, U32]),
        ("ivfb_max_grid_x", U32, []), ("ivfb_default_budget", U64, []), ("ivfb_query_bytes", U64, [U32, U32, U32, U32]),
        ("ivfb_train_queries", U32, [U32, U32, U32, U32, U32, U64]), ("ivfb_trains", U32, [U32, U32]), ("ivfb_scratch", None, [U64, U32, P]),
    ]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


# ---- the envelope
def test_envelope_edges(lib):
    """the train answers 1 <= nprobe <= 128 and 1 <= kk <= 128; one entry per lane up to kk = 64, two above"""
    for nprobe, kk, on in [(128, 10, 1), (129, 10, 0), (1, 128, 1), (1, 129, 0), (128, 128, 1), (129, 129, 0), (1, 1, 1), (0, 10, 0), (4, 0, 0),
                           (16, 64, 1), (16, 65, 1), (1000, 10, 0), (4, 1000, 0)]:
        assert lib.ivfb_on_device(nprobe, kk) == on, (nprobe, kk)
    for kk, wide in [(1, 0), (64, 0), (65, 1), (128, 1)]:
        assert lib.ivfb_wide_list(kk) == wide, kk
    # the engine's default: the batch call for two queries and more inside the envelope, single searches otherwise
    for nq, nprobe, kk, on in [(1, 16, 11, 0), (2, 16, 11, 1), (256, 16, 11, 1), (4096, 64, 128, 1), (256, 129, 11, 0), (256, 16, 129, 0)]:
        assert lib.ivfb_default_on_device(nq, nprobe, kk) == on == (1 if nq >= 2 and nprobe <= MAX_PROBE and kk <= MAX_KK else 0), (nq, nprobe, kk)


# ---- trains against a budget
def query_bytes_py(dim, nprobe, kk, gridx):
    # the query, its partial lists (dist + row), its result (dist + row + count), the coarse result (ids + distances + count), the running
    # chunk counts, the rows probed
    return dim * 4 + gridx * kk * 8 + kk * 8 + 4 + nprobe * 8 + 4 + (nprobe + 1) * 4 + 8


@pytest.mark.parametrize("dim,nprobe,kk,gridx", [(40, 1, 1, 1), (768, 16, 11, 8), (768, 64, 128, 32), (128, 128, 65, 256)])
@pytest.mark.parametrize("budget", [0, 1000, 100_000, 1 << 20, 256 << 20])
@pytest.mark.parametrize("nq", [1, 2, 7, 300, 4096, 100_000])
def test_trains_cover_the_queries_within_the_budget(lib, nq, dim, nprobe, kk, gridx, budget):
    per_query = query_bytes_py(dim, nprobe, kk, gridx)
    assert lib.ivfb_query_bytes(dim, nprobe, kk, gridx) == per_query
    per = lib.ivfb_train_queries(nq, dim, nprobe, kk, gridx, budget)
    assert per == min(nq, MAX_TRAIN_QUERIES, max(1, budget // per_query))
    # the budget holds a train, unless it is smaller than one query: then a train is that one query
    assert 1 <= per <= nq and (per * per_query <= budget or per == 1)
    trains = lib.ivfb_trains(nq, per)
    assert trains == -(-nq // per) and (trains - 1) * per < nq <= trains * per


def test_default_budget_makes_the_readme_shapes_one_train(lib):
    assert lib.ivfb_default_budget() == 256 << 20
    for nq, nprobe in [(256, 1), (256, 16), (256, 64), (4096, 1), (4096, 16), (4096, 64)]:
        gridx = lib.ivfb_grid_x(nq, nprobe, 1024, 1_000_000, 4000, 256)
        assert lib.ivfb_train_queries(nq, 768, nprobe, 11, gridx, 256 << 20) == nq, (nq, nprobe, gridx)
    # ... and a small one cuts 300 queries into several
    assert lib.ivfb_trains(300, lib.ivfb_train_queries(300, 40, 4, 10, 2, 20_000)) > 1


# ---- the chunk rule
def walk(lib, lens):
    """every chunk of the concatenation -> (slot, offset); returns per slot the number of times each entry was visited"""
    lens = [int(v) for v in lens]
    nprobe = len(lens)
    cum = np.zeros(nprobe + 1, np.uint32)
    for s, n in enumerate(lens):
        assert lib.ivfb_list_chunks(n) == -(-n // CHUNK)
        cum[s + 1] = cum[s] + -(-n // CHUNK)
    seen = [np.zeros(n, np.int32) for n in lens]
    out = (U32 * 2)()
    prev = (-1, -1)
    for c in range(int(cum[nprobe])):
        lib.ivfb_chunk_at(cum.ctypes.data, nprobe, c, out)
        slot, off = int(out[0]), int(out[1])
        assert 0 <= slot < nprobe and off % CHUNK == 0 and off < lens[slot], (c, slot, off)     # inside ONE list: no chunk spans two
        assert (slot, off) > prev                                                                # the concatenation in order
        prev = (slot, off)
        seen[slot][off:off + CHUNK] += 1                                                         # (numpy clips at the list's end, as the kernel does)
    return seen


@pytest.mark.parametrize("lens", [[0], [1], [63], [64], [65], [0, 0, 0], [0, 1, 63, 64, 65, 0], [64, 0, 65, 0, 1], [5000, 1, 0, 64], [1] * 128, [0] * 127 + [3]])
def test_chunks_visit_every_entry_once_edge_lists(lib, lens):
    for s in walk(lib, lens):
        assert np.all(s == 1)


@pytest.mark.parametrize("seed", range(6))
def test_chunks_visit_every_entry_once_random_lists(lib, seed):
    rng = np.random.default_rng(seed)
    nprobe = int(rng.integers(1, MAX_PROBE + 1))
    lens = rng.integers(0, 300, nprobe)
    lens[rng.integers(0, nprobe, 6)] = [0, 1, 63, 64, 65, 0]
    lens[int(rng.integers(0, nprobe))] = int(lens.sum())          # one list holds half of all rows
    seen = walk(lib, lens)
    assert all(np.all(s == 1) for s in seen) and sum(s.size for s in seen) == int(lens.sum())


# ---- gridx
@pytest.mark.parametrize("nq", [1, 2, 8, 256, 4096, 100_000])
@pytest.mark.parametrize("nprobe", [1, 16, 64, 128])
@pytest.mark.parametrize("nlist,rows,longest", [(1024, 1_000_000, 4000), (24, 6000, 3000), (40, 3000, 1500), (300, 9000, 60), (16, 0, 0), (1, 1, 1),
                                                (65536, 10_000_000, 1_000_000)])
def test_grid_x_is_bounded_and_useful(lib, nq, nprobe, nlist, rows, longest):
    assert lib.ivfb_max_grid_x() == MAX_GRID_X
    nprobe = min(nprobe, nlist)
    g = lib.ivfb_grid_x(nq, nprobe, nlist, rows, longest, 256)
    assert 1 <= g <= MAX_GRID_X
    # no more workgroups than a query can have chunks for, one chunk per wavefront: at most nprobe longest lists, at most every row
    most = min(nprobe * -(-longest // CHUNK), -(-rows // CHUNK) + nprobe)
    assert g <= max(1, -(-most // WAVES))
    # it does not depend on anything the device would have to be asked for, and never shrinks when the batch does
    assert g >= lib.ivfb_grid_x(nq * 2, nprobe, nlist, rows, longest, 256)


def test_grid_x_of_the_readme_shape(lib):
    """1M x 768 rows in 1024 lists, 256 CUs: 977 rows = 16 chunks per average list.  256 queries at nprobe 16 expect 256 chunks each: 8 per
    wavefront make 8 workgroups; at nprobe 1 the 16 chunks are one workgroup's, and two per query fill the 512 workgroup slots."""
    assert lib.ivfb_grid_x(256, 16, 1024, 1_000_000, 4000, 256) == 8
    assert lib.ivfb_grid_x(256, 1, 1024, 1_000_000, 4000, 256) == 2
    assert lib.ivfb_grid_x(4096, 64, 1024, 1_000_000, 4000, 256) == 32
    assert lib.ivfb_grid_x(2, 16, 1024, 1_000_000, 4000, 256) == 252      # two queries: 256 workgroups each would fill the machine; 16 x 63 chunks / 4 caps it


# ---- scratch
def test_scratch_parts_are_aligned_and_do_not_overlap(lib):
    out = (U64 * 6)()
    for q, nprobe in [(1, 1), (7, 24), (300, 128), (4096, 64), (32768, 128)]:
        lib.ivfb_scratch(q, nprobe, out)
        o = [int(v) for v in out]
        sizes = [q * nprobe * 4, q * nprobe * 4, q * 4, q * (nprobe + 1) * 4, q * 8]
        assert o[0] == 0
        for i in range(5):
            assert o[i] % 256 == 0 and o[i] + sizes[i] <= o[i + 1]
        assert o[5] % 256 == 0
