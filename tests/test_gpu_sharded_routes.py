"""-m gpu: which ROUTE a call on a row-range sharded index takes (reindexer_amd/csrc/shard_plan.h decides, rxgpu_sharded.hip executes) — through
the exchange on the devices (one more collective) or through the host — and that the route does not change the answer: every result is compared
bit for bit with a single-device index over the same rows.  The sibling of test_gpu_ft_routes.py.  The shapes are the smallest at which this
host code can go wrong: dim 24, capacity 1000 over the device list [0, 0, 0] = 352 rows a shard, so that 351 | 352 and 703 | 704 are the shard
boundaries.  (tests/test_gpu_sharded_map.py holds the same index against the reference engine on larger corpora: exchange at kk 1 / 11 / 64 on
full, partial and empty shards, host merge at kk 100, swap-with-last deletes, rxgpu_distances over an unordered list.)"""
import contextlib
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from .conftest import make_corpus

pytestmark = pytest.mark.gpu

D, CAP, SHARDS = 24, 1000, 3
SHARD_ROWS = 352                                   # (ceil(1000 / 3) + 31) & ~31
ACROSS = np.array([0, 17, 351, 352, 353, 500, 703, 704, 705], np.uint32)   # a row list that crosses both boundaries
PLAN_SRC = Path(__file__).resolve().parent / "cpp" / "shard_plan_cpu.cc"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def corpus():
    return make_corpus(31, CAP, D), make_corpus(32, 4, D)


@pytest.fixture
def pair(rxgpu, corpus, monkeypatch):
    """(sharded, single-device) indexes over the first `fill` rows of the corpus"""
    from reindexer_amd import capi
    monkeypatch.delenv("RXGPU_SHARD_MERGE", raising=False)

    @contextlib.contextmanager
    def make(fill, metric=capi.METRIC_IP):
        with capi.ShardedVectorIndex(metric, D, CAP, [0] * SHARDS) as sx, capi.VectorIndex(metric, D, CAP) as one:
            assert sx.merge_mode == "rccl" and sx.shard_rows == SHARD_ROWS
            for ix in (sx, one):
                ix.upload_rows(0, corpus[0][:fill])
            yield sx, one
    return make


def collectives_of(sx, call):
    before = sx.collectives
    out = call()
    return out, sx.collectives - before


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_exchange_route_takes_one_collective_per_call(pair, corpus, metric):
    from reindexer_amd import capi
    q = corpus[1]
    with pair(900, capi.METRICS[metric]) as (sx, one):
        for kk, want in ((11, 1), (64, 1), (65, 0)):       # 65: past the fused scan's lists, merged on the host
            for qs in (q[:1], q):
                got, n = collectives_of(sx, lambda: sx.search_knn(qs, kk))
                assert n == want, (kk, len(qs))
                assert same(got, one.search_knn(qs, kk)), (kk, len(qs))


def test_a_shard_shorter_than_kk_sends_the_call_through_the_host(pair, corpus):
    q = corpus[1]
    with pair(710) as (sx, one):                           # the last shard holds 710 - 704 = 6 rows
        assert sx.shard(2).count == 6
        for kk, want in ((11, 0), (6, 1), (7, 0)):
            for qs in (q[:1], q):
                got, n = collectives_of(sx, lambda: sx.search_knn(qs, kk))
                assert n == want, (kk, len(qs))
                assert same(got, one.search_knn(qs, kk)), (kk, len(qs))
                assert (got[2] == kk).all()


def test_a_row_list_goes_through_the_host_and_is_checked_alike(pair, corpus):
    from reindexer_amd import capi
    q = corpus[1]
    with pair(900) as (sx, one):
        for kk in (1, 5, 9, 11):                           # 11 > the 9 listed rows: short counts
            for qs in (q[:1], q):
                got, n = collectives_of(sx, lambda: sx.search_knn_subset(qs, kk, ACROSS))
                assert n == 0
                assert same(got, one.search_knn_subset(qs, kk, ACROSS)), kk
                assert (got[2] == min(kk, len(ACROSS))).all() and np.isin(got[1][:, :min(kk, len(ACROSS))], ACROSS).all()
        one_shard = np.array([352, 400, 703], np.uint32)   # every row in the middle shard: the others are not asked
        assert same(sx.search_knn_subset(q, 3, one_shard), one.search_knn_subset(q, 3, one_shard))
        for bad in ([0, 352, 351, 704], [0, 352, 352, 704], [0, 352, 900], [900]):   # a descent, equal neighbours, an id equal to count
            for ix in (sx, one):
                with pytest.raises(capi.RxGpuError) as e:
                    ix.search_knn_subset(q, 5, np.array(bad, np.uint32))
                assert e.value.code == capi.RXGPU_ERR_PARAMS, (bad, ix)
                with pytest.raises(capi.RxGpuError) as e:
                    ix.search_range_subset(q[0], 0.0, np.array(bad, np.uint32))
                assert e.value.code == capi.RXGPU_ERR_PARAMS, (bad, ix)


def range_call(ix, query, radius, cap, row_ids=None):
    from reindexer_amd import capi
    L = capi.lib()
    dist, row, total = np.full(max(cap, 1), -7.0, np.float32), np.full(max(cap, 1), 0xEEEEEEEE, np.uint32), C.c_uint64(0)
    q = np.ascontiguousarray(query, np.float32)
    if row_ids is None:
        rc = L.rxgpu_search_range(ix._h, q.ctypes.data, C.c_float(radius), 0, dist.ctypes.data, row.ctypes.data, cap, C.byref(total))
    else:
        rc = L.rxgpu_search_range_subset(ix._h, q.ctypes.data, C.c_float(radius), 0, row_ids.ctypes.data, row_ids.size, dist.ctypes.data, row.ctypes.data, cap,
                                         C.byref(total))
    return rc, int(total.value), dist, row


def test_range_calls_and_their_overflow(pair, corpus):
    from reindexer_amd import capi
    q = corpus[1][0]
    listed = np.arange(0, 900, 3, dtype=np.uint32)
    with pair(900) as (sx, one):
        everything = one.distances(q, np.arange(900, dtype=np.uint32))
        radius = float(np.sort(everything)[120])           # ~120 of 900 rows: hits in all three shards
        for ids in (None, listed):
            rc1, n1, d1, r1 = range_call(one, q, radius, 400, ids)
            rc3, n3, d3, r3 = range_call(sx, q, radius, 400, ids)
            assert rc1 == rc3 == 0 and n1 == n3 and n1 >= 30
            assert np.array_equal(r3[:n3], r1[:n1]) and np.array_equal(bits(d3[:n3]), bits(d1[:n1]))
            assert len({int(r) // SHARD_ROWS for r in r3[:n3]}) == SHARDS
            assert sx.collectives == 0                     # range calls never take the exchange
            for cap in (5, n1 - 1):                        # fewer than the hits: the same code and the same total from both handles
                o1, o3 = range_call(one, q, radius, cap, ids), range_call(sx, q, radius, cap, ids)
                assert o1[0] == o3[0] == capi.RXGPU_ERR_OVERFLOW and o1[1] == o3[1] == n1, (cap, o1[:2], o3[:2])
            o1, o3 = range_call(one, q, radius, n1, ids), range_call(sx, q, radius, n1, ids)   # exactly the hits: fits
            assert o1[0] == o3[0] == 0 and np.array_equal(o1[3][:n1], o3[3][:n1])


def test_truncation_and_moves_keep_the_shards_in_step(pair, corpus):
    q = corpus[1]
    with pair(900) as (sx, one):
        for count in (500, SHARD_ROWS):                    # mid-shard, then exactly on a boundary
            for ix in (sx, one):
                ix.truncate(count)
            assert [sx.shard(s).count for s in range(SHARDS)] == [min(max(count - s * SHARD_ROWS, 0), SHARD_ROWS) for s in range(SHARDS)]
            for kk in (11, 100):
                got = sx.search_knn(q, kk)
                assert same(got, one.search_knn(q, kk)) and got[1][got[1] != 0xFFFFFFFF].max() < count
    with pair(900) as (sx, one):
        moves = [(899, 710), (340, 3), (800, 351), (352, 703), (10, 899)]   # inside the last and the first shard, across two shards, onto boundaries
        for src, dst in moves:
            for ix in (sx, one):
                ix.move_row(src, dst)
        pick = np.array([899, 710, 703, 703, 351, 3, 0], np.uint32)         # moved rows in descending order, with a repeat
        assert np.array_equal(bits(sx.distances(q[0], pick)), bits(one.distances(q[0], pick)))
        assert same(sx.search_knn(q, 11), one.search_knn(q, 11))


def test_layout_matches_the_plan(rxgpu):
    """rxgpu_index_shard_rows / _shard_count / _shard_ranks against the rule restated here and, where this tree has it, the CPU build of the plan"""
    from reindexer_amd import capi
    plan = None
    if PLAN_SRC.exists():
        lib_path = PLAN_SRC.parent / "libshard_plan_cpu.so"
        if not lib_path.exists():
            from reindexer_amd import build
            build.build_cpp_tests()
        plan = C.CDLL(str(lib_path))
        plan.shard_plan_rows.restype, plan.shard_plan_rows.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32]
        plan.shard_plan_local_count.restype, plan.shard_plan_local_count.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint64]
    for capacity, n in ((1000, 3), (3000, 5), (3, 8), (64, 2), (65, 2)):
        with capi.ShardedVectorIndex(capi.METRIC_IP, D, capacity, [0] * n) as sx:
            rows = (-(-capacity // n) + 31) // 32 * 32
            assert (sx.shard_rows, sx.shard_count, sx.ranks) == (rows, n, 1)   # one distinct device: one rank
            caps = [max(min(capacity - s * rows, rows), 0) for s in range(n)]
            assert [sx.shard(s).capacity for s in range(n)] == [max(c, 1) for c in caps]   # a shard past the end is created with one row
            if plan is not None:
                assert plan.shard_plan_rows(capacity, n) == sx.shard_rows
                assert [plan.shard_plan_local_count(rows, s, capacity) for s in range(n)] == caps
