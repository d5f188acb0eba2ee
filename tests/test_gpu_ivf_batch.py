"""-m gpu: rxgpu_search_knn_lists_batch — IVF-Flat list search for a batch of queries in one launch train — and GpuIvfFlat::SearchBatch on top
of it.  The contract under test: for every query of a batch, rows, distance bits, (dist, row) order, count and rows scanned are what
rxgpu_search_knn_lists gives for that query alone; for one shape also the oracle's exact search over the union of the probed lists.
Inside the envelope (clamped nprobe <= 128, kk <= 128) the device train answers (knn_scan_lists over the concatenated lists), outside it
the single call's chain inside the same call; rxgpu_ivf_read_batch_stats says which.
(The issue's shape list calls d = 192 "fixed form"; the rule it states — the dimensions launch_scan_subset gives to its fixed kernel — sends
192 floats to the generic kernel, with three whole 64-float blocks and no tail.  The shape is tested as listed.)"""
import ctypes as C

import numpy as np
import pytest

from .conftest import lex_topk, make_corpus

pytestmark = pytest.mark.gpu

ERR_PARAMS, ERR_LOGIC = -3, -4
NQS = (1, 2, 7, 33, 300)
PROBE_KK = ((1, 1), (1, 10), (4, 10), (7, 100), (24, 64), (24, 65), (40, 128), (40, 129), (1000, 10))
FAR_STRIDE, FAR_N, FAR_D = 1 << 20, 4160, 768


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def round4(d):
    return (d + 3) & ~3


def clustered(seed, n, d, clusters=64):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 0.25, (clusters, d)).astype(np.float32)
    return (centres[rng.integers(0, clusters, n)] + rng.normal(0, 0.05, (n, d))).astype(np.float32)


def hand_made_lists(n, nlist, seed):
    """list 0 empty, list 1 one row, lists 2 / 3 exactly 64 / 65 rows, list 4 half of all rows, the rest shared out at random; every list ascending"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(np.uint32)
    sizes = [0, 1, 64, 65, n // 2]
    cuts = np.cumsum(sizes)
    lists = [np.sort(perm[a:b]) for a, b in zip(np.concatenate([[0], cuts[:-1]]), cuts)]
    rest = perm[cuts[-1]:]
    owner = rng.integers(5, nlist, rest.size)
    lists += [np.sort(rest[owner == l]) for l in range(5, nlist)]
    assert [l.size for l in lists[:5]] == sizes and sum(l.size for l in lists) == n
    return lists


def make_case(oracle, metric, n, d, nlist, seed):
    """rows, centroids, lists and 300 prepared queries.  The centroids of lists 0..3 are three times as long as the others, so that a query
    placed on one of them has it as its nearest under every metric (checked against the coarse search where it is used); queries 0..3 are
    those four centroids, query 5 repeats query 4."""
    rows = clustered(seed, n, d, 30)
    cents = clustered(seed + 1, nlist, d, 30)
    cents[:4] = np.random.default_rng(seed + 2).normal(0, 0.75, (4, d)).astype(np.float32)
    lists = hand_made_lists(n, nlist, seed + 3)
    q = clustered(seed + 4, 300, d, 30)
    q[:4] = cents[:4]
    q[5] = q[4]
    inv = cinv = None
    if metric == 2:
        inv, cinv = oracle.l2_modules(rows), oracle.l2_modules(cents)
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    return rows, inv, cents, cinv, lists, np.ascontiguousarray(q, np.float32)


def singles(ix, cx, q, nprobe, kk):
    return [ix.search_knn_lists(cx, v, nprobe, kk) for v in q]


def check_batch(ix, cx, q, nprobe, kk, want, what):
    """one batch call over q == want[i] = (dist, row, scanned) of the single call for q[i]"""
    bd, br, bc, bs = ix.search_knn_lists_batch(cx, q, nprobe, kk)
    assert bd.shape == br.shape == (q.shape[0], kk) and bc.shape == bs.shape == (q.shape[0],)
    for i, (sd, sr, ss) in enumerate(want):
        c = int(bc[i])
        assert c == sd.size and int(bs[i]) == ss, what + (i, c, sd.size, int(bs[i]), ss)
        assert c == min(kk, ss), what + (i,)
        assert np.array_equal(br[i, :c], sr) and np.array_equal(bits(bd[i, :c]), bits(sd)), what + (i,)
    return bd, br, bc, bs


SHAPES = {"generic40": (6000, 40, 24), "fixed128": (3000, 128, 40), "blocks192": (3000, 192, 40)}


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_equals_single_per_query(rxgpu, oracle, shape, metric):
    n, d, nlist = SHAPES[shape]
    rows, inv, cents, cinv, lists, q = make_case(oracle, metric, n, d, nlist, 700 + d)
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx:
        ix.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, cinv)
        ix.set_lists(lists)
        ix.ivf_read_batch_stats()
        for l in range(4):   # the four long centroids are their own nearest: queries 0..3 probe lists 0..3 first
            assert int(cx.search_knn(q[l], 1)[1][0, 0]) == l, (metric, l)
        for nprobe, kk in PROBE_KK:
            want = singles(ix, cx, q, nprobe, kk)
            for nq in NQS:
                first = 0 if nq in (7, 300) else 40 - nq   # 7 and 300 hold the centroid queries and the identical pair, the others end at query 39
                check_batch(ix, cx, q[first:first + nq], nprobe, kk, want[first:first + nq], (shape, metric, nprobe, kk, nq))
            calls, queries, trains, single = ix.ivf_read_batch_stats()
            assert calls == len(NQS) and queries == sum(NQS)
            if kk <= 128:   # nprobe is clamped to nlist <= 40: every call is one train
                assert trains == len(NQS) and single == 0, (nprobe, kk, trains, single)
            else:
                assert trains == 0 and single == sum(NQS), (nprobe, kk, trains, single)
            if nprobe == 1:
                # the query on the empty list's centroid: nothing scanned, nothing found, its neighbours in the batch served
                assert want[0][2] == 0 and want[0][0].size == 0 and (want[1][2], want[2][2], want[3][2]) == (1, 64, 65)
                # kk above the rows probed: the one-row list gives count = scanned = 1, the 64-row list 64 when kk = 100
                bd, br, bc, bs = ix.search_knn_lists_batch(cx, q[:7], 1, 100)
                assert (int(bc[0]), int(bs[0])) == (0, 0) and (int(bc[1]), int(bs[1])) == (1, 1) and (int(bc[2]), int(bs[2])) == (64, 64)
                assert int(br[1, 0]) == int(lists[1][0]) and int(bc[3]) == 65 and int(bc[4]) == min(100, int(bs[4]))
                ix.ivf_read_batch_stats()
        # the identical pair
        bd, br, bc, _ = ix.search_knn_lists_batch(cx, q[:7], 4, 10)
        assert np.array_equal(br[4], br[5]) and np.array_equal(bits(bd[4]), bits(bd[5])) and int(bc[4]) == int(bc[5]) == 10
        # the degenerate calls
        bd, br, bc, bs = ix.search_knn_lists_batch(cx, q[:3], 4, 0)
        assert np.all(bc == 0) and np.all(bs == 0)
        bd, br, bc, bs = ix.search_knn_lists_batch(cx, q[:0], 4, 10)
        assert bc.size == 0
        if shape != "generic40":
            return
        # the oracle's exact search over the union of the probed lists
        for nprobe, kk in ((1, 10), (4, 10), (7, 100), (24, 65)):
            bd, br, bc, bs = ix.search_knn_lists_batch(cx, q[:33], nprobe, kk)
            for i in range(33):
                _, probed = lex_topk(oracle.dist_many(metric, q[i], cents, cinv), nprobe)
                ids = np.sort(np.concatenate([lists[int(l)] for l in probed]))
                assert int(bs[i]) == ids.size, (metric, nprobe, kk, i)
                if ids.size == 0:
                    assert int(bc[i]) == 0
                    continue
                wd, wpos = lex_topk(oracle.dist_many(metric, q[i], rows[ids], inv[ids] if inv is not None else None), min(kk, ids.size))
                c = int(bc[i])
                assert c == wd.size and np.array_equal(br[i, :c], ids[wpos]) and np.array_equal(bits(bd[i, :c]), bits(wd)), (metric, nprobe, kk, i)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_wide_nlist_takes_the_train_up_to_128_lists_and_single_calls_above(rxgpu, oracle, metric):
    n, d, nlist = 9000, 24, 300
    rng = np.random.default_rng(400 + metric)
    rows = clustered(17, n, d, 40)
    cents = clustered(18, nlist, d, 40)
    owner = rng.integers(0, nlist, n)
    lists = [np.flatnonzero(owner == l).astype(np.uint32) for l in range(nlist)]
    q = clustered(19, 20, d, 40)
    inv = cinv = None
    if metric == 2:
        inv, cinv = oracle.l2_modules(rows), oracle.l2_modules(cents)
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx:
        ix.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, cinv)
        ix.set_lists(lists)
        ix.ivf_read_batch_stats()
        for nprobe, kk, train in ((128, 10, True), (65, 100, True), (129, 10, False), (300, 10, False)):
            check_batch(ix, cx, q, nprobe, kk, singles(ix, cx, q, nprobe, kk), ("wide", metric, nprobe, kk))
            calls, queries, trains, single = ix.ivf_read_batch_stats()
            assert (calls, queries) == (1, 20)
            if train:
                assert trains >= 1 and single == 0, (nprobe, trains, single)
            else:
                assert trains == 0 and single == 20, (nprobe, trains, single)


def test_one_scan_launch_per_train_whatever_the_batch(rxgpu, oracle, monkeypatch):
    metric, (n, d, nlist) = 0, SHAPES["generic40"]
    rows, inv, cents, cinv, lists, q = make_case(oracle, metric, n, d, nlist, 900)
    monkeypatch.delenv("RXGPU_IVF_BATCH_SCRATCH_BYTES", raising=False)
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx:
        ix.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, cinv)
        ix.set_lists(lists)
        want = singles(ix, cx, q, 4, 10)
        ix.profile_enable(True)
        ix.ivf_read_batch_stats()
        seen = []
        for nq in (8, 300):
            before = [ix.profile_read(s)[0] for s in ("scan_lists", "ivf_batch_offsets")]
            check_batch(ix, cx, q[:nq], 4, 10, want[:nq], ("launches", nq))
            seen.append([ix.profile_read(s)[0] - b for s, b in zip(("scan_lists", "ivf_batch_offsets"), before)])
            assert ix.ivf_read_batch_stats() == (1, nq, 1, 0)
        assert seen[0] == seen[1] == [1, 1], seen          # one scan, one offsets launch per train: 8 queries or 300
        # a small scratch budget cuts the 300 queries into several trains: one scan launch each, the same bits
        monkeypatch.setenv("RXGPU_IVF_BATCH_SCRATCH_BYTES", "40000")
        before = ix.profile_read("scan_lists")[0]
        check_batch(ix, cx, q, 4, 10, want, ("small budget",))
        calls, queries, trains, single = ix.ivf_read_batch_stats()
        assert (calls, queries, single) == (1, 300, 0) and trains > 1
        assert ix.profile_read("scan_lists")[0] - before == trains
        ix.profile_enable(False)


# ---------------------------------------------------------------------------------------------------------------- row layouts
def device_layout(rows, inv, stride, guard=0):
    """the rows in a torch device buffer of [guard + n + guard][stride] floats, NaN wherever no element of a live row lies (the construction of
    tests/test_gpu_row_layout.py) -> (ptr of row 0, keepalive, ptr of the norm of row 0 or None)"""
    import torch
    n, d = rows.shape
    buf = torch.full((n + 2 * guard, stride), float("nan"), dtype=torch.float32, device="cuda")
    buf[guard:guard + n, :d] = torch.from_numpy(np.array(rows)).cuda()
    t_inv, inv_ptr = None, None
    if inv is not None:
        t_inv = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
        t_inv[guard:guard + n] = torch.from_numpy(np.array(inv)).cuda()
        inv_ptr = t_inv.data_ptr() + guard * 4
    torch.cuda.synchronize()
    return buf.data_ptr() + guard * stride * 4, (buf, t_inv), inv_ptr


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("shape", ["generic40", "fixed128"])
def test_batch_over_padded_rows(rxgpu, oracle, shape, metric):
    """rows and centroids adopted at stride = round4(dim) + 20, three guard rows of NaN around them: the same answers as the owned index"""
    n, d, nlist = SHAPES[shape]
    rows, inv, cents, cinv, lists, q = make_case(oracle, metric, n, d, nlist, 1100 + d)
    q = q[:33]
    stride = round4(d) + 20
    ptr, keep, inv_ptr = device_layout(rows, inv, stride, guard=3)
    cptr, ckeep, cinv_ptr = device_layout(cents, cinv, stride, guard=3)
    with rxgpu.VectorIndex(metric, d, n) as own, rxgpu.VectorIndex(metric, d, nlist) as cown, rxgpu.VectorIndex(metric, d) as ix, \
            rxgpu.VectorIndex(metric, d) as cx:
        own.upload_rows(0, rows, inv)
        cown.upload_rows(0, cents, cinv)
        own.set_lists(lists)
        ix.adopt_device_rows(ptr, n, stride, inv_ptr, keepalive=keep)
        cx.adopt_device_rows(cptr, nlist, stride, cinv_ptr, keepalive=ckeep)
        assert ix.row_stride == stride and cx.row_stride == stride
        ix.set_lists(lists)
        for nprobe, kk in ((1, 10), (7, 100), (24, 65)):
            check_batch(ix, cx, q, nprobe, kk, singles(own, cown, q, nprobe, kk), ("padded", shape, metric, nprobe, kk))


@pytest.fixture(scope="module")
def far_buffer():
    """the 16.25 GiB buffer of the far layout (stride 2^20 floats: rows from 4096 on start beyond 2^32 elements): one allocation for the module"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device visible")
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip(f"the far layout needs 16.25 GiB in one piece: {free / 2 ** 30:.1f} GiB of device memory are free, 20 GiB are asked for")
    buf = torch.full((FAR_N, FAR_STRIDE), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    state = {"buf": buf}
    yield state
    state.clear()
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_batch_over_rows_beyond_2_to_the_32_elements(rxgpu, oracle, far_buffer, metric):
    """4160 x 768 rows a 2^20 floats apart; near-duplicates of the queries planted in rows 4100..4150, so that a 32-bit row * stride would answer
    with other rows.  The batch over the far rows == the single calls over an owned index of the same rows."""
    import torch
    rows = make_corpus(4242, FAR_N, FAR_D)
    q = make_corpus(4243, 7, FAR_D)
    noise = make_corpus(4244, 51, FAR_D, scale=0.01)
    for j in range(51):
        rows[4100 + j] = q[j % 7] + noise[j]
    nlist = 16
    cents = make_corpus(4245, nlist, FAR_D)
    lists = [np.flatnonzero(np.random.default_rng(6).integers(0, nlist, FAR_N) == l).astype(np.uint32) for l in range(nlist)]
    inv = cinv = None
    if metric == 2:
        inv, cinv = oracle.l2_modules(rows), oracle.l2_modules(cents)
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    buf = far_buffer["buf"]
    buf[:, :FAR_D] = torch.from_numpy(rows).cuda()
    t_inv = torch.from_numpy(inv).cuda() if inv is not None else None
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0 and 4096 * FAR_STRIDE == 1 << 32
    with rxgpu.VectorIndex(metric, FAR_D, FAR_N) as own, rxgpu.VectorIndex(metric, FAR_D, nlist) as cx, rxgpu.VectorIndex(metric, FAR_D) as ix:
        own.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, cinv)
        own.set_lists(lists)
        ix.adopt_device_rows(buf.data_ptr(), FAR_N, FAR_STRIDE, t_inv.data_ptr() if t_inv is not None else None, keepalive=(buf, t_inv))
        assert ix.row_stride == FAR_STRIDE
        ix.set_lists(lists)
        for nprobe, kk in ((16, 11), (16, 100), (3, 11)):
            want = singles(own, cx, q, nprobe, kk)
            _, br, _, _ = check_batch(ix, cx, q, nprobe, kk, want, ("far", metric, nprobe, kk))
            if nprobe == 16:
                assert np.all(br[:, 0] >= 4100), br[:, 0]   # every list probed: a query's best row is one of its planted copies


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors_are_the_single_entry_s(rxgpu, oracle):
    n, d, nlist = 500, 16, 8
    rows, cents = clustered(1, n, d), clustered(2, nlist, d)
    lists = [np.flatnonzero(np.arange(n) % nlist == l).astype(np.uint32) for l in range(nlist)]
    L = rxgpu.lib()
    q = np.ascontiguousarray(rows[:3])
    dist, row = np.zeros((3, 5), np.float32), np.zeros((3, 5), np.uint32)
    cnt, scanned = np.zeros(3, np.uint32), np.zeros(3, np.uint64)

    def both(h, c):
        one = L.rxgpu_search_knn_lists(h._h, c._h, q.ctypes.data, 2, 5, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data, None)
        many = L.rxgpu_search_knn_lists_batch(h._h, c._h, q.ctypes.data, 3, 2, 5, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data, scanned.ctypes.data)
        return one, many

    with rxgpu.VectorIndex(0, d, n + 1) as ix, rxgpu.VectorIndex(0, d, nlist) as cx, rxgpu.VectorIndex(0, d, nlist + 1) as big, \
            rxgpu.VectorIndex(0, d + 4, nlist) as wide, rxgpu.ShardedVectorIndex(0, d, n, [0, 0]) as sx:
        ix.upload_rows(0, rows)
        cx.upload_rows(0, cents)
        big.upload_rows(0, clustered(3, nlist + 1, d))
        wide.upload_rows(0, clustered(4, nlist, d + 4))
        sx.upload_rows(0, rows)
        assert both(ix, cx) == (ERR_LOGIC, ERR_LOGIC)                      # lists not set
        ix.set_lists(lists)
        assert both(ix, cx) == (0, 0)
        assert both(ix, big) == (ERR_PARAMS, ERR_PARAMS)                   # a coarse index of another size
        assert both(ix, wide) == (ERR_PARAMS, ERR_PARAMS)                  # ... of another dimension
        assert both(sx, cx) == (ERR_LOGIC, ERR_LOGIC)                      # a sharded handle, either side
        assert both(ix, sx) == (ERR_LOGIC, ERR_LOGIC)
        ix.upload_rows(n, rows[:1])                                        # the index grew: the lists are stale
        assert both(ix, cx) == (ERR_LOGIC, ERR_LOGIC)
        assert L.rxgpu_search_knn_lists_batch(ix._h, cx._h, None, 3, 2, 5, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data, None) == ERR_PARAMS
        with pytest.raises(rxgpu.RxGpuError):
            ix.search_knn_lists_batch(cx, q, 2, 5)


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def hostapi(rxgpu):
    from reindexer_amd import hostapi as h
    h.lib()
    return h


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_engine_batch_equals_single_searches(hostapi, monkeypatch, metric):
    monkeypatch.delenv("RXGPU_IVF_BATCH", raising=False)
    n, d, nlist = 8000, 32, 200
    rows = clustered(27, n, d, 25)
    ivf = hostapi.GpuIvfFlat(metric, d, nlist)
    ivf.add_with_ids(rows, np.arange(n, dtype=np.int64) * 3 + 1)
    ivf.train()
    qs = clustered(28, 24, d, 25)
    ivf.batch_stats()
    for k in (10, 127):
        want = {nprobe: [ivf.search(v, k, nprobe=nprobe) for v in qs] for nprobe in (4, 100, 180)}
        for mode in ("default", "threads"):
            if mode == "threads":
                monkeypatch.setenv("RXGPU_IVF_BATCH", "threads")
            else:
                monkeypatch.delenv("RXGPU_IVF_BATCH", raising=False)
            for nprobe in (4, 100, 180):
                bd, bl = ivf.search_batch(qs, k, nprobe=nprobe)
                for i, (sd, sl) in enumerate(want[nprobe]):
                    assert np.array_equal(bl[i], sl) and np.array_equal(bits(bd[i]), bits(sd)), (metric, mode, k, nprobe, i)
                st = ivf.batch_stats()
                if mode == "threads" or nprobe > 128:     # 180 lists are outside the train's envelope: the engine keeps its threads there
                    assert st["trains"] == 0 and st["calls"] == 0, (mode, nprobe, st)
                else:
                    assert st == {"calls": 1, "queries": 24, "trains": 1, "queries_one_by_one": 0}, (mode, nprobe, st)
    monkeypatch.delenv("RXGPU_IVF_BATCH", raising=False)
    bd, bl = ivf.search_batch(qs[:1], 10, nprobe=4)      # one query: the single search, no batch call
    sd, sl = ivf.search(qs[0], 10, nprobe=4)
    assert np.array_equal(bl[0], sl) and np.array_equal(bits(bd[0]), bits(sd))
    assert ivf.batch_stats()["calls"] == 0
    ivf.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_engine_replays_ties_per_query(hostapi, monkeypatch, metric):
    """Exact copies among the vectors: for some queries of a batch equal distances straddle the k-th place (the scanner's order decides: that
    query is replayed), for others they do not.  The batch equals the single searches either way."""
    monkeypatch.delenv("RXGPU_IVF_BATCH", raising=False)
    rng = np.random.default_rng(60 + metric)
    n, d, nlist = 4000, 12, 16
    base = clustered(80 + metric, n, d, 12)
    rows = np.where((rng.random(n) < 0.35)[:, None], base[rng.integers(0, n, n)], base).astype(np.float32)
    ids = rng.permutation(n * 3)[:n].astype(np.int64)
    g = hostapi.GpuIvfFlat(metric, d, nlist)
    g.add_with_ids(rows, ids)
    g.train()
    qs = (rows[rng.integers(0, n, 40)] + rng.normal(0, 0.02, (40, d))).astype(np.float32)
    g.batch_stats()
    straddle = clean = 0
    for nprobe, k in ((3, 1), (8, 3), (16, 10), (5, 50)):
        bd, bl = g.search_batch(qs, k, nprobe=nprobe)
        for i in range(qs.shape[0]):
            sd, sl = g.search(qs[i], k, nprobe=nprobe)
            assert np.array_equal(bl[i], sl) and np.array_equal(bits(bd[i]), bits(sd)), (metric, nprobe, k, i)
            d1, l1 = g.search(qs[i], k + 1, nprobe=nprobe)
            tie = bool(l1[k] >= 0 and d1[k] == d1[k - 1])
            straddle += tie
            clean += not tie
    assert straddle > 5 and clean > 5, (straddle, clean)
    st = g.batch_stats()
    assert st["calls"] == 4 and st["trains"] == 4 and st["queries_one_by_one"] == 0
    g.close()
