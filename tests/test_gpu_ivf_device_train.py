"""-m gpu: IVF-Flat trained on the device from the rows the index already holds (rxgpu_ivf_assign, rxgpu_ivf_kmeans_step, GpuIvfFlat.train /
add_with_ids by default; RXGPU_IVF_TRAIN=host keeps the host path).

What the device computes is held to restatements written here:
  * the nearest centroid of a resident row is what rxgpu_search_knn(coarse, k = 1) answers for the row's prepared vector computed in numpy
    (row, for cosine row * (1 / |row|) in float32) — row ranges, lists in any order, several chunks of the gathered block, adopted padded rows;
  * one k-means step's centroids are the SEQUENTIAL loop `for i in range(n): c[a[i]] += p[i]` in float32 over the list positions, then
    c[k] *= 1 / count_k — compared as bit patterns.  The test shows on the host that its inputs tell the orders apart: the same loop in
    ascending ROW order, and a fused (float64) accumulation for cosine, give other bits;
  * GpuIvfFlat.train() / add_with_ids() give the centroid bits and lists of the host path and of the vendored FAISS (RefIvf,
    exact_assignment), and train_stats() tells which path ran."""
import numpy as np
import pytest

from .conftest import lex_topk
from .test_gpu_ivf import bits, clustered

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]   # l2, ip, cosine
SHAPES = [(3000, 40, 8), (2500, 37, 16), (1200, 768, 32)]   # (n, d, nlist)
ERR_PARAMS, ERR_LOGIC = -3, -4
ENV = ("RXGPU_IVF_TRAIN", "RXGPU_IVF_TRAIN_SCRATCH_BYTES")


@pytest.fixture(scope="module")
def hostapi(rxgpu):
    from reindexer_amd import hostapi as h
    h.lib()
    return h


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def round4(d):
    return (d + 3) & ~3


# ---------------------------------------------------------------------------------------------------------------- data, made once
_cache = {}


def prepare(rows, inv):
    """the vectors the reference trains on and assigns: the row, for cosine row * (1 / |row|) — one float32 multiply per element"""
    return rows if inv is None else (rows * inv[:, None]).astype(np.float32)


def data(oracle, metric, n, d, nlist):
    """(rows, inv or None, prepared, centroids, centroid inv or None), read-only"""
    key = ("data", metric, n, d, nlist)
    if key not in _cache:
        rows = clustered(700 + d, n, d)
        cents = clustered(800 + d, nlist, d)
        inv = oracle.l2_modules(rows) if metric == 2 else None
        cinv = oracle.l2_modules(cents) if metric == 2 else None
        out = (rows, inv, prepare(rows, inv), cents, cinv)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def open_pair(rxgpu, metric, rows, inv, cents, cinv):
    ix = rxgpu.VectorIndex(metric, rows.shape[1], rows.shape[0])
    cx = rxgpu.VectorIndex(metric, rows.shape[1], cents.shape[0])
    ix.upload_rows(0, rows, inv)
    cx.upload_rows(0, cents, cinv)
    return ix, cx


def expected_assign(rxgpu, oracle, metric, n, d, nlist):
    """search_knn(k = 1) on the coarse index over the prepared vectors computed in numpy: the host-query call, once per shape"""
    key = ("want", metric, n, d, nlist)
    if key not in _cache:
        rows, inv, prepared, cents, cinv = data(oracle, metric, n, d, nlist)
        with rxgpu.VectorIndex(metric, d, nlist) as cx:
            cx.upload_rows(0, cents, cinv)
            _, row, cnt = cx.search_knn(prepared, 1)
        assert np.all(cnt == 1)
        want = row[:, 0].copy()
        want.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def lists_of(n, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(n).astype(np.uint32), rng.integers(0, n, 257).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. rxgpu_ivf_assign
@pytest.mark.parametrize("n,d,nlist", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_assign_equals_the_host_query_call(rxgpu, oracle, monkeypatch, metric, n, d, nlist):
    rows, inv, _, cents, cinv = data(oracle, metric, n, d, nlist)
    want = expected_assign(rxgpu, oracle, metric, n, d, nlist)
    perm, short = lists_of(n, 11 + n)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    with ix, cx:
        assert np.array_equal(ix.ivf_assign(cx, None, 0, n), want)
        assert np.array_equal(ix.ivf_assign(cx, None, 17, n - 22), want[17:n - 5])     # first_row != 0, the range ends below count
        assert np.array_equal(ix.ivf_assign(cx, perm), want[perm])
        assert np.array_equal(ix.ivf_assign(cx, np.array([n - 1], np.uint32)), want[n - 1:])
        assert np.array_equal(ix.ivf_assign(cx, short), want[short])                    # 257 entries: a full query tile and one more
        assert ix.ivf_assign(cx, np.empty(0, np.uint32)).size == 0                      # n == 0 is RXGPU_OK
        monkeypatch.setenv("RXGPU_IVF_TRAIN_SCRATCH_BYTES", "1")                        # chunks of one query tile: n is no multiple of 256
        assert np.array_equal(ix.ivf_assign(cx, perm), want[perm])
        assert np.array_equal(ix.ivf_assign(cx, None, 3, n - 3), want[3:])
        monkeypatch.delenv("RXGPU_IVF_TRAIN_SCRATCH_BYTES")
        rows_assigned, steps, ms, _ = ix.ivf_read_train_stats()
        assert rows_assigned == n + (n - 22) + n + 1 + 257 + n + (n - 3) and steps == 0 and ms > 0
        assert ix.ivf_read_train_stats()[:2] == (0, 0)                                  # reading resets


def device_layout(rows, inv, stride, guard):
    """The rows in a torch device buffer of [guard + n + guard][stride] floats, NaN wherever no element of a live row lies (the layout
    pattern of tests/test_gpu_row_layout.py).  -> (ptr of row 0, keepalive, ptr of the norm of row 0 or None)"""
    import torch
    n, d = rows.shape
    assert stride >= d and stride % 4 == 0
    buf = torch.full((n + 2 * guard, stride), float("nan"), dtype=torch.float32, device="cuda")
    buf[guard:guard + n, :d] = torch.from_numpy(np.array(rows)).cuda()
    t_inv, inv_ptr = None, None
    if inv is not None:
        t_inv = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
        t_inv[guard:guard + n] = torch.from_numpy(np.array(inv)).cuda()
        inv_ptr = t_inv.data_ptr() + guard * 4
    torch.cuda.synchronize()
    return buf.data_ptr() + guard * stride * 4, (buf, t_inv), inv_ptr


@pytest.mark.parametrize("metric", METRICS)
def test_assign_and_step_over_adopted_padded_rows(rxgpu, oracle, metric):
    """stride = round4(37) + 20 floats, three guard rows of NaN around the rows, NaN in every pad: only the first dim floats of a row count"""
    n, d, nlist = 2500, 37, 16
    rows, inv, prepared, cents, cinv = data(oracle, metric, n, d, nlist)
    want = expected_assign(rxgpu, oracle, metric, n, d, nlist)
    perm, short = lists_of(n, 21)
    ptr, keep, inv_ptr = device_layout(rows, inv, round4(d) + 20, 3)
    with rxgpu.VectorIndex(metric, d, 0) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx:
        ix.adopt_device_rows(ptr, n, round4(d) + 20, inv_ptr, keepalive=keep)
        cx.upload_rows(0, cents, cinv)
        assert np.array_equal(ix.ivf_assign(cx, None, 0, n), want)
        assert np.array_equal(ix.ivf_assign(cx, None, 5, n - 5), want[5:])
        assert np.array_equal(ix.ivf_assign(cx, perm), want[perm])
        assert np.array_equal(ix.ivf_assign(cx, short), want[short])
        cent, hassign, a = ix.ivf_kmeans_step(cx, perm)
        assert np.array_equal(a, want[perm])
        wc, wh = sequential_centroids(prepared[perm], a, nlist)
        assert np.array_equal(bits(cent), bits(wc)) and np.array_equal(hassign, wh)


@pytest.mark.parametrize("metric", METRICS)
def test_assign_errors(rxgpu, oracle, metric):
    n, d, nlist = 3000, 40, 8
    rows, inv, _, cents, cinv = data(oracle, metric, n, d, nlist)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    out_c, out_h = np.empty((nlist, d), np.float32), np.empty(nlist, np.float32)
    with ix, cx:
        for bad in (np.array([n], np.uint32), np.array([0, 5, n, 7], np.uint32), np.array([0xFFFFFFFF], np.uint32)):
            with pytest.raises(rxgpu.RxGpuError) as e:   # an id == count (or beyond) is refused on the host, before any launch
                ix.ivf_assign(cx, bad)
            assert e.value.code == ERR_PARAMS
            with pytest.raises(rxgpu.RxGpuError) as e:
                ix.ivf_kmeans_step(cx, bad)
            assert e.value.code == ERR_PARAMS
        with pytest.raises(rxgpu.RxGpuError) as e:       # a range past count
            ix.ivf_assign(cx, None, n - 3, 4)
        assert e.value.code == ERR_PARAMS
        with pytest.raises(rxgpu.RxGpuError) as e:       # more points than rows
            ix.ivf_kmeans_step(cx, None, n + 1)
        assert e.value.code == ERR_PARAMS
        with rxgpu.VectorIndex(metric, d + 4, nlist) as other:   # a coarse index of another dimension: what the list search answers
            other.upload_rows(0, np.zeros((nlist, d + 4), np.float32) + 1, np.ones(nlist, np.float32) if metric == 2 else None)
            with pytest.raises(rxgpu.RxGpuError) as e:
                ix.ivf_assign(other, None, 0, 10)
            assert e.value.code == ERR_PARAMS
            ix.set_lists([np.arange(n, dtype=np.uint32)] + [np.empty(0, np.uint32)] * (nlist - 1))
            with pytest.raises(rxgpu.RxGpuError) as e2:
                ix.search_knn_lists(other, rows[0], 1, 1)
            assert e2.value.code == e.value.code
        with rxgpu.ShardedVectorIndex(metric, d, n, [0, 0]) as sx:
            sx.upload_rows(0, rows, inv)
            with pytest.raises(rxgpu.RxGpuError) as e:
                sx.ivf_assign(cx, None, 0, 10)
            assert e.value.code == ERR_LOGIC
            with pytest.raises(rxgpu.RxGpuError) as e:
                sx.ivf_kmeans_step(cx, None, 10)
            assert e.value.code == ERR_LOGIC
        # 2^24 points and more: refused before the list is looked at
        from reindexer_amd import capi
        rc = capi.lib().rxgpu_ivf_kmeans_step(ix._h, cx._h, None, 1 << 24, out_c.ctypes.data, out_h.ctypes.data, None)
        assert rc == ERR_PARAMS
        # nothing above left the index unusable
        assert np.array_equal(ix.ivf_assign(cx, None, 0, 300), expected_assign(rxgpu, oracle, metric, n, d, nlist)[:300])


# ---------------------------------------------------------------------------------------------------------------- 2. rxgpu_ivf_kmeans_step
def sequential_centroids(p, a, nlist, order=None):
    """compute_centroids as the reference runs it: one float32 add per point and component, in the order given (default: list order)"""
    c = np.zeros((nlist, p.shape[1]), np.float32)
    for i in (range(p.shape[0]) if order is None else order):
        c[a[i]] += p[i]
    counts = np.bincount(a, minlength=nlist)
    for k in range(nlist):
        if counts[k]:
            c[k] *= np.float32(1) / np.float32(counts[k])
    return c, counts.astype(np.float32)


def fused_centroids(rows, inv, a, nlist):
    """the cosine multiply contracted into the add: sum = round32(sum + row * inv) with the product kept exact (float64)"""
    c = np.zeros((nlist, rows.shape[1]), np.float32)
    r64, i64 = rows.astype(np.float64), inv.astype(np.float64)
    for i in range(rows.shape[0]):
        c[a[i]] = (c[a[i]].astype(np.float64) + r64[i] * i64[i]).astype(np.float32)
    counts = np.bincount(a, minlength=nlist)
    for k in range(nlist):
        if counts[k]:
            c[k] *= np.float32(1) / np.float32(counts[k])
    return c


@pytest.mark.parametrize("n,d,nlist", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_step_equals_the_sequential_restatement(rxgpu, oracle, monkeypatch, metric, n, d, nlist):
    rows, inv, prepared, cents, cinv = data(oracle, metric, n, d, nlist)
    want = expected_assign(rxgpu, oracle, metric, n, d, nlist)
    perm, _ = lists_of(n, 31 + n)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    with ix, cx:
        cent, hassign, a = ix.ivf_kmeans_step(cx, perm)
        assert np.array_equal(a, want[perm])                       # the step's own assignment, first
        p = prepared[perm]                                         # the prepared vectors in LIST order
        wc, wh = sequential_centroids(p, a, nlist)
        # the inputs tell the orders apart: ascending ROW order is another sum ...
        by_row, _ = sequential_centroids(p, a, nlist, order=np.argsort(perm, kind="stable"))
        assert np.any(bits(by_row) != bits(wc))
        if metric == 2:   # ... and so is a multiply fused into the add
            assert np.any(bits(fused_centroids(rows[perm], inv[perm], a, nlist)) != bits(wc))
        assert np.array_equal(hassign, wh)
        diff = int((bits(cent) != bits(wc)).sum())
        assert diff == 0, (metric, n, d, nlist, diff, cent.size)
        # the first n rows without a list (row_ids == NULL), and the same list over chunks of one query tile
        cent0, hassign0, a0 = ix.ivf_kmeans_step(cx, None, n - 7)
        assert np.array_equal(a0, want[:n - 7])
        wc0, wh0 = sequential_centroids(prepared[:n - 7], a0, nlist)
        assert np.array_equal(bits(cent0), bits(wc0)) and np.array_equal(hassign0, wh0)
        monkeypatch.setenv("RXGPU_IVF_TRAIN_SCRATCH_BYTES", "1")
        cent1, hassign1, a1 = ix.ivf_kmeans_step(cx, perm)
        assert np.array_equal(a1, a) and np.array_equal(bits(cent1), bits(wc)) and np.array_equal(hassign1, wh)
        monkeypatch.delenv("RXGPU_IVF_TRAIN_SCRATCH_BYTES")
        rows_assigned, steps, ms, sums_ms = ix.ivf_read_train_stats()
        assert rows_assigned == 3 * n - 7 and steps == 3 and ms >= sums_ms > 0


def offset_rows(seed, n, d):
    """clustered rows moved to 1 +- 0.3 per component: a centroid at -100 is then the farthest under every metric (L2: far away; inner
    product and cosine: the most negative similarity with every row)"""
    return (clustered(seed, n, d) + np.float32(1)).astype(np.float32)


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_step_with_empty_centroids(rxgpu, oracle, metric):
    n, d, nlist = 3000, 40, 8
    rows = offset_rows(41, n, d)
    cents = offset_rows(42, nlist, d)
    cents[2] = -100.0
    cents[7] = -130.0   # the last one: the segment offsets end with an empty segment
    inv = oracle.l2_modules(rows) if metric == 2 else None
    cinv = oracle.l2_modules(cents) if metric == 2 else None
    perm, _ = lists_of(n, 43)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    with ix, cx:
        _, wrow, _ = cx.search_knn(prepare(rows, inv), 1)
        cent, hassign, a = ix.ivf_kmeans_step(cx, perm)
        assert np.array_equal(a, wrow[perm, 0])
        assert hassign[2] == 0 and hassign[7] == 0 and int(hassign.sum()) == n
        assert not cent[2].any() and not cent[7].any()              # rows of zeros, not NaN (0 x 1 / 0)
        assert np.array_equal(bits(cent[[2, 7]]), np.zeros((2, d), np.uint32))
        wc, wh = sequential_centroids(prepare(rows, inv)[perm], a, nlist)
        assert np.array_equal(bits(cent), bits(wc)) and np.array_equal(hassign, wh)


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_step_with_one_centroid_taking_every_point(rxgpu, oracle, metric):
    """the long chain: one wavefront per 64 columns adds 6000 members in order"""
    n, d, nlist = 6000, 40, 5
    rows = offset_rows(51, n, d)
    cents = np.empty((nlist, d), np.float32)
    cents[:] = (-100.0 - 10.0 * np.arange(nlist, dtype=np.float32))[:, None]
    cents[3] = rows.mean(axis=0)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    cinv = oracle.l2_modules(cents) if metric == 2 else None
    perm, _ = lists_of(n, 53)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    with ix, cx:
        cent, hassign, a = ix.ivf_kmeans_step(cx, perm)
        assert np.all(a == 3) and hassign.tolist() == [0, 0, 0, float(n), 0]
        wc, _ = sequential_centroids(prepare(rows, inv)[perm], a, nlist)
        assert np.array_equal(bits(cent), bits(wc))
        by_row, _ = sequential_centroids(prepare(rows, inv)[perm], a, nlist, order=np.argsort(perm, kind="stable"))
        assert np.any(bits(by_row) != bits(wc))                     # 6000 adds in another order are another sum


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_step_dim_1(rxgpu, oracle, metric):
    n, d, nlist = 3000, 1, 4
    rows, inv, prepared, cents, cinv = data(oracle, metric, n, d, nlist)
    want = expected_assign(rxgpu, oracle, metric, n, d, nlist)
    perm, _ = lists_of(n, 61)
    ix, cx = open_pair(rxgpu, metric, rows, inv, cents, cinv)
    with ix, cx:
        assert np.array_equal(ix.ivf_assign(cx, perm), want[perm])
        cent, hassign, a = ix.ivf_kmeans_step(cx, perm)
        assert np.array_equal(a, want[perm])
        wc, wh = sequential_centroids(prepared[perm], a, nlist)
        assert np.array_equal(bits(cent), bits(wc)) and np.array_equal(hassign, wh)


# ---------------------------------------------------------------------------------------------------------------- 3. GpuIvfFlat.train()
TRAIN_SHAPES = [(2500, 32, 16, 16), (9000, 48, 32, 200), (700, 24, 16, 3), (3000, 40, 8, 64), (2600, 37, 10, 64)]   # (n, d, nlist, clusters)


def trained(hostapi, metric, d, nlist, rows, ids, first=None):
    g = hostapi.GpuIvfFlat(metric, d, nlist)
    g.add_with_ids(rows if first is None else rows[:first], ids if first is None else ids[:first])
    g.train_stats()   # (nothing ran on the device yet; start from zero in any case)
    g.train()
    return g


def sorted_lists(g, nlist):
    return [np.sort(g.list_ids(c)) for c in range(nlist)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,nlist,clusters", TRAIN_SHAPES)
def test_train_on_the_device_equals_the_host_path_and_the_vendored_faiss(hostapi, monkeypatch, metric, n, d, nlist, clusters):
    """The four shapes of test_training_equals_vendored_faiss_bit_for_bit ((9000, 32 lists) takes the rand_perm subsample, (700, 16 lists, 3
    clusters) runs split_clusters) and (2600, 37, 10): a row stride that is not the dimension, with the subsample taken."""
    from oracle.pyoracle import RefIvf, ref_ivf_available
    rows = clustered(50 + metric, n, d, clusters)
    ids = (np.arange(n, dtype=np.int64) * 7 + 3)
    ns = min(n, nlist * 256)
    dev = trained(hostapi, metric, d, nlist, rows, ids)
    st = dev.train_stats()
    assert st["steps"] == (0 if ns == nlist else 10), st
    assert st["rows_assigned"] == st["steps"] * ns + n and st["rows_assigned"] >= n, st
    assert st["kernel_ms"] > 0 and st["sums_ms"] > 0
    monkeypatch.setenv("RXGPU_IVF_TRAIN", "host")
    host = trained(hostapi, metric, d, nlist, rows, ids)
    monkeypatch.delenv("RXGPU_IVF_TRAIN")
    assert host.train_stats() == {"rows_assigned": 0, "steps": 0, "kernel_ms": 0.0, "sums_ms": 0.0}
    cent_dev, cent_host = dev.centroids(), host.centroids()
    assert np.array_equal(bits(cent_dev), bits(cent_host)), (metric, int((bits(cent_dev) != bits(cent_host)).sum()))
    lists_dev, lists_host = sorted_lists(dev, nlist), sorted_lists(host, nlist)
    for c in range(nlist):
        assert np.array_equal(lists_dev[c], lists_host[c]), (metric, c)
    assert sum(l.size for l in lists_dev) == n
    if ref_ivf_available():
        ref = RefIvf(metric, d, nlist, rows, ids, exact_assignment=True)
        cent_ref, lists_ref = ref.export()
        assert np.array_equal(bits(cent_dev), bits(cent_ref)), (metric, int((bits(cent_dev) != bits(cent_ref)).sum()))
        for c in range(nlist):
            assert np.array_equal(lists_dev[c], np.sort(lists_ref[c])), (metric, c)
        ref.close()
    dev.close()
    host.close()


# ---------------------------------------------------------------------------------------------------------------- 4. add_with_ids after training
@pytest.mark.parametrize("metric", METRICS)
def test_add_with_ids_after_training(hostapi, oracle, monkeypatch, metric):
    """Half of the rows before train(), the rest after, in batches of 1, 255 and the remainder.  The reference shim trains and fills its
    lists in one call and has no add behind it, so: the first half's lists and the centroids against RefIvf over that half, and every
    later row against its nearest centroid in the oracle's arithmetic over those centroids — which is where IndexIVF::add_with_ids puts it."""
    from oracle.pyoracle import RefIvf, ref_ivf_available
    n, d, nlist = 3000, 40, 8
    rows = clustered(90 + metric, n, d, 64)
    ids = (np.arange(n, dtype=np.int64) * 5 + 11)
    half = n // 2
    batches = [(half, half + 1), (half + 1, half + 256), (half + 256, n)]

    def build():
        g = trained(hostapi, metric, d, nlist, rows, ids, first=half)
        g.train_stats()
        grown = []
        for a, b in batches:
            g.add_with_ids(rows[a:b], ids[a:b])
            grown.append(g.train_stats()["rows_assigned"])
        return g, grown

    dev, grown = build()
    assert grown == [b - a for a, b in batches]                     # rows_assigned grows by exactly the added rows
    monkeypatch.setenv("RXGPU_IVF_TRAIN", "host")
    host, grown_host = build()
    monkeypatch.delenv("RXGPU_IVF_TRAIN")
    assert grown_host == [0, 0, 0]
    assert dev.ntotal == n and np.array_equal(bits(dev.centroids()), bits(host.centroids()))
    lists_dev, lists_host = sorted_lists(dev, nlist), sorted_lists(host, nlist)
    for c in range(nlist):
        assert np.array_equal(lists_dev[c], lists_host[c]), (metric, c)
    assert sum(l.size for l in lists_dev) == n
    if ref_ivf_available():
        ref = RefIvf(metric, d, nlist, rows[:half], ids[:half], exact_assignment=True)
        cent_ref, lists_ref = ref.export()
        ref.close()
        assert np.array_equal(bits(dev.centroids()), bits(cent_ref))
        cinv = oracle.l2_modules(cent_ref) if metric == 2 else None
        want = [list(np.asarray(l).tolist()) for l in lists_ref]
        for r in range(half, n):
            q = oracle.normalize_copy(rows[r])[0] if metric == 2 else rows[r]
            _, pos = lex_topk(oracle.dist_many(metric, q, cent_ref, cinv), 1)
            want[int(pos[0])].append(int(ids[r]))
        for c in range(nlist):
            assert np.array_equal(lists_dev[c], np.sort(np.array(want[c], np.int64))), (metric, c)
    dev.close()
    host.close()
