"""The default scan policy of a single query (rxgpu_knn_chains.hip: scan_policy_pruned / enqueue_knn).

RXGPU_SCAN_BF16 unset = automatic: nq == 1 on an index of at least RXGPU_SCAN_BF16_MIN_BYTES (default 1 GiB) of f32 rows takes the bf16-pruned
scan where the dimension is supported, the shadow fits and the row statistics are finite; 0 = the f32 paths always; 1 = forced on.  The
yardstick of every comparison here is THE SAME BUILD with RXGPU_SCAN_BF16=0: turning the default on must change no output bit, for finite
and for non-finite inputs alike.  The path taken is observed through the profile slots ("scan" = the f32 knn_scan_fixed launch and nothing
else, "scan_bf16" = the bf16 kernel)."""
import numpy as np
import pytest

from .conftest import make_corpus

METRICS = [0, 1, 2]   # l2, ip, cosine


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU: the decision itself
def test_policy_function_decides_as_documented(monkeypatch):
    from reindexer_amd import capi
    capi.lib()
    GiB = 1 << 30
    rows_1g = GiB // (768 * 4) + 1   # just past 1 GiB of f32 rows at 768 dims
    monkeypatch.delenv("RXGPU_SCAN_BF16", raising=False)
    monkeypatch.delenv("RXGPU_SCAN_BF16_MIN_BYTES", raising=False)
    # automatic: size
    assert capi.scan_policy(10_000_000, 768)
    assert capi.scan_policy(rows_1g, 768)
    assert not capi.scan_policy(rows_1g - 2, 768)
    assert not capi.scan_policy(200_000, 768)          # 614 MB: the sizes whose f32 profile slot other tests pin
    assert not capi.scan_policy(100_000, 128)
    # automatic: only single queries, only with a shadow and finite statistics, only supported dimensions (ld = dim rounded up to 64 must be 128 x {1,2,3,4,6,8})
    assert not capi.scan_policy(10_000_000, 768, nq=2)
    assert not capi.scan_policy(10_000_000, 768, nq=8)
    assert not capi.scan_policy(10_000_000, 768, shadow_available=False)
    assert not capi.scan_policy(10_000_000, 768, stats_finite=False)
    assert not capi.scan_policy(40_000_000, 64) and not capi.scan_policy(10_000_000, 640) and not capi.scan_policy(10_000_000, 1100)
    assert capi.scan_policy(40_000_000, 100) and capi.scan_policy(10_000_000, 1024) and capi.scan_policy(10_000_000, 750)
    # the threshold moves with RXGPU_SCAN_BF16_MIN_BYTES
    monkeypatch.setenv("RXGPU_SCAN_BF16_MIN_BYTES", str(1000 * 128 * 4))
    assert capi.scan_policy(1000, 128) and not capi.scan_policy(999, 128)
    monkeypatch.setenv("RXGPU_SCAN_BF16_MIN_BYTES", str(64 * GiB))
    assert not capi.scan_policy(10_000_000, 768)
    monkeypatch.delenv("RXGPU_SCAN_BF16_MIN_BYTES")
    # forced off: never
    monkeypatch.setenv("RXGPU_SCAN_BF16", "0")
    assert not capi.scan_policy(10_000_000, 768) and not capi.scan_policy(100_000_000, 128)
    # forced on: up to 8 queries at any size, whatever the statistics say; still needs the dimension and the shadow
    monkeypatch.setenv("RXGPU_SCAN_BF16", "1")
    assert capi.scan_policy(100, 128) and capi.scan_policy(100, 128, nq=8) and capi.scan_policy(100, 128, stats_finite=False)
    assert not capi.scan_policy(100, 128, nq=9) and not capi.scan_policy(100, 64) and not capi.scan_policy(100, 128, shadow_available=False)


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def _auto(monkeypatch, min_bytes=1):
    monkeypatch.delenv("RXGPU_SCAN_BF16", raising=False)
    monkeypatch.setenv("RXGPU_SCAN_BF16_MIN_BYTES", str(min_bytes))


def _off(monkeypatch):
    monkeypatch.setenv("RXGPU_SCAN_BF16", "0")


def _slots(ix, fn):
    """(result of fn, launches of the f32 scan slot, launches of the bf16 scan slot) with profiling on around fn"""
    ix.profile_enable(True)
    out = fn()
    n_f32, n_bf16 = ix.profile_read("scan")[0], ix.profile_read("scan_bf16")[0]
    ix.profile_enable(False)
    return out, n_f32, n_bf16


def _same(a, b, what):
    (da, ra, ca), (db, rb, cb) = a, b
    assert np.array_equal(ca, cb), what
    assert np.array_equal(ra, rb), what
    assert np.array_equal(bits(da), bits(db)), what


def _corpus(oracle, metric, seed, n, d):
    rows = make_corpus(seed, n, d)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    q = make_corpus(seed + 1000, 6, d)
    if metric == 2:
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    return rows, inv, q


@gpu
def test_automatic_mode_follows_size_switch_dimension_and_batch(rxgpu, oracle, monkeypatch):
    n, d = 20_000, 128
    rows, _, q = _corpus(oracle, 1, 3, n, d)
    size = n * d * 4
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _auto(monkeypatch, size)       # at the threshold: the pruned scan
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert (f32, b16) == (0, 1)
        _auto(monkeypatch, size + 1)   # below it: the f32 scan
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert (f32, b16) == (1, 0)
        monkeypatch.delenv("RXGPU_SCAN_BF16_MIN_BYTES")   # the built-in threshold (>= 1 GiB): a small index keeps the f32 kernel
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert (f32, b16) == (1, 0)
        _auto(monkeypatch, 1)
        ix.profile_enable(True)        # nq >= 2: the batched path as before (its nomination GEMM, neither single-query slot)
        ix.search_knn(q[:3], 11)
        assert (ix.profile_read("gemm")[0], ix.profile_read("scan")[0], ix.profile_read("scan_bf16")[0]) == (1, 0, 0)
        ix.profile_enable(False)
        _off(monkeypatch)              # forced off wins over any threshold
        monkeypatch.setenv("RXGPU_SCAN_BF16_MIN_BYTES", "1")
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert (f32, b16) == (1, 0)
    d2 = 64   # ld = 64: not a dimension of the bf16 scan
    rows2 = make_corpus(4, 5000, d2)
    with rxgpu.VectorIndex(1, d2, 5000) as ix:
        ix.upload_rows(0, rows2)
        _auto(monkeypatch, 1)
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(make_corpus(5, 1, d2), 11))
        assert (f32, b16) == (1, 0)


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", [(128, 30_000), (768, 12_000)])
def test_automatic_mode_returns_the_bits_of_the_f32_scan(rxgpu, oracle, monkeypatch, metric, d, n):
    rows, inv, q = _corpus(oracle, metric, 10 + d + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)

        def compare(what):
            for kk in (1, 11, 64):
                for qi in range(3):
                    _auto(monkeypatch)
                    got, f32, b16 = _slots(ix, lambda: ix.search_knn(q[qi:qi + 1], kk))
                    assert (f32, b16) == (0, 1), what
                    _off(monkeypatch)
                    want, f32, b16 = _slots(ix, lambda: ix.search_knn(q[qi:qi + 1], kk))
                    assert (f32, b16) == (1, 0), what
                    _same(got, want, (what, metric, d, kk, qi))

        compare("fresh")
        _auto(monkeypatch)
        ix.search_knn(q[:1], 11)                       # statistics and shadow exist: the mutations below keep them up to date in place
        new = make_corpus(77 + metric, 40, d)
        new[0] = q[0] / (np.linalg.norm(q[0]) or 1.0) if metric == 2 else q[0]   # a new best row for query 0
        ix.upload_rows(100, new, oracle.l2_modules(new) if metric == 2 else None)
        compare("upload_rows over existing rows")
        ix.move_row(n - 1, 100)
        compare("move_row")
        ix.truncate(n - 1)
        compare("truncate")


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_automatic_mode_through_the_device_entry_point_and_two_shards(rxgpu, oracle, monkeypatch, metric):
    import torch
    n, d, kk = 24_000, 128, 11
    rows, inv, q = _corpus(oracle, metric, 50 + metric, n, d)
    dev = torch.device("cuda", 0)
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.ShardedVectorIndex(metric, d, n, [0, 0]) as sx:
        ix.upload_rows(0, rows, inv)
        sx.upload_rows(0, rows, inv)
        dq = torch.from_numpy(q).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def device_search(qi):
            od = torch.empty((1, kk), dtype=torch.float32, device=dev)
            orow = torch.empty((1, kk), dtype=torch.int32, device=dev)
            oc = torch.zeros(1, dtype=torch.int32, device=dev)
            ix.search_knn_device(dq.data_ptr() + qi * d * 4, 1, kk, od.data_ptr(), orow.data_ptr(), oc.data_ptr(), stream)
            torch.cuda.synchronize(dev)
            return od.cpu().numpy(), orow.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)

        for qi in range(3):
            _off(monkeypatch)
            want = ix.search_knn(q[qi:qi + 1], kk)
            want_sharded = sx.search_knn(q[qi:qi + 1], kk)
            _same(want_sharded, want, ("sharded f32 vs one index", metric, qi))
            _auto(monkeypatch)
            got, f32, b16 = _slots(ix, lambda: device_search(qi))
            assert (f32, b16) == (0, 1)
            _same(got, want, ("rxgpu_search_knn_device", metric, qi))
            views = [sx.shard(s) for s in range(2)]
            for v in views:
                v.profile_enable(True)
            got_sharded = sx.search_knn(q[qi:qi + 1], kk)
            assert [(v.profile_read("scan")[0], v.profile_read("scan_bf16")[0]) for v in views] == [(0, 1), (0, 1)]
            for v in views:
                v.profile_enable(False)
            _same(got_sharded, want, ("two shards", metric, qi))


def _nonfinite_rows(kind, d):
    if kind == "nan":
        r = np.full(d, 0.1, np.float32)
        r[d // 2] = np.nan
    elif kind == "inf":
        r = np.full(d, 0.1, np.float32)
        r[3] = np.inf
    else:   # finite entries whose |x|^2 overflows
        r = np.full(d, 3e38, np.float32)
    return r


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf", "3e38"])
@pytest.mark.parametrize("where", ["inside_first_kk", "outside_first_kk"])
def test_nonfinite_rows_keep_the_index_on_the_f32_scan(rxgpu, oracle, monkeypatch, metric, kind, where):
    n, d, kk = 9_000, 128, 11
    rows, _, q = _corpus(oracle, metric, 90 + metric, n, d)
    rows[3 if where == "inside_first_kk" else 5_000] = _nonfinite_rows(kind, d)
    with np.errstate(all="ignore"):
        inv = oracle.l2_modules(rows) if metric == 2 else None
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for qi in range(2):
            _off(monkeypatch)
            want = ix.search_knn(q[qi:qi + 1], kk)
            _auto(monkeypatch)
            got, f32, b16 = _slots(ix, lambda: ix.search_knn(q[qi:qi + 1], kk))
            assert (f32, b16) == (1, 0), "an index with a non-finite row statistic must take the f32 scan"
            _same(got, want, (metric, kind, where, qi))


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_nonfinite_row_uploaded_after_the_statistics_exist(rxgpu, oracle, monkeypatch, metric):
    """upload_rows folds new rows into the cached statistics: the index must notice a non-finite one there too."""
    n, d, kk = 9_000, 128, 11
    rows, inv, q = _corpus(oracle, metric, 95 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _auto(monkeypatch)
        _, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], kk))
        assert (f32, b16) == (0, 1)
        bad = _nonfinite_rows("nan", d)[None, :]
        with np.errstate(all="ignore"):
            ix.upload_rows(4_000, bad, oracle.l2_modules(bad) if metric == 2 else None)
        _off(monkeypatch)
        want = ix.search_knn(q[:1], kk)
        _auto(monkeypatch)
        got, f32, b16 = _slots(ix, lambda: ix.search_knn(q[:1], kk))
        assert (f32, b16) == (1, 0)
        _same(got, want, metric)


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf", "zero"])
def test_nonfinite_queries_are_answered_by_the_exact_scan_behind_the_gate(rxgpu, oracle, monkeypatch, metric, kind):
    """A NaN / infinite query has no finite bound: the pruned path must hand it, on the device, to the exact scan it keeps behind its gate, and
    the caller gets what the f32 path gives.  An all-zero query (what a cosine caller sends for a null vector) ties every row."""
    n, d, kk = 9_000, 128, 11
    rows, inv, q = _corpus(oracle, metric, 120 + metric, n, d)
    query = q[0].copy()
    if kind == "nan":
        query[7] = np.nan
    elif kind == "inf":
        query[7] = np.inf
    else:
        query[:] = 0.0
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _off(monkeypatch)
        want = ix.search_knn(query[None, :], kk)
        _auto(monkeypatch)
        got, f32, b16 = _slots(ix, lambda: ix.search_knn(query[None, :], kk))
        assert (f32, b16) == (0, 1)   # the index is fine: the query took the pruned path and was re-routed on the device
        _same(got, want, (metric, kind))
        got2 = ix.search_knn(q[1:2], kk)   # and the context is fit for the next, ordinary query
        _off(monkeypatch)
        _same(got2, ix.search_knn(q[1:2], kk), (metric, kind, "next query"))
