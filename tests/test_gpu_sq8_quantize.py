"""-m gpu: SQ8 codes and corrective offsets computed ON THE DEVICE from the index's float rows — hnsw_sq8_quantize.hip behind
rxgpu_hnsw_quantize_sq8, and behind GpuHnswMap::Quantize / points added to a quantised Map.
Bar: hnswlib::Quantizer::quantize row by row as oracle/oracle_sq8.c restates it (pinned to the real reference in tests/test_sq8_oracle.py):
codes compared as bytes, offsets as uint32 bit patterns.  No tolerance anywhere: a kernel that reorders a row's sums, fuses a multiply-add
or divides approximately differs in the offsets' bits in the first case."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 3, 31, 63, 64, 65, 100, 127, 128, 130, 257, 384, 512, 768, 1000, 1024, 1536, 4096]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def round4(d):
    return (d + 3) & ~3


@pytest.fixture(scope="module")
def sq8(oracle):
    from oracle.pyoracle import Sq8Oracle
    return Sq8Oracle(oracle)


def want_table(sq8, metric, p, rows):
    """The yardstick: Sq8Oracle.quantize row by row -> (codes [n][dim] u8, corr [n] f32)."""
    stored = [sq8.quantize(metric, p, x) for x in rows]
    return np.stack([c for c, _ in stored]), np.array([o for _, o in stored], np.float32)


def code_rows(ix, p, first, n):
    ix.hnsw_quantize_sq8(first, n, p["min_q"], p["alpha"], p["delta"], p["alpha_2"])


def same_table(got, want, what):
    (gc, go), (wc, wo) = got, want
    assert gc.dtype == np.uint8 and gc.shape == wc.shape, what
    bad = np.flatnonzero((gc != wc).any(axis=1))
    assert bad.size == 0, (what, "codes differ in rows", bad[:8].tolist())
    bad = np.flatnonzero(bits(go) != bits(wo))
    assert bad.size == 0, (what, "offset bits differ in rows", bad[:8].tolist(), bits(go)[bad[:4]].tolist(), bits(wo)[bad[:4]].tolist())


def norms_of(oracle, metric, rows):
    return oracle.l2_modules(rows) if metric == 2 else None


def uniform_rows(seed, n, d):
    """uniform in [-1.5, 1.5]: under the range [-1, 1] both clamps fire"""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (n, d)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", DIMS)
def test_all_dimensions(rxgpu, oracle, sq8, metric, d):
    n = 130
    rows = uniform_rows(100 * d + metric, n, d)
    p = sq8.params(-1.0, 1.0, d)
    want = want_table(sq8, metric, p, rows)
    assert want[0].min() == 0 and want[0].max() == 255
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, norms_of(oracle, metric, rows))
        ix.hnsw_read_sq8_quantize_stats()
        code_rows(ix, p, 0, n)
        same_table(ix.hnsw_read_sq8_rows(0, n), want, (metric, d))
        got_rows, launches, ms = ix.hnsw_read_sq8_quantize_stats()
        assert (got_rows, launches) == (n, 1) and ms > 0.0
        assert ix.hnsw_read_sq8_quantize_stats() == (0, 0, 0.0)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_row_counts_around_the_tile(rxgpu, oracle, sq8, metric, d, n):
    rows = uniform_rows(7 * n + d + metric, n, d)
    p = sq8.params(-1.0, 1.0, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, norms_of(oracle, metric, rows))
        code_rows(ix, p, 0, n)
        same_table(ix.hnsw_read_sq8_rows(0, n), want_table(sq8, metric, p, rows), (metric, d, n))


RANGES = [(-1.0, 1.0), (0.25, 0.251), (1000.0, 1001.5)]   # [-1, 1]; max_q - min_q = 1e-3; far from zero


def crafted_values(sq8, d):
    """Every code boundary of every range, one ulp to either side; zeros; subnormals."""
    vals = []
    for lo, hi in RANGES:
        p = sq8.params(lo, hi, d)
        edge = [np.float32(lo), np.float32(hi)] + [np.float32(np.float32(lo) + np.float32(k) * p["alpha"]) for k in range(256)]
        for v in edge:
            vals += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
    tiny = np.array([1, 2, 0x7FFFFF, 0x400000], np.uint32).view(np.float32)   # f32 subnormals: the smallest, the largest, one in between
    vals += [np.float32(0.0), np.float32(-0.0)] + list(tiny) + list(-tiny)
    return np.array(vals, np.float32)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_crafted_values(rxgpu, oracle, sq8, metric):
    d = 100
    vals = crafted_values(sq8, d)
    rng = np.random.default_rng(11)
    fill = (-len(vals)) % d
    body = np.concatenate([vals, rng.choice(vals, fill)]).reshape(-1, d)
    # huge and infinite components: a row each and in different columns (their offsets overflow / are NaN, which would hide everything else in the row)
    special = rng.uniform(-1.5, 1.5, (8, d)).astype(np.float32)
    for i, v in enumerate([1e30, -1e30, np.inf, -np.inf]):
        special[2 * i, 7 + 23 * i] = v
        special[2 * i + 1, [0, d - 1]] = v
    rows = np.concatenate([body, rng.permutation(vals)[:d * (len(vals) // d)].reshape(-1, d), special]).astype(np.float32)
    n = rows.shape[0]
    with np.errstate(all="ignore"):
        assert np.isinf(rows).sum() == 6 and not np.isnan(rows).any()
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, np.ones(n, np.float32) if metric == 2 else None)
        for lo, hi in RANGES:
            p = sq8.params(lo, hi, d)
            code_rows(ix, p, 0, n)
            same_table(ix.hnsw_read_sq8_rows(0, n), want_table(sq8, metric, p, rows), (metric, lo, hi))


# ---------------------------------------------------------------------------------------------------------------- ranges of rows
@pytest.mark.parametrize("metric", [0, 2])
def test_row_ranges_appends_and_growth(rxgpu, oracle, sq8, metric):
    d, n, extra = 100, 300, 77
    rows = uniform_rows(31 + metric, n + 2 * extra, d)
    p = sq8.params(-1.0, 1.0, d)
    p2 = sq8.params(-0.5, 0.75, d)
    with rxgpu.VectorIndex(metric, d, n + extra) as ix:
        ix.upload_rows(0, rows[:n], norms_of(oracle, metric, rows[:n]))
        code_rows(ix, p, 0, n)
        wc, wo = want_table(sq8, metric, p, rows[:n])
        same_table(ix.hnsw_read_sq8_rows(0, n), (wc, wo), "whole")
        # other floats for [a, b), then only [a, b) coded again (with other parameters, so that a row coded by mistake shows)
        a, b = 61, 199
        other = uniform_rows(99, b - a, d)
        ix.upload_rows(a, other, norms_of(oracle, metric, other))
        code_rows(ix, p2, a, b - a)
        nc, no = want_table(sq8, metric, p2, other)
        wc[a:b], wo[a:b] = nc, no
        same_table(ix.hnsw_read_sq8_rows(0, n), (wc, wo), "inner range")
        same_table(ix.hnsw_read_sq8_rows(a, b - a), (nc, no), "inner range, read alone")
        # append: first_row == rows that have codes
        ix.upload_rows(n, rows[n:n + extra], norms_of(oracle, metric, rows[n:n + extra]))
        assert ix.count == n + extra
        code_rows(ix, p, n, extra)
        tc, to = want_table(sq8, metric, p, rows[n:n + extra])
        wc, wo = np.concatenate([wc, tc]), np.concatenate([wo, to])
        same_table(ix.hnsw_read_sq8_rows(0, n + extra), (wc, wo), "appended")
        # a reserve that grows the capacity: the table grows with the next rows and keeps the earlier codes
        ix.reserve(n + 2 * extra + 500)
        ix.upload_rows(n + extra, rows[n + extra:], norms_of(oracle, metric, rows[n + extra:]))
        code_rows(ix, p, n + extra, extra)
        tc, to = want_table(sq8, metric, p, rows[n + extra:])
        same_table(ix.hnsw_read_sq8_rows(0, n + 2 * extra), (np.concatenate([wc, tc]), np.concatenate([wo, to])), "after a reserve")


def test_error_codes(rxgpu, oracle, sq8):
    d, n = 64, 200
    rows = uniform_rows(5, n, d)
    p = sq8.params(-1.0, 1.0, d)
    L = rxgpu.lib()
    args = (float(p["min_q"]), float(p["alpha"]), float(p["delta"]), float(p["alpha_2"]))
    codes, corr = np.zeros((n, d), np.uint8), np.zeros(n, np.float32)
    with rxgpu.VectorIndex(0, d, n) as ix:
        ix.upload_rows(0, rows, None)
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 0, 0, *args) == rxgpu.RXGPU_OK                      # n == 0
        assert L.rxgpu_hnsw_read_sq8_rows(ix._h, 0, 1, codes.ctypes.data, corr.ctypes.data) == rxgpu.RXGPU_ERR_LOGIC   # no codes yet
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 1, 10, *args) == rxgpu.RXGPU_ERR_PARAMS              # a hole in front
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 0, n + 1, *args) == rxgpu.RXGPU_ERR_PARAMS           # past count
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 0, 100, *args) == rxgpu.RXGPU_OK
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 101, 10, *args) == rxgpu.RXGPU_ERR_PARAMS            # a hole behind the coded rows
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 100, n - 99, *args) == rxgpu.RXGPU_ERR_PARAMS        # past count
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, n + 5, 1, *args) == rxgpu.RXGPU_ERR_PARAMS
        assert L.rxgpu_hnsw_read_sq8_rows(ix._h, 90, 11, codes.ctypes.data, corr.ctypes.data) == rxgpu.RXGPU_ERR_LOGIC   # row 100 has no code
        assert L.rxgpu_hnsw_read_sq8_rows(ix._h, 90, 10, None, corr.ctypes.data) == rxgpu.RXGPU_OK
        assert L.rxgpu_hnsw_read_sq8_rows(ix._h, 90, 10, codes.ctypes.data, None) == rxgpu.RXGPU_OK
        assert L.rxgpu_hnsw_quantize_sq8(ix._h, 100, n - 100, *args) == rxgpu.RXGPU_OK
        same_table(ix.hnsw_read_sq8_rows(0, n), want_table(sq8, 0, p, rows), "two halves")
    with rxgpu.ShardedVectorIndex(0, d, n, [0, 0]) as sx:
        sx.upload_rows(0, rows, None)
        assert L.rxgpu_hnsw_quantize_sq8(sx._h, 0, n, *args) == rxgpu.RXGPU_ERR_LOGIC
        assert L.rxgpu_hnsw_read_sq8_rows(sx._h, 0, 1, codes.ctypes.data, corr.ctypes.data) == rxgpu.RXGPU_ERR_LOGIC
        # the shard handles take the call
        first = 0
        for s in range(sx.shard_count):
            sh = sx.shard(s)
            cnt = sh.count
            code_rows(sh, p, 0, cnt)
            same_table(sh.hnsw_read_sq8_rows(0, cnt), want_table(sq8, 0, p, rows[first:first + cnt]), ("shard", s))
            first += cnt
        assert first == n


# ---------------------------------------------------------------------------------------------------------------- adopted storage
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [65, 100, 768])
@pytest.mark.parametrize("pad", [4, 12])
def test_adopted_strided_rows(rxgpu, oracle, sq8, metric, d, pad):
    """row_stride = dim (rounded up to 4) + 4 / + 12, NaN in every pad, in the guard rows in front of row 0 and behind the last: the result
    is the owned index's (and the oracle's)."""
    from .test_gpu_row_layout import device_layout
    n = 130
    rows = uniform_rows(17 * d + pad + metric, n, d)
    inv = norms_of(oracle, metric, rows)
    p = sq8.params(-1.0, 1.0, d)
    with rxgpu.VectorIndex(metric, d, n) as owned:
        owned.upload_rows(0, rows, inv)
        code_rows(owned, p, 0, n)
        want = owned.hnsw_read_sq8_rows(0, n)
    same_table(want, want_table(sq8, metric, p, rows), ("owned", metric, d))
    ptr, stride, keep, inv_ptr = device_layout(rows, inv, round4(d) + pad, guard=3)
    with rxgpu.VectorIndex(metric, d) as ix:
        ix.adopt_device_rows(ptr, n, stride, inv_ptr, keepalive=keep)
        assert ix.row_stride == stride == round4(d) + pad
        code_rows(ix, p, 0, n)
        same_table(ix.hnsw_read_sq8_rows(0, n), want, ("adopted", metric, d, pad))
        code_rows(ix, p, 40, 27)   # a range that starts inside a tile
        same_table(ix.hnsw_read_sq8_rows(0, n), want, ("adopted, inner range", metric, d, pad))
    del keep


# ---------------------------------------------------------------------------------------------------------------- search over the device's codes
def lattice(n, M=16):
    """A level-0 ring lattice in the shape of test_gpu_sq8's clique helper: node i is linked to the 2M nodes around it."""
    maxM0 = 2 * M
    links0 = np.zeros((n, 1 + maxM0), np.uint32)
    hops = np.concatenate([np.arange(1, M + 1), -np.arange(1, M + 1)])
    links0[:, 0] = maxM0
    links0[:, 1:] = (np.arange(n)[:, None] + hops[None, :]) % n
    return dict(links0=links0, upper_off=np.zeros(n + 1, np.uint64), upper=np.zeros(0, np.uint32), deleted=np.zeros(n, np.uint8), M=M, maxM0=maxM0,
                maxlevel=0, entry=0, num_deleted=0)


def quantised_queries(oracle, sq8, metric, p, raw):
    """prepareData (hnswalg.h:510-529) with the oracle's quantiser: codes, corrective offsets, normCoef"""
    qc, qo, qn = [], [], []
    for q in raw:
        coef = np.float32(1.0)
        if metric == 2:
            q, k_ = oracle.normalize_copy(q)
            coef = np.float32(k_)
        c, o = sq8.quantize(metric, p, q, float(np.float32(1.0) / coef))
        qc.append(c), qo.append(o), qn.append(coef)
    return np.stack(qc), np.array(qo, np.float32), np.array(qn, np.float32)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [128, 768])
def test_search_over_device_codes_equals_search_over_oracle_codes(rxgpu, oracle, sq8, metric, d):
    n, nq, k, ef = 2000, 8, 10, 64
    rng = np.random.default_rng(d + metric)
    rows = rng.normal(0, 0.25, (n, d)).astype(np.float32)
    inv = norms_of(oracle, metric, rows)
    g = lattice(n)
    raw = rng.normal(0, 0.25, (nq, d)).astype(np.float32)
    tables = {}
    for rg in ((-0.6, 0.6), (-0.3, 0.45)):
        p = sq8.params(rg[0], rg[1], d)
        tables[rg] = (p, want_table(sq8, metric, p, rows), quantised_queries(oracle, sq8, metric, p, raw))
    with rxgpu.VectorIndex(metric, d, n) as dev, rxgpu.VectorIndex(metric, d, n) as orc:
        for ix in (dev, orc):
            ix.upload_rows(0, rows, inv)
            ix.hnsw_attach_graph(g)
        for rg, (p, (wc, wo), (qc, qo, qn)) in tables.items():   # the second round re-codes an index that has codes (and a resident kernel)
            code_rows(dev, p, 0, n)
            orc.hnsw_attach_sq8(wc, wo, float(p["alpha_2"]))
            gd, gr, gcnt = dev.hnsw_search_knn_sq8(qc, qo, qn, k, ef)
            wd, wr, wcnt = orc.hnsw_search_knn_sq8(qc, qo, qn, k, ef)
            assert np.array_equal(gcnt, wcnt) and (gcnt == k).all(), (metric, d, rg)
            assert np.array_equal(gr, wr) and np.array_equal(bits(gd), bits(wd)), (metric, d, rg)
            if d == 128:   # one query through the resident kernel: before and after the re-coding it answers from the table of the moment
                pd, pr, pc, served = dev.hnsw_search_knn_sq8_posted(qc[0], qo[0], qn[0], k, ef)
                assert served and pc == int(wcnt[0]), (metric, rg)
                assert np.array_equal(pr[:pc], wr[0, :pc]) and np.array_equal(bits(pd[:pc]), bits(wd[0, :pc])), (metric, rg)


# ---------------------------------------------------------------------------------------------------------------- the Map
def map_table(m, rxgpu, cnt):
    """the Map's code table as the device holds it"""
    codes, corr = np.empty((cnt, m.dim), np.uint8), np.empty(cnt, np.float32)
    rc = rxgpu.lib().rxgpu_hnsw_read_sq8_rows(m.device_index, 0, cnt, codes.ctypes.data, corr.ctypes.data)
    assert rc == rxgpu.RXGPU_OK, rc
    return codes, corr


def device_stats(m, rxgpu):
    rows, launches, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
    assert rxgpu.lib().rxgpu_hnsw_read_sq8_quantize_stats(m.device_index, C.byref(rows), C.byref(launches), C.byref(ms)) == rxgpu.RXGPU_OK
    return int(rows.value), int(launches.value)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("mode", ["device", "host"])
def test_map_codes_on_the_device(rxgpu, oracle, sq8, monkeypatch, metric, mode):
    from reindexer_amd import hostapi
    if mode == "host":
        monkeypatch.setenv("RXGPU_SQ8_QUANTIZE", "host")
    else:
        monkeypatch.delenv("RXGPU_SQ8_QUANTIZE", raising=False)
    n, d, extra = 1500, 96, 200
    rng = np.random.default_rng(40 + metric)
    rows = rng.normal(0, 0.25, (n + extra, d)).astype(np.float32)
    labels = (np.arange(n + extra, dtype=np.uint64) << np.uint64(32)) | np.uint64(3)
    q = rng.normal(0, 0.25, d).astype(np.float32)
    norm = None
    if metric == 2:
        q, k_ = oracle.normalize_copy(q)
        norm = float(np.float32(1.0) / np.float32(k_))
    m = hostapi.GpuHnswMap(metric, d, n + extra, M=8, ef_construction=60)
    try:
        m.add(rows[:n], labels[:n])
        m.search_knn_norm(q, 5, 32, norm)   # the float rows and the graph are on the device
        assert m.device_coded_rows() == 0
        min_q, max_q = -0.6, 0.6
        p = sq8.params(min_q, max_q, d)
        m.quantize(min_q, max_q)
        m.search_knn_norm(q, 5, 32, norm)
        coded = n if mode == "device" else 0
        assert m.device_coded_rows() == coded
        assert device_stats(m, rxgpu) == (coded, 1 if coded else 0)
        vecs = np.array(m.export_graph(with_views=True)["vectors"])
        assert vecs.shape[0] == n
        same_table(map_table(m, rxgpu, vecs.shape[0]), want_table(sq8, metric, p, vecs), (metric, mode, "quantize"))
        # points added to the quantised Map: the appended rows are coded on the device too (or the whole table again, where the change
        # tracker gave up); rows whose links changed keep their codes
        m.add(rows[n:], labels[n:])
        m.search_knn_norm(q, 5, 32, norm)
        more, launches = device_stats(m, rxgpu)
        if mode == "device":
            assert (more, launches) in ((extra, 1), (n + extra, 1)), (more, launches)
            assert m.device_coded_rows() == n + more
        else:
            assert (more, launches) == (0, 0) and m.device_coded_rows() == 0
        vecs = np.array(m.export_graph(with_views=True)["vectors"])
        assert vecs.shape[0] == n + extra
        same_table(map_table(m, rxgpu, vecs.shape[0]), want_table(sq8, metric, p, vecs), (metric, mode, "added"))
        # a new range: the whole table again
        p = sq8.params(-0.4, 0.5, d)
        m.quantize(-0.4, 0.5)
        m.search_knn_norm(q, 5, 32, norm)
        assert device_stats(m, rxgpu) == ((n + extra, 1) if mode == "device" else (0, 0))
        same_table(map_table(m, rxgpu, vecs.shape[0]), want_table(sq8, metric, p, vecs), (metric, mode, "new range"))
    finally:
        m.close()
