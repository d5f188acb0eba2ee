"""-m gpu: the int8 shadow tier of the single-query scan (knn_scan_i8.hip, knn_query_prep_i8; arithmetic and bound in knn_i8_quant.h).

The yardstick of every comparison is THE SAME BUILD with RXGPU_SCAN_BF16=0: counts, rows and distance bits must be equal.  The path taken
is observed through the profile slots ("scan" = the f32 knn_scan_fixed launch and nothing else, "scan_bf16" the bf16 kernel, "scan_i8" the
int8 kernel) and through rxgpu_index_last_candidates: count <= cap means the pruned chain, not the exact scan behind its gate, produced
what was compared."""
import numpy as np
import pytest

from .conftest import make_corpus

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]   # l2, ip, cosine
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES")


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


def _slots(ix, fn):
    """(result of fn, (launches of the f32 / bf16 / int8 scan slots), (candidates, cap)) with profiling on around fn"""
    ix.profile_enable(True)
    out = fn()
    n = tuple(ix.profile_read(s)[0] for s in ("scan", "scan_bf16", "scan_i8"))
    cand = ix.last_candidates()
    ix.profile_enable(False)
    return out, n, cand


def _same(a, b, what):
    (da, ra, ca), (db, rb, cb) = a, b
    assert np.array_equal(ca, cb), what
    assert np.array_equal(ra, rb), what
    assert np.array_equal(bits(da), bits(db)), what


def _corpus(oracle, metric, seed, n, d, nq=3):
    rows = make_corpus(seed, n, d)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    q = make_corpus(seed + 1000, nq, d)
    if metric == 2:
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    return rows, inv, q


def _forced_equals_f32(ix, monkeypatch, query, kk, what, pruned=True):
    """one query through the forced int8 tier and through the f32 scan; returns the candidates of the forced call"""
    _env(monkeypatch, I8=1)
    got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn(query[None, :], kk))
    assert slots == (0, 0, 1), what
    _env(monkeypatch, BF16=0)
    want, slots, _ = _slots(ix, lambda: ix.search_knn(query[None, :], kk))
    assert slots == (1, 0, 0), what
    _same(got, want, what)
    assert cap >= 64, what
    if pruned:
        assert cand <= cap, (what, "the candidate list overflowed", cand, cap)
    return cand, cap


# ---------------------------------------------------------------------------------------------------------------- 1. the forced tier
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", [(768, 12_007), (256, 30_000), (1024, 4_000), (750, 5_000)])
def test_forced_tier_returns_the_bits_of_the_f32_scan(rxgpu, oracle, monkeypatch, metric, d, n):
    rows, inv, q = _corpus(oracle, metric, 20 + d + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        worst = {}
        for kk in (1, 11, 64):
            for qi in range(3):
                cand, cap = _forced_equals_f32(ix, monkeypatch, q[qi], kk, (metric, d, n, kk, qi))
                worst[kk] = max(worst.get(kk, 0), cand)
        print(f"candidates metric={metric} d={d} n={n}: {worst} (cap {cap})")


@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_on_seven_rows(rxgpu, oracle, monkeypatch, metric):
    rows, inv, q = _corpus(oracle, metric, 40 + metric, 7, 256)
    with rxgpu.VectorIndex(metric, 256, 16) as ix:
        ix.upload_rows(0, rows, inv)
        for qi in range(3):
            _forced_equals_f32(ix, monkeypatch, q[qi], 11, (metric, qi))   # kk > n


# ---------------------------------------------------------------------------------------------------------------- 2. automatic mode
def test_automatic_mode_follows_both_thresholds_the_dimension_the_batch_and_the_switches(rxgpu, oracle, monkeypatch):
    n, d = 20_000, 256
    rows, _, q = _corpus(oracle, 1, 3, n, d)
    size = n * d * 4
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=size)          # at both thresholds: the int8 tier
        got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert slots == (0, 0, 1) and cand <= cap
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=size + 1)      # below the int8 threshold: the bf16 tier
        got16, slots, _ = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert slots == (0, 1, 0)
        _same(got, got16, "int8 tier vs bf16 tier")
        _env(monkeypatch, BF16_MIN_BYTES=1)                             # only the bf16 threshold lowered: the bf16 tier
        assert _slots(ix, lambda: ix.search_knn(q[:1], 11))[1] == (0, 1, 0)
        _env(monkeypatch, I8_MIN_BYTES=1)                               # the int8 threshold alone does not widen the automatic mode
        assert _slots(ix, lambda: ix.search_knn(q[:1], 11))[1] == (1, 0, 0)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
        ix.profile_enable(True)                                         # nq = 3: the batched path, none of the single-query slots
        ix.search_knn(q[:3], 11)
        assert tuple(ix.profile_read(s)[0] for s in ("gemm", "scan", "scan_bf16", "scan_i8")) == (1, 0, 0, 0)
        ix.profile_enable(False)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1, I8=0)       # this tier off
        assert _slots(ix, lambda: ix.search_knn(q[:1], 11))[1] == (0, 1, 0)
        _env(monkeypatch, BF16=0, I8=1)                                 # the f32 paths win over a forced int8 tier
        want, slots, _ = _slots(ix, lambda: ix.search_knn(q[:1], 11))
        assert slots == (1, 0, 0)
        _same(got, want, "int8 tier vs f32 scan")
        _env(monkeypatch, BF16=1, I8=1)                                 # RXGPU_SCAN_BF16=1 means the bf16 kernel
        assert _slots(ix, lambda: ix.search_knn(q[:1], 11))[1] == (0, 1, 0)
    for d2, want in ((128, (0, 1, 0)), (1100, (1, 0, 0))):   # 128: a code row is no shorter than the bf16 row; 1100: no tier serves it
        with rxgpu.VectorIndex(1, d2, 5000) as ix:
            ix.upload_rows(0, make_corpus(4, 5000, d2))
            _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
            assert _slots(ix, lambda: ix.search_knn(make_corpus(5, 1, d2), 11))[1] == want


# ---------------------------------------------------------------------------------------------------------------- 3. mass ties
@pytest.mark.parametrize("metric", [1, 0])
def test_mass_ties_overflow_the_list_and_the_gated_scan_answers(rxgpu, monkeypatch, metric):
    """Rows in {-1, 0, 1} quantise without residual, so the window is a few ulps: every row tied at the kk-th distance is a candidate.  ip: a
    query with one non-zero component ties a third of the rows at each of three distances, the zero query ties all of them.  L2: rows in
    {-1, 1} (all of one norm) tie completely against the zero query."""
    rng = np.random.default_rng(5)
    n, d = 60_000, 256
    rows = (rng.integers(-1, 2, (n, d)) if metric == 1 else rng.integers(0, 2, (n, d)) * 2 - 1).astype(np.float32)
    assert set(np.unique(rows)) <= {-1.0, 0.0, 1.0}
    unit = np.zeros(d, np.float32)
    unit[17] = 1.0
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows)
        for name, query in (("zero", np.zeros(d, np.float32)), ("unit", unit)):
            if metric == 0 and name == "unit":
                continue
            cand, cap = _forced_equals_f32(ix, monkeypatch, query, 11, (metric, name), pruned=False)
            assert cand > cap, (metric, name, cand, cap)
        q = rng.integers(-1, 2, d).astype(np.float32)                   # an ordinary query over the same rows: exact as well
        _forced_equals_f32(ix, monkeypatch, q, 11, (metric, "ordinary"), pruned=False)


# ---------------------------------------------------------------------------------------------------------------- 4. adversarial magnitudes
@pytest.mark.parametrize("metric", [0, 1])
def test_adversarial_magnitudes_and_mutations(rxgpu, monkeypatch, metric):
    rng = np.random.default_rng(78)
    n, d = 20_000, 256
    rows = (rng.normal(0, 1, (n, d)) * np.exp(rng.uniform(-14, 14, (n, 1)))).astype(np.float32)
    rows[1000:1200] = rows[0] * (1 + rng.uniform(-1e-4, 1e-4, (200, 1))).astype(np.float32)
    rows[2000:2050] = rows[0]
    rows[3000] = rng.normal(0, 1, d)
    rows[3000, 5] *= 1e6                                                 # one component 10^6 x the others
    rows[3001] = 0.0                                                     # an all-zero row
    queries = (rng.normal(0, 1, (6, d)) * np.exp(rng.uniform(-6, 6, (6, 1)))).astype(np.float32)
    queries[0] = rows[0]                                                 # a query equal to a stored row
    queries[1] = rows[3000]
    queries[2] = 0.0                                                     # an all-zero query
    with rxgpu.VectorIndex(metric, d, n + 10) as ix:
        ix.upload_rows(0, rows)
        for qi in range(6):
            _forced_equals_f32(ix, monkeypatch, queries[qi], 11, (metric, qi), pruned=False)
        new = rows[5:45].copy()
        new[0] = queries[3]                                              # a new best row for query 3
        ix.upload_rows(5, new)
        for qi in (3, 4):
            _forced_equals_f32(ix, monkeypatch, queries[qi], 5, (metric, "upload_rows over existing rows", qi), pruned=False)
        ix.move_row(n - 1, 5)
        for qi in (3, 4):
            _forced_equals_f32(ix, monkeypatch, queries[qi], 5, (metric, "move_row", qi), pruned=False)
        ix.truncate(n - 1)
        for qi in (3, 4):
            _forced_equals_f32(ix, monkeypatch, queries[qi], 5, (metric, "truncate", qi), pruned=False)


@pytest.mark.parametrize("metric", METRICS)
def test_mutations_keep_the_shadow_in_step(rxgpu, oracle, monkeypatch, metric):
    """the same mutations on the benchmark's distribution, where the pruned chain itself (count <= cap) must stay exact"""
    n, d = 12_000, 256
    rows, inv, q = _corpus(oracle, metric, 60 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)
        _forced_equals_f32(ix, monkeypatch, q[0], 11, (metric, "fresh"))
        new = make_corpus(77 + metric, 40, d)
        new[0] = q[0] / (np.linalg.norm(q[0]) or 1.0) if metric == 2 else q[0]   # a new best row for query 0
        ix.upload_rows(100, new, oracle.l2_modules(new) if metric == 2 else None)
        _forced_equals_f32(ix, monkeypatch, q[0], 11, (metric, "upload_rows over existing rows"))
        ix.move_row(100, 7)                                              # the best row moves
        _forced_equals_f32(ix, monkeypatch, q[0], 11, (metric, "move_row"))
        ix.truncate(n - 1)
        _forced_equals_f32(ix, monkeypatch, q[0], 11, (metric, "truncate"))
        ix.upload_rows(n - 1, new[:5], oracle.l2_modules(new[:5]) if metric == 2 else None)   # growing again
        _forced_equals_f32(ix, monkeypatch, q[1], 11, (metric, "upload_rows past the end"))


# ---------------------------------------------------------------------------------------------------------------- 5. non-finite
def _nonfinite_row(kind, d):
    r = np.full(d, 0.1, np.float32)
    r[d // 2] = np.nan if kind == "nan" else np.inf
    return r


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_rows_keep_the_index_off_the_tier(rxgpu, oracle, monkeypatch, metric, kind):
    n, d, kk = 9_000, 256, 11
    rows, _, q = _corpus(oracle, metric, 90 + metric, n, d)
    rows[5_000] = _nonfinite_row(kind, d)
    with np.errstate(all="ignore"):
        inv = oracle.l2_modules(rows) if metric == 2 else None
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, BF16=0)
        want = ix.search_knn(q[:1], kk)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
        got, slots, _ = _slots(ix, lambda: ix.search_knn(q[:1], kk))
        assert slots == (1, 0, 0), "an index with a non-finite row statistic must take the f32 scan"
        _same(got, want, (metric, kind))
        _forced_equals_f32(ix, monkeypatch, q[0], kk, (metric, kind, "forced"), pruned=False)   # forced: the gate answers, same bits


@pytest.mark.parametrize("metric", METRICS)
def test_nonfinite_row_uploaded_after_the_shadow_exists(rxgpu, oracle, monkeypatch, metric):
    n, d, kk = 9_000, 256, 11
    rows, inv, q = _corpus(oracle, metric, 95 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
        assert _slots(ix, lambda: ix.search_knn(q[:1], kk))[1] == (0, 0, 1)
        bad = _nonfinite_row("nan", d)[None, :]
        with np.errstate(all="ignore"):
            ix.upload_rows(4_000, bad, oracle.l2_modules(bad) if metric == 2 else None)
        _env(monkeypatch, BF16=0)
        want = ix.search_knn(q[:1], kk)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
        got, slots, _ = _slots(ix, lambda: ix.search_knn(q[:1], kk))
        assert slots == (1, 0, 0)
        _same(got, want, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_queries_through_the_forced_tier(rxgpu, oracle, monkeypatch, metric, kind):
    n, d, kk = 9_000, 256, 11
    rows, inv, q = _corpus(oracle, metric, 120 + metric, n, d)
    query = q[0].copy()
    query[7] = np.nan if kind == "nan" else np.inf
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        cand, cap = _forced_equals_f32(ix, monkeypatch, query, kk, (metric, kind), pruned=False)
        assert cand == cap + 1   # no finite bound: re-routed on the device
        _forced_equals_f32(ix, monkeypatch, q[1], kk, (metric, kind, "next query"))   # the context is fit for the next, ordinary query


# ---------------------------------------------------------------------------------------------------------------- 6. entry points
@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_through_the_device_entry_point_and_two_shards(rxgpu, oracle, monkeypatch, metric):
    import torch
    n, d, kk = 24_000, 256, 11
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
            _env(monkeypatch, BF16=0)
            want = ix.search_knn(q[qi:qi + 1], kk)
            _same(sx.search_knn(q[qi:qi + 1], kk), want, ("sharded f32 vs one index", metric, qi))
            _env(monkeypatch, I8=1)
            got, slots, _ = _slots(ix, lambda: device_search(qi))
            assert slots == (0, 0, 1)
            _same(got, want, ("rxgpu_search_knn_device", metric, qi))
            views = [sx.shard(s) for s in range(2)]
            for v in views:
                v.profile_enable(True)
            got_sharded = sx.search_knn(q[qi:qi + 1], kk)
            assert [tuple(v.profile_read(s)[0] for s in ("scan", "scan_bf16", "scan_i8")) for v in views] == [(0, 0, 1), (0, 0, 1)]
            for v in views:
                v.profile_enable(False)
            _same(got_sharded, want, ("two shards", metric, qi))
