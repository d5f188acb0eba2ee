"""-m gpu: the int8 shadow tier of the searches over a ROW LIST (knn_scan_i8_subset in knn_scan_i8.hip, enqueue_knn_pruned_i8 with a row list): the
pre-filtered search (rxgpu_search_knn_subset / _bitmap / _subset_device), IVF (rxgpu_search_knn_lists) and their per-shard calls.

The yardstick of every comparison is THE SAME BUILD with RXGPU_SCAN_BF16=0, the f32 subset path that test_gpu_prefilter.py pins to the
oracle: counts, rows and distance bits must be equal.  The path taken is observed through the profile slots ("scan_subset" = the f32
gather scan of a call the tier did not serve, "scan_i8_subset" the int8 gather kernel, "fallback_scan" the exact subset scan behind the
tier's gate, counted when the gate opened) and through rxgpu_index_last_candidates: count <= cap means the pruned chain, not the exact scan
behind its gate, produced what was compared."""
import numpy as np
import pytest

from .conftest import make_corpus

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]   # l2, ip, cosine
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_WG_PER_CU")
SLOTS = ("scan_subset", "scan_i8_subset", "fallback_scan")


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


def _slots(ix, fn):
    """(result of fn, (launches of the f32 subset scan, of the int8 subset scan, opened gates), (candidates, cap)) with profiling on around fn"""
    ix.profile_enable(True)
    out = fn()
    n = tuple(ix.profile_read(s)[0] for s in SLOTS)
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


def _list(rng, n, density, ends=False):
    keep = rng.random(n) < density
    if ends:
        keep[0] = keep[n - 1] = True
    return np.flatnonzero(keep).astype(np.uint32)


def _trim(res):
    """only what the call defines: the first count entries of every query"""
    d, r, c = res
    d, r = d.copy(), r.copy()
    for q in range(d.shape[0]):
        d[q, int(c[q]):] = 0
        r[q, int(c[q]):] = 0
    return d, r, c


def _forced_equals_f32(ix, monkeypatch, query, kk, ids, what, pruned=True):
    """one query over the list through the forced int8 tier and through the f32 subset scan; returns (f32 result, candidates, cap)"""
    query = np.atleast_2d(query)
    _env(monkeypatch, I8=1)
    got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn_subset(query, kk, ids))
    assert slots == ((0, 1, 0) if pruned else (0, 1, int(cand > cap))), (what, slots, cand, cap)
    _env(monkeypatch, BF16=0)
    want, slots, _ = _slots(ix, lambda: ix.search_knn_subset(query, kk, ids))
    assert slots == (1, 0, 0), what
    got, want = _trim(got), _trim(want)
    assert int(want[2][0]) == min(kk, ids.size), what
    _same(got, want, what)
    assert cap == min(4096, max(64, (ids.size + 63) // 64 * 64)), what
    if pruned:
        assert cand <= cap, (what, "the candidate list overflowed", cand, cap)
    return want, cand, cap


# ---------------------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", [(768, 12_007), (256, 30_000), (1024, 4_000), (750, 5_000)])
def test_forced_tier_returns_the_bits_of_the_f32_subset_scan(rxgpu, oracle, monkeypatch, metric, d, n):
    rows, inv, q = _corpus(oracle, metric, 20 + d + metric, n, d)
    rng = np.random.default_rng(d + metric)
    lists = {"0.5": _list(rng, n, 0.5), "0.5+ends": _list(rng, n, 0.5, True), "0.03": _list(rng, n, 0.03), "0.03+ends": _list(rng, n, 0.03, True),
             "all": np.arange(n, dtype=np.uint32)}
    if n >= 12_007:
        assert lists["0.5"].size > 4096   # more entries than the candidate list holds: the cap is a real limit
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        worst = {}
        for name, ids in lists.items():
            for kk in (1, 11, 64):
                for qi in range(3):
                    want, cand, cap = _forced_equals_f32(ix, monkeypatch, q[qi], kk, ids, (metric, d, n, name, kk, qi))
                    worst[name, kk] = max(worst.get((name, kk), 0), cand)
                    if name == "all":   # ... and the unfiltered search (RXGPU_SCAN_BF16=0 is still set)
                        _same(want, ix.search_knn(q[qi:qi + 1], kk), (metric, d, n, "unfiltered", kk, qi))
        print(f"candidates metric={metric} d={d} n={n}: {worst}")


def test_long_list_takes_the_chunked_kernel(rxgpu, oracle, monkeypatch):
    """A list of at least 2 x 64 entries per wavefront of the grid goes to the chunked, double-buffered form of the kernel (the lists above are
    served by the one-set-per-step form).  At one workgroup per CU that is 131 072 entries on 256 CUs."""
    n, d = 140_003, 256
    rows = make_corpus(300, n, d)
    ids = np.flatnonzero(np.arange(n) % 17 != 3).astype(np.uint32)   # 131 767 entries, no multiple of 64, rows 0 and n - 1 among them
    assert ids.size > 131_072 and ids.size % 64 and ids[0] == 0 and ids[-1] == n - 1
    for metric in METRICS:
        inv = oracle.l2_modules(rows) if metric == 2 else None
        q = make_corpus(301, 2, d)
        if metric == 2:
            q = np.stack([oracle.normalize_copy(v)[0] for v in q])
        with rxgpu.VectorIndex(metric, d, n) as ix:
            ix.upload_rows(0, rows, inv)
            for kk, qi in ((11, 0), (64, 1)):
                _env(monkeypatch, I8=1, I8_WG_PER_CU=1)
                got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn_subset(q[qi:qi + 1], kk, ids))
                print(f"candidates metric={metric} kk={kk}: {cand} (cap {cap})")
                assert slots == (0, 1, 0) and cand <= cap == 4096, (metric, kk, slots, cand, cap)
                _env(monkeypatch, BF16=0)
                _same(got, ix.search_knn_subset(q[qi:qi + 1], kk, ids), (metric, kk))


# ---------------------------------------------------------------------------------------------------------------- 2. tails
@pytest.mark.parametrize("metric", METRICS)
def test_tails_of_short_lists(rxgpu, oracle, monkeypatch, metric):
    n, d, kk = 2_000, 256, 11
    rows, inv, q = _corpus(oracle, metric, 40 + metric, n, d)
    rng = np.random.default_rng(40 + metric)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for n_ids in (1, 7, 15, 16, 17, 63, 64, 65, 129):
            ids = np.sort(rng.choice(n, n_ids, replace=False)).astype(np.uint32)
            for qi in range(3):
                want, _, _ = _forced_equals_f32(ix, monkeypatch, q[qi], kk, ids, (metric, n_ids, qi))   # kk > n_ids for the first two
                assert int(want[2][0]) == min(kk, n_ids)
        for ids in (np.array([0], np.uint32), np.array([n - 1], np.uint32), np.array([0, n - 1], np.uint32)):
            _forced_equals_f32(ix, monkeypatch, q[0], kk, ids, (metric, ids.tolist()))


# ---------------------------------------------------------------------------------------------------------------- 3. the filter filters
@pytest.mark.parametrize("metric", METRICS)
def test_excluded_rows_do_not_come_back(rxgpu, oracle, monkeypatch, metric):
    n, d, kk = 12_007, 768, 11
    rows, inv, q = _corpus(oracle, metric, 70 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for qi in range(3):
            _env(monkeypatch, BF16=0)
            _, best, cnt = ix.search_knn(q[qi:qi + 1], kk)
            assert int(cnt[0]) == kk
            ids = np.setdiff1d(np.arange(n, dtype=np.uint32), best[0]).astype(np.uint32)
            want, _, _ = _forced_equals_f32(ix, monkeypatch, q[qi], kk, ids, (metric, qi))
            assert not np.intersect1d(want[1][0], best[0]).size
            _env(monkeypatch, I8=1)
            got = ix.search_knn_subset(q[qi:qi + 1], kk, ids)
            assert not np.intersect1d(got[1][0], best[0]).size and int(got[2][0]) == kk


# ---------------------------------------------------------------------------------------------------------------- 4. what stays off the tier
def test_what_stays_off_the_tier(rxgpu, oracle, monkeypatch):
    n, d = 20_000, 256
    rows, _, q = _corpus(oracle, 1, 3, n, d)
    ids = _list(np.random.default_rng(3), n, 0.5)
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _env(monkeypatch, BF16=0)
        want = [_trim(ix.search_knn_subset(q[qi:qi + 1], 11, ids)) for qi in range(3)]
        _env(monkeypatch, I8=1)                                          # kk = 100: two list entries per lane, the f32 subset scan
        assert _slots(ix, lambda: ix.search_knn_subset(q[:1], 100, ids))[1] == (1, 0, 0)
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1, I8_SUBSET_MIN_BYTES=1)   # automatic mode: single queries only
        assert _slots(ix, lambda: ix.search_knn_subset(q[:3], 11, ids))[1] == (1, 0, 0)
        _env(monkeypatch, I8=1)                                          # forced: one launch serves the three queries
        got, slots, _ = _slots(ix, lambda: ix.search_knn_subset(q[:3], 11, ids))
        assert slots == (0, 1, 0)
        for qi in range(3):
            _same(tuple(a[qi:qi + 1] for a in got), want[qi], ("nq = 3", qi))
        for kw in (dict(I8=0), dict(BF16=0), dict(BF16=1), dict(I8=0, I8_SUBSET_MIN_BYTES=1), dict(BF16=0, I8=1), dict(BF16=1, I8=1)):
            _env(monkeypatch, **kw)
            got, slots, _ = _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))
            assert slots == (1, 0, 0), kw
            _same(_trim(got), want[0], kw)
    for d2 in (128, 1100):   # 128: a code row is no shorter than a bf16 row; 1100: the tier does not serve it
        with rxgpu.VectorIndex(1, d2, 3000) as ix:
            ix.upload_rows(0, make_corpus(4, 3000, d2))
            _env(monkeypatch, I8=1)
            assert _slots(ix, lambda: ix.search_knn_subset(make_corpus(5, 1, d2), 11, np.arange(0, 3000, 2, dtype=np.uint32)))[1] == (1, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- 5. automatic threshold
def test_automatic_threshold_counts_the_listed_bytes(rxgpu, oracle, monkeypatch):
    n, d = 20_000, 256
    rows, _, q = _corpus(oracle, 1, 5, n, d)
    ids = _list(np.random.default_rng(5), n, 0.5)
    listed = ids.size * d * 4
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _env(monkeypatch)                                                # the default threshold: these sizes keep the f32 subset scan
        want, slots, _ = _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))
        assert slots == (1, 0, 0)
        _env(monkeypatch, I8_SUBSET_MIN_BYTES=listed)
        got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))
        assert slots == (0, 1, 0) and cand <= cap
        _same(got, want, "at the threshold")
        _env(monkeypatch, I8_SUBSET_MIN_BYTES=listed + 1)
        got, slots, _ = _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))
        assert slots == (1, 0, 0)
        _same(got, want, "below the threshold")
        _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)              # the thresholds of the unfiltered tiers do not move this one
        assert _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))[1] == (1, 0, 0)
        _env(monkeypatch, I8_SUBSET_MIN_BYTES=n * d * 4)                 # the unit is the listed rows, not the index
        assert _slots(ix, lambda: ix.search_knn_subset(q[:1], 11, ids))[1] == (1, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- 6. overflow behind the gate
def test_mass_ties_overflow_the_list_and_the_gated_subset_scan_answers(rxgpu, monkeypatch):
    """The {-1, 0, 1} corpus of test_gpu_scan_i8.py's mass-ties test: rows quantise without residual, the zero query ties every listed row."""
    rng = np.random.default_rng(5)
    n, d = 60_000, 256
    rows = rng.integers(-1, 2, (n, d)).astype(np.float32)
    ids = np.arange(0, n, 2, dtype=np.uint32)
    assert ids.size == 30_000
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _, cand, cap = _forced_equals_f32(ix, monkeypatch, np.zeros(d, np.float32), 11, ids, "zero", pruned=False)
        assert cand > cap, (cand, cap)   # ... so the helper has seen "fallback_scan" = 1 and "scan_subset" = 0
        _forced_equals_f32(ix, monkeypatch, rng.integers(-1, 2, d).astype(np.float32), 11, ids, "ordinary", pruned=False)


# ---------------------------------------------------------------------------------------------------------------- 7. non-finite
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_queries_through_the_forced_tier(rxgpu, oracle, monkeypatch, metric, kind):
    n, d, kk = 9_000, 256, 11
    rows, inv, q = _corpus(oracle, metric, 120 + metric, n, d)
    ids = _list(np.random.default_rng(120 + metric), n, 0.5)
    query = q[0].copy()
    query[7] = np.nan if kind == "nan" else np.inf
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, cand, cap = _forced_equals_f32(ix, monkeypatch, query, kk, ids, (metric, kind), pruned=False)
        assert cand == cap + 1   # no finite bound: re-routed on the device
        _forced_equals_f32(ix, monkeypatch, q[1], kk, ids, (metric, kind, "next query"))   # the context is fit for the next, ordinary query


@pytest.mark.parametrize("metric", METRICS)
def test_nonfinite_row_outside_the_list(rxgpu, oracle, monkeypatch, metric):
    n, d, kk = 9_000, 256, 11
    rows, _, q = _corpus(oracle, metric, 90 + metric, n, d)
    rows[5_000] = 0.1
    rows[5_000, d // 2] = np.nan
    with np.errstate(all="ignore"):
        inv = oracle.l2_modules(rows) if metric == 2 else None
    ids = np.setdiff1d(_list(np.random.default_rng(90 + metric), n, 0.5), [5_000]).astype(np.uint32)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, BF16=0)
        want = ix.search_knn_subset(q[:1], kk, ids)
        _env(monkeypatch, I8_SUBSET_MIN_BYTES=1)
        got, slots, _ = _slots(ix, lambda: ix.search_knn_subset(q[:1], kk, ids))
        assert slots == (1, 0, 0), "an index with a non-finite row statistic keeps the f32 subset scan"
        _same(got, want, metric)
        _, cand, cap = _forced_equals_f32(ix, monkeypatch, q[0], kk, ids, (metric, "forced"), pruned=False)   # forced: the gate answers
        assert cand == cap + 1


# ---------------------------------------------------------------------------------------------------------------- 8. mutations
@pytest.mark.parametrize("metric", METRICS)
def test_mutations_keep_the_shadow_in_step(rxgpu, oracle, monkeypatch, metric):
    n, d = 12_000, 256
    rows, inv, q = _corpus(oracle, metric, 60 + metric, n, d)
    keep = np.random.default_rng(60 + metric).random(n) < 0.5
    keep[100:140] = True        # the rows that are overwritten
    keep[7] = True              # where the best row moves to
    keep[n - 1] = True
    ids = np.flatnonzero(keep).astype(np.uint32)
    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)
        _forced_equals_f32(ix, monkeypatch, q[0], 11, ids, (metric, "fresh"))
        new = make_corpus(77 + metric, 40, d)
        new[0] = q[0] / (np.linalg.norm(q[0]) or 1.0) if metric == 2 else q[0]   # a new best row for query 0
        ix.upload_rows(100, new, oracle.l2_modules(new) if metric == 2 else None)
        want, _, _ = _forced_equals_f32(ix, monkeypatch, q[0], 11, ids, (metric, "upload_rows over listed rows"))
        if metric != 1:
            assert want[1][0, 0] == 100
        ix.move_row(100, 7)                                              # the best row moves
        want, _, _ = _forced_equals_f32(ix, monkeypatch, q[0], 11, ids, (metric, "move_row"))
        if metric != 1:
            assert want[1][0, 0] == 7
        ix.truncate(n - 1)
        _forced_equals_f32(ix, monkeypatch, q[0], 11, ids[:-1], (metric, "truncate"))


# ---------------------------------------------------------------------------------------------------------------- 9. entry points
def _to_words(ids, n):
    words = np.zeros((n + 31) // 32, np.uint32)
    ids = np.asarray(ids, np.int64)
    np.bitwise_or.at(words, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return words


@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_through_every_entry_point(rxgpu, oracle, monkeypatch, metric):
    import torch
    n, d, kk, nlist, nprobe = 24_000, 256, 11, 64, 16
    rows, inv, q = _corpus(oracle, metric, 50 + metric, n, d)
    rng = np.random.default_rng(50 + metric)
    ids = _list(rng, n, 0.5)
    words = _to_words(ids, n)
    cents = make_corpus(500 + metric, nlist, d)
    owner = rng.integers(0, nlist, n)
    lists = [np.flatnonzero(owner == l).astype(np.uint32) for l in range(nlist)]
    dev = torch.device("cuda", 0)
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx, rxgpu.ShardedVectorIndex(metric, d, n, [0, 0]) as sx:
        ix.upload_rows(0, rows, inv)
        sx.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, oracle.l2_modules(cents) if metric == 2 else None)
        ix.set_lists(lists)
        dq = torch.from_numpy(q).to(dev)
        dids = torch.from_numpy(ids.view(np.int32)).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def device_search(qi):
            od = torch.empty((1, kk), dtype=torch.float32, device=dev)
            orow = torch.empty((1, kk), dtype=torch.int32, device=dev)
            oc = torch.zeros(1, dtype=torch.int32, device=dev)
            ix.search_knn_subset_device(dq.data_ptr() + qi * d * 4, 1, kk, dids.data_ptr(), ids.size, od.data_ptr(), orow.data_ptr(), oc.data_ptr(),
                                        stream)
            torch.cuda.synchronize(dev)
            return od.cpu().numpy(), orow.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)

        for qi in range(3):
            one = q[qi:qi + 1]
            _env(monkeypatch, BF16=0)
            want = ix.search_knn_subset(one, kk, ids)
            want_lists, slots, _ = _slots(ix, lambda: ix.search_knn_lists(cx, q[qi], nprobe, kk))
            assert slots == (1, 0, 0)
            _same(sx.search_knn_subset(one, kk, ids), want, ("sharded f32 vs one index", metric, qi))
            _env(monkeypatch, I8=1)
            got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn_bitmap(one, kk, words))
            assert slots == (0, 1, 0) and cand <= cap and got[3] == ids.size
            _same(got[:3], want, ("rxgpu_search_knn_bitmap", metric, qi))
            got, slots, _ = _slots(ix, lambda: device_search(qi))
            assert slots == (0, 1, 0)
            _same(got, want, ("rxgpu_search_knn_subset_device", metric, qi))
            got, slots, (cand, cap) = _slots(ix, lambda: ix.search_knn_lists(cx, q[qi], nprobe, kk))
            assert slots == (0, 1, 0) and cand <= cap
            assert np.array_equal(got[1], want_lists[1]) and np.array_equal(bits(got[0]), bits(want_lists[0])) and got[2] == want_lists[2]
            assert got[1].size == kk and 0 < got[2] < n
            views = [sx.shard(s) for s in range(2)]
            for v in views:
                v.profile_enable(True)
            got_sharded = sx.search_knn_subset(one, kk, ids)
            assert [tuple(v.profile_read(s)[0] for s in SLOTS) for v in views] == [(0, 1, 0), (0, 1, 0)]
            for v in views:
                v.profile_enable(False)
            _same(got_sharded, want, ("two shards", metric, qi))
