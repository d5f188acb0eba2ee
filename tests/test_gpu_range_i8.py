"""-m gpu: range searches served from the int8 shadow (knn_range_i8 / knn_range_i8_subset in knn_scan_i8.hip, knn_range_rescore in knn_range.hip,
enqueue_range_pruned_i8 / range_on_device on the host; the bound is i8_range_bound in knn_i8_quant.h).

The yardstick of every comparison is THE SAME BUILD with RXGPU_SCAN_BF16=0, the f32 range kernels that test_gpu_bruteforce.py and
test_gpu_ivf.py pin to the oracle: the return code, *out_total, rows and distance bits must be equal.  The path taken is observed through
the profile slots ("range" / "range_subset" = the f32 kernel was launched, "range_i8" / "range_i8_subset" the pruning scan, "range_rescore"
its exact tail) and through rxgpu_index_last_candidates: candidates <= ccap means the tier, not the f32 kernel behind it, produced what
was compared.  Radii are distances of stored rows, so the strict form must exclude exactly that row and the inclusive form include it:
the boundary at which a wrong bound shows."""
import ctypes as C

import numpy as np
import pytest

from .conftest import make_corpus

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]   # l2, ip, cosine
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_RANGE_MIN_BYTES", "RXGPU_SCAN_I8_WG_PER_CU")
WHOLE = ("range", "range_i8", "range_rescore")
LISTED = ("range_subset", "range_i8_subset", "range_rescore")
OVERFLOW = -8   # RXGPU_ERR_OVERFLOW


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


def _corpus(oracle, metric, seed, n, d, nq=3):
    rows = make_corpus(seed, n, d)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    q = make_corpus(seed + 1000, nq, d)
    if metric == 2:
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    return rows, inv, q


def _range(rxgpu, ix, query, radius, inclusive, cap, ids=None):
    """one call at the C level (no retry): (return code, *out_total, dist[:written], row[:written])"""
    L = rxgpu.lib()
    q = np.ascontiguousarray(query, np.float32).reshape(ix.dim)
    dist, row = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.uint32)
    total = C.c_uint64(0)
    if ids is None:
        rc = L.rxgpu_search_range(ix._h, q.ctypes.data, C.c_float(radius), int(inclusive), dist.ctypes.data, row.ctypes.data, cap, C.byref(total))
    else:
        ids = np.ascontiguousarray(ids, np.uint32)
        rc = L.rxgpu_search_range_subset(ix._h, q.ctypes.data, C.c_float(radius), int(inclusive), ids.ctypes.data, ids.size, dist.ctypes.data,
                                         row.ctypes.data, cap, C.byref(total))
    t = int(total.value)
    w = t if t <= cap else 0
    return rc, t, dist[:w].copy(), row[:w].copy()


def _slots(ix, fn, names=WHOLE):
    """(result of fn, launches filed under `names`, (candidates, ccap)) with profiling on around fn"""
    ix.profile_enable(True)
    out = fn()
    n = tuple(ix.profile_read(s)[0] for s in names)
    cand = ix.last_candidates()
    ix.profile_enable(False)
    return out, n, cand


def _same(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], (what, a[:2], b[:2])
    assert np.array_equal(a[3], b[3]), what
    assert np.array_equal(bits(a[2]), bits(b[2])), what


def _ccap(n, cap):
    return min(n, max(4096, 2 * min(cap, n)))


def _forced_equals_f32(rxgpu, ix, monkeypatch, query, radius, inclusive, cap, what, ids=None, served=True):
    """the call through the forced tier and through the f32 kernel; served: the tier itself must have answered.  Returns (f32 result, candidates, ccap)"""
    names = WHOLE if ids is None else LISTED
    n = ix.count if ids is None else len(ids)
    _env(monkeypatch, I8=1)
    got, slots, (cand, ccap) = _slots(ix, lambda: _range(rxgpu, ix, query, radius, inclusive, cap, ids), names)
    assert ccap == _ccap(n, cap), (what, ccap)
    assert slots == (int(cand > ccap), 1, 1), (what, slots, cand, ccap)
    if served:
        assert cand <= ccap, (what, "the candidate list overflowed", cand, ccap)
    _env(monkeypatch, BF16=0)
    want, slots, _ = _slots(ix, lambda: _range(rxgpu, ix, query, radius, inclusive, cap, ids), names)
    assert slots == (1, 0, 0), what
    _same(got, want, what)
    return want, cand, ccap


def _radii(kd):
    """(radius, inclusive, expected hits or None) from the ascending f32 KNN distances of the query: ranks 1, 10 and 64 (as far as there are that
    many) strict and inclusive, halfway between ranks 10 and 11, and below the best"""
    out = []
    for rank in (1, 10, 64):
        if rank <= kd.size:
            out += [(float(kd[rank - 1]), False), (float(kd[rank - 1]), True)]
    if kd.size >= 11:
        out.append((float(np.float32((np.float64(kd[9]) + np.float64(kd[10])) / 2)), False))
    out.append((float(np.nextafter(kd[0], np.float32(-np.inf))), True))
    return out


def _expected(kd, radius, inclusive):
    """hits among the first kd.size ranks (exact while below kd.size)"""
    r = np.float32(radius)
    return int((kd <= r).sum() if inclusive else (kd < r).sum())


# ---------------------------------------------------------------------------------------------------------------- 1. the forced tier
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", [(768, 12_007), (256, 30_000), (1024, 4_000), (750, 5_000)])
def test_forced_tier_returns_the_total_rows_and_bits_of_the_f32_kernel(rxgpu, oracle, monkeypatch, metric, d, n):
    rows, inv, q = _corpus(oracle, metric, 20 + d + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        worst = 0
        for qi in range(3):
            _env(monkeypatch, BF16=0)
            kd = ix.search_knn(q[qi:qi + 1], 65)[0][0]
            for radius, inclusive in _radii(kd[:64]):
                want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[qi], radius, inclusive, 1024, (metric, d, n, qi, radius, inclusive))
                assert want[0] == 0 and want[1] == _expected(kd, radius, inclusive) <= 64, (metric, d, n, qi, radius, inclusive, want[1])
                worst = max(worst, cand)
        print(f"candidates metric={metric} d={d} n={n}: at most {worst} (ccap {ccap})")


# ---------------------------------------------------------------------------------------------------------------- 2. few rows, count < capacity
@pytest.mark.parametrize("metric", METRICS)
def test_seven_rows_and_rows_past_the_count(rxgpu, oracle, monkeypatch, metric):
    rows, inv, q = _corpus(oracle, metric, 40 + metric, 7, 256)
    with rxgpu.VectorIndex(metric, 256, 16) as ix:
        ix.upload_rows(0, rows, inv)
        for qi in range(3):
            _env(monkeypatch, BF16=0)
            kd = ix.search_knn(q[qi:qi + 1], 7)[0][0]
            for radius, inclusive in _radii(kd) + [(float(kd[6]), True), (3.0e38, False)]:
                want, _, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[qi], radius, inclusive, 16, (metric, qi, radius, inclusive))
                assert ccap == 7 and want[1] == _expected(kd, radius, inclusive)
    n = 5_000
    rows, inv, q = _corpus(oracle, metric, 45 + metric, n, 256)
    with rxgpu.VectorIndex(metric, 256, n) as ix:
        ix.upload_rows(0, rows, inv)
        _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], 3.0e38, False, n, (metric, "full"))          # the shadow covers all n rows
        ix.truncate(3_001)
        want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], 3.0e38, False, n, (metric, "truncated"))
        assert want[1] == 3_001 and cand == 3_001 == ccap and want[3].max() == 3_000                  # no row past the count is a candidate or a hit


# ---------------------------------------------------------------------------------------------------------------- 3. the overflow protocol
@pytest.mark.parametrize("metric", METRICS)
def test_overflow_protocol_is_the_f32_kernels(rxgpu, oracle, monkeypatch, metric):
    n, d = 12_007, 768
    rows, inv, q = _corpus(oracle, metric, 20 + d + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, BF16=0)
        kd = ix.search_knn(q[:1], 64)[0][0]
        want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], float(kd[63]), True, 16, (metric, "cap 16"))
        assert want[0] == OVERFLOW and want[1] == 64 and want[2].size == 0 and ccap == 4096
        want, _, _ = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], float(kd[63]), True, 64, (metric, "cap = total"))
        assert want[0] == 0 and want[1] == 64 and np.array_equal(bits(want[2]), bits(kd))


# ---------------------------------------------------------------------------------------------------------------- 4. the candidate list overflows
@pytest.mark.parametrize("metric", METRICS)
def test_candidate_list_overflow_ends_in_the_f32_kernels_answer(rxgpu, oracle, monkeypatch, metric):
    n, d = 60_000, 256
    rows, inv, q = _corpus(oracle, metric, 70 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for radius in (float("inf"), 1.0e30):
            want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], radius, False, 16, (metric, radius, "cap 16"), served=False)
            assert want[0] == OVERFLOW and want[1] == n and ccap == 4096 and cand > ccap          # the scan ran, the f32 kernel answered
            want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], radius, False, n, (metric, radius, "cap n"))
            assert want[0] == 0 and want[1] == n and cand == n == ccap                            # every row a candidate, all re-scored by the tier


# ---------------------------------------------------------------------------------------------------------------- 5. no finite bound
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_rows_leave_the_call_to_the_f32_kernel(rxgpu, oracle, monkeypatch, metric, kind):
    n, d = 9_000, 256
    rows, _, q = _corpus(oracle, metric, 90 + metric, n, d)
    rows[5_000] = 0.1
    rows[5_000, d // 2] = np.nan if kind == "nan" else np.inf
    with np.errstate(all="ignore"):
        inv = oracle.l2_modules(rows) if metric == 2 else None
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, BF16=0)
        kd = ix.search_knn(q[:1], 11)[0][0]
        for radius, inclusive in ((float(kd[9]), True), (float(kd[9]), False), (float("inf"), False)):
            want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], radius, inclusive, n, (metric, kind, radius), served=False)
            assert cand == ccap + 1                                                              # the query prep's mark: the scan emitted nothing
        _env(monkeypatch, BF16=0)
        want = _range(rxgpu, ix, q[0], float(kd[9]), True, n)
        _env(monkeypatch, I8_RANGE_MIN_BYTES=1)                                                  # automatic mode: not even the scan
        got, slots, _ = _slots(ix, lambda: _range(rxgpu, ix, q[0], float(kd[9]), True, n))
        assert slots == (1, 0, 0)
        _same(got, want, (metric, kind, "automatic"))


@pytest.mark.parametrize("metric", METRICS)
def test_nan_radius_nonfinite_and_zero_queries(rxgpu, oracle, monkeypatch, metric):
    n, d = 9_000, 256
    rows, inv, q = _corpus(oracle, metric, 120 + metric, n, d)
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for inclusive in (False, True):
            want, cand, _ = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], float("nan"), inclusive, 64, (metric, "nan radius", inclusive))
            assert want[:2] == (0, 0) and cand == 0                                              # no row passes a NaN threshold; the f32 kernel finds none
        zero = np.zeros(d, np.float32)
        for radius, inclusive in ((0.0, True), (0.0, False), (-0.0, True), (1.0, False), (-1.0, True)):
            _forced_equals_f32(rxgpu, ix, monkeypatch, zero, radius, inclusive, n, (metric, "zero query", radius, inclusive), served=False)
        for bad in (np.nan, np.inf):
            query = q[1].copy()
            query[7] = bad
            want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, query, 0.5, True, n, (metric, "query", bad), served=False)
            assert cand == ccap + 1
        _env(monkeypatch, BF16=0)
        kd = ix.search_knn(q[2:3], 11)[0][0]
        _forced_equals_f32(rxgpu, ix, monkeypatch, q[2], float(kd[9]), True, 64, (metric, "the context is fit for the next, ordinary query"))


# ---------------------------------------------------------------------------------------------------------------- 6. the shadow follows the rows
@pytest.mark.parametrize("metric", METRICS)
def test_mutations_keep_the_shadow_in_step(rxgpu, oracle, monkeypatch, metric):
    n, d = 12_000, 256
    rows, inv, q = _corpus(oracle, metric, 60 + metric, n, d)

    def check(ix, what):
        _env(monkeypatch, BF16=0)
        kd = ix.search_knn(q[:1], 11)[0][0]
        for inclusive in (False, True):
            want, _, _ = _forced_equals_f32(rxgpu, ix, monkeypatch, q[0], float(kd[9]), inclusive, 64, (metric, what, inclusive))
            assert want[1] == 9 + int(inclusive)
        return kd

    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)
        check(ix, "fresh")
        new = make_corpus(77 + metric, 40, d)
        new[0] = q[0] / (np.linalg.norm(q[0]) or 1.0) if metric == 2 else q[0]                   # a new best row for query 0
        ix.upload_rows(6_000, new, oracle.l2_modules(new) if metric == 2 else None)
        kd = check(ix, "upload_rows over a middle block")
        _env(monkeypatch, I8=1)
        assert ix.search_range(q[0], float(kd[0]), inclusive=True)[1].tolist() == [6_000]
        ix.move_row(6_000, 7)                                                                    # the best row moves
        check(ix, "move_row")
        ix.truncate(n - 1)
        check(ix, "truncate")
        ix.upload_rows(n - 1, new[:5], oracle.l2_modules(new[:5]) if metric == 2 else None)      # growing again
        kd = check(ix, "append")
        _env(monkeypatch, I8=1)                                                                  # the best row three times: moved to, moved from, appended
        assert ix.search_range(q[0], float(kd[0]), inclusive=True)[1].tolist() == [7, 6_000, n - 1]


# ---------------------------------------------------------------------------------------------------------------- 7. mass ties
def test_mass_ties_at_the_radius(rxgpu, monkeypatch):
    """Rows in {-1, 0, 1} quantise without residual and a one-hot query ties a third of the rows at each of the distances -1, 0 and 1 (ip): at
    a radius equal to a tied distance the strict and the inclusive form differ by 20 000 rows, all of them inside the scan's window."""
    rng = np.random.default_rng(5)
    n, d = 60_000, 256
    rows = rng.integers(-1, 2, (n, d)).astype(np.float32)
    unit = np.zeros(d, np.float32)
    unit[17] = 1.0
    tied = {r: int((rows[:, 17] == -r).sum()) for r in (-1.0, 0.0, 1.0)}
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        for radius in (-1.0, 0.0):
            below = sum(c for r, c in tied.items() if r < radius)
            for inclusive in (False, True):
                hits = below + (tied[radius] if inclusive else 0)
                want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, unit, radius, inclusive, n, ("ties", radius, inclusive, "cap n"), served=False)
                assert want[:2] == (0, hits) and ccap == n and hits <= cand <= n                 # the list holds every row: the tier answers
                want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, unit, radius, inclusive, 16, ("ties", radius, inclusive, "cap 16"), served=False)
                assert want[1] == hits and want[0] == (OVERFLOW if hits > 16 else 0) and ccap == 4096
                assert cand >= below + tied[radius] > ccap                                       # the tied rows are candidates of both forms: the f32 kernel answers


# ---------------------------------------------------------------------------------------------------------------- 8. row lists
@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_over_row_lists(rxgpu, oracle, monkeypatch, metric):
    n, d = 12_007, 768
    rows, inv, q = _corpus(oracle, metric, 20 + d + metric, n, d)
    rng = np.random.default_rng(d + metric)
    lists = [np.sort(rng.choice(n, size, replace=False)).astype(np.uint32) for size in (1, 15, 17, 5_000)] + [np.arange(n, dtype=np.uint32)]
    lists[1][-1] = n - 1                                                                         # the last row of the index in a list
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for ids in lists:
            for qi in range(3):
                _env(monkeypatch, BF16=0)
                kd, _, cnt = ix.search_knn_subset(q[qi:qi + 1], 65, ids)
                kd = kd[0][:int(cnt[0])]
                for radius, inclusive in _radii(kd[:64]):
                    what = (metric, ids.size, qi, radius, inclusive)
                    want, _, _ = _forced_equals_f32(rxgpu, ix, monkeypatch, q[qi], radius, inclusive, 1024, what, ids=ids)
                    assert want[0] == 0 and want[1] == _expected(kd, radius, inclusive) and np.isin(want[3], ids).all(), what
                want, cand, ccap = _forced_equals_f32(rxgpu, ix, monkeypatch, q[qi], 3.0e38, False, n, (metric, ids.size, qi, "all"), ids=ids)
                assert want[1] == ids.size == cand == ccap and np.array_equal(np.sort(want[3]), ids)


@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_through_the_ivf_range_call(rxgpu, oracle, monkeypatch, metric):
    """rows and lists of the size test_gpu_ivf.py's device-list test uses (9 000 rows in 300 lists), at a dimension the tier serves"""
    n, d, nlist = 9_000, 256, 300
    rows, inv, q = _corpus(oracle, metric, 50 + metric, n, d)
    rng = np.random.default_rng(50 + metric)
    cents = make_corpus(500 + metric, nlist, d)
    owner = rng.integers(0, nlist, n)
    lists = [np.flatnonzero(owner == l).astype(np.uint32) for l in range(nlist)]
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.VectorIndex(metric, d, nlist) as cx:
        ix.upload_rows(0, rows, inv)
        cx.upload_rows(0, cents, oracle.l2_modules(cents) if metric == 2 else None)
        ix.set_lists(lists)
        for nprobe in (1, 16):
            for qi in range(3):
                _env(monkeypatch, BF16=0)
                kd, krow, scanned = ix.search_knn_lists(cx, q[qi], nprobe, 11)
                for radius, inclusive in _radii(kd):
                    _env(monkeypatch, BF16=0)
                    want, slots, _ = _slots(ix, lambda: ix.search_range_lists(cx, q[qi], nprobe, radius, inclusive=inclusive, cap=4), LISTED)
                    assert slots[1:] == (0, 0) and slots[0] >= 1
                    _env(monkeypatch, I8=1)
                    got, slots, (cand, ccap) = _slots(ix, lambda: ix.search_range_lists(cx, q[qi], nprobe, radius, inclusive=inclusive, cap=4), LISTED)
                    assert slots[0] == 0 and slots[1] == slots[2] >= 1 and cand <= ccap == min(scanned, 4096), (metric, nprobe, qi, slots, cand, ccap)
                    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0])) and got[2] == want[2] == scanned
                    assert got[1].size == _expected(kd, radius, inclusive)


# ---------------------------------------------------------------------------------------------------------------- 9. a row-sharded index
@pytest.mark.parametrize("metric", METRICS)
def test_forced_tier_on_two_shards(rxgpu, oracle, monkeypatch, metric):
    n, d = 24_000, 256
    rows, inv, q = _corpus(oracle, metric, 50 + metric, n, d)
    ids = np.flatnonzero(np.random.default_rng(9 + metric).random(n) < 0.5).astype(np.uint32)
    with rxgpu.VectorIndex(metric, d, n) as ix, rxgpu.ShardedVectorIndex(metric, d, n, [0, 0]) as sx:
        ix.upload_rows(0, rows, inv)
        sx.upload_rows(0, rows, inv)
        views = [sx.shard(s) for s in range(2)]
        for qi in range(3):
            _env(monkeypatch, BF16=0)
            kd = ix.search_knn(q[qi:qi + 1], 64)[0][0]
            ks = ix.search_knn_subset(q[qi:qi + 1], 64, ids)[0][0]
            for inclusive in (False, True):
                for listed, radius, names in ((None, float(kd[63]), WHOLE), (ids, float(ks[63]), LISTED)):
                    call = (lambda x: x.search_range(q[qi], radius, inclusive=inclusive)) if listed is None else \
                           (lambda x: x.search_range_subset(q[qi], radius, listed, inclusive=inclusive))
                    _env(monkeypatch, BF16=0)
                    want, want_sharded = call(ix), call(sx)
                    _env(monkeypatch, I8=1)
                    for v in views:
                        v.profile_enable(True)
                    got_sharded = call(sx)
                    assert [tuple(v.profile_read(s)[0] for s in names) for v in views] == [(0, 1, 1), (0, 1, 1)]   # the per-shard calls reach the chain
                    for v in views:
                        v.profile_enable(False)
                    got = call(ix)
                    assert want[1].size == 63 + int(inclusive)
                    for res in (want_sharded, got_sharded, got):
                        assert np.array_equal(res[1], want[1]) and np.array_equal(bits(res[0]), bits(want[0])), (metric, qi, inclusive, listed is None)


# ---------------------------------------------------------------------------------------------------------------- 10. automatic mode, the switches
def test_automatic_mode_follows_the_thresholds_the_dimension_and_the_switches(rxgpu, oracle, monkeypatch):
    n, d = 20_000, 256
    rows, _, q = _corpus(oracle, 1, 3, n, d)
    size = n * d * 4
    ids = np.arange(0, n, 4, dtype=np.uint32)
    lsize = ids.size * d * 4
    tier = rxgpu.scan_tier_range
    with rxgpu.VectorIndex(1, d, n) as ix:
        ix.upload_rows(0, rows)
        _env(monkeypatch, BF16=0)
        kd = ix.search_knn(q[:1], 11)[0][0]
        ks = ix.search_knn_subset(q[:1], 11, ids)[0][0]
        want = _range(rxgpu, ix, q[0], float(kd[9]), True, 64)
        want_l = _range(rxgpu, ix, q[0], float(ks[9]), True, 64, ids)

        def whole(expect_i8, **env):
            _env(monkeypatch, **env)
            got, slots, _ = _slots(ix, lambda: _range(rxgpu, ix, q[0], float(kd[9]), True, 64))
            assert slots == ((0, 1, 1) if expect_i8 else (1, 0, 0)), (env, slots)
            assert tier(n, d) == (2 if expect_i8 else 0), env
            _same(got, want, env)

        def listed(expect_i8, **env):
            _env(monkeypatch, **env)
            got, slots, _ = _slots(ix, lambda: _range(rxgpu, ix, q[0], float(ks[9]), True, 64, ids), LISTED)
            assert slots == ((0, 1, 1) if expect_i8 else (1, 0, 0)), (env, slots)
            assert tier(ids.size, d, listed=True) == (2 if expect_i8 else 0), env
            _same(got, want_l, env)

        whole(False)                                                     # the default threshold is 16 GiB: the f32 kernel
        whole(True, I8_RANGE_MIN_BYTES=size)                             # at the threshold
        whole(False, I8_RANGE_MIN_BYTES=size + 1)                        # one above
        whole(False, I8_RANGE_MIN_BYTES=1, I8=0)
        whole(False, I8_RANGE_MIN_BYTES=1, BF16=0)
        whole(False, I8_RANGE_MIN_BYTES=1, BF16=1)
        whole(False, I8=1, BF16=0)
        whole(False, I8=1, BF16=1)
        whole(False, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)                   # the KNN thresholds do not move a range call
        whole(True, I8=1)
        listed(False)
        listed(False, I8_RANGE_MIN_BYTES=1)                              # a list call follows both thresholds
        listed(False, I8_SUBSET_MIN_BYTES=1)
        listed(True, I8_RANGE_MIN_BYTES=lsize, I8_SUBSET_MIN_BYTES=lsize)
        listed(False, I8_RANGE_MIN_BYTES=lsize + 1, I8_SUBSET_MIN_BYTES=lsize)
        listed(False, I8_RANGE_MIN_BYTES=lsize, I8_SUBSET_MIN_BYTES=lsize + 1)
        listed(False, I8_RANGE_MIN_BYTES=1, I8_SUBSET_MIN_BYTES=1, I8=0)
        listed(True, I8=1)
    for d2 in (128, 1100):                                              # 128: a code row is no shorter than the bf16 row; 1100: the tier does not serve it
        with rxgpu.VectorIndex(1, d2, 5000) as ix:
            ix.upload_rows(0, make_corpus(4, 5000, d2))
            query = make_corpus(5, 1, d2)[0]
            for env in (dict(I8=1), dict(I8_RANGE_MIN_BYTES=1)):
                _env(monkeypatch, **env)
                _, slots, _ = _slots(ix, lambda: _range(rxgpu, ix, query, 0.0, False, 64))
                assert slots == (1, 0, 0) and tier(5000, d2) == 0, (d2, env)


# ---------------------------------------------------------------------------------------------------------------- 11. the Map
@pytest.mark.parametrize("metric", METRICS)
def test_map_range_search_and_tie_replay(rxgpu, oracle, monkeypatch, metric):
    """GpuBruteforceMap::SearchRange, and a SearchKnn whose k-th place is tied (a block of rows stored twice under different labels), which
    replays the reference's admission rule with an inclusive range call: both return what they return on the f32 kernels."""
    from reindexer_amd import hostapi
    hostapi.lib()
    n, d = 6_000, 256
    rows, _, q = _corpus(oracle, metric, 130 + metric, n, d)
    rows = np.concatenate([rows, rows[100:140]])
    rng = np.random.default_rng(130 + metric)
    labels = (rng.permutation(rows.shape[0]).astype(np.uint64) << np.uint64(32)) | np.uint64(3)
    m = hostapi.GpuBruteforceMap(metric, d, rows.shape[0] + 16)
    try:
        m.add(rows, labels)
        queries = [q[0], q[1]] + [rows[100 + i] * np.float32(1.0) for i in (0, 7, 39)]          # the nearest rows of the last three are stored twice
        results = {}
        for mode, env in (("f32", dict(BF16=0)), ("i8", dict(I8=1))):
            _env(monkeypatch, **env)
            before = m.tie_replays
            out = []
            for query in queries:
                kd, kl = m.search_knn(query, 11)
                out.append((kd, kl))
                out.append(m.search_knn(query, 1))                                              # the tied pair straddles the first place
                out.append(m.search_range(query, float(kd[9])))
                out.append(m.search_range(query, float(kd[0])))
            results[mode] = (out, m.tie_replays - before)
        assert results["i8"][1] == results["f32"][1] >= 3, (results["i8"][1], results["f32"][1])
        for a, b in zip(results["i8"][0], results["f32"][0]):
            assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0])), metric
    finally:
        m.close()
