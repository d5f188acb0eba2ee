"""The arithmetic of the int8 shadow tier (reindexer_amd/csrc/knn_i8_quant.h), compiled for the host (tests/cpp/knn_i8_quant_cpu.cc) and pinned
on the CPU against float64: the stored residual bounds the real one, the approximate distance is within the bound the kernel and the margin
add up to, [lo, up] (+ the per-query part) brackets the float64 distance, the query planes reconstruct, the integer sum cannot overflow; and
rxgpu_scan_tier decides as include/rxgpu.h documents (no device is touched)."""
import ctypes as C

import numpy as np
import pytest

from . import i8_model
from .i8_model import COS, IP, L2, PF, PI8, PI32, _p, quantize_queries, quantize_rows


@pytest.fixture(scope="module")
def lib():
    return i8_model.load()


def corpus(d, seed):
    """random rows + the adversarial ones: scales exp(U(-14, 14)), one huge component, a zero row, a subnormal row, a constant row"""
    rng = np.random.default_rng(seed)
    plain = rng.normal(0, 0.25, (300, d))
    scaled = rng.normal(0, 1, (190, d)) * np.exp(rng.uniform(-14, 14, (190, 1)))
    huge = rng.normal(0, 0.25, (6, d))
    huge[np.arange(6), rng.integers(0, d, 6)] *= 1e6
    rows = np.concatenate([plain, scaled, huge, np.zeros((1, d)), np.full((1, d), 1e-39), np.full((1, d), 0.37), np.full((1, d), -3e-3)]).astype(np.float32)
    queries = np.concatenate([rng.normal(0, 0.25, (100, d)), rng.normal(0, 1, (97, d)) * np.exp(rng.uniform(-6, 6, (97, 1))), rows[[3, 350]],
                              np.zeros((1, d))]).astype(np.float32)
    return rows, queries


@pytest.fixture(scope="module", params=[768, 200])
def quantized(request, lib):
    d = request.param
    rows, queries = corpus(d, d)
    assert rows.shape[0] * queries.shape[0] == 100_000
    codes, scale, resid = quantize_rows(lib, rows)
    h, l, t, info = quantize_queries(lib, queries)
    return dict(d=d, rows=rows, queries=queries, codes=codes, scale=scale, resid=resid, h=h, l=l, t=t, info=info)


def test_stored_residual_bounds_the_float64_residual(quantized):
    z = quantized
    d = z["d"]
    real = np.sqrt(((z["rows"].astype(np.float64) - z["scale"].astype(np.float64)[:, None] * z["codes"][:, :d]) ** 2).sum(1))
    assert np.all(z["resid"].astype(np.float64) >= real)
    assert np.all(z["resid"] <= real * (1 + 1e-6) + 1e-44)          # ... and it is not loose: one f32 rounding above the residual
    assert np.all(z["codes"][:, d:] == 0) and np.abs(z["codes"].astype(int)).max() <= 127
    # degenerate rows (zero, subnormal scale) carry no codes: their bound is their norm
    for r in (496, 497):
        assert z["scale"][r] == 0 and not z["codes"][r].any()
        assert z["resid"][r] >= np.sqrt((z["rows"][r].astype(np.float64) ** 2).sum())
    # the query side: r_q bounds |q - s_q t|, |q|^ bounds |q|
    q64, info = z["queries"].astype(np.float64), z["info"].astype(np.float64)
    assert np.all(info[:, 2] >= np.sqrt(((q64 - info[:, :1] * z["t"][:, :d]) ** 2).sum(1)))
    assert np.all(info[:, 1] >= np.sqrt((q64 ** 2).sum(1)))


def test_planes_reconstruct_the_quantised_query(quantized):
    z = quantized
    h, l, t = z["h"].astype(np.int64), z["l"].astype(np.int64), z["t"].astype(np.int64)
    assert np.array_equal(128 * h + l, t)
    assert np.abs(h).max() <= 127 and l.min() >= -64 and l.max() <= 63 and np.abs(t).max() <= 16256
    assert np.abs(t).max(1)[:-1].min() >= 16255   # every non-zero query uses the whole range
    assert not t[-1].any() and z["info"][-1, 0] == 0   # the all-zero query


def test_split_covers_every_value(lib):
    q = np.zeros(1, np.float32)
    ts = np.arange(-16256, 16257)
    h = (ts + 64) // 128
    assert np.abs(h).max() == 127 and (ts - 128 * h).min() == -64 and (ts - 128 * h).max() == 63
    # through the library: a query whose elements hit every t
    q = (ts / 16256.0).astype(np.float32)
    hh, ll, tt, _ = quantize_queries(lib, q[None, :1024])
    assert np.array_equal(128 * hh.astype(int) + ll, tt)


def test_no_int32_overflow_at_the_largest_dimension(lib):
    ld8 = 1024
    assert lib.i8_cpu_ld(1024) == 1024 and lib.i8_cpu_dim_supported(1024) and not lib.i8_cpu_dim_supported(1025) and lib.i8_cpu_ld(750) == 768
    assert lib.i8_cpu_dim_supported(129) and not lib.i8_cpu_dim_supported(128) and not lib.i8_cpu_dim_supported(0)
    for sc, st in ((127, 16256), (-127, 16256), (127, -16256), (-127, -16256)):
        c = np.full(ld8, sc, np.int8)
        t = np.full(ld8, st, np.int64)
        h = (t + 64) // 128
        l = t - 128 * h
        ov = C.c_int(0)
        s = lib.i8_cpu_dot(_p(h.astype(np.int8), PI8), _p(l.astype(np.int8), PI8), _p(c, PI8), ld8, C.byref(ov))
        assert ov.value == 0 and s == ld8 * sc * st and abs(s) < 2 ** 31


def _stats(z, inv, upto=None):
    """the four statistics words of the rows [0, upto) as floats"""
    xx = (z["rows"][:upto].astype(np.float64) ** 2).sum(1)
    e, inv = z["resid"][:upto].astype(np.float64), inv[:upto].astype(np.float64)
    return np.float32(xx.max()), np.float32((xx * inv ** 2).max()), np.float32((e ** 2).max()), np.float32(((e * inv) ** 2).max())


def _slack(lib, z, metric, stats):
    """per query: G, and for L2 the f32 terms of the decomposed form as well (half of the filter's margin = delta + G)"""
    out = np.zeros(z["queries"].shape[0])
    for qi in range(out.shape[0]):
        m = np.zeros(2, np.float32)
        lib.i8_cpu_margin(metric, z["info"][qi, 3], z["d"], z["info"][qi, 1], z["info"][qi, 2], *stats, _p(m, PF))
        assert np.isfinite(m).all() and m[1] >= 2 * m[0]
        out[qi] = m[1] / 2 if metric == L2 else m[0]
    return out


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_bound_holds_against_float64_on_every_pair(lib, quantized, metric):
    z = quantized
    d, rows, queries = z["d"], z["rows"].astype(np.float64), z["queries"].astype(np.float64)
    nr, nq = rows.shape[0], queries.shape[0]
    norm = np.sqrt((rows ** 2).sum(1))
    inv = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1), 0).astype(np.float32)
    S = z["t"].astype(np.int64) @ z["codes"].astype(np.int64).T            # [nq][nr], exact
    assert np.abs(S).max() < 2 ** 31
    ov = C.c_int(0)
    for qi, r in ((0, 0), (5, 301), (150, 493), (199, 496)):               # the library's int32 evaluation agrees
        assert lib.i8_cpu_dot(_p(z["h"][qi], PI8), _p(z["l"][qi], PI8), _p(z["codes"][r], PI8), z["codes"].shape[1], C.byref(ov)) == S[qi, r] and not ov.value
    ip = queries @ rows.T
    if metric == IP:
        want = -ip
        aux = np.zeros(nr, np.float32)
    elif metric == L2:
        want = ((queries[:, None, :] - rows[None, :, :]) ** 2).sum(2)
        aux = (z["rows"] * z["rows"]).sum(1, dtype=np.float32)             # |x|^2 as an f32 sum
    else:
        want = -ip * inv.astype(np.float64)[None, :]
        aux = inv
    n = nq * nr
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32)[None, :], (nq, nr)).reshape(-1))
    per_q = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a, np.float32), nr))
    out = np.zeros((n, 3), np.float32)
    lib.i8_cpu_bounds_many(metric, n, _p(per_q(z["info"][:, 0]), PF), _p(rep(z["scale"]), PF), _p(np.ascontiguousarray(S.reshape(-1).astype(np.int32)), PI32),
                           _p(per_q(z["info"][:, 1]), PF), _p(rep(z["resid"]), PF), _p(per_q(z["info"][:, 3]), PF), _p(rep(aux), PF), _p(out, PF))
    approx, lo, up = (out[:, i].reshape(nq, nr).astype(np.float64) for i in range(3))
    assert np.all(lo <= approx) and np.all(approx <= up)
    slack = _slack(lib, z, metric, _stats(z, inv))
    half = (up - lo) / 2
    assert np.all(np.abs(approx - want) <= half + slack[:, None]), "|d~ - d(float64)| exceeds the bound"
    assert np.all(lo - slack[:, None] <= want) and np.all(want <= up + slack[:, None]), "[lo, up] does not bracket the float64 distance"
    # the window means something: for an index of the plain rows alone it stays below the spread of the distances.  Every residual component
    # is at most s_r / 2 with s_r = max|x| / 127 <= 6 sigma / 127, so |q| e_r <= (sigma sqrt(D)) (3 sigma / 127) sqrt(D) = 0.65 sigma^2 sqrt(D)
    # at 768 dims, and sigma^2 sqrt(D) is the spread of an inner product (twice that with L2's factor 2, whose spread is larger still)
    plain = half[:100, :300] + _slack(lib, z, metric, _stats(z, inv, 300))[:100, None]
    assert plain.max() < want[:100, :300].std()


# ---------------------------------------------------------------------------------------------------------------- the policy
GiB = 1 << 30
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES")


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


def test_scan_tier_under_every_environment(monkeypatch):
    from reindexer_amd import capi
    capi.lib()
    tier, policy = capi.scan_tier, capi.scan_policy
    rows_1g = GiB // (768 * 4) + 1
    _env(monkeypatch)
    # automatic: the int8 tier refines what the automatic mode accepts, from 1 GiB on, for dim <= 1024
    assert tier(10_000_000, 768) == 2 and tier(rows_1g, 768) == 2 and tier(rows_1g - 2, 768) == 0
    assert tier(200_000, 768) == 0 and tier(100_000, 128) == 0
    assert tier(10_000_000, 768, nq=2) == 0 and tier(10_000_000, 768, nq=8) == 0
    assert tier(10_000_000, 768, shadow_available=False) == 0 and tier(10_000_000, 768, stats_finite=False) == 0
    assert tier(40_000_000, 64) == 0 and tier(10_000_000, 640) == 0 and tier(10_000_000, 1100) == 0
    assert tier(10_000_000, 1024) == 2 and tier(10_000_000, 750) == 2 and tier(10_000_000, 200) == 2 and tier(10_000_000, 256) == 2 and tier(10_000_000, 129) == 0
    assert tier(40_000_000, 100) == 1 and tier(10_000_000, 128) == 1   # up to 128 dims a code row is as long as the bf16 row: the bf16 tier stays
    # only RXGPU_SCAN_BF16_MIN_BYTES lowered (what the bf16 tier's tests do): the bf16 tier
    _env(monkeypatch, BF16_MIN_BYTES=1000 * 128 * 4)
    assert tier(1000, 128) == 1 and tier(999, 128) == 0 and tier(10_000_000, 768) == 2
    _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1000 * 256 * 4)
    assert tier(1000, 256) == 2 and tier(999, 256) == 1 and tier(4000, 128) == 1
    _env(monkeypatch, I8_MIN_BYTES=1)                       # the int8 threshold alone never widens the automatic mode
    assert tier(1000, 256) == 0 and tier(rows_1g, 768) == 2
    _env(monkeypatch, BF16_MIN_BYTES=64 * GiB)
    assert tier(10_000_000, 768) == 0
    _env(monkeypatch, I8_MIN_BYTES=64 * GiB)
    assert tier(10_000_000, 768) == 1
    # RXGPU_SCAN_I8=0: only this tier off
    _env(monkeypatch, I8=0)
    assert tier(10_000_000, 768) == 1 and tier(200_000, 768) == 0
    _env(monkeypatch, I8=0, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
    assert tier(1000, 256) == 1
    # RXGPU_SCAN_I8=1: forced at any size, up to 8 queries, whatever the statistics say; still the dimension and the shadow
    _env(monkeypatch, I8=1)
    assert tier(100, 256) == 2 and tier(100, 256, nq=8) == 2 and tier(100, 256, stats_finite=False) == 2 and tier(100, 160) == 2 and tier(7, 750) == 2
    assert tier(100, 256, nq=9) == 0 and tier(100, 1100) == 0 and tier(100, 256, shadow_available=False) == 0
    assert tier(100, 128) == 0 and tier(100, 64) == 0 and tier(10_000_000, 128) == 1   # not a dimension of this tier: the automatic mode decides
    assert tier(10_000_000, 768, nq=9) == 0 and policy(100, 256) and not policy(100, 256, nq=9)
    # RXGPU_SCAN_BF16=0 wins over everything; =1 means the bf16 tier exactly
    _env(monkeypatch, BF16=0, I8=1)
    assert tier(10_000_000, 768) == 0 and tier(100, 128) == 0 and not policy(10_000_000, 768)
    _env(monkeypatch, BF16=0)
    assert tier(10_000_000, 768) == 0
    for i8 in ({}, {"I8": 1}, {"I8": 0}, {"I8_MIN_BYTES": 1}):
        _env(monkeypatch, BF16=1, **i8)
        assert tier(10_000_000, 768) == 1 and tier(100, 128) == 1 and tier(100, 128, nq=8) == 1 and tier(100, 128, stats_finite=False) == 1
        assert tier(100, 128, nq=9) == 0 and tier(100, 64) == 0 and tier(100, 128, shadow_available=False) == 0


def test_scan_policy_answers_are_unchanged(monkeypatch):
    """the exact calls of tests/test_gpu_scan_policy.py::test_policy_function_decides_as_documented, and tier > 0 wherever the policy says yes"""
    from reindexer_amd import capi
    capi.lib()
    rows_1g = GiB // (768 * 4) + 1
    both = lambda *a, **k: (capi.scan_policy(*a, **k), capi.scan_tier(*a, **k) > 0)
    _env(monkeypatch)
    for args, kw, want in [((10_000_000, 768), {}, True), ((rows_1g, 768), {}, True), ((rows_1g - 2, 768), {}, False), ((200_000, 768), {}, False),
                           ((100_000, 128), {}, False), ((10_000_000, 768), dict(nq=2), False), ((10_000_000, 768), dict(nq=8), False),
                           ((10_000_000, 768), dict(shadow_available=False), False), ((10_000_000, 768), dict(stats_finite=False), False),
                           ((40_000_000, 64), {}, False), ((10_000_000, 640), {}, False), ((10_000_000, 1100), {}, False), ((40_000_000, 100), {}, True),
                           ((10_000_000, 1024), {}, True), ((10_000_000, 750), {}, True)]:
        assert both(*args, **kw) == (want, want), (args, kw)
    _env(monkeypatch, BF16_MIN_BYTES=1000 * 128 * 4)
    assert both(1000, 128) == (True, True) and both(999, 128) == (False, False)
    _env(monkeypatch, BF16_MIN_BYTES=64 * GiB)
    assert both(10_000_000, 768) == (False, False)
    _env(monkeypatch, BF16=0)
    assert both(10_000_000, 768) == (False, False) and both(100_000_000, 128) == (False, False)
    _env(monkeypatch, BF16=1)
    assert both(100, 128) == (True, True) and both(100, 128, nq=8) == (True, True) and both(100, 128, stats_finite=False) == (True, True)
    assert both(100, 128, nq=9) == (False, False) and both(100, 64) == (False, False) and both(100, 128, shadow_available=False) == (False, False)
