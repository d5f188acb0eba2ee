"""The 6-bit shadow of the int8-pruned scan (reindexer_amd/csrc/knn_i6_quant.h), compiled for the host (tests/cpp/knn_i6_quant_cpu.cc) and
pinned on the CPU: the tile layout packs and unpacks every code at every chunk count, the integer sum the scan forms from the packed planes
is the exact dot product and cannot overflow, and the window of knn_i8_quant.h, fed with 6-bit codes and their residuals, still brackets
the float64 distance on the adversarial rows of tests/test_knn_i8_quant.py."""
import ctypes as C

import numpy as np
import pytest

from . import i6_model, i8_model
from .i6_model import BIAS, CODE_MAX, PU8
from .i8_model import COS, IP, L2, PF, PI8, PI32, _p, quantize_queries
from .test_knn_i8_quant import corpus

DIMS = [129, 256, 300, 750, 768, 1024]


@pytest.fixture(scope="module")
def lib6():
    return i6_model.load()


@pytest.fixture(scope="module")
def lib8():
    return i8_model.load()


@pytest.mark.parametrize("d", DIMS)
def test_pack_and_unpack_round_trip(lib6, d):
    """every code value at every position class of a lane's 16 codes, rows 0..3 of a tile and a partial last tile; pad bytes and the rows the
    last tile lacks stay zero; a row's bytes are its own"""
    ld6 = lib6.i6_cpu_ld(d)
    assert ld6 == (d + 255) // 256 * 256
    n = 64 + 3                                                   # 16 whole tiles and one of three rows
    rng = np.random.default_rng(d)
    u = np.zeros((n, ld6), np.uint8)
    u[:, :d] = rng.integers(1, 64, (n, d))
    for v in range(64):                                          # row v: value v everywhere; rows 64..66: a ramp over all values
        u[v, :d] = v
    u[64:, :d] = (np.arange(d)[None, :] + np.arange(3)[:, None]) % 64
    shadow = i6_model.pack(lib6, u)
    assert shadow.size == (n + 3) // 4 * 3 * ld6 == lib6.i6_cpu_shadow_bytes(n, ld6)   # 0.75 bytes per element, whole tiles
    assert np.array_equal(i6_model.unpack(lib6, shadow, n, ld6), u)
    # the last tile's fourth row, and every pad code, is zero bits: unpacking one more row gives zeros, and zero rows pack to zero bytes
    assert not i6_model.unpack(lib6, shadow, n + 1, ld6)[n].any()
    assert not i6_model.pack(lib6, np.zeros((n, ld6), np.uint8)).any()
    # a row's bytes are its own: changing one row changes no byte another row reads
    v = u.copy()
    v[5, :d] = 63 - v[5, :d]
    other = i6_model.unpack(lib6, i6_model.pack(lib6, v), n, ld6)
    assert np.array_equal(np.delete(other, 5, 0), np.delete(u, 5, 0)) and np.array_equal(other[5], v[5])
    changed = np.flatnonzero(i6_model.pack(lib6, v) != shadow)
    assert changed.size and changed.min() >= 3 * ld6 and changed.max() < 6 * ld6   # inside tile 1 (rows 4..7)


@pytest.mark.parametrize("d", DIMS)
def test_integer_sum_is_the_exact_dot_product(lib6, lib8, d):
    """S = dot(t, u) - 32 sum(t) from the packed planes == the int64 dot(t, c), for the extreme codes and the extreme query and for random ones"""
    ld6 = lib6.i6_cpu_ld(d)
    rng = np.random.default_rng(100 + d)
    codes = np.stack([np.full(d, CODE_MAX), np.full(d, -CODE_MAX), np.where(np.arange(d) % 2, CODE_MAX, -CODE_MAX),
                      rng.integers(-CODE_MAX, CODE_MAX + 1, d), np.zeros(d, np.int64)])
    u = np.zeros((codes.shape[0], ld6), np.uint8)
    u[:, :d] = codes + BIAS
    shadow = i6_model.pack(lib6, u)
    ts = np.stack([np.full(d, 16256), np.full(d, -16256), np.where(np.arange(d) % 2, -16256, 16256), rng.integers(-16256, 16257, d)])
    for t in ts:
        tp = np.zeros(ld6, np.int64)
        tp[:d] = t
        h = (tp + 64) // 128
        l = tp - 128 * h
        assert np.abs(h).max() <= 127 and l.min() >= -64 and l.max() <= 63
        for r in range(codes.shape[0]):
            ov = C.c_int(0)
            s = lib6.i6_cpu_sum(_p(h.astype(np.int8), PI8), _p(l.astype(np.int8), PI8), _p(shadow, PU8), r, ld6, C.byref(ov))
            want = int((t * codes[r]).sum())
            assert not ov.value and s == want and abs(want) < 2 ** 31, (d, r, s, want)
    assert 1024 * 63 * 16256 < 2 ** 31 and 32 * 1024 * 16256 < 2 ** 31


@pytest.fixture(scope="module", params=[768, 200])
def quantized(request, lib6, lib8):
    d = request.param
    rows, queries = corpus(d, d)
    u, scale, resid = i6_model.quantize_rows(lib6, rows)
    h, l, t, info = quantize_queries(lib8, queries)
    return dict(d=d, rows=rows, queries=queries, u=u, scale=scale, resid=resid, t=t, info=info)


def test_codes_and_stored_residual(quantized):
    z = quantized
    d = z["d"]
    c = z["u"][:, :d].astype(np.int64) - BIAS
    assert np.abs(c).max() == CODE_MAX and not z["u"][:, d:].any() and z["u"][:, :d].min() >= 1 and z["u"].max() <= 63
    real = np.sqrt(((z["rows"].astype(np.float64) - z["scale"].astype(np.float64)[:, None] * c) ** 2).sum(1))
    assert np.all(z["resid"].astype(np.float64) >= real) and np.all(z["resid"] <= real * (1 + 1e-6) + 1e-44)
    for r in (496, 497):                                          # degenerate rows carry no codes (u = 32): their bound is their norm
        assert z["scale"][r] == 0 and np.all(z["u"][r, :d] == BIAS)


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_window_holds_against_float64(lib8, quantized, metric):
    """lo_r <= d_r + margin / 2 for every pair and T >= D_kk - margin / 2 for every query, d in float64, T the kk-th smallest up_r"""
    z = quantized
    kk = 11
    d, rows, queries = z["d"], z["rows"].astype(np.float64), z["queries"].astype(np.float64)
    nr, nq = rows.shape[0], queries.shape[0]
    norm = np.sqrt((rows ** 2).sum(1))
    inv = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1), 0).astype(np.float32)
    S = z["t"][:, :d].astype(np.int64) @ (z["u"][:, :d].astype(np.int64) - BIAS).T
    assert np.abs(S).max() < 2 ** 31
    ip = queries @ rows.T
    if metric == IP:
        want, aux = -ip, np.zeros(nr, np.float32)
    elif metric == L2:
        want, aux = ((queries[:, None, :] - rows[None, :, :]) ** 2).sum(2), (z["rows"] * z["rows"]).sum(1, dtype=np.float32)
    else:
        want, aux = -ip * inv.astype(np.float64)[None, :], inv
    n = nq * nr
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32)[None, :], (nq, nr)).reshape(-1))
    per_q = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a, np.float32), nr))
    out = np.zeros((n, 3), np.float32)
    lib8.i8_cpu_bounds_many(metric, n, _p(per_q(z["info"][:, 0]), PF), _p(rep(z["scale"]), PF), _p(np.ascontiguousarray(S.reshape(-1).astype(np.int32)), PI32),
                            _p(per_q(z["info"][:, 1]), PF), _p(rep(z["resid"]), PF), _p(per_q(z["info"][:, 3]), PF), _p(rep(aux), PF), _p(out, PF))
    lo, up = (out[:, i].reshape(nq, nr).astype(np.float64) for i in (1, 2))
    xx = (rows ** 2).sum(1)
    e = z["resid"].astype(np.float64)
    stats = (np.float32(xx.max()), np.float32((xx * inv.astype(np.float64) ** 2).max()), np.float32((e ** 2).max()),
             np.float32(((e * inv) ** 2).max()))                   # the two row maxima and the two maxima of the 6-bit residuals
    half = np.zeros(nq)
    for qi in range(nq):
        m = np.zeros(2, np.float32)
        lib8.i8_cpu_margin(metric, z["info"][qi, 3], d, z["info"][qi, 1], z["info"][qi, 2], *stats, _p(m, PF))
        assert np.isfinite(m).all()
        half[qi] = np.float64(m[1]) / 2
    assert np.all(lo <= want + half[:, None]), "lo_r > d_r + margin / 2"
    T = np.sort(up, axis=1)[:, kk - 1]
    D_kk = np.sort(want, axis=1)[:, kk - 1]
    assert np.all(T >= D_kk - half), "T < D_kk - margin / 2"
