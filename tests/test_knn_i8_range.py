"""The range bound of the int8 shadow tier (i8_range_bound in reindexer_amd/csrc/knn_i8_quant.h), compiled for the host
(tests/cpp/knn_i8_range_cpu.cc) and pinned on the CPU over the 100 000 (row, query) pairs of tests/test_knn_i8_quant.py's adversarial corpus:
no row whose f32 distance, as the oracle computes it, is within the radius has a lower bound above the threshold the range scan compares
against, at radii that ARE such distances and one ulp to either side; and the threshold excludes the rows that are far outside."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from . import i8_model
from .i8_model import COS, IP, L2, PF, PI32, _p, quantize_queries, quantize_rows
from .test_knn_i8_quant import corpus

LIB = Path(__file__).resolve().parent / "cpp" / "libknn_i8_range_cpu.so"


@pytest.fixture(scope="module")
def lib():
    return i8_model.load()


@pytest.fixture(scope="module")
def rlib():
    assert LIB.exists(), f"{LIB} is missing: run `python -m reindexer_amd.build`"
    so = C.CDLL(str(LIB))
    so.i8_range_cpu_bound.argtypes = [C.c_float, C.c_float]
    so.i8_range_cpu_bound.restype = C.c_float
    so.i8_range_cpu_bound_many.argtypes = [C.c_uint64, PF, PF, PF]
    return so


def bound_many(rlib, radius, margin):
    radius, margin = np.ascontiguousarray(radius, np.float32), np.ascontiguousarray(margin, np.float32)
    out = np.empty(radius.shape, np.float32)
    rlib.i8_range_cpu_bound_many(radius.size, _p(radius, PF), _p(margin, PF), _p(out, PF))
    return out


@pytest.fixture(scope="module", params=[768, 200])
def quantized(request, lib):
    d = request.param
    rows, queries = corpus(d, d)
    assert rows.shape[0] * queries.shape[0] == 100_000
    codes, scale, resid = quantize_rows(lib, rows)
    h, l, t, info = quantize_queries(lib, queries)
    norm = np.sqrt((rows.astype(np.float64) ** 2).sum(1))
    inv = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1), 0).astype(np.float32)
    S = (t.astype(np.int64) @ codes.astype(np.int64).T).astype(np.int32)   # [nq][nr], exact
    return dict(d=d, rows=rows, queries=queries, scale=scale, resid=resid, info=info, inv=inv, S=S)


def _pairs(lib, oracle, z, metric):
    """per (query, row): the f32 distance as the oracle computes it, the lower bound as the scan computes it; per query: the margin the query
    prep writes for an index of these rows"""
    rows, queries, inv, info = z["rows"], z["queries"], z["inv"], z["info"]
    nr, nq = rows.shape[0], queries.shape[0]
    with np.errstate(all="ignore"):
        dist = np.stack([oracle.dist_many(metric, queries[qi], rows, inv if metric == COS else None) for qi in range(nq)])
    aux = {IP: np.zeros(nr, np.float32), L2: (rows * rows).sum(1, dtype=np.float32), COS: inv}[metric]
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32)[None, :], (nq, nr)).reshape(-1))
    per_q = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a, np.float32), nr))
    out = np.zeros((nq * nr, 3), np.float32)
    lib.i8_cpu_bounds_many(metric, nq * nr, _p(per_q(info[:, 0]), PF), _p(rep(z["scale"]), PF), _p(np.ascontiguousarray(z["S"].reshape(-1)), PI32),
                           _p(per_q(info[:, 1]), PF), _p(rep(z["resid"]), PF), _p(per_q(info[:, 3]), PF), _p(rep(aux), PF), _p(out, PF))
    lo = out[:, 1].reshape(nq, nr)
    xx = (rows.astype(np.float64) ** 2).sum(1)
    e, i64 = z["resid"].astype(np.float64), inv.astype(np.float64)

    def margins(upto):
        stats = (np.float32(xx[:upto].max()), np.float32((xx * i64 ** 2)[:upto].max()), np.float32((e[:upto] ** 2).max()),
                 np.float32(((e * i64)[:upto] ** 2).max()))
        m = np.zeros((nq, 2), np.float32)
        for qi in range(nq):
            lib.i8_cpu_margin(metric, info[qi, 3], z["d"], info[qi, 1], info[qi, 2], *stats, _p(m[qi], PF))
        assert np.isfinite(m).all()
        return m[:, 1].copy()

    return dist, lo, margins


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_no_hit_lies_above_the_bound(lib, rlib, oracle, quantized, metric):
    z = quantized
    dist, lo, margins = _pairs(lib, oracle, z, metric)
    assert np.isfinite(dist).all() and np.isfinite(lo).all()
    margin = margins(None)
    nq, nr = dist.shape
    up1 = np.nextafter(dist, np.float32(np.inf), dtype=np.float32)
    dn1 = np.nextafter(dist, np.float32(-np.inf), dtype=np.float32)
    checked = 0
    for qi in range(nq):
        order = np.argsort(dist[qi], kind="stable")
        ds = dist[qi][order]
        worst = np.maximum.accumulate(lo[qi][order])             # the largest lower bound among the rows with the i smallest distances
        for radius in (dist[qi], up1[qi], dn1[qi]):                # a radius per pair: its distance, one ulp up, one ulp down
            inside = np.searchsorted(ds, radius, side="right")     # rows with d <= radius
            t = bound_many(rlib, radius, np.full(nr, margin[qi], np.float32))
            has = inside > 0
            assert np.all(worst[inside[has] - 1] <= t[has]), (metric, z["d"], qi)
            checked += int(has.sum())
    assert checked >= 2 * nq * nr + nq * nr // 2                  # (one ulp below a query's best distance, tied rows included, nothing is inside)


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_the_bound_excludes_rows_far_outside(lib, rlib, oracle, quantized, metric):
    """Not vacuous: on the plain Gaussian part of the corpus (an index of those 300 rows, the 100 plain queries, every pair's distance as a
    radius), of the rows with d > radius + 4 margin only a small share passes lo <= bound.  The share is NOT below 1 in 20 everywhere: the
    margin is the per-QUERY part of the error (2 delta + 2 G) while a row passes on its per-ROW window B_r = |q| e_r, which is far wider
    (the residual of a 7-bit code against a query quantised to 15 bits), so "4 margins outside" is still inside the window of the rows just
    beyond the radius.  Measured on this corpus with the arithmetic as it stood before the bound was added (lo and the margin are the KNN
    tier's), ip / l2 / cosine: 768 dims 0.1094 / 0.0843 / 0.1101, 200 dims 0.0499 / 0.0400 / 0.0504.  The bound asserted is the largest of
    those plus a fifth, 0.132.  What a vacuous threshold would do - let through rows whose lower bound is beyond the margin - is pinned
    exactly: no row with lo > radius + 2 margin passes at all."""
    z = quantized
    dist, lo, margins = _pairs(lib, oracle, z, metric)
    margin = margins(300)
    far = passed = 0
    for qi in range(100):
        d, l = dist[qi, :300], lo[qi, :300]
        t = bound_many(rlib, d, np.full(300, margin[qi], np.float32))                  # a radius per plain row
        outside = d[None, :].astype(np.float64) > d[:, None].astype(np.float64) + 4.0 * float(margin[qi])   # [radius][row]
        ok = l[None, :] <= t[:, None]
        far += int(outside.sum())
        passed += int((outside & ok).sum())
        beyond = l[None, :].astype(np.float64) > d[:, None].astype(np.float64) + 2.0 * float(margin[qi])
        assert not (beyond & ok).any(), (metric, z["d"], qi)
    share = passed / far
    print(f"metric={metric} d={z['d']}: {passed} of {far} rows with d > radius + 4 margin pass the bound ({share:.4f})")
    assert far > 1_000_000 and share < 0.132, (metric, z["d"], share)


def test_special_radii_and_margins(rlib):
    b = rlib.i8_range_cpu_bound
    inf, nan = float("inf"), float("nan")
    assert np.isnan(b(nan, 1e-3)) and np.isnan(b(nan, inf))                      # no row passes lo <= NaN; the f32 kernel finds no hit either
    assert b(1.0, inf) == inf and b(-inf, inf) == inf and b(1.0, nan) == inf    # no finite margin: no bound
    assert b(inf, 1e-3) == inf and b(-inf, 1e-3) == -inf
    for r in (0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 3e38, -3e38, 1e-45, -1e-45, 123456.0, -123456.0):
        for m in (0.0, 1e-45, 1e-7, 1e-3, 10.0):
            r32, m32 = np.float32(r), np.float32(m)
            t = np.float32(b(r, m))
            assert float(t) > float(r32) + float(m32) or t == np.float32(inf), (r, m, t)   # rounded outward: above the real sum
            assert float(t) <= float(np.nextafter(np.nextafter(np.float32(r32 + m32), np.float32(inf)), np.float32(inf))), (r, m, t)
