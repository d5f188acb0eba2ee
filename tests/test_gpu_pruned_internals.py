"""-m gpu: what the pruned single-query chains keep ON THE DEVICE, read back through rxgpu_index_inspect and held against the CPU model of
the int8 tier (tests/i8_model.py: reindexer_amd/csrc/knn_i8_quant.h compiled for the host) and float64 numpy.

The chains are exact only because of inequalities proven in knn_i8_quant.h and in the header of the bf16 scan (knn_scan.hip):
    int8:  lo_r <= d_r + margin/2 for every row, and T >= D_kk - margin/2        bf16:  |d~_r - d_r| <= margin/2
A comparison of final results does not see a bound that is unsound but wide enough; these tests look at the quantities themselves:
  A  the shadows as built: codes, {s_r, e_r}, the statistics words, |x|^2 per row, the bf16 rows
  B  the query side: planes, s_q, |q|^, |q|^2, the margin
  C  the scan: lo_r / d~_r of every row (or list position), T
  D  the filter: the number and the set of the candidates
  E  the incremental upkeep of A under upload_rows / move_row / truncate / reserve, against a fresh index of the same rows
Device and model are compiled with -ffp-contract=off, so equality is asked wherever both see the same inputs; where the device sums in
another order than the model (the lane-parallel fp64 sums behind e_r, |q|^ and r_q, the f32 |q|^2) the device's own value is fed into the
model and the value itself is held to one ulp / the standard summation bound.  Exact distances d_r are rxgpu_distances.

Data: the benchmark's distribution (make_corpus) with adversarial rows scattered through it - a block scaled by exp(U(-14, hi)), one row
with a single component `spike` x the rest, a zero row - and the query equal to a stored row.  hi = 14 and spike = 10^6 under cosine, whose
margin sees |x| inv_norm = 1 whatever the magnitudes.  L2 and ip keep to hi = 0 and spike = 30 wherever D is checked: their margins grow
with the index-wide maxima - ip: 2 r_q max |x| with r_q ~ 2^-13 |q|; L2: 4 gamma max |x|^2 on top, gamma = 1.1 (D + 64) 2^-24 - while
the distances of the ordinary rows do not, so one row of norm 10^3 |q| puts every ordinary row within the margin of T: the filter then
passes all of them, which pins nothing about it, and no list of 4096 holds more rows than that.  Large magnitudes under L2 and ip are the
bulk case's.  Every case of C and D asserts candidates <= capacity and the tier's profile slot == 1: the chain itself, not the exact scan
behind its gate, produced what is checked.  The case with adversarial rows in bulk may overflow and asserts A, B and the per-row
inequality only.

Printed, not asserted: the largest (lo_r - d_r) / (margin/2) resp. |d~_r - d_r| / (margin/2) per case - how much of the proven room the
data uses (DESIGN.md keeps the figures)."""
import ctypes as C

import numpy as np
import pytest

from . import i8_model
from .conftest import make_corpus
from .i8_model import PF, PI32, _p, quantize_queries, quantize_rows

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
METRICS = [L2, IP, COS]
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_WG_PER_CU")
U = 2.0 ** -24
LIST_CAP = 4096
PRUNED = {"i8": ("pruned_values", "pruned_margin", "pruned_q_sq", "pruned_qinfo", "pruned_qplanes", "pruned_top", "pruned_cand_rows"),
          "bf16": ("pruned_values", "pruned_margin", "pruned_q_sq", "pruned_top", "pruned_cand_rows")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ulps(a, b):
    """distance in units of the last place between non-negative floats"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def _env(mp, **kw):
    for name in ENV:
        mp.delenv(name, raising=False)
    for k, v in kw.items():
        mp.setenv("RXGPU_SCAN_" + k, str(v))


@pytest.fixture(scope="module")
def lib():
    return i8_model.load()


# ---------------------------------------------------------------------------------------------------------------- data
def corpus(oracle, metric, seed, n, d, hi=14.0, spike=1e6, block=24):
    """(rows, inv_norms or None, query, row the query equals)"""
    rng = np.random.default_rng(seed)
    rows = make_corpus(seed, n, d)
    block = min(block, n // 3)
    special = rng.choice(n, block + 3, replace=False)
    rows[special[:block]] = (rng.normal(0, 1, (block, d)) * np.exp(rng.uniform(-14, hi, (block, 1)))).astype(np.float32)
    rows[special[block], int(rng.integers(0, d))] *= np.float32(spike)
    rows[special[block + 1]] = 0.0
    inv = oracle.l2_modules(rows) if metric == COS else None
    query = rows[special[block + 2]].copy()
    if metric == COS:
        query = oracle.normalize_copy(query)[0]
    return rows, inv, query, int(special[block + 2])


def _mag(metric):
    """the adversarial magnitudes a case of D can carry (module docstring)"""
    return {} if metric == COS else dict(hi=0.0, spike=30.0)


# ---------------------------------------------------------------------------------------------------------------- one search, with what it left
def pruned_search(ix, mp, tier, query, kk, ids=None, wg=None):
    """one query through the forced tier with profiling on -> (result, launches of the tier's scan slot, candidates, cap, the pruned_* buffers)"""
    env = dict(I8=1) if tier == "i8" else dict(BF16=1)
    if wg:
        env["I8_WG_PER_CU"] = wg
    _env(mp, **env)
    slot = "scan_bf16" if tier == "bf16" else "scan_i8" if ids is None else "scan_i8_subset"
    ix.profile_enable(True)
    res = ix.search_knn(query[None, :], kk) if ids is None else ix.search_knn_subset(query[None, :], kk, ids)
    launches = ix.profile_read(slot)[0]
    cand, cap = ix.last_candidates()
    snap = {name: ix.inspect(name).copy() for name in PRUNED[tier]}   # before any other call on the index
    ix.profile_enable(False)
    _env(mp)
    return res, launches, cand, cap, snap


# ---------------------------------------------------------------------------------------------------------------- A
def check_stats(ix, metric, rows, inv, e_r=None):
    """the statistics words bound what they stand for -> the words as floats"""
    stats = ix.inspect("stats")
    assert stats.shape == (5,) and stats[2] == 0, stats
    w = stats.view(np.float32)
    norm = np.sqrt((rows.astype(np.float64) ** 2).sum(1))
    assert 1.01 * np.sqrt(np.float64(w[0])) >= norm.max(), (w[0], norm.max())
    if metric == COS:
        assert 1.01 * np.sqrt(np.float64(w[1])) >= (norm * inv.astype(np.float64)).max(), w[1]
    if e_r is not None:   # f32 exactly as knn_i8_build forms them
        assert w[3] >= (e_r * e_r).max(), (w[3], (e_r * e_r).max())
        if metric == COS:
            ei = e_r * inv
            assert w[4] >= (ei * ei).max(), (w[4], (ei * ei).max())
    return w


def check_row_sq(ix, rows):
    row_sq = ix.inspect("row_sq")
    xx = (rows.astype(np.float64) ** 2).sum(1)
    d = rows.shape[1]
    assert row_sq.shape == xx.shape
    bad = np.abs(row_sq.astype(np.float64) - xx) > (d / 16 + 4) * U * xx   # 16 lanes: chains of ceil(D / 16) fmaf + 4 butterfly adds
    assert not bad.any(), (np.flatnonzero(bad)[:5], row_sq[bad][:5], xx[bad][:5])
    return row_sq


def check_i8_shadow(lib, ix, metric, rows, inv):
    """A for the int8 shadow -> (codes, s_r, e_r, the statistics words as floats)"""
    n, d = rows.shape
    ld8 = lib.i8_cpu_ld(d)
    codes = ix.inspect("codes_i8").reshape(n, ld8)
    side = ix.inspect("side_i8").reshape(n, 2)
    s_r, e_r = np.ascontiguousarray(side[:, 0]), np.ascontiguousarray(side[:, 1])
    mc, ms, me = quantize_rows(lib, rows)
    assert np.array_equal(bits(s_r), bits(ms)), np.flatnonzero(bits(s_r) != bits(ms))[:5]
    assert np.array_equal(codes, mc), np.argwhere(codes != mc)[:5]      # the zero pad up to ld8 included
    resid = np.sqrt(((rows.astype(np.float64) - s_r.astype(np.float64)[:, None] * codes[:, :d]) ** 2).sum(1))
    assert np.all(e_r.astype(np.float64) >= resid), np.flatnonzero(e_r < resid)[:5]   # the premise of the bound, from the DEVICE's codes
    assert _ulps(e_r, me).max() <= 1, np.flatnonzero(_ulps(e_r, me) > 1)[:5]          # a reordered fp64 sum moves i8_norm_up by an ulp at most
    return codes, s_r, e_r, check_stats(ix, metric, rows, inv, e_r)


def check_bf16_shadow(ix, rows):
    n, d = rows.shape
    ld = (d + 63) // 64 * 64
    got = ix.inspect("rows_bf16").reshape(n, ld)
    u = np.ascontiguousarray(rows).view(np.uint32).astype(np.uint64)
    want = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)            # round to nearest even
    assert np.array_equal(got[:, :d], want), np.argwhere(got[:, :d] != want)[:5]
    assert not got[:, d:].any()
    return got


# ---------------------------------------------------------------------------------------------------------------- B
def check_q_sq(snap, query):
    d = query.shape[0]
    q_sq = snap["pruned_q_sq"][0]
    true = (query.astype(np.float64) ** 2).sum()
    assert abs(np.float64(q_sq) - true) <= (d / 64 + 6) * U * true, (q_sq, true)   # 64 lanes: chains of ceil(D / 64) fmaf + 6 butterfly adds
    return q_sq


def check_i8_query(lib, snap, metric, query, w):
    """B for the int8 tier -> (t of the device's planes, s_q, |q|^, |q|^2, margin)"""
    d = query.shape[0]
    ld8 = lib.i8_cpu_ld(d)
    h, l, t, info = quantize_queries(lib, query[None, :])
    planes = snap["pruned_qplanes"].reshape(2, ld8).astype(np.int64)
    assert np.abs(planes[0]).max() <= 127 and planes[1].min() >= -64 and planes[1].max() <= 63
    t_dev = 128 * planes[0] + planes[1]
    assert np.array_equal(t_dev, t[0]), np.flatnonzero(t_dev != t[0])[:5]
    s_q, qn = snap["pruned_qinfo"]
    assert bits(s_q) == bits(info[0, 0]), (s_q, info[0, 0])
    assert _ulps(qn, info[0, 1]) <= 1 and np.float64(qn) >= np.sqrt((query.astype(np.float64) ** 2).sum()), (qn, info[0, 1])
    q_sq = check_q_sq(snap, query)
    margin = snap["pruned_margin"][0]
    rq = info[0, 2]
    lim = []
    for r in (np.nextafter(rq, np.float32(0)), np.nextafter(rq, np.float32(np.inf))):   # r_q is a reordered fp64 sum as well: one ulp
        m = np.zeros(2, np.float32)
        lib.i8_cpu_margin(metric, q_sq, d, qn, r, w[0], w[1], w[3], w[4], _p(m, PF))
        lim.append(m[1])
    assert lim[0] <= margin <= lim[1] and np.isfinite(margin), (lim, margin)
    return t_dev, np.float32(s_q), np.float32(qn), np.float32(q_sq), np.float32(margin)


# ---------------------------------------------------------------------------------------------------------------- C, D
def check_top_and_filter(snap, res, values, upper, dist, listed, kk, margin, cand, cap, what, filter_too=True):
    """T against the values the top lists were made of (`upper`), then D: the filter over `values`; listed = the rows the positions stand for"""
    m = values.shape[0]
    kk = min(kk, m)
    top = snap["pruned_top"]
    assert top.shape == (kk + 1,) and top[kk] == kk, (what, top)
    T = top[:kk].view(np.float32)[kk - 1]
    assert bits(T) == bits(np.sort(upper)[kk - 1]), (what, T, np.sort(upper)[kk - 1])
    order = np.lexsort((listed, dist))[:kk]                     # the exact top-kk under (dist, row)
    if not filter_too:
        return T
    assert cand <= cap, (what, "the candidate list overflowed: the exact scan behind the gate answered", cand, cap)
    passing = values <= np.float32(T) + np.float32(margin)      # the sum in f32, as knn_filter_approx forms it
    assert cand == int(passing.sum()), (what, cand, int(passing.sum()))
    got = snap["pruned_cand_rows"]
    assert got.shape == (cand,) and np.array_equal(np.sort(got), listed[passing]), what   # (listed ascends)
    assert np.isin(listed[order], got).all(), (what, "a row of the exact top-kk is no candidate")
    assert int(res[2][0]) == kk and np.array_equal(res[1][0, :kk], listed[order]), what
    assert np.array_equal(bits(res[0][0, :kk]), bits(dist[order])), what
    return T


def check_i8_scan(lib, ix, snap, res, metric, query, kk, shadow, q, aux_all, cand, cap, what, ids=None, filter_too=True):
    """C and D for the int8 tier; shadow = (codes, s_r, e_r), q = (t, s_q, |q|^, |q|^2, margin) of the device -> the largest (lo - d) / (margin / 2)"""
    codes, s_r, e_r = shadow
    t_dev, s_q, qn, q_sq, margin = q
    listed = np.arange(codes.shape[0], dtype=np.uint32) if ids is None else ids
    m = listed.shape[0]
    S = codes[listed].astype(np.int64) @ t_dev                  # the integer dot over the device's planes and codes: exact
    assert np.abs(S).max() < 2 ** 31
    ov = C.c_int(0)
    ld8 = codes.shape[1]
    planes = np.ascontiguousarray(snap["pruned_qplanes"].reshape(2, ld8))
    for j in (0, m // 2, m - 1):                                # ... and the model's int32 evaluation agrees
        row = np.ascontiguousarray(codes[listed[j]])
        assert lib.i8_cpu_dot(_p(planes[0], i8_model.PI8), _p(planes[1], i8_model.PI8), _p(row, i8_model.PI8), ld8, C.byref(ov)) == S[j] and not ov.value
    full = lambda v: np.full(m, v, np.float32)
    aux = np.ascontiguousarray(aux_all[listed], np.float32) if aux_all is not None else np.zeros(m, np.float32)
    out = np.zeros((m, 3), np.float32)
    lib.i8_cpu_bounds_many(metric, m, _p(full(s_q), PF), _p(np.ascontiguousarray(s_r[listed]), PF), _p(np.ascontiguousarray(S.astype(np.int32)), PI32),
                           _p(full(qn), PF), _p(np.ascontiguousarray(e_r[listed]), PF), _p(full(q_sq), PF), _p(aux, PF), _p(out, PF))
    lo, up = np.ascontiguousarray(out[:, 1]), np.ascontiguousarray(out[:, 2])
    values = snap["pruned_values"]
    assert values.shape == (m,), (what, values.shape)
    assert np.array_equal(bits(values), bits(lo)), (what, np.flatnonzero(bits(values) != bits(lo))[:5])
    dist = ix.distances(query, listed)
    room = (values.astype(np.float64) - dist.astype(np.float64)) / (np.float64(margin) / 2)
    assert room.max() <= 1.0, (what, "lo_r > d_r + margin/2", int(room.argmax()), room.max())
    T = check_top_and_filter(snap, res, values, up, dist, listed, kk, margin, cand, cap, what, filter_too)
    D_kk = np.sort(dist)[min(kk, m) - 1]
    assert np.float64(T) >= np.float64(D_kk) - np.float64(margin) / 2, (what, T, D_kk, margin)
    return float(room.max())


def run_i8_case(lib, ix, mp, metric, rows, inv, query, kk, what, ids=None, wg=None, shadow=None, filter_too=True):
    """A (unless `shadow` carries an earlier call's), B, C and D of one forced int8 search -> (shadow, room used)"""
    res, launches, cand, cap, snap = pruned_search(ix, mp, "i8", query, kk, ids, wg)
    assert launches == 1, (what, launches)
    n = rows.shape[0]
    assert cap == min(LIST_CAP, max(64, ((n if ids is None else ids.size) + 63) // 64 * 64)), (what, cap)
    if shadow is None:
        codes, s_r, e_r, w = check_i8_shadow(lib, ix, metric, rows, inv)
        aux = check_row_sq(ix, rows) if metric == L2 else inv
        shadow = (codes, s_r, e_r, w, aux)
    codes, s_r, e_r, w, aux = shadow
    q = check_i8_query(lib, snap, metric, query, w)
    room = check_i8_scan(lib, ix, snap, res, metric, query, kk, (codes, s_r, e_r), q, aux, cand, cap, what, ids, filter_too)
    return shadow, room, cand


def run_bf16_case(lib, ix, mp, metric, rows, inv, query, kk, what):
    res, launches, cand, cap, snap = pruned_search(ix, mp, "bf16", query, kk)
    assert launches == 1, (what, launches)
    n, d = rows.shape
    check_bf16_shadow(ix, rows)
    w = check_stats(ix, metric, rows, inv)
    if metric == L2:
        check_row_sq(ix, rows)
    q_sq = check_q_sq(snap, query)
    margin = snap["pruned_margin"][0]
    assert bits(margin) == bits(np.float32(lib.i8_cpu_f32_margin(metric, 1, q_sq, d, w[0], w[1]))), (what, margin)
    values = snap["pruned_values"]
    listed = np.arange(n, dtype=np.uint32)
    dist = ix.distances(query, listed)
    room = np.abs(values.astype(np.float64) - dist.astype(np.float64)) / (np.float64(margin) / 2)
    assert values.shape == (n,) and room.max() <= 1.0, (what, "|d~_r - d_r| > margin/2", int(room.argmax()), room.max())
    check_top_and_filter(snap, res, values, values, dist, listed, kk, margin, cand, cap, what)
    return float(room.max()), cand


# ---------------------------------------------------------------------------------------------------------------- the int8 tier, every row
# one shape per code-row chunk count 1..4 (130 and 750 leave a float4 tail), n off the multiples of 16 and 64, and the tails of one step
I8_SHAPES = [(130, 4_099, 11), (300, 4_099, 1), (300, 4_099, 11), (300, 4_099, 64), (750, 4_099, 11), (1024, 2_051, 11), (256, 13, 11), (256, 16, 11),
             (256, 17, 11)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n,kk", I8_SHAPES)
def test_int8_tier_on_the_device(rxgpu, oracle, lib, monkeypatch, metric, d, n, kk):
    rows, inv, query, _ = corpus(oracle, metric, 1000 + d + n + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, room, cand = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, d, n, kk))
    print(f"room int8 metric={metric} d={d} n={n} kk={kk}: max (lo - d) / (margin/2) = {room:.3g}, {cand} candidates")


@pytest.mark.parametrize("metric", METRICS)
def test_int8_tier_with_every_wavefront_looping(rxgpu, oracle, lib, monkeypatch, metric):
    """40 003 rows at one workgroup per CU: 2 501 steps of 16 rows over 1 024 wavefronts, so every wavefront goes round its double-buffered
    loop more than twice"""
    d, n, kk = 256, 40_003, 11
    rows, inv, query, _ = corpus(oracle, metric, 2000 + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, room, cand = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, "looping"), wg=1)
    print(f"room int8 metric={metric} d={d} n={n} kk={kk}: max (lo - d) / (margin/2) = {room:.3g}, {cand} candidates")


@pytest.mark.parametrize("metric", METRICS)
def test_int8_tier_with_adversarial_rows_in_bulk(rxgpu, oracle, lib, monkeypatch, metric):
    """every row scaled by exp(U(-14, 14)): the list may overflow (the gate answers then), so A, B and the per-row inequality only"""
    d, n, kk = 256, 4_099, 11
    rng = np.random.default_rng(3000 + metric)
    rows = (rng.normal(0, 1, (n, d)) * np.exp(rng.uniform(-14, 14, (n, 1)))).astype(np.float32)
    rows[1000, 5] *= np.float32(1e6)
    rows[1001] = 0.0
    inv = oracle.l2_modules(rows) if metric == COS else None
    query = oracle.normalize_copy(rows[7])[0] if metric == COS else rows[7].copy()
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, room, cand = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, "bulk"), filter_too=False)
    print(f"room int8 bulk metric={metric} d={d} n={n}: max (lo - d) / (margin/2) = {room:.3g}, {cand} candidates")


# ---------------------------------------------------------------------------------------------------------------- the int8 tier over row lists
def _list(rng, n, density, ends):
    keep = rng.random(n) < density
    keep[0] = keep[n - 1] = ends
    return np.flatnonzero(keep).astype(np.uint32)


@pytest.mark.parametrize("metric", METRICS)
def test_int8_tier_over_row_lists(rxgpu, oracle, lib, monkeypatch, metric):
    """lower bounds by LIST POSITION, the side pair / |x|^2 / inv_norm of the listed row, candidates mapped back to rows"""
    d, n, kk = 300, 4_099, 11
    rows, inv, query, at = corpus(oracle, metric, 4000 + metric, n, d, **_mag(metric))
    rng = np.random.default_rng(4100 + metric)
    lists = {f"{dens}{'+ends' if ends else ''}": _list(rng, n, dens, ends) for dens in (0.5, 0.03) for ends in (False, True)}
    for length in (1, 15, 16, 17, 63, 64, 65):
        ids = np.sort(rng.choice(n, length, replace=False)).astype(np.uint32)
        ids[length // 2] = at if at not in ids else ids[length // 2]   # the row the query equals is on the list
        lists[str(length)] = np.unique(ids).astype(np.uint32)
    rooms = {}
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        shadow = None
        for name, ids in lists.items():
            assert name[0] == "0" or ids.size == int(name)
            shadow, rooms[name], _ = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, name), ids=ids, shadow=shadow)
    print(f"room int8 lists metric={metric} d={d} n={n}: " + ", ".join(f"{k}: {v:.3g}" for k, v in rooms.items()))


def test_int8_tier_over_a_long_list_in_chunks(rxgpu, oracle, lib, monkeypatch):
    """the chunked, double-buffered form of the gather kernel (the list of test_gpu_scan_i8_subset.py::test_long_list_takes_the_chunked_kernel), L2:
    the side pair and |x|^2 both follow the list"""
    metric, d, n, kk = L2, 256, 140_003, 11
    rows, inv, query, at = corpus(oracle, metric, 5000, n, d, **_mag(metric))
    ids = np.flatnonzero(np.arange(n) % 17 != 3).astype(np.uint32)
    assert ids.size > 131_072 and ids.size % 64 and ids[0] == 0 and ids[-1] == n - 1
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, room, cand = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, "chunked", ids=ids, wg=1)
    print(f"room int8 chunked list metric={metric} d={d} n={ids.size}: max (lo - d) / (margin/2) = {room:.3g}, {cand} candidates")


def test_int8_tier_through_a_shard_view(rxgpu, oracle, lib, monkeypatch):
    """shard 1 of a two-shard index on device 0, searched and inspected through its view; the sharded handle itself has nothing to inspect"""
    metric, d, n, kk = COS, 256, 4_099, 11
    rows, inv, _, _ = corpus(oracle, metric, 6000, n, d, **_mag(metric))
    with rxgpu.ShardedVectorIndex(metric, d, n, [0, 0]) as sx:
        sx.upload_rows(0, rows, inv)
        with pytest.raises(rxgpu.RxGpuError) as err:
            sx.inspect("stats")
        assert err.value.code == rxgpu.RXGPU_ERR_PARAMS
        first = sx.shard_rows
        view = sx.shard(1)
        local, local_inv = rows[first:], inv[first:]
        assert view.count == local.shape[0] > 0
        query = oracle.normalize_copy(local[local.shape[0] // 2])[0]
        _, room, cand = run_i8_case(lib, view, monkeypatch, metric, local, local_inv, query, kk, "shard 1")
    print(f"room int8 shard view metric={metric} d={d} n={local.shape[0]}: max (lo - d) / (margin/2) = {room:.3g}, {cand} candidates")


# ---------------------------------------------------------------------------------------------------------------- the bf16 tier
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [24, 100, 768])
def test_bf16_tier_on_the_device(rxgpu, oracle, lib, monkeypatch, metric, d):
    n, kk = 4_099, 11
    rows, inv, query, _ = corpus(oracle, metric, 7000 + d + metric, n, d, **_mag(metric))
    _env(monkeypatch, BF16=1)
    served = rxgpu.scan_tier(n, d) == 1
    assert served == (d != 24)   # rows of 64 bf16 elements (up to 64 dims) have no kernel in this tier: the policy keeps them on the f32 scan
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        if served:
            room, cand = run_bf16_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, d))
            print(f"room bf16 metric={metric} d={d} n={n}: max |d~ - d| / (margin/2) = {room:.3g}, {cand} candidates")
            return
        # 24 dims: the forced tier does not take the call (so there is no scan to look at), and says so - the f32 scan answers and nothing is
        # recorded; the bf16 shadow of such rows exists for the batched nomination and is checked as built by it
        ix.profile_enable(True)
        ix.search_knn(query[None, :], kk)
        assert tuple(ix.profile_read(s)[0] for s in ("scan", "scan_bf16", "scan_i8")) == (1, 0, 0)
        for name in ("pruned_values", "rows_bf16"):
            with pytest.raises(rxgpu.RxGpuError) as err:
                ix.inspect(name)
            assert err.value.code == rxgpu.RXGPU_ERR_LOGIC, name
        ix.profile_enable(False)
        _env(monkeypatch)
        ix.search_knn(np.stack([query, query]), kk)                # two queries: the bf16 nomination builds the shadow
        check_bf16_shadow(ix, rows)
        check_stats(ix, metric, rows, inv)


def test_inspect_refuses_what_does_not_exist(rxgpu, oracle, monkeypatch):
    rows = make_corpus(1, 100, 256)
    with rxgpu.VectorIndex(IP, 256, 100) as ix:
        ix.upload_rows(0, rows)
        for name in ("stats", "row_sq", "codes_i8", "side_i8", "rows_bf16") + PRUNED["i8"]:
            with pytest.raises(rxgpu.RxGpuError) as err:
                ix.inspect(name)
            assert err.value.code == rxgpu.RXGPU_ERR_LOGIC, name
        for name in ("", "pruned_", "pruned_nothing", "rows"):
            with pytest.raises(rxgpu.RxGpuError) as err:
                ix.inspect(name)
            assert err.value.code == rxgpu.RXGPU_ERR_PARAMS, name
        _env(monkeypatch, I8=1)
        ix.search_knn(rows[:1], 5)                                  # not profiling: the shadow exists, no call is recorded
        assert ix.inspect("codes_i8").shape == (100 * 256,) and ix.inspect("stats").shape == (5,)
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.inspect("pruned_values")
        assert err.value.code == rxgpu.RXGPU_ERR_LOGIC
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.inspect("row_sq")                                    # no |x|^2 per row off L2
        assert err.value.code == rxgpu.RXGPU_ERR_LOGIC
        need = C.c_uint64(0)
        small = np.zeros(8, np.uint8)
        rc = rxgpu.lib().rxgpu_index_inspect(ix._h, b"stats", small.ctypes.data, small.size, C.byref(need))
        assert rc == rxgpu.RXGPU_ERR_OVERFLOW and need.value == 20 and not small.any()
        ix.profile_enable(True)
        ix.search_knn(rows[:1], 5)                                  # recorded: kk values and the count
        top = ix.inspect("pruned_top")
        assert top.shape == (6,) and top[5] == 5 and np.all(np.diff(top[:5].view(np.float32)) >= 0)
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.inspect("pruned_nothing")
        assert err.value.code == rxgpu.RXGPU_ERR_PARAMS
        _env(monkeypatch, BF16=0)
        ix.search_knn(rows[:1], 5)                                  # the f32 scan answered: nothing to show
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.inspect("pruned_top")
        assert err.value.code == rxgpu.RXGPU_ERR_LOGIC
        ix.profile_enable(False)


# ---------------------------------------------------------------------------------------------------------------- E
DERIVED = ("codes_i8", "side_i8", "rows_bf16", "row_sq")


def _derived(ix, metric):
    return {name: ix.inspect(name).copy() for name in DERIVED if name != "row_sq" or metric == L2}


def _through_each_tier(ix, mp, query, kk):
    for env in (dict(BF16=1), dict(I8=1)):
        _env(mp, **env)
        ix.search_knn(query[None, :], kk)
    _env(mp)


@pytest.mark.parametrize("metric", METRICS)
def test_upkeep_keeps_every_derived_buffer_equal_to_a_fresh_build(rxgpu, oracle, lib, monkeypatch, metric):
    """upload_rows over rows / past the end / past the old capacity, move_row + truncate: after each step the shadows and |x|^2 of the index
    are byte-equal to those of a fresh index of the same rows, and its statistics words (maxima that never shrink) still bound the rows"""
    d, n, kk = 256, 3_001, 11   # (at most 3 264 rows in the end: the candidate list holds them all, whatever the 50 x row does to the L2 margin)
    rows, inv, query, _ = corpus(oracle, metric, 8000 + metric, n, d, **_mag(metric))
    norms = lambda r: oracle.l2_modules(r) if metric == COS else None

    def same_as_fresh(ix, rows, inv, step):
        assert ix.count == rows.shape[0]
        with rxgpu.VectorIndex(metric, d, rows.shape[0]) as fresh:
            fresh.upload_rows(0, rows, inv)
            _through_each_tier(fresh, monkeypatch, query, kk)
            want, fresh_stats = _derived(fresh, metric), fresh.inspect("stats").copy()
        got = _derived(ix, metric)
        for name in want:
            assert got[name].shape == want[name].shape and np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), (step, name)
        side = got["side_i8"].reshape(-1, 2)
        w = check_stats(ix, metric, rows, inv, np.ascontiguousarray(side[:, 1]))
        assert np.all(bits(w)[[0, 1, 3, 4]] >= fresh_stats[[0, 1, 3, 4]]), (step, w, fresh_stats)   # non-negative floats order like their bits

    rng = np.random.default_rng(8100 + metric)
    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)
        _through_each_tier(ix, monkeypatch, query, kk)                                  # 1. both shadows and the statistics exist
        same_as_fresh(ix, rows, inv, "built")
        new = make_corpus(8200 + metric, 40, d)
        new[17] *= np.float32(50 * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max() / np.sqrt((new[17].astype(np.float64) ** 2).sum()))
        rows = rows.copy()
        rows[1_500:1_540] = new                                                         # 2. 40 rows in the middle, one of 50 x the largest norm
        inv = norms(rows)
        ix.upload_rows(1_500, new, norms(new))
        same_as_fresh(ix, rows, inv, "upload_rows over existing rows")
        ix.move_row(n - 1, 5)                                                           # 3. swap-delete of row 5
        ix.truncate(n - 1)
        rows[5] = rows[n - 1]
        rows = rows[:n - 1]
        inv = norms(rows)
        same_as_fresh(ix, rows, inv, "move_row + truncate")
        more = make_corpus(8300 + metric, 5, d)
        more[2] *= np.float32(np.exp(rng.uniform(-14, -10)))
        ix.upload_rows(n - 1, more, norms(more))                                        # 4. past the end, within the capacity
        rows = np.concatenate([rows, more])
        inv = norms(rows)
        same_as_fresh(ix, rows, inv, "upload_rows past the end")
        ix.reserve(n + 300)                                                             # 5. past the old capacity
        late = make_corpus(8400 + metric, 200, d)
        ix.upload_rows(n + 4, late, norms(late))
        rows = np.concatenate([rows, late])
        inv = norms(rows)
        _through_each_tier(ix, monkeypatch, query, kk)                                  # (buffers that were too small are rebuilt by the next search)
        same_as_fresh(ix, rows, inv, "reserve + upload_rows past the old capacity")
        _, room, cand = run_i8_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, "after the mutations"))
        room16, cand16 = run_bf16_case(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, "after the mutations"))
    print(f"room after mutations metric={metric}: int8 {room:.3g} ({cand} candidates), bf16 {room16:.3g} ({cand16} candidates)")
