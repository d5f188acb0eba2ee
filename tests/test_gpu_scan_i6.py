"""-m gpu: the 6-bit front of the int8-pruned chain (knn_scan_i6.hip), forced with RXGPU_SCAN_I6=1, on the shapes of
test_gpu_pruned_internals.py (one per chunk count, n off the multiples of 16 and 64, the tails of one step and of one tile, 40 003 rows at
one workgroup per CU) plus 70 001 rows, the smallest size class at which the seed pass samples (every second set).

  shadow     codes_i6 / side_i6 equal the CPU model's bytes and bits (tests/i6_model.py), e_r held as the int8 test holds it, stats_i6 bound it
  upkeep     after upload_rows / move_row / truncate / reserve the shadow is byte-equal to a fresh index's
  scan       a recording call: lo_r of every row bit-equal to i8_bounds over the device's own query side and codes; T bit-equal to the kk-th
             smallest model up; T_seed bit-equal to the same over the sampled sets.  The segment of every wavefront equals the rule restated
             here, set by set: rows with lo <= f32(min(thr, T_seed) + margin), ascending - hence every such row is emitted, no other is, none twice
  filter     the candidates are exactly {lo <= T + margin} and contain the exact top-kk
  share      on the plain corpus at kk = 11 the model's own share of candidates stays below the bounds of SHARE_BOUNDS and the device counts
             what the model counts.  The model's shares with the margin in, one random query of the corpus's distribution per metric
             (L2 / ip / cosine): 0.114 / 0.128 / 0.126 at 4 099 x 750, 0.222 / 0.253 / 0.257 at 2 051 x 1024, 0.029 / 0.043 / 0.043 at
             40 003 x 768 - all inside the bounds the shapes were given (0.35, 0.35, 0.08), none widened
  result     rows, distance bits and counts equal the f32 path's for one and three queries, and the int8 front's
  gate       a NaN query and a list overflow (5 000 identical rows, RXGPU_SCAN_I6_CAP=4096 < n) take the gated exact scan: "fallback_scan" is
             filed, the result is the f32 path's.  RXGPU_ERR_NOMEM for the shadow -> the int8 front: there is no mechanism to make a shadow
             unavailable in a test (the int8 tests have none either); left to the code review
  stale      a later, smaller call does not read counts of a larger grid"""
import numpy as np
import pytest

from . import i6_model, i8_model
from .conftest import make_corpus
from .i6_model import BIAS
from .i8_model import PF, PI32, _p
from .test_gpu_pruned_internals import _mag, _ulps, bits, check_i8_query, check_row_sq, check_stats, corpus

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
METRICS = [L2, IP, COS]
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_WG_PER_CU", "RXGPU_SCAN_I8_EMIT",
       "RXGPU_SCAN_I6", "RXGPU_SCAN_I6_MIN_BYTES", "RXGPU_SCAN_I6_CAP")
SNAP = ("pruned_values", "pruned_margin", "pruned_q_sq", "pruned_qinfo", "pruned_qplanes", "pruned_top", "pruned_seed", "pruned_cand_rows",
        "pruned_emit_cnt", "pruned_emitted")
SLOTS = dict(scan_i6=1, seed_i6=1, scan_i8=0, filter_approx=1, rescore=1, fallback_scan=1)
LIST_CAP = 65536
SEED_SETS = 4096
SHAPES = [(130, 4_099, 11), (300, 4_099, 1), (300, 4_099, 11), (300, 4_099, 64), (750, 4_099, 11), (1024, 2_051, 11), (256, 13, 11), (256, 16, 11),
          (256, 17, 11), (256, 1, 11), (256, 3, 11), (256, 5, 11)]
SHARE_BOUNDS = {(750, 4_099): 0.35, (1024, 2_051): 0.35, (768, 40_003): 0.08}


def _env(mp, **kw):
    for name in ENV:
        mp.delenv(name, raising=False)
    for k, v in kw.items():
        mp.setenv("RXGPU_SCAN_" + k, str(v))


@pytest.fixture(scope="module")
def lib():
    return i8_model.load()


@pytest.fixture(scope="module")
def lib6():
    return i6_model.load()


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def recorded(ix, mp, query, kk, wg=None, **more):
    """one query through the forced front with profiling on -> (result, candidates, cap, profile slots, what the chain left)"""
    env = dict(I6=1, **more)
    if wg:
        env["I8_WG_PER_CU"] = wg
    _env(mp, **env)
    ix.profile_enable(True)
    res = ix.search_knn(query[None, :], kk)
    slots = {s: ix.profile_read(s)[0] for s in SLOTS}
    cand, cap = ix.last_candidates()
    snap = {name: ix.inspect(name).copy() for name in SNAP}
    ix.profile_enable(False)
    _env(mp)
    return res, cand, cap, slots, snap


def check_i6_shadow(lib6, ix, metric, rows, inv):
    """-> (u, s_r, e_r, the five statistics words the margin of this front takes, as floats)"""
    n, d = rows.shape
    ld6 = lib6.i6_cpu_ld(d)
    u = ix.inspect("codes_i6").reshape(n, ld6)
    side = ix.inspect("side_i6").reshape(n, 2)
    s_r, e_r = np.ascontiguousarray(side[:, 0]), np.ascontiguousarray(side[:, 1])
    mu, ms, me = i6_model.quantize_rows(lib6, rows)
    assert np.array_equal(bits(s_r), bits(ms)), np.flatnonzero(bits(s_r) != bits(ms))[:5]
    assert np.array_equal(u, mu), np.argwhere(u != mu)[:5]              # the zero pad up to ld6 included
    resid = np.sqrt(((rows.astype(np.float64) - s_r.astype(np.float64)[:, None] * (u[:, :d].astype(np.float64) - BIAS)) ** 2).sum(1))
    assert np.all(e_r.astype(np.float64) >= resid), np.flatnonzero(e_r < resid)[:5]   # the premise of the bound, from the DEVICE's codes
    assert _ulps(e_r, me).max() <= 1, np.flatnonzero(_ulps(e_r, me) > 1)[:5]          # a reordered fp64 sum moves i8_norm_up by an ulp at most
    w = check_stats(ix, metric, rows, inv).copy()
    s6 = ix.inspect("stats_i6")
    assert s6.shape == (3,) and s6[2] == 0, s6
    w6 = s6.view(np.float32)
    assert w6[0] >= (e_r * e_r).max(), (w6[0], (e_r * e_r).max())
    if metric == COS:
        ei = e_r * inv
        assert w6[1] >= (ei * ei).max(), (w6[1], (ei * ei).max())
    w[3], w[4] = w6[0], w6[1]
    return u, s_r, e_r, w


def bounds_of(lib, metric, u, s_r, e_r, aux, t, s_q, qn, q_sq):
    """lo, up of every row through i8_bounds, from 6-bit codes u and the query side"""
    m, d = u.shape[0], t.shape[0]
    S = (u.astype(np.int64) - BIAS) @ t                                 # t is zero in the pad, so the pad codes (u = 0) do not count
    assert np.abs(S).max() < 2 ** 31
    full = lambda v: np.full(m, v, np.float32)
    aux = np.ascontiguousarray(aux, np.float32) if aux is not None else np.zeros(m, np.float32)
    out = np.zeros((m, 3), np.float32)
    lib.i8_cpu_bounds_many(metric, m, _p(full(s_q), PF), _p(np.ascontiguousarray(s_r), PF), _p(np.ascontiguousarray(S.astype(np.int32)), PI32),
                           _p(full(qn), PF), _p(np.ascontiguousarray(e_r), PF), _p(full(q_sq), PF), _p(aux, PF), _p(out, PF))
    return np.ascontiguousarray(out[:, 1]), np.ascontiguousarray(out[:, 2])


def model_bounds(lib, lib6, ix, snap, metric, rows, inv, query):
    u, s_r, e_r, w = check_i6_shadow(lib6, ix, metric, rows, inv)
    aux = check_row_sq(ix, rows) if metric == L2 else inv
    t_dev, s_q, qn, q_sq, margin = check_i8_query(lib, snap, metric, query, w)     # the int8 prep, its margin over the 6-bit maxima
    lo, up = bounds_of(lib, metric, u, s_r, e_r, aux, t_dev, s_q, qn, q_sq)
    return lo, up, np.float32(margin)


def seed_rows(n):
    """the rows of the seed pass: the first set of 16 of every `step` sets"""
    nsets = (n + 15) // 16
    step = max(1, (nsets + SEED_SETS - 1) // SEED_SETS)
    return np.concatenate([np.arange(16 * s, min(16 * s + 16, n)) for s in range(0, nsets, step)]), step


def expected_segments(lo, up, margin, t_seed, kk, nwaves):
    """the rule, wavefront by wavefront and set by set -> the rows each wavefront emits, ascending"""
    n = lo.shape[0]
    nsets = (n + 15) // 16
    segs = []
    for w in range(nwaves):
        seen = np.empty(0, np.float32)   # the kk smallest up of the wavefront's earlier sets
        mine = []
        for s in range(w, nsets, nwaves):
            r = np.arange(16 * s, min(16 * s + 16, n))
            thr = np.float32(seen[kk - 1]) if seen.size >= kk else np.float32(np.inf)
            with np.errstate(over="ignore"):
                bound = np.float32(min(thr, t_seed) + margin)           # one f32 addition, as the kernel forms it
            mine.append(r[lo[r] <= bound])
            seen = np.sort(np.concatenate([seen, up[r]]))[:kk]
        segs.append(np.concatenate(mine) if mine else np.empty(0, np.int64))
    return segs


def check_front(lib, lib6, ix, mp, metric, rows, inv, query, kk, what, wg=None):
    """scan, emission and filter of one recording call -> (result, rows emitted, candidates, lo, T, margin)"""
    res, cand, cap, slots, snap = recorded(ix, mp, query, kk, wg)
    assert slots == SLOTS, (what, slots)
    n = rows.shape[0]
    kk = min(kk, n)
    assert cap == min(LIST_CAP, max(64, (n + 63) // 64 * 64)) and cand <= cap, (what, cand, cap)
    lo, up, margin = model_bounds(lib, lib6, ix, snap, metric, rows, inv, query)
    assert np.array_equal(bits(snap["pruned_values"]), bits(lo)), (what, np.flatnonzero(bits(snap["pruned_values"]) != bits(lo))[:5])
    top, seed = snap["pruned_top"], snap["pruned_seed"]
    assert top.shape == (kk + 1,) and top[kk] == kk, (what, top)
    T = top[:kk].view(np.float32)[kk - 1]
    assert bits(T) == bits(np.sort(up)[kk - 1]), (what, T, np.sort(up)[kk - 1])
    sampled, step = seed_rows(n)
    assert seed.shape == (kk + 1,) and seed[kk] == min(kk, sampled.size), (what, seed, sampled.size)
    t_seed = np.float32(np.inf)
    if sampled.size >= kk:
        t_seed = seed[:kk].view(np.float32)[kk - 1]
        assert bits(t_seed) == bits(np.sort(up[sampled])[kk - 1]) and t_seed >= T, (what, t_seed, T)
    counts = snap["pruned_emit_cnt"]
    nwaves, nsets = counts.size, (n + 15) // 16
    assert nwaves % 4 == 0 and nwaves >= 4 and (nwaves - 4 < nsets or nwaves == 4), (what, nwaves, nsets)
    entries = snap["pruned_emitted"].reshape(n, 2)
    segs = expected_segments(lo, up, margin, t_seed, kk, nwaves)
    rows_of = [sum(min(16 * s + 16, n) - 16 * s for s in range(w, nsets, nwaves)) for w in range(nwaves)]
    offset = np.concatenate([[0], np.cumsum(rows_of)])
    for w in range(nwaves):
        want = segs[w]
        assert counts[w] == want.size <= rows_of[w], (what, w, int(counts[w]), want.size)
        got = entries[offset[w]:offset[w] + want.size]
        assert np.array_equal(got[:, 1], want), (what, w, got[:8, 1], want[:8])
        assert np.array_equal(got[:, 0], bits(lo[want])), (what, w)
    emitted = np.concatenate(segs)
    assert np.unique(emitted).size == emitted.size, (what, "a row was emitted twice")
    passing = np.flatnonzero(lo <= np.float32(T) + margin)
    assert np.isin(passing, emitted).all(), (what, "a row inside the final window was not emitted")
    assert cand == passing.size and np.array_equal(np.sort(snap["pruned_cand_rows"]), passing), (what, cand, passing.size)
    listed = np.arange(n, dtype=np.uint32)
    dist = ix.distances(query, listed)
    assert ((lo.astype(np.float64) - dist.astype(np.float64)) / (np.float64(margin) / 2)).max() <= 1.0, (what, "lo_r > d_r + margin/2")
    order = np.lexsort((listed, dist))[:kk]
    assert np.isin(order, passing).all(), (what, "a row of the exact top-kk is no candidate")
    assert int(res[2][0]) == kk and np.array_equal(res[1][0, :kk], listed[order]) and np.array_equal(bits(res[0][0, :kk]), bits(dist[order])), what
    return res, int(emitted.size), cand, step


def check_result(ix, mp, queries, kk, what, wg=None):
    """profiling off: the forced front against the f32 path and the int8 front, one and three queries"""
    _env(mp, BF16=0)
    want = [ix.search_knn(queries[:nq], kk) for nq in (1, 3)]
    extra = dict(I8_WG_PER_CU=wg) if wg else {}
    for env in (dict(I6=1), dict(I8=1)):
        _env(mp, **env, **extra)
        for nq, ref in zip((1, 3), want):
            assert same(ix.search_knn(queries[:nq], kk), ref), (what, env, nq)
    _env(mp)
    return want[0]


def _queries(oracle, metric, rows, query, seed):
    more = make_corpus(seed, 2, rows.shape[1])
    if metric == COS:
        more = np.stack([oracle.normalize_copy(v)[0] for v in more])
    return np.concatenate([query[None, :], more])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n,kk", SHAPES)
def test_front_on_the_device(rxgpu, oracle, lib, lib6, monkeypatch, metric, d, n, kk):
    if n >= 13:
        rows, inv, query, _ = corpus(oracle, metric, 1000 + d + n + metric, n, d, **_mag(metric))
    else:   # a partial tile: too few rows for the adversarial ones of corpus()
        rows = make_corpus(1000 + d + n + metric, n, d)
        inv = oracle.l2_modules(rows) if metric == COS else None
        query = oracle.normalize_copy(rows[n // 2])[0] if metric == COS else rows[n // 2].copy()
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        res, emitted, cand, _ = check_front(lib, lib6, ix, monkeypatch, metric, rows, inv, query, kk, (metric, d, n, kk))
        ref = check_result(ix, monkeypatch, _queries(oracle, metric, rows, query, 50 + d), kk, (metric, d, n, kk))
        assert same(res, ref), "the recording call's own answer"
    print(f"i6 metric={metric} d={d} n={n} kk={kk}: {emitted} rows emitted, {cand} candidates")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,wg", [(40_003, 1), (70_001, None)])
def test_front_with_wavefronts_looping_and_a_sampled_seed(rxgpu, oracle, lib, lib6, monkeypatch, metric, n, wg):
    """40 003 rows at one workgroup per CU: every wavefront goes round its double-buffered loop more than twice.  70 001 rows: 4 376 sets, the seed
    pass takes every second one"""
    d, kk = 256, 11
    rows, inv, query, _ = corpus(oracle, metric, 2000 + metric + n, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, emitted, cand, step = check_front(lib, lib6, ix, monkeypatch, metric, rows, inv, query, kk, (metric, n), wg=wg)
        assert step == (2 if n == 70_001 else 1) and emitted < n
        check_result(ix, monkeypatch, _queries(oracle, metric, rows, query, 60), kk, (metric, n), wg=wg)
    print(f"i6 looping metric={metric} d={d} n={n} kk={kk}: {emitted} rows emitted, {cand} candidates, seed step {step}")


def model_share(lib, lib6, metric, rows, inv, query, kk):
    """candidates / rows of the CPU model alone, the margin in"""
    d = rows.shape[1]
    u, s_r, e_r = i6_model.quantize_rows(lib6, rows)
    _, _, t, info = i8_model.quantize_queries(lib, query[None, :])
    xx = (rows.astype(np.float64) ** 2).sum(1)
    i64 = inv.astype(np.float64) if inv is not None else np.zeros(rows.shape[0])
    e64 = e_r.astype(np.float64)
    stats = [np.float32(xx.max()), np.float32((xx * i64 ** 2).max()), np.float32((e64 ** 2).max()), np.float32(((e64 * i64) ** 2).max())]
    m = np.zeros(2, np.float32)
    lib.i8_cpu_margin(metric, info[0, 3], d, info[0, 1], info[0, 2], *stats, _p(m, PF))
    aux = (rows * rows).sum(1, dtype=np.float32) if metric == L2 else inv
    lo, up = bounds_of(lib, metric, u, s_r, e_r, aux, t[0].astype(np.int64), info[0, 0], info[0, 1], info[0, 3])
    T = np.sort(up)[kk - 1]
    return float((lo <= np.float32(T) + m[1]).mean())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", list(SHARE_BOUNDS))
def test_the_window_prunes_on_the_plain_corpus(rxgpu, oracle, lib, lib6, monkeypatch, metric, d, n):
    """non-vacuity: the plain corpus, one query of its distribution, kk = 11 - the model's own share of candidates is below the bound of the
    shape, and the device counts what the device-side model of check_front counts"""
    kk = 11
    rows = make_corpus(3000 + d, n, d)
    inv = oracle.l2_modules(rows) if metric == COS else None
    query = make_corpus(3100 + d, 1, d)[0]
    if metric == COS:
        query = oracle.normalize_copy(query)[0]
    share = model_share(lib, lib6, metric, rows, inv, query, kk)
    print(f"i6 share metric={metric} d={d} n={n}: model {share:.3f} (bound {SHARE_BOUNDS[d, n]})")
    assert share < SHARE_BOUNDS[d, n], share
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, emitted, cand, _ = check_front(lib, lib6, ix, monkeypatch, metric, rows, inv, query, kk, ("share", metric, d, n))   # (asserts cand == the model's count)
    assert cand / n < SHARE_BOUNDS[d, n], (cand, n)
    print(f"i6 share metric={metric} d={d} n={n}: device {cand / n:.3f}, {emitted} rows emitted")


@pytest.mark.parametrize("metric", METRICS)
def test_the_gate(rxgpu, oracle, monkeypatch, metric):
    """a query with a NaN has no bound; 5 000 identical rows among 8 192 with the list lowered to 4 096 overflow it: the gated exact scan answers"""
    d, n, kk = 256, 8_192, 11
    rows = make_corpus(9000 + metric, n, d)
    dup = np.sort(np.random.default_rng(9100 + metric).choice(n, 5_000, replace=False))
    rows[dup] = rows[dup[0]]
    inv = oracle.l2_modules(rows) if metric == COS else None
    tie = oracle.normalize_copy(rows[dup[0]])[0] if metric == COS else rows[dup[0]].copy()
    nan = tie.copy()
    nan[d // 3] = np.nan
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for name, q, cap_env in (("ties", tie, dict(I6_CAP=4096)), ("nan", nan, {})):
            _env(monkeypatch, BF16=0)
            ref = ix.search_knn(q[None, :], kk)
            _env(monkeypatch, I6=1, **cap_env)
            assert same(ix.search_knn(q[None, :], kk), ref), (metric, name)
            ix.profile_enable(True)
            got = ix.search_knn(q[None, :], kk)
            cand, cap = ix.last_candidates()
            slots = {s: ix.profile_read(s)[0] for s in SLOTS}
            ix.profile_enable(False)
            assert slots == SLOTS and cap == (4096 if cap_env else n) and cand > cap, (metric, name, slots, cand, cap)
            assert same(got, ref), (metric, name, "recording")
        _env(monkeypatch)


def test_counts_of_an_earlier_larger_grid_are_not_read(rxgpu, oracle, monkeypatch):
    """40 003 rows fill the counts of 1 024 wavefronts; after truncate(13) the grid is one workgroup: wavefront 0 owns the only set"""
    metric, d, n, kk = L2, 256, 40_003, 11
    rows, inv, query, _ = corpus(oracle, metric, 2000 + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, _, _, _, snap = recorded(ix, monkeypatch, query, kk, wg=1)
        big = snap["pruned_emit_cnt"]
        assert big.size == 1024 and big.sum() > 0
        ix.truncate(13)
        _env(monkeypatch, BF16=0)
        ref = ix.search_knn(query[None, :], kk)
        got, cand, cap, slots, snap = recorded(ix, monkeypatch, query, kk, wg=1)
        assert same(got, ref) and slots == SLOTS
        # (the seed pass has seen all 13 rows, T_seed = T: the only wavefront with a set emits exactly the candidates; the idle ones say 0)
        counts = snap["pruned_emit_cnt"].tolist()
        assert counts[1:] == [0, 0, 0] and 11 <= counts[0] == cand <= 13 and cap == 64, (counts, cand, cap)
        assert snap["pruned_seed"][-1] == 11 and snap["pruned_top"][-1] == 11


@pytest.mark.parametrize("metric", METRICS)
def test_upkeep_keeps_the_shadow_equal_to_a_fresh_build(rxgpu, oracle, lib6, monkeypatch, metric):
    """the sequence of test_gpu_pruned_internals.py (table row E of DESIGN section 4): upload_rows over rows / past the end / past the old
    capacity, move_row + truncate; after each step codes_i6 and side_i6 are byte-equal to those of a fresh index of the same rows"""
    d, n, kk = 256, 3_001, 11
    rows, inv, query, _ = corpus(oracle, metric, 8000 + metric, n, d, **_mag(metric))
    norms = lambda r: oracle.l2_modules(r) if metric == COS else None

    def through(ix):
        _env(monkeypatch, I6=1)
        ix.search_knn(query[None, :], kk)
        _env(monkeypatch)

    def same_as_fresh(ix, rows, inv, step):
        assert ix.count == rows.shape[0]
        with rxgpu.VectorIndex(metric, d, rows.shape[0]) as fresh:
            fresh.upload_rows(0, rows, inv)
            through(fresh)
            want = {name: fresh.inspect(name).copy() for name in ("codes_i6", "side_i6")}
            fresh_stats = fresh.inspect("stats_i6").copy()
        for name in want:
            got = ix.inspect(name)
            assert got.shape == want[name].shape and np.array_equal(got.view(np.uint8), want[name].view(np.uint8)), (step, name)
        assert np.all(ix.inspect("stats_i6")[:2] >= fresh_stats[:2]), step   # maxima that never shrink; non-negative floats order like their bits
        check_i6_shadow(lib6, ix, metric, rows, inv)

    rng = np.random.default_rng(8100 + metric)
    with rxgpu.VectorIndex(metric, d, n + 8) as ix:
        ix.upload_rows(0, rows, inv)
        through(ix)
        same_as_fresh(ix, rows, inv, "built")
        new = make_corpus(8200 + metric, 40, d)
        new[17] *= np.float32(50 * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max() / np.sqrt((new[17].astype(np.float64) ** 2).sum()))
        rows = rows.copy()
        rows[1_500:1_540] = new
        inv = norms(rows)
        ix.upload_rows(1_500, new, norms(new))
        same_as_fresh(ix, rows, inv, "upload_rows over existing rows")
        ix.move_row(n - 1, 5)
        ix.truncate(n - 1)
        rows[5] = rows[n - 1]
        rows = rows[:n - 1]
        inv = norms(rows)
        same_as_fresh(ix, rows, inv, "move_row + truncate")
        more = make_corpus(8300 + metric, 5, d)
        more[2] *= np.float32(np.exp(rng.uniform(-14, -10)))
        ix.upload_rows(n - 1, more, norms(more))
        rows = np.concatenate([rows, more])
        inv = norms(rows)
        same_as_fresh(ix, rows, inv, "upload_rows past the end")
        ix.reserve(n + 300)
        late = make_corpus(8400 + metric, 200, d)
        ix.upload_rows(n + 4, late, norms(late))
        rows = np.concatenate([rows, late])
        inv = norms(rows)
        through(ix)                                                   # (a shadow that was too small is rebuilt by the next search)
        same_as_fresh(ix, rows, inv, "reserve + upload_rows past the old capacity")
        _env(monkeypatch, BF16=0)
        ref = ix.search_knn(query[None, :], kk)
        _env(monkeypatch, I6=1)
        assert same(ix.search_knn(query[None, :], kk), ref)
        _env(monkeypatch)
