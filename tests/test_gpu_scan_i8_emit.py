"""-m gpu: the emitting form of the int8-pruned scan (knn_scan_i8<.., kEmit>), knn_filter_emitted behind it and knn_merge_final at the end
of every pruned chain (knn_scan_i8.hip, knn_filter.hip, knn_merge.hip).

While it scans, a wavefront emits the rows whose lower bound lo is within the margin of thr_d, the kk-th smallest upper bound it has seen
so far (+inf until it has seen kk): a superset of what the filter keeps, which is then held against the final T.  The shapes are those of
test_gpu_pruned_internals.py - one per code-row chunk count, n off the multiples of 16 and 64, the tails of one step, 40 003 rows at one
workgroup per CU where every wavefront loops - and its data (adversarial rows inside the benchmark's distribution).

  emission   a recording call (profiling on, one query) keeps lo of every row AND what was emitted.  lo and up come from the CPU model
             exactly as check_i8_scan forms them; the expected segment of wavefront w (sets w, w + nwaves, ... of 16 rows; before each set
             thr = the kk-th smallest up of its earlier sets or inf; rows with lo <= f32(thr + margin), ascending) must equal the device's,
             rows and lo bits.  Hence no row twice, the emitted set contains {lo <= T + margin}, and the candidates are exactly that set.
  timed form profiling off (no value per row is kept): rows, distance bits and counts of the f32 path for one and three queries, with the
             emission switched off (RXGPU_SCAN_I8_EMIT=0: the store-all sequence) as well.
  gate       more candidates than the list holds (5 000 identical rows), and a query with a NaN: knn_merge_final takes the exact scan's lists.
  stale      counts of a larger grid must not be read by a later, smaller call; idle wavefronts report 0."""
import numpy as np
import pytest

from . import i8_model
from .conftest import make_corpus
from .i8_model import PF, PI32, _p
from .test_gpu_pruned_internals import I8_SHAPES, LIST_CAP, _mag, bits, check_i8_query, check_i8_shadow, check_row_sq, corpus

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
METRICS = [L2, IP, COS]
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_WG_PER_CU", "RXGPU_SCAN_I8_EMIT")
SNAP = ("pruned_values", "pruned_margin", "pruned_q_sq", "pruned_qinfo", "pruned_qplanes", "pruned_top", "pruned_cand_rows", "pruned_emit_cnt",
        "pruned_emitted")


def _env(mp, **kw):
    for name in ENV:
        mp.delenv(name, raising=False)
    for k, v in kw.items():
        mp.setenv("RXGPU_SCAN_" + k, str(v))


@pytest.fixture(scope="module")
def lib():
    return i8_model.load()


def recorded(ix, mp, query, kk, wg=None):
    """one query through the forced int8 tier with profiling on -> (result, candidates, cap, what the chain left)"""
    env = dict(I8=1)
    if wg:
        env["I8_WG_PER_CU"] = wg
    _env(mp, **env)
    ix.profile_enable(True)
    res = ix.search_knn(query[None, :], kk)
    slots = {s: ix.profile_read(s)[0] for s in ("scan_i8", "filter_approx", "rescore", "fallback_scan")}
    cand, cap = ix.last_candidates()
    snap = {name: ix.inspect(name).copy() for name in SNAP}
    ix.profile_enable(False)
    _env(mp)
    assert slots == dict(scan_i8=1, filter_approx=1, rescore=1, fallback_scan=1), slots
    return res, cand, cap, snap


def model_bounds(lib, ix, snap, metric, rows, inv, query):
    """lo, up of every row from the CPU model over the device's shadow and query side, as check_i8_scan forms them; and the margin"""
    codes, s_r, e_r, w = check_i8_shadow(lib, ix, metric, rows, inv)
    aux = check_row_sq(ix, rows) if metric == L2 else inv
    t_dev, s_q, qn, q_sq, margin = check_i8_query(lib, snap, metric, query, w)
    m = rows.shape[0]
    S = codes.astype(np.int64) @ t_dev
    assert np.abs(S).max() < 2 ** 31
    full = lambda v: np.full(m, v, np.float32)
    aux = np.ascontiguousarray(aux, np.float32) if aux is not None else np.zeros(m, np.float32)
    out = np.zeros((m, 3), np.float32)
    lib.i8_cpu_bounds_many(metric, m, _p(full(s_q), PF), _p(np.ascontiguousarray(s_r), PF), _p(np.ascontiguousarray(S.astype(np.int32)), PI32),
                           _p(full(qn), PF), _p(np.ascontiguousarray(e_r), PF), _p(full(q_sq), PF), _p(aux, PF), _p(out, PF))
    return np.ascontiguousarray(out[:, 1]), np.ascontiguousarray(out[:, 2]), np.float32(margin)


def expected_segments(lo, up, margin, kk, nwaves):
    """the rule, wavefront by wavefront -> [(rows emitted, ascending)] per wavefront"""
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
                bound = np.float32(thr + margin)      # one f32 addition, as the kernel forms it
            mine.append(r[lo[r] <= bound])
            seen = np.sort(np.concatenate([seen, up[r]]))[:kk]
        segs.append(np.concatenate(mine) if mine else np.empty(0, np.int64))
    return segs


def check_emission(lib, ix, mp, metric, rows, inv, query, kk, what, wg=None):
    res, cand, cap, snap = recorded(ix, mp, query, kk, wg)
    n = rows.shape[0]
    kk = min(kk, n)
    assert cap == min(LIST_CAP, max(64, (n + 63) // 64 * 64)) and cand <= cap, (what, cand, cap)
    lo, up, margin = model_bounds(lib, ix, snap, metric, rows, inv, query)
    assert np.array_equal(bits(snap["pruned_values"]), bits(lo)), what   # the recording call kept lo of every row
    counts = snap["pruned_emit_cnt"]
    nwaves, nsets = counts.size, (n + 15) // 16
    assert nwaves % 4 == 0 and nwaves >= 4 and (nwaves - 4 < nsets or nwaves == 4), (what, nwaves, nsets)
    entries = snap["pruned_emitted"].reshape(n, 2)
    segs = expected_segments(lo, up, margin, kk, nwaves)
    rows_of = [sum(min(16 * s + 16, n) - 16 * s for s in range(w, nsets, nwaves)) for w in range(nwaves)]
    assert sum(rows_of) == n
    offset = np.concatenate([[0], np.cumsum(rows_of)])
    for w in range(nwaves):
        want = segs[w]
        assert counts[w] == want.size <= rows_of[w], (what, w, int(counts[w]), want.size)
        got = entries[offset[w]:offset[w] + want.size]
        assert np.array_equal(got[:, 1], want), (what, w, got[:8, 1], want[:8])
        assert np.array_equal(got[:, 0], bits(lo[want])), (what, w)
    for w in range(nsets, nwaves):
        assert counts[w] == 0, (what, "an idle wavefront reports", int(counts[w]))
    emitted = np.concatenate(segs)
    assert np.unique(emitted).size == emitted.size, (what, "a row was emitted twice")
    top = snap["pruned_top"]
    assert top[kk] == kk
    T = top[:kk].view(np.float32)[kk - 1]
    assert bits(T) == bits(np.sort(up)[kk - 1]), what
    passing = np.flatnonzero(lo <= np.float32(T) + margin)
    assert np.isin(passing, emitted).all(), (what, "a row inside the final window was not emitted")
    assert cand == passing.size and np.array_equal(np.sort(snap["pruned_cand_rows"]), passing), (what, cand, passing.size)
    return res, int(emitted.size), cand


def check_timed_form(ix, mp, queries, kk, what, wg=None):
    """profiling off: the forced tier, emitting and not, against the f32 path"""
    _env(mp, BF16=0)
    want = [ix.search_knn(queries[:nq], kk) for nq in (1, 3)]
    extra = dict(I8_WG_PER_CU=wg) if wg else {}
    for emit in ({}, dict(I8_EMIT=0)):
        _env(mp, I8=1, **extra, **emit)
        for nq, ref in zip((1, 3), want):
            got = ix.search_knn(queries[:nq], kk)
            assert np.array_equal(got[2], ref[2]), (what, emit, nq)
            assert np.array_equal(got[1], ref[1]), (what, emit, nq)
            assert np.array_equal(bits(got[0]), bits(ref[0])), (what, emit, nq)
    _env(mp)
    return want[0]


def _queries(oracle, metric, rows, query, seed):
    """the query that equals a stored row, and two of the corpus's distribution"""
    more = make_corpus(seed, 2, rows.shape[1])
    if metric == COS:
        more = np.stack([oracle.normalize_copy(v)[0] for v in more])
    return np.concatenate([query[None, :], more])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n,kk", I8_SHAPES)
def test_emission_is_the_rule_and_the_timed_form_is_exact(rxgpu, oracle, lib, monkeypatch, metric, d, n, kk):
    rows, inv, query, _ = corpus(oracle, metric, 1000 + d + n + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        res, emitted, cand = check_emission(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, d, n, kk))
        ref = check_timed_form(ix, monkeypatch, _queries(oracle, metric, rows, query, 50 + d), kk, (metric, d, n, kk))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(res, ref)), "the recording call's own answer"
    print(f"emit metric={metric} d={d} n={n} kk={kk}: {emitted} rows emitted, {cand} candidates")


@pytest.mark.parametrize("metric", METRICS)
def test_emission_with_every_wavefront_looping(rxgpu, oracle, lib, monkeypatch, metric):
    """40 003 rows at one workgroup per CU: every wavefront owns more than two sets, so its threshold is finite for most of them"""
    d, n, kk = 256, 40_003, 11
    rows, inv, query, _ = corpus(oracle, metric, 2000 + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _, emitted, cand = check_emission(lib, ix, monkeypatch, metric, rows, inv, query, kk, (metric, "looping"), wg=1)
        assert emitted < n, "no wavefront ever had a finite threshold"
        check_timed_form(ix, monkeypatch, _queries(oracle, metric, rows, query, 60), kk, (metric, "looping"), wg=1)
    print(f"emit looping metric={metric} d={d} n={n} kk={kk}: {emitted} rows emitted, {cand} candidates")


@pytest.mark.parametrize("metric", METRICS)
def test_the_gate_through_the_final_merge(rxgpu, oracle, monkeypatch, metric):
    """5 000 identical rows among 8 192: more rows inside the window than the list of 4 096 holds; and a query with a NaN component, which
    has no bound at all.  Both are answered by the exact scan behind the gate, whose lists knn_merge_final takes."""
    d, n, kk = 256, 8_192, 11
    rows = make_corpus(9000 + metric, n, d)
    same = np.sort(np.random.default_rng(9100 + metric).choice(n, 5_000, replace=False))
    rows[same] = rows[same[0]]
    inv = oracle.l2_modules(rows) if metric == COS else None
    tie = oracle.normalize_copy(rows[same[0]])[0] if metric == COS else rows[same[0]].copy()
    nan = tie.copy()
    nan[d // 3] = np.nan
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        for name, q in (("ties", tie), ("nan", nan)):
            _env(monkeypatch, BF16=0)
            ref = ix.search_knn(q[None, :], kk)
            for emit in ({}, dict(I8_EMIT=0)):
                _env(monkeypatch, I8=1, **emit)
                got = ix.search_knn(q[None, :], kk)
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, ref)), (metric, name, emit)
            _env(monkeypatch, I8=1)
            ix.profile_enable(True)
            got = ix.search_knn(q[None, :], kk)
            cand, cap = ix.last_candidates()
            launches = ix.profile_read("scan_i8")[0]
            ix.profile_enable(False)
            assert launches == 1 and cap == LIST_CAP and cand > cap, (metric, name, cand, cap)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, ref)), (metric, name, "recording")
        _env(monkeypatch)


def test_counts_of_an_earlier_larger_grid_are_not_read(rxgpu, oracle, lib, monkeypatch):
    """40 003 rows fill the counts of 1 024 wavefronts; after truncate(13) the grid is one workgroup: wavefront 0 owns the only set, the other
    three are idle and must say so"""
    metric, d, n, kk = L2, 256, 40_003, 11
    rows, inv, query, _ = corpus(oracle, metric, 2000 + metric, n, d, **_mag(metric))
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows, inv)
        _env(monkeypatch, I8=1, I8_WG_PER_CU=1)
        ix.search_knn(query[None, :], kk)
        ix.profile_enable(True)
        ix.search_knn(query[None, :], kk)
        big = ix.inspect("pruned_emit_cnt").copy()
        ix.profile_enable(False)
        assert big.size > 4 and np.count_nonzero(big) == big.size
        ix.truncate(13)
        _env(monkeypatch, BF16=0)
        ref = ix.search_knn(query[None, :], kk)
        _env(monkeypatch, I8=1, I8_WG_PER_CU=1)
        got = ix.search_knn(query[None, :], kk)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, ref))
        ix.profile_enable(True)
        got = ix.search_knn(query[None, :], kk)
        counts = ix.inspect("pruned_emit_cnt").copy()
        cand, cap = ix.last_candidates()
        ix.profile_enable(False)
        _env(monkeypatch)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, ref))
        assert counts.tolist() == [13, 0, 0, 0] and cand <= cap == 64, (counts, cand, cap)
