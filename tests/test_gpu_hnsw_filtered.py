"""-m gpu: HNSW search under an allowed-rows bitmap — rxgpu_hnsw_search_knn_filtered / _sq8_filtered (hnsw_filtered.hip) and
GpuHnswMap::SearchKnnFiltered.  The expected result is always the restated engine (oracle_hnsw_search_knn / _sq8) on a copy of the graph in
which every node outside the filter also carries the delete mark and num_deleted counts both kinds: labels and distance BITS, as sorted
pairs.  Where the reference engine itself is loadable it is asked as well (RefHnsw.import_graph of the same copy)."""
import threading

import numpy as np
import pytest

from .conftest import make_corpus
from .test_golden import golden_hnsw_graph
from .test_gpu_hnsw import as_sorted_pairs, bits

pytestmark = pytest.mark.gpu
TEAM_MAX = 256   # searches per launch up to which floats at 128 / 768 take the four-wavefront team (HnswLaunchPlan::team_max)


def hidden_copy(g, allowed):
    """the graph the reference would search: MarkDelete applied to every node outside the filter"""
    h = dict(g)
    h["deleted"] = np.ascontiguousarray(np.asarray(g["deleted"], np.uint8) | (~allowed).astype(np.uint8))
    h["num_deleted"] = int(np.count_nonzero(h["deleted"]))
    return h


def words_of(allowed, garbage=False):
    n = allowed.shape[0]
    w = np.zeros((n + 31) // 32 + (3 if garbage else 0), np.uint32)
    idx = np.nonzero(allowed)[0]
    np.bitwise_or.at(w, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    if garbage:   # bits at and above n are ignored
        if n & 31:
            w[n >> 5] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
        w[(n + 31) // 32:] = 0xFFFFFFFF
    return w


def check_rows(got_dist, got_row, got_cnt, labels, want, tag):
    for qi, (wd, wl) in enumerate(want):
        c = int(got_cnt[qi])
        gd, gl = as_sorted_pairs(got_dist[qi, :c], labels[got_row[qi, :c]])
        wd, wl = as_sorted_pairs(wd, wl)
        assert np.array_equal(gl, wl), (tag, qi)
        assert np.array_equal(bits(gd), bits(wd)), (tag, qi)


# ------------------------------------------------------------------------------------------------ 1. the golden graph
GOLDEN_FILTERS = ["all", "share0.9", "share0.5", "share0.1", "eleven", "last", "none", "not_entry", "word_edges"]
GOLDEN_KEF = [(10, 128), (10, 10), (1, 0), (40, 64), (10, 160), (10, 224), (10, 300)]


def golden_filter(name, g):
    n = g["n"]
    rng = np.random.default_rng(len(name) * 1000 + n)
    a = np.zeros(n, bool)
    if name == "all":
        a[:] = True
    elif name.startswith("share"):
        a = rng.random(n) < float(name[5:])
    elif name == "eleven":
        a[rng.choice(n, 11, replace=False)] = True
    elif name == "last":
        a[n - 1] = True
    elif name == "not_entry":
        a[:] = True
        a[g["entry"]] = False
    elif name == "word_edges":
        a[[31, 32, 63, 64, n - 1]] = True
    return a


@pytest.fixture(scope="module")
def golden_queries(oracle):
    return np.stack([oracle.normalize_copy(q)[0] for q in make_corpus(4711, TEAM_MAX + 1, 48)])


@pytest.mark.parametrize("name", GOLDEN_FILTERS)
@pytest.mark.parametrize("phase", [0, 1])
def test_golden_graph_under_filters(rxgpu, oracle, golden_queries, phase, name):
    """1500 x 48 cosine, the generic distance batch; phase 1 has delete marks of its own, so filter and marks combine.  nq = 1 and 5 take
    the single-wavefront kernels (no fixed batch at 48 components), TEAM_MAX + 1 a launch past the team's limit; the selective filters mark
    every node, so the hash set of the first pass overflows and the bitset re-run tier runs under the filter."""
    from oracle.pyoracle import oracle_hnsw_search_knn
    _, g = golden_hnsw_graph(oracle, phase)
    inv = oracle.l2_modules(g["vectors"])
    allowed = golden_filter(name, g)
    gh = hidden_copy(g, allowed)
    live = int(np.count_nonzero(gh["deleted"] == 0))
    words, dirty = words_of(allowed), words_of(allowed, garbage=True)
    with rxgpu.VectorIndex(g["metric"], g["dim"], g["n"]) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        ix.hnsw_attach_graph(g)
        for k, ef in GOLDEN_KEF:
            want = [oracle_hnsw_search_knn(oracle, gh, q, k, ef, inv) for q in golden_queries]
            if name == "none":
                assert all(len(wl) == 0 for _, wl in want)
            if live and ef >= k:
                assert all(len(wl) == min(k, live) for _, wl in want)   # a hidden entry point, a near-empty filter: still everything there is
            for nq, w in ((1, words), (5, dirty), (TEAM_MAX + 1, words)):
                dist, row, cnt, n_allowed = ix.hnsw_search_knn_filtered(golden_queries[:nq], k, ef, w)
                assert n_allowed == int(np.count_nonzero(allowed))
                check_rows(dist, row, cnt, g["labels"], want[:nq], (phase, name, k, ef, nq))


def test_golden_graph_against_the_reference_engine(rxgpu, ref, oracle, golden_queries):
    from oracle.pyoracle import RefHnsw
    _, g = golden_hnsw_graph(oracle, 1)
    inv = oracle.l2_modules(g["vectors"])
    with rxgpu.VectorIndex(g["metric"], g["dim"], g["n"]) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        ix.hnsw_attach_graph(g)
        for name in ("share0.5", "share0.1", "eleven", "not_entry"):
            allowed = golden_filter(name, g)
            gh = hidden_copy(g, allowed)
            r = RefHnsw(ref, g["metric"], g["dim"], g["n"], M=g["M"])
            r.import_graph(gh)
            for k, ef in ((10, 128), (10, 10), (10, 300)):
                want = [r.search_knn(q, k, ef) for q in golden_queries[:20]]
                dist, row, cnt, _ = ix.hnsw_search_knn_filtered(golden_queries[:20], k, ef, words_of(allowed))
                check_rows(dist, row, cnt, g["labels"], want, (name, k, ef))
            r.close()


# ------------------------------------------------------------------------------------------------ 2. graphs the product builds
N_BUILT = 3000   # not a multiple of 32
_built = {}


def built_graph(oracle, metric, d):
    """(graph with vectors, inv norms, labels): 3000 rows, M = 16, built once per (metric, dim) by the host builder"""
    if (metric, d) not in _built:
        from reindexer_amd import hostapi
        rows = make_corpus(5000 + d, N_BUILT, d)
        labels = (np.arange(N_BUILT, dtype=np.uint64) << np.uint64(32)) | np.uint64(9)
        m = hostapi.GpuHnswMap(metric, d, N_BUILT, M=16, ef_construction=100)
        m.add(rows, labels)
        g = m.export_graph()
        m.close()
        g["vectors"] = rows
        _built[(metric, d)] = (g, oracle.l2_modules(rows) if metric == 2 else None, labels)
    return _built[(metric, d)]


def built_queries(oracle, metric, d, nq):
    q = make_corpus(6000 + d, nq, d)
    return np.stack([oracle.normalize_copy(x)[0] for x in q]) if metric == 2 else q


def share_filter(share, n=N_BUILT):
    return np.random.default_rng(int(share * 100)).random(n) < share


@pytest.mark.parametrize("d", [128, 768, 384])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_built_graphs_floats(rxgpu, oracle, metric, d):
    """128 and 768 floats: the fixed batches, the team at nq = 1; 384: the generic batch.  ef = 64 on the list of two entries a lane, 200 of four."""
    from oracle.pyoracle import oracle_hnsw_search_knn
    g, inv, labels = built_graph(oracle, metric, d)
    queries = built_queries(oracle, metric, d, 6)
    with rxgpu.VectorIndex(metric, d, N_BUILT) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        ix.hnsw_attach_graph(g)
        for share in (0.5, 0.1):
            allowed = share_filter(share)
            gh = hidden_copy(g, allowed)
            for ef in (64, 200):
                want = [oracle_hnsw_search_knn(oracle, gh, q, 10, ef, inv) for q in queries]
                for nq in (1, 6):
                    dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries[:nq], 10, ef, words_of(allowed))
                    check_rows(dist, row, cnt, labels, want[:nq], (metric, d, share, ef, nq))


@pytest.fixture(scope="module")
def sq8(oracle):
    from oracle.pyoracle import Sq8Oracle
    return Sq8Oracle(oracle)


@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_built_graphs_codes(rxgpu, oracle, sq8, metric, d):
    from oracle.pyoracle import oracle_hnsw_search_knn_sq8
    from reindexer_amd.hostapi import sq8_quantize, sq8_quantize_many
    g, inv, labels = built_graph(oracle, metric, d)
    rows = g["vectors"]
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))
    p = sq8.params(min_q, max_q, d)
    codes, corr = sq8_quantize_many(metric, min_q, max_q, rows)
    c0, o0 = sq8.quantize(metric, p, rows[17])
    assert np.array_equal(c0, codes[17]) and bits(o0) == bits(corr[17])   # the table is the reference quantiser's
    sq = dict(min_q=p["min_q"], alpha=p["alpha"], alpha_2=p["alpha_2"], delta=p["delta"], codes=codes, corr=corr)
    raw = make_corpus(6100 + d, 6, d)
    queries, norms, qc, qo, qn = [], [], [], [], []
    for x in raw:
        norm = None
        coef = np.float32(1.0)
        if metric == 2:
            x, k_ = oracle.normalize_copy(x)
            norm = float(np.float32(1.0) / np.float32(k_))
            coef = np.float32(1.0) / np.float32(norm)
        c, o, _ = sq8_quantize(metric, min_q, max_q, x, float(np.float32(1.0) / coef))   # prepareData: norm = 1.f / normCoef
        queries.append(x), norms.append(norm), qc.append(c), qo.append(o), qn.append(coef)
    with rxgpu.VectorIndex(metric, d, N_BUILT) as ix:
        ix.upload_rows(0, rows, inv)
        ix.hnsw_attach_graph(g)
        ix.hnsw_attach_sq8(codes, corr, float(p["alpha_2"]))
        for share in (0.5, 0.1):
            allowed = share_filter(share)
            gh = hidden_copy(g, allowed)
            for ef in (64, 200):
                want = [oracle_hnsw_search_knn_sq8(oracle, gh, sq, q, 10, ef, inv, nm) for q, nm in zip(queries, norms)]
                for nq in (1, 6):
                    dist, row, cnt, _ = ix.hnsw_search_knn_sq8_filtered(np.stack(qc[:nq]), np.array(qo[:nq], np.float32), np.array(qn[:nq], np.float32), 10, ef,
                                                                        words_of(allowed))
                    check_rows(dist, row, cnt, labels, want[:nq], (metric, d, share, ef, nq))


# ------------------------------------------------------------------------------------------------ 3. forced tiers
@pytest.mark.parametrize("hook", [None, ("RXGPU_HNSW_SORTED", "0"), ("RXGPU_HNSW_LDS_CAND_CAP", "4")])
def test_forced_tiers_give_the_same_answers(rxgpu, oracle, monkeypatch, hook):
    """768 floats, cosine, half of the nodes allowed: on the lists (default), on the heaps alone, and with the LDS candidate area shrunk so
    that every search goes through the global-candidate re-runs — under the filter in every tier."""
    from oracle.pyoracle import oracle_hnsw_search_knn
    g, inv, labels = built_graph(oracle, 2, 768)
    queries = built_queries(oracle, 2, 768, 6)
    allowed = share_filter(0.5)
    gh = hidden_copy(g, allowed)
    if hook:
        monkeypatch.setenv(*hook)
    with rxgpu.VectorIndex(2, 768, N_BUILT) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        ix.hnsw_attach_graph(g)
        for ef in (64, 200):
            want = [oracle_hnsw_search_knn(oracle, gh, q, 10, ef, inv) for q in queries]
            for nq in (1, 6):
                dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries[:nq], 10, ef, words_of(allowed))
                check_rows(dist, row, cnt, labels, want[:nq], (hook, ef, nq))


def test_the_list_form_answers_most_searches(rxgpu, oracle):
    """share 0.9, ef = 64 on the default path: fewer searches handed to the heaps than searches — otherwise the list form was never tested"""
    from oracle.pyoracle import oracle_hnsw_search_knn
    g, inv, labels = built_graph(oracle, 2, 768)
    queries = built_queries(oracle, 2, 768, 40)
    allowed = share_filter(0.9)
    gh = hidden_copy(g, allowed)
    with rxgpu.VectorIndex(2, 768, N_BUILT) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        ix.hnsw_attach_graph(g)
        ix.hnsw_read_tie_reruns()
        want = [oracle_hnsw_search_knn(oracle, gh, q, 10, 64, inv) for q in queries]
        dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries, 10, 64, words_of(allowed))
        check_rows(dist, row, cnt, labels, want, "batch")
        for qi in range(len(queries)):
            dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries[qi:qi + 1], 10, 64, words_of(allowed))
            check_rows(dist, row, cnt, labels, want[qi:qi + 1], ("single", qi))
        searches = 2 * len(queries)
        reruns = ix.hnsw_read_tie_reruns()   # launches of their own and restarts inside the list kernel
        print("searches handed to the heaps / searches:", reruns, searches)
        assert reruns < searches


# ------------------------------------------------------------------------------------------------ 4. errors and delegation
def test_errors_and_delegation(rxgpu, oracle):
    from reindexer_amd import capi
    _, g = golden_hnsw_graph(oracle, 0)
    inv = oracle.l2_modules(g["vectors"])
    n = g["n"]
    q = np.stack([oracle.normalize_copy(x)[0] for x in make_corpus(31, 3, 48)])
    every = words_of(np.ones(n, bool))
    L = capi.lib()
    out_d, out_r, out_c = np.full((3, 10), -1.0, np.float32), np.full((3, 10), 77, np.uint32), np.full(3, 77, np.uint32)

    def raw(ix, nq=3, k=10, ef=64, words=every, n_words=None, handle=None):
        return L.rxgpu_hnsw_search_knn_filtered(handle if handle is not None else ix._h, q.ctypes.data, nq, k, ef, None if words is None else words.ctypes.data,
                                                len(every) if n_words is None else n_words, out_d.ctypes.data, out_r.ctypes.data, out_c.ctypes.data, None)

    with rxgpu.VectorIndex(g["metric"], g["dim"], n) as ix:
        ix.upload_rows(0, g["vectors"], inv)
        assert raw(ix) == capi.RXGPU_ERR_LOGIC                      # no graph attached
        ix.hnsw_attach_graph(g)
        assert raw(ix, words=None) == capi.RXGPU_ERR_PARAMS
        assert raw(ix, n_words=len(every) - 1) == capi.RXGPU_ERR_PARAMS
        assert raw(ix, ef=4097) == capi.RXGPU_ERR_PARAMS
        qc = np.zeros((3, 48), np.uint8)
        one = np.ones(3, np.float32)
        assert L.rxgpu_hnsw_search_knn_sq8_filtered(ix._h, qc.ctypes.data, one.ctypes.data, one.ctypes.data, 3, 10, 64, every.ctypes.data, len(every),
                                                    out_d.ctypes.data, out_r.ctypes.data, out_c.ctypes.data, None) == capi.RXGPU_ERR_LOGIC   # no codes attached
        assert raw(ix, nq=0) == capi.RXGPU_OK and raw(ix, k=0) == capi.RXGPU_OK
        assert np.all(out_d == -1.0) and np.all(out_r == 77) and np.all(out_c == 77)   # nothing written
        # every bit set, no delete marks: the unfiltered call's pairs
        wd, wr, wc = ix.hnsw_search_knn(q, 10, 64)
        gd, gr, gc, n_allowed = ix.hnsw_search_knn_filtered(q, 10, 64, every)
        assert n_allowed == n and np.array_equal(gc, wc)
        for qi in range(3):
            a, b = as_sorted_pairs(gd[qi, :gc[qi]], gr[qi, :gc[qi]]), as_sorted_pairs(wd[qi, :wc[qi]], wr[qi, :wc[qi]])
            assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    sharded = rxgpu.ShardedVectorIndex(g["metric"], g["dim"], n, [0, 0])
    try:
        assert raw(None, handle=sharded._h) == capi.RXGPU_ERR_LOGIC
    finally:
        sharded.close()


# ------------------------------------------------------------------------------------------------ 5. the Map
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_map_search_knn_filtered(rxgpu, oracle, metric):
    from oracle.pyoracle import oracle_hnsw_search_knn
    from reindexer_amd import hostapi
    n, d, k = N_BUILT, 128, 10
    rows = make_corpus(5000 + d, n, d)
    labels = (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(9)
    m = hostapi.GpuHnswMap(metric, d, n, M=16, ef_construction=100)
    m.add(rows, labels)
    for lab in labels[np.random.default_rng(8).choice(n, 100, replace=False)]:
        m.mark_delete(int(lab))
    g = m.export_graph()
    g["vectors"] = rows
    inv = oracle.l2_modules(rows) if metric == 2 else None
    queries = built_queries(oracle, metric, d, 8)
    rng = np.random.default_rng(metric)
    m.filtered_stats()
    for qi, q in enumerate(queries):
        # more allowed live nodes than ef: the graph search, unknown and duplicate labels tolerated
        allowed = rng.random(n) < (0.5 if qi & 1 else 0.1)
        ids = np.nonzero(allowed)[0]
        given = np.concatenate([labels[ids], labels[ids[:7]], np.array([12345, (n + 5) << 32], np.uint64)])
        rng.shuffle(given)
        for ef in (64, 0):
            wd, wl = oracle_hnsw_search_knn(oracle, hidden_copy(g, allowed), q, k, ef, inv)
            gd, gl = m.search_knn_filtered(q, k, ef, given)
            assert np.array_equal(as_sorted_pairs(gd, gl)[1], as_sorted_pairs(wd, wl)[1]), (metric, qi, ef)
            assert np.array_equal(bits(as_sorted_pairs(gd, gl)[0]), bits(as_sorted_pairs(wd, wl)[0]))
        assert m.filtered_stats() == (2, 0)
        # at most ef allowed live nodes: the exact k nearest of them (ties by internal row), no graph walk
        few = np.zeros(n, bool)
        few[rng.choice(n, 64, replace=False)] = True
        live = np.nonzero(few & (g["deleted"] == 0))[0]
        assert k < len(live) <= 64
        wd, wl = oracle.bf_search_knn(metric, rows[live], labels[live], None if inv is None else inv[live], q, k)
        gd, gl = m.search_knn_filtered(q, k, 64, labels[few])
        assert np.array_equal(as_sorted_pairs(gd, gl)[1], as_sorted_pairs(wd, wl)[1]), (metric, qi)
        assert np.array_equal(bits(as_sorted_pairs(gd, gl)[0]), bits(as_sorted_pairs(wd, wl)[0]))
        assert m.filtered_stats() == (0, 1)
    assert m.search_knn_filtered(queries[0], k, 64, np.array([12345], np.uint64))[1].size == 0   # nothing the Map holds
    assert m.search_knn_filtered(queries[0], k, 64, np.zeros(0, np.uint64))[1].size == 0
    m.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_quantised_map_never_takes_the_exact_scan(rxgpu, oracle, sq8, metric):
    from oracle.pyoracle import oracle_hnsw_search_knn_sq8
    from reindexer_amd import hostapi
    from reindexer_amd.hostapi import sq8_quantize_many
    n, d, k = N_BUILT, 128, 10
    rows = make_corpus(5000 + d, n, d)
    labels = (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(9)
    m = hostapi.GpuHnswMap(metric, d, n, M=16, ef_construction=100)
    m.add(rows, labels)
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))
    m.quantize(min_q, max_q)
    g = m.export_graph()
    p = sq8.params(min_q, max_q, d)
    codes, corr = sq8_quantize_many(metric, min_q, max_q, rows)
    sq = dict(min_q=p["min_q"], alpha=p["alpha"], alpha_2=p["alpha_2"], delta=p["delta"], codes=codes, corr=corr)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    rng = np.random.default_rng(50 + metric)
    m.filtered_stats()
    for qi in range(6):
        q = make_corpus(6200 + qi, 1, d)[0]
        norm = None
        if metric == 2:
            q, k_ = oracle.normalize_copy(q)
            norm = float(np.float32(1.0) / np.float32(k_))
        allowed = np.zeros(n, bool)
        allowed[rng.choice(n, 40 if qi & 1 else 1500, replace=False)] = True   # 40 <= ef: a float Map would scan
        wd, wl = oracle_hnsw_search_knn_sq8(oracle, hidden_copy(g, allowed), sq, q, k, 64, inv, norm)
        gd, gl = m.search_knn_filtered(q, k, 64, labels[allowed], norm)
        assert np.array_equal(as_sorted_pairs(gd, gl)[1], as_sorted_pairs(wd, wl)[1]), (metric, qi)
        assert np.array_equal(bits(as_sorted_pairs(gd, gl)[0]), bits(as_sorted_pairs(wd, wl)[0]))
    assert m.filtered_stats() == (6, 0)
    m.close()


# ------------------------------------------------------------------------------------------------ 6. the Map over a device list
def test_map_over_a_device_list(rxgpu, oracle):
    from oracle.pyoracle import oracle_hnsw_search_knn
    from reindexer_amd import hostapi
    n, d, k, metric = 4512, 64, 10, 0
    rows = make_corpus(77, n, d)
    labels = (np.random.default_rng(5).permutation(n).astype(np.uint64) << np.uint64(32)) | np.uint64(5)
    many = hostapi.GpuHnswMap(metric, d, n, M=8, ef_construction=80, devices=[0, 0, 0])
    many.add(rows, labels)
    graphs = [many.shard(s).export_graph(with_views=True) for s in range(3)]
    rng = np.random.default_rng(6)
    for qi in range(8):
        q = make_corpus(7800 + qi, 1, d)[0]
        chosen = labels[rng.random(n) < (0.3 if qi & 1 else 0.05)]
        parts = []
        for g in graphs:
            allowed = np.isin(g["labels"][:g["n"]], chosen)
            gv = dict(g)
            gv["vectors"] = np.array(g["vectors"])
            live = int(np.count_nonzero(allowed))
            if live == 0:
                continue
            if live <= 64:   # that shard takes the exact scan over its allowed rows
                idx = np.nonzero(allowed)[0]
                wd, wl = oracle.bf_search_knn(metric, gv["vectors"][idx], g["labels"][idx], None, q, k)
            else:
                wd, wl = oracle_hnsw_search_knn(oracle, hidden_copy(gv, allowed), q, k, 64, None)
            parts += list(zip(wd.tolist(), wl.tolist()))
        parts.sort()
        want = parts[:k]
        gd, gl = many.search_knn_filtered(q, k, 64, chosen)
        got = sorted(zip(gd.tolist(), gl.tolist()))
        assert [x[1] for x in got] == [x[1] for x in want], qi
        assert np.array_equal(bits([x[0] for x in got]), bits([x[0] for x in want]))
    many.close()


# ------------------------------------------------------------------------------------------------ 7. concurrent calls, each with its own filter
def test_concurrent_calls_bring_their_own_filters(rxgpu, oracle):
    from reindexer_amd import hostapi
    n, d, k = N_BUILT, 128, 10
    rows = make_corpus(5000 + d, n, d)
    labels = (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(9)
    m = hostapi.GpuHnswMap(0, d, n, M=16, ef_construction=100)
    m.add(rows, labels)
    queries = make_corpus(6300, 50, d)
    filters = [labels[np.random.default_rng(70 + t).random(n) < share] for t, share in enumerate((0.7, 0.4, 0.2, 0.08))]
    alone = [[m.search_knn_filtered(q, k, 64, f) for q in queries] for f in filters]
    wrong = []

    def work(t):
        for qi, q in enumerate(queries):
            gd, gl = m.search_knn_filtered(q, k, 64, filters[t])
            wd, wl = alone[t][qi]
            if not (np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd))):
                wrong.append((t, qi))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not wrong, wrong[:5]
    assert len({tuple(a[1].tolist()) for a in (alone[t][0] for t in range(4))}) > 1   # the filters do differ in what they return
    m.close()
