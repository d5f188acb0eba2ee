"""-m gpu: HNSW level 0 built on the device in batches (hnsw_build.hip through rxgpu_hnsw_link_batch, and through GpuHnswMap under
RXGPU_HNSW_BUILD=device).

Bar: the batch rule is deterministic given the rows and their order, so the device's level-0 lists equal the lists of the Python
restatement (tests/hnsw_batch_model.py: the oracle's search, the oracle's distances, selectNeighbors and connect()'s write order restated)
LINK FOR LINK — the whole [n][1 + maxM0] array.  Through the Map the upper levels, the entry point and the top level equal the sequential
host build's exactly; level 0 is the batched graph, whose recall@10 stays within 0.02 of the host-built graph's (the tolerance
tests/test_hnsw_builder.py gives the concurrent host build)."""
import ctypes as C

import numpy as np
import pytest

from . import hnsw_batch_model as bm
from .conftest import make_corpus
from .test_hnsw_batch_model import upper_fields_equal
from .test_hnsw_builder import exact_topk, graph_invariants, graphs_equal

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def labels_of(n):
    return np.arange(n, dtype=np.uint64) << np.uint64(32)


def upper_patch(after, touched, a, cnt):
    """(ids, levels, upper rows) of one rxgpu_hnsw_patch_upper: the older nodes LinkUpper touched, then every node of the batch."""
    ids = np.concatenate([touched[touched < a].astype(np.uint32), np.arange(a, a + cnt, dtype=np.uint32)])
    levels = after["levels"][ids].astype(np.int32)
    off = after["upper_off"]
    blocks = [after["upper"][int(off[i]):int(off[i]) + int(lv)].reshape(-1) for i, lv in zip(ids, levels) if lv]
    return ids, levels, np.concatenate(blocks) if blocks else np.empty(0, np.uint32)


def device_against_model(rxgpu, oracle, metric, rows, M, efc, seed, ratio, graph=None):
    """The model over the rows, its batches recorded; then the same batches through the C-ABI.  Returns (model lists, device lists, model
    statistics, device statistics)."""
    n, d = rows.shape
    labels = labels_of(n)
    recorded = []
    want, stats = bm.build(oracle, metric, rows, labels, M, efc, seed=seed, ratio=ratio, graph=graph,
                           on_batch=lambda a, cnt, before, touched, after: recorded.append((a, cnt, touched, after)))
    first, L = stats["first_export"], stats["seed"]
    inv = want["inv_norms"]
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows[:L], inv[:L] if inv is not None else None)
        ix.hnsw_attach_graph(bm.search_graph(first, L, rows) | dict(labels=first["labels"][:L]))
        ix.upload_rows(L, rows[L:], inv[L:] if inv is not None else None)
        for a, cnt, touched, after in recorded:
            ix.hnsw_link_batch(a, cnt, efc)
            ids, levels, upper_rows = upper_patch(after, touched, a, cnt)
            ix.hnsw_patch_upper(ids, levels, upper_rows, after["maxlevel"], after["entry"])
        got = ix.hnsw_read_links0(0, n, want["maxM0"])
        dstats = ix.hnsw_read_build_stats()
        # the finished mirror answers searches like the restated engine on the model's graph
        from oracle.pyoracle import oracle_hnsw_search_knn
        for qi in range(4):
            q = make_corpus(4000 + qi, 1, d)[0]
            if metric == 2:
                q, _ = oracle.normalize_copy(q)
            wd, wl = oracle_hnsw_search_knn(oracle, want, q, 10, 64, inv)
            dist, row, cnt_ = ix.hnsw_search_knn(q, 10, 64)
            c = int(cnt_[0])
            order = np.lexsort((row[0, :c], dist[0, :c]))
            assert np.array_equal(want["labels"][row[0, :c][order]], wl) and np.array_equal(bits(dist[0, :c][order]), bits(wd)), qi
    return want["links0"], got, stats, dstats


def assert_link_for_link(want, got):
    if not np.array_equal(want, got):
        bad = np.flatnonzero((want != got).any(axis=1))
        raise AssertionError(f"{bad.size} of {want.shape[0]} lists differ; first: node {bad[0]}\n model  {want[bad[0]]}\n device {got[bad[0]]}")


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_general_path_link_for_link(rxgpu, oracle, metric):
    rows = make_corpus(77, 3000, 48)
    want, got, stats, dstats = device_against_model(rxgpu, oracle, metric, rows, 12, 100, 256, 16)
    assert_link_for_link(want, got)
    assert dstats["rows"] == 3000 - 256 and dstats["batches"] == stats["batches"] and dstats["reselected"] == stats["reselected"] > 0
    assert dstats["past_cap"] == 0


def test_768_cosine_kept_rows_in_lds(rxgpu, oracle):
    rows = make_corpus(78, 1500, 768)
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 2, rows, 16, 200, 1024, 16)
    assert_link_for_link(want, got)
    assert dstats["rows"] == 1500 - 1024


def test_padded_stride_few_candidates_everything_reselected(rxgpu, oracle):
    """D = 50: a row stride of 52 floats, and the queries of a batch are packed first.  M = 4, efConstruction = 8, and batches half the size
    of the graph they search (ratio 2): almost every touched node overflows its 8 slots and is re-selected."""
    rows = make_corpus(79, 1000, 50)
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 0, rows, 4, 8, 64, 2)
    assert_link_for_link(want, got)
    assert dstats["reselected"] == stats["reselected"] and stats["reselected"] > 100


def test_fewer_candidates_than_m(rxgpu, oracle):
    """A graph of 6 nodes in front of the first batch, M = 8: every search returns fewer than M candidates and selectNeighbors returns
    them all — in connect()'s order."""
    rows = make_corpus(80, 200, 24)
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 2, rows, 8, 40, 6, 16)
    assert_link_for_link(want, got)


def test_equal_distances_and_a_hub(rxgpu, oracle):
    """64 exact copies of row 10 fill one batch: each finds its original at distance 0 and the copies before the batch do not exist yet, so
    row 10 receives 64 links at once; among equal distances the id order of selectNeighbors decides."""
    rows = make_corpus(81, 600, 32)
    rows[320:384] = rows[10]
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 0, rows, 8, 50, 64, 16)
    assert_link_for_link(want, got)
    assert (want[320:384, 1:1 + 8] == 10).any(axis=1).all()
    assert dstats["past_cap"] == 0


def test_a_hub_past_the_kernels_cap_is_finished_not_truncated(rxgpu, oracle):
    """280 copies of row 5 in one batch of 300 (ratio 1): row 5 holds more than 256 entries — the second launch re-selects it."""
    rows = make_corpus(82, 700, 32)
    rows[300:580] = rows[5]
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 0, rows, 8, 50, 300, 1)
    assert_link_for_link(want, got)
    assert dstats["past_cap"] >= 1


def test_appending_to_a_host_built_graph(rxgpu, oracle):
    from reindexer_amd import hostapi
    rows = make_corpus(83, 3000, 40)
    g = hostapi.HnswGraph(0, 40, 3000, M=10, ef_construction=80)
    g.add(rows[:2000], labels_of(3000)[:2000])
    want, got, stats, dstats = device_against_model(rxgpu, oracle, 0, rows, 10, 80, 1024, 16, graph=g)
    g.close()
    assert_link_for_link(want, got)
    assert dstats["rows"] == 1000


# ------------------------------------------------------------------------------------------------------------------ kept rows in L2; the caps
FIXED_LDS = (3 * 256 + 4 * 128) * 4   # candidate ids / distances / order; kept and heap ids / distances: the static arrays of the selection kernel


def select_lds_plan(d, M):
    """(static bytes, dynamic bytes, kept rows in LDS) of the selection kernel's launch for rows of d floats, as hnsw_build_plan.h decides it
    (tests/cpp/hnsw_build_plan_cpu.cc): a case asserts what it claims of its plan, so a changed budget cannot move it to the other kernel
    unnoticed."""
    from .test_hnsw_build_plan import LIB
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.hnsw_build_plan_lds.restype, L.hnsw_build_plan_lds.argtypes = None, [C.c_uint32, C.c_uint32, C.c_void_p]
    out = (C.c_uint32 * 3)()
    L.hnsw_build_plan_lds((d + 3) // 4 * 4, M, out)
    return tuple(int(x) for x in out)


def assert_rows_from_l2(d, M):
    """the new row and M kept rows do not fit beside the static arrays: hnsw_build_select<kMetric, false> reads the kept rows from L2"""
    assert (1 + M) * ((d + 3) // 4 * 4) * 4 + FIXED_LDS > 64 * 1024
    assert select_lds_plan(d, M) == (FIXED_LDS, 0, 0), (d, M, select_lds_plan(d, M))


def link_for_link_with_reselection(rxgpu, oracle, metric, rows, M, efc, seed, ratio=16):
    want, got, stats, dstats = device_against_model(rxgpu, oracle, metric, rows, M, efc, seed, ratio)
    assert_link_for_link(want, got)
    assert stats["reselected"] > 0, stats["reselected"]
    assert dstats["rows"] == rows.shape[0] - seed and dstats["batches"] == stats["batches"] and dstats["reselected"] == stats["reselected"], (
        dstats, stats["batches"], stats["reselected"])
    return want, got, stats, dstats


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_1024_float_rows_kept_rows_from_l2(rxgpu, oracle, metric):
    """1024 floats at M = 16: 17 rows are 69 632 bytes.  The batch search runs over the wide-row kernels, with a sink."""
    assert_rows_from_l2(1024, 16)
    link_for_link_with_reselection(rxgpu, oracle, metric, make_corpus(85, 1400, 1024), 16, 100, 1024)


def test_1536_float_rows_kept_rows_from_l2(rxgpu, oracle):
    """the same at three chunks of 512 floats"""
    assert_rows_from_l2(1536, 16)
    link_for_link_with_reselection(rxgpu, oracle, 2, make_corpus(86, 1300, 1536), 16, 100, 1024)


@pytest.mark.parametrize("metric", [0, 2])
def test_768_float_rows_at_m_32_kept_rows_from_l2(rxgpu, oracle, metric):
    """the fixed-dimension size whose kept rows fit at M = 16 (test_768_cosine_kept_rows_in_lds) and not from M = 19 on"""
    assert select_lds_plan(768, 18)[2] == 1 and select_lds_plan(768, 19)[2] == 0
    assert_rows_from_l2(768, 32)
    link_for_link_with_reselection(rxgpu, oracle, metric, make_corpus(87, 1300, 768), 32, 100, 1024)


@pytest.mark.parametrize("M,kept", [(58, True), (59, False)])
def test_launch_on_the_lds_budget_and_one_link_past_it(rxgpu, oracle, M, kept):
    """256 floats at M = 58: 59 rows are 60 416 bytes, and with the 5120 static bytes the launch takes 65 536 bytes, the whole budget;
    at M = 59 the kept rows are read from L2."""
    if kept:
        assert FIXED_LDS == 5120 and select_lds_plan(256, M) == (5120, 60416, 1) and 5120 + 60416 == 64 * 1024
    else:
        assert_rows_from_l2(256, M)
    link_for_link_with_reselection(rxgpu, oracle, 0, make_corpus(88, 900, 256), M, 120, 512)


@pytest.mark.parametrize("copies", [80, 300])
def test_m_and_ef_construction_at_their_caps(rxgpu, oracle, copies):
    """M = 64 (maxM0 = 128, the length of the kernel's kept and heap arrays) and efConstruction = 256 (its candidate arrays).  The batch
    [300, 600) (ratio 1) begins with copies of seed row 7: all of them find it at distance 0, so row 7 holds more than 128 entries and is
    re-selected at maxM0 = 128; with 300 copies it holds more than 256 and the second launch finishes it."""
    assert select_lds_plan(32, 64) == (FIXED_LDS, 65 * 32 * 4, 1)
    rows = make_corpus(89, 900, 32)
    rows[300:300 + copies] = rows[7]
    want, got, stats, dstats = link_for_link_with_reselection(rxgpu, oracle, 0, rows, 64, 256, 300, ratio=1)
    assert want.shape[1] == 1 + 128 and int(want[:, 0].max()) > 64, int(want[:, 0].max())
    held = stats["reselected_entries"].get(7, 0)   # the model: what row 7 held when it was re-selected
    if copies == 300:
        assert held > 256 and dstats["past_cap"] >= 1, (held, dstats)
    else:
        assert 128 < held <= 256 and max(stats["reselected_entries"].values()) <= 256 and dstats["past_cap"] == 0, (held, dstats)


def test_link_batch_refuses_what_it_does_not_take(rxgpu, oracle):
    rows = make_corpus(84, 400, 16)
    from reindexer_amd import hostapi
    g = hostapi.HnswGraph(0, 16, 400, M=8, ef_construction=40)
    g.add(rows[:300], labels_of(400)[:300])
    e = g.export()
    e["vectors"] = rows
    g.close()
    def refused(code, *args):
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.hnsw_link_batch(*args)
        assert err.value.code == code, (err.value, args)

    with rxgpu.VectorIndex(0, 16, 400) as ix:
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(e)
        refused(rxgpu.RXGPU_ERR_PARAMS, 300, 50, 40)      # rows not uploaded
        ix.upload_rows(300, rows[300:], None)
        refused(rxgpu.RXGPU_ERR_PARAMS, 299, 50, 40)      # not the attached node count
        refused(rxgpu.RXGPU_ERR_PARAMS, 300, 50, 257)     # efConstruction past the kernel's arrays
        ix.hnsw_link_batch(300, 50, 40)
        refused(rxgpu.RXGPU_ERR_LOGIC, 350, 50, 40)       # the upper lists of the batch before are not patched in
        assert ix.hnsw_read_links0(300, 50, 16)[:, 0].min() >= 1
    with rxgpu.VectorIndex(0, 16, 400) as ix:             # a graph with a deleted node
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(dict(e, num_deleted=1))
        ix.upload_rows(300, rows[300:], None)
        refused(rxgpu.RXGPU_ERR_PARAMS, 300, 50, 40)
    with rxgpu.VectorIndex(0, 16, 300) as ix:             # the level-0 array of the attach has no room for the batch
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(e)
        ix.reserve(400)
        ix.upload_rows(300, rows[300:], None)
        refused(rxgpu.RXGPU_ERR_OVERFLOW, 300, 50, 40)


# ------------------------------------------------------------------------------------------------------------------ through the Map
N, D, MM, EFC = 12000, 32, 16, 200


@pytest.fixture(scope="module")
def corpus():
    return make_corpus(5, N, D), labels_of(N), make_corpus(6, 300, D)


@pytest.fixture(scope="module")
def host_built(corpus):
    from reindexer_amd import hostapi
    rows, labels, _ = corpus
    out = {}
    for metric in (0, 2):
        g = hostapi.HnswGraph(metric, D, N, M=MM, ef_construction=EFC)
        g.add(rows, labels)
        out[metric] = g.export()
        out[metric]["vectors"] = rows
        g.close()
    return out


def recall_of(oracle, graph, metric, rows, labels, queries):
    from oracle.pyoracle import oracle_hnsw_search_knn
    lab2row = {int(l): i for i, l in enumerate(labels)}
    vec = np.stack([rows[lab2row[int(l)]] for l in graph["labels"]])
    g = dict(graph, vectors=vec)
    inv = oracle.l2_modules(vec) if metric == 2 else None
    hit = 0
    for q in queries:
        qq = oracle.normalize_copy(q)[0] if metric == 2 else q
        _, got = oracle_hnsw_search_knn(oracle, g, qq, 10, 64, inv)
        hit += len(set(int(x) for x in got) & set(int(x) for x in labels[exact_topk(rows, qq, 10, metric)]))
    return hit / (10 * len(queries))


def device_lists(rxgpu, m, n, max_m0):
    out = np.empty((n, 1 + max_m0), np.uint32)
    rc = rxgpu.lib().rxgpu_hnsw_read_links0(C.c_void_p(m.device_index), 0, n, out.ctypes.data)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("threads", [0, 8])
@pytest.mark.parametrize("metric", [0, 2])
def test_map_builds_on_the_device(rxgpu, oracle, corpus, host_built, monkeypatch, metric, threads):
    from oracle.pyoracle import oracle_hnsw_search_knn
    from reindexer_amd import hostapi
    rows, labels, queries = corpus
    monkeypatch.setenv("RXGPU_HNSW_BUILD", "device")
    m = hostapi.GpuHnswMap(metric, D, N, M=MM, ef_construction=EFC, multithread=True)
    if threads:
        m.add(rows, labels, threads=threads)          # AddPointConcurrent from 8 threads: row order = arrival order
    else:
        m.add_points(rows, labels)
    assert m.count == N and m.pending_rows == N
    q0 = oracle.normalize_copy(queries[0])[0] if metric == 2 else queries[0]
    m.search_knn(q0, 10, 64)                          # the first search links everything
    assert m.pending_rows == 0
    st = m.build_stats()
    assert st["seed_rows"] == 1024 and st["device_rows"] == N - 1024 and st["host_rows"] == 0 and st["past_cap"] == 0, st
    e = m.export_graph()
    graph_invariants(e, N, MM)
    if not threads:
        upper_fields_equal(e, host_built[metric])     # levels, every upper list, entry point, top level: the sequential build's
    else:
        assert np.array_equal(np.sort(e["labels"]), labels)
    assert np.array_equal(device_lists(rxgpu, m, N, 2 * MM), e["links0"])
    r_dev, r_host = recall_of(oracle, e, metric, rows, labels, queries), recall_of(oracle, host_built[metric], metric, rows, labels, queries)
    print(f"recall@10 ef=64 metric {metric} threads {threads}: device-built {r_dev:.4f} host-built {r_host:.4f}")
    assert abs(r_dev - r_host) <= 0.02, (r_dev, r_host)
    lab2row = {int(l): i for i, l in enumerate(labels)}
    vec = np.stack([rows[lab2row[int(l)]] for l in e["labels"]])
    g = dict(e, vectors=vec)
    inv = oracle.l2_modules(vec) if metric == 2 else None
    for q in queries[:10]:
        qq = oracle.normalize_copy(q)[0] if metric == 2 else q
        wd, wl = oracle_hnsw_search_knn(oracle, g, qq, 10, 64, inv)
        gd, gl = m.search_knn(qq, 10, 64)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd))
    m.close()


# ------------------------------------------------------------------------------------------------------------------ deferral
SN, SD, SM, SEFC = 3000, 32, 8, 60


@pytest.fixture()
def small(monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_BUILD", "device")
    monkeypatch.setenv("RXGPU_HNSW_BUILD_SEED", "256")
    return make_corpus(91, SN + 1, SD), labels_of(SN + 1)


def test_rows_are_stored_at_once_and_linked_by_the_first_search(rxgpu, small):
    from reindexer_amd import hostapi
    rows, labels = small
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add(rows[:SN], labels[:SN], threads=4)
    assert m.count == SN and m.pending_rows == SN
    assert np.array_equal(m.vector(labels[1234]), rows[1234])
    assert m.build_stats()["device_rows"] == 0
    _, gl = m.search_knn(rows[77], 1, 32)
    assert gl[0] == labels[77] and m.pending_rows == 0
    st = m.build_stats()
    assert st["device_rows"] == SN - 256 and st["seed_rows"] == 256 and st["batches"] > 0
    m.close()


def test_mark_delete_and_save_index_flush_first(rxgpu, small):
    from reindexer_amd import hostapi
    rows, labels = small
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows[:SN], labels[:SN])
    assert m.pending_rows == SN
    m.mark_delete(labels[2000])
    assert m.pending_rows == 0 and m.deleted_count == 1 and m.build_stats()["device_rows"] == SN - 256
    m.close()
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows[:SN], labels[:SN])
    blob = m.save_index()
    assert m.pending_rows == 0 and len(blob) > SN * 8
    graph_invariants(m.export_graph(), SN, SM)
    m.close()


def test_a_later_add_point_is_the_hosts(rxgpu, small):
    """After the device build AddPointNoLock runs on the host as ever: it produces what HnswGraph::AddPoint produces on that graph."""
    from reindexer_amd import hostapi
    rows, labels = small
    m = hostapi.GpuHnswMap(2, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows[:SN], labels[:SN])
    e = m.export_graph()
    assert m.pending_rows == 0
    g = hostapi.HnswGraph(2, SD, SN + 1, M=SM, ef_construction=SEFC)   # the same graph on the host: same levels, same upper lists, the device's level 0
    g.append_unlinked(rows[:SN], labels[:SN])
    g.link_stored(0, 256)
    g.link_upper(256, SN - 256)
    g.set_links0(0, e["links0"])
    graphs_equal(g.export(), e)
    m.add(rows[SN:], labels[SN:])
    g.add(rows[SN:], labels[SN:])
    e2 = m.export_graph()
    graphs_equal(g.export(), e2)
    _, gl = m.search_knn(m.vector(labels[SN]) / np.linalg.norm(rows[SN]), 1, 32)   # ... and the mirror follows (patched in place)
    assert gl[0] == labels[SN]
    assert np.array_equal(device_lists(rxgpu, m, SN + 1, 2 * SM), e2["links0"])
    g.close()
    m.close()


def test_a_graph_with_a_deleted_node_takes_the_host_path(rxgpu, small):
    from reindexer_amd import hostapi
    rows, labels = small
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows[:600], labels[:600])
    m.mark_delete(labels[5])
    m.mark_delete(labels[6])
    m.build_stats()
    m.add_points(rows[600:601], labels[600:601])      # recycles a slot: a host insertion
    assert m.pending_rows == 0
    st = m.build_stats()
    assert st["host_rows"] == 1 and st["host_reason"] == 1 and st["device_rows"] == 0, st
    m.add(rows[601:700], labels[601:700], threads=4)
    st = m.build_stats()
    assert st["host_rows"] >= 1 and st["host_reason"] == 1, st
    _, gl = m.search_knn(rows[650], 1, 32)
    assert gl[0] == labels[650]
    m.close()


def test_without_the_variable_nothing_changes(rxgpu, small, monkeypatch):
    from reindexer_amd import hostapi
    rows, labels = small
    monkeypatch.delenv("RXGPU_HNSW_BUILD")
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add(rows[:SN], labels[:SN], threads=4)
    assert m.pending_rows == 0
    m.add_points(rows[SN:], labels[SN:])
    assert m.pending_rows == 0
    m.search_knn(rows[3], 1, 32)
    st = m.build_stats()
    assert all(st[k] == 0 for k in ("device_rows", "batches", "seed_rows", "host_rows", "host_reason")), st
    m.close()


def test_variable_switched_back_with_rows_pending(rxgpu, small, monkeypatch):
    """The variable is read per call: rows stored under "device" are linked before a later concurrent add takes the host path."""
    from reindexer_amd import hostapi
    rows, labels = small
    m = hostapi.GpuHnswMap(0, SD, SN + 1, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows[:1000], labels[:1000])
    assert m.pending_rows == 1000
    monkeypatch.setenv("RXGPU_HNSW_BUILD", "host")
    m.add_concurrent(rows[1000], labels[1000])
    assert m.pending_rows == 0 and m.count == 1001
    st = m.build_stats()
    assert st["device_rows"] == 1000 - 256, st
    graph_invariants(m.export_graph(), 1001, SM)
    _, gl = m.search_knn(rows[1000], 1, 32)
    assert gl[0] == labels[1000]
    m.close()


# ------------------------------------------------------------------------------------------------------------------ quantised Maps
def sq8_codes(rxgpu, m, n, d):
    codes, corr = np.empty((n, d), np.uint8), np.empty(n, np.float32)
    rc = rxgpu.lib().rxgpu_hnsw_read_sq8_rows(C.c_void_p(m.device_index), 0, n, codes.ctypes.data, corr.ctypes.data)
    assert rc == 0, rc
    return codes, corr


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("order", ["quantize_first", "extend_synced"])
def test_quantised_map_built_on_the_device(rxgpu, oracle, small, monkeypatch, metric, order):
    """A quantised Map codes the rows the device build links as it codes every other new row: on the device, with the Map's parameters.
    quantize_first: Quantize on an empty Map, then the rows, then the first search (codes and links in one flush + sync); extend_synced: a
    searched, quantised Map is extended.  Codes and corrective offsets equal those of a host-built Map over the same rows (they depend on
    the row alone), and searches equal the restated quantised engine on the exported graph."""
    from oracle.pyoracle import Sq8Oracle, oracle_hnsw_search_knn_sq8
    from reindexer_amd import hostapi
    rows, labels = small
    rows, labels = rows[:SN], labels[:SN]
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))
    first = 0 if order == "quantize_first" else 1200

    def query(x):   # (vector, query_data_norm) as HnswIndexBase::search passes them: a quantised cosine graph needs the norm
        if metric != 2:
            return x, None
        v, k_ = oracle.normalize_copy(x)
        return v, float(np.float32(1.0) / np.float32(k_))

    def search(m, x, k=10, ef=64):
        v, norm = query(x)
        return m.search_knn_norm(v, k, ef, norm)

    def build(mode):
        monkeypatch.setenv("RXGPU_HNSW_BUILD", mode)
        m = hostapi.GpuHnswMap(metric, SD, SN, M=SM, ef_construction=SEFC, multithread=True)
        if first:
            m.add_points(rows[:first], labels[:first])
            search(m, rows[0], 1, 32)
        m.quantize(min_q, max_q)
        if first:
            search(m, rows[0], 1, 32)
        m.add_points(rows[first:], labels[first:])
        return m

    dev, host = build("device"), build("host")
    assert dev.pending_rows == SN - first and host.pending_rows == 0
    q = make_corpus(92, 6, SD)
    got = [search(dev, x) for x in q]
    search(host, q[0])
    assert dev.pending_rows == 0 and dev.build_stats()["device_rows"] == SN - 256   # (both flushes of the extended Map together)
    dc, dr = sq8_codes(rxgpu, dev, SN, SD)
    hc, hr = sq8_codes(rxgpu, host, SN, SD)
    assert np.array_equal(dc, hc) and np.array_equal(bits(dr), bits(hr))
    assert dev.device_coded_rows() >= SN
    e = dev.export_graph()
    e["vectors"] = rows
    sq8 = Sq8Oracle(oracle)
    pq = sq8.params(min_q, max_q, SD)
    stored = [sq8.quantize(metric, pq, x) for x in rows]
    assert np.array_equal(np.stack([c for c, _ in stored]), dc)
    sq = dict(min_q=pq["min_q"], alpha=pq["alpha"], alpha_2=pq["alpha_2"], delta=pq["delta"], codes=dc, corr=dr)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    for x, (gd, gl) in zip(q, got):
        v, norm = query(x)
        wd, wl = oracle_hnsw_search_knn_sq8(oracle, e, sq, v, 10, 64, inv, norm)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd))
    dev.close()
    host.close()
