"""-m gpu: GpuHnswMap under RXGPU_HNSW_BUILD=device with RXGPU_HNSW_BUILD_UPPER=device — level 1 of every batch linked on the device, the
levels >= 2 on the host beside it, level 1 taken home when the flush ends.

Bar: the exported graph equals the Python restatement's (tests/hnsw_batch_model_l1.py) IN FULL — every list of every level, the entry
point, the top level — the device's level-0 and level-1 lists equal the export, and searches equal the restated engine on the export.
Recall@10 of the larger build stays within 0.02 of the host-built graph's (the tolerance tests/test_hnsw_builder.py gives the concurrent
host build)."""
import ctypes as C

import numpy as np
import pytest

from . import hnsw_batch_model as bm
from . import hnsw_batch_model_l1 as bm1
from . import hnsw_l1_cases as cases
from .conftest import make_corpus
from .test_gpu_hnsw_build import corpus, device_lists, host_built, recall_of, sq8_codes  # noqa: F401  (corpus, host_built: fixtures)
from .test_hnsw_batch_model import upper_fields_equal
from .test_hnsw_builder import graph_invariants, graphs_equal

pytestmark = pytest.mark.gpu

SN, SD, SM, SEFC = 3000, 32, 8, 60


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture()
def small(monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_BUILD", "device")
    monkeypatch.setenv("RXGPU_HNSW_BUILD_UPPER", "device")
    monkeypatch.setenv("RXGPU_HNSW_BUILD_SEED", "256")
    return make_corpus(191, SN, SD), cases.labels_of(SN)


def device_level1(rxgpu, m, n, M):
    ids = np.arange(n, dtype=np.uint32)
    out = np.empty((n, 1 + M), np.uint32)
    rc = rxgpu.lib().rxgpu_hnsw_read_level(C.c_void_p(m.device_index), 1, n, ids.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def searches_equal_the_engine(oracle, m, e, rows, metric, queries):
    from oracle.pyoracle import oracle_hnsw_search_knn
    g = dict(e, vectors=rows)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    for q in queries:
        qq = oracle.normalize_copy(q)[0] if metric == 2 else q
        wd, wl = oracle_hnsw_search_knn(oracle, g, qq, 10, 64, inv)
        gd, gl = m.search_knn(qq, 10, 64)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd))


def map_against_model(rxgpu, oracle, metric, rows, labels, M, efc, seed, max_elements=None):
    """The Map over the rows (one flush, at the first search) against build_l1: the whole graph, both mirrors, the searches.  Returns
    (export, model statistics, the Map's statistics)."""
    from reindexer_amd import hostapi
    n, d = rows.shape
    want, stats = bm1.build_l1(oracle, metric, rows, labels, M, efc, seed=seed)
    m = hostapi.GpuHnswMap(metric, d, max_elements or n, M=M, ef_construction=efc, multithread=True)
    m.add_points(rows, labels)
    assert m.pending_rows == n
    m.search_knn(rows[0] if metric != 2 else oracle.normalize_copy(rows[0])[0], 1, 32)       # the first search links everything
    assert m.pending_rows == 0
    st = m.build_stats()
    e = m.export_graph()
    graphs_equal(e, want)
    assert np.array_equal(device_lists(rxgpu, m, n, 2 * M), e["links0"])
    assert np.array_equal(device_level1(rxgpu, m, n, M), cases.level1_lists(e))
    searches_equal_the_engine(oracle, m, e, rows, metric, make_corpus(192, 6, d))
    m.close()
    return e, stats, st


@pytest.mark.parametrize("metric", [0, 2])
def test_map_link_for_link(rxgpu, oracle, small, metric):
    rows, labels = small
    e, stats, st = map_against_model(rxgpu, oracle, metric, rows, labels, SM, SEFC, 256)
    up = int((e["levels"][256:] >= 1).sum())
    assert st["seed_rows"] == 256 and st["device_rows"] == SN - 256 and st["batches"] == stats["batches"], st
    assert st["upper_device_rows"] == up == stats["l1_rows"] > 100 and st["upper_host_rows"] == 0, st      # every level-1 row on the device
    assert st["reselected"] == stats["reselected"] and st["upper_reselected"] == stats["reselected_l1"] > 0, (st, stats["reselected_l1"])
    assert st["upper_past_cap"] == 0 and st["upper_search_ms"] > 0, st


def test_map_with_a_tiny_seed(rxgpu, oracle, small, monkeypatch):
    """A seed of 4 rows of level 0: the first batches have a graph of top level 0 in front of them and the host links their level 1; the
    device takes over later in the same flush."""
    monkeypatch.setenv("RXGPU_HNSW_BUILD_SEED", "4")
    rows, labels = small
    rows, labels = rows[:2000], labels[:2000]
    lv = cases.levels_of(0, rows, 16, SEFC)
    assert (lv[:4] == 0).all()
    e, stats, st = map_against_model(rxgpu, oracle, 0, rows, labels, 16, SEFC, 4)
    assert st["seed_rows"] == 4 and stats["l1_host_rows"] >= 1 and stats["l1_rows"] >= 1, stats
    assert st["upper_host_rows"] == stats["l1_host_rows"] and st["upper_device_rows"] == stats["l1_rows"], (st, stats)
    assert st["upper_host_rows"] + st["upper_device_rows"] == int((lv[4:] >= 1).sum())


def test_map_with_upper_blocks_running_out(rxgpu, oracle, small, monkeypatch):
    """40 blocks of headroom an attach: rxgpu_hnsw_patch_upper_from answers RXGPU_ERR_OVERFLOW several times in the flush, level 0 and the
    device's level 1 — the waiting lists of the batch included — come home, the graph is attached again and the build goes on."""
    monkeypatch.setenv("RXGPU_HNSW_UPPER_HEADROOM", "40")
    rows, labels = small
    e, stats, st = map_against_model(rxgpu, oracle, 0, rows, labels, SM, SEFC, 256)
    blocks = int(e["levels"][256:].sum())
    assert blocks > 5 * 40                                            # more than five attaches' worth
    assert st["upper_device_rows"] == stats["l1_rows"] and st["upper_reselected"] == stats["reselected_l1"], (st, stats["reselected_l1"])


@pytest.mark.parametrize("metric", [0, 2])
def test_map_recall(rxgpu, oracle, corpus, host_built, monkeypatch, metric):
    from reindexer_amd import hostapi
    N, D, MM, EFC = 12000, 32, 16, 200
    rows, labels, queries = corpus
    monkeypatch.setenv("RXGPU_HNSW_BUILD", "device")
    monkeypatch.setenv("RXGPU_HNSW_BUILD_UPPER", "device")
    m = hostapi.GpuHnswMap(metric, D, N, M=MM, ef_construction=EFC, multithread=True)
    m.add_points(rows, labels)
    q0 = oracle.normalize_copy(queries[0])[0] if metric == 2 else queries[0]
    m.search_knn(q0, 10, 64)
    assert m.pending_rows == 0
    st = m.build_stats()
    e = m.export_graph()
    graph_invariants(e, N, MM)
    assert st["upper_device_rows"] == int((e["levels"][1024:] >= 1).sum()) and st["upper_host_rows"] == 0, st
    assert np.array_equal(e["levels"], host_built[metric]["levels"]) and e["entry"] == host_built[metric]["entry"]
    assert np.array_equal(device_level1(rxgpu, m, N, MM), cases.level1_lists(e))
    r_dev, r_host = recall_of(oracle, e, metric, rows, labels, queries), recall_of(oracle, host_built[metric], metric, rows, labels, queries)
    print(f"recall@10 ef=64 metric {metric}: level 0 and 1 device-built {r_dev:.4f} host-built {r_host:.4f}")
    assert abs(r_dev - r_host) <= 0.02, (r_dev, r_host)
    m.close()


def test_quantised_map(rxgpu, oracle, small, monkeypatch):
    """quantize_first: Quantize on an empty Map, then the rows, then the first search.  Codes and corrective offsets equal those of a
    host-built Map over the same rows, and searches equal the restated quantised engine on the exported graph."""
    from oracle.pyoracle import Sq8Oracle, oracle_hnsw_search_knn_sq8
    from reindexer_amd import hostapi
    rows, labels = small
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))

    def build(mode):
        monkeypatch.setenv("RXGPU_HNSW_BUILD", mode)
        m = hostapi.GpuHnswMap(0, SD, SN, M=SM, ef_construction=SEFC, multithread=True)
        m.quantize(min_q, max_q)
        m.add_points(rows, labels)
        return m

    dev, host = build("device"), build("host")
    assert dev.pending_rows == SN and host.pending_rows == 0
    q = make_corpus(193, 6, SD)
    got = [dev.search_knn_norm(x, 10, 64, None) for x in q]
    host.search_knn_norm(q[0], 10, 64, None)
    st = dev.build_stats()
    assert dev.pending_rows == 0 and st["device_rows"] == SN - 256 and st["upper_device_rows"] > 100 and st["upper_host_rows"] == 0, st
    dc, dr = sq8_codes(rxgpu, dev, SN, SD)
    hc, hr = sq8_codes(rxgpu, host, SN, SD)
    assert np.array_equal(dc, hc) and np.array_equal(bits(dr), bits(hr))
    e = dev.export_graph()
    e["vectors"] = rows
    sq8 = Sq8Oracle(oracle)
    pq = sq8.params(min_q, max_q, SD)
    sq = dict(min_q=pq["min_q"], alpha=pq["alpha"], alpha_2=pq["alpha_2"], delta=pq["delta"], codes=dc, corr=dr)
    for x, (gd, gl) in zip(q, got):
        wd, wl = oracle_hnsw_search_knn_sq8(oracle, e, sq, x, 10, 64, None, None)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd))
    dev.close()
    host.close()


def test_variable_unset_nothing_changes(rxgpu, oracle, small, monkeypatch):
    """RXGPU_HNSW_BUILD=device alone: level 1 stays on the host — the graph is the level-0 rule's, its upper fields the sequential build's."""
    from reindexer_amd import hostapi
    monkeypatch.delenv("RXGPU_HNSW_BUILD_UPPER")
    rows, labels = small
    want, stats = bm.build(oracle, 0, rows, labels, SM, SEFC, seed=256)
    seq = hostapi.HnswGraph(0, SD, SN, M=SM, ef_construction=SEFC)
    seq.add(rows, labels)
    m = hostapi.GpuHnswMap(0, SD, SN, M=SM, ef_construction=SEFC, multithread=True)
    m.add_points(rows, labels)
    m.search_knn(rows[0], 1, 32)
    st = m.build_stats()
    assert st["upper_device_rows"] == 0 and st["upper_reselected"] == 0 and st["upper_search_ms"] == 0, st
    assert st["upper_host_rows"] == int((want["levels"][256:] >= 1).sum()) and st["device_rows"] == SN - 256, st
    e = m.export_graph()
    graphs_equal(e, want)
    upper_fields_equal(e, seq.export())
    monkeypatch.setenv("RXGPU_HNSW_BUILD_UPPER", "host")              # "host" says the same
    m2 = hostapi.GpuHnswMap(0, SD, SN, M=SM, ef_construction=SEFC, multithread=True)
    m2.add_points(rows, labels)
    m2.search_knn(rows[0], 1, 32)
    assert m2.build_stats()["upper_device_rows"] == 0
    graphs_equal(m2.export_graph(), want)
    seq.close()
    m.close()
    m2.close()
