"""HNSW search over float rows of 1024 and 1536 components: the fixed-dimension distance batch that reads a row in chunks
(batch_distances_wide, hnsw_search_core.hip.h) behind every launch path and behind the resident kernel (hnsw_server_wide_kernel).  The bar is
the one of tests/test_gpu_row_layout.py, whose harness this file uses: the labels and the distance bits of the restated engine, on owned,
padded and page-aligned rows.  3000 rows, M = 16: a hop's fresh neighbours are rarely a multiple of 4 or 8, the four plans cover both list
classes, the 12 single queries take the team launch (or the mailbox), the 300 tiled ones the one-wavefront latency form and 3600 the
throughput form.  The sizes next to the new ones (17 and 23 blocks) keep the generic batch."""
import numpy as np
import pytest

from .test_gpu_row_layout import PLANS, _check_hnsw, _graph, _hnsw_layouts, _hnsw_wants

pytestmark = pytest.mark.gpu

WIDE = (1024, 1536)   # 16 and 24 blocks of 64 floats: two and three chunks of eight
DELETED = 300


def _launched(monkeypatch, ixs, g, q, wants, k, ef, what):
    """the 12 queries one at a time as launches (no resident kernel), then 300 in one call"""
    batch = np.tile(q, (25, 1))
    monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")
    for name, ix in ixs.items():
        for i in range(12):
            _check_hnsw(g, ix.hnsw_search_knn(q[i][None, :], k, ef), wants[i:i + 1], what + ("nq = 1, launched", name, k, ef, i))
        _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 25, what + ("nq = 300", name, k, ef))


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", WIDE)
def test_wide_rows_launches_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    g, rows, inv, q = _graph(oracle, metric, d)
    with _hnsw_layouts(rxgpu, metric, g, rows, inv) as ixs:
        for k, ef in PLANS:
            _launched(monkeypatch, ixs, g, q, _hnsw_wants(oracle, metric, d, k, ef), k, ef, (metric, d))


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("deleted", [0, DELETED])
@pytest.mark.parametrize("d", WIDE)
def test_wide_rows_throughput_form(rxgpu, oracle, monkeypatch, metric, deleted, d):
    """a launch of up to 3072 searches (1024 at 1536 floats) takes the latency form — two row sets in chunks of 8; above that the throughput
    form reads one row set in chunks of 4: 3600 searches in one call are the smallest batch that takes it at both sizes"""
    g, rows, inv, q = _graph(oracle, metric, d, deleted)
    batch = np.tile(q, (300, 1))
    monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, ("owned", "padded20")) as ixs:
        for k, ef in PLANS:
            wants = _hnsw_wants(oracle, metric, d, k, ef, deleted)
            for name, ix in ixs.items():
                _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 300, ("nq = 3600", name, metric, d, deleted, k, ef))


@pytest.mark.parametrize("d", WIDE)
def test_wide_rows_inner_product(rxgpu, oracle, monkeypatch, d):
    g, rows, inv, q = _graph(oracle, 1, d)
    with _hnsw_layouts(rxgpu, 1, g, rows, inv, ("owned",)) as ixs:
        for k, ef in PLANS:
            _launched(monkeypatch, ixs, g, q, _hnsw_wants(oracle, 1, d, k, ef), k, ef, (1, d))


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("case", ["heaps_only", "global_candidate_heap", "300_deleted"])
@pytest.mark.parametrize("d", WIDE)
def test_wide_rows_other_kernels_behind_the_switch(rxgpu, oracle, monkeypatch, metric, case, d):
    """the heap kernels, the global candidate heap (kGlobalCand with NB > 0) and the sorted list of a graph with deleted nodes"""
    deleted = DELETED if case == "300_deleted" else 0
    g, rows, inv, q = _graph(oracle, metric, d, deleted)
    if case == "heaps_only":
        monkeypatch.setenv("RXGPU_HNSW_SORTED", "0")
    if case == "global_candidate_heap":
        monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "4")
    batch = np.tile(q, (25, 1))
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, ("owned", "padded20")) as ixs:
        for k, ef in PLANS:
            wants = _hnsw_wants(oracle, metric, d, k, ef, deleted)
            for name, ix in ixs.items():
                for i in range(12):
                    _check_hnsw(g, ix.hnsw_search_knn(q[i][None, :], k, ef), wants[i:i + 1], (case, "nq = 1", name, metric, d, k, ef, i))
                _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 25, (case, "nq = 300", name, metric, d, k, ef))


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("deleted", [0, DELETED])
@pytest.mark.parametrize("d", WIDE)
def test_wide_rows_through_the_mailbox(rxgpu, oracle, metric, deleted, d):
    """the resident kernel serves 1024 and 1536 floats per row in both list classes, with and without deleted nodes, on strided rows too; a
    search that comes back flagged for the re-run tiers is answered by rxgpu_hnsw_search_knn, the caller's next step.  The allowance is the
    one of test_hnsw_posted_search_over_every_layout, 0.9 of the calls — of the calls the mailbox takes at all: on a graph with deleted nodes
    it declines ef > 224 at every size (include/rxgpu.h), which is the plan (60, 250): there 36 of the 48 calls can be served, and the
    twelve of that plan must be declined."""
    g, rows, inv, q = _graph(oracle, metric, d, deleted)
    taken = [(k, ef) for k, ef in PLANS if ef <= (224 if deleted else 256)]
    assert len(taken) == (3 if deleted else 4)
    with _hnsw_layouts(rxgpu, metric, g, rows, inv) as ixs:
        for name, ix in ixs.items():
            served = 0
            for k, ef in PLANS:
                wants = _hnsw_wants(oracle, metric, d, k, ef, deleted)
                for i in range(12):
                    pd, pr, pc, ok = ix.hnsw_search_knn_posted(q[i], k, ef)
                    if (k, ef) not in taken:
                        assert not ok, (name, metric, d, deleted, k, ef, i)
                    if ok:
                        served += 1
                        got = (pd[None, :], pr[None, :], np.array([pc]))
                    else:
                        got = ix.hnsw_search_knn(q[i][None, :], k, ef)
                    _check_hnsw(g, got, wants[i:i + 1], ("posted", ok, name, metric, d, deleted, k, ef, i))
            print("served", name, metric, d, deleted, served, "of", 12 * len(taken))
            assert served >= 0.9 * 12 * len(taken), (name, metric, d, deleted, served)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [1088, 1472])   # 17 and 23 blocks
def test_sizes_next_to_the_wide_ones_stay_generic(rxgpu, oracle, monkeypatch, metric, d):
    from reindexer_amd import capi
    assert capi.hnsw_distance_blocks(d) == (0, False) and capi.hnsw_distance_blocks(d, deleted=True) == (0, False)
    g, rows, inv, q = _graph(oracle, metric, d)
    batch = np.tile(q, (25, 1))
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, ("owned", "padded20")) as ixs:
        for k, ef in PLANS:
            wants = _hnsw_wants(oracle, metric, d, k, ef)
            for name, ix in ixs.items():
                for i in range(12):
                    pd, pr, pc, ok = ix.hnsw_search_knn_posted(q[i], k, ef)
                    assert not ok, (name, metric, d, k, ef, i)
                    _check_hnsw(g, ix.hnsw_search_knn(q[i][None, :], k, ef), wants[i:i + 1], ("nq = 1", name, metric, d, k, ef, i))
                _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 25, ("nq = 300", name, metric, d, k, ef))
