"""CPU: the host side of the batched HNSW build (HnswGraph::AppendUnlinked / LinkStored / LinkUpper / SetLinks0) and the batch rule as
tests/hnsw_batch_model.py restates it.

  * stored rows linked by LinkStored give the sequential graph, link for link;
  * AppendUnlinked + LinkUpper over all rows give the levels, every upper list, the entry point and the top level of the sequential add():
    levels >= 1 never read level 0;
  * the model's graph is a valid graph, and its recall@10 is within 0.02 of the sequential graph's — the tolerance
    tests/test_hnsw_builder.py gives the reference-style concurrent build (same corpus, same queries, same ef)."""
import numpy as np
import pytest

from . import hnsw_batch_model as bm
from .conftest import make_corpus
from .test_hnsw_builder import exact_topk, graph_invariants, graphs_equal


def upper_fields_equal(a, b):
    for key in ("n", "M", "maxM0", "maxlevel", "entry", "num_deleted"):
        assert a[key] == b[key], key
    for key in ("levels", "labels", "deleted", "upper_off"):
        assert np.array_equal(a[key], b[key]), key
    blocks = int(a["upper_off"][-1])
    assert np.array_equal(a["upper"][:blocks], b["upper"][:blocks]), "upper"


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_link_upper_gives_the_sequential_upper_levels(metric):
    from reindexer_amd import hostapi
    n, d, M, efc = 3000, 48, 12, 100
    rows = make_corpus(77, n, d)
    labels = np.arange(n, dtype=np.uint64) << np.uint64(32)
    seq = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    seq.add(rows, labels)
    g = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    g.append_unlinked(rows, labels)
    assert g.pending_from == 0
    g.link_stored(0, 1)            # the first element has nothing to search
    touched = g.link_upper(1, n - 1)
    e, s = g.export(), seq.export()
    upper_fields_equal(e, s)
    assert (e["links0"][1:, 0] == 0).all()                       # level 0 untouched
    assert set(int(x) for x in touched) <= set(int(x) for x in np.flatnonzero(s["levels"] > 0))
    assert g.pending_from == 1
    with pytest.raises(hostapi.HostError, match="not linked yet"):
        g.add(rows[:1], np.array([1 << 60], np.uint64))
    g.set_links0(0, s["links0"])
    assert g.pending_from == n
    graphs_equal(g.export(), s)
    seq.close()
    g.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_link_stored_equals_add(metric):
    from reindexer_amd import hostapi
    n, d, M, efc = 1200, 40, 8, 60
    rows = make_corpus(9, n, d)
    labels = np.arange(n, dtype=np.uint64) << np.uint64(32)
    seq = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    seq.add(rows, labels)
    g = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    g.add(rows[:300], labels[:300])
    g.append_unlinked(rows[300:], labels[300:])
    g.link_stored(300, 500)
    g.link_stored(800, 400)
    graphs_equal(g.export(), seq.export())
    with pytest.raises(hostapi.HostError, match="the label exists"):
        g.append_unlinked(rows[:1], labels[:1])
    seq.close()
    g.close()


def test_model_heap_and_walk_order():
    """The two orders of the rule on a hand-made case: equal distances are walked larger id first; the written order is what a max-heap on
    the distance alone pops."""
    m = bm.BatchModel(None, 0, None, None)
    ids, dist = np.array([3, 9, 5, 7]), np.array([0.5, 0.25, 0.25, 1.0], np.float32)
    assert m.select(ids, dist, 8) == [7, 3, 9, 5]    # fewer than the limit: all kept (walk 9, 5, 3, 7), heap pops 7, 3, then 9 before 5
    h = bm._ByFirstHeap()
    for d_, i_ in [(1.0, 1), (1.0, 2), (1.0, 3)]:
        h.push(d_, i_)
    assert [h.pop() for _ in range(3)] == [1, 3, 2]  # ties: the heap's sift order, not the ids


@pytest.fixture(scope="module")
def recall_case(oracle):
    n, d, M, efc = 12000, 32, 16, 200
    rows = make_corpus(5, n, d)
    labels = np.arange(n, dtype=np.uint64) << np.uint64(32)
    return n, d, M, efc, rows, labels, make_corpus(6, 300, d)


@pytest.mark.parametrize("metric", [0, 2])
def test_model_graph_is_valid_and_keeps_the_recall(oracle, recall_case, metric):
    from oracle.pyoracle import oracle_hnsw_search_knn
    from reindexer_amd import hostapi
    n, d, M, efc, rows, labels, queries = recall_case
    seq = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    seq.add(rows, labels)
    s = seq.export()
    s["vectors"] = rows
    seq.close()
    g, stats = bm.build(oracle, metric, rows, labels, M, efc)
    assert stats["seed"] == 1024 and stats["batches"] > 10
    graph_invariants(g, n, M)
    upper_fields_equal(g, s)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    recall = {}
    for name, graph in (("seq", s), ("batched", g)):
        hit = 0
        for q in queries:
            qq = oracle.normalize_copy(q)[0] if metric == 2 else q
            _, got = oracle_hnsw_search_knn(oracle, graph, qq, 10, 64, inv)
            hit += len(set(int(x) for x in got) & set(int(x) for x in labels[exact_topk(rows, qq, 10, metric)]))
        recall[name] = hit / (10 * len(queries))
    print("recall@10, ef = 64:", recall)
    assert abs(recall["batched"] - recall["seq"]) <= 0.02, recall
