"""CPU: the batch rule of level 1 as tests/hnsw_batch_model_l1.py restates it, the host members it stands on (HnswGraph::LinkUpper with a
first level, SetLevelLists), and the corpora of tests/test_gpu_hnsw_build_upper.py — each proven here to hold what its GPU case relies on
(level-1 re-selections, a hub past 256 entries, ...) before a card sees it."""
import numpy as np
import pytest

from . import hnsw_batch_model as bm
from . import hnsw_batch_model_l1 as bm1
from . import hnsw_l1_cases as cases
from .conftest import make_corpus
from .test_hnsw_builder import graph_invariants


def blocks_from(e, first_level):
    """The upper lists of the levels >= first_level, node by node."""
    off = e["upper_off"].astype(np.int64)
    return [e["upper"][off[i] + first_level - 1:off[i] + lv] for i, lv in enumerate(e["levels"]) if lv >= first_level]


def test_model_self_test(oracle):
    n, d, M, efc, seed = 1500, 24, 4, 40, 128
    rows = make_corpus(128, n, d)
    labels = cases.labels_of(n)
    seen = []
    g1, s1 = bm1.build_l1(oracle, 0, rows, labels, M, efc, seed=seed, on_batch=lambda a, cnt, before, touched, after: seen.append((a, cnt, before, touched)))
    g0, s0 = bm.build(oracle, 0, rows, labels, M, efc, seed=seed)
    graph_invariants(g1, n, M)
    assert np.array_equal(g1["levels"], g0["levels"]) and g1["entry"] == g0["entry"] and g1["maxlevel"] == g0["maxlevel"]
    assert np.array_equal(g1["upper_off"], g0["upper_off"])
    for x, y in zip(blocks_from(g1, 2), blocks_from(g0, 2)):      # the levels >= 2 read no level-1 list: the sequential build's
        assert np.array_equal(x, y)
    assert s1["batches"] == s0["batches"] == len(seen) and s1["seed"] == seed
    assert s1["reselected_l1"] > 0 and s1["batches_with_level2"] >= 1 and s1["l1_host_rows"] == 0
    assert s1["l1_rows"] == int((g1["levels"][seed:] >= 1).sum())
    # level 1 differs from the sequential build's somewhere (the rows of a batch do not see each other), level 0 follows the level-1 lists
    # its descent went through
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(blocks_from(g1, 1), blocks_from(g0, 1)))
    # under the rule the host touches no level-1 list: every node it reports has level >= 2
    for a, cnt, before, touched in seen:
        assert before["maxlevel"] >= 1 and (g1["levels"][touched] >= 2).all()
    # the rows of a batch do not see each other: a level-1 list names no other row of its own batch (later batches link back to it)
    l1 = cases.level1_lists(g1)
    for a, cnt, _, _ in seen:
        for i in range(a, a + cnt):
            ll = l1[i, 1:1 + l1[i, 0]]
            assert not ((ll >= a) & (ll < a + cnt)).any(), i


def test_a_graph_with_top_level_0_leaves_level_1_to_the_host(oracle):
    """A seed of 2 rows of level 0: the first batches have no level-1 node to start from — the host links their levels >= 1 as ever —
    and the rule takes over with the first batch whose graph has one."""
    n, d, M, efc = 700, 16, 16, 40
    rows = make_corpus(129, n, d)
    lv = cases.levels_of(0, rows, M, efc)
    assert lv[0] == 0 and lv[1] == 0 and (lv >= 1).sum() >= 10
    seen = []
    g1, s1 = bm1.build_l1(oracle, 0, rows, cases.labels_of(n), M, efc, seed=2, on_batch=lambda a, cnt, before, touched, after: seen.append((a, before["maxlevel"])))
    graph_invariants(g1, n, M)
    assert s1["l1_host_rows"] >= 1 and s1["l1_rows"] >= 1 and s1["l1_host_rows"] + s1["l1_rows"] == int((lv[2:] >= 1).sum())
    tops = [t for _, t in seen]
    assert tops[0] == 0 and tops == sorted(tops)                          # the top level only grows


def test_link_upper_from_level_2_and_set_level_lists():
    from reindexer_amd import hostapi
    n, d, M, efc = 2000, 24, 4, 40
    rows = make_corpus(130, n, d)
    labels = cases.labels_of(n)
    seq = hostapi.HnswGraph(0, d, n, M=M, ef_construction=efc)
    seq.add(rows, labels)
    s = seq.export()
    seq.close()
    g = hostapi.HnswGraph(0, d, n, M=M, ef_construction=efc)
    g.append_unlinked(rows, labels)
    g.link_stored(0, 200)
    assert g.export()["maxlevel"] >= 1
    touched = g.link_upper(200, n - 200, min_level=2)
    e = g.export()
    assert (e["levels"][touched] >= 2).all()
    assert e["entry"] == s["entry"] and e["maxlevel"] == s["maxlevel"] and np.array_equal(e["upper_off"], s["upper_off"])
    for x, y in zip(blocks_from(e, 2), blocks_from(s, 2)):
        assert np.array_equal(x, y)
    off = e["upper_off"].astype(np.int64)
    late = np.flatnonzero(e["levels"][200:] >= 1) + 200
    assert (e["upper"][off[late], 0] == 0).all()                         # level 1 of the later rows: untouched
    ids = np.flatnonzero(s["levels"] >= 1).astype(np.uint32)
    g.set_level_lists(1, ids, s["upper"][s["upper_off"][ids].astype(np.int64)])
    e = g.export()
    blocks = int(s["upper_off"][-1])
    assert np.array_equal(e["upper"][:blocks], s["upper"][:blocks])
    with pytest.raises(hostapi.HostError, match="does not reach the level"):
        g.set_level_lists(1, np.flatnonzero(s["levels"] == 0)[:1].astype(np.uint32), np.zeros((1, 1 + M), np.uint32))
    with pytest.raises(hostapi.HostError, match="longer than M"):
        g.set_level_lists(1, ids[:1], np.full((1, 1 + M), M + 1, np.uint32))
    g.close()


def test_map_corpora_hold_what_their_gpu_cases_rely_on(oracle):
    """tests/test_gpu_hnsw_build_upper_map.py: 3000 x 32, M = 8, efConstruction = 60 with a seed of 256 — level-1 rows by the hundred and
    level-1 re-selections — and its first 2000 rows with M = 16 and a seed of 4, whose first batches meet a graph of top level 0."""
    rows, labels = make_corpus(191, 3000, 32), cases.labels_of(3000)
    g, s = bm1.build_l1(oracle, 0, rows, labels, 8, 60, seed=256)
    assert s["l1_rows"] == int((g["levels"][256:] >= 1).sum()) > 100 and s["reselected_l1"] > 0 and s["l1_host_rows"] == 0, s["l1_rows"]
    assert int(g["levels"][256:].sum()) > 5 * 40                          # upper blocks of the batches: several attaches at 40 blocks of headroom
    lv = cases.levels_of(0, rows[:2000], 16, 60)
    assert (lv[:4] == 0).all()
    g, s = bm1.build_l1(oracle, 0, rows[:2000], labels[:2000], 16, 60, seed=4)
    assert s["l1_host_rows"] >= 1 and s["l1_rows"] >= 1 and s["l1_host_rows"] + s["l1_rows"] == int((lv[4:] >= 1).sum())


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_corpus_holds_what_its_gpu_case_relies_on(oracle, name):
    rows, hub, want, stats = cases.model_of(oracle, name)
    metric, n, d, M, efc, seed, ratio, have = cases.CASES[name]
    graph_invariants(want, n, M)
    print(name, {k: v for k, v in stats.items() if k != "first_export"})
    cases.check_conditions(name, hub, want, stats)
