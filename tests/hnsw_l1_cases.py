"""The corpora of the level-1 device build's tests, and what each has to show — defined once, so that tests/test_hnsw_batch_model_l1.py
proves the conditions on the CPU (over tests/hnsw_batch_model_l1.py) before tests/test_gpu_hnsw_build_upper.py lets a card see them.
Not a test module."""
import numpy as np

from . import hnsw_batch_model_l1 as bm1
from .conftest import make_corpus


def labels_of(n):
    return np.arange(n, dtype=np.uint64) << np.uint64(32)


def levels_of(metric, rows, M, efc):
    """The levels the builder draws for these rows: they depend on the row order (and M) alone, so a throwaway graph tells them."""
    from reindexer_amd import hostapi
    g = hostapi.HnswGraph(metric, rows.shape[1], rows.shape[0], M=M, ef_construction=efc)
    g.append_unlinked(rows, labels_of(rows.shape[0]))
    lv = g.export()["levels"].copy()
    g.close()
    return lv


def first_with_level(levels, below, at_least=1):
    return int(np.flatnonzero(levels[:below] >= at_least)[0])


# name: (metric, n, d, M, efc, seed, ratio, rows already in a host-built graph)
CASES = {
    "general_l2": (0, 3000, 48, 4, 40, 256, 16, 0),
    "general_ip": (1, 3000, 48, 4, 40, 256, 16, 0),
    "general_cos": (2, 3000, 48, 4, 40, 256, 16, 0),
    "cos768": (2, 1500, 768, 16, 200, 1024, 16, 0),
    "rows1024": (2, 1400, 1024, 16, 100, 1024, 16, 0),
    "padded": (0, 1000, 50, 4, 8, 64, 2, 0),
    "ties_hub": (0, 600, 32, 4, 50, 64, 16, 0),
    "hub_past_cap": (0, 2600, 32, 4, 50, 1300, 1, 0),
    "append": (0, 3000, 40, 6, 60, 1024, 16, 2000),
}
CORPUS_SEED = dict(general_l2=177, general_ip=177, general_cos=177, cos768=178, rows1024=184, padded=179, ties_hub=181, hub_past_cap=182, append=183)
TIES_BATCH = (320, 384)        # ties_hub: the batch [320, 384) (a = 320: 320 // 16 = 20 < 64 rows, so 64) is all copies of one row
HUB_COPIES = (1300, 2500)      # hub_past_cap: 1200 rows of the one batch [1300, 2600) are copies of one row


def rows_of(name):
    metric, n, d, M, efc, seed, ratio, have = CASES[name]
    rows = make_corpus(CORPUS_SEED[name], n, d)
    hub = None
    if name == "ties_hub":
        hub = first_with_level(levels_of(metric, rows, M, efc), 64)
        rows[TIES_BATCH[0]:TIES_BATCH[1]] = rows[hub]
    elif name == "hub_past_cap":
        hub = first_with_level(levels_of(metric, rows, M, efc), 1300)
        rows[HUB_COPIES[0]:HUB_COPIES[1]] = rows[hub]
    return rows, hub


def host_graph(name, rows):
    """append: the graph the host built over the first rows; None elsewhere."""
    from reindexer_amd import hostapi
    metric, n, d, M, efc, seed, ratio, have = CASES[name]
    if not have:
        return None
    g = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    g.add(rows[:have], labels_of(n)[:have])
    return g


def model_of(orc, name, on_batch=None):
    """(rows, hub row or None, finished export, statistics) of build_l1 over the case."""
    metric, n, d, M, efc, seed, ratio, have = CASES[name]
    rows, hub = rows_of(name)
    g = host_graph(name, rows)
    want, stats = bm1.build_l1(orc, metric, rows, labels_of(n), M, efc, seed=seed, ratio=ratio, graph=g, on_batch=on_batch)
    if g is not None:
        g.close()
    return rows, hub, want, stats


def level1_lists(e):
    """[n][1 + M]: the level-1 list of every node, an empty list where it has level 0 — what rxgpu_hnsw_read_level(1) returns."""
    out = np.zeros((e["n"], 1 + e["M"]), np.uint32)
    has = np.flatnonzero(e["levels"] >= 1)
    out[has] = e["upper"][e["upper_off"][has].astype(np.int64)]
    return out


def check_conditions(name, hub, want, stats):
    """What the GPU case of this name relies on; a corpus that misses one is changed, the condition is not."""
    metric, n, d, M, efc, seed, ratio, have = CASES[name]
    lv = want["levels"]
    assert stats["l1_rows"] > 0 and stats["l1_batches"] > 0, stats
    if name.startswith("general"):
        assert 650 <= int((lv >= 1).sum()) <= 850 and 140 <= int((lv >= 2).sum()) <= 240, ((lv >= 1).sum(), (lv >= 2).sum())
        assert stats["reselected_l1"] > 50 and stats["batches_with_level2"] >= 1 and stats["l1_host_rows"] == 0, stats
    elif name == "cos768":
        assert (1 + M) * d * 4 + (3 * 256 + 4 * 128) * 4 <= 64 * 1024      # hnsw_build_select_lds: the kept rows fit in LDS
        assert stats["l1_rows"] == int((lv[1024:] >= 1).sum()) >= 10, stats
    elif name == "rows1024":
        assert (1 + M) * d * 4 + (3 * 256 + 4 * 128) * 4 > 64 * 1024       # hnsw_build_select_lds: the kept rows do not fit in LDS, they are read from L2
        assert stats["l1_rows"] == int((lv[1024:] >= 1).sum()) >= 10, stats
    elif name == "padded":
        assert d % 4 and stats["reselected_l1"] > 30, stats
    elif name == "ties_hub":
        a, b = TIES_BATCH
        assert lv[hub] >= 1 and int((lv[a:b] >= 1).sum()) > M, (hub, lv[hub], (lv[a:b] >= 1).sum())
        assert stats["reselected_l1"] >= 1, stats
    elif name == "hub_past_cap":
        a, b = HUB_COPIES
        assert lv[hub] >= 1 and int((lv[a:b] >= 1).sum()) > 256, (hub, (lv[a:b] >= 1).sum())
        assert stats["past_cap_l1"] >= 1, stats
    elif name == "append":
        assert stats["seed"] == have and stats["l1_rows"] == int((lv[have:] >= 1).sum()) > 50, stats
