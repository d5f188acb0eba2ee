"""-m gpu: HNSW level 1 built on the device under the batch rule (hnsw_build_upper.hip and the kernels of hnsw_build.hip on the dense
level-1 view, through rxgpu_hnsw_link_batch_upper / rxgpu_hnsw_patch_upper_from).

Bar: the rule is deterministic given the rows and their order, so the device's lists equal the lists of the Python restatement
(tests/hnsw_batch_model_l1.py) LINK FOR LINK — the whole level-0 array AND every level-1 list (rxgpu_hnsw_read_level), the statistics of
both levels, and four restated searches on the finished mirror.  The corpora and what each has to show are tests/hnsw_l1_cases.py; the
conditions are asserted on the CPU by tests/test_hnsw_batch_model_l1.py and once more here on the model's statistics."""
import numpy as np
import pytest

from . import hnsw_batch_model as bm
from . import hnsw_l1_cases as cases
from .conftest import make_corpus

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def upper_patch(after, touched, a, cnt, first_level):
    """(ids, levels, staged blocks) of one patch: the older nodes the host touched, then every node of the batch; the blocks of the levels
    >= first_level."""
    ids = np.concatenate([touched[touched < a].astype(np.uint32), np.arange(a, a + cnt, dtype=np.uint32)])
    levels = after["levels"][ids].astype(np.int32)
    off = after["upper_off"].astype(np.int64)
    blocks = [after["upper"][off[i] + first_level - 1:off[i] + lv].reshape(-1) for i, lv in zip(ids, levels) if lv >= first_level]
    return ids, levels, np.concatenate(blocks) if blocks else np.empty(0, np.uint32)


def assert_link_for_link(want, got, what):
    if not np.array_equal(want, got):
        bad = np.flatnonzero((want != got).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {want.shape[0]} lists differ; first: node {bad[0]}\n model  {want[bad[0]]}\n device {got[bad[0]]}")


def device_against_model(rxgpu, oracle, name):
    """The model over the case, its batches recorded; then the same batches through the C-ABI, level 1 on the device wherever the rule
    puts it there.  Asserts the bar; returns (finished export, model statistics, level-0 device statistics, level-1 device statistics)."""
    from oracle.pyoracle import oracle_hnsw_search_knn
    metric, n, d, M, efc, seed, ratio, have = cases.CASES[name]
    recorded = []
    rows, hub, want, stats = cases.model_of(oracle, name, on_batch=lambda a, cnt, before, touched, after: recorded.append((a, cnt, before["maxlevel"], touched, after)))
    cases.check_conditions(name, hub, want, stats)
    first, L = stats["first_export"], stats["seed"]
    inv = want["inv_norms"]
    with rxgpu.VectorIndex(metric, d, n) as ix:
        ix.upload_rows(0, rows[:L], inv[:L] if inv is not None else None)
        ix.hnsw_attach_graph(bm.search_graph(first, L, rows) | dict(labels=first["labels"][:L]))
        ix.upload_rows(L, rows[L:], inv[L:] if inv is not None else None)
        device_rows = 0
        for a, cnt, top, touched, after in recorded:
            ix.hnsw_link_batch(a, cnt, efc)
            U = np.flatnonzero(after["levels"][a:a + cnt] >= 1).astype(np.uint32) + np.uint32(a)
            if top >= 1 and U.size:
                ix.hnsw_link_batch_upper(a, cnt, U, efc)
                assert_link_for_link(cases.level1_lists(after)[U], ix.hnsw_read_level(1, U, M), f"batch {a}: level 1 of its rows before the patch")
                ix.hnsw_patch_upper_from(2, *upper_patch(after, touched, a, cnt, 2), after["maxlevel"], after["entry"])
                device_rows += U.size
            else:
                ix.hnsw_patch_upper(*upper_patch(after, touched, a, cnt, 1), after["maxlevel"], after["entry"])
        assert device_rows == stats["l1_rows"]
        everyone = np.arange(n, dtype=np.uint32)
        assert_link_for_link(want["links0"], ix.hnsw_read_links0(0, n, want["maxM0"]), "level 0")
        assert_link_for_link(cases.level1_lists(want), ix.hnsw_read_level(1, everyone, M), "level 1")
        off = want["upper_off"].astype(np.int64)
        for lv in range(2, want["maxlevel"] + 1):                     # the host's levels arrive beside the device's level 1
            ids = np.flatnonzero(want["levels"] >= lv).astype(np.uint32)
            assert_link_for_link(want["upper"][off[ids] + lv - 1], ix.hnsw_read_level(lv, ids, M), f"level {lv}")
        d0, d1 = ix.hnsw_read_build_stats(), ix.hnsw_read_build_upper_stats()
        assert d0["rows"] == n - L and d0["batches"] == stats["batches"] and d0["reselected"] == stats["reselected"], (d0, stats["reselected"])
        assert d1["rows"] == stats["l1_rows"] and d1["reselected"] == stats["reselected_l1"] and d1["past_cap"] == stats["past_cap_l1"], (
            d1, {k: v for k, v in stats.items() if k != "first_export"})
        assert ix.hnsw_read_build_upper_stats()["rows"] == 0          # taken
        ix.hnsw_release_build_view()
        for qi in range(4):                                           # the finished mirror answers searches like the restated engine
            q = make_corpus(4000 + qi, 1, d)[0]
            if metric == 2:
                q, _ = oracle.normalize_copy(q)
            wd, wl = oracle_hnsw_search_knn(oracle, want, q, 10, 64, inv)
            dist, row, cnt_ = ix.hnsw_search_knn(q, 10, 64)
            c = int(cnt_[0])
            order = np.lexsort((row[0, :c], dist[0, :c]))
            assert np.array_equal(want["labels"][row[0, :c][order]], wl) and np.array_equal(bits(dist[0, :c][order]), bits(wd)), qi
    return want, stats, d0, d1


@pytest.mark.parametrize("name", ["general_l2", "general_ip", "general_cos"])
def test_general_path_link_for_link(rxgpu, oracle, name):
    want, stats, d0, d1 = device_against_model(rxgpu, oracle, name)
    assert d1["reselected"] == stats["reselected_l1"] > 50 and d1["past_cap"] == 0
    assert 650 <= int((want["levels"] >= 1).sum()) <= 850 and 140 <= int((want["levels"] >= 2).sum()) <= 240


def test_768_cosine_kept_rows_in_lds(rxgpu, oracle):
    device_against_model(rxgpu, oracle, "cos768")


def test_1024_float_rows_kept_rows_from_l2(rxgpu, oracle):
    """17 rows of 1024 floats do not fit in LDS: the level-1 selection reads its kept rows from L2, and the level-1 search runs over the
    wide-row kernels"""
    device_against_model(rxgpu, oracle, "rows1024")


def test_padded_stride_nearly_everything_reselected(rxgpu, oracle):
    """D = 50: a row stride of 52 floats.  M = 4, efConstruction = 8, batches half the size of the graph they search: nearly every touched
    level-1 node overflows its 4 slots and is re-selected."""
    want, stats, d0, d1 = device_against_model(rxgpu, oracle, "padded")
    assert d1["reselected"] > 30


def test_equal_distances_and_a_hub_on_level_1(rxgpu, oracle):
    """The batch [320, 384) is 64 copies of a seed row of level >= 1: those of them with level >= 1 all find it at distance 0 on level 1,
    and among equal distances the id order of selectNeighbors decides."""
    want, stats, d0, d1 = device_against_model(rxgpu, oracle, "ties_hub")
    assert d1["reselected"] >= 1 and d1["past_cap"] == 0


def test_a_hub_past_the_kernels_cap_on_level_1_is_finished_not_truncated(rxgpu, oracle):
    """1200 rows of the one batch are copies of a seed row of level >= 1: more than 256 of them have level >= 1 and arrive at the hub's
    level-1 list at once — the second launch re-selects it."""
    want, stats, d0, d1 = device_against_model(rxgpu, oracle, "hub_past_cap")
    assert d1["past_cap"] >= 1


def test_appending_to_a_host_built_graph(rxgpu, oracle):
    want, stats, d0, d1 = device_against_model(rxgpu, oracle, "append")
    assert d0["rows"] == 1000


def test_link_batch_upper_refuses_what_it_does_not_take(rxgpu, oracle):
    from reindexer_amd import hostapi
    n, d, M, efc = 400, 16, 4, 40
    rows = make_corpus(184, n, d)
    labels = cases.labels_of(n)
    g = hostapi.HnswGraph(0, d, n, M=M, ef_construction=efc)
    g.add(rows[:300], labels[:300])
    e = g.export()
    e["vectors"] = rows
    g.append_unlinked(rows[300:], labels[300:])
    g.link_upper(300, 50, min_level=2)
    after = g.export()
    g.close()
    assert e["maxlevel"] >= 1
    U = np.flatnonzero(after["levels"][300:350] >= 1).astype(np.uint32) + np.uint32(300)
    assert U.size >= 3

    def refused(ix, code, *args):
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.hnsw_link_batch_upper(*args)
        assert err.value.code == code, (err.value, args)

    with rxgpu.VectorIndex(0, d, n) as ix:
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(e)
        ix.upload_rows(300, rows[300:], None)
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, U, efc)                      # before the level-0 batch
        ix.hnsw_link_batch(300, 50, efc)
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, np.append(U, 350), efc)      # a row outside the batch
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, np.append(299, U), efc)
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, U[::-1], efc)                # not ascending
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, np.append(U[:1], U), efc)    # a row twice
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, U, 257)                      # efConstruction past the kernel's arrays
        with pytest.raises(rxgpu.RxGpuError) as err:                              # level 1 of the new nodes was not built: no patch from level 2
            ix.hnsw_patch_upper_from(2, *upper_patch(after, np.empty(0, np.uint32), 300, 50, 2), after["maxlevel"], after["entry"])
        assert err.value.code == rxgpu.RXGPU_ERR_LOGIC
        ix.hnsw_link_batch_upper(300, 50, U, efc)
        refused(ix, rxgpu.RXGPU_ERR_LOGIC, 300, 50, U, efc)                       # twice
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.hnsw_release_build_view()                                          # the lists of U wait there
        assert err.value.code == rxgpu.RXGPU_ERR_LOGIC
        ix.hnsw_patch_upper_from(2, *upper_patch(after, np.empty(0, np.uint32), 300, 50, 2), after["maxlevel"], after["entry"])
        refused(ix, rxgpu.RXGPU_ERR_LOGIC, 300, 50, U, efc)                       # after the patch
        assert (ix.hnsw_read_level(1, U, M)[:, 0] >= 1).all()
        with pytest.raises(rxgpu.RxGpuError) as err:
            ix.hnsw_read_level(1, np.array([350], np.uint32), M)                  # not a node yet
        assert err.value.code == rxgpu.RXGPU_ERR_PARAMS
        ix.hnsw_release_build_view()
    flat = dict(e, maxlevel=0, upper_off=np.zeros(301, np.uint64), upper=np.zeros((1, 1 + M), np.uint32), entry=0)
    with rxgpu.VectorIndex(0, d, n) as ix:                                        # a graph whose top level is 0
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(flat)
        ix.upload_rows(300, rows[300:], None)
        ix.hnsw_link_batch(300, 50, efc)
        refused(ix, rxgpu.RXGPU_ERR_LOGIC, 300, 50, U, efc)
    with rxgpu.VectorIndex(0, d, n) as ix:                                        # a node deleted between level 0 and level 1 of the batch
        ix.upload_rows(0, rows[:300], None)
        ix.hnsw_attach_graph(e)
        ix.upload_rows(300, rows[300:], None)
        ix.hnsw_link_batch(300, 50, efc)
        flags = np.zeros(350, np.uint8)
        flags[7] = 1
        ix.hnsw_update_deleted(flags, 1)
        refused(ix, rxgpu.RXGPU_ERR_PARAMS, 300, 50, U, efc)
    with rxgpu.ShardedVectorIndex(0, d, n, [0, 0]) as sx:                         # a sharded index
        refused(sx, rxgpu.RXGPU_ERR_LOGIC, 300, 50, U, efc)
