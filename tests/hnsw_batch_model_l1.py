"""The batch rule of the device build of HNSW level 1 (reindexer_amd/csrc/hnsw_build_plan.h) restated in Python on top of
tests/hnsw_batch_model.py — the checker of rxgpu_hnsw_link_batch_upper, link for link.  Not a test module.

For a batch [a, b) over G-, the graph of the nodes < a as it stood after the batch before, and U, the rows of the batch with level >= 1:
  * level 0 of the batch is hnsw_batch_model.link_batch as it is — its searches descend through G-, so it runs before the batch changes a
    level-1 list;
  * where G- has a top level >= 1 and U is not empty, level 1 of the batch follows the same rule one level up: the candidates of a row of
    U are the oracle's restated SearchKnn with k = ef = efConstruction on a SHIFTED copy of G- — links0 = the level-1 lists padded to
    1 + maxM0, the levels >= 2 renumbered down by one, the top level one lower, the same entry point — so its descent is the greedy one
    from G-'s entry point through the levels >= 2 and its base-layer search runs over the level-1 lists.  That holds for the rows of level
    >= 2 too.  The list of the row is BatchModel.select with limit M; a target's incoming rows are appended ascending while
    len(cur) + len(inc) <= M, else the list is re-selected ONCE over cur + inc on distIds(x, t) with limit M;
  * the levels >= 2 of the batch's rows, the entry point and the top level are the host builder's (link_upper(first, n, min_level=2));
  * a batch whose G- has top level 0 has no level-1 node to start from: the host links its levels >= 1 as ever.
"""
import numpy as np

from . import hnsw_batch_model as bm

ENTRIES = 256   # kHnswBuildEntries: what one wavefront orders in LDS; a node with more entries is finished by the second launch


def level1_graph(e, a, rows):
    """The shifted copy of the export e cut to its first a nodes: level 1 as the base layer."""
    M, max_m0 = e["M"], e["maxM0"]
    lv = e["levels"][:a].astype(np.int64)
    off = e["upper_off"].astype(np.int64)
    links0 = np.zeros((a, 1 + max_m0), np.uint32)
    has = np.flatnonzero(lv >= 1)
    links0[has, :1 + M] = e["upper"][off[has]]
    new_lv = np.maximum(lv - 1, 0)
    new_off = np.zeros(a + 1, np.uint64)
    new_off[1:] = np.cumsum(new_lv)
    upper = np.zeros((max(int(new_off[-1]), 1), 1 + M), np.uint32)
    for i in np.flatnonzero(lv >= 2):
        upper[int(new_off[i]):int(new_off[i + 1])] = e["upper"][off[i] + 1:off[i] + lv[i]]
    g = dict(e)
    g.update(n=a, links0=links0, upper_off=new_off, upper=upper, levels=new_lv.astype(np.int32), labels=np.arange(a, dtype=np.uint64),
             deleted=np.ascontiguousarray(e["deleted"][:a]), vectors=rows, maxlevel=e["maxlevel"] - 1)
    return g


def upper_rows_of(e, a, cnt):
    """U: the rows of the batch [a, a + cnt) with level >= 1, ascending."""
    return [i for i in range(a, a + cnt) if e["levels"][i] >= 1]


def link_batch_l1(model, orc, e, a, cnt, M, efc):
    """Level 1 of the batch on the export e in front of it.  Returns ({node: its new level-1 list}, re-selected nodes, nodes past ENTRIES)."""
    from oracle.pyoracle import oracle_hnsw_search_knn
    g = level1_graph(e, a, model.rows)
    inv = np.ascontiguousarray(model.inv[:a]) if model.metric == 2 else None
    off = e["upper_off"]
    lists, incoming = {}, {}
    for i in upper_rows_of(e, a, cnt):
        _, cand = oracle_hnsw_search_knn(orc, g, model.rows[i], min(efc, a), efc, inv)
        cand = cand.astype(np.int64)
        chosen = model.select(cand, model.dist_from(i, cand), M)
        lists[i] = chosen
        for t in chosen:
            incoming.setdefault(t, []).append(i)
    reselected = past = 0
    for t, inc in incoming.items():
        row = e["upper"][int(off[t])]
        cur = [int(x) for x in row[1:1 + int(row[0])]]
        inc = sorted(inc)
        if len(cur) + len(inc) <= M:
            lists[t] = cur + inc
            continue
        reselected += 1
        past += len(cur) + len(inc) > ENTRIES
        ids = np.array(cur + inc, np.int64)
        lists[t] = model.select(ids, model.dist_to(ids, t), M)
    return lists, reselected, past


def list_rows(lists, ids, M):
    out = np.zeros((len(ids), 1 + M), np.uint32)
    for j, i in enumerate(ids):
        out[j, 0] = len(lists[i])
        out[j, 1:1 + len(lists[i])] = lists[i]
    return out


def build_l1(orc, metric, rows, labels, M, efc, seed=bm.SEED, ratio=bm.RATIO, cap=bm.BATCH_CAP, graph=None, on_batch=None):
    """hnsw_batch_model.build with level 1 under the batch rule.  on_batch(a, cnt, export_before, touched_upper, export_after) as there;
    touched_upper are the nodes whose lists the HOST changed (levels >= 2 of a batch whose level 1 the rule links, levels >= 1 otherwise).
    Returns (export of the finished graph, statistics) — level 1 counted separately: l1_rows / l1_host_rows (rows of level >= 1 linked under
    the rule / by the host), reselected_l1, past_cap_l1, l1_batches, batches_with_level2 (rule-linked batches that hold a row of level >= 2)."""
    from reindexer_amd import hostapi
    n, d = rows.shape
    g = graph if graph is not None else hostapi.HnswGraph(metric, d, n, M=M, ef_construction=efc)
    have = g.pending_from
    g.append_unlinked(rows[have:], labels[have:])
    L = have
    if L < seed:
        s = min(seed, n) - L
        g.link_stored(L, s)
        L += s
    vec, inv = g.vector_views(n)
    model = bm.BatchModel(orc, metric, rows, inv)
    e = g.export()
    links0 = e["links0"].copy()
    stats = dict(batches=0, reselected=0, seed=L, first_export=e, l1_rows=0, l1_host_rows=0, reselected_l1=0, past_cap_l1=0, l1_batches=0,
                 batches_with_level2=0)
    while L < n:
        cnt = bm.batch_rows(L, n, ratio, cap)
        stats["reselected"] += bm.link_batch(model, orc, e, links0, L, cnt, e["M"], e["maxM0"], efc)
        U = upper_rows_of(e, L, cnt)
        if e["maxlevel"] >= 1 and U:
            lists, resel, past = link_batch_l1(model, orc, e, L, cnt, e["M"], efc)
            touched = g.link_upper(L, cnt, min_level=2)
            ids = sorted(lists)
            g.set_level_lists(1, ids, list_rows(lists, ids, e["M"]))
            stats["l1_rows"] += len(U)
            stats["reselected_l1"] += resel
            stats["past_cap_l1"] += past
            stats["l1_batches"] += 1
            stats["batches_with_level2"] += bool((e["levels"][U] >= 2).any())
        else:
            touched = g.link_upper(L, cnt)
            stats["l1_host_rows"] += len(U)
        after = g.export()
        if on_batch is not None:
            on_batch(L, cnt, e, touched, after)
        e = after
        stats["batches"] += 1
        L += cnt
    g.set_links0(0, links0)
    out = g.export()
    out["vectors"] = rows
    out["inv_norms"] = None if inv is None else np.array(inv)
    if graph is None:
        g.close()
    return out, stats
