#!/usr/bin/env python3
"""`WHERE cond AND KNN(...)` on an HNSW index until `needed` allowed rows are in hand, six ways on ONE graph (1M x 768 cosine, M = 16,
efC = 200, the graph of tools/bench_hnsw_filtered.py) at allowed shares 1.0 / 0.5 / 0.1 / 0.01, needed = 10, ef = first batch = 100, all
through the C-ABI with the filter as a bitmap:
  host_loop        the rule of csrc/hnsw_stream_collect_plan.h driven from the host over rxgpu_hnsw_stream_continue (a launch, two
                   synchronisations and three copies per batch) on a session begun outside the clock;
  collect          rxgpu_hnsw_stream_collect on a session begun outside the clock: the same rule in one device call — like for like with
                   host_loop;
  host_loop_full   rxgpu_hnsw_stream_begin + the host loop + _end, all inside the clock: what a caller without the feature pays per query;
  session_full     begin + collect + end inside the clock;
  one_shot         rxgpu_hnsw_collect_knn: Begin and the collection in one call on a leased search context — like for like with
                   host_loop_full;
  filtered         rxgpu_hnsw_search_knn_filtered, k = needed, ef as above: one call that fills ef allowed results.
The host loop is Python over the C-ABI (the Map's RXGPU_HNSW_COLLECT=host loop takes labels, and turning up to a million labels into a bitmap
per call would swamp every leg alike); its interpreter cost per batch is microseconds against calls of a millisecond and more.
One process, the legs alternating pass by pass; per leg ms per query (median of the passes and their range, host clock around calls that end
in a synchronise) and recall@10 against the exact answer among the allowed rows.  The five session legs must return identical rows and
distance bits: the run stops if they do not.
    python tools/bench_hnsw_collect.py [--rows 1000000] [--queries 64] [--build host|device] [--out profiles/hnsw_collect_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_hnsw import make_clustered  # noqa: E402
from reindexer_amd import capi, hostapi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--ef", type=int, default=100)
ap.add_argument("--needed", type=int, default=10)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--build", default="host", choices=["host", "device"])
ap.add_argument("--out", default=str(ROOT / "profiles" / "hnsw_collect_ab.json"))
a = ap.parse_args()
d, needed, ef = a.dim, a.needed, a.ef
corpus = make_clustered(a.rows + a.queries, d, 2000, 20261021, 0)
rows = corpus[:a.rows]
queries = np.stack([hostapi.normalize_copy(q)[0] for q in corpus[a.rows:]])
labels = np.arange(a.rows, dtype=np.uint64) << np.uint64(32)
if a.build == "device":
    os.environ["RXGPU_HNSW_BUILD"] = "device"
    os.environ["RXGPU_HNSW_BUILD_UPPER"] = "device"
m = hostapi.GpuHnswMap(2, d, a.rows, M=16, ef_construction=200, multithread=True)
t0 = time.perf_counter()
if a.build == "device":
    m.add_points(rows, labels)
    m.search_knn(queries[0], 10, ef)   # the first search links the stored rows
else:
    m.add(rows, labels, threads=16)
print("build s", round(time.perf_counter() - t0, 1), flush=True)
g = m.export_graph(with_views=True)
del corpus, rows
item_of_row = (np.asarray(g["labels"][:g["n"]]) >> np.uint64(32)).astype(np.int64)   # a concurrent build stores the points in its own order
ix = capi.VectorIndex(2, d, a.rows)
ix.upload_rows(0, g["vectors"], g["inv_norms"])
ix.hnsw_attach_graph(g)
L = capi.lib()
out = {"rows": a.rows, "dim": d, "metric": "cosine", "M": 16, "ef_construction": 200, "ef": ef, "first_batch": ef, "needed": needed, "queries": a.queries,
       "passes": a.passes, "build": a.build, "interface": "C-ABI, the filter as a bitmap", "shares": {}}


def cut(dist, row, ends):
    """each call's accepted rows ascending by (dist, item), calls concatenated, cut at needed -> (items, distance bits)"""
    items, bits_, at = [], [], 0
    for end in ends:
        it, ds = item_of_row[row[at:end]], dist[at:end]
        order = np.lexsort((it, ds))
        items += it[order].tolist()
        bits_ += ds[order].view(np.uint32).tolist()
        at = end
    return items[:needed], bits_[:needed]


rng = np.random.default_rng(7)
for share in (1.0, 0.5, 0.1, 0.01):
    allowed = np.ones(a.rows, bool) if share == 1.0 else rng.random(a.rows) < share   # by item (label >> 32): what `cond` let through
    allowed_row = allowed[item_of_row]
    ids = np.nonzero(allowed_row)[0].astype(np.uint32)
    words = np.zeros((a.rows + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    stats = {"calls": 0, "presented": 0, "launches": 0}

    def host_loop(qi, s):
        ds, rs, ends = [], [], []
        calls = presented = accepted = 0
        batch = ef
        while True:
            dist, row, exhausted = s.next(batch)
            ok = allowed_row[row]
            calls, presented, accepted = calls + 1, presented + len(row), accepted + int(np.count_nonzero(ok))
            ds.append(dist[ok]), rs.append(row[ok]), ends.append(accepted)
            if accepted >= needed or exhausted or calls >= 1000:
                break
            batch = int(L.rxgpu_hnsw_stream_collect_batch(accepted, presented, needed))
        return cut(np.concatenate(ds), np.concatenate(rs), ends)

    def collect(qi, s):
        r = s.collect(words, needed, ef)
        stats["calls"] += len(r["calls"])
        stats["presented"] += r["presented"]
        stats["launches"] += r["launches"]
        return cut(r["dist"], r["row"], r["calls"][:, 2].tolist())

    def host_loop_full(qi, _s=None):
        with ix.hnsw_stream(queries[qi], ef) as s:
            return host_loop(qi, s)

    def session_full(qi, _s=None):
        with ix.hnsw_stream(queries[qi], ef) as s:
            r = s.collect(words, needed, ef)
        return cut(r["dist"], r["row"], r["calls"][:, 2].tolist())

    def one_shot(qi, _s=None):
        r = ix.hnsw_collect_knn(queries[qi], ef, words, needed, ef)
        return cut(r["dist"], r["row"], r["calls"][:, 2].tolist())

    def filtered(qi, _s=None):
        dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries[qi:qi + 1], needed, ef, words)
        return item_of_row[row[0, :int(cnt[0])]].tolist(), None

    truth = []
    for qi in range(len(queries)):
        dist, row, cnt = ix.search_knn_subset(queries[qi:qi + 1], needed, ids)
        truth.append(item_of_row[row[0, :int(cnt[0])]].tolist())
    legs = {"host_loop": host_loop, "collect": collect, "host_loop_full": host_loop_full, "session_full": session_full, "one_shot": one_shot,
            "filtered": filtered}
    begun = ("host_loop", "collect")
    per = {name: [] for name in legs}
    res = {}
    for p in range(a.passes + 1):   # pass 0 warms up and is not counted
        for name, fn in legs.items():
            sessions = [ix.hnsw_stream(q, ef) for q in queries] if name in begun else [None] * len(queries)
            t0 = time.perf_counter()
            res[name] = [fn(qi, sessions[qi]) for qi in range(len(queries))]
            ms = (time.perf_counter() - t0) / len(queries) * 1e3
            for s in sessions:
                if s is not None:
                    s.close()
            if p:
                per[name].append(ms)
    if not (res["host_loop"] == res["collect"] == res["host_loop_full"] == res["session_full"] == res["one_shot"]):
        raise SystemExit(f"share {share}: the session legs differ")
    n_coll = (a.passes + 1) * len(queries)
    entry = {"allowed_rows": int(ids.size), "identical_rows_and_distance_bits": True,
             "calls_per_query": stats["calls"] / n_coll, "presented_per_query": stats["presented"] / n_coll, "launches_per_query": stats["launches"] / n_coll}
    for name in legs:
        got = [r[0] for r in res[name]]
        entry[name] = {"ms_median": statistics.median(per[name]), "ms_min": min(per[name]), "ms_max": max(per[name]),
                       "recall_at_10": sum(len(set(r) & set(t)) for r, t in zip(got, truth)) / max(1, sum(len(t) for t in truth))}
    for name, base in (("collect", "host_loop"), ("session_full", "host_loop_full"), ("one_shot", "host_loop_full")):
        entry[name + "_over_" + base] = {"median": entry[name]["ms_median"] / entry[base]["ms_median"],
                                         "best_case": entry[name]["ms_min"] / entry[base]["ms_max"],
                                         "worst_case": entry[name]["ms_max"] / entry[base]["ms_min"],
                                         "ranges_overlap": not (entry[name]["ms_max"] < entry[base]["ms_min"] or entry[base]["ms_max"] < entry[name]["ms_min"])}
    out["shares"][str(share)] = entry
    print(share, json.dumps(entry), flush=True)
ix.close()
m.close()
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
