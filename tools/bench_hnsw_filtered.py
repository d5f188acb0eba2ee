#!/usr/bin/env python3
"""`WHERE cond AND KNN(...)` on an HNSW index, three ways on ONE graph (1M x 768 cosine, M = 16, efC = 200, ef = 128, k = 10) at allowed
shares 1.0 / 0.5 / 0.1 / 0.01:
  filtered   rxgpu_hnsw_search_knn_filtered: one device call under the allowed-rows bitmap;
  streaming  what a caller does without it: a streaming session continued, batch by batch, until k allowed rows are in hand;
  subset     rxgpu_search_knn_subset over the allowed rows (the exact answer; what the Map takes for very selective filters).
Per leg: ms per query (median of 5 passes and their range); for the filtered call also distance evaluations, hops and the searches handed
to the heaps (rxgpu_hnsw_read_tie_reruns) per query; recall@10 of every leg against the exact answer among the allowed rows.
    python tools/bench_hnsw_filtered.py [--rows 1000000] [--queries 64] [--build host|device] [--out profiles/hnsw_filtered_ab.json]
--build device links the graph on the device in batches (RXGPU_HNSW_BUILD=device, RXGPU_HNSW_BUILD_UPPER=device: seconds instead of a
minute for a million rows); every leg searches the one graph either way."""
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
ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--stream-batch", type=int, default=32)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--build", default="host", choices=["host", "device"])
ap.add_argument("--out", default=str(ROOT / "profiles" / "hnsw_filtered_ab.json"))
a = ap.parse_args()
d, k, ef = a.dim, 10, a.ef
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
    m.search_knn(queries[0], k, ef)   # the first search links the stored rows
else:
    m.add(rows, labels, threads=16)
print("build s", round(time.perf_counter() - t0, 1), flush=True)
g = m.export_graph(with_views=True)
del corpus, rows
item_of_row = (np.asarray(g["labels"][:g["n"]]) >> np.uint64(32)).astype(np.int64)   # a concurrent build stores the points in its own order
ix = capi.VectorIndex(2, d, a.rows)
ix.upload_rows(0, g["vectors"], g["inv_norms"])
ix.hnsw_attach_graph(g)
out = {"rows": a.rows, "dim": d, "metric": "cosine", "M": 16, "ef_construction": 200, "ef": ef, "k": k, "queries": a.queries, "stream_batch": a.stream_batch,
       "build": a.build, "shares": {}}


def timed(fn):
    """ms per query of `passes` passes over the queries: median, min, max; the last pass's answers"""
    per, res = [], None
    for _ in range(a.passes):
        t0 = time.perf_counter()
        res = [fn(qi) for qi in range(len(queries))]
        per.append((time.perf_counter() - t0) / len(queries) * 1e3)
    return {"ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}, res


def recall(res, truth):
    return sum(len(set(r) & set(t)) for r, t in zip(res, truth)) / max(1, sum(len(t) for t in truth))


rng = np.random.default_rng(7)
for share in (1.0, 0.5, 0.1, 0.01):
    allowed = np.ones(a.rows, bool) if share == 1.0 else rng.random(a.rows) < share   # by item (label >> 32): what `cond` let through
    ids = np.nonzero(allowed[item_of_row])[0].astype(np.uint32)                          # ... as internal rows
    words = np.zeros((a.rows + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))

    def filtered(qi):
        dist, row, cnt, _ = ix.hnsw_search_knn_filtered(queries[qi:qi + 1], k, ef, words)
        return item_of_row[row[0, :int(cnt[0])]].tolist()

    def streaming(qi):
        have = []
        s = m.stream(queries[qi], ef)
        try:
            while len(have) < k:
                dist, lab, exhausted = s.next(a.stream_batch)
                have += [(float(x), int(y) >> 32) for x, y in zip(dist, lab) if allowed[int(y) >> 32]]
                if exhausted:
                    break
        finally:
            s.close()
        return [item for _, item in sorted(have)[:k]]   # the k nearest of the allowed rows the session delivered

    def subset(qi):
        dist, row, cnt = ix.search_knn_subset(queries[qi:qi + 1], k, ids)
        return item_of_row[row[0, :int(cnt[0])]].tolist()

    exact_t, truth = timed(subset)
    filtered(0)
    ix.hnsw_read_stats()
    ix.hnsw_read_tie_reruns()
    filt_t, filt = timed(filtered)
    reruns = ix.hnsw_read_tie_reruns()   # (first: reading the evaluations and hops resets the kernels' restart counter with them)
    evals, hops = ix.hnsw_read_stats()
    calls = a.passes * len(queries)
    stream_t, stream = timed(streaming)
    out["shares"][str(share)] = {
        "allowed_rows": int(ids.size),
        "filtered": {**filt_t, "evals_per_query": evals / calls, "hops_per_query": hops / calls, "heap_reruns_per_query": reruns / calls, "recall_at_10": recall(filt, truth)},
        "streaming": {**stream_t, "recall_at_10": recall(stream, truth)},
        "subset": {**exact_t, "recall_at_10": 1.0},
    }
    print(share, json.dumps(out["shares"][str(share)]), flush=True)
ix.close()
m.close()
print(json.dumps(out))
if a.out:
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
