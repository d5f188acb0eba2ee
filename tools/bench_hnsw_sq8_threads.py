#!/usr/bin/env python3
"""The planner's call shape over a QUANTISED Map: T threads, one SearchKnn each, through GpuHnswMap::SearchKnn on an SQ8 graph.

    python tools/bench_hnsw_sq8_threads.py --rows 1000000 --dim 768 [--save-graph g.bin | --graph g.bin] [--out profiles/sq8_server_threads.json]

Builds the graph on this box (or loads the Map's own index cache written by --save-graph over the same corpus: same --rows / --dim / --seed),
quantises the Map with the reference's sampler (GpuHnswMap::Quantize(config), what HnswIndexBase::Quantize() calls) and measures, once with the
resident kernel over codes (the mailbox, rxgpu_hnsw_server.hip) and once with RXGPU_HNSW_SERVER_SQ8=0 (a launch per query, what a quantised Map
did before the mailbox over codes existed):
  * single-query latency (64 calls from one thread, after warm-up);
  * T = 1 / 16 / 64 / 256 native threads through search_knn_norm_mt: queries/s, how many the mailbox answered (`posted`) and, from
    rxgpu_hnsw_server_times, the mean duration of a posted search on the device and from the request's store to the answer seen by the caller.
--repeat N runs the whole set of legs N times (the run-to-run spread)."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_hnsw import make_clustered, server_times  # noqa: E402
from reindexer_amd import capi, hostapi  # noqa: E402


def legs(m, queries, norms, o) -> dict:
    """One set of legs in the current environment."""
    nr = norms if norms is not None else np.ones(queries.shape[0], np.float32)
    for i in range(5):   # the first search mirrors graph and code table into HBM; the next ones launch the resident kernel's first generation
        m.search_knn_norm(queries[i], o.k, o.ef, None if norms is None else float(norms[i]))
    t0 = time.perf_counter()
    for i in range(5, 69):
        m.search_knn_norm(queries[i], o.k, o.ef, None if norms is None else float(norms[i]))
    out = {"single_query_latency_ms": (time.perf_counter() - t0) / 64 * 1e3, "threads": []}
    for T in o.threads:
        m.search_knn_norm_mt(queries, nr, o.k, o.ef, T, 2, 10.0)   # warm-up: contexts and buffers of T concurrent callers
        p0, tm0 = m.posted_queries(), server_times(m)
        secs, done, _ = m.search_knn_norm_mt(queries, nr, o.k, o.ef, T, o.per_thread, 20.0)
        posted, tm1 = m.posted_queries() - p0, server_times(m)
        out["threads"].append({"threads": T, "queries": done, "queries_per_sec": done / secs if secs else None, "posted": posted,
                               "posted_ms_on_device": (tm1[0] - tm0[0]) / posted / 1e3 if posted else None,
                               "posted_ms_at_caller": (tm1[1] - tm0[1]) / posted / 1e3 if posted else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=20260924)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--build-threads", type=int, default=0)
    ap.add_argument("--threads", type=lambda t: tuple(int(x) for x in t.split(",")), default=(1, 16, 64, 256))
    ap.add_argument("--per-thread", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--graph", default=None, help="the Map's index cache written by --save-graph over the same corpus: skip the host build")
    ap.add_argument("--save-graph", default=None)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    metric = capi.METRICS[o.metric]
    from cpu_scaling import effective_cpus
    build_threads = o.build_threads or 2 * effective_cpus()
    corpus = make_clustered(o.rows + o.queries, o.dim, o.clusters, o.seed, o.device)
    rows, queries = corpus[:o.rows], corpus[o.rows:]
    labels = np.arange(o.rows, dtype=np.uint64) << np.uint64(32)
    norms = None
    if metric == 2:
        pairs = [hostapi.normalize_copy(q) for q in queries]
        queries = np.stack([a for a, _ in pairs])
        norms = (np.float32(1.0) / np.array([b for _, b in pairs], np.float32)).astype(np.float32)
    t0 = time.perf_counter()
    m = hostapi.GpuHnswMap(metric, o.dim, o.rows, M=o.M, ef_construction=o.efc, multithread=not o.graph and build_threads > 1, device=o.device)
    if o.graph:
        m.load_index(Path(o.graph).read_bytes(), labels, rows)
    else:
        m.add(rows, labels, threads=build_threads if build_threads > 1 else 0)
        if o.save_graph:
            Path(o.save_graph).write_bytes(m.save_index())
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    params = m.quantize_config(sample_size=20000, switch=True)   # the reference's sampled range (QuantizingParams)
    quant_s = time.perf_counter() - t0
    out = {"workload": f"quantised (SQ8) HNSW Map, {o.metric} M={o.M} efC={o.efc} ef={o.ef} k={o.k}, {o.rows} x {o.dim}, T threads with one SearchKnn each",
           "build_seconds": build_s, "graph_loaded": bool(o.graph), "quantize_seconds": quant_s,
           "params": {k: float(v) for k, v in zip(("min_q", "max_q", "alpha", "alpha_2", "delta"), params)}, "runs": []}
    for _ in range(max(1, o.repeat)):
        run = {}
        for name, off in (("code_mailbox", False), ("launch_per_query", True)):
            if off:
                os.environ["RXGPU_HNSW_SERVER_SQ8"] = "0"
            try:
                run[name] = legs(m, queries, norms, o)
            finally:
                os.environ.pop("RXGPU_HNSW_SERVER_SQ8", None)
        out["runs"].append(run)
    m.close()
    text = json.dumps(out)
    print(text)
    if o.out:
        Path(o.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
