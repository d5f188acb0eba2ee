#!/usr/bin/env python3
"""A/B of the HNSW build: level 0 on the device in batches (RXGPU_HNSW_BUILD=device) against the host's concurrent insertions
(RXGPU_HNSW_BUILD=host, --threads inserting threads), same corpus, same session.

    python tools/bench_hnsw_build.py --ab [--rows 1000000] [--out profiles/hnsw_build_ab.json]
    python tools/bench_hnsw_build.py --upper [--parent-json FILE] [--out profiles/hnsw_build_upper_ab.json]

--upper adds a third leg beside the two: RXGPU_HNSW_BUILD=device with RXGPU_HNSW_BUILD_UPPER=device (level 1 of every batch on the device
too, the host keeps the levels >= 2).  --parent-json: the output of the same tool at the parent commit, run in the same session — its two
legs are quoted in the file as the yardsticks.

The corpus is the clustered one of bench.py's HNSW leg (tools/bench_hnsw.py: make_clustered), cosine, M = 16, efConstruction = 200.
Per leg: build seconds (the adds and, for the device leg, the flush the first search triggers), the device's milliseconds per phase
(search, select + pair grouping, back-links), the host's seconds in the upper levels, and recall@10 at ef = 128 of --recall-queries
queries against the exact scan of the same rows on the GPU.  The statement the file makes is the ratio of the two build times, with both
recalls beside it."""
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
os.environ.setdefault("RX_TARGET_INSTRUCTIONS", "avx512")

from reindexer_amd import capi, hostapi  # noqa: E402


def leg(name: str, o, rows, labels, queries, truth) -> dict:
    mode = "device" if name == "device_upper" else name
    os.environ["RXGPU_HNSW_BUILD"] = mode
    os.environ["RXGPU_HNSW_BUILD_UPPER"] = "device" if name == "device_upper" else "host"
    print(f"leg {name} ...", file=sys.stderr, flush=True)
    m = hostapi.GpuHnswMap(2, o.dim, o.rows, M=o.M, ef_construction=o.efc, multithread=True, device=o.device)
    t0 = time.perf_counter()
    if mode == "device":
        m.add_points(rows, labels)
    else:
        m.add(rows, labels, threads=o.threads)
    add_s = time.perf_counter() - t0
    m.search_knn(queries[0], o.k, o.ef)              # device leg: links the stored rows; both: mirrors the graph
    first_search_s = time.perf_counter() - t0 - add_s
    st = m.build_stats()
    build_s = add_s + (st["flush_seconds"] if mode == "device" else 0.0)
    hit = 0
    for q, want in zip(queries, truth):
        _, got = m.search_knn(q, o.k, o.ef)
        hit += len(set(int(x) >> 32 for x in got) & set(int(x) for x in want))
    e = m.export_graph()
    print(f"leg {name}: build {build_s:.1f} s", file=sys.stderr, flush=True)
    out = {"mode": name, "build_seconds": build_s, "add_seconds": add_s, "first_search_seconds": first_search_s,
           "inserts_per_sec": o.rows / build_s, "recall_at_10": hit / (o.k * len(queries)), "mean_level0_degree": float(e["links0"][:, 0].mean()),
           "threads": o.threads if mode == "host" else 1, "stats": st}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true", help="both legs in this session: the device build, then the host build; without it the device leg alone")
    ap.add_argument("--upper", action="store_true", help="three legs: the device build, the device build with level 1 on the device, the host build")
    ap.add_argument("--parent-json", default=None, help="this tool's output at the parent commit, same session: quoted as the yardsticks")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16, help="inserting threads of the host leg")
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=20260924)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--legs", default=None, help="comma-separated legs in the order they run (overrides --ab)")
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    o.legs = o.legs or ("device,device_upper,host" if o.upper else "device,host" if o.ab else "device")
    o.out = o.out or str(ROOT / "profiles" / ("hnsw_build_upper_ab.json" if o.upper else "hnsw_build_ab.json"))
    from bench_hnsw import make_clustered
    corpus = make_clustered(o.rows + o.recall_queries, o.dim, o.clusters, o.seed, o.device)
    rows, raw_q = corpus[:o.rows], corpus[o.rows:]
    labels = np.arange(o.rows, dtype=np.uint64) << np.uint64(32)
    queries = np.stack([hostapi.normalize_copy(q)[0] for q in raw_q])
    inv = np.array([hostapi.l2_module(r) for r in rows], np.float32)
    with capi.VectorIndex(2, o.dim, o.rows, device=o.device) as ix:   # exact: the brute-force scan of the same rows
        ix.upload_rows(0, rows, inv)
        truth = np.stack([ix.search_knn(q, o.k)[1][0, :o.k] for q in queries])
    legs = {name: leg(name, o, rows, labels, queries, truth) for name in o.legs.split(",")}
    out = {"tool": "tools/bench_hnsw_build.py", "device": capi.device_arch(o.device), "rows": o.rows, "dim": o.dim, "metric": "cosine", "M": o.M,
           "ef_construction": o.efc, "recall_ef": o.ef, "recall_queries": o.recall_queries, "corpus": f"{o.clusters} gaussian clusters (tools/bench_hnsw.py)",
           "legs": legs}
    if "device" in legs and "host" in legs:
        out["host_over_device_build_time"] = legs["host"]["build_seconds"] / legs["device"]["build_seconds"]
        st = legs["device"]["stats"]
        phases = {"device search": st["search_ms"] / 1e3, "device select": st["select_ms"] / 1e3, "device back-links": st["backlink_ms"] / 1e3,
                  "host upper levels": st["upper_seconds"]}
        out["device_leg_largest_phase"] = max(phases, key=phases.get)
        out["device_leg_phase_seconds"] = phases
    if "device_upper" in legs:
        st = legs["device_upper"]["stats"]
        up = {"build_seconds": legs["device_upper"]["build_seconds"], "upperSeconds": st["upper_seconds"],
              "level0_device_ms": st["search_ms"] + st["select_ms"] + st["backlink_ms"],
              "level1_device_ms": st["upper_search_ms"] + st["upper_select_ms"] + st["upper_backlink_ms"],
              "recall_at_10": {name: l["recall_at_10"] for name, l in legs.items()}}
        if "device" in legs:
            up["device_over_device_upper_build_time"] = legs["device"]["build_seconds"] / legs["device_upper"]["build_seconds"]
        if "host" in legs:
            up["host_over_device_upper_build_time"] = legs["host"]["build_seconds"] / legs["device_upper"]["build_seconds"]
        phases = {"device level 0": up["level0_device_ms"] / 1e3, "device level 1": up["level1_device_ms"] / 1e3, "host levels >= 2": st["upper_seconds"]}
        up["largest_phase"] = max(phases, key=phases.get)
        up["phase_seconds"] = phases
        out["device_upper"] = up
    if o.parent_json:
        parent = json.loads(Path(o.parent_json).read_text())
        out["parent_commit"] = {name: {k: l[k] for k in ("build_seconds", "recall_at_10", "threads")} | {"upper_seconds": l["stats"]["upper_seconds"]}
                                for name, l in parent["legs"].items()}
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
