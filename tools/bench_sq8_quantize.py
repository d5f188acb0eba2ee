#!/usr/bin/env python3
"""Quantize() of an HNSW Map to the end of its first search: SQ8 codes computed on the device against coded on the host and uploaded.
(GPU box only.)

    python tools/bench_sq8_quantize.py --parent DIR [--rows 1000000] [--out profiles/sq8_quantize_ab.json]
    python tools/bench_sq8_quantize.py --leg NAME [--tree DIR] [--host-path]      # one leg, one JSON line (what the first form starts)

Three legs, each a process of its own (a process holds one build of the library):
    parent    a build of the parent commit checked out at DIR: Sq8Quantize on one host thread, a rows x dim byte buffer, rxgpu_hnsw_attach_sq8
    host      this tree with RXGPU_SQ8_QUANTIZE=host: the same path, kept for this comparison
    default   this tree: rxgpu_hnsw_quantize_sq8 over the float rows the device holds
The legs run one after another, --rounds times in that order, so a drift of the machine shows as a difference between a leg's rounds.

Per leg and metric (L2, cosine): a Map of --rows x --dim synthetic rows (N(0, 0.25), seeded) under a trivial graph (M = 2, efConstruction = 1:
the graph build must not dominate, and the quantisation does not look at the graph).  One search puts rows and graph on the device; one
Quantize + search is the warm-up (code objects, buffers); then --repeats times: Quantize(minQ, maxQ) with alternating ranges, and the host
clock from before Quantize to the return of the first search (the search synchronises: it returns results).  On this tree the kernel's own
time comes from rxgpu_hnsw_read_sq8_quantize_stats (device events around the launch) and is set against the bytes the pass has to move,
rows x dim x 5 + rows x 4, over the HBM peak (8.0 TB/s by specification; 6.3 TB/s is what a float4 copy reaches).  Every leg reports
the labels and distance bits of its searches: the driver refuses to report timings of legs that disagree."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
RANGES = ((-0.6, 0.6), (-0.45, 0.5))
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def run_leg(args):
    if args.host_path:
        os.environ["RXGPU_SQ8_QUANTIZE"] = "host"
    else:
        os.environ.pop("RXGPU_SQ8_QUANTIZE", None)
    sys.path.insert(0, args.tree)
    import numpy as np
    from reindexer_amd import capi, hostapi

    L = capi.lib()
    has_stats = hasattr(L, "rxgpu_hnsw_read_sq8_quantize_stats")
    n, d = args.rows, args.dim
    out = {"leg": args.leg, "tree_has_device_coding": has_stats, "host_path": bool(args.host_path), "rows": n, "dim": d, "arch": capi.device_arch(0), "metrics": {}}
    for mname in args.metrics.split(","):
        metric = capi.METRICS[mname]
        rng = np.random.default_rng(7)
        rows = rng.normal(0.0, 0.25, (n, d)).astype(np.float32)
        labels = np.arange(n, dtype=np.uint64) << np.uint64(32)
        q = rng.normal(0.0, 0.25, d).astype(np.float32)
        norm = None
        if metric == capi.METRIC_COSINE:
            norm = float(np.sqrt(np.sum(q.astype(np.float64) ** 2)))
            q = (q / np.float32(norm)).astype(np.float32)
        t0 = time.perf_counter()
        m = hostapi.GpuHnswMap(metric, d, n, M=2, ef_construction=1)
        m.add(rows, labels)
        del rows
        build_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        m.search_knn_norm(q, 10, 64, norm)            # rows + graph go up
        first_sync_s = time.perf_counter() - t0

        def stats():
            r, l_, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
            assert L.rxgpu_hnsw_read_sq8_quantize_stats(m.device_index, C.byref(r), C.byref(l_), C.byref(ms)) == 0
            return int(r.value), int(l_.value), float(ms.value)

        wall, kernel_ms, coded, answers = [], [], [], []
        for it in range(1 + args.repeats):            # the first is the warm-up
            lo, hi = RANGES[it % 2]
            if has_stats:
                stats()
            t0 = time.perf_counter()
            m.quantize(lo, hi)
            dist, lab = m.search_knn_norm(q, 10, 64, norm)
            dt = time.perf_counter() - t0
            if has_stats:
                r, l_, ms = stats()
                assert (r, l_) == ((n, 1) if not args.host_path else (0, 0)), (r, l_)
            if it:
                wall.append(dt * 1e3)
                if has_stats and not args.host_path:
                    kernel_ms.append(ms)
                    coded.append(r)
            answers.append([lab.tolist(), dist.view(np.uint32).tolist()])
        m.close()
        res = {"build_s": round(build_s, 2), "first_sync_s": round(first_sync_s, 3), "quantize_to_first_search_ms": [round(x, 3) for x in wall],
               "median_ms": statistics.median(wall), "min_ms": min(wall), "max_ms": max(wall), "answers": answers}
        if kernel_ms:
            byts = n * d * 5 + n * 4
            k = statistics.median(kernel_ms)
            res["kernel_ms"] = [round(x, 4) for x in kernel_ms]
            res["kernel_median_ms"] = k
            res["kernel_bytes"] = byts
            res["kernel_tb_per_s"] = byts / (k * 1e-3) / 1e12
            res["kernel_fraction_of_hbm_spec_8.0"] = (byts / HBM_SPEC) / (k * 1e-3)
            res["kernel_fraction_of_hbm_copy_6.3"] = (byts / HBM_COPY) / (k * 1e-3)
        out["metrics"][mname] = res
    print("LEG " + json.dumps(out), flush=True)


def drive(args):
    legs = (("parent", args.parent, False), ("host", str(HERE), True), ("default", str(HERE), False))
    runs = []
    for rnd in range(args.rounds):
        for name, tree, host_path in legs:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--tree", tree, "--rows", str(args.rows), "--dim", str(args.dim),
                   "--metrics", args.metrics, "--repeats", str(args.repeats)] + (["--host-path"] if host_path else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
            line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"leg {name} failed (exit {p.returncode})")   # nothing more is started on the device
            leg = json.loads(line[-1][4:])
            leg["round"] = rnd
            runs.append(leg)
            print(json.dumps({"round": rnd, "leg": name, **{mn: {k: v for k, v in r.items() if k != "answers"} for mn, r in leg["metrics"].items()}}), flush=True)
    result = {"rows": args.rows, "dim": args.dim, "repeats_per_leg_and_round": args.repeats, "rounds": args.rounds, "arch": runs[0]["arch"],
              "timing": "host clock from before Quantize(minQ, maxQ) to the return of the first search, ms; kernel: device events around the launch",
              "clocks": "not pinned, not read: the legs run one after another, round by round", "graph": "M = 2, efConstruction = 1 (trivial)",
              "metrics": {}}
    for mname in args.metrics.split(","):
        ans = [r["metrics"][mname]["answers"] for r in runs]
        same = all(a == ans[0] for a in ans)
        entry = {"every_leg_returns_the_same_labels_and_distance_bits": same}
        for name, _, _ in legs:
            mine = [r["metrics"][mname] for r in runs if r["leg"] == name]
            wall = [x for r in mine for x in r["quantize_to_first_search_ms"]]
            e = {"quantize_to_first_search_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall), "all": wall},
                 "build_s": [r["build_s"] for r in mine], "first_sync_s": [r["first_sync_s"] for r in mine]}
            ks = [x for r in mine for x in r.get("kernel_ms", [])]
            if ks:
                byts = mine[0]["kernel_bytes"]
                k = statistics.median(ks)
                e["kernel_ms"] = {"median": k, "min": min(ks), "max": max(ks), "all": ks}
                e["kernel_bytes"] = byts
                e["kernel_tb_per_s"] = byts / (k * 1e-3) / 1e12
                e["kernel_fraction_of_hbm_spec_8.0_tb_s"] = (byts / HBM_SPEC) / (k * 1e-3)
                e["kernel_fraction_of_hbm_copy_6.3_tb_s"] = (byts / HBM_COPY) / (k * 1e-3)
            entry[name] = e
        d_, p_, h_ = (entry[x]["quantize_to_first_search_ms"] for x in ("default", "parent", "host"))
        entry["default_over_parent_medians"] = d_["median"] / p_["median"]
        entry["default_over_host_medians"] = d_["median"] / h_["median"]
        entry["default_faster_than_parent_beyond_spread"] = d_["max"] < p_["min"]
        result["metrics"][mname] = entry
    print(json.dumps({mn: {k: v for k, v in e.items() if not isinstance(v, dict)} for mn, e in result["metrics"].items()}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    if not all(e["every_leg_returns_the_same_labels_and_distance_bits"] for e in result["metrics"].values()):
        raise SystemExit("the legs disagree on a search result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a build of the parent commit: run the three legs")
    ap.add_argument("--leg", default=None)
    ap.add_argument("--tree", default=str(HERE))
    ap.add_argument("--host-path", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--leg-timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        run_leg(args)
    elif args.parent:
        drive(args)
    else:
        ap.error("--parent DIR (all legs) or --leg NAME (one)")


if __name__ == "__main__":
    main()
