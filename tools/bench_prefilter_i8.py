#!/usr/bin/env python3
"""Pre-filtered and IVF single-query KNN: the int8-pruned subset scan against the f32 subset scan.  (GPU box only.)

    python tools/bench_prefilter_i8.py crossover [--out profiles/scan_i8_subset_crossover.json]
    python tools/bench_prefilter_i8.py default [--tree DIR] [--densities 0.1,1.0] [--ivf 64,256]

crossover: one process, one resident corpus (10M x 768 f32, inner product, k = 10).  Per density of a random row list the two series
    (RXGPU_SCAN_I8=1: the tier; RXGPU_SCAN_I8=0: the f32 subset scan; read by the library on every call) ALTERNATE, --rounds times each, every
    round timing --queries single-query searches through rxgpu_search_knn_subset_device with one synchronisation at the end.  The tier "wins"
    at a density when its worst round beats the f32 scan's best round; the automatic threshold (RXGPU_SCAN_I8_SUBSET_MIN_BYTES, in f32 bytes
    of the LISTED rows) is the smallest listed-bytes value from which it wins at every larger measured point, rounded up to a power of two and
    never below 1 GiB.  At density 1.0 the unfiltered int8 tier (rxgpu_search_knn_device) is timed in the same rounds.
default: the library's own decision (no switch set), one JSON line: ms per query per density and, with --ivf, per nprobe of
    rxgpu_search_knn_lists over 1M x 768 cosine rows in 1024 lists.  The lists are a random assignment (what the scan costs does not depend
    on which rows a list holds).  --tree DIR imports reindexer_amd from another checkout: alternate a build of the parent commit and this
    one, process by process, for an A/B record."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path


def series(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": [round(x, 5) for x in v]}


def set_env(env):
    for k, v in env.items():   # None: unset
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["crossover", "default"])
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--densities", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--ivf", default=None, metavar="NPROBE,..")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import torch
    from reindexer_amd import capi

    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream(device).cuda_stream
    g = torch.Generator(device=device)
    g.manual_seed(1)
    n, dim, kk, nq = args.rows, args.dim, args.k, args.queries
    corpus = torch.empty((n, dim), dtype=torch.float32, device=device)
    for a in range(0, n, 1 << 20):
        corpus[a:a + (1 << 20)].normal_(0.0, 0.25, generator=g)
    q = torch.empty((nq, dim), dtype=torch.float32, device=device).normal_(0.0, 0.25, generator=g)
    out_d = torch.empty((nq, kk), dtype=torch.float32, device=device)
    out_r = torch.empty((nq, kk), dtype=torch.int32, device=device)

    def row_list(density):
        keep = torch.rand(n, device=device, generator=g) < density if density < 1.0 else torch.ones(n, dtype=torch.bool, device=device)
        return torch.nonzero(keep).flatten().to(torch.int32)   # ascending; the same bits as uint32

    def time_subset(ix, ids, count):
        t0 = time.perf_counter()
        for i in range(count):
            ix.search_knn_subset_device(q.data_ptr() + i * dim * 4, 1, kk, ids.data_ptr(), ids.numel(), out_d.data_ptr() + i * kk * 4,
                                        out_r.data_ptr() + i * kk * 4, None, stream)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / count * 1e3

    def time_unfiltered(ix, count):
        t0 = time.perf_counter()
        for i in range(count):
            ix.search_knn_device(q.data_ptr() + i * dim * 4, 1, kk, out_d.data_ptr() + i * kk * 4, out_r.data_ptr() + i * kk * 4, None, stream)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / count * 1e3

    switches = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES")
    for name in switches:
        os.environ.pop(name, None)
    result = {"mode": args.mode, "label": args.label, "rows": n, "dim": dim, "metric": "ip", "k": kk, "queries_per_round": nq,
              "rounds": args.rounds, "arch": capi.device_arch(0)}
    with capi.VectorIndex(capi.METRICS["ip"], dim, device=0) as ix:
        ix.adopt_device_rows(corpus.data_ptr(), n, dim, None, keepalive=(corpus,))
        if args.mode == "crossover":
            variants = [("int8", {"RXGPU_SCAN_I8": "1"}), ("f32", {"RXGPU_SCAN_I8": "0"})]
            result["points"] = []
            for density in [float(x) for x in (args.densities or "0.01,0.03,0.1,0.3,1.0").split(",")]:
                ids = row_list(density)
                times = {name: [] for name, _ in variants}
                got = {}
                for name, env in variants:   # warm-up (statistics, shadow, buffers) and the rows each path returns
                    set_env(env)
                    time_subset(ix, ids, 4)
                    got[name] = (out_d[:4].clone(), out_r[:4].clone())
                unfiltered = []
                for _ in range(args.rounds):
                    for name, env in variants:
                        set_env(env)
                        times[name].append(time_subset(ix, ids, nq))
                    if density >= 1.0:
                        set_env({"RXGPU_SCAN_I8": None})   # the library's own choice for the unfiltered search: the int8 tier at this size
                        unfiltered.append(time_unfiltered(ix, nq))
                entry = {"density": density, "n_ids": ids.numel(), "listed_f32_bytes": ids.numel() * dim * 4,
                         **{name: series(v) for name, v in times.items()},
                         "same_rows_and_bits": bool(torch.equal(got["int8"][1], got["f32"][1]) and
                                                    torch.equal(got["int8"][0].view(torch.int32), got["f32"][0].view(torch.int32))),
                         "int8_wins_beyond_spread": max(times["int8"]) < min(times["f32"]),
                         "ratio_of_medians": statistics.median(times["int8"]) / statistics.median(times["f32"])}
                if unfiltered:
                    entry["unfiltered_int8_tier"] = series(unfiltered)
                result["points"].append(entry)
                print(json.dumps(entry), flush=True)
            wins = [e["listed_f32_bytes"] for e in result["points"] if e["int8_wins_beyond_spread"]]
            losing = [e["listed_f32_bytes"] for e in result["points"] if not e["int8_wins_beyond_spread"]]
            first = min((b for b in wins if all(b > l for l in losing)), default=None)
            result["smallest_winning_listed_bytes"] = first
            result["threshold_bytes"] = max(1 << (first - 1).bit_length(), 1 << 30) if first else None
            result["threshold_rule"] = "smallest winning listed-bytes value rounded up to a power of two, not below 1 GiB; none: forced-only"
        else:
            result["densities"] = []
            for density in [float(x) for x in (args.densities or "0.1,1.0").split(",")]:
                ids = row_list(density)
                time_subset(ix, ids, 4)
                result["densities"].append({"density": density, "n_ids": ids.numel(),
                                            **series([time_subset(ix, ids, nq) for _ in range(args.rounds)])})
    if args.mode == "default" and args.ivf:
        import numpy as np
        rows_n, nlist = 1_000_000, 1024
        sub = corpus[:rows_n]
        inv = (1.0 / torch.linalg.vector_norm(sub, dim=1)).contiguous()
        rng = np.random.default_rng(7)
        owner = rng.integers(0, nlist, rows_n)
        lists = [np.flatnonzero(owner == l).astype(np.uint32) for l in range(nlist)]
        cents = rng.normal(0, 0.25, (nlist, dim)).astype(np.float32)
        cents /= np.linalg.norm(cents, axis=1, keepdims=True)
        hq = (q / torch.linalg.vector_norm(q, dim=1, keepdim=True)).cpu().numpy()
        result["ivf"] = {"rows": rows_n, "metric": "cosine", "nlist": nlist, "lists": "random assignment", "nprobe": []}
        with capi.VectorIndex(capi.METRICS["cosine"], dim, device=0) as ix, capi.VectorIndex(capi.METRICS["cosine"], dim, nlist, device=0) as cx:
            ix.adopt_device_rows(sub.data_ptr(), rows_n, dim, inv.data_ptr(), keepalive=(corpus, inv))
            cx.upload_rows(0, cents, np.ones(nlist, np.float32))
            ix.set_lists(lists)
            for nprobe in [int(x) for x in args.ivf.split(",")]:
                ix.search_knn_lists(cx, hq[0], nprobe, kk)
                rounds, scanned = [], 0
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for i in range(nq):
                        scanned = ix.search_knn_lists(cx, hq[i], nprobe, kk)[2]
                    rounds.append((time.perf_counter() - t0) / nq * 1e3)
                result["ivf"]["nprobe"].append({"nprobe": nprobe, "rows_scanned": int(scanned), "listed_f32_bytes": int(scanned) * dim * 4,
                                                **series(rounds)})
    print(json.dumps(result if args.mode == "default" else {k_: v for k_, v in result.items() if k_ != "points"}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
