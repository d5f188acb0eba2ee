#!/usr/bin/env python3
"""IVF-Flat on the GPU engines (first cut): build (k-means on the matrix-core batch path) and search at several nprobe.

    python tools/bench_ivf.py --rows 1000000 --dim 768 --nlist 1024 --queries 200 [--out profiles/r1_ivf_1m.json]
    python tools/bench_ivf.py --train-ab --rows 1000000 --dim 768 --nlist 1024 [--metric l2] [--parent-root DIR] [--out FILE]
        train() on the device path against RXGPU_IVF_TRAIN=host (and a checkout of the parent commit), every leg in a fresh child process
    python tools/bench_ivf.py --batch-ab --rows 1000000 --dim 768 --nlist 1024 [--metric cosine] [--out profiles/ivf_batch_ab.json]
        search_batch on one index in one session: the batched list search against RXGPU_IVF_BATCH=threads, 256 and 4096 queries at nprobe 1 / 16 / 64

Per query: coarse quantiser (KNN over the centroids) -> host merge of the probed lists' rows -> row-list scan (knn_scan_subset).  Recall@k is
measured against the exact result (the same index with every list probed, which the tests pin to the brute-force oracle).  There is no CPU
line: the reference's IVF backend is FAISS, which cannot be built in this image (BLAS)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if "--root" in sys.argv:   # a training leg over another checkout of the package (the parent commit, built in place)
    ROOT = Path(sys.argv[sys.argv.index("--root") + 1]).resolve()
sys.path.insert(0, str(ROOT))

from reindexer_amd import capi, hostapi  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8.0e12   # MI355X HBM3E specification


def make_rows(rows, dim, clusters, seed=20260924):
    """the bench's clustered corpus, in float32 from the start (3 GB at 1M x 768: one generation serves every leg)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim), dtype=np.float32) * np.float32(0.25)
    out = np.empty((rows, dim), np.float32)
    step = 65536
    for a in range(0, rows, step):
        b = min(rows, a + step)
        out[a:b] = centres[rng.integers(0, clusters, b - a)] + rng.standard_normal((b - a, dim), dtype=np.float32) * np.float32(0.08)
    return out


def train_leg(args):
    """One timed train() in this process: rows from --rows-file, one small warm-up index first (it loads the kernels every leg uses), then
    add_with_ids + train() on the clock (train() ends in device synchronisation).  Prints one JSON line."""
    metric = capi.METRICS[args.metric]
    rows = np.load(args.rows_file, mmap_mode="r")
    n, dim = rows.shape
    warm = hostapi.GpuIvfFlat(metric, dim, 16)
    warm.add_with_ids(np.ascontiguousarray(rows[:8192]), np.arange(8192, dtype=np.int64))
    warm.train()
    warm.close()
    ivf = hostapi.GpuIvfFlat(metric, dim, args.nlist)
    t0 = time.perf_counter()
    step = 100_000
    for a in range(0, n, step):
        ivf.add_with_ids(np.ascontiguousarray(rows[a:a + step]), np.arange(a, min(n, a + step), dtype=np.int64))
    add_s = time.perf_counter() - t0
    if hasattr(ivf, "train_stats"):
        ivf.train_stats()
    t0 = time.perf_counter()
    ivf.train()
    train_s = time.perf_counter() - t0
    stats = ivf.train_stats() if hasattr(ivf, "train_stats") else None
    sizes = ivf.list_sizes()
    out = {"leg": args.train_leg, "train_seconds": train_s, "add_seconds": add_s, "stats": stats,
           "centroids_crc32": zlib.crc32(np.ascontiguousarray(ivf.centroids()).tobytes()), "list_sizes_crc32": zlib.crc32(sizes.tobytes()),
           "RXGPU_IVF_TRAIN": os.environ.get("RXGPU_IVF_TRAIN")}
    ivf.close()
    print("LEG " + json.dumps(out), flush=True)


def train_ab(args):
    """train() under the default (device) path, under RXGPU_IVF_TRAIN=host and, with --parent-root, in a checkout of the parent commit: the
    same rows, every leg in a fresh child process, the legs alternating, --repeat of each; medians.  kernel_ms / sums_ms are the device
    path's own event pairs (GpuIvfFlat.train_stats); the sums kernel's bytes are counted from the shapes (10 iterations over
    min(rows, 256 nlist) points: every point's row once per iteration, its row number and 1 / |x| per 64-column tile, the table once)."""
    tmp = Path(tempfile.mkdtemp(prefix="bench_ivf_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None))
    try:
        rows_file = tmp / "rows.npy"
        np.save(rows_file, make_rows(args.rows, args.dim, args.clusters))
        legs = [("device", None, None), ("host", "host", None)]
        if args.parent_root:
            legs.append(("parent", None, args.parent_root))
        runs = {name: [] for name, _, _ in legs}
        for rep in range(args.repeat):
            for name, env_value, root in legs:
                env = dict(os.environ)
                env.pop("RXGPU_IVF_TRAIN", None)
                if env_value:
                    env["RXGPU_IVF_TRAIN"] = env_value
                cmd = [sys.executable, str(Path(__file__).resolve()), "--train-leg", name, "--rows-file", str(rows_file), "--nlist", str(args.nlist),
                       "--metric", args.metric]
                if root:
                    cmd += ["--root", root]
                res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.leg_timeout)
                line = [l for l in res.stdout.splitlines() if l.startswith("LEG ")]
                if res.returncode != 0 or not line:
                    raise RuntimeError(f"leg {name} failed (rc {res.returncode}): {res.stderr[-2000:]}")
                runs[name].append(json.loads(line[-1][4:]))
                print(f"# rep {rep} {name}: train {runs[name][-1]['train_seconds']:.3f} s", file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    def summary(name):
        t = [r["train_seconds"] for r in runs[name]]
        out = {"train_seconds_median": statistics.median(t), "train_seconds_min": min(t), "train_seconds_max": max(t), "train_seconds": t,
               "add_seconds_median": statistics.median(r["add_seconds"] for r in runs[name])}
        st = [r["stats"] for r in runs[name] if r["stats"]]
        if st:
            out["stats_median"] = {k: statistics.median(s[k] for s in st) for k in st[0]}
        return out

    ns = min(args.rows, 256 * args.nlist)
    tiles = -(-args.dim // 64)
    cosine = args.metric == "cosine"
    sums_bytes = 10 * (ns * (args.dim * 4 + 4 * tiles * (2 if cosine else 1)) + args.nlist * args.dim * 4)
    out = {"workload": f"IVF-Flat train(), {args.metric}, {args.rows} x {args.dim}, nlist={args.nlist}, {args.clusters} gaussian clusters; "
                       f"k-means 10 iterations over {ns} points + list assignment of every row",
           "arch": capi.device_arch(0), "repeat": args.repeat, "protocol": "every leg a fresh child process over the same rows (one warm-up index of 8192 rows "
           "first), legs alternating; host clock around train(), which ends in a device synchronisation",
           "legs": {name: summary(name) for name in runs}}
    crcs = {(r["centroids_crc32"], r["list_sizes_crc32"]) for name in runs for r in runs[name]}
    out["every_leg_same_centroid_bits_and_list_sizes"] = len(crcs) == 1
    dev = out["legs"]["device"]
    out["device_over_host"] = dev["train_seconds_median"] / out["legs"]["host"]["train_seconds_median"]
    if "parent" in out["legs"]:
        out["device_over_parent"] = dev["train_seconds_median"] / out["legs"]["parent"]["train_seconds_median"]
    if "stats_median" in dev and dev["stats_median"]["sums_ms"] > 0:
        sums_s = dev["stats_median"]["sums_ms"] * 1e-3
        out["sums_kernel"] = {"bytes_10_iterations": sums_bytes, "ms_10_iterations": dev["stats_median"]["sums_ms"], "bytes_per_second": sums_bytes / sums_s,
                              "fraction_of_hbm_spec_8TBps": sums_bytes / sums_s / HBM_SPEC_BYTES_PER_S}
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


def batch_ab(args):
    """search_batch on ONE trained index in one session: the default (rxgpu_search_knn_lists_batch, one launch train for all queries) against
    RXGPU_IVF_BATCH=threads (four host threads driving single searches), --batch-queries queries at --batch-nprobe, the legs alternating,
    --repeat timed calls of each behind one warm-up call; medians and ranges.  Labels and distance bits of the two legs are compared.  The
    scan kernel's own time comes from the C-ABI over the same rows, centroids and lists (event pairs of the "scan_lists" profile slot), its
    bytes are the rows probed x dim x 4."""
    metric = capi.METRICS[args.metric]
    nqs = [int(x) for x in args.batch_queries.split(",")]
    nprobes = [int(x) for x in args.batch_nprobe.split(",")]
    rows = make_rows(args.rows, args.dim, args.clusters)
    rng = np.random.default_rng(20260925)
    queries = np.ascontiguousarray(rows[rng.integers(0, args.rows, max(nqs))] + rng.standard_normal((max(nqs), args.dim), dtype=np.float32) * np.float32(0.08))
    ivf = hostapi.GpuIvfFlat(metric, args.dim, args.nlist)
    step = 100_000
    for a in range(0, args.rows, step):
        ivf.add_with_ids(rows[a:a + step], np.arange(a, min(args.rows, a + step), dtype=np.int64))
    ivf.train()
    sizes = ivf.list_sizes()
    out = {"workload": f"IVF-Flat search_batch, {args.metric}, {args.rows} x {args.dim}, nlist={args.nlist}, k={args.k}, {args.clusters} gaussian clusters; "
                       "queries = stored rows + noise",
           "arch": capi.device_arch(0), "repeat": args.repeat,
           "protocol": "one index, one process; per shape one untimed call of each leg, then the legs alternating, host clock around search_batch "
                       "(which ends in a device synchronisation); median of the timed calls, min and max given",
           "legs": {"train": "default: one rxgpu_search_knn_lists_batch call", "threads": "RXGPU_IVF_BATCH=threads: four host threads, one rxgpu_search_knn_lists per query"},
           "list_sizes": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
           "shapes": []}

    def set_leg(leg):
        if leg == "threads":
            os.environ["RXGPU_IVF_BATCH"] = "threads"
        else:
            os.environ.pop("RXGPU_IVF_BATCH", None)

    for nq in nqs:
        for nprobe in nprobes:
            q = queries[:nq]
            times = {"train": [], "threads": []}
            got, stats = {}, {}
            for leg in times:
                set_leg(leg)
                ivf.search_batch(q, args.k, nprobe=nprobe)
            ivf.batch_stats()
            for _ in range(args.repeat):
                for leg in times:
                    set_leg(leg)
                    t0 = time.perf_counter()
                    d, l = ivf.search_batch(q, args.k, nprobe=nprobe)
                    times[leg].append(time.perf_counter() - t0)
                    got[leg] = (np.ascontiguousarray(d).view(np.uint32).copy(), l.copy())
                    stats[leg] = ivf.batch_stats()
            set_leg("train")
            entry = {"queries": nq, "nprobe": nprobe}
            for leg, t in times.items():
                med = statistics.median(t)
                entry[leg] = {"seconds_median": med, "seconds_min": min(t), "seconds_max": max(t), "seconds": t, "queries_per_sec_median": nq / med,
                              "batch_stats_last_call": stats[leg]}
            entry["threads_over_train"] = entry["threads"]["seconds_median"] / entry["train"]["seconds_median"]
            entry["same_labels_and_distance_bits"] = bool(np.array_equal(got["train"][0], got["threads"][0]) and np.array_equal(got["train"][1], got["threads"][1]))
            out["shapes"].append(entry)
            print(f"# nq {nq} nprobe {nprobe}: train {entry['train']['seconds_median'] * 1e3:.2f} ms, threads {entry['threads']['seconds_median'] * 1e3:.2f} ms, "
                  f"same {entry['same_labels_and_distance_bits']}", file=sys.stderr, flush=True)
    # the scan kernel alone: the same rows, centroids and lists behind the C-ABI, profiling on
    cents = np.ascontiguousarray(ivf.centroids())
    lists = [ivf.list_ids(l).astype(np.uint32) for l in range(args.nlist)]   # ids are row numbers here
    ivf.close()
    cosine = args.metric == "cosine"
    qprep = np.stack([hostapi.normalize_copy(v)[0] for v in queries]) if cosine else queries
    with capi.VectorIndex(metric, args.dim, args.rows) as ix, capi.VectorIndex(metric, args.dim, args.nlist) as cx:
        for a in range(0, args.rows, step):
            r = rows[a:a + step]
            ix.upload_rows(a, r, (1.0 / np.sqrt(np.einsum("ij,ij->i", r.astype(np.float64), r.astype(np.float64)))).astype(np.float32) if cosine else None)
        cx.upload_rows(0, cents, (1.0 / np.linalg.norm(cents.astype(np.float64), axis=1)).astype(np.float32) if cosine else None)
        ix.set_lists(lists)
        ix.profile_enable(True)
        for entry in out["shapes"]:
            nq, nprobe = entry["queries"], entry["nprobe"]
            ix.search_knn_lists_batch(cx, qprep[:nq], nprobe, args.k + 1)
            n0, ms0 = ix.profile_read("scan_lists")
            m0 = ix.profile_read("merge")[1]
            o0 = ix.profile_read("ivf_batch_offsets")[1]
            for _ in range(args.repeat):
                _, _, _, scanned = ix.search_knn_lists_batch(cx, qprep[:nq], nprobe, args.k + 1)
            n1, ms1 = ix.profile_read("scan_lists")
            launches = n1 - n0
            ms = (ms1 - ms0) / max(launches, 1)
            nbytes = int(scanned.sum()) * args.dim * 4
            entry["scan_lists_kernel"] = {"launches_per_call": launches / args.repeat, "ms_per_launch_mean": ms, "rows_probed": int(scanned.sum()), "bytes": nbytes,
                                          "bytes_per_second": nbytes / (ms * 1e-3) if ms > 0 else None,
                                          "fraction_of_hbm_spec_8TBps": nbytes / (ms * 1e-3) / HBM_SPEC_BYTES_PER_S if ms > 0 else None,
                                          "merge_ms_per_call_mean": (ix.profile_read("merge")[1] - m0) / args.repeat,
                                          "offsets_ms_per_call_mean": (ix.profile_read("ivf_batch_offsets")[1] - o0) / args.repeat,
                                          "note": "the norms of this leg's rows are computed in numpy (not the engine's): timing only, no bits are compared here"}
        ix.profile_enable(False)
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--nprobe", default="1,4,16,64,128,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--train-ab", action="store_true", help="time train() on the device path, under RXGPU_IVF_TRAIN=host (and in --parent-root), fresh processes")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (its reindexer_amd package) for a third leg")
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--batch-ab", action="store_true", help="time search_batch on one index: the batched list search against RXGPU_IVF_BATCH=threads")
    ap.add_argument("--batch-queries", default="256,4096")
    ap.add_argument("--batch-nprobe", default="1,16,64")
    ap.add_argument("--train-leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rows-file", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.train_leg:
        return train_leg(args)
    if args.train_ab:
        return train_ab(args)
    if args.batch_ab:
        return batch_ab(args)
    metric = capi.METRICS[args.metric]
    rng = np.random.default_rng(20260924)
    centres = rng.normal(0, 0.25, (args.clusters, args.dim)).astype(np.float32)
    rows = (centres[rng.integers(0, args.clusters, args.rows)] + rng.normal(0, 0.08, (args.rows, args.dim))).astype(np.float32)
    queries = (centres[rng.integers(0, args.clusters, args.queries)] + rng.normal(0, 0.08, (args.queries, args.dim))).astype(np.float32)
    ids = np.arange(args.rows, dtype=np.int64)
    ivf = hostapi.GpuIvfFlat(metric, args.dim, args.nlist)
    t0 = time.perf_counter()
    step = 100_000
    for a in range(0, args.rows, step):
        ivf.add_with_ids(rows[a:a + step], ids[a:a + step])
    add_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ivf.train()
    train_s = time.perf_counter() - t0
    sizes = ivf.list_sizes()
    ivf.search(queries[0], args.k, nprobe=1)
    exact = [ivf.search(q, args.k, nprobe=args.nlist)[1] for q in queries]
    out = {"workload": f"IVF-Flat {args.metric}, {args.rows} x {args.dim}, nlist={args.nlist}, k={args.k}, {args.clusters} gaussian clusters",
           "arch": capi.device_arch(0), "add_seconds": add_s,
           "train_seconds": train_s, "train": "k-means 10 iterations over min(rows, 256 * nlist) points + assignment of every row, on the device from the resident rows (RXGPU_IVF_TRAIN=host: through host queries, 256 points per device call)",
           "list_sizes": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
           "nprobe": []}
    for nprobe in [int(x) for x in args.nprobe.split(",")]:
        t0 = time.perf_counter()
        got = [ivf.search(q, args.k, nprobe=nprobe)[1] for q in queries]
        dt = (time.perf_counter() - t0) / args.queries
        recall = float(np.mean([len(set(g.tolist()) & set(e.tolist())) / args.k for g, e in zip(got, exact)]))
        scanned = float(np.mean([ivf.probed_rows(q, nprobe).size for q in queries[:32]]))
        out["nprobe"].append({"nprobe": nprobe, "ms_per_query": dt * 1e3, "queries_per_sec": 1.0 / dt, "recall_at_k_vs_exact": recall,
                              "rows_scanned_avg": scanned, "fraction_of_corpus": scanned / args.rows})
    t0 = time.perf_counter()
    for q in queries[:32]:
        ivf.search(q, args.k, nprobe=args.nlist)
    out["all_lists_ms_per_query"] = (time.perf_counter() - t0) / 32 * 1e3
    # the queries of one call side by side (GpuIvfFlat::SearchBatch: a few host threads, every search on its own stream) and the range form
    ivf.search_batch(queries[:8], args.k, nprobe=16)
    t0 = time.perf_counter()
    bd, bl = ivf.search_batch(queries, args.k, nprobe=16)
    dt = (time.perf_counter() - t0) / args.queries
    one = [ivf.search(q, args.k, nprobe=16) for q in queries]
    out["batch_nprobe16"] = {"ms_per_query": dt * 1e3, "queries_per_sec": 1.0 / dt,
                             "identical_to_single_searches": bool(all(np.array_equal(bl[i], one[i][1]) and
                                                                      np.array_equal(bd[i].view(np.uint32), one[i][0].view(np.uint32)) for i in range(args.queries)))}
    kd, _ = ivf.search(queries[0], 50, nprobe=16)
    t0 = time.perf_counter()
    hits = 0
    for q in queries[:64]:
        kd, _ = ivf.search(q, 50, nprobe=16)
        rd, _ = ivf.range_search(q, float(kd[40]), nprobe=16)
        hits += rd.size
    out["range_nprobe16"] = {"ms_per_knn50_plus_range_query": (time.perf_counter() - t0) / 64 * 1e3, "hits_avg": hits / 64,
                             "note": "radius = the 41st best distance of the same probe: the device lists are scanned by rxgpu_search_range_lists"}
    ivf.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
