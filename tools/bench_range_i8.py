#!/usr/bin/env python3
"""Brute-force range search: the int8-pruned range scan against the f32 range kernel.  (GPU box only.)

    python tools/bench_range_i8.py [--rows 10000000,5000000,...] [--out profiles/range_i8_ab.json]
    python tools/bench_range_i8.py --tree DIR --label parent ...      # the same calls on another checkout (a build of the parent commit)

One process, one resident corpus (N(0, 0.25) rows x 768 f32, inner product), generated on the device from a seed; an index per row count
adopts the first rows of it.  Per row count and per query the radii are taken from that query's exact f32 KNN distances: the ones that
select about 10, about 1 000 and about 100 000 hits (strict), and the 11th-best distance, inclusive (the shape of the tie replay of
GpuBruteforceMap::SearchKnn).  The two series (RXGPU_SCAN_I8=1: the tier; RXGPU_SCAN_BF16=0: the f32 kernel; both read by the library on
every call) ALTERNATE, --rounds times each; a round is --repeat rxgpu_search_range calls per query, host to host, timed with the host clock
(the call synchronises before it returns).  cap = twice the hits, so no call overflows the caller's buffer.  Afterwards, with profiling enabled
and untimed, the kernel times of the profile slots ("range_i8", "range_rescore", "range") and the candidates of the tier.  The tier "wins"
at a size when its worst round beats the f32 kernel's best round for EVERY radius shape; RXGPU_SCAN_I8_RANGE_MIN_BYTES is meant to be the
smallest f32 size from which it wins at every larger measured size, rounded up to a power of two and never below 1 GiB."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from pathlib import Path

SHAPES = (("about_10_hits", 10, False), ("about_1000_hits", 1_000, False), ("about_100000_hits", 100_000, False), ("tie_replay_11th_inclusive", 11, True))
VARIANTS = (("int8", {"RXGPU_SCAN_I8": "1", "RXGPU_SCAN_BF16": None}), ("f32", {"RXGPU_SCAN_I8": None, "RXGPU_SCAN_BF16": "0"}))


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
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--rows", default="10000000,5000000,2500000,1250000,700000,350000")   # 30.7 GB .. 1.0 GiB of f32 rows at 768 dims
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=4, help="passes over the queries in one timed round")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from reindexer_amd import capi

    L = capi.lib()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator(device=device)
    g.manual_seed(1)
    sizes = sorted((int(x) for x in args.rows.split(",")), reverse=True)
    n_max, dim, nq = sizes[0], args.dim, args.queries
    corpus = torch.empty((n_max, dim), dtype=torch.float32, device=device)
    for a in range(0, n_max, 1 << 20):
        corpus[a:a + (1 << 20)].normal_(0.0, 0.25, generator=g)
    queries = torch.empty((nq, dim), dtype=torch.float32, device=device).normal_(0.0, 0.25, generator=g).cpu().numpy()

    def call(ix, qi, radius, inclusive, cap, bufs):
        total = C.c_uint64(0)
        rc = L.rxgpu_search_range(ix._h, queries[qi].ctypes.data, C.c_float(radius), int(inclusive), bufs[0].ctypes.data, bufs[1].ctypes.data, cap,
                                  C.byref(total))
        assert rc == 0, (rc, capi.last_error() if hasattr(capi, "last_error") else "")
        return int(total.value)

    for name in ("RXGPU_SCAN_BF16", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_RANGE_MIN_BYTES"):
        os.environ.pop(name, None)
    has_tier = hasattr(L, "rxgpu_scan_tier_range")
    result = {"label": args.label, "dim": dim, "metric": "ip", "queries": nq, "calls_per_round": nq * args.repeat, "rounds": args.rounds, "arch": capi.device_arch(0),
              "library_has_the_range_tier": has_tier, "timing": "host clock around rxgpu_search_range (host to host, synchronous), ms per call",
              "clocks": "not pinned, not read: the two series alternate round by round", "points": []}
    for n in sizes:
        with capi.VectorIndex(capi.METRICS["ip"], dim, device=0) as ix:
            ix.adopt_device_rows(corpus.data_ptr(), n, dim, None, keepalive=(corpus,))
            set_env(VARIANTS[1][1])
            kmax = min(100_000, n // 10)
            kd = ix.search_knn(queries, kmax + 1)[0]                      # exact f32 distances, ascending
            point = {"rows": n, "f32_bytes": n * dim * 4, "shapes": []}
            for shape, hits, inclusive in SHAPES:
                hits = min(hits, kmax)
                radii = [float(kd[qi][hits - 1] if inclusive else kd[qi][hits]) for qi in range(nq)]
                cap = 2 * hits
                bufs = (np.empty(cap, np.float32), np.empty(cap, np.uint32))
                got = {}
                for vname, env in VARIANTS:                               # warm-up (statistics, shadow, buffers) and what each path returns
                    set_env(env)
                    outs = []
                    for qi in range(nq):
                        t = call(ix, qi, radii[qi], inclusive, cap, bufs)
                        outs.append((t, bufs[0][:t].copy(), bufs[1][:t].copy()))
                    got[vname] = outs
                same = all(a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
                           for a, b in zip(got["int8"], got["f32"]))
                times = {vname: [] for vname, _ in VARIANTS}
                for _ in range(args.rounds):
                    for vname, env in VARIANTS:
                        set_env(env)
                        t0 = time.perf_counter()
                        for _rep in range(args.repeat):
                            for qi in range(nq):
                                call(ix, qi, radii[qi], inclusive, cap, bufs)
                        times[vname].append((time.perf_counter() - t0) / (nq * args.repeat) * 1e3)
                slots, cands = {}, []
                for vname, env in VARIANTS:                               # kernel times of the profile slots, in a pass of their own
                    set_env(env)
                    ix.profile_enable(True)
                    for qi in range(nq):
                        call(ix, qi, radii[qi], inclusive, cap, bufs)
                        if vname == "int8":
                            cands.append(ix.last_candidates())
                    slots[vname] = {s: {"launches": c, "ms_per_launch": (ms / c if c else None)}
                                    for s in ("range_i8", "range_rescore", "range") for c, ms in [ix.profile_read(s)]}
                    ix.profile_enable(False)
                entry = {"shape": shape, "hits": [o[0] for o in got["f32"]], "inclusive": inclusive, "cap": cap,
                         **{vname: series(v) for vname, v in times.items()}, "profile_slots": slots,
                         "candidates": [c[0] for c in cands], "candidate_list": cands[0][1] if cands else None,
                         "same_total_rows_and_bits": bool(same), "int8_wins_beyond_spread": max(times["int8"]) < min(times["f32"]),
                         "ratio_of_medians": statistics.median(times["int8"]) / statistics.median(times["f32"])}
                point["shapes"].append(entry)
                print(json.dumps({"rows": n, **{k: v for k, v in entry.items() if k not in ("hits", "candidates")}}), flush=True)
            point["int8_wins_every_shape"] = all(e["int8_wins_beyond_spread"] for e in point["shapes"])
            result["points"].append(point)
    wins = [p["f32_bytes"] for p in result["points"] if p["int8_wins_every_shape"]]
    losing = [p["f32_bytes"] for p in result["points"] if not p["int8_wins_every_shape"]]
    first = min((b for b in wins if all(b > l for l in losing)), default=None)
    result["smallest_winning_f32_bytes"] = first
    result["threshold_bytes"] = max(1 << (first - 1).bit_length(), 1 << 30) if first else None
    result["threshold_rule"] = "smallest size from which the tier wins every shape at every larger measured size, rounded up to a power of two, not below 1 GiB; none: forced-only"
    print(json.dumps({k: v for k, v in result.items() if k != "points"}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
