#!/usr/bin/env python3
"""Where do the bf16-pruned and the int8-pruned single-query scans start to pay?  (GPU box only.)

    python tools/scan_policy_crossover.py [--dim 768] [--rows 100000,...,10000000] [--rounds 5] [--queries 40] [--out FILE]
    python tools/scan_policy_crossover.py --ab RXGPU_SCAN_BF16_WG_PER_CU=2,3,4 --rows 10000000   # a tuning knob of the bf16 scan, same method
    python tools/scan_policy_crossover.py --ab RXGPU_SCAN_I8_WG_PER_CU=2,3 --rows 10000000       # ... of the int8 scan (a knob named RXGPU_SCAN_I8_*)

One process, one resident corpus per size; per size the four series (RXGPU_SCAN_BF16=0, =1, RXGPU_SCAN_I8=1 with RXGPU_SCAN_BF16 unset, and
RXGPU_SCAN_I6=1 with both unset: the 6-bit front of the int8 tier; all read by the library on every call; the int8 and 6-bit series only at
dimensions those serve) ALTERNATE,
--rounds times each, every round timing --queries single-query searches through rxgpu_search_knn_device with one synchronisation at the end
(what bench.py calls ms_per_step).  Reported per size and series: median, min, max of the rounds.  The pruned path "wins" at a size when its
worst round beats the f32 path's best round; the automatic threshold in rxgpu_knn_chains.hip (kPrunedAutoMinBytes) is the smallest such size in
bytes of f32 rows, rounded up to a power of two, and never below 1 GiB.  The int8 tier's threshold (kPrunedI8AutoMinBytes) follows the same
rule against the bf16 series, and the 6-bit front's (kPrunedI6AutoMinBytes) against the int8 series and every other one.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from reindexer_amd import capi  # noqa: E402


def time_round(ix, q, out_d, out_r, dim, kk, nq, stream, device):
    t0 = time.perf_counter()
    for i in range(nq):
        ix.search_knn_device(q.data_ptr() + i * dim * 4, 1, kk, out_d.data_ptr() + i * kk * 4, out_r.data_ptr() + i * kk * 4, None, stream)
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) / nq * 1e3


def set_env(env):
    for k, v in env.items():   # None: unset
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def series(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": [round(x, 5) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rows", default="100000,200000,350000,500000,700000,1000000,1400000,2000000,4000000,10000000")
    ap.add_argument("--metric", default="ip")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--queries", type=int, default=40)
    ap.add_argument("--ab", default=None, metavar="VAR=a,b,..", help="alternate these values of an environment knob of the pruned scan "
                                                                     "(RXGPU_SCAN_BF16=1 throughout) instead of the 0 / 1 switch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    kk = args.k + 1
    stream = torch.cuda.current_stream(device).cuda_stream
    g = torch.Generator(device=device)
    g.manual_seed(1)
    sizes = sorted(int(x) for x in args.rows.split(","))
    corpus = torch.empty((sizes[-1], args.dim), dtype=torch.float32, device=device)
    for a in range(0, sizes[-1], 1 << 20):
        corpus[a:a + (1 << 20)].normal_(0.0, 0.25, generator=g)
    q = torch.empty((args.queries, args.dim), dtype=torch.float32, device=device).normal_(0.0, 0.25, generator=g)
    d_inv = None
    if args.metric == "cosine":
        d_inv = 1.0 / torch.linalg.vector_norm(corpus, dim=1)
        q = q / torch.linalg.vector_norm(q, dim=1, keepdim=True)
    out_d = torch.empty((args.queries, kk), dtype=torch.float32, device=device)
    out_r = torch.empty((args.queries, kk), dtype=torch.int32, device=device)
    if args.ab:
        knob, vals = args.ab.split("=", 1)
        base = {"RXGPU_SCAN_BF16": None, "RXGPU_SCAN_I8": "1"} if knob.startswith("RXGPU_SCAN_I8") else {"RXGPU_SCAN_BF16": "1", "RXGPU_SCAN_I8": None}
        variants = [("%s=%s" % (knob, w), {**base, knob: w}) for w in vals.split(",")]
    else:
        variants = [("f32", {"RXGPU_SCAN_BF16": "0", "RXGPU_SCAN_I8": None, "RXGPU_SCAN_I6": None}),
                    ("pruned", {"RXGPU_SCAN_BF16": "1", "RXGPU_SCAN_I8": None, "RXGPU_SCAN_I6": None})]
        os.environ.pop("RXGPU_SCAN_BF16", None)
        os.environ["RXGPU_SCAN_I8"] = "1"
        if capi.scan_tier(1000, args.dim) == 2:
            variants.append(("int8", {"RXGPU_SCAN_BF16": None, "RXGPU_SCAN_I8": "1", "RXGPU_SCAN_I6": None}))
        os.environ.pop("RXGPU_SCAN_I8", None)
        os.environ["RXGPU_SCAN_I6"] = "1"
        if capi.scan_i6(1000, args.dim):
            variants.append(("i6", {"RXGPU_SCAN_BF16": None, "RXGPU_SCAN_I8": None, "RXGPU_SCAN_I6": "1"}))
    result = {"dim": args.dim, "metric": args.metric, "k": args.k, "queries_per_round": args.queries, "rounds": args.rounds,
              "arch": capi.device_arch(0), "ab": args.ab, "sizes": []}
    for n in sizes:
        with capi.VectorIndex(capi.METRICS[args.metric], args.dim, device=0) as ix:
            ix.adopt_device_rows(corpus.data_ptr(), n, args.dim, d_inv.data_ptr() if d_inv is not None else None, keepalive=(corpus, d_inv))
            times = {name: [] for name, _ in variants}
            for name, env in variants:   # warm-up: statistics, shadow, buffers
                set_env(env)
                time_round(ix, q, out_d, out_r, args.dim, kk, 4, stream, device)
            for _ in range(args.rounds):
                for name, env in variants:
                    set_env(env)
                    times[name].append(time_round(ix, q, out_d, out_r, args.dim, kk, args.queries, stream, device))
            entry = {"rows": n, "f32_bytes": n * args.dim * 4, **{name: series(v) for name, v in times.items()}}
            if not args.ab:
                entry["pruned_wins_beyond_spread"] = max(times["pruned"]) < min(times["f32"])
                if "int8" in times:
                    entry["int8_wins_beyond_spread"] = max(times["int8"]) < min(times["pruned"]) and max(times["int8"]) < min(times["f32"])
                if "i6" in times:
                    entry["i6_wins_beyond_spread"] = all(max(times["i6"]) < min(v) for name, v in times.items() if name != "i6")
            result["sizes"].append(entry)
            print(json.dumps(entry), flush=True)
    for k_ in ["RXGPU_SCAN_BF16", "RXGPU_SCAN_I8", "RXGPU_SCAN_I6"] + ([args.ab.split("=", 1)[0]] if args.ab else []):
        os.environ.pop(k_, None)
    if not args.ab:
        wins = [e["f32_bytes"] for e in result["sizes"] if e["pruned_wins_beyond_spread"]]
        losing_above = [e["f32_bytes"] for e in result["sizes"] if not e["pruned_wins_beyond_spread"]]
        first = min((b for b in wins if all(b > l for l in losing_above)), default=None)   # smallest size from which it wins at every larger one
        result["smallest_winning_f32_bytes"] = first
        if first:
            p2 = 1 << (first - 1).bit_length()
            result["threshold_bytes"] = max(p2, 1 << 30)
            result["threshold_rule"] = "smallest winning size rounded up to a power of two, not below 1 GiB"
        if any("int8_wins_beyond_spread" in e for e in result["sizes"]):   # the int8 tier against the bf16 tier (and the f32 scan), same rule
            wins = [e["f32_bytes"] for e in result["sizes"] if e["int8_wins_beyond_spread"]]
            losing_above = [e["f32_bytes"] for e in result["sizes"] if not e["int8_wins_beyond_spread"]]
            first = min((b for b in wins if all(b > l for l in losing_above)), default=None)
            result["int8_smallest_winning_f32_bytes"] = first
            if first:
                result["int8_threshold_bytes"] = max(1 << (first - 1).bit_length(), 1 << 30)
        if any("i6_wins_beyond_spread" in e for e in result["sizes"]):   # the 6-bit front against every other series, same rule
            wins = [e["f32_bytes"] for e in result["sizes"] if e["i6_wins_beyond_spread"]]
            losing_above = [e["f32_bytes"] for e in result["sizes"] if not e["i6_wins_beyond_spread"]]
            first = min((b for b in wins if all(b > l for l in losing_above)), default=None)
            result["i6_smallest_winning_f32_bytes"] = first
            if first:
                result["i6_threshold_bytes"] = max(1 << (first - 1).bit_length(), 1 << 30)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({k_: v for k_, v in result.items() if k_ != "sizes"}))


if __name__ == "__main__":
    main()
