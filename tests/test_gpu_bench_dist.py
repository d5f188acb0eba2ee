"""-m gpu: bench.py's N > 1 code path on the one GPU there is — launched the way the driver launches it (python -m torch.distributed.run, one
rank) with RXGPU_BENCH_FORCE_DIST=1: RCCL process group, local scan -> all_gather_into_tensor of the per-shard lists -> knn_merge_shards, the
barrier + max-over-ranks timing, ONE JSON line from rank 0 (the contract the SCALE run reads).  Small corpus: this checks the path, not a number."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_distributed_path_on_one_rank(rxgpu, scaling, tmp_path):
    env = dict(os.environ, RXGPU_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--rows", "200000", "--total-rows", "200000", "--scaling", scaling,
           "--no-cpu", "--batch", "0", "--hnsw-rows", "0", "--hybrid-docs", "0", "--ft-packed-words", "0", "--full-json", str(tmp_path / "full.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env, cwd=str(tmp_path))
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["metric"] == "knn_queries_per_sec" and out["n_gpus"] == 1 and out["steps"] == 6 and out["warmup"] == 2 and out["scaling"] == scaling
    assert out["config"]["rccl_ranks"] == 1 and out["config"]["sharding"].startswith("row-range shards")
    assert out["value"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) / out["value"] < 1e-3
    assert out["roofline"]["launches"] == 6 and out["roofline"]["frac"] > 0


def test_bench_plain_run_dumps_last_step(rxgpu, tmp_path):
    """A plain run (no --full): the headline steps only, no extra leg; --dump-outputs holds the last timed step's list, which a fresh
    search of the same seeded query over the same seeded corpus reproduces bit for bit."""
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--rows", "100000", "--dim", "128",
           "--dump-outputs", str(tmp_path / "dump"), "--full-json", str(tmp_path / "full.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=str(tmp_path))
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["steps"] == 5 and out["warmup"] == 2 and out["roofline"]["launches"] == 5
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) / out["value"] < 1e-3
    for leg in ("sharded_in_process", "batched", "pruned_scan", "prefilter", "cpu_baseline", "parity", "hybrid", "ft_packed", "hnsw"):
        assert leg not in out, leg
    import numpy as np
    import torch
    dist, row = np.load(tmp_path / "dump" / "knn_dist.npy"), np.load(tmp_path / "dump" / "knn_row.npy")
    assert dist.dtype == np.float32 and row.dtype == np.float64 and dist.shape == row.shape == (1, 11)
    # bench.py's inputs, rebuilt: corpus chunk 0 (seed 20260924 * 1_000_003), queries from seed 7 in a (256, 128) block; last step = query 6
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(20260924 * 1_000_003)
    corpus = torch.empty((100000, 128), dtype=torch.float32, device=dev).normal_(0.0, 0.25, generator=g)
    g.manual_seed(7)
    queries = torch.empty((256, 128), dtype=torch.float32, device=dev).normal_(0.0, 0.25, generator=g)
    with rxgpu.VectorIndex(rxgpu.METRIC_IP, 128, device=0) as ix:
        ix.adopt_device_rows(corpus.data_ptr(), 100000, 128, None, keepalive=(corpus,))
        d, rr, _ = ix.search_knn(queries[6:7].cpu().numpy(), 11)
    assert np.array_equal(rr.astype(np.int64), row.astype(np.int64)) and np.array_equal(d.view(np.uint32), dist.view(np.uint32))
