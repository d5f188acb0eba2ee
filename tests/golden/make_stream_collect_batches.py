"""Writes tests/golden/stream_collect_batches.npz: (accepted, presented, needed) -> the batch StreamingKnnEstimator::EstimateBatchSize
(cpp_src/core/nsselecter/knn_streaming_estimator.h:26-38) answers — recorded results, data only.  The points: a grid over the clamp's
edges plus seeded random draws with accepted <= 2000, presented <= 800 000, needed <= 2000.  The batches come from the reference's own
estimator: tests/cpp/hnsw_stream_collect_plan_cpu.cc built with -DRX_WITH_REFERENCE against the reference tree (its `reftable` mode), so the
script runs only where that tree is present.

    python tests/golden/make_stream_collect_batches.py
"""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def points():
    rng = np.random.default_rng(20261)
    edge = [0, 1, 2, 3, 9, 10, 11, 99, 100, 101, 149, 150, 151, 799, 800, 801, 1999, 2000]
    pres = edge + [2988, 3000, 6000, 79999, 80000, 800000]
    grid = np.array([(a, p, n) for a in edge for p in pres for n in edge if n >= 1], np.uint64)
    rnd = np.stack([rng.integers(0, 2001, 20000), rng.integers(0, 800001, 20000), rng.integers(1, 2001, 20000)], axis=1).astype(np.uint64)
    # the region where the estimate is between the clamps: presented / accepted * remaining in 100 .. 800
    acc = rng.integers(1, 2001, 20000)
    need = np.minimum(acc + rng.integers(1, 200, 20000), 2000)
    amp = rng.uniform(1, 50, 20000)
    mid = np.stack([acc, np.minimum((acc * amp).astype(np.int64), 800000), need], axis=1).astype(np.uint64)
    return np.concatenate([grid, rnd, mid])


def main():
    from oracle import pyoracle
    if not pyoracle.reference_tree_available():
        raise SystemExit("the reference tree is needed to record the table")
    pts = points()
    with tempfile.TemporaryDirectory() as tmp:
        exe, f = Path(tmp) / "plan_ref", Path(tmp) / "points.txt"
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'reindexer_amd' / 'csrc'}", "-DRX_WITH_REFERENCE", f"-I{pyoracle.REFERENCE_TREE}",
                        str(ROOT / "tests" / "cpp" / "hnsw_stream_collect_plan_cpu.cc"), "-o", str(exe)], check=True)
        np.savetxt(f, pts, fmt="%d")
        out = subprocess.run([str(exe), "reftable", str(f)], capture_output=True, text=True, check=True).stdout
    batch = np.array(out.split(), np.uint32)
    assert batch.shape[0] == pts.shape[0]
    np.savez_compressed(ROOT / "tests" / "golden" / "stream_collect_batches.npz", accepted=pts[:, 0], presented=pts[:, 1], needed=pts[:, 2], batch=batch)
    print(f"{pts.shape[0]} points; batches {batch.min()} .. {batch.max()}, {np.count_nonzero((batch > 100) & (batch < 800))} between the clamps")


if __name__ == "__main__":
    main()
