"""CPU: the rule of a collected streaming session (reindexer_amd/csrc/hnsw_stream_collect_plan.h) — the batch estimate, the stop test and the
bounds — through the stand-alone program tests/cpp/hnsw_stream_collect_plan_cpu.cc: plain, under -fsanitize=address,undefined (a plain
executable, no preload), against the recorded table tests/golden/stream_collect_batches.npz, against the export librxgpu.so offers
(rxgpu_hnsw_stream_collect_batch), and — where the reference tree is present — against StreamingKnnEstimator::EstimateBatchSize itself, its
header compiled in place into a temporary directory."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "hnsw_stream_collect_plan_cpu.cc"
CSRC = ROOT / "reindexer_amd" / "csrc"
TABLE = ROOT / "tests" / "golden" / "stream_collect_batches.npz"


def _build(out, *extra):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", *extra, str(SRC), "-o", str(out)], check=True)
    return out


def _run(exe, *args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("collect_plan") / "hnsw_stream_collect_plan_cpu")


def test_plan_holds_on_the_grid(program):
    assert "ok" in _run(program, "check")


def test_plan_holds_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path / "plan_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")
    assert "ok" in _run(exe, "check")


def test_plan_equals_the_reference_estimator(tmp_path):
    from oracle import pyoracle
    if not pyoracle.reference_tree_available():
        pytest.skip("the reference tree is not on this machine")
    exe = _build(tmp_path / "plan_ref", "-DRX_WITH_REFERENCE", f"-I{pyoracle.REFERENCE_TREE}")
    assert "against the reference's estimator" in _run(exe, "check")


def _table_points(tmp_path):
    z = np.load(TABLE)
    pts = np.stack([z["accepted"], z["presented"], z["needed"]], axis=1)
    f = tmp_path / "points.txt"
    np.savetxt(f, pts, fmt="%d")
    return z, f


def test_plan_equals_the_recorded_table(program, tmp_path):
    z, f = _table_points(tmp_path)
    got = np.array(_run(program, "table", str(f)).split(), np.uint32)
    assert got.shape == z["batch"].shape and z["batch"].shape[0] >= 10000
    assert np.array_equal(got, z["batch"])
    # the table walks the clamp's edges and the cases of the GPU tests
    assert z["batch"].min() == 100 and z["batch"].max() == 800 and np.count_nonzero((z["batch"] > 100) & (z["batch"] < 800)) > 1000


def test_library_export_equals_the_recorded_table():
    from reindexer_amd import capi
    L = capi.lib()
    z = np.load(TABLE)
    idx = np.arange(0, z["batch"].shape[0], 7)
    got = [L.rxgpu_hnsw_stream_collect_batch(int(z["accepted"][i]), int(z["presented"][i]), int(z["needed"][i])) for i in idx]
    assert np.array_equal(np.array(got, np.uint32), z["batch"][idx])
    # the ladder of a collection nothing passes: 100, 100, 200, 400, 800 presented -> the next batch
    assert [L.rxgpu_hnsw_stream_collect_batch(0, p, 10) for p in (10, 100, 200, 400, 800, 1600)] == [100, 800, 800, 800, 800, 800]
    assert [L.rxgpu_hnsw_stream_collect_batch(0, p, 1) for p in (100, 200, 400, 800)] == [100, 200, 400, 800]
    assert L.rxgpu_hnsw_stream_collect_bound(3000, 150, 100) == 949 and L.rxgpu_hnsw_stream_collect_bound(500, 150, 100) == 500
    assert L.rxgpu_hnsw_stream_collect_bound(3000, 10, 1200) == 1209 and L.rxgpu_hnsw_stream_collect_bound(3000, 0, 100) == 0
    assert L.rxgpu_hnsw_stream_collect_calls_bound(3000, 10, 100, 1000) == 1000 and L.rxgpu_hnsw_stream_collect_calls_bound(200, 10, 100, 0) == 201
