"""CPU: build-time resource check of the int8 range scans (knn_range_i8 / knn_range_i8_subset in reindexer_amd/csrc/knn_scan_i8.hip).

hipcc cross-compiles gfx950 without a GPU; `-Rpass-analysis=kernel-resource-usage` prints what the code object header will say.  Every
instantiation must stay in registers (0 spilled VGPRs, no scratch) and need no more VGPRs than knn_scan_i8<metric, NC8, kEmit = true,
kKeep = false> of the same metric and NC8, compiled in the same run: that kernel is the one the range forms were cut from, they carry
strictly less state (no top list, no emit plan), so needing more registers would mean the double buffer of the loads was lost."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "reindexer_amd" / "csrc" / "knn_scan_i8.hip"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def resource_usage(src: Path, tmp: Path) -> dict:
    from reindexer_amd.build import HIP_FLAGS
    flags = [f for f in HIP_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([HIPCC, *flags, "-c", str(src), "-o", str(tmp / (src.stem + ".o")), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
def test_range_scans_stay_in_registers_and_below_the_knn_scan(tmp_path):
    usage = resource_usage(SRC, tmp_path)
    # Itanium names: rxgpu::knn_scan_i8<metric, NC8, emit, keep>, rxgpu::knn_range_i8<metric, NC8>, rxgpu::knn_range_i8_subset<metric, NC8>
    parent, whole, subset = {}, {}, {}
    for name, u in usage.items():
        if m := re.match(r"_ZN5rxgpu11knn_scan_i8ILi(\d)ELi(\d)ELb1ELb0EEEv", name):
            parent[(int(m.group(1)), int(m.group(2)))] = u
        elif m := re.match(r"_ZN5rxgpu12knn_range_i8ILi(\d)ELi(\d)EEEv", name):
            whole[(int(m.group(1)), int(m.group(2)))] = u
        elif m := re.match(r"_ZN5rxgpu19knn_range_i8_subsetILi(\d)ELi(\d)EEEv", name):
            subset[(int(m.group(1)), int(m.group(2)))] = u
    shapes = {(metric, nc8) for metric in (0, 1, 2) for nc8 in (1, 2, 3, 4)}
    assert set(parent) == shapes and set(whole) == shapes and set(subset) == shapes, (sorted(parent), sorted(whole), sorted(subset))
    for key in sorted(shapes):
        for form, u in (("knn_range_i8", whole[key]), ("knn_range_i8_subset", subset[key])):
            print(f"{form}{key}: {u['VGPRs']} VGPRs (knn_scan_i8: {parent[key]['VGPRs']})")
            assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (form, key, u)
            assert u["VGPRs"] <= parent[key]["VGPRs"], (form, key, u["VGPRs"], parent[key]["VGPRs"])
