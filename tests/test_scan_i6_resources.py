"""CPU: build-time resource check of the 6-bit scan (knn_scan_i6 in reindexer_amd/csrc/knn_scan_i6.hip), after tests/test_range_i8_resources.py.

Every instantiation must stay in registers (0 spilled VGPRs, no scratch) and need no more VGPRs than the budget: knn_scan_i8<metric, NC8,
kEmit = true, kKeep> of the same metric, chunk count and kKeep, compiled in the same run (154 at 768 dims).  The 6-bit kernel holds 9 loads
per step and buffer where that one holds 12, so needing more registers would mean the unpacked codes of more than one row are kept alive."""
import re
import shutil
from pathlib import Path

import pytest

from .test_range_i8_resources import resource_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "reindexer_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
def test_scan_i6_stays_in_registers_and_within_the_int8_budget(tmp_path):
    mine, budget = {}, {}
    for name, u in resource_usage(CSRC / "knn_scan_i6.hip", tmp_path).items():   # rxgpu::knn_scan_i6<metric, NC, emit, keep>
        if m := re.match(r"_ZN5rxgpu11knn_scan_i6ILi(\d)ELi(\d)ELb(\d)ELb(\d)EEEv", name):
            mine[tuple(int(g) for g in m.groups())] = u
    for name, u in resource_usage(CSRC / "knn_scan_i8.hip", tmp_path).items():
        if m := re.match(r"_ZN5rxgpu11knn_scan_i8ILi(\d)ELi(\d)ELb1ELb(\d)EEEv", name):
            budget[tuple(int(g) for g in m.groups())] = u["VGPRs"]
    forms = [(0, 0), (1, 0), (1, 1)]   # the seed pass, the timed scan, the recording scan
    assert set(mine) == {(metric, nc, e, k) for metric in (0, 1, 2) for nc in (1, 2, 3, 4) for e, k in forms}, sorted(mine)
    assert set(budget) == {(metric, nc, k) for metric in (0, 1, 2) for nc in (1, 2, 3, 4) for k in (0, 1)}, sorted(budget)
    for key in sorted(mine):
        metric, nc, emit, keep = key
        u, most = mine[key], budget[(metric, nc, keep)]
        print(f"knn_scan_i6{key}: {u['VGPRs']} VGPRs (knn_scan_i8: {most})")
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (key, u)
        assert u["VGPRs"] <= most, (key, u["VGPRs"], most)
