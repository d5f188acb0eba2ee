"""CPU: build-time resource check of the single-workgroup kernels around the pruned single-query scan: knn_merge_lists and knn_merge_final
(reindexer_amd/csrc/knn_merge.hip) and knn_query_prep_i8 (knn_batched.hip); and of the range and distance kernels of knn_range.hip.

As tests/test_range_i8_resources.py: hipcc cross-compiles gfx950 without a GPU and `-Rpass-analysis=kernel-resource-usage` prints what the code
object header will say.  These kernels are latency chains of one workgroup; a spill would put scratch round trips into them.  Every
instantiation must stay in registers (knn_query_prep_i8 now holds a lane's 16 query elements there), and the merge kernels may not need more
static LDS than before the selections were added: 4096 keys of 8 bytes, 4096 payloads of 4 and one counter word."""
import re
import shutil
from pathlib import Path

import pytest

from tests.test_range_i8_resources import resource_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "reindexer_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MERGE_LDS_MAX = -(-(4096 * 8 + 4096 * 4 + 4) // 8) * 8   # the remark reports the block's allocation, a multiple of 8 bytes: 49160 before too


def instantiations(usage: dict, kernel: str) -> dict:
    return {name: u for name, u in usage.items() if re.match(rf"_ZN5rxgpu\d+{kernel}I", name)}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
def test_merge_kernels_stay_in_registers_and_in_their_lds(tmp_path):
    usage = resource_usage(CSRC / "knn_merge.hip", tmp_path)
    for kernel in ("knn_merge_lists", "knn_merge_final"):
        found = instantiations(usage, kernel)
        assert len(found) == 2, (kernel, sorted(found))   # WaveTopK, WaveTopK2
        for name, u in found.items():
            print(f"{name}: {u['VGPRs']} VGPRs, {u['LDS Size']} bytes of LDS")
            assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (name, u)
            assert u["LDS Size"] <= MERGE_LDS_MAX, (name, u["LDS Size"])


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
def test_query_prep_i8_stays_in_registers(tmp_path):
    found = instantiations(resource_usage(CSRC / "knn_batched.hip", tmp_path), "knn_query_prep_i8")
    assert len(found) == 3, sorted(found)   # L2, IP, cosine
    for name, u in found.items():
        print(f"{name}: {u['VGPRs']} VGPRs")
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (name, u)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
def test_range_kernels_stay_in_registers(tmp_path):
    """The three range kernels are one body (range_body) with the row lookup passed in: no form of it may cost a spill or scratch."""
    usage = resource_usage(CSRC / "knn_range.hip", tmp_path)
    for kernel in ("knn_range", "knn_range_subset", "knn_range_rescore", "knn_distances"):
        found = instantiations(usage, kernel)
        assert len(found) == 3, (kernel, sorted(found))   # L2, IP, cosine
        for name, u in found.items():
            print(f"{name}: {u['VGPRs']} VGPRs")
            assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (name, u)
