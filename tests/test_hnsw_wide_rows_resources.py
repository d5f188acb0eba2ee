"""CPU: the HNSW search kernels over float rows of 1024 and 1536 components (NB = 16 and 24: batch_distances_wide, hnsw_search_core.hip.h),
from the built objects.  A row is read in chunks so that the search's own state stays in registers beside it: no instantiation may spill
VGPRs or use scratch memory, and the throughput form (one wavefront per search, big batches) keeps at least four wavefronts per SIMD
(<= 128 VGPRs)."""
import re

import pytest

from .test_kernel_resources import LLVM_BIN, ROOT, built_kernel_metadata

pytestmark = pytest.mark.skipif(not (LLVM_BIN / "llvm-readelf").exists(), reason="needs the ROCm llvm tools")
THROUGHPUT_VGPRS = 128


def _meta(name, tmp_path):
    obj = ROOT / "reindexer_amd" / "build" / "obj" / name
    if not obj.exists():
        from reindexer_amd import build
        build.build_device()
    return built_kernel_metadata(obj, tmp_path)


def _in_registers(kernels):
    for name, v in kernels.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)


@pytest.mark.parametrize("nb", [16, 24])
def test_wide_search_and_team_kernels(tmp_path, nb):
    meta = _meta("hnsw_search.o", tmp_path)
    # hnsw_search_kernel<kMetric, kGlobalCand, NB, kLatency, kSq8, kSorted, kDel>, float rows: kSq8 false
    search = {k: v for k, v in meta.items() if re.search(rf"hnsw_search_kernelILi[012]ELb[01]ELi{nb}ELb[01]ELb0ELi[0-4]ELb[01]EE", k)}
    # 3 metrics x (heaps in LDS and with global candidates, throughput and latency form each = 4; lists: 2 sizes bare + 3 with deleted nodes, two forms each = 10)
    assert len(search) == 3 * 14, sorted(search)
    _in_registers(search)
    # hnsw_team_kernel<kMetric, NB, kSorted, kDel, kTeam>
    team = {k: v for k, v in meta.items() if re.search(rf"hnsw_team_kernelILi[012]ELi{nb}ELi[2-4]ELb[01]ELi4EE", k)}
    assert len(team) == 3 * 5, sorted(team)
    _in_registers(team)
    helper = {k: v for k, v in meta.items() if re.search(rf"hnsw_helper_kernelILi[012]ELi{nb}ELb0EE", k)}
    assert len(helper) == 3, sorted(helper)
    _in_registers(helper)
    throughput = {k: v for k, v in search.items() if re.search(rf"ILi[012]ELb0ELi{nb}ELb0ELb0ELi2ELb0EE", k)}
    assert len(throughput) == 3, sorted(throughput)
    for name, v in throughput.items():
        assert v["vgpr_count"] <= THROUGHPUT_VGPRS, (name, v)


def test_wide_resident_kernels(tmp_path):
    meta = _meta("hnsw_server.o", tmp_path)
    wide = {k: v for k, v in meta.items() if "hnsw_server_wide_kernel" in k}
    # 3 metrics x 2 list classes x bare / deleted x 2 sizes
    assert len(wide) == 24, sorted(wide)
    for nb in (16, 24):
        assert sum(1 for k in wide if re.search(rf"hnsw_server_wide_kernelILi[012]ELi{nb}ELi[24]ELb[01]ELi4EE", k)) == 12, (nb, sorted(wide))
    _in_registers(wide)
