"""CPU: the HNSW search kernels under an allowed-rows bitmap (reindexer_amd/csrc/hnsw_filtered.hip), from the built object: the
instantiation set the pick header states (hnsw_filtered_kernel_exists), counted by name, and the bar every HNSW search kernel here meets —
no instantiation spills VGPRs or uses scratch memory.  The unit holds nothing of the unfiltered families."""
import re

import pytest

from .test_kernel_resources import LLVM_BIN, ROOT, built_kernel_metadata

pytestmark = pytest.mark.skipif(not (LLVM_BIN / "llvm-readelf").exists(), reason="needs the ROCm llvm tools")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    obj = ROOT / "reindexer_amd" / "build" / "obj" / "hnsw_filtered.o"
    if not obj.exists():
        from reindexer_amd import build
        build.build_device()
    return built_kernel_metadata(obj, tmp_path_factory.mktemp("hnsw_filtered"))


def _in_registers(kernels):
    for name, v in kernels.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)


def test_single_wavefront_kernels(meta):
    # hnsw_filtered_kernel<kMetric, kGlobalCand, NB, kSq8, kSorted>
    single = {k: v for k, v in meta.items() if "hnsw_filtered_kernel" in k}
    # 3 metrics x floats / codes x (generic, 128, 768) x (heaps in LDS, heaps with global candidates, lists of 2 / 3 / 4 entries a lane)
    assert len(single) == 3 * 2 * 3 * 5, sorted(single)
    for nb in (0, 2, 12):
        for sq8 in (0, 1):
            heaps = [k for k in single if re.search(rf"hnsw_filtered_kernelILi[012]ELb[01]ELi{nb}ELb{sq8}ELi0EE", k)]
            lists = [k for k in single if re.search(rf"hnsw_filtered_kernelILi[012]ELb0ELi{nb}ELb{sq8}ELi[234]EE", k)]
            assert (len(heaps), len(lists)) == (6, 9), (nb, sq8, sorted(heaps), sorted(lists))
    _in_registers(single)


def test_team_kernels(meta):
    # hnsw_filtered_team_kernel<kMetric, NB, kSorted>: floats at 128 and 768, the three lists
    team = {k: v for k, v in meta.items() if "hnsw_filtered_team_kernel" in k}
    assert len(team) == 3 * 2 * 3, sorted(team)
    for nb in (2, 12):
        assert sum(1 for k in team if re.search(rf"hnsw_filtered_team_kernelILi[012]ELi{nb}ELi[234]EE", k)) == 9, (nb, sorted(team))
    _in_registers(team)


def test_nothing_else_lives_in_the_unit(meta):
    assert all("hnsw_filtered_kernel" in k or "hnsw_filtered_team_kernel" in k for k in meta), sorted(meta)
