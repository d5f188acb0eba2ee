"""CPU: the kernels of the batched HNSW build (hnsw_build.hip) from the built object.  One wavefront orders up to 256 entries in LDS and
walks them against the kept rows: no instantiation may spill VGPRs or use scratch memory, and the static LDS is what
hnsw_build_plan.h counts when it decides whether the kept rows fit beside it."""
import pytest

from .test_kernel_resources import LLVM_BIN, ROOT, built_kernel_metadata

FIXED_LDS = (3 * 256 + 4 * 128) * 4   # hnsw_build_fixed_lds_bytes(): candidate ids / distances / order, kept and heap ids / distances


@pytest.mark.skipif(not (LLVM_BIN / "llvm-readelf").exists(), reason="needs the ROCm llvm tools")
def test_build_kernels_stay_in_registers_and_within_the_lds_budget(tmp_path):
    obj = ROOT / "reindexer_amd" / "build" / "obj" / "hnsw_build.o"
    if not obj.exists():
        from reindexer_amd import build
        build.build_device()
    meta = built_kernel_metadata(obj, tmp_path)
    select = {k: v for k, v in meta.items() if "hnsw_build_select" in k}
    backlink = {k: v for k, v in meta.items() if "hnsw_build_backlink" in k}
    assert len(select) == 6, sorted(select)       # 3 metrics x (rows in LDS, rows from L2)
    assert len(backlink) == 6, sorted(backlink)   # 3 metrics x (first launch, nodes past the cap)
    for name, v in {**select, **backlink}.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == FIXED_LDS, (name, v)   # + (1 + M) rows of dynamic LDS where the plan says they fit in 64 KB
        assert v["vgpr_count"] <= 128, (name, v)
    for k, v in meta.items():
        if "hnsw_build_segments" in k or "hnsw_build_scatter" in k or "hnsw_build_patch_upper" in k:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, (k, v)
