"""CPU: the kernels of level 1 of the batched HNSW build (hnsw_build_upper.hip) from the built object.  They are copies between the
level-1 blocks and the dense view: no spills, no scratch memory, and no LDS — hnsw_build_plan.h counts none for them, the selection and
back-link kernels that run on the view keep the LDS tests/test_hnsw_build_resources.py pins."""
import pytest

from .test_kernel_resources import LLVM_BIN, ROOT, built_kernel_metadata

KERNELS = ("hnsw_upper_view_gather", "hnsw_upper_view_store", "hnsw_upper_view_store_ids", "hnsw_upper_pack_rows")


@pytest.mark.skipif(not (LLVM_BIN / "llvm-readelf").exists(), reason="needs the ROCm llvm tools")
def test_view_kernels_stay_in_registers_without_lds(tmp_path):
    obj = ROOT / "reindexer_amd" / "build" / "obj" / "hnsw_build_upper.o"
    if not obj.exists():
        from reindexer_amd import build
        build.build_device()
    meta = built_kernel_metadata(obj, tmp_path)
    assert len(meta) == len(KERNELS), sorted(meta)
    for want in KERNELS:
        hits = [k for k in meta if want in k and (want != "hnsw_upper_view_store" or "store_ids" not in k)]
        assert len(hits) == 1, (want, sorted(meta))
        v = meta[hits[0]]
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (want, v)
        assert v["group_segment_fixed_size"] == 0, (want, v)
        assert v["vgpr_count"] <= 32, (want, v)
    # no kernel of this unit carries a name tests/test_hnsw_build_resources.py counts in hnsw_build.o
    assert not [k for k in meta if "hnsw_build_select" in k or "hnsw_build_backlink" in k]
