"""CPU: the resident HNSW search kernel over SQ8 codes (hnsw_server_sq8_kernel, hnsw_server.hip) from the built object.  Its sorted list
lives in registers for as long as the kernel stays on the chip — up to its lifetime, search after search: no instantiation may spill VGPRs or
use scratch memory."""
import pytest

from .test_kernel_resources import LLVM_BIN, ROOT, built_kernel_metadata


@pytest.mark.skipif(not (LLVM_BIN / "llvm-readelf").exists(), reason="needs the ROCm llvm tools")
def test_resident_sq8_kernels_stay_in_registers(tmp_path):
    obj = ROOT / "reindexer_amd" / "build" / "obj" / "hnsw_server.o"
    if not obj.exists():
        from reindexer_amd import build
        build.build_device()
    meta = built_kernel_metadata(obj, tmp_path)
    sq8 = {k: v for k, v in meta.items() if "hnsw_server_sq8_kernel" in k}
    # 3 metrics x 2 list sizes x (6 embedding sizes of a bare graph + 2 of a graph with deleted nodes)
    assert len(sq8) == 48, sorted(sq8)
    for name, v in sq8.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
    # the float kernels beside them share the protocol code: still there, still without scratch
    floats = {k: v for k, v in meta.items() if "hnsw_server_kernel" in k}
    assert len(floats) == 36, sorted(floats)
    for name, v in floats.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
