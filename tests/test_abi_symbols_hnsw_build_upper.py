"""CPU: the entry points of level 1 of the batched HNSW build are declared in include/rxgpu.h, bound in capi.py and exported by
librxgpu.so, and the host library exports its half (no compute calls) — the extension of tests/test_abi_symbols.py for this feature."""
import ctypes

from .test_abi_symbols import header_symbols

NEW = ["rxgpu_hnsw_link_batch_upper", "rxgpu_hnsw_patch_upper_from", "rxgpu_hnsw_read_level", "rxgpu_hnsw_read_build_upper_stats",
       "rxgpu_hnsw_release_build_view"]


def test_upper_build_entry_points_are_declared_bound_and_exported():
    from reindexer_amd import capi
    declared = header_symbols()
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in NEW:
        assert name in declared and name in capi.declared_symbols(), name
        assert hasattr(lib, name), f"librxgpu.so does not export {name}"
    for name in ("hnsw_link_batch_upper", "hnsw_patch_upper_from", "hnsw_read_level", "hnsw_read_build_upper_stats", "hnsw_release_build_view"):
        assert hasattr(capi.VectorIndex, name), name


def test_host_library_exports_the_upper_build_entry_points():
    from reindexer_amd import hostapi
    lib = hostapi.lib()
    for name in ("rxhost_graph_link_upper", "rxhost_graph_link_upper_from", "rxhost_graph_set_level_lists"):
        assert hasattr(lib, name), name
