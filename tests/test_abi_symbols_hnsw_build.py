"""CPU: the entry points of the batched HNSW build are declared in include/rxgpu.h, bound in capi.py and exported by librxgpu.so (no
compute calls) — the extension of tests/test_abi_symbols.py for what this feature adds."""
import ctypes

from .test_abi_symbols import header_symbols

NEW = ["rxgpu_hnsw_link_batch", "rxgpu_hnsw_patch_upper", "rxgpu_hnsw_read_build_stats", "rxgpu_hnsw_read_links0"]


def test_build_entry_points_are_declared_bound_and_exported():
    from reindexer_amd import capi
    declared = header_symbols()
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in NEW:
        assert name in declared and name in capi.declared_symbols(), name
        assert hasattr(lib, name), f"librxgpu.so does not export {name}"


def test_host_library_exports_the_build_entry_points():
    from reindexer_amd import hostapi
    lib = hostapi.lib()
    for name in ("rxhost_hnsw_add_bulk", "rxhost_hnsw_pending_rows", "rxhost_hnsw_build_stats", "rxhost_graph_append_unlinked", "rxhost_graph_link_stored",
                 "rxhost_graph_link_upper", "rxhost_graph_set_links0", "rxhost_graph_pending_from"):
        assert hasattr(lib, name), name
