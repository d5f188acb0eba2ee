"""CPU: the entry points of the filtered HNSW search are declared in include/rxgpu.h, bound in capi.py and exported by librxgpu.so, the
host library exports its half, and the ABI version stays 2 (the calls are additions) — the extension of tests/test_abi_symbols.py for this
feature.  No compute calls."""
import ctypes

from .test_abi_symbols import header_symbols

NEW = ["rxgpu_hnsw_search_knn_filtered", "rxgpu_hnsw_search_knn_sq8_filtered"]


def test_filtered_entry_points_are_declared_bound_and_exported():
    from reindexer_amd import capi
    declared = header_symbols()
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in NEW:
        assert name in declared and name in capi.declared_symbols(), name
        assert hasattr(lib, name), f"librxgpu.so does not export {name}"
    for name in ("hnsw_search_knn_filtered", "hnsw_search_knn_sq8_filtered"):
        assert hasattr(capi.VectorIndex, name), name
    lib.rxgpu_abi_version.restype = ctypes.c_int
    assert lib.rxgpu_abi_version() == 2


def test_host_library_exports_the_filtered_search():
    from reindexer_amd import hostapi
    lib = hostapi.lib()
    for name in ("rxhost_hnsw_search_knn_filtered", "rxhost_hnsw_filtered_stats"):
        assert hasattr(lib, name), name
    for name in ("search_knn_filtered", "filtered_stats"):
        assert hasattr(hostapi.GpuHnswMap, name), name
