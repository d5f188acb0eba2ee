"""CPU: the entry points of the collected streaming session are declared in include/rxgpu.h, bound in capi.py and exported by librxgpu.so,
the host library exports its half, and the ABI version stays 2 (the calls are additions) — the extension of tests/test_abi_symbols.py for
this feature.  No compute calls."""
import ctypes

from .test_abi_symbols import header_symbols

NEW = ["rxgpu_hnsw_collect_knn", "rxgpu_hnsw_collect_knn_sq8", "rxgpu_hnsw_stream_collect", "rxgpu_hnsw_stream_collect_batch", "rxgpu_hnsw_stream_collect_bound", "rxgpu_hnsw_stream_collect_calls_bound"]


def test_collect_entry_points_are_declared_bound_and_exported():
    from reindexer_amd import capi
    declared = header_symbols()
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in NEW:
        assert name in declared and name in capi.declared_symbols(), name
        assert hasattr(lib, name), f"librxgpu.so does not export {name}"
    for name in ("hnsw_stream", "hnsw_stream_sq8", "hnsw_collect_knn", "hnsw_collect_knn_sq8"):
        assert hasattr(capi.VectorIndex, name), name
    for name in ("next", "collect", "close"):
        assert hasattr(capi.HnswStream, name), name
    lib.rxgpu_abi_version.restype = ctypes.c_int
    assert lib.rxgpu_abi_version() == 2


def test_host_library_exports_the_collection():
    from reindexer_amd import hostapi
    lib = hostapi.lib()
    for name in ("rxhost_hnsw_stream_collect", "rxhost_hnsw_search_knn_streamed"):
        assert hasattr(lib, name), name
    assert hasattr(hostapi.GpuHnswMap, "search_knn_streamed") and hasattr(hostapi._HnswStream, "collect")
