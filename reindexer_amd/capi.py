"""ctypes binding of the C-ABI in include/rxgpu.h (librxgpu.so).

Python here is plumbing for tests / bench / multi-GPU launch only: numpy arrays or torch device pointers in,
numpy arrays out.  There is NO fallback: if the HIP library is missing or fails to load, importing the symbols
raises — a product path must never silently route around the kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "librxgpu.so"

METRIC_L2, METRIC_IP, METRIC_COSINE = 0, 1, 2
METRICS = {"l2": METRIC_L2, "ip": METRIC_IP, "inner_product": METRIC_IP, "cosine": METRIC_COSINE}

RXGPU_OK = 0
RXGPU_ERR_PARAMS = -3
RXGPU_ERR_LOGIC = -4
RXGPU_ERR_NOMEM = -5
RXGPU_ERR_DEVICE = -6
RXGPU_ERR_NOTFOUND = -7
RXGPU_ERR_OVERFLOW = -8

# every symbol include/rxgpu.h declares (tests/test_abi_symbols.py cross-checks this list against the header)
_vp, _u32, _u64, _i, _f = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
_SIGNATURES = {
    "rxgpu_last_error": (C.c_char_p, []),
    "rxgpu_abi_version": (_i, []),
    "rxgpu_device_count": (_i, []),
    "rxgpu_device_arch": (_i, [_i, C.c_char_p, C.c_size_t]),
    "rxgpu_index_create": (_i, [_i, _u32, _u64, _i, C.POINTER(_vp)]),
    "rxgpu_index_destroy": (None, [_vp]),
    "rxgpu_index_create_sharded": (_i, [_i, _u32, _u64, _u32, _vp, C.POINTER(_vp)]),
    "rxgpu_index_shard_count": (_u32, [_vp]),
    "rxgpu_index_shard_rows": (_u64, [_vp]),
    "rxgpu_index_shard_merge_mode": (_i, [_vp]),
    "rxgpu_index_shard_merge_note": (C.c_char_p, [_vp]),
    "rxgpu_index_shard_ranks": (_u32, [_vp]),
    "rxgpu_index_shard_collectives": (_u64, [_vp]),
    "rxgpu_index_shard": (_vp, [_vp, _u32]),
    "rxgpu_index_shard_sync_count": (_i, [_vp]),
    "rxgpu_index_download_row": (_i, [_vp, _u64, _vp, _vp]),
    "rxgpu_index_reserve": (_i, [_vp, _u64]),
    "rxgpu_index_upload_rows": (_i, [_vp, _u64, _u64, _vp, _vp]),
    "rxgpu_index_adopt_device_rows": (_i, [_vp, _vp, _u64, _u32, _vp]),
    "rxgpu_index_move_row": (_i, [_vp, _u64, _u64]),
    "rxgpu_index_truncate": (_i, [_vp, _u64]),
    "rxgpu_index_count": (_u64, [_vp]),
    "rxgpu_index_capacity": (_u64, [_vp]),
    "rxgpu_index_dim": (_u32, [_vp]),
    "rxgpu_index_row_stride": (_u32, [_vp]),
    "rxgpu_index_metric": (_i, [_vp]),
    "rxgpu_index_device": (_i, [_vp]),
    "rxgpu_index_device_bytes": (_u64, [_vp]),
    "rxgpu_search_knn": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "rxgpu_index_upload_row_ids": (_i, [_vp, _u64, _u64, _vp]),
    "rxgpu_index_row_ids_device": (_vp, [_vp]),
    "rxgpu_search_knn_resident": (_i, [_vp, _vp, _u32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u32)]),
    "rxgpu_index_resident_contexts": (_u32, [_vp]),
    "rxgpu_search_knn_device": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "rxgpu_scan_policy": (_i, [_u64, _u32, _u32, _i, _i]),
    "rxgpu_scan_tier": (_i, [_u64, _u32, _u32, _i, _i]),
    "rxgpu_scan_i6": (_i, [_u64, _u32, _u32, _i, _i]),
    "rxgpu_scan_tier_subset": (_i, [_u64, _u32, _u32, _u32, _i, _i]),
    "rxgpu_scan_tier_range": (_i, [_u64, _u32, _i, _i, _i]),
    "rxgpu_index_last_candidates": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "rxgpu_index_inspect": (_i, [_vp, C.c_char_p, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_knn_merge_probe": (_i, [_i, _i, _vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32), C.POINTER(_i)]),
    "rxgpu_search_knn_subset": (_i, [_vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "rxgpu_search_knn_bitmap": (_i, [_vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    "rxgpu_index_set_lists": (_i, [_vp, _u32, _vp, _vp]),
    "rxgpu_search_knn_lists": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u64)]),
    "rxgpu_search_range_lists": (_i, [_vp, _vp, _vp, _u32, C.c_float, _i, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_search_knn_lists_batch": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "rxgpu_ivf_read_batch_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_ivf_batch_default": (_i, [_u32, _u32, _u32]),
    "rxgpu_ivf_assign": (_i, [_vp, _vp, _vp, _u64, _u64, _vp]),
    "rxgpu_ivf_kmeans_step": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "rxgpu_ivf_read_train_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rxgpu_search_knn_subset_device": (_i, [_vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "rxgpu_check_row_list_device": (_i, [_vp, _vp, _u64, _vp, C.POINTER(C.c_int32)]),
    "rxgpu_search_range_subset": (_i, [_vp, _vp, _f, _i, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_merge_shards_device": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "rxgpu_search_range": (_i, [_vp, _vp, _f, _i, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_distances": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "rxgpu_hnsw_attach_graph": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _u32, _u32, C.c_int32, _u32, _u64]),
    "rxgpu_hnsw_update_deleted": (_i, [_vp, _vp, _u64]),
    "rxgpu_hnsw_patch_graph": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _u32, _u64]),
    "rxgpu_hnsw_search_knn": (_i, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "rxgpu_hnsw_search_knn_posted": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "rxgpu_hnsw_distance_blocks": (_i, [_u32, _i, _i, C.POINTER(C.c_int)]),
    "rxgpu_hnsw_server_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_hnsw_server_times": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_hnsw_read_stats4": (_i, [_vp, _vp]),
    "rxgpu_hnsw_attach_sq8": (_i, [_vp, _vp, _vp, _u64, _f]),
    "rxgpu_hnsw_upload_sq8_rows": (_i, [_vp, _u64, _u64, _vp, _vp, _f]),
    "rxgpu_hnsw_link_batch": (_i, [_vp, _u64, _u64, _u32]),
    "rxgpu_hnsw_patch_upper": (_i, [_vp, _u32, _vp, _vp, _vp, C.c_int32, _u32]),
    "rxgpu_hnsw_read_links0": (_i, [_vp, _u64, _u64, _vp]),
    "rxgpu_hnsw_read_build_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rxgpu_hnsw_link_batch_upper": (_i, [_vp, _u64, _u64, _u32, _vp, _u32]),
    "rxgpu_hnsw_patch_upper_from": (_i, [_vp, C.c_int32, _u32, _vp, _vp, _vp, C.c_int32, _u32]),
    "rxgpu_hnsw_read_level": (_i, [_vp, C.c_int32, _u64, _vp, _vp]),
    "rxgpu_hnsw_read_build_upper_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rxgpu_hnsw_release_build_view": (_i, [_vp]),
    "rxgpu_hnsw_quantize_sq8": (_i, [_vp, _u64, _u64, _f, _f, _f, _f]),
    "rxgpu_hnsw_read_sq8_rows": (_i, [_vp, _u64, _u64, _vp, _vp]),
    "rxgpu_hnsw_read_sq8_quantize_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rxgpu_hnsw_search_knn_sq8": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "rxgpu_hnsw_search_knn_filtered": (_i, [_vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    "rxgpu_hnsw_search_knn_sq8_filtered": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    "rxgpu_hnsw_search_knn_sq8_posted": (_i, [_vp, _vp, _f, _f, _u32, _u32, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "rxgpu_hnsw_read_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_hnsw_read_tie_reruns": (_i, [_vp, C.POINTER(_u64)]),
    "rxgpu_hnsw_read_lds_reruns": (_i, [_vp, C.POINTER(_u64)]),
    "rxgpu_hnsw_search_range": (_i, [_vp, _vp, _f, _u32, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_hnsw_search_range_sq8": (_i, [_vp, _vp, _f, _f, _f, _u32, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_hnsw_stream_begin_sq8": (_i, [_vp, _vp, _f, _f, _u32, C.POINTER(_vp)]),
    "rxgpu_hnsw_stream_begin": (_i, [_vp, _vp, _u32, C.POINTER(_vp)]),
    "rxgpu_hnsw_stream_continue": (_i, [_vp, _u32, _vp, _vp, C.POINTER(_u32), C.POINTER(_i)]),
    "rxgpu_hnsw_stream_end": (None, [_vp]),
    "rxgpu_hnsw_stream_collect": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(_u64),
                                       C.POINTER(_u64), C.POINTER(C.c_int32), C.POINTER(_u32), _vp]),
    "rxgpu_hnsw_collect_knn": (_i, [_vp, _vp, _u32, _vp, _u64, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(_u64),
                                    C.POINTER(_u64), C.POINTER(C.c_int32), C.POINTER(_u32), _vp]),
    "rxgpu_hnsw_collect_knn_sq8": (_i, [_vp, _vp, _f, _f, _u32, _vp, _u64, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_u32),
                                        C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_int32), C.POINTER(_u32), _vp]),
    "rxgpu_hnsw_stream_collect_batch": (_u32, [_u64, _u64, _u64]),
    "rxgpu_hnsw_stream_collect_bound": (_u64, [_u64, _u32, _u32]),
    "rxgpu_hnsw_stream_collect_calls_bound": (_u64, [_u64, _u32, _u32, _u32]),
    "rxgpu_ft_create": (_i, [_u32, _i, C.POINTER(_vp)]),
    "rxgpu_ft_create_sharded": (_i, [_u32, _u32, _vp, C.POINTER(_vp)]),
    "rxgpu_ft_shard_count": (_u32, [_vp]),
    "rxgpu_ft_shard_imbalance": (C.c_double, [_vp]),
    "rxgpu_ft_shard_exchange_mode": (_i, [_vp]),
    "rxgpu_ft_shard_collectives": (_u64, [_vp]),
    "rxgpu_ft_shard_ranges": (_i, [_vp, _u32, _vp, _vp]),
    "rxgpu_ft_word_df": (_i, [_vp, _u32, C.POINTER(_u64)]),
    "rxgpu_ft_destroy": (None, [_vp]),
    "rxgpu_ft_set_docs": (_i, [_vp, _u64, _vp, _vp, _vp]),
    "rxgpu_ft_set_word": (_i, [_vp, _u32, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rxgpu_ft_merge_simple_raw": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_ft_set_word_positions": (_i, [_vp, _u32, _u64, _vp, _vp, _vp]),
    "rxgpu_ft_merge_terms_raw": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "rxgpu_ft_merge_query_raw": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "rxgpu_ft_merge_query2_raw": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "rxgpu_ft_merge_query_areas_raw": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i), _vp, _vp]),
    "rxgpu_ft_merge_batch_raw": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "rxgpu_ft_read_batch_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_ft_set_train_mode": (None, [_i]),
    "rxgpu_ft_read_train_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_ft_merge_query_resident": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "rxgpu_ft_merge_query2_resident": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "rxgpu_ft_read_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rxgpu_ft_set_words_packed": (_i, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "rxgpu_ft_set_words_packed_ptrs": (_i, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "rxgpu_ft_read_packed_wall": (_i, [_vp, C.POINTER(C.c_double)]),
    "rxgpu_ft_read_packed_stats": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_u64), C.POINTER(_u64)]),
    "rxgpu_ft_get_word": (_i, [_vp, _u32, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u32), _vp]),
    "rxgpu_ft_merge_simple_resident": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "rxgpu_ft_merge_terms_resident": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rxgpu_hybrid_prepare_resident": (_i, [_vp, C.c_int32, _vp, _i, _vp]),
    "rxgpu_hybrid_fuse_resident": (_i, [_vp, C.c_int32, _vp, _i, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64),
                                        C.POINTER(_u32)]),
    "rxgpu_hybrid_read_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rxgpu_hybrid_fuse": (_i, [_i, _vp, _i, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rxgpu_profile_enable": (_i, [_vp, _i]),
    "rxgpu_profile_read": (_i, [_vp, C.c_char_p, C.POINTER(_u64), C.POINTER(C.c_double)]),
}

_lib = None


class RxGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rxgpu error {code}: {msg}")
        self.code = code


def declared_symbols() -> list[str]:
    return sorted(_SIGNATURES)


def lib() -> C.CDLL:
    """Load librxgpu.so (once). Raises if it is not built — there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m reindexer_amd.build` "
                "(hipcc --offload-arch=gfx950). The GPU engine has no CPU fallback.")
        # One process can hold only one HIP runtime.  PyTorch wheels bundle their own libamdhip64.so.7 (same SONAME as
        # /opt/rocm's): whichever is loaded first serves both.  torch must win that race or its device enumeration fails
        # ("No HIP GPUs are available"), so when torch is installed it is imported before librxgpu.so is opened.
        if not os.environ.get("RXGPU_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(_lib, name)
            fn.restype = res
            fn.argtypes = args
    return _lib


def _check(rc: int) -> None:
    if rc != RXGPU_OK:
        raise RxGpuError(rc, lib().rxgpu_last_error().decode(errors="replace"))


def device_count() -> int:
    n = lib().rxgpu_device_count()
    if n < 0:
        _check(n)
    return n


def device_arch(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    _check(lib().rxgpu_device_arch(device, buf, 256))
    return buf.value.decode()


def scan_policy(rows: int, dim: int, nq: int = 1, shadow_available: bool = True, stats_finite: bool = True) -> bool:
    """rxgpu_scan_policy: does such a call take the bf16-pruned scan under the current environment?  Touches no device."""
    return bool(lib().rxgpu_scan_policy(rows, dim, nq, int(shadow_available), int(stats_finite)))


def scan_tier(rows: int, dim: int, nq: int = 1, shadow_available: bool = True, stats_finite: bool = True) -> int:
    """rxgpu_scan_tier: 0 / 1 / 2 = such a call takes the f32 / bf16-pruned / int8-pruned scan under the current environment.  Touches no device."""
    return int(lib().rxgpu_scan_tier(rows, dim, nq, int(shadow_available), int(stats_finite)))


def scan_i6(rows: int, dim: int, nq: int = 1, i6_available: bool = True, stats_finite: bool = True) -> bool:
    """rxgpu_scan_i6: does such a call (whole index) read the 6-bit shadow instead of the int8 one under the current environment?  Touches no device."""
    return bool(lib().rxgpu_scan_i6(rows, dim, nq, int(i6_available), int(stats_finite)))


MERGE_LISTS, MERGE_CANDIDATES, MERGE_FOLD = 0, 1, 2


def knn_merge_probe(what: int, dist: np.ndarray, row: np.ndarray, kk: int, device: int = 0):
    """rxgpu_knn_merge_probe (test instrumentation): one merge kernel over host arrays.  MERGE_LISTS: dist / row are [nlists][kk] sorted lists;
    MERGE_CANDIDATES / MERGE_FOLD: [n] pairs.  Returns (dist[kk], row[kk], count, fast)."""
    dist = np.ascontiguousarray(dist, np.float32)
    row = np.ascontiguousarray(row, np.uint32)
    assert dist.shape == row.shape
    n = dist.shape[0] if what == MERGE_LISTS else dist.size
    assert what != MERGE_LISTS or dist.shape == (n, kk)
    out_d, out_r = np.empty(kk, np.float32), np.empty(kk, np.uint32)
    cnt, path = _u32(0), _i(0)
    _check(lib().rxgpu_knn_merge_probe(device, what, dist.ctypes.data, row.ctypes.data, n, kk, out_d.ctypes.data, out_r.ctypes.data, C.byref(cnt),
                                       C.byref(path)))
    return out_d, out_r, int(cnt.value), bool(path.value)


def scan_tier_range(rows: int, dim: int, listed: bool = False, shadow_available: bool = True, stats_finite: bool = True) -> int:
    """rxgpu_scan_tier_range: 0 / 2 = a range call that scans `rows` rows (the index's, or the entries of a row list when `listed`) takes the
    f32 / int8-pruned range kernel under the current environment.  Touches no device."""
    return int(lib().rxgpu_scan_tier_range(rows, dim, int(listed), int(shadow_available), int(stats_finite)))


def hnsw_distance_blocks(dim: int, sq8: bool = False, deleted: bool = False) -> tuple[int, bool]:
    """rxgpu_hnsw_distance_blocks: (64-float blocks of the fixed-dimension distance batch a search over rows of `dim` components takes, 0 = the
    generic batch; whether the resident kernel serves that row format).  Touches no device."""
    mailbox = C.c_int(0)
    blocks = int(lib().rxgpu_hnsw_distance_blocks(dim, int(sq8), int(deleted), C.byref(mailbox)))
    return blocks, bool(mailbox.value)


def scan_tier_subset(n_ids: int, dim: int, nq: int = 1, kk: int = 10, shadow_available: bool = True, stats_finite: bool = True) -> int:
    """rxgpu_scan_tier_subset: 0 / 2 = a search over a row list of n_ids entries (kk = min(kk, n_ids)) takes the f32 / int8-pruned subset scan
    under the current environment.  Touches no device."""
    return int(lib().rxgpu_scan_tier_subset(n_ids, dim, nq, kk, int(shadow_available), int(stats_finite)))


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _collect_call(fn, head, n, allowed_words, needed, first_batch, max_calls, cap, calls_cap, n_words):
    """the argument tail rxgpu_hnsw_stream_collect and rxgpu_hnsw_collect_knn(_sq8) share, and their results as a dict"""
    L = lib()
    words = None if allowed_words is None else np.ascontiguousarray(allowed_words, np.uint32).reshape(-1)
    if cap is None:
        cap = int(L.rxgpu_hnsw_stream_collect_bound(n, needed, first_batch))
    if calls_cap is None:
        calls_cap = int(L.rxgpu_hnsw_stream_collect_calls_bound(n, needed, first_batch, max_calls))
    if n_words is None:
        n_words = 0 if words is None else words.size
    od, orow, opos = np.empty(max(cap, 1), np.float32), np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
    cb, ce, cend = (np.zeros(max(calls_cap, 1), np.uint32) for _ in range(3))
    calls, launches, ex = _u32(0), _u32(0), C.c_int32(0)
    presented, accepted = _u64(0), _u64(0)
    _check(fn(*head, None if words is None else words.ctypes.data, n_words, needed, first_batch, max_calls, od.ctypes.data, orow.ctypes.data, cap,
              cb.ctypes.data, ce.ctypes.data, cend.ctypes.data, calls_cap, C.byref(calls), C.byref(presented), C.byref(accepted), C.byref(ex),
              C.byref(launches), opos.ctypes.data))
    nc, na = int(calls.value), int(accepted.value)
    return dict(dist=od[:na].copy(), row=orow[:na].copy(), pos=opos[:na].copy(), calls=np.stack([cb[:nc], ce[:nc], cend[:nc]], axis=1),
                presented=int(presented.value), accepted=na, exhausted=bool(ex.value), launches=int(launches.value))


class HnswStream:
    """A streaming KNN session over an attached HNSW graph (rxgpu_hnsw_stream_begin / _begin_sq8 / _continue / _collect / _end)."""

    def __init__(self, ix, query, ef: int = 0, sq8=None):
        self._ix, self._n = ix, int(ix.count)
        self._s = _vp()
        if sq8 is None:
            self._q = _f32c(query).reshape(ix.dim)
            _check(lib().rxgpu_hnsw_stream_begin(ix._h, self._q.ctypes.data, ef, C.byref(self._s)))
        else:
            self._q = np.ascontiguousarray(query, np.uint8).reshape(ix.dim)
            _check(lib().rxgpu_hnsw_stream_begin_sq8(ix._h, self._q.ctypes.data, sq8[0], sq8[1], ef, C.byref(self._s)))

    def next(self, batch: int):
        """rxgpu_hnsw_stream_continue: (dist, row, exhausted), worst first."""
        cap = max(1, min(batch, self._n))
        od, orow = np.empty(cap, np.float32), np.empty(cap, np.uint32)
        cnt, ex = _u32(0), C.c_int(0)
        _check(lib().rxgpu_hnsw_stream_continue(self._s, batch, od.ctypes.data, orow.ctypes.data, C.byref(cnt), C.byref(ex)))
        return od[:cnt.value].copy(), orow[:cnt.value].copy(), bool(ex.value)

    def collect(self, allowed_words, needed: int, first_batch: int, max_calls: int = 1000, cap=None, calls_cap=None, n_words=None):
        """rxgpu_hnsw_stream_collect: the iterator's loop under an allowed-rows bitmap (None: every row) in one device call.  Returns a dict:
        dist / row / pos (the accepted rows of every call, in delivery order, and their positions in their calls' batches), calls ([n][3]:
        batch, emitted, running count of accepted rows), presented, accepted, exhausted, launches.  cap / calls_cap / n_words default to what
        the call requires."""
        return _collect_call(lib().rxgpu_hnsw_stream_collect, (self._s,), self._n, allowed_words, needed, first_batch, max_calls, cap, calls_cap, n_words)

    def close(self):
        if self._s:
            lib().rxgpu_hnsw_stream_end(self._s)
            self._s = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class VectorIndex:
    """One float_vector index shard on one GPU (thin wrapper over rxgpu_index*)."""

    def __init__(self, metric: int | str, dim: int, capacity: int = 0, device: int = 0):
        if isinstance(metric, str):
            metric = METRICS[metric.lower()]
        self.metric, self.dim = int(metric), int(dim)
        h = _vp()
        _check(lib().rxgpu_index_create(self.metric, self.dim, capacity, device, C.byref(h)))
        self._h = h
        self._keepalive = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().rxgpu_index_destroy(self._h)
            self._h = None
            self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- storage
    @property
    def count(self) -> int:
        return lib().rxgpu_index_count(self._h)

    @property
    def capacity(self) -> int:
        return lib().rxgpu_index_capacity(self._h)

    @property
    def row_stride(self) -> int:
        return lib().rxgpu_index_row_stride(self._h)

    @property
    def device_bytes(self) -> int:
        return lib().rxgpu_index_device_bytes(self._h)

    def reserve(self, capacity: int) -> None:
        _check(lib().rxgpu_index_reserve(self._h, capacity))

    def upload_rows(self, first_row: int, rows, inv_norms=None) -> None:
        rows = _f32c(rows).reshape(-1, self.dim)
        nptr = None
        if inv_norms is not None:
            inv_norms = _f32c(inv_norms).reshape(-1)
            assert inv_norms.shape[0] == rows.shape[0]
            nptr = inv_norms.ctypes.data
        _check(lib().rxgpu_index_upload_rows(self._h, first_row, rows.shape[0], rows.ctypes.data, nptr))

    def adopt_device_rows(self, d_rows_ptr: int, n: int, row_stride: int, d_inv_norms_ptr: int | None = None, keepalive=None) -> None:
        _check(lib().rxgpu_index_adopt_device_rows(self._h, d_rows_ptr, n, row_stride, d_inv_norms_ptr))
        self._keepalive = keepalive

    def move_row(self, src: int, dst: int) -> None:
        _check(lib().rxgpu_index_move_row(self._h, src, dst))

    def truncate(self, count: int) -> None:
        _check(lib().rxgpu_index_truncate(self._h, count))

    # ---- search
    def search_knn(self, queries, kk: int):
        """-> (dist[nq,kk] f32, row[nq,kk] u32, count[nq] u32); exact top-kk under (dist,row) order."""
        q = _f32c(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        dist = np.full((nq, max(kk, 1)), np.inf, np.float32)
        row = np.full((nq, max(kk, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        _check(lib().rxgpu_search_knn(self._h, q.ctypes.data, nq, kk, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data))
        return dist[:, :kk], row[:, :kk], cnt

    def search_knn_device(self, d_queries_ptr: int, nq: int, kk: int, d_out_dist_ptr: int, d_out_row_ptr: int,
                          d_out_count_ptr: int | None, stream_ptr: int) -> None:
        _check(lib().rxgpu_search_knn_device(self._h, d_queries_ptr, nq, kk, d_out_dist_ptr, d_out_row_ptr, d_out_count_ptr, stream_ptr))

    # ---- pre-filtered search (`WHERE cond AND KNN(...)`)
    def search_knn_resident(self, query, kk: int):
        """rxgpu_search_knn_resident: one host query, the (dist, row) list left in the index's device buffers.
        Returns (d_dist_ptr, d_row_ptr, d_count_ptr, stream_ptr, entries)."""
        q = _f32c(query)
        dd, dr, dc, st = _vp(), _vp(), _vp(), _vp()
        n = _u32(0)
        _check(lib().rxgpu_search_knn_resident(self._h, q.ctypes.data, kk, C.byref(dd), C.byref(dr), C.byref(dc), C.byref(st), C.byref(n)))
        return dd.value, dr.value, dc.value, st.value, int(n.value)

    def search_knn_subset(self, queries, kk: int, row_ids):
        """Exact top-kk among the listed rows only (strictly increasing uint32 internal rows) -> (dist, row, count)."""
        q = _f32c(queries).reshape(-1, self.dim)
        ids = np.ascontiguousarray(row_ids, dtype=np.uint32).reshape(-1)
        nq = q.shape[0]
        dist = np.full((nq, max(kk, 1)), np.inf, np.float32)
        row = np.full((nq, max(kk, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        _check(lib().rxgpu_search_knn_subset(self._h, q.ctypes.data, nq, kk, ids.ctypes.data if ids.size else None, ids.size,
                                             dist.ctypes.data, row.ctypes.data, cnt.ctypes.data))
        return dist[:, :kk], row[:, :kk], cnt

    def search_knn_bitmap(self, queries, kk: int, allowed_words):
        """Same, the allowed rows given as a bitmap (uint32 words, bit r % 32 of word r // 32) -> (dist, row, count, n_allowed)."""
        q = _f32c(queries).reshape(-1, self.dim)
        words = np.ascontiguousarray(allowed_words, dtype=np.uint32).reshape(-1)
        nq = q.shape[0]
        dist = np.full((nq, max(kk, 1)), np.inf, np.float32)
        row = np.full((nq, max(kk, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        allowed = _u64(0)
        _check(lib().rxgpu_search_knn_bitmap(self._h, q.ctypes.data, nq, kk, words.ctypes.data, words.size, dist.ctypes.data, row.ctypes.data,
                                             cnt.ctypes.data, C.byref(allowed)))
        return dist[:, :kk], row[:, :kk], cnt, int(allowed.value)

    def search_knn_subset_device(self, d_queries_ptr: int, nq: int, kk: int, d_row_ids_ptr: int, n_ids: int, d_out_dist_ptr: int,
                                 d_out_row_ptr: int, d_out_count_ptr: int | None, stream_ptr: int) -> None:
        _check(lib().rxgpu_search_knn_subset_device(self._h, d_queries_ptr, nq, kk, d_row_ids_ptr, n_ids, d_out_dist_ptr, d_out_row_ptr,
                                                    d_out_count_ptr, stream_ptr))

    def check_row_list_device(self, d_row_ids_ptr: int, n_ids: int, stream_ptr: int) -> bool:
        ok = C.c_int32(0)
        _check(lib().rxgpu_check_row_list_device(self._h, d_row_ids_ptr, n_ids, stream_ptr, C.byref(ok)))
        return bool(ok.value)

    def search_range_subset(self, query, radius: float, row_ids, inclusive: bool = False, cap: int = 1 << 16):
        """SearchRange over the listed rows only -> (dist, row) sorted by (dist, row)."""
        q = _f32c(query).reshape(self.dim)
        ids = np.ascontiguousarray(row_ids, dtype=np.uint32).reshape(-1)
        while True:
            dist = np.empty(max(cap, 1), np.float32)
            row = np.empty(max(cap, 1), np.uint32)
            total = _u64(0)
            rc = lib().rxgpu_search_range_subset(self._h, q.ctypes.data, radius, int(inclusive), ids.ctypes.data if ids.size else None, ids.size,
                                                 dist.ctypes.data, row.ctypes.data, cap, C.byref(total))
            if rc == RXGPU_ERR_OVERFLOW:
                cap = int(total.value)
                continue
            _check(rc)
            return dist[:total.value].copy(), row[:total.value].copy()

    def search_range(self, query, radius: float, inclusive: bool = False, cap: int = 1 << 16):
        q = _f32c(query).reshape(self.dim)
        while True:
            dist = np.empty(cap, np.float32)
            row = np.empty(cap, np.uint32)
            total = _u64(0)
            rc = lib().rxgpu_search_range(self._h, q.ctypes.data, radius, int(inclusive), dist.ctypes.data, row.ctypes.data, cap, C.byref(total))
            if rc == RXGPU_ERR_OVERFLOW:
                cap = int(total.value)
                continue
            _check(rc)
            return dist[: total.value].copy(), row[: total.value].copy()

    def distances(self, query, rows) -> np.ndarray:
        q = _f32c(query).reshape(self.dim)
        r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        out = np.empty(r.shape[0], np.float32)
        _check(lib().rxgpu_distances(self._h, q.ctypes.data, r.ctypes.data, r.shape[0], out.ctypes.data))
        return out

    # ---- HNSW
    # ---- IVF: device-resident inverted lists
    def set_lists(self, lists) -> None:
        """lists: sequence of row arrays (disjoint) -> CSR in HBM (rxgpu_index_set_lists)."""
        off = np.zeros(len(lists) + 1, np.uint64)
        off[1:] = np.cumsum([len(l) for l in lists])
        rows = np.ascontiguousarray(np.concatenate([np.asarray(l, np.uint32) for l in lists]) if len(lists) else np.empty(0, np.uint32), np.uint32)
        _check(lib().rxgpu_index_set_lists(self._h, len(lists), off.ctypes.data, rows.ctypes.data if rows.size else None))

    def search_knn_lists(self, coarse: "VectorIndex", query, nprobe: int, k: int):
        """IndexIVFFlat::search in one call: (dist[k'], row[k'], rows scanned)."""
        q = _f32c(query).reshape(self.dim)
        dist = np.full(max(k, 1), np.inf, np.float32)
        row = np.full(max(k, 1), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(1, np.uint32)
        scanned = _u64(0)
        _check(lib().rxgpu_search_knn_lists(self._h, coarse._h, q.ctypes.data, nprobe, k, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data,
                                            C.byref(scanned)))
        c = int(cnt[0])
        return dist[:c], row[:c], int(scanned.value)

    def search_knn_lists_batch(self, coarse: "VectorIndex", queries, nprobe: int, k: int):
        """rxgpu_search_knn_lists for every row of `queries` in one call: (dist [nq][k], row [nq][k], count [nq], scanned [nq]); entries past
        a query's count keep +inf / 0xFFFFFFFF."""
        q = _f32c(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        row = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(max(nq, 1), np.uint32)
        scanned = np.zeros(max(nq, 1), np.uint64)
        _check(lib().rxgpu_search_knn_lists_batch(self._h, coarse._h, q.ctypes.data, nq, nprobe, k, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data,
                                                  scanned.ctypes.data))
        return dist[:, :k], row[:, :k], cnt[:nq], scanned[:nq]

    def ivf_read_batch_stats(self):
        """(batch calls, their queries, device trains, queries answered one by one) since the last call."""
        calls, queries, trains, single = _u64(0), _u64(0), _u64(0), _u64(0)
        _check(lib().rxgpu_ivf_read_batch_stats(self._h, C.byref(calls), C.byref(queries), C.byref(trains), C.byref(single)))
        return int(calls.value), int(queries.value), int(trains.value), int(single.value)

    def search_range_lists(self, coarse: "VectorIndex", query, nprobe: int, radius: float, inclusive: bool = False, cap: int = 1 << 14):
        """IndexIVFFlat::range_search over the device lists in one call: (dist[n], row[n], rows scanned), ascending by (dist, row)."""
        q = _f32c(query).reshape(self.dim)
        while True:
            dist, row = np.empty(max(cap, 1), np.float32), np.empty(max(cap, 1), np.uint32)
            total, scanned = _u64(0), _u64(0)
            rc = lib().rxgpu_search_range_lists(self._h, coarse._h, q.ctypes.data, nprobe, float(radius), int(inclusive), dist.ctypes.data, row.ctypes.data,
                                                cap, C.byref(total), C.byref(scanned))
            if rc == RXGPU_ERR_OVERFLOW:
                cap = int(total.value)
                continue
            _check(rc)
            n = int(total.value)
            return dist[:n].copy(), row[:n].copy(), int(scanned.value)

    # ---- IVF training from resident rows
    def ivf_assign(self, coarse: "VectorIndex", row_ids=None, first_row: int = 0, n: int | None = None) -> np.ndarray:
        """Nearest centroid (a row of `coarse`) of the listed rows, or of rows [first_row, first_row + n) (rxgpu_ivf_assign)."""
        ids = None if row_ids is None else np.ascontiguousarray(row_ids, np.uint32).reshape(-1)
        n = ids.shape[0] if ids is not None else int(n)
        out = np.empty(n, np.uint32)
        _check(lib().rxgpu_ivf_assign(self._h, coarse._h, ids.ctypes.data if ids is not None else None, first_row, n, out.ctypes.data))
        return out

    def ivf_kmeans_step(self, coarse: "VectorIndex", row_ids=None, n: int | None = None):
        """One k-means iteration's device half over the listed rows (or the first n): (centroids [nlist][dim], hassign [nlist], assign [n]) —
        the assignment and compute_centroids' ordered single-precision sums (rxgpu_ivf_kmeans_step)."""
        ids = None if row_ids is None else np.ascontiguousarray(row_ids, np.uint32).reshape(-1)
        n = ids.shape[0] if ids is not None else int(n)
        nlist = coarse.count
        cent = np.empty((nlist, self.dim), np.float32)
        hassign = np.empty(nlist, np.float32)
        assign = np.empty(n, np.uint32)
        _check(lib().rxgpu_ivf_kmeans_step(self._h, coarse._h, ids.ctypes.data if ids is not None else None, n, cent.ctypes.data, hassign.ctypes.data,
                                           assign.ctypes.data))
        return cent, hassign, assign

    def ivf_read_train_stats(self):
        """(rows assigned on the device, k-means steps, device milliseconds, of which the sums kernel) since the last call."""
        rows, steps, ms, sums = _u64(0), _u64(0), C.c_double(0.0), C.c_double(0.0)
        _check(lib().rxgpu_ivf_read_train_stats(self._h, C.byref(rows), C.byref(steps), C.byref(ms), C.byref(sums)))
        return int(rows.value), int(steps.value), float(ms.value), float(sums.value)

    def hnsw_attach_graph(self, g: dict) -> None:
        """g: flat graph dict (links0, upper_off, upper, deleted, M, maxM0, maxlevel, entry, num_deleted)."""
        links0 = np.ascontiguousarray(g["links0"], np.uint32)
        upper_off = np.ascontiguousarray(g["upper_off"], np.uint64)
        upper = np.ascontiguousarray(g["upper"], np.uint32)
        deleted = np.ascontiguousarray(g["deleted"], np.uint8)
        blocks = int(upper_off[-1])
        _check(lib().rxgpu_hnsw_attach_graph(self._h, links0.ctypes.data, upper_off.ctypes.data, upper.ctypes.data, blocks, deleted.ctypes.data,
                                             g["M"], g["maxM0"], g["maxlevel"], g["entry"], g["num_deleted"]))

    def hnsw_link_batch(self, first_row: int, n: int, ef_construction: int) -> None:
        """Rows [first_row, first_row + n) — uploaded, first_row = the attached node count — searched against the graph before them, given
        their level-0 lists and linked back, on the device (rxgpu_hnsw_link_batch)."""
        _check(lib().rxgpu_hnsw_link_batch(self._h, first_row, n, ef_construction))

    def hnsw_patch_upper(self, ids, levels, upper_rows, maxlevel: int, entry: int) -> None:
        """The upper lists of the listed nodes (every node of the last batch among them, ascending) into the mirror; upper_rows = their
        blocks of 1 + M words concatenated in that order (rxgpu_hnsw_patch_upper)."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
        upper_rows = np.ascontiguousarray(upper_rows, np.uint32).reshape(-1)
        if ids.shape[0] != levels.shape[0]:
            raise ValueError("one level per node")
        _check(lib().rxgpu_hnsw_patch_upper(self._h, ids.shape[0], ids.ctypes.data, levels.ctypes.data, upper_rows.ctypes.data if upper_rows.size else None,
                                            maxlevel, entry))

    def hnsw_link_batch_upper(self, first_row: int, n: int, up_rows, ef_construction: int) -> None:
        """Level 1 of the batch hnsw_link_batch(first_row, n) linked last, on the device: up_rows = every row of the batch whose level is
        >= 1, ascending (rxgpu_hnsw_link_batch_upper)."""
        up = np.ascontiguousarray(up_rows, np.uint32).reshape(-1)
        _check(lib().rxgpu_hnsw_link_batch_upper(self._h, first_row, n, up.shape[0], up.ctypes.data if up.size else None, ef_construction))

    def hnsw_patch_upper_from(self, first_level: int, ids, levels, upper_rows, maxlevel: int, entry: int) -> None:
        """hnsw_patch_upper with a first level: 2 = upper_rows holds the blocks of the levels >= 2 only, and level 1 of the new nodes is
        what hnsw_link_batch_upper built (rxgpu_hnsw_patch_upper_from)."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
        upper_rows = np.ascontiguousarray(upper_rows, np.uint32).reshape(-1)
        if ids.shape[0] != levels.shape[0]:
            raise ValueError("one level per node")
        _check(lib().rxgpu_hnsw_patch_upper_from(self._h, first_level, ids.shape[0], ids.ctypes.data, levels.ctypes.data,
                                                 upper_rows.ctypes.data if upper_rows.size else None, maxlevel, entry))

    def hnsw_read_level(self, level: int, ids, M: int):
        """The lists [len(ids)][1 + M] of one level >= 1 of the mirror; an empty list where a node does not reach it (rxgpu_hnsw_read_level)."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        out = np.empty((ids.shape[0], 1 + M), np.uint32)
        _check(lib().rxgpu_hnsw_read_level(self._h, level, ids.shape[0], ids.ctypes.data, out.ctypes.data))
        return out

    def hnsw_read_build_upper_stats(self) -> dict:
        """rxgpu_hnsw_link_batch_upper since the last call: rows, nodes re-selected, nodes past the kernel's cap, milliseconds per phase."""
        rows, resel, over = _u64(0), _u64(0), _u64(0)
        ms = (C.c_double * 3)()
        _check(lib().rxgpu_hnsw_read_build_upper_stats(self._h, C.byref(rows), C.byref(resel), C.byref(over), ms))
        return dict(rows=int(rows.value), reselected=int(resel.value), past_cap=int(over.value), search_ms=float(ms[0]), select_ms=float(ms[1]),
                    backlink_ms=float(ms[2]))

    def hnsw_release_build_view(self) -> None:
        _check(lib().rxgpu_hnsw_release_build_view(self._h))

    def hnsw_read_links0(self, first_row: int, n: int, max_m0: int):
        """Level-0 lists [n][1 + max_m0] of the mirror (rxgpu_hnsw_read_links0)."""
        out = np.empty((n, 1 + max_m0), np.uint32)
        _check(lib().rxgpu_hnsw_read_links0(self._h, first_row, n, out.ctypes.data))
        return out

    def hnsw_read_build_stats(self) -> dict:
        """rxgpu_hnsw_link_batch since the last call: rows, batches, nodes re-selected, nodes past the kernel's cap, milliseconds per phase."""
        rows, batches, resel, over = _u64(0), _u64(0), _u64(0), _u64(0)
        ms = (C.c_double * 3)()
        _check(lib().rxgpu_hnsw_read_build_stats(self._h, C.byref(rows), C.byref(batches), C.byref(resel), C.byref(over), ms))
        return dict(rows=int(rows.value), batches=int(batches.value), reselected=int(resel.value), past_cap=int(over.value),
                    search_ms=float(ms[0]), select_ms=float(ms[1]), backlink_ms=float(ms[2]))

    def hnsw_update_deleted(self, deleted, num_deleted: int) -> None:
        deleted = np.ascontiguousarray(deleted, np.uint8)
        _check(lib().rxgpu_hnsw_update_deleted(self._h, deleted.ctypes.data, num_deleted))

    def hnsw_search_knn(self, queries, k: int, ef: int = 0):
        q = _f32c(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        row = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        _check(lib().rxgpu_hnsw_search_knn(self._h, q.ctypes.data, nq, k, ef, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data))
        return dist[:, :k], row[:, :k], cnt

    def hnsw_search_knn_filtered(self, queries, k: int, ef: int, allowed_words):
        """SearchKnn under an allowed-rows bitmap (rxgpu_hnsw_search_knn_filtered): bit r % 32 of word r // 32 set = node r may be returned;
        one bitmap for all queries.  (dist, row, count, set bits below the node count)."""
        q = _f32c(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        words = np.ascontiguousarray(allowed_words, np.uint32).reshape(-1)
        dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        row = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        n_allowed = _u64(0)
        _check(lib().rxgpu_hnsw_search_knn_filtered(self._h, q.ctypes.data, nq, k, ef, words.ctypes.data, words.size, dist.ctypes.data, row.ctypes.data,
                                                    cnt.ctypes.data, C.byref(n_allowed)))
        return dist[:, :k], row[:, :k], cnt, int(n_allowed.value)

    def hnsw_search_knn_sq8_filtered(self, qcodes, qcorr, qnorm, k: int, ef: int, allowed_words):
        """The same over the SQ8 codes (rxgpu_hnsw_search_knn_sq8_filtered); the queries travel as for hnsw_search_knn_sq8."""
        qc = np.ascontiguousarray(qcodes, np.uint8).reshape(-1, self.dim)
        nq = qc.shape[0]
        qcorr = _f32c(qcorr).reshape(-1)
        qnorm = _f32c(qnorm).reshape(-1)
        if qcorr.shape[0] != nq or qnorm.shape[0] != nq:
            raise ValueError("one corrective offset and one normCoef per query")
        words = np.ascontiguousarray(allowed_words, np.uint32).reshape(-1)
        dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        row = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        n_allowed = _u64(0)
        _check(lib().rxgpu_hnsw_search_knn_sq8_filtered(self._h, qc.ctypes.data, qcorr.ctypes.data, qnorm.ctypes.data, nq, k, ef, words.ctypes.data,
                                                        words.size, dist.ctypes.data, row.ctypes.data, cnt.ctypes.data, C.byref(n_allowed)))
        return dist[:, :k], row[:, :k], cnt, int(n_allowed.value)

    def hnsw_stream(self, query, ef: int = 0):
        """rxgpu_hnsw_stream_begin: a streaming KNN session (HnswStream) with .next(batch), .collect(...) and .close()."""
        return HnswStream(self, query, ef)

    def hnsw_stream_sq8(self, qcodes, qcorr: float, qnorm: float, ef: int = 0):
        """rxgpu_hnsw_stream_begin_sq8: the same session over the attached SQ8 codes."""
        return HnswStream(self, qcodes, ef, sq8=(float(qcorr), float(qnorm)))

    def hnsw_collect_knn(self, query, ef: int, allowed_words, needed: int, first_batch: int, max_calls: int = 1000, cap=None, calls_cap=None, n_words=None):
        """rxgpu_hnsw_collect_knn: begin + collect + end for one query in one call on a leased search context; the dict of HnswStream.collect."""
        q = _f32c(query).reshape(self.dim)
        return _collect_call(lib().rxgpu_hnsw_collect_knn, (self._h, q.ctypes.data, ef), int(self.count), allowed_words, needed, first_batch, max_calls, cap,
                             calls_cap, n_words)

    def hnsw_collect_knn_sq8(self, qcodes, qcorr: float, qnorm: float, ef: int, allowed_words, needed: int, first_batch: int, max_calls: int = 1000):
        """rxgpu_hnsw_collect_knn_sq8: the same over the attached SQ8 codes."""
        qc = np.ascontiguousarray(qcodes, np.uint8).reshape(self.dim)
        return _collect_call(lib().rxgpu_hnsw_collect_knn_sq8, (self._h, qc.ctypes.data, float(qcorr), float(qnorm), ef), int(self.count), allowed_words, needed,
                             first_batch, max_calls, None, None, None)

    def hnsw_search_knn_posted(self, query, k: int, ef: int = 0):
        """One query through the index's resident search kernel (rxgpu_hnsw_search_knn_posted): (dist, row, count, served)."""
        q = _f32c(query).reshape(self.dim)
        dist = np.full(max(k, 1), np.inf, np.float32)
        row = np.full(max(k, 1), 0xFFFFFFFF, np.uint32)
        cnt = _u32(0)
        served = C.c_int32(0)
        _check(lib().rxgpu_hnsw_search_knn_posted(self._h, q.ctypes.data, k, ef, dist.ctypes.data, row.ctypes.data, C.addressof(cnt), C.byref(served)))
        return dist[:k], row[:k], int(cnt.value), bool(served.value)

    def hnsw_read_stats4(self):
        """(distance evaluations, hops, in-kernel restarts, distance trips of the look-ahead team searches) since the last read."""
        v = (_u64 * 4)()
        _check(lib().rxgpu_hnsw_read_stats4(self._h, C.addressof(v)))
        return tuple(int(x) for x in v)

    def hnsw_server_times(self):
        """(microseconds on the device, microseconds at the callers) summed over the queries the mailbox has answered."""
        a, b = _u64(0), _u64(0)
        _check(lib().rxgpu_hnsw_server_times(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def hnsw_server_stats(self):
        a, b = _u64(0), _u64(0)
        _check(lib().rxgpu_hnsw_server_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def hnsw_attach_sq8(self, codes, corr, alpha_2: float) -> None:
        """SQ8 copy of the rows (Quantizer::Quantize, quantizer.h:93-124): codes [count][dim] u8, corr [count] f32."""
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.dim)
        corr = _f32c(corr).reshape(-1)
        if codes.shape[0] != corr.shape[0]:
            raise ValueError("one corrective offset per code row")
        _check(lib().rxgpu_hnsw_attach_sq8(self._h, codes.ctypes.data, corr.ctypes.data, codes.shape[0], float(alpha_2)))

    def hnsw_upload_sq8_rows(self, first_row: int, codes, corr, alpha_2: float) -> None:
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.dim)
        corr = _f32c(corr).reshape(-1)
        if codes.shape[0] != corr.shape[0]:
            raise ValueError("one corrective offset per code row")
        _check(lib().rxgpu_hnsw_upload_sq8_rows(self._h, first_row, codes.shape[0], codes.ctypes.data, corr.ctypes.data, float(alpha_2)))

    def hnsw_quantize_sq8(self, first_row: int, n: int, min_q: float, alpha: float, delta: float, alpha_2: float) -> None:
        """Codes and corrective offsets of rows [first_row, first_row + n) computed on the device from the index's float rows
        (rxgpu_hnsw_quantize_sq8): what Quantizer::quantize gives, bit for bit."""
        _check(lib().rxgpu_hnsw_quantize_sq8(self._h, first_row, n, float(min_q), float(alpha), float(delta), float(alpha_2)))

    def hnsw_read_sq8_rows(self, first_row: int, n: int):
        """(codes [n][dim] u8, corr [n] f32) of the code table (test instrumentation)."""
        codes = np.empty((n, self.dim), np.uint8)
        corr = np.empty(n, np.float32)
        _check(lib().rxgpu_hnsw_read_sq8_rows(self._h, first_row, n, codes.ctypes.data, corr.ctypes.data))
        return codes, corr

    def hnsw_read_sq8_quantize_stats(self):
        """(rows coded on the device, launches, kernel milliseconds) since the last call."""
        rows, launches, ms = _u64(0), _u64(0), C.c_double(0.0)
        _check(lib().rxgpu_hnsw_read_sq8_quantize_stats(self._h, C.byref(rows), C.byref(launches), C.byref(ms)))
        return int(rows.value), int(launches.value), float(ms.value)

    def hnsw_search_knn_sq8(self, qcodes, qcorr, qnorm, k: int, ef: int = 0):
        qc = np.ascontiguousarray(qcodes, np.uint8).reshape(-1, self.dim)
        nq = qc.shape[0]
        qcorr = _f32c(qcorr).reshape(-1)
        qnorm = _f32c(qnorm).reshape(-1)
        if qcorr.shape[0] != nq or qnorm.shape[0] != nq:
            raise ValueError("one corrective offset and one normCoef per query")
        dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        row = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(nq, np.uint32)
        _check(lib().rxgpu_hnsw_search_knn_sq8(self._h, qc.ctypes.data, qcorr.ctypes.data, qnorm.ctypes.data, nq, k, ef, dist.ctypes.data,
                                               row.ctypes.data, cnt.ctypes.data))
        return dist[:, :k], row[:, :k], cnt

    def hnsw_search_knn_sq8_posted(self, qcodes, qcorr: float, qnorm: float, k: int, ef: int = 0):
        """One quantised query through the index's resident search kernel over the SQ8 codes (rxgpu_hnsw_search_knn_sq8_posted):
        (dist, row, count, served)."""
        qc = np.ascontiguousarray(qcodes, np.uint8).reshape(self.dim)
        dist = np.full(max(k, 1), np.inf, np.float32)
        row = np.full(max(k, 1), 0xFFFFFFFF, np.uint32)
        cnt = _u32(0)
        served = C.c_int32(0)
        _check(lib().rxgpu_hnsw_search_knn_sq8_posted(self._h, qc.ctypes.data, float(qcorr), float(qnorm), k, ef, dist.ctypes.data, row.ctypes.data,
                                                      C.addressof(cnt), C.byref(served)))
        return dist[:k], row[:k], int(cnt.value), bool(served.value)

    def hnsw_read_stats(self):
        a, b = _u64(0), _u64(0)
        _check(lib().rxgpu_hnsw_read_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def hnsw_read_tie_reruns(self) -> int:
        a = _u64(0)
        _check(lib().rxgpu_hnsw_read_tie_reruns(self._h, C.byref(a)))
        return int(a.value)

    def hnsw_read_lds_reruns(self) -> int:
        a = _u64(0)
        _check(lib().rxgpu_hnsw_read_lds_reruns(self._h, C.byref(a)))
        return int(a.value)

    # ---- instrumentation
    def profile_enable(self, on: bool = True) -> None:
        _check(lib().rxgpu_profile_enable(self._h, int(on)))

    def profile_read(self, name: str) -> tuple[int, float]:
        n, ms = _u64(0), C.c_double(0.0)
        _check(lib().rxgpu_profile_read(self._h, name.encode(), C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def last_candidates(self) -> tuple[int, int]:
        """(candidates, list capacity) of the last pruned single-query search_knn made while profiling was enabled."""
        n, cap = _u32(0), _u32(0)
        _check(lib().rxgpu_index_last_candidates(self._h, C.byref(n), C.byref(cap)))
        return int(n.value), int(cap.value)

    _INSPECT_DTYPES = {"stats": np.uint32, "row_sq": np.float32, "codes_i8": np.int8, "side_i8": np.float32, "rows_bf16": np.uint16,
                       "codes_i6": np.uint8, "side_i6": np.float32, "stats_i6": np.uint32, "pruned_seed": np.uint32,
                       "pruned_values": np.float32, "pruned_margin": np.float32, "pruned_q_sq": np.float32, "pruned_qinfo": np.float32,
                       "pruned_qplanes": np.int8, "pruned_top": np.uint32, "pruned_cand_rows": np.uint32,
                       "pruned_emit_cnt": np.uint32, "pruned_emitted": np.uint32}

    def inspect(self, name: str) -> np.ndarray:
        """rxgpu_index_inspect: a named internal buffer as a flat array (test instrumentation; include/rxgpu.h lists the names and shapes).
        "pruned_top" comes as kk + 1 uint32 words: the bits of the kk list values, then the number of entries; "pruned_emitted" as 2 n words:
        per entry the bits of lo, then the row."""
        need = _u64(0)
        rc = lib().rxgpu_index_inspect(self._h, name.encode(), None, 0, C.byref(need))
        if rc != RXGPU_ERR_OVERFLOW:
            _check(rc)
        out = np.empty(int(need.value), np.uint8)
        if out.size:
            _check(lib().rxgpu_index_inspect(self._h, name.encode(), out.ctypes.data, out.size, C.byref(need)))
        return out.view(self._INSPECT_DTYPES.get(name, np.uint8))


class ShardedVectorIndex(VectorIndex):
    """rxgpu_index_create_sharded: the same index row-range sharded over a device list of THIS process (a device may repeat).  Rows in and out
    are global rows; SearchKnn's per-shard lists meet in one RCCL all-gather on the devices (merge_mode == 1) unless RXGPU_SHARD_MERGE=host
    was set when the index was created."""

    def __init__(self, metric: int | str, dim: int, capacity: int, devices):
        if isinstance(metric, str):
            metric = METRICS[metric.lower()]
        self.metric, self.dim = int(metric), int(dim)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = _vp()
        _check(lib().rxgpu_index_create_sharded(self.metric, self.dim, capacity, len(devices), devs, C.byref(h)))
        self._h = h
        self._keepalive = None

    @property
    def merge_mode(self) -> str:
        return {1: "rccl", 0: "host"}[lib().rxgpu_index_shard_merge_mode(self._h)]

    @property
    def merge_note(self) -> str:
        """why the index merges on the host ("" in rccl mode)"""
        return (lib().rxgpu_index_shard_merge_note(self._h) or b"").decode()

    @property
    def ranks(self) -> int:
        return lib().rxgpu_index_shard_ranks(self._h)

    @property
    def collectives(self) -> int:
        return lib().rxgpu_index_shard_collectives(self._h)

    @property
    def shard_count(self) -> int:
        return lib().rxgpu_index_shard_count(self._h)

    @property
    def shard_rows(self) -> int:
        return lib().rxgpu_index_shard_rows(self._h)

    def shard(self, s: int) -> "VectorIndex":
        """Shard s as a NON-owning single-device view (adopt_device_rows / profile_enable / profile_read on it)."""
        hs = lib().rxgpu_index_shard(self._h, s)
        if not hs:
            raise RxGpuError("no such shard")
        return _ShardView(self.metric, self.dim, _vp(hs))

    def sync_count(self) -> None:
        _check(lib().rxgpu_index_shard_sync_count(self._h))


class _ShardView(VectorIndex):
    def __init__(self, metric: int, dim: int, handle):
        self.metric, self.dim, self._keepalive = metric, dim, None
        self._h = handle

    def close(self) -> None:   # owned by the sharded index
        self._h = None
        self._keepalive = None


def merge_shards_device(d_gathered_ptr: int, world: int, nq: int, kk: int, shard_rows: int, d_out_dist_ptr: int, d_out_row_ptr: int,
                        d_out_count_ptr: int | None, stream_ptr: int) -> None:
    _check(lib().rxgpu_merge_shards_device(d_gathered_ptr, world, nq, kk, shard_rows, d_out_dist_ptr, d_out_row_ptr, d_out_count_ptr, stream_ptr))


class HybridParams(C.Structure):
    """rxgpu_hybrid_params"""
    _fields_ = [("kind", C.c_int32), ("is_union", C.c_int32), ("desc", C.c_int32), ("reserved", C.c_int32), ("params", C.c_double * 5)]


def hybrid_fuse(kind: str, params, knn_ids, knn_ranks, ft_ids, ft_ranks_u8, union=True, desc=True, metric=METRIC_IP, device: int = 0):
    """rxgpu_hybrid_fuse: the device rank fusion on host arrays.  knn_* best first (the planner's ranks), ft_ids unique in any order with
    their uint8 ranks.  Returns (ids, ranks) in Merged<desc> order."""
    hp = HybridParams()
    hp.kind = 0 if kind == "rrf" else 1
    hp.is_union, hp.desc = int(union), int(desc)
    for i, v in enumerate(params):
        hp.params[i] = float(v)
    ki, kr = np.ascontiguousarray(knn_ids, np.int32), _f32c(knn_ranks)
    fi, fr = np.ascontiguousarray(ft_ids, np.int32), np.ascontiguousarray(ft_ranks_u8, np.uint8)
    cap = ki.shape[0] + fi.shape[0] + 1
    oi, orank = np.empty(cap, np.int32), np.empty(cap, np.float32)
    n = _u64(0)
    _check(lib().rxgpu_hybrid_fuse(device, C.addressof(hp), metric, ki.ctypes.data, kr.ctypes.data, ki.shape[0], fi.ctypes.data, fr.ctypes.data,
                                   fi.shape[0], oi.ctypes.data, orank.ctypes.data, cap, C.byref(n)))
    return oi[:n.value].copy(), orank[:n.value].copy()


def gpu_available() -> bool:
    if os.environ.get("RXGPU_FORCE_NO_GPU"):
        return False
    try:
        return device_count() > 0
    except Exception:
        return False
