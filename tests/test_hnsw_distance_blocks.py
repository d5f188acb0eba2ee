"""CPU: rxgpu_hnsw_distance_blocks, the one list of embedding sizes with a fixed-dimension HNSW distance batch (csrc/hnsw_distance_blocks.h),
answers as include/rxgpu.h documents — and is declared, bound and exported.  No device is touched."""
import ctypes

import pytest

from .test_abi_symbols import header_symbols

NAME = "rxgpu_hnsw_distance_blocks"


@pytest.mark.parametrize("deleted", [False, True])
@pytest.mark.parametrize("dim,blocks", [(128, 2), (512, 8), (768, 12), (1024, 16), (1536, 24)])
def test_float_rows_with_a_fixed_form(dim, blocks, deleted):
    from reindexer_amd import capi
    assert capi.hnsw_distance_blocks(dim, sq8=False, deleted=deleted) == (blocks, True)


@pytest.mark.parametrize("deleted", [False, True])
@pytest.mark.parametrize("dim", [384, 100, 1088, 2048])
def test_float_rows_on_the_generic_batch(dim, deleted):
    from reindexer_amd import capi
    assert capi.hnsw_distance_blocks(dim, sq8=False, deleted=deleted) == (0, False)


@pytest.mark.parametrize("dim", [128, 384, 512, 768, 1024, 1536])
def test_codes(dim):
    """six sizes on a bare graph; with deleted nodes 128 and 768 only"""
    from reindexer_amd import capi
    assert capi.hnsw_distance_blocks(dim, sq8=True, deleted=False) == (dim // 64, True)
    want = (dim // 64, True) if dim in (128, 768) else (0, False)
    assert capi.hnsw_distance_blocks(dim, sq8=True, deleted=True) == want


@pytest.mark.parametrize("dim", [100, 256, 1088, 2048])
def test_codes_on_the_generic_batch(dim):
    from reindexer_amd import capi
    assert capi.hnsw_distance_blocks(dim, sq8=True, deleted=False) == (0, False)
    assert capi.hnsw_distance_blocks(dim, sq8=True, deleted=True) == (0, False)


def test_mailbox_pointer_may_be_null():
    from reindexer_amd import capi
    assert capi.lib().rxgpu_hnsw_distance_blocks(1536, 0, 0, None) == 24


def test_declared_bound_and_exported():
    from reindexer_amd import capi
    assert NAME in header_symbols() and NAME in capi.declared_symbols()
    assert hasattr(ctypes.CDLL(str(capi.LIB_PATH)), NAME), f"librxgpu.so does not export {NAME}"
    assert callable(capi.hnsw_distance_blocks)
