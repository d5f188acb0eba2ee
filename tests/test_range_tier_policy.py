"""rxgpu_scan_tier_range decides as include/rxgpu.h documents: which kernel a range call takes (0 the f32 range kernel, 2 the int8-pruned one)
under every environment.  No device is touched."""
GiB = 1 << 30
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_RANGE_MIN_BYTES")


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


def test_scan_tier_range_under_every_environment(monkeypatch):
    from reindexer_amd import capi
    capi.lib()
    tier = capi.scan_tier_range
    assert capi.lib().rxgpu_abi_version() == 2                       # the export is additive
    rows_1g = GiB // (768 * 4) + 1
    # unset: the default of RXGPU_SCAN_I8_RANGE_MIN_BYTES is 16 GiB (profiles/range_i8_ab.json); a list needs RXGPU_SCAN_I8_SUBSET_MIN_BYTES too,
    # whose default is the maximum value
    _env(monkeypatch)
    rows_16g = 16 * GiB // (768 * 4) + 1
    assert tier(10_000_000, 768) == 2 and tier(rows_16g, 768) == 2 and tier(rows_16g - 2, 768) == 0 and tier(5_000_000, 768) == 0 and tier(100, 256) == 0
    assert tier(100_000_000, 1024) == 2 and tier(100_000_000, 128) == 0 and tier(10_000_000, 768, listed=True) == 0
    assert tier(10_000_000, 768, stats_finite=False) == 0 and tier(10_000_000, 768, shadow_available=False) == 0
    # automatic with the threshold given: the f32 bytes of the scanned rows decide, on an index with finite statistics and a shadow
    _env(monkeypatch, I8_RANGE_MIN_BYTES=GiB)
    assert tier(rows_1g, 768) == 2 and tier(rows_1g - 2, 768) == 0 and tier(10_000_000, 768) == 2
    assert tier(10_000_000, 768, stats_finite=False) == 0 and tier(10_000_000, 768, shadow_available=False) == 0
    assert tier(10_000_000, 1024) == 2 and tier(10_000_000, 750) == 2 and tier(10_000_000, 200) == 2 and tier(10_000_000, 129) == 2
    assert tier(40_000_000, 128) == 0 and tier(40_000_000, 64) == 0 and tier(10_000_000, 1025) == 0 and tier(10_000_000, 1100) == 0
    assert tier(0, 768) == 0
    _env(monkeypatch, I8_RANGE_MIN_BYTES=1000 * 256 * 4)
    assert tier(1000, 256) == 2 and tier(999, 256) == 0
    # the KNN thresholds do not move a range call
    _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
    assert tier(5_000_000, 768) == 0 and tier(1000, 256) == 0
    _env(monkeypatch, I8_RANGE_MIN_BYTES=1, BF16_MIN_BYTES=64 * GiB, I8_MIN_BYTES=64 * GiB)
    assert tier(1000, 256) == 2
    # a list call needs RXGPU_SCAN_I8_SUBSET_MIN_BYTES as well, like a KNN search over a list (its default is the maximum value too)
    _env(monkeypatch, I8_RANGE_MIN_BYTES=1)
    assert tier(5000, 256) == 2 and tier(5000, 256, listed=True) == 0
    _env(monkeypatch, I8_SUBSET_MIN_BYTES=1)
    assert tier(5000, 256, listed=True) == 0 and tier(5000, 256) == 0 and tier(10_000_000, 768, listed=True) == 2
    _env(monkeypatch, I8_RANGE_MIN_BYTES=1000 * 256 * 4, I8_SUBSET_MIN_BYTES=2000 * 256 * 4)
    assert tier(1000, 256) == 2 and tier(1999, 256, listed=True) == 0 and tier(2000, 256, listed=True) == 2
    _env(monkeypatch, I8_RANGE_MIN_BYTES=2000 * 256 * 4, I8_SUBSET_MIN_BYTES=1000 * 256 * 4)
    assert tier(1999, 256, listed=True) == 0 and tier(2000, 256, listed=True) == 2 and tier(1999, 256) == 0
    # RXGPU_SCAN_I8=1: forced at any size, whatever the statistics say, lists too; still the dimension, the shadow and at least one row
    _env(monkeypatch, I8=1)
    assert tier(7, 256) == 2 and tier(7, 256, stats_finite=False) == 2 and tier(1, 750, listed=True) == 2 and tier(10_000_000, 768) == 2
    assert tier(7, 128) == 0 and tier(7, 1100) == 0 and tier(7, 256, shadow_available=False) == 0 and tier(0, 256) == 0
    # RXGPU_SCAN_I8=0: off, whatever the thresholds say
    _env(monkeypatch, I8=0, I8_RANGE_MIN_BYTES=1, I8_SUBSET_MIN_BYTES=1)
    assert tier(10_000_000, 768) == 0 and tier(10_000_000, 768, listed=True) == 0
    # RXGPU_SCAN_BF16=0 and =1 both win: there is no bf16 range form
    for bf16 in (0, 1):
        for i8 in ({}, {"I8": 1}, {"I8_RANGE_MIN_BYTES": 1, "I8_SUBSET_MIN_BYTES": 1}):
            _env(monkeypatch, BF16=bf16, **i8)
            assert tier(10_000_000, 768) == 0 and tier(7, 256) == 0 and tier(10_000_000, 768, listed=True) == 0
    # the environment is read per call
    _env(monkeypatch, I8=1)
    assert tier(7, 256) == 2
    _env(monkeypatch)
    assert tier(7, 256) == 0
