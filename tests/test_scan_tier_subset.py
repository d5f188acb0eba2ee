"""CPU-only: rxgpu_scan_tier_subset, the decision between the f32 subset scan (0) and the int8-pruned subset scan (2) for a search over a
row list, decides as include/rxgpu.h documents under every environment combination (no device is touched)."""
import itertools

import pytest

GiB = 1 << 30
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES")


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


@pytest.fixture(scope="module")
def tier():
    from reindexer_amd import capi
    capi.lib()
    return capi.scan_tier_subset


def expected(bf16, i8, min_bytes, n_ids, dim, nq, kk, shadow, finite):
    """the table of the header, restated"""
    if bf16 is not None or i8 == 0 or not shadow or not (128 < dim <= 1024) or kk > 64 or n_ids == 0:
        return 0
    if i8 == 1:
        return 2 if nq <= 8 else 0
    return 2 if nq == 1 and finite and min_bytes is not None and n_ids * dim * 4 >= min_bytes else 0   # unset: no finite default yet


def test_every_environment_combination(monkeypatch, tier):
    n_ids = 10_000
    seen = set()
    for bf16, i8, dim in itertools.product((None, 0, 1), (None, 0, 1), (128, 129, 768, 1024, 1100)):
        listed = n_ids * dim * 4
        for min_bytes in (None, 1, listed, listed + 1):
            _env(monkeypatch, BF16=bf16, I8=i8, I8_SUBSET_MIN_BYTES=min_bytes)
            for nq, kk, shadow, finite in itertools.product((1, 8, 9), (1, 64, 65), (True, False), (True, False)):
                want = expected(bf16, i8, min_bytes, n_ids, dim, nq, kk, shadow, finite)
                assert tier(n_ids, dim, nq, kk, shadow, finite) == want, (bf16, i8, min_bytes, dim, nq, kk, shadow, finite)
                seen.add(want)
            assert tier(0, dim, 1, 1, True, True) == 0          # an empty list
    assert seen == {0, 2}


def test_automatic_threshold_counts_the_listed_bytes(monkeypatch, tier):
    _env(monkeypatch)
    for n_ids in (100_000, 10_000_000, 1 << 40):               # no finite default until the crossover is measured: never below 1 GiB then
        assert tier(n_ids, 768, 1, 10) == 0
    _env(monkeypatch, I8_SUBSET_MIN_BYTES=GiB)
    assert tier(GiB // (768 * 4) + 1, 768, 1, 10) == 2         # 1 GiB of LISTED f32 rows
    assert tier(GiB // (768 * 4), 768, 1, 10) == 0             # (2^30 / 3072 is not whole: one entry fewer is below)
    assert tier(GiB // (1024 * 4), 1024, 1, 10) == 2           # exactly 1 GiB
    assert tier(GiB // (1024 * 4) - 1, 1024, 1, 10) == 0
    assert tier(10_000_000, 768, 1, 10) == 2                   # the headline corpus behind a 100 % filter
    assert tier(1_000_000, 768, 1, 10) == 2                    # ... behind a 10 % filter: 3 GB listed
    assert tier(100_000, 768, 1, 10) == 0                      # ... behind a 1 % filter
    for nq in (2, 8, 9):
        assert tier(10_000_000, 768, nq, 10) == 0              # automatic mode: single queries only
    assert tier(10_000_000, 768, 1, 10, True, False) == 0      # a non-finite row statistic
    assert tier(10_000_000, 768, 1, 10, False, True) == 0      # no room for the shadow
    for dim, want in ((128, 0), (129, 2), (1024, 2), (1100, 0)):
        assert tier(10_000_000, dim, 1, 10) == want
    assert tier(10_000_000, 768, 1, 64) == 2 and tier(10_000_000, 768, 1, 65) == 0
    listed = 5_000 * 256 * 4
    _env(monkeypatch, I8_SUBSET_MIN_BYTES=listed)
    assert tier(5_000, 256, 1, 10) == 2 and tier(4_999, 256, 1, 10) == 0
    _env(monkeypatch, I8_SUBSET_MIN_BYTES=listed + 1)
    assert tier(5_000, 256, 1, 10) == 0 and tier(5_001, 256, 1, 10) == 2
    # the thresholds of the unfiltered tiers do not move this one
    _env(monkeypatch, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
    assert tier(5_000, 256, 1, 10) == 0
    _env(monkeypatch, BF16_MIN_BYTES=64 * GiB, I8_MIN_BYTES=64 * GiB, I8_SUBSET_MIN_BYTES=GiB)
    assert tier(10_000_000, 768, 1, 10) == 2


def test_forced_and_switched_off(monkeypatch, tier):
    _env(monkeypatch, I8=1)
    for nq, want in ((1, 2), (8, 2), (9, 0)):
        assert tier(7, 256, nq, 7) == want                     # any size
        assert tier(7, 256, nq, 7, True, False) == want        # whatever the statistics: the gate answers such a call
    assert tier(7, 256, 1, 7, False, True) == 0
    assert tier(1000, 768, 1, 64) == 2 and tier(1000, 768, 1, 65) == 0
    assert tier(1000, 128, 1, 10) == 0 and tier(1000, 1100, 1, 10) == 0 and tier(0, 768, 1, 1) == 0
    _env(monkeypatch, I8=1, I8_SUBSET_MIN_BYTES=64 * GiB)      # forced: the threshold is not asked
    assert tier(1000, 768, 1, 10) == 2
    for kw in (dict(BF16=0), dict(BF16=1), dict(I8=0), dict(BF16=0, I8=1), dict(BF16=1, I8=1), dict(I8=0, I8_SUBSET_MIN_BYTES=1)):
        _env(monkeypatch, **kw)
        assert tier(10_000_000, 768, 1, 10) == 0, kw
        assert tier(1000, 768, 1, 10) == 0, kw
