"""rxgpu_scan_i6 decides as include/rxgpu.h documents, under every combination of the environment it reads, and rxgpu_scan_tier keeps every
answer it gave before RXGPU_SCAN_I6 existed (no device is touched)."""
import itertools

import pytest

GiB = 1 << 30
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I6", "RXGPU_SCAN_I6_MIN_BYTES")
# calls whose tier is interesting: big / small, every dimension class, several queries, no shadow, no finite statistics
CALLS = [((10_000_000, 768), {}), ((GiB // (768 * 4) + 1, 768), {}), ((200_000, 768), {}), ((100, 256), {}), ((100, 256), dict(nq=8)), ((100, 256), dict(nq=9)),
         ((10_000_000, 768), dict(nq=2)), ((10_000_000, 768), dict(stats_finite=False)), ((10_000_000, 128), {}), ((10_000_000, 1100), {}),
         ((10_000_000, 1024), {}), ((10_000_000, 129), {}), ((10_000_000, 768), dict(shadow_available=False))]


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv("RXGPU_SCAN_" + k, str(v))


@pytest.fixture(scope="module")
def capi():
    from reindexer_amd import capi
    capi.lib()
    return capi


def test_scan_i6_under_every_environment(monkeypatch, capi):
    i6 = capi.scan_i6
    big, small = (10_000_000, 768), (100, 256)
    _env(monkeypatch)                                            # the default threshold is "never" until the crossover says otherwise, or a size
    default_on = i6(*big)
    assert not i6(*small) and not i6(200_000, 768)
    _env(monkeypatch, I6_MIN_BYTES=GiB)                         # automatic: a call tier 2 takes automatically, from the threshold on
    rows_1g = GiB // (768 * 4) + 1
    assert i6(*big) and i6(rows_1g, 768) and not i6(rows_1g - 2, 768) and not i6(*small)
    assert not i6(*big, nq=2) and not i6(*big, stats_finite=False) and not i6(*big, i6_available=False)
    assert i6(10_000_000, 1024) and i6(10_000_000, 200) and not i6(10_000_000, 128) and not i6(10_000_000, 129) and not i6(10_000_000, 1100)
    _env(monkeypatch, I6_MIN_BYTES=64 * GiB)
    assert not i6(*big)
    _env(monkeypatch, I6_MIN_BYTES=1)                           # the threshold alone never widens what tier 2 takes
    assert not i6(*small) and i6(*big)
    _env(monkeypatch, I6_MIN_BYTES=1, BF16_MIN_BYTES=1, I8_MIN_BYTES=1)
    assert i6(*small) and i6(1000, 256) and not i6(1000, 128)
    _env(monkeypatch, I6_MIN_BYTES=1, I8_MIN_BYTES=64 * GiB)    # the call goes to the bf16 tier: not ours
    assert not i6(*big)
    _env(monkeypatch, I6=0, I6_MIN_BYTES=1)                     # off
    assert not i6(*big) and not i6(*small)
    _env(monkeypatch, I6=1)                                     # forced: any size, up to 8 queries, whatever the statistics say; still the dimension and the shadow
    assert i6(*small) and i6(*small, nq=8) and i6(*small, stats_finite=False) and i6(7, 750) and i6(*big) and i6(100, 160)
    assert not i6(*small, nq=9) and not i6(100, 1100) and not i6(100, 128) and not i6(*small, i6_available=False)
    for other in (dict(BF16=0), dict(BF16=1), dict(I8=0), dict(I8=1)):   # these win, forced or automatic: RXGPU_SCAN_I8=1 means the int8 front exactly
        for mine in (dict(I6=1), dict(I6_MIN_BYTES=1), dict(I6=1, I6_MIN_BYTES=1)):
            _env(monkeypatch, **other, **mine)
            assert not i6(*big) and not i6(*small), (other, mine)
    _env(monkeypatch)
    assert i6(*big) == default_on


def test_scan_tier_does_not_know_the_variable(monkeypatch, capi):
    """every combination of the older variables x every value of the new ones: rxgpu_scan_tier and rxgpu_scan_policy answer as without them"""
    older = [dict(zip(("BF16", "I8", "BF16_MIN_BYTES", "I8_MIN_BYTES"), v))
             for v in itertools.product((None, 0, 1), (None, 0, 1), (None, 1, 64 * GiB), (None, 1, 64 * GiB))]
    newer = [dict(I6=a, I6_MIN_BYTES=b) for a in (None, 0, 1) for b in (None, 1, 64 * GiB)]
    for env in older:
        _env(monkeypatch, **env)
        want = [(capi.scan_tier(*a, **k), capi.scan_policy(*a, **k)) for a, k in CALLS]
        for mine in newer[1:]:
            _env(monkeypatch, **env, **mine)
            assert [(capi.scan_tier(*a, **k), capi.scan_policy(*a, **k)) for a, k in CALLS] == want, (env, mine)
            for a, k in CALLS:                                  # a call that reads the 6-bit shadow automatically is a call of tier 2
                k6 = {("i6_available" if n == "shadow_available" else n): v for n, v in k.items()}
                if mine["I6"] is None and capi.scan_i6(*a, **k6):
                    assert capi.scan_tier(*a, **k) == 2, (env, mine, a, k)


def test_the_pinned_answers_of_the_int8_tier_hold_with_the_variable_unset(monkeypatch):
    """tests/test_knn_i8_quant.py::test_scan_tier_under_every_environment, run here with RXGPU_SCAN_I6 and its threshold removed from the environment"""
    from .test_knn_i8_quant import test_scan_tier_under_every_environment as pinned
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    pinned(monkeypatch)
