"""-m gpu: the merge kernels of the single-query KNN chains on their own, through rxgpu_knn_merge_probe (reindexer_amd/csrc/knn_merge.hip):
knn_merge_lists over sorted lists, the candidate branch of knn_merge_final over unsorted pairs, and the insertion fold over the same pairs.

Expected result, in numpy: the valid pairs ordered by (distance with -0.0 -> +0.0, row), the first kk, padded with +inf / 0xFFFFFFFF; distances
are compared as bit patterns.  A NaN distance has no place in that order: there the insertion fold is the definition and the candidate branch
must equal it.

The path a kernel reports (selection or insertion merge) is deterministic and is asserted per case against the rule the kernels document,
restated here: keys are (distance, row) pairs, a selection collects every key at or below the kk-th smallest group head and gives way to the
insertion merge when more than 2048 are collected, when there are fewer than kk heads, or (candidates) on a NaN.  Equal distances alone do not
overflow the selection, because the row is part of the key: with distinct rows in random order such a case is answered by the selection like a
random one.  The all-equal cases that do overflow are the ones where the rows pack the smallest keys into fewer than kk groups ("equal_packed":
only kk = 64 at 65 536 candidates has groups long enough; lists of consecutive rows from kk = 46) and the ones where the pairs are identical
("identical", every size above 2048)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = np.uint32(0xFFFFFFFF)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
HEADS_MAX, CAND_MAX, THREADS = 4096, 2048, 512


@pytest.fixture(scope="module")
def rx():
    from reindexer_amd import capi
    capi.lib()
    assert capi.device_count() > 0
    return capi


def keys(d, r):
    b = np.ascontiguousarray(d, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    b ^= np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    k = (b.astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    k[r == INVALID] = ALL
    return k


def expected(d, r, kk):
    d, r = d.ravel(), r.ravel()
    valid = r != INVALID
    d, r = d[valid], r[valid]
    order = np.lexsort((r, np.where(d == 0, np.float32(0), d)))[:kk]
    out_d, out_r = np.full(kk, np.inf, np.float32), np.full(kk, INVALID, np.uint32)
    out_d[:order.size], out_r[:order.size] = d[order], r[order]
    return out_d, out_r, order.size


def lists_path(d, r, kk):
    nl = d.shape[0]
    if nl < kk or nl > HEADS_MAX:
        return False
    k = keys(d.ravel(), r.ravel()).reshape(nl, kk)
    bound = np.sort(k[:, 0])[kk - 1]
    walked = np.cumprod((r != INVALID) & (k <= bound), axis=1).sum()
    return bool(walked <= CAND_MAX)


def cand_path(d, r, kk):
    valid = r != INVALID
    if np.isnan(d[valid]).any():
        return False
    k = keys(d, r)
    bound = ALL
    if d.size > THREADS:
        heads = np.array([k[t::THREADS].min() for t in range(THREADS)])
        bound = np.sort(heads)[kk - 1]
        if bound == ALL:
            return False
    return bool((valid & (k <= bound)).sum() <= CAND_MAX)


def same(got, want):
    gd, gr, gc = got[:3]
    wd, wr, wc = want[:3]
    return gc == wc and np.array_equal(gr, wr) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------- lists

def sorted_lists(d, r, lens):
    """[nl][kk] pairs -> every list cut to its length, sorted by key, padded the way the scans pad"""
    nl, kk = d.shape
    cut = np.arange(kk)[None, :] >= np.asarray(lens)[:, None]
    d, r = np.where(cut, np.float32(np.inf), d).astype(np.float32), np.where(cut, INVALID, r).astype(np.uint32)
    order = np.argsort(keys(d.ravel(), r.ravel()).reshape(nl, kk), axis=1, kind="stable")
    return np.take_along_axis(d, order, 1), np.take_along_axis(r, order, 1)


def list_cases(rng, nl, kk):
    full = np.full(nl, kk)
    rows = rng.permutation(nl * kk).astype(np.uint32).reshape(nl, kk)
    rand = rng.normal(0, 1, (nl, kk)).astype(np.float32)
    yield "random", sorted_lists(rand, rows, full)
    yield "equal_random_rows", sorted_lists(np.ones((nl, kk), np.float32), rows, full)
    yield "equal_packed", sorted_lists(np.ones((nl, kk), np.float32), np.arange(nl * kk, dtype=np.uint32).reshape(nl, kk), full)
    yield "zeros", sorted_lists(rng.choice(np.array([0.0, -0.0, 0.5], np.float32), (nl, kk)), rows, full)
    yield "inf", sorted_lists(np.where(rng.random((nl, kk)) < 0.5, np.float32(np.inf), rand), rows, full)
    yield "padded", sorted_lists(rand, rows, rng.choice([0, 1, kk - 1, kk], nl))
    few = np.zeros(nl, int)
    few[: kk // 2] = 1
    yield "few", sorted_lists(rand, rows, few)
    if nl:
        one = np.abs(rand) + 1
        one[nl // 3] = -1 - np.arange(kk, dtype=np.float32)
        yield "one_list", sorted_lists(one, rows, full)


@pytest.mark.parametrize("kk", [1, 11, 64, 65, 101, 128])
def test_merge_lists(rx, kk):
    rng = np.random.default_rng(kk)
    for nl in (kk - 1, kk, 64, 65, 512, 513, 1024, 1025, 4096, 4097):
        for name, (d, r) in list_cases(rng, nl, kk):
            got = rx.knn_merge_probe(rx.MERGE_LISTS, d, r, kk)
            assert same(got, expected(d, r, kk)), (name, nl, kk)
            assert got[3] == lists_path(d, r, kk), (name, nl, kk, got[3])
            if name == "random" and 512 <= nl <= HEADS_MAX:
                assert got[3], (name, nl, kk)
            if name == "equal_packed" and kk >= 46 and kk <= nl <= HEADS_MAX:
                assert not got[3], (name, nl, kk)


# -------------------------------------------------------------------------------------------------------------------------- candidates

def cand_cases(rng, n, kk):
    rows = rng.permutation(n).astype(np.uint32) * np.uint32(3)
    rand = rng.normal(0, 1, n).astype(np.float32)
    ones = np.ones(n, np.float32)
    yield "random", rand, rows
    yield "ascending", np.arange(n, dtype=np.float32), rows
    yield "descending", np.arange(n, dtype=np.float32)[::-1].copy(), rows
    one = np.abs(rand) + 1
    at = np.arange(7, n, THREADS)[:kk]
    one[at] = -1 - np.arange(at.size, dtype=np.float32)
    yield "one_group", one, rows
    yield "equal_random_rows", ones, rows
    # position p belongs to group p % 512: the smallest rows fill group 0, then group 1, ...
    p = np.arange(n)
    per = -(-n // THREADS)
    yield "equal_packed", ones, ((p % THREADS) * per + p // THREADS).astype(np.uint32)
    yield "identical", ones, np.full(n, 5, np.uint32)
    yield "zeros", rng.choice(np.array([0.0, -0.0, 0.5], np.float32), n), rows
    yield "inf", np.where(rng.random(n) < 0.5, np.float32(np.inf), rand), rows
    yield "invalid", rand, np.where(rng.random(n) < 0.5, INVALID, rows)
    for where in sorted({0, n // 2, n - 1} if n else ()):
        d = rand.copy()
        d[where] = np.nan
        yield f"nan@{where}", d, rows


@pytest.mark.parametrize("kk", [1, 11, 64])
def test_merge_candidates(rx, kk):
    rng = np.random.default_rng(100 + kk)
    for n in (0, 1, kk - 1, kk, 255, 256, 257, 511, 512, 513, 2048, 2049, 13_000, 65_536):
        for name, d, r in cand_cases(rng, n, kk):
            got = rx.knn_merge_probe(rx.MERGE_CANDIDATES, d, r, kk)
            fold = rx.knn_merge_probe(rx.MERGE_FOLD, d, r, kk)
            assert not fold[3]
            assert same(got, fold), (name, n, kk)
            if not name.startswith("nan"):
                assert same(got, expected(d, r, kk)), (name, n, kk)
            assert got[3] == cand_path(d, r, kk), (name, n, kk, got[3])
            if name in ("random", "ascending", "descending"):
                assert got[3], (name, n, kk)
            if name.startswith("nan") or (name == "identical" and n > CAND_MAX) or (name == "equal_packed" and kk == 64 and n == 65_536):
                assert not got[3], (name, n, kk)
