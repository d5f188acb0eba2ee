"""The decisions of a row-range sharded index (reindexer_amd/csrc/shard_plan.h), compiled for the host (tests/cpp/shard_plan_cpu.cc) and pinned
on the CPU: row cut, rank layout, row-list split, exchange shape and routes, host merges, comparator, retry sizes — for device lists no one-GPU
box ever sees.  Every expectation is a plain restatement of the rule written here (the *_py functions, numpy) or a property stated in the
test; the header's own output is never read as its expectation."""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libshard_plan_cpu.so"
INVALID = 0xFFFFFFFF   # kInvalidRow
FUSED_K = 64           # kMaxFusedK
P = C.c_void_p
U32, U64, I32 = C.c_uint32, C.c_uint64, C.c_int


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    for name, res, args in [
        ("shard_plan_rows", U64, [U64, U32]), ("shard_plan_local_count", U64, [U64, U32, U64]), ("shard_plan_locate", None, [U64, U64, P]),
        ("shard_plan_piece", I32, [U64, U32, U64, U64, P]), ("shard_plan_prefix", I32, [P, U32, U64, P]),
        ("shard_plan_layout", None, [P, U32, U64, U32, P, P, P, P, P, P]), ("shard_plan_split", I32, [P, U64, U64, U64, U32, I32, P, P, P, P]),
        ("shard_plan_check_rows", I32, [P, U64, U64, I32, P]), ("shard_plan_exchange_shape", None, [U32, U32, U32, U32, U32, P]),
        ("shard_plan_routes", None, [P, U32, P, I32, I32, U32, U32, P]), ("shard_plan_less", I32, [C.c_float, U32, C.c_float, U32]),
        ("shard_plan_merge_topk", None, [U32, P, P, P, P, P, U64, U32, U32, P, P, P]),
        ("shard_plan_merge_ranges", U64, [U32, P, P, P, P, U64, U64, I32, P, P]), ("shard_plan_range_want", U64, [I32, U64, U64, U64]),
        ("shard_plan_range_attempts", I32, [I32]),
    ]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the row cut
def shard_rows_py(capacity, n):
    return (-(-capacity // n) + 31) // 32 * 32


def local_count_py(rows, s, count):
    return min(max(count - s * rows, 0), rows)


@pytest.mark.parametrize("capacity,n,rows,fill,counts", [
    (1000, 3, 352, 900, [352, 352, 196]),           # the number tests/test_gpu_sharded_map.py pins on the device
    (3000, 5, 608, 2000, [608, 608, 608, 176, 0]),
    (3000, 4, 768, 700, [700, 0, 0, 0]),
    (3, 8, 32, 3, [3, 0, 0, 0, 0, 0, 0, 0]),        # most shards have capacity 0
    (2 ** 32 - 2, 64, 67108864, 2 ** 32 - 2, [67108864] * 63 + [67108862]),
])
def test_row_cut(lib, capacity, n, rows, fill, counts):
    assert rows == shard_rows_py(capacity, n) and rows % 32 == 0 and rows * n >= capacity   # the literals above against the rule
    assert lib.shard_plan_rows(capacity, n) == rows
    assert [lib.shard_plan_local_count(rows, s, fill) for s in range(n)] == counts == [local_count_py(rows, s, fill) for s in range(n)]
    caps = [lib.shard_plan_local_count(rows, s, capacity) for s in range(n)]
    assert sum(caps) == capacity and caps == [local_count_py(rows, s, capacity) for s in range(n)]
    out = (U64 * 2)()
    for row in {0, min(rows, capacity) - 1, capacity - 1, capacity // 2} | {s * rows + d for s in range(1, n) for d in (-1, 0, 1) if s * rows + d < capacity}:
        lib.shard_plan_locate(rows, row, out)
        assert (out[0], out[1]) == divmod(row, rows) and out[0] < n


def test_upload_pieces_around_a_boundary(lib):
    """Upload ranges that start and end exactly on, one before and one after a shard boundary: the pieces are disjoint, lie inside their
    shards and add up to the range."""
    rows, n = 352, 3
    ab = (U64 * 2)()
    edges = [0, 1, 351, 352, 353, 703, 704, 705, 1000]
    for first, end in itertools.combinations(edges, 2):
        covered = []
        for s in range(n):
            hit = lib.shard_plan_piece(rows, s, first, end - first, ab)
            lo, hi = max(first, s * rows), min(end, (s + 1) * rows)
            assert hit == int(lo < hi), (first, end, s)
            if hit:
                assert (ab[0], ab[1]) == (lo, hi)
                covered += list(range(ab[0], ab[1]))
        assert covered == list(range(first, min(end, n * rows)))
    assert lib.shard_plan_piece(rows, 1, 352, 0, ab) == 0   # an empty range touches nothing


def test_prefix_rule(lib):
    def prefix(counts, rows=352):
        a = np.array(counts, np.uint64)
        t = U64(0)
        ok = lib.shard_plan_prefix(a.ctypes.data, len(counts), rows, C.byref(t))
        return t.value if ok else None
    assert prefix([352, 352, 196]) == 900
    assert prefix([352, 100, 0]) == 452
    assert prefix([352, 352, 352]) == 1056
    assert prefix([0, 0, 0]) == 0
    assert prefix([100, 0, 0]) == 100
    assert prefix([352, 100, 1]) is None     # a partial shard, then a non-empty one
    assert prefix([0, 1, 0]) is None
    assert prefix([100, 352, 0]) is None
    assert prefix([353, 0, 0]) is None       # more than a shard holds
    assert prefix([352, 352, 353]) is None


# ---- the rank layout
def layout(L, devices, rows=352):
    n = len(devices)
    dv = np.array(devices, np.int32)
    head, rank_dev = np.zeros(2, np.uint32), np.full(n, -1, np.int32)
    rank, slot, pos, base = [np.full(m, 0xEEEEEEEE, np.uint32) for m in (n, n, n, n * n)]
    L.shard_plan_layout(dv.ctypes.data, n, rows, INVALID, *(a.ctypes.data for a in (head, rank_dev, rank, slot, pos, base)))
    nranks, slots = int(head[0]), int(head[1])
    return dict(nranks=nranks, slots=slots, rank_dev=rank_dev[:nranks].tolist(), rank=rank.tolist(), slot=slot.tolist(), pos=pos.tolist(),
                base=base[:nranks * slots].tolist(), rest=base[nranks * slots:])


@pytest.mark.parametrize("devices", [[0], [0, 0, 0], [0, 1], [0, 1, 0, 2, 2], [5, 3, 5, 3, 5], list(range(64))], ids=str)
def test_rank_layout(lib, devices):
    rows = 352
    l = layout(lib, devices, rows)
    first_seen = list(dict.fromkeys(devices))
    assert l["rank_dev"] == first_seen and l["nranks"] == len(first_seen)
    assert l["slots"] == max(devices.count(d) for d in first_seen)
    assert [l["rank_dev"][r] for r in l["rank"]] == devices                      # a shard's rank is its device's
    for d in first_seen:                                                         # the shards of one device take slots 0, 1, ... in shard order
        assert [l["slot"][s] for s, dv in enumerate(devices) if dv == d] == list(range(devices.count(d)))
    assert l["pos"] == [r * l["slots"] + t for r, t in zip(l["rank"], l["slot"])]
    assert len(set(l["pos"])) == len(devices) and max(l["pos"]) < l["nranks"] * l["slots"]   # a bijection onto the used positions
    want = [INVALID] * (l["nranks"] * l["slots"])
    for s, p in enumerate(l["pos"]):
        want[p] = s * rows
    assert l["base"] == want and (l["rest"] == 0xEEEEEEEE).all()
    assert l["base"].count(INVALID) == l["nranks"] * l["slots"] - len(devices)


# ---- the row-list split
def split(L, ids, count, rows, n, ordered):
    a = np.array(ids, np.uint32)
    at, sizes = U64(0), np.zeros(n, np.uint64)
    local, where = np.full(max(len(ids), 1), 0xEEEEEEEE, np.uint32), np.full(max(len(ids), 1), 0xEEEEEEEE, np.uint32)
    rule = L.shard_plan_split(a.ctypes.data, len(ids), count, rows, n, int(ordered), C.byref(at), sizes.ctypes.data, local.ctypes.data, where.ctypes.data)
    at2 = U64(0)
    assert L.shard_plan_check_rows(a.ctypes.data, len(ids), count, int(ordered), C.byref(at2)) == rule and (rule == 0 or at2.value == at.value)
    if rule:
        return rule, at.value
    cuts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    assert cuts[-1] == len(ids)
    return [local[cuts[s]:cuts[s + 1]].tolist() for s in range(n)], [where[cuts[s]:cuts[s + 1]].tolist() for s in range(n)]


def test_row_list_split(lib):
    OK_IDS = [0, 351, 352, 703, 704, 899]
    local, where = split(lib, OK_IDS, 900, 352, 3, True)
    assert local == [[0, 351], [0, 351], [0, 195]]
    assert all(w == [0xEEEEEEEE] * len(l) for w, l in zip(where, local))   # the ordered form keeps no scatter table
    assert split(lib, [], 900, 352, 3, True)[0] == [[], [], []]
    assert split(lib, [899], 900, 352, 3, True)[0] == [[], [], [195]]
    NOT_INCREASING, OUT_OF_RANGE = 1, 2
    assert split(lib, [0, 5, 5, 900], 900, 352, 3, True) == (NOT_INCREASING, 2)      # equal neighbours (before the id out of range behind them)
    assert split(lib, [0, 400, 399, 10], 900, 352, 3, True) == (NOT_INCREASING, 2)   # a descent
    assert split(lib, [0, 351, 900], 900, 352, 3, True) == (OUT_OF_RANGE, 2)         # an id equal to count
    assert split(lib, [900], 900, 352, 3, True) == (OUT_OF_RANGE, 0)
    assert split(lib, [7, 900, 3], 900, 352, 3, False) == (OUT_OF_RANGE, 1)


def test_unordered_split_round_trips_through_where(lib):
    rng = np.random.default_rng(3)
    ids = [899, 704, 704, 352, 351, 0, 0, 703] + rng.integers(0, 900, 50).tolist()
    local, where = split(lib, ids, 900, 352, 3, False)
    back = np.full(len(ids), -1, np.int64)
    for s in range(3):
        assert len(local[s]) == len(where[s]) and where[s] == sorted(where[s])       # list order inside a shard
        assert all(0 <= v < 352 for v in local[s])
        back[where[s]] = np.array(local[s], np.int64) + s * 352
    assert back.tolist() == ids


# ---- the exchange
def test_exchange_shape(lib):
    out = (U64 * 10)()
    for nq, kk, nranks, slots, dim in [(1, 11, 1, 3, 24), (4, 64, 1, 3, 24), (256, 64, 8, 1, 768), (1, 1, 3, 2, 1), (9, 10, 2, 4, 4096)]:
        lib.shard_plan_exchange_shape(nq, kk, nranks, slots, dim, out)
        qbytes, list_words = nq * dim * 4, 2 * nq * kk          # one shard's piece: [nq][kk] distance bits | [nq][kk] rows
        local = list_words * slots * 4                          # a rank sends `slots` pieces
        outb = (2 * nq * kk + nq) * 4                           # [nq][kk] distances | [nq][kk] rows | [nq] counts
        assert list(out) == [qbytes, list_words, local, local * nranks, outb, 0, nq * kk, 2 * nq * kk, max(qbytes, outb), outb]
        assert out[7] * 4 + nq * 4 == outb                      # the counts end the buffer


def routes(L, devices, counts, has_exchange, has_row_list, kk):
    dv, c, out = np.array(devices, np.int32), np.array(counts, np.uint64), (I32 * 3)()
    L.shard_plan_routes(dv.ctypes.data, len(devices), c.ctypes.data, int(has_exchange), int(has_row_list), kk, FUSED_K, out)
    return tuple(bool(v) for v in out)


def test_routes(lib):
    full = [352, 352, 196]
    assert routes(lib, [0, 0, 0], full, True, False, 11) == (True, True, False)
    assert routes(lib, [0, 0, 0], full, True, False, 64) == (True, True, False)
    assert routes(lib, [0, 0, 0], full, True, False, 65) == (False, False, False)          # past the fused scan's lists
    assert routes(lib, [0, 0, 0], full, False, False, 11) == (False, False, False)         # no exchange
    assert routes(lib, [0, 0, 0], full, True, True, 11)[0] is False                        # a row list goes through the host ...
    assert routes(lib, [0, 0, 0], full, True, True, 11)[1] is True                         # ... (HNSW has none)
    assert routes(lib, [0, 0, 0], [352, 352, 6], True, False, 11) == (False, True, False)  # a shard holding 6 rows at kk = 11: host
    assert routes(lib, [0, 0, 0], [352, 352, 6], True, False, 6) == (True, True, False)
    assert routes(lib, [0, 0, 0], [352, 348, 0], True, False, 11) == (True, True, True)    # an empty shard: exchange, with a hole
    assert routes(lib, [0, 1, 0], full, True, False, 11) == (True, True, True)             # rank 1 pads its second slot
    assert routes(lib, [0, 1], [352, 352], True, False, 11) == (True, True, False)


# ---- the comparator
def old_less(da, ra, db, rb):
    return bool(da < db or (not (db < da) and ra < rb))   # the former spelling of the range tails and sort_dist_row


def test_comparator_is_a_strict_weak_order_and_the_old_order_without_nan(lib):
    rng = np.random.default_rng(11)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1e-45, 3.5], np.float32)
    d = np.concatenate([special, special, rng.normal(0, 1, 12).astype(np.float32)])
    r = rng.integers(0, 6, d.shape[0]).astype(np.uint32)      # few rows: equal (dist, row) pairs occur
    n = d.shape[0]
    less = np.array([[lib.shard_plan_less(d[i], r[i], d[j], r[j]) for j in range(n)] for i in range(n)], bool)   # n * n = 1024 pairs
    assert not less.diagonal().any()                          # irreflexive
    assert not (less & less.T).any()                          # asymmetric
    reach = less.astype(np.int64) @ less.astype(np.int64)
    assert not ((reach > 0) & ~less).any()                    # transitive
    equiv = ~less & ~less.T                                   # ... and so is "neither is less"
    assert not (((equiv.astype(np.int64) @ equiv.astype(np.int64)) > 0) & ~equiv).any()
    nan = np.isnan(d)
    assert less[np.ix_(~nan, nan)].all() and not less[np.ix_(nan, ~nan)].any()   # NaN last
    for i in np.flatnonzero(~nan):
        for j in np.flatnonzero(~nan):
            assert less[i, j] == old_less(d[i], r[i], d[j], r[j])
    assert not lib.shard_plan_less(-0.0, 4, 0.0, 4) and not lib.shard_plan_less(0.0, 4, -0.0, 4)
    assert lib.shard_plan_less(0.0, 3, -0.0, 4) and lib.shard_plan_less(-0.0, 3, 0.0, 4)


# ---- the merges
def lex_order(dist, rows):
    return np.lexsort((rows, dist, np.isnan(dist)))   # (isnan, dist, global row); +0 == -0 for lexsort too


def merge_topk(L, lists, strides, shard_rows, nq, k):
    """lists[s] = (dist [nq][stride_s], row [nq][stride_s], count [nq])"""
    ns = len(lists)
    off = np.concatenate([[0], np.cumsum([l[0].size for l in lists])]).astype(np.uint64)
    dist = np.concatenate([l[0].ravel() for l in lists] + [np.zeros(1, np.float32)]).astype(np.float32)
    row = np.concatenate([l[1].ravel() for l in lists] + [np.zeros(1, np.uint32)]).astype(np.uint32)
    cnt = np.concatenate([l[2] for l in lists]).astype(np.uint32)
    st = np.array(strides, np.uint64)
    od, orow, oc = np.full((nq, k), -7.0, np.float32), np.full((nq, k), 0xEEEEEEEE, np.uint32), np.full(nq, 0xEEEEEEEE, np.uint32)
    L.shard_plan_merge_topk(ns, dist.ctypes.data, row.ctypes.data, off.ctypes.data, cnt.ctypes.data, st.ctypes.data, shard_rows, nq, k, od.ctypes.data, orow.ctypes.data,
                            oc.ctypes.data)
    return od, orow, oc


def check_topk(L, lists, strides, shard_rows, nq, k):
    od, orow, oc = merge_topk(L, lists, strides, shard_rows, nq, k)
    for q in range(nq):
        d = np.concatenate([l[0][q, :l[2][q]] for l in lists])
        r = np.concatenate([l[1][q, :l[2][q]].astype(np.uint64) + s * shard_rows for s, l in enumerate(lists)]).astype(np.uint32)
        o = lex_order(d, r)[:k]
        assert oc[q] == len(o)
        assert np.array_equal(orow[q, :len(o)], r[o]) and np.array_equal(bits(od[q, :len(o)]), bits(d[o])), q
        assert (orow[q, len(o):] == 0xEEEEEEEE).all()          # nothing written past the count


def shard_list(rng, nq, stride, count, values):
    d = rng.choice(values, (nq, max(stride, 1))).astype(np.float32)[:, :stride]
    r = np.stack([rng.permutation(300)[:stride] for _ in range(nq)]).astype(np.uint32).reshape(nq, stride)
    return d, r, np.full(nq, count, np.uint32) if np.isscalar(count) else np.array(count, np.uint32)


def test_topk_merge(lib):
    rng = np.random.default_rng(5)
    ties = np.array([0.5, 0.5, 0.25, 1.0], np.float32)                       # equal distances across three shards: the global row decides
    zeros = np.array([0.0, -0.0, 0.5], np.float32)
    with_nan = np.array([np.nan, 0.5, 0.25, 2.0], np.float32)
    for kk in (1, 5, 11):
        check_topk(lib, [shard_list(rng, 3, kk, kk, ties) for _ in range(3)], [kk] * 3, 352, 3, kk)
        check_topk(lib, [shard_list(rng, 3, kk, kk, zeros) for _ in range(3)], [kk] * 3, 352, 3, kk)
        check_topk(lib, [shard_list(rng, 2, kk, kk, with_nan if s == 1 else ties) for s in range(3)], [kk] * 3, 352, 2, kk)   # NaN in one shard
        check_topk(lib, [shard_list(rng, 2, kk, kk, with_nan) for _ in range(3)], [kk] * 3, 352, 2, kk)                       # ... and in all
    # counts shorter than kk (a pre-filtered shard with few listed rows), one shard with none
    lists = [shard_list(rng, 4, 11, [11, 3, 0, 7], ties), shard_list(rng, 4, 11, [0, 0, 0, 2], ties), shard_list(rng, 4, 11, [5, 11, 0, 1], ties)]
    check_topk(lib, lists, [11] * 3, 352, 4, 11)
    # HNSW: a shard's lists have the stride min(k, rows it holds) — a 3-row shard at k = 10
    lists = [shard_list(rng, 5, 10, [10, 9, 10, 4, 10], ties), shard_list(rng, 5, 3, [3, 3, 2, 0, 3], ties), shard_list(rng, 5, 10, 10, ties)]
    check_topk(lib, lists, [10, 3, 10], 352, 5, 10)
    # all shards empty
    od, orow, oc = merge_topk(lib, [shard_list(rng, 2, 4, 0, ties) for _ in range(3)], [4] * 3, 352, 2, 4)
    assert (oc == 0).all() and (orow == 0xEEEEEEEE).all()
    # global rows of the last of 64 shards at the largest capacity still fit 32 bits
    big = shard_rows_py(2 ** 32 - 2, 64)
    lists = [shard_list(rng, 1, 2, 2, ties) for _ in range(64)]
    check_topk(lib, lists, [2] * 64, big, 1, 5)


def merge_ranges(L, hits, shard_rows, cap, concat):
    ns = len(hits)
    off = np.concatenate([[0], np.cumsum([len(h[0]) for h in hits])]).astype(np.uint64)
    dist = np.concatenate([h[0] for h in hits] + [np.zeros(1, np.float32)]).astype(np.float32)
    row = np.concatenate([h[1] for h in hits] + [np.zeros(1, np.uint32)]).astype(np.uint32)
    total = np.array([len(h[0]) for h in hits], np.uint64)
    od, orow = np.full(cap + 1, -7.0, np.float32), np.full(cap + 1, 0xEEEEEEEE, np.uint32)
    n = L.shard_plan_merge_ranges(ns, dist.ctypes.data, row.ctypes.data, off.ctypes.data, total.ctypes.data, shard_rows, cap, int(concat), od.ctypes.data, orow.ctypes.data)
    assert orow[cap] == 0xEEEEEEEE and od[cap] == -7.0          # never past cap
    return n, od[:cap], orow[:cap]


def test_range_merges(lib):
    rng = np.random.default_rng(8)
    vals = np.array([0.5, 0.5, 0.25, -0.0, 0.0, np.nan, 3.0], np.float32)
    hits = [(rng.choice(vals, m).astype(np.float32), rng.permutation(352)[:m].astype(np.uint32)) for m in (7, 0, 12)]
    d = np.concatenate([h[0] for h in hits])
    r = np.concatenate([h[1].astype(np.uint64) + s * 352 for s, h in enumerate(hits)]).astype(np.uint32)
    total = 19
    for cap in (0, 5, 18, 19, 20, 40):                           # below, at and above the total
        for concat in (False, True):
            n, od, orow = merge_ranges(lib, hits, 352, cap, concat)
            o = (np.arange(total) if concat else lex_order(d, r))[:cap]   # HNSW: shard after shard, in the order the shards reported
            assert n == total
            assert np.array_equal(orow[:len(o)], r[o]) and np.array_equal(bits(od[:len(o)]), bits(d[o]))
            assert (orow[len(o):] == 0xEEEEEEEE).all()
    for concat in (False, True):
        assert merge_ranges(lib, [(np.zeros(0, np.float32), np.zeros(0, np.uint32))] * 3, 352, 4, concat)[0] == 0


def test_retry_sizes(lib):
    assert (lib.shard_plan_range_attempts(0), lib.shard_plan_range_attempts(1)) == (2, 8)
    for cap in (0, 1, 63, 64, 65, 255, 256, 257, 10 ** 6):
        assert lib.shard_plan_range_want(0, cap, 0, 0) == max(cap, 64)            # brute force: first max(cap, 64) ...
        assert lib.shard_plan_range_want(1, cap, 0, 0) == max(cap, 256)           # HNSW: first max(cap, 256) ...
    assert lib.shard_plan_range_want(0, 10, 64, 977) == 977                       # ... then the size the shard reported
    for want, reported in [(256, 257), (256, 5000), (1024, 1025), (4096, 100)]:
        assert lib.shard_plan_range_want(1, 10, want, reported) == max(4 * want, 2 * reported)   # ... then max(4 want, 2 reported)
