"""The decisions of one packed upload (reindexer_amd/csrc/ft_packed_plan.h), compiled for the host (tests/cpp/ft_packed_plan_cpu.cc) and pinned
on the CPU: launch order, offsets, pieces, staging layout, chunks, gather ranges and the pool.  Every expectation is a plain restatement of the
rule written here (the *_py functions) or a property stated in the test; the header's own output is never read as its expectation."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libft_packed_plan_cpu.so"
PARAMS = -3
SEG = 1024            # kFtPackedSegBytes
RANGE_DOCS = 8192     # kFtRangeDocs
NONE = (1 << 64) - 1  # no chunk target
P = C.c_void_p


class Out(C.Structure):
    _fields_ = [("code", C.c_int32), ("msg", C.c_char * 252), ("scalars", C.c_uint64 * 8), ("nchunks", C.c_uint32), ("pad", C.c_uint32), ("order", P),
                ("off", P), ("afp", P), ("seg_first", P), ("seg_word", P), ("chunk_first", P), ("gather", P)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.ft_packed_plan_cpu.restype = C.c_int
    L.ft_packed_plan_cpu.argtypes = [C.c_uint32, P, P, C.c_int, C.c_uint64, C.POINTER(Out)]
    L.ft_packed_pool_cpu.restype = C.c_uint64
    L.ft_packed_pool_cpu.argtypes = [C.c_uint32, P, P, P]
    L.ft_packed_seg_bytes.restype = C.c_uint32
    assert L.ft_packed_seg_bytes() == SEG
    return L


def plan(L, lens, afp=None, wave=True, target=NONE, tables=True):
    """tables=False: lengths only (no piece -> word table, no gather ranges: the overflow cases name 2^32 pieces)"""
    n = len(lens)
    ln = np.array(lens, np.uint64)
    af = np.array(afp if afp is not None else [0] * n, np.uint64)
    o = Out()
    order, off, oafp = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint64), np.zeros(n, np.uint64)
    seg_first, chunk_first = np.full(n + 1, 0xFFFFFFFF, np.uint32), np.zeros(n + 1, np.uint32)
    nsegs_py = int(sum(pieces_py(l) for l in lens)) if tables and wave else 0
    seg_word = np.full(max(nsegs_py, 1), 0xFFFFFFFF, np.uint32)
    gather = np.zeros((n + 1) * 4 * 2, np.uint32)
    o.order, o.off, o.afp, o.seg_first, o.chunk_first = (a.ctypes.data for a in (order, off, oafp, seg_first, chunk_first))
    o.seg_word = seg_word.ctypes.data if tables else None
    o.gather = gather.ctypes.data if tables else None
    rc = L.ft_packed_plan_cpu(n, ln.ctypes.data, af.ctypes.data, int(wave), target, C.byref(o))
    assert rc == o.code
    if rc:
        return dict(code=rc, msg=o.msg.decode())
    s = dict(zip(["total_bytes", "nsegs", "o_off", "o_afp", "o_sw", "o_sf", "in_bytes", "nthr"], (int(v) for v in o.scalars)))
    nthr = s["nthr"]
    return dict(s, code=0, order=order, off=off, afp=oafp, seg_first=seg_first, seg_word=seg_word[:s["nsegs"]], chunk_first=chunk_first[:o.nchunks + 1],
                gather=gather[:o.nchunks * nthr * 2].reshape(o.nchunks, nthr, 2))


# ---- the rules, restated
def bucket_py(l):
    return int(l).bit_length()   # 64 - clz(len); 0 for an empty stream


def order_py(lens):
    return sorted(range(len(lens)), key=lambda w: -bucket_py(lens[w]))   # (sorted is stable: input order inside a bucket)


def pieces_py(l):
    return max(1, -(-int(l) // SEG))


def al(v):
    return (v + 255) & ~255


def pool_py(counts):
    """counts: (n, npos, nent, last_doc) per word -> (slices per word or None, n_ranges per word, pool bytes)"""
    at, slices, ranges = 0, [], []
    for n, npos, nent, last in counts:
        if not n:
            slices.append(None)
            ranges.append(0)
            continue
        nr = last // RANGE_DOCS + 2
        offs = []
        for elems, width in zip((n, n + 1, npos, n + 1, nent, nent, nent, nr), (4, 4, 8, 4, 1, 4, 4, 4)):
            offs.append(at)
            at = al(at + elems * width)
        slices.append(offs)
        ranges.append(nr)
    return slices, ranges, at


def check_order(lens, order):
    assert sorted(order.tolist()) == list(range(len(lens))), "a permutation"
    b = [bucket_py(lens[w]) for w in order]
    assert all(b[i] >= b[i + 1] for i in range(len(b) - 1)), "longest bucket first"
    assert all(order[i] < order[i + 1] for i in range(len(b) - 1) if b[i] == b[i + 1]), "input order inside a bucket"


# ---- the cases
def test_order_is_a_stable_bucket_sort_longest_first(lib):
    lens = [0, 1, 1, 2, 3, 1024, 1023, 1025, 0, 7]
    p = plan(lib, lens)
    check_order(lens, p["order"])
    assert p["order"].tolist() == [5, 7, 6, 9, 3, 4, 1, 2, 0, 8]   # worked out by hand: buckets 11, 11, 10, 3, 2, 2, 1, 1, 0, 0
    lens = np.random.default_rng(1234).integers(0, 5000, 1000).tolist()
    p = plan(lib, lens)
    check_order(lens, p["order"])
    assert p["order"].tolist() == order_py(lens)


def test_offsets_are_contiguous_in_launch_order(lib):
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 5000, 300).tolist()
    afp = rng.integers(0, 1 << 40, 300).tolist()
    p = plan(lib, lens, afp)
    off, order = p["off"], p["order"]
    assert off[0, 0] == 0 and np.array_equal(off[1:, 0], off[:-1, 1])
    assert np.array_equal(off[:, 1] - off[:, 0], np.array(lens, np.uint64)[order])
    assert int(off[-1, 1]) == sum(lens) == p["total_bytes"]
    assert np.array_equal(p["afp"], np.array(afp, np.uint64)[order])


def test_pieces_of_1024_bytes(lib):
    lens = [2048, 1025, 1024, 1023, 1, 0]   # already in launch order
    p = plan(lib, lens)
    assert p["order"].tolist() == list(range(6))
    assert np.diff(p["seg_first"].astype(np.int64)).tolist() == [2, 2, 1, 1, 1, 1] == [pieces_py(l) for l in lens]
    assert p["seg_first"].tolist() == [0, 2, 4, 5, 6, 7, 8] and p["nsegs"] == 8
    assert p["seg_word"].tolist() == [0, 0, 1, 1, 2, 3, 4, 5]
    for l, want in zip((0, 1, 1023, 1024, 1025, 2048), (1, 1, 1, 1, 2, 2)):
        assert plan(lib, [l])["nsegs"] == want == pieces_py(l)


def test_too_many_pieces_are_refused(lib):
    """Lengths are numbers here, no memory behind them.  Three words of 2^41 bytes are 2^31 pieces each: the second reaches 2^32."""
    r = plan(lib, [1 << 41] * 3, tables=False)
    assert r["code"] == PARAMS and r["msg"] == "rxgpu_ft_set_words_packed: too many stream bytes in one call"
    assert plan(lib, [((1 << 32) - 1) * SEG], tables=False)["code"] == PARAMS      # 2^32 - 1 pieces: the bound itself
    ok = plan(lib, [((1 << 32) - 2) * SEG], tables=False)                           # one piece less: accepted
    assert ok["code"] == 0 and ok["nsegs"] == (1 << 32) - 2
    ok = plan(lib, [((1 << 31) - 1) * SEG] * 2, tables=False)
    assert ok["code"] == 0 and ok["nsegs"] == (1 << 32) - 2 and ok["seg_first"].tolist() == [0, (1 << 31) - 1, (1 << 32) - 2]
    assert plan(lib, [1 << 41] * 3, wave=False, tables=False)["code"] == 0        # the thread-per-word kernels have no pieces


@pytest.mark.parametrize("wave", [True, False])
def test_staging_layout(lib, wave):
    lens = np.random.default_rng(8).integers(0, 3000, 77).tolist()
    p = plan(lib, lens, wave=wave)
    n, total = len(lens), sum(lens)
    assert p["nsegs"] == (sum(pieces_py(l) for l in lens) if wave else 0)
    regions = [(0, total + 16), (p["o_off"], n * 16), (p["o_afp"], n * 8), (p["o_sw"], p["nsegs"] * 4), (p["o_sf"], (n + 1) * 4)]
    assert all(o % 256 == 0 for o, _ in regions) and p["in_bytes"] % 256 == 0
    assert p["o_off"] >= total + 16   # the 16 zero bytes behind the streams
    for (o, b), (nxt, _) in zip(regions, regions[1:] + [(p["in_bytes"], 0)]):
        assert o + b <= nxt
    assert [o for o, _ in regions[1:]] + [p["in_bytes"]] == [al(total + 16), al(total + 16) + al(n * 16), al(total + 16) + al(n * 16) + al(n * 8),
                                                            al(total + 16) + al(n * 16) + al(n * 8) + al(p["nsegs"] * 4),
                                                            al(total + 16) + al(n * 16) + al(n * 8) + al(p["nsegs"] * 4) + al((n + 1) * 4)]


def test_chunks_are_whole_words_closed_at_the_target(lib):
    lens = [1000] * 10
    assert plan(lib, lens)["chunk_first"].tolist() == [0, 10]   # no target: one chunk
    rng = np.random.default_rng(3)
    lens = rng.integers(100, 9000, 2000)
    lens = (lens * (3.5 * (1 << 20) / lens.sum())).astype(np.int64)
    lens[0] += int(3.5 * (1 << 20)) - int(lens.sum())
    assert int(lens.sum()) == int(3.5 * (1 << 20))
    target = 1 << 20
    p = plan(lib, lens.tolist(), target=target)
    cf = p["chunk_first"].tolist()
    assert cf[0] == 0 and cf[-1] == len(lens) and all(a < b for a, b in zip(cf, cf[1:])), "whole words, no empty chunk (the last included)"
    sizes = [int((p["off"][b - 1, 1] - p["off"][a, 0])) for a, b in zip(cf, cf[1:])]
    for (a, b), size in list(zip(zip(cf, cf[1:]), sizes))[:-1]:
        assert size >= target > size - int(p["off"][b - 1, 1] - p["off"][b - 1, 0]), "the word that closes a chunk is the one that reaches the target"
    assert len(cf) - 1 in (3, 4) and sum(sizes) == int(lens.sum())
    # a target the last word alone reaches: it still closes no chunk of its own behind it
    assert plan(lib, [10, 10, 5000], target=15)["chunk_first"].tolist() == [0, 1, 3]   # launch order: 5000, 10, 10


@pytest.mark.parametrize("total_mb,nthr", [(1, 1), (9, 4)])
def test_gather_ranges_partition_every_chunk(lib, total_mb, nthr):
    """One thread up to 8 MB of streams, four above; chunks with fewer words than threads included (big words in front: launch order)."""
    lens = [total_mb << 19, total_mb << 18] + [(total_mb << 18) // 50] * 50
    p = plan(lib, lens, target=total_mb << 18)
    assert p["nthr"] == nthr == (4 if sum(lens) > (8 << 20) else 1)
    cf = p["chunk_first"].tolist()
    assert any(b - a < nthr for a, b in zip(cf, cf[1:])) or nthr == 1
    for c, (a, b) in enumerate(zip(cf, cf[1:])):
        g = p["gather"][c].tolist()
        assert g[0][0] == a and g[-1][1] == b and all(x[1] == y[0] for x, y in zip(g, g[1:])) and all(x[0] <= x[1] for x in g)
        assert [x for x in g] == [[a + (b - a) * t // nthr, a + (b - a) * (t + 1) // nthr] for t in range(nthr)]


def test_pool_layout(lib):
    counts = [(5, 9, 7, 100), (0, 0, 0, 0), (300, 1000, 450, 20000), (1, 1, 1, 0), (64, 64, 64, 8191), (64, 70, 66, 8192)]
    c = np.array(counts, np.uint32)
    slices, ranges = np.zeros((len(counts), 8), np.uint64), np.zeros(len(counts), np.uint32)
    total = int(lib.ft_packed_pool_cpu(len(counts), c.ctypes.data, slices.ctypes.data, ranges.ctypes.data))
    want_slices, want_ranges, want_total = pool_py(counts)
    assert total == want_total and ranges.tolist() == want_ranges == [2, 0, 4, 2, 2, 3]
    at = 0
    for k, (n, npos, nent, last) in enumerate(counts):
        if not n:
            assert not slices[k].any()   # a word without postings takes no bytes: its neighbours lie back to back
            continue
        assert slices[k].tolist() == want_slices[k]
        sizes = [e * w for e, w in zip((n, n + 1, npos, n + 1, nent, nent, nent, int(ranges[k])), (4, 4, 8, 4, 1, 4, 4, 4))]
        for o, b in zip(slices[k].tolist(), sizes):   # doc, pos_off, fpos, ent_off, ent_field, ent_tf, ent_first, range_off: in this order, disjoint
            assert o % 256 == 0 and o >= at
            at = o + b
    assert total >= at and total % 256 == 0
    for last, nr in ((0, 2), (8191, 2), (8192, 3)):
        r = np.zeros(1, np.uint32)
        lib.ft_packed_pool_cpu(1, np.array([1, 1, 1, last], np.uint32).ctypes.data, None, r.ctypes.data)
        assert int(r[0]) == nr
