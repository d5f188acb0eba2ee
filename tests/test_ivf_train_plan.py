"""The decisions of IVF training on the device (reindexer_amd/csrc/ivf_train_plan.h), compiled for the host (tests/cpp/ivf_train_plan_cpu.cc)
and pinned on the CPU: the 2^24 rule, the chunks of the gathered block against a scratch budget, the stable per-centroid segments of a training
list, the (centroid, column tile) units of the sums kernel and the scratch layout.  Every expectation is a restatement of the rule written
here, or a property stated in the test; the header's own output is never read as its expectation."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libivf_train_plan_cpu.so"
P = C.c_void_p
U32, U64, I32 = C.c_uint32, C.c_uint64, C.c_int
QUANTUM = 256       # kIvfGatherQuantum: a chunk is whole query tiles of the batched search
TILE_COLS = 64      # kIvfSumTileCols
WAVES_PER_BLOCK = 4 # kIvfSumWavesPerBlock
PLACE_TILE = 256    # kIvfPlaceTile
TABLE_WORDS = 4 << 20
MAX_BLOCKS = 512


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    for name, res, args in [
        ("ivf_plan_points_ok", I32, [U64]), ("ivf_plan_default_budget", U64, []), ("ivf_plan_chunk_rows", U64, [U64, U32, U64]),
        ("ivf_plan_chunks", U64, [U64, U64]), ("ivf_plan_chunk", None, [U64, U64, U64, P]), ("ivf_plan_place_shape", None, [U64, U64, P]),
        ("ivf_plan_place", None, [P, U32, U32, P, P]), ("ivf_plan_sum_tiles", U32, [U32]), ("ivf_plan_sum_waves", U64, [U64, U32]),
        ("ivf_plan_sum_blocks", U64, [U64, U32]), ("ivf_plan_sum_unit", None, [U64, U32, P]),
        ("ivf_plan_scratch", None, [U64, U64, U32, P]),
    ]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


# ---- the 2^24 rule
def test_a_step_takes_fewer_than_2_to_24_points(lib):
    """compute_centroids counts with += 1.0f; the device converts an integer count.  float32 holds every integer up to 2^24 and not
    2^24 + 1, so the two agree for every count a list of fewer than 2^24 points can produce — and the rule refuses from 2^24 on."""
    assert np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)            # where += 1.0f stops counting
    assert np.float32(2 ** 24 - 1) + np.float32(1) == np.float32(2 ** 24)        # ... and not before
    for n, ok in [(0, 1), (1, 1), (2 ** 24 - 1, 1), (2 ** 24, 0), (2 ** 24 + 1, 0), (2 ** 32, 0), (2 ** 40, 0)]:
        assert lib.ivf_plan_points_ok(n) == ok, n


# ---- chunks of the gathered block
def chunk_rows_py(n, dim, budget):
    rows = budget // (dim * 4) // QUANTUM * QUANTUM
    return min(max(rows, QUANTUM), n)


@pytest.mark.parametrize("dim", [1, 37, 64, 65, 768, 4096])
@pytest.mark.parametrize("budget", [0, 1000, 256 * 37 * 4, 1 << 20, 64 << 20])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 21845, 262144, 1_000_003, 2 ** 24 - 1])
def test_chunks_cover_the_list_once_within_the_budget(lib, n, dim, budget):
    rows = lib.ivf_plan_chunk_rows(n, dim, budget)
    assert rows == chunk_rows_py(n, dim, budget)
    # the budget holds a chunk, unless the budget is smaller than one query tile: then a chunk is that one tile (or the whole short list)
    assert rows * dim * 4 <= budget or rows == min(QUANTUM, n)
    assert rows <= n and (rows % QUANTUM == 0 or rows == n)
    chunks = lib.ivf_plan_chunks(n, rows)
    assert chunks == (0 if n == 0 else -(-n // rows))
    if chunks > 4096:   # walk the ends only
        which = list(range(3)) + list(range(chunks - 3, chunks))
    else:
        which = range(chunks)
    out = (U64 * 2)()
    covered, expect_first = 0, 0
    for i in which:
        lib.ivf_plan_chunk(n, rows, i, out)
        first, cnt = int(out[0]), int(out[1])
        assert first == i * rows and 1 <= cnt <= rows and first + cnt <= n
        assert cnt == rows or i == chunks - 1          # only the last chunk is short
        if chunks <= 4096:
            assert first == expect_first                # back to back: every position exactly once
            expect_first = first + cnt
            covered += cnt
    if chunks <= 4096:
        assert covered == n
    else:
        lib.ivf_plan_chunk(n, rows, chunks - 1, out)
        assert int(out[0]) + int(out[1]) == n


def test_default_budget_is_64_mib_and_cuts_the_readme_shape(lib):
    assert lib.ivf_plan_default_budget() == 64 << 20
    rows = lib.ivf_plan_chunk_rows(262144, 768, 64 << 20)
    assert rows == 21760 and rows * 768 * 4 <= 64 << 20 < (rows + QUANTUM) * 768 * 4
    assert lib.ivf_plan_chunks(262144, rows) == 13


# ---- stable placement
def place_shape_py(n, nlist):
    if n == 0:
        return 0, PLACE_TILE
    max_blocks = min(max(TABLE_WORDS // nlist, 1), MAX_BLOCKS)
    tiles = -(-n // PLACE_TILE)
    span = -(-tiles // max_blocks) * PLACE_TILE
    return -(-n // span), span


@pytest.mark.parametrize("n,nlist", [(0, 8), (1, 1), (255, 8), (256, 8), (257, 8), (6000, 10), (262144, 1024), (1_000_000, 1024),
                                     (2 ** 24 - 1, 65536), (2 ** 24 - 1, 5_000_000), (300_000, 1)])
def test_place_shape(lib, n, nlist):
    out = (U32 * 2)()
    lib.ivf_plan_place_shape(n, nlist, out)
    blocks, span = int(out[0]), int(out[1])
    assert (blocks, span) == place_shape_py(n, nlist)
    assert span % PLACE_TILE == 0 and blocks <= MAX_BLOCKS
    assert blocks * span >= n and (blocks == 0 or (blocks - 1) * span < n)       # the spans cover the list, none is empty
    assert blocks * nlist <= max(TABLE_WORDS, nlist)                             # the table's bound (one row at least)


def place(lib, assign, nlist):
    assign = np.ascontiguousarray(assign, np.uint32)
    seg_off = np.full(nlist + 1, 0xDEADBEEF, np.uint32)
    order = np.full(max(assign.size, 1), 0xDEADBEEF, np.uint32)
    lib.ivf_plan_place(assign.ctypes.data, assign.size, nlist, seg_off.ctypes.data, order.ctypes.data)
    return seg_off, order[:assign.size]


def check_placement(seg_off, order, assign, nlist):
    """seg_off = exclusive prefix of the counts; segment c = the positions with assign == c, ascending (the list order)"""
    counts = np.bincount(assign, minlength=nlist)[:nlist]
    assert np.array_equal(seg_off, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32))
    for c in range(nlist):
        assert np.array_equal(order[seg_off[c]:seg_off[c + 1]], np.flatnonzero(assign == c).astype(np.uint32)), c


@pytest.mark.parametrize("n,nlist", [(1, 1), (255, 8), (256, 8), (257, 8), (3000, 8), (2500, 16), (6000, 10), (70_000, 300), (140_000, 3)])
def test_segments_list_their_positions_in_list_order(lib, n, nlist):
    rng = np.random.default_rng(n + nlist)
    assign = rng.integers(0, nlist, n).astype(np.uint32)
    check_placement(*place(lib, assign, nlist), assign, nlist)


def test_segments_with_empty_centroids_and_one_centroid_holding_everything(lib):
    n, nlist = 6000, 10
    # one centroid takes every point: its segment is 0 .. n - 1, every other is empty and the offsets repeat
    for owner in (0, 4, 9):
        assign = np.full(n, owner, np.uint32)
        seg_off, order = place(lib, assign, nlist)
        assert np.array_equal(seg_off, np.array([0] * (owner + 1) + [n] * (nlist - owner), np.uint32))
        assert np.array_equal(order, np.arange(n, dtype=np.uint32))
    # empty centroids in front, in the middle and at the end
    rng = np.random.default_rng(5)
    assign = rng.choice(np.array([1, 2, 5, 7], np.uint32), n)
    seg_off, order = place(lib, assign, nlist)
    check_placement(seg_off, order, assign, nlist)
    for empty in (0, 3, 4, 6, 8, 9):
        assert seg_off[empty] == seg_off[empty + 1]
    # no points at all: every segment empty
    seg_off, order = place(lib, np.empty(0, np.uint32), nlist)
    assert np.array_equal(seg_off, np.zeros(nlist + 1, np.uint32)) and order.size == 0


def test_positions_without_a_centroid_are_left_out(lib):
    """an assignment >= nlist (the search found no centroid) takes no slot; the others keep their order"""
    assign = np.array([2, 0xFFFFFFFF, 2, 1, 7, 1, 0], np.uint32)
    seg_off, order = place(lib, assign, 3)
    assert seg_off.tolist() == [0, 1, 3, 5]
    assert order[:5].tolist() == [6, 3, 5, 0, 2]


# ---- the sums kernel's units
@pytest.mark.parametrize("dim,tiles", [(1, 1), (37, 1), (64, 1), (65, 2), (768, 12)])
def test_tile_counts(lib, dim, tiles):
    assert lib.ivf_plan_sum_tiles(dim) == tiles == -(-dim // TILE_COLS)
    for nlist in (1, 3, 1024):
        waves = lib.ivf_plan_sum_waves(nlist, dim)
        assert waves == nlist * tiles
        assert lib.ivf_plan_sum_blocks(nlist, dim) == -(-waves // WAVES_PER_BLOCK)
    # the units of three centroids cover every (centroid, column) exactly once, a centroid's tiles side by side
    seen = np.zeros((3, dim), np.int32)
    out = (U32 * 3)()
    for w in range(3 * tiles):
        lib.ivf_plan_sum_unit(w, dim, out)
        c, col0, cols = int(out[0]), int(out[1]), int(out[2])
        assert c == w // tiles and col0 == (w % tiles) * TILE_COLS and 1 <= cols <= TILE_COLS and col0 + cols <= dim
        seen[c, col0:col0 + cols] += 1
    assert np.all(seen == 1)


def test_scratch_parts_are_aligned_and_do_not_overlap(lib):
    out = (U64 * 7)()
    for n, nlist, dim in [(1, 1, 1), (6000, 10, 37), (262144, 1024, 768), (2 ** 24 - 1, 65536, 64)]:
        lib.ivf_plan_scratch(n, nlist, dim, out)
        o = [int(v) for v in out]
        blocks, _ = place_shape_py(n, nlist)
        sizes = [blocks * nlist * 4, (nlist + 1) * 4, n * 4, nlist * dim * 4, nlist * 4, 4]
        assert o[0] == 0
        for i in range(6):   # every part on a 256-byte boundary, large enough, none overlapping the next
            assert o[i] % 256 == 0 and o[i] + sizes[i] <= o[i + 1]
        assert o[6] % 256 == 0
