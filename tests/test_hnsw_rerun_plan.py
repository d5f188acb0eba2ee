"""The re-run ladder of an HNSW search (reindexer_amd/csrc/hnsw_rerun_plan.h: HnswRerunLadder), compiled for the host
(tests/cpp/hnsw_launch_plan_cpu.cc) and pinned on the CPU with the test in the device's place: it says which counts "come back" behind the
first pass and behind every step, the ladder says what runs again.  The expected values are the rules as they stood inline in
hnsw_search_impl before the ladder was split out of it: ties once more on the heaps, overflows once more with the largest LDS heap, then the
global tiers of 64 K entries and of one entry per node — and the two counters that follow from them."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_launch_plan_cpu.so"

TIE, OVER = 0xFFFFFFFE, 0xFFFFFFFF
TIES, LDS_MAX, GLOBAL0, GLOBAL1 = 0, 1, 2, 3
M1, M10 = 1_000_000, 10_000_000
# what plan_hnsw_search gives the shapes below (pinned by tests/test_hnsw_launch_plan.py): words of a bitset, searches per re-run launch
WORDS_1M, SLOTS_1M = 31250, 17179
WORDS_10M, SLOTS_10M = 312500, 1717


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.hnsw_rerun_cpu.restype = C.c_int
    L.hnsw_rerun_cpu.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.hnsw_rerun_constants.argtypes = [C.c_void_p]
    return L


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    import os
    for name in list(os.environ):
        if name.startswith("RXGPU_HNSW_"):
            monkeypatch.delenv(name)


class Step:
    def __init__(self, words, ids):
        (self.rung, _, self.slots, ties, self.vis_hash_log2, self.visited_words, self.lds_cand_cap, self.vis_lds_log2, self.gcand_cap) = (int(w) for w in words)
        self.name = "hnsw_ties" if ties else "hnsw_redo"
        self.ids = [int(q) for q in ids]

    def overrides(self):
        return (self.vis_hash_log2, self.visited_words, self.lds_cand_cap, self.vis_lds_log2, self.gcand_cap)


def counts(nq, ties=(), over=()):
    """what nq searches leave: a count each, kHnswTie for `ties`, kHnswOverflow for `over`"""
    c = np.arange(nq, dtype=np.uint32) % 11   # (any count from 0 to k = 10)
    c[list(ties)] = TIE
    c[list(over)] = OVER
    return c


def run(L, rounds, n=M1, ef=128, bare=True, helper=0, filtered=False):
    """-> (steps, tie_reruns, lds_reruns, ended in the overflow error).  The ladder asks exactly len(rounds) times: once behind the first pass
    and once behind every step."""
    rounds = np.ascontiguousarray(np.stack(rounds), np.uint32)
    nq = rounds.shape[1]
    steps = np.full(8 * 9 + 1, 0xDEAD, np.uint64)
    ids = np.full(8 * nq + 1, 0xDEAD, np.uint32)
    totals = np.zeros(4, np.uint64)
    args = (n, 768, int(bare), nq, 10, ef, 0, int(filtered), helper)
    n_steps = L.hnsw_rerun_cpu(*args, rounds.ctypes.data, len(rounds), steps.ctypes.data, 8, ids.ctypes.data, 8 * nq, totals.ctypes.data)
    assert n_steps == len(rounds) - 1
    assert L.hnsw_rerun_cpu(*args, rounds.ctypes.data, len(rounds) - 1, steps.copy().ctypes.data, 8, ids.copy().ctypes.data, 8 * nq, totals.copy().ctypes.data) == -1
    assert steps[n_steps * 9] == 0xDEAD and ids[int(totals[3])] == 0xDEAD
    out, at = [], 0
    for s in range(n_steps):
        w = steps[s * 9:(s + 1) * 9]
        out.append(Step(w, ids[at:at + int(w[1])]))
        at += int(w[1])
    assert at == totals[3]
    return out, int(totals[0]), int(totals[1]), bool(totals[2])


def test_constants(lib):
    c = np.zeros(3, np.uint32)
    lib.hnsw_rerun_constants(c.ctypes.data)
    assert list(c) == [TIE, OVER, 4096]


def test_all_clean(lib):
    assert run(lib, [counts(8)]) == ([], 0, 0, False)
    assert run(lib, [counts(1)]) == ([], 0, 0, False)


def test_ties_only(lib):
    steps, ties, lds, err = run(lib, [counts(8, ties=(6, 1, 4)), counts(8)])
    assert (ties, lds, err) == (3, 0, False)
    (s,) = steps
    assert (s.rung, s.name, s.ids, s.slots) == (TIES, "hnsw_ties", [1, 4, 6], SLOTS_1M)
    assert s.overrides() == (0, WORDS_1M, 1024, 13, 0)   # the first pass's bitset and LDS hash set, the plan's heap area, no global heap
    # 10M rows: the first pass's visited set is the hash set of 2^14 words, 32768 searches a launch — the ties' too
    steps, ties, lds, err = run(lib, [counts(3, ties=(0, 1, 2)), counts(3)], n=M10)
    assert (ties, lds, err) == (3, 0, False)
    (s,) = steps
    assert (s.rung, s.ids, s.slots) == (TIES, [0, 1, 2], 32768) and s.overrides() == (14, 16384, 1024, 13, 0)


def test_a_tie_that_overflows_on_the_heaps(lib):
    steps, ties, lds, err = run(lib, [counts(8, ties=(2, 5)), counts(8, over=(2,)), counts(8)])
    assert (ties, lds, err) == (2, 1, False)
    a, b = steps
    assert (a.rung, a.ids) == (TIES, [2, 5])
    assert (b.rung, b.name, b.ids, b.slots) == (LDS_MAX, "hnsw_redo", [2], SLOTS_1M)
    assert b.overrides() == (0, WORDS_1M, 2048, 0, 0)   # a bitset, the largest LDS heap, no hash set in LDS


def test_overflows_beside_ties_wait_for_the_tie_rung(lib):
    # query 3 overflowed in the first pass, query 6 on the tie re-run: both are collected behind it, in ascending order
    steps, ties, lds, err = run(lib, [counts(8, ties=(6, 0), over=(3,)), counts(8, over=(3, 6)), counts(8)], n=M10)
    assert (ties, lds, err) == (2, 2, False)
    a, b = steps
    assert (a.rung, a.ids) == (TIES, [0, 6])
    assert (b.rung, b.ids, b.slots) == (LDS_MAX, [3, 6], SLOTS_10M) and b.overrides() == (0, WORDS_10M, 2048, 0, 0)


def test_ef_512_has_the_largest_lds_heap_already(lib):
    steps, ties, lds, err = run(lib, [counts(8, over=(7, 0)), counts(8)], ef=512)
    assert (ties, lds, err) == (0, 0, False)
    (s,) = steps
    assert (s.rung, s.name, s.ids, s.slots) == (GLOBAL0, "hnsw_redo", [0, 7], 2048)   # 2^30 / (65536 * 8)
    assert s.overrides() == (0, WORDS_1M, 2048, 15, 65536)


def test_lds_cand_cap_hook_skips_the_lds_rung(lib, monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "4")
    steps, ties, lds, err = run(lib, [counts(8, over=(1, 2)), counts(8)], helper=5)
    assert (ties, lds, err) == (0, 5, False)   # what the helpers had queued, nothing for a rung that did not run
    (s,) = steps
    assert (s.rung, s.ids, s.slots) == (GLOBAL0, [1, 2], 2048) and s.overrides() == (0, WORDS_1M, 4, 13, 65536)


def test_big_ef_starts_on_the_global_tiers(lib):
    # no first pass: what the counts array holds at the first question is nobody's result
    steps, ties, lds, err = run(lib, [counts(5), counts(5)], ef=2048)
    assert (ties, lds, err) == (0, 0, False)
    (s,) = steps
    assert (s.rung, s.name, s.ids, s.slots) == (GLOBAL0, "hnsw_redo", [0, 1, 2, 3, 4], 2048)
    assert s.overrides() == (0, WORDS_1M, 2048, 17, 65536)
    steps, ties, lds, err = run(lib, [counts(5, ties=(1,)), counts(5, over=(4,)), counts(5)], ef=2048)
    assert (ties, lds, err) == (0, 0, False)
    assert [(s.rung, s.ids, s.gcand_cap) for s in steps] == [(GLOBAL0, [0, 1, 2, 3, 4], 65536), (GLOBAL1, [4], M1 + 1)]


def test_small_graph_has_one_global_tier(lib):
    # 1000 nodes: both tiers hold one entry per node (1001) — the second is never offered, a search still flagged is the overflow error
    steps, ties, lds, err = run(lib, [counts(4, over=(2,)), counts(4, over=(2,)), counts(4, over=(2,))], n=1000)
    assert (ties, lds, err) == (0, 1, True)
    a, b = steps
    assert (a.rung, a.ids, a.slots) == (LDS_MAX, [2], 32768) and a.overrides() == (0, 32, 2048, 0, 0)
    assert (b.rung, b.ids, b.slots) == (GLOBAL0, [2], 32768) and b.overrides() == (0, 32, 1024, 13, 1001)
    steps, ties, lds, err = run(lib, [counts(4, over=(2,)), counts(4, over=(2,)), counts(4)], n=1000)
    assert len(steps) == 2 and not err


def test_gcand_cap_hook_walks_both_tiers(lib, monkeypatch):
    monkeypatch.setenv("RXGPU_HNSW_GCAND_CAP", "8")
    rounds = [counts(6, over=(0, 2, 3, 5)), counts(6, over=(0, 3, 5)), counts(6, over=(3, 5)), counts(6)]
    steps, ties, lds, err = run(lib, rounds, n=M10)
    assert (ties, lds, err) == (0, 4, False)
    a, b, c = steps
    assert (a.rung, a.ids, a.slots) == (LDS_MAX, [0, 2, 3, 5], SLOTS_10M)
    assert (b.rung, b.ids, b.slots) == (GLOBAL0, [0, 3, 5], SLOTS_10M) and b.overrides() == (0, WORDS_10M, 1024, 13, 8)
    # one entry per node at 10M rows: 2^30 / (10 000 001 * 8) = 13 searches per launch
    assert (c.rung, c.name, c.ids, c.slots) == (GLOBAL1, "hnsw_redo", [3, 5], 13) and c.overrides() == (0, WORDS_10M, 1024, 13, M10 + 1)
    steps, ties, lds, err = run(lib, rounds[:3] + [counts(6, over=(5,))], n=M10)
    assert len(steps) == 3 and err   # one entry per node overflowed


@pytest.mark.parametrize("helper, want", [(0, 3), (2, 2 + 1), (5, 5 + 0), (5000, 4096 + 0)])
def test_helper_accounting(lib, helper, want):
    # three searches take the LDS rung; those the helpers had queued are among them and counted once
    steps, ties, lds, err = run(lib, [counts(8, over=(1, 3, 4)), counts(8)], helper=helper)
    assert [(s.rung, s.ids) for s in steps] == [(LDS_MAX, [1, 3, 4])]
    assert (ties, lds, err) == (0, want, False)


def test_helper_entries_count_without_a_step(lib):
    assert run(lib, [counts(8)], helper=7) == ([], 0, 7, False)
    assert run(lib, [counts(8)], helper=4097) == ([], 0, 4096, False)


def test_filtered_call_walks_the_same_rungs(lib):
    # a call under a bitmap is never bare: the sorted list holds ef <= 224, and its re-runs are those of any other call
    steps, ties, lds, err = run(lib, [counts(8, ties=(2,), over=(5,)), counts(8, over=(5,)), counts(8)], bare=False, filtered=True)
    assert (ties, lds, err) == (1, 1, False)
    assert [(s.rung, s.ids) for s in steps] == [(TIES, [2]), (LDS_MAX, [5])]
