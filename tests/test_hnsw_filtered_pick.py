"""Which kernel an HNSW search under an allowed-rows bitmap gets (reindexer_amd/csrc/hnsw_kernel_pick.h: HnswPickInput::filtered,
pick_hnsw_filtered, hnsw_filtered_kernel_exists), compiled for the host (tests/cpp/hnsw_filtered_pick_cpu.cc) and pinned on the CPU.
With the flag unset the pick is the unfiltered one, field for field (tests/test_hnsw_kernel_pick.py pins its values through the shim that
knows no such flag); with it set the pick is never bare, has no helper or resident form, takes the lists with deleted nodes up to ef = 224
and the heaps above, and always names an instantiation hnsw_filtered.hip has."""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

from .test_hnsw_kernel_pick import DEFAULTS, DIMS, FIELDS, IN, Pick
from .test_hnsw_kernel_pick import LIB as PLAIN_LIB

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_filtered_pick_cpu.so"
SEARCH, TEAM, HELPER, SERVER, SERVER_WIDE, SERVER_SQ8, FILTERED, FILTERED_TEAM = range(8)
NB_FILTERED = {128: 2, 384: 0, 512: 0, 768: 12, 1024: 0, 1536: 0, 100: 0}   # the fixed batches of the family; every other size takes the generic one

# the shapes tests/test_hnsw_kernel_pick.py sweeps: every dimension, both row formats, bare or not, list sizes, launch sizes on both sides
# of every threshold, list or heaps, candidates in LDS or global, the visited-set sizes, the team switches and areas
SWEEP = dict(dim=DIMS, sq8=[0, 1], bare=[1, 0], ef=[10, 96, 97, 128, 129, 160, 161, 224, 225, 300, 1024], blocks=[1, 256, 257, 512, 513, 1024, 1025, 3072, 3073, 4096],
             sorted=[1, 0], global_cand=[0, 1])
EXTRA = [dict(vis_lds_log2=v, vis_hash_log2=16) for v in (0, 11, 12, 13, 14, 15)] + [dict(team=t) for t in (0, 1, 2)] + \
        [dict(team_max=0), dict(blocks=8, team_max=8), dict(blocks=9, team_max=8)] + \
        [dict(nbl=a, spec=b, maxM0=m, ef=96) for a in (0, 1) for b in (0, 1) for m in (32, 64, 128)] + \
        [dict(lds_cand_cap=c, nbl=1) for c in (9000, 10000)] + [dict(sorted=0, ef=1024, ef_cap=1024, lds_cand_cap=2048, blocks=300, dim=d) for d in (768, 1536)]


@pytest.fixture(scope="module")
def libs():
    if not LIB.exists() or not PLAIN_LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L, P = C.CDLL(str(LIB)), C.CDLL(str(PLAIN_LIB))
    L.hnsw_filtered_pick_cpu.restype = None
    L.hnsw_filtered_pick_cpu.argtypes = [C.c_void_p, C.c_void_p]
    L.hnsw_filtered_exists_cpu.restype = C.c_int
    L.hnsw_filtered_exists_cpu.argtypes = [C.c_int] * 6
    P.hnsw_pick_cpu.restype = None
    P.hnsw_pick_cpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return L, P


def _args(kw):
    assert set(kw) <= set(IN)
    return np.array([int({**DEFAULTS, **kw}[n]) for n in IN], np.uint32)


def pick(L, filtered, **kw):
    args = np.concatenate([_args(kw), np.array([filtered], np.uint32)])
    out = np.full(len(FIELDS) + 1, 0xDEAD, np.uint64)
    L.hnsw_filtered_pick_cpu(args.ctypes.data, out.ctypes.data)
    assert out[-1] == 0xDEAD
    return Pick(out[:-1])


def plain(P, **kw):
    args = _args(kw)
    out = np.full(len(FIELDS) + 1, 0xDEAD, np.uint64)
    P.hnsw_pick_cpu(0, args.ctypes.data, out.ctypes.data)
    return Pick(out[:-1])


def shapes():
    names = list(SWEEP)
    for values in itertools.product(*(SWEEP[n] for n in names)):
        kw = dict(zip(names, values))
        kw["ef_cap"] = (kw["ef"] + 63) & ~63
        yield kw
    yield from EXTRA


def test_unset_flag_leaves_every_pick_as_it_is(libs):
    L, P = libs
    n = 0
    for kw in shapes():
        a, b = pick(L, 0, **kw), plain(P, **kw)
        assert [getattr(a, f) for f in FIELDS] == [getattr(b, f) for f in FIELDS], kw
        assert a.family in (SEARCH, TEAM) and a.exists, kw
        n += 1
    assert n > 10000


def test_filtered_pick_is_never_bare_helped_or_served_and_always_exists(libs):
    L, _ = libs
    families = set()
    for kw in shapes():
        k = pick(L, 1, **kw)
        assert k.family in (FILTERED, FILTERED_TEAM), kw
        assert k.exists, (kw, vars(k))   # hnsw_filtered_kernel_exists: the dispatcher's guard
        # never bare: a list is the one with deleted nodes, whatever the graph says
        assert k.del_ == int(k.sorted > 0), kw
        use_list = kw.get("sorted", 1) and not kw.get("global_cand", 0) and kw.get("ef", 128) <= 224
        assert (k.sorted > 0) == bool(use_list), kw
        if k.sorted:
            ef = kw.get("ef", 128)
            assert k.sorted == (2 if ef <= 96 else 3 if ef <= 160 else 4), kw
        # no helper family, no resident family, no link-block or look-ahead area
        assert (k.nbl_off, k.spec_off, k.served) == (0, 0, 1), kw
        dim, sq8 = kw.get("dim", 768), kw.get("sq8", 0)
        assert (k.nb, k.sq8, k.global_cand) == (NB_FILTERED[dim], sq8, kw.get("global_cand", 0)), kw
        team = (not sq8 and k.nb > 0 and k.sorted > 0 and kw.get("team", 4) > 1 and kw.get("blocks", 1) <= kw.get("team_max", 256))
        assert k.family == (FILTERED_TEAM if team else FILTERED), kw
        assert (k.team, k.threads, k.latency) == ((4, 256, 1) if team else (1, 64, 0)), kw
        if not team:
            assert k.vis_lds == 0 and k.vis_hash_log2 == kw.get("vis_hash_log2", 0), kw
        assert k.needs_raised_lds == int(k.lds_bytes > (60 << 10)), kw
        families.add(k.family)
    assert families == {FILTERED, FILTERED_TEAM}


@pytest.mark.parametrize("sq8", [0, 1])
@pytest.mark.parametrize("ef,slots", [(96, 2), (160, 3), (224, 4), (225, 0)])
def test_list_sizes_and_heaps_past_224(libs, sq8, ef, slots):
    L, _ = libs
    for blocks in (1, 4096):
        for bare in (1, 0):
            k = pick(L, 1, ef=ef, ef_cap=(ef + 63) & ~63, sq8=sq8, blocks=blocks, bare=bare)
            assert (k.sorted, k.del_) == (slots, int(slots > 0))


def test_layout_of_the_dynamic_lds(libs):
    """heaps (8 bytes an entry) + the query fragment of a fixed float batch (256 bytes a block); a team adds its visited set one size up"""
    L, _ = libs
    heaps = (128 + 600) * 8
    k = pick(L, 1, blocks=4096)
    assert (k.family, k.lds_bytes, k.vis_lds) == (FILTERED, heaps + 256 * 12, 0)
    k = pick(L, 1, blocks=1)
    assert (k.family, k.lds_bytes, k.vis_lds, k.vis_hash_log2, k.needs_raised_lds) == (FILTERED_TEAM, heaps + 256 * 12 + 65536, 1, 14, 1)
    k = pick(L, 1, blocks=1, sq8=1)
    assert (k.family, k.lds_bytes) == (FILTERED, heaps)
    k = pick(L, 1, blocks=1, dim=512)   # no fixed batch of its own in this family: the generic one, no team
    assert (k.family, k.nb, k.lds_bytes) == (FILTERED, 0, heaps)
    k = pick(L, 1, blocks=1, global_cand=1, vis_hash_log2=15)
    assert (k.family, k.sorted, k.lds_bytes, k.vis_hash_log2) == (FILTERED, 0, 128 * 8 + 256 * 12, 15)


def test_instantiation_set(libs):
    L, _ = libs
    have = [(t, g, nb, q, s, d) for t in (0, 1) for g in (0, 1) for nb in (0, 2, 6, 8, 12, 16, 24) for q in (0, 1) for s in (0, 1, 2, 3, 4, 5) for d in (0, 1)
            if L.hnsw_filtered_exists_cpu(t, g, nb, q, s, d)]
    single = [x for x in have if not x[0]]
    team = [x for x in have if x[0]]
    # per row format and batch: heaps in LDS, heaps with global candidates, three lists with deleted nodes
    assert len(single) == 3 * 2 * 5 and {x[2] for x in single} == {0, 2, 12}
    assert all((s == 0 and not d) or (s in (2, 3, 4) and d and not g) for _, g, _, _, s, d in single)
    assert sorted(team) == sorted((1, 0, nb, 0, s, 1) for nb in (2, 12) for s in (2, 3, 4))
