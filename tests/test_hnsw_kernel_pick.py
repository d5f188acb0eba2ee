"""Which kernel an HNSW search gets (reindexer_amd/csrc/hnsw_kernel_pick.h: pick_hnsw_search, pick_hnsw_helper, pick_hnsw_server,
hnsw_lds_layout), compiled for the host (tests/cpp/hnsw_kernel_pick_cpu.cc) and pinned on the CPU.  The expected values are written out by
hand from the launch switches as they stood in hnsw_search.hip and hnsw_server.hip before the pick was split out of them; the byte counts
are sums of: 8 bytes a heap entry, 256 bytes a 64-float block of the query fragment, 4 << log2 bytes of a visited set in LDS, 8192 bytes of
link blocks, 17664 bytes of look-ahead area."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libhnsw_kernel_pick_cpu.so"

IN = ["dim", "ef", "ef_cap", "lds_cand_cap", "sorted", "bare", "sq8", "team", "team_max", "vis_lds", "vis_lds_log2", "vis_hash_log2", "has_visited",
      "sq8_query", "nbl", "spec", "maxM0", "blocks", "global_cand"]
FIELDS = ["family", "nb", "sorted", "del_", "latency", "sq8", "global_cand", "team", "threads", "lds_bytes", "vis_lds", "vis_hash_log2", "nbl_off", "spec_off",
          "needs_raised_lds", "served", "exists"]
SEARCH, TEAM, HELPER, SERVER, SERVER_WIDE, SERVER_SQ8 = range(6)
# a single query of the sorted-list search over a bare graph of 768 floats: ef = 128, 600 restart entries, the 2^13-word set allowed in LDS
DEFAULTS = dict(dim=768, ef=128, ef_cap=128, lds_cand_cap=600, sorted=1, bare=1, sq8=0, team=4, team_max=256, vis_lds=0, vis_lds_log2=13, vis_hash_log2=0,
                has_visited=1, sq8_query=1, nbl=0, spec=0, maxM0=32, blocks=1, global_cand=0)
HEAPS = (128 + 600) * 8   # 5824
NBL, SPEC = 8192, 17664
K60, K150 = 60 << 10, 150 << 10

DIMS = [128, 384, 512, 768, 1024, 1536, 100]
NB_FLOAT = {128: 2, 384: 0, 512: 8, 768: 12, 1024: 16, 1536: 24, 100: 0}
NB_SQ8 = {128: 2, 384: 6, 512: 8, 768: 12, 1024: 16, 1536: 24, 100: 0}
NB_SQ8_DEL = {128: 2, 384: 0, 512: 0, 768: 12, 1024: 0, 1536: 0, 100: 0}
NB_HELPER = {128: 2, 384: 0, 512: 0, 768: 12, 1024: 16, 1536: 24, 100: 0}


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.hnsw_pick_cpu.restype = None
    L.hnsw_pick_cpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.hnsw_lds_layout_cpu.restype = None
    L.hnsw_lds_layout_cpu.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.hnsw_pick_constants.argtypes = [C.c_void_p]
    return L


class Pick:
    def __init__(self, values):
        for name, v in zip(FIELDS, values):
            setattr(self, name, int(v))


def pick(L, which, **kw):
    assert set(kw) <= set(IN)
    args = np.array([int({**DEFAULTS, **kw}[n]) for n in IN], np.uint32)
    out = np.full(len(FIELDS) + 1, 0xDEAD, np.uint64)
    L.hnsw_pick_cpu(which, args.ctypes.data, out.ctypes.data)
    assert out[-1] == 0xDEAD   # the shim wrote exactly the fields named here
    return Pick(out[:-1])


def search(L, **kw):
    k = pick(L, 0, **kw)
    assert k.exists and k.served and k.needs_raised_lds == (k.lds_bytes > K60)
    return k


def test_constants_and_layout(lib):
    c = np.zeros(4, np.uint32)
    lib.hnsw_pick_constants(c.ctypes.data)
    assert list(c) == [NBL, SPEC, 32, 11]   # kHnswNblBytes, kHnswSpecBytes, kHnswNblRows, kHnswSpecLog2
    o = np.zeros(3, np.uint64)
    for args, want in [((128, 600, 0, 12, 0), (1024, 5824, 8896)), ((128, 600, 1, 12, 0), (1024, 1024, 4096)), ((128, 600, 0, 12, 1), (1024, 5824, 5824)),
                       ((256, 1024, 0, 24, 0), (2048, 10240, 16384)), ((0, 0, 0, 0, 0), (0, 0, 0))]:
        lib.hnsw_lds_layout_cpu(*args, o.ctypes.data)
        assert tuple(int(x) for x in o) == want   # candidate heap, query fragment, visited set


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("sq8", [0, 1])
@pytest.mark.parametrize("bare", [1, 0])
def test_search_distance_blocks_by_dim(lib, dim, sq8, bare):
    """a large batch (no team, no latency form): NB follows the list of sizes; the heaps know one list, the sorted list two over codes"""
    nb_sorted = (NB_SQ8 if bare else NB_SQ8_DEL)[dim] if sq8 else NB_FLOAT[dim]
    nb_heap = NB_SQ8[dim] if sq8 else NB_FLOAT[dim]
    k = search(lib, dim=dim, sq8=sq8, bare=bare, blocks=4096)
    assert (k.family, k.nb, k.sorted, k.del_, k.sq8, k.latency, k.global_cand) == (SEARCH, nb_sorted, 2 if bare else 3, 1 - bare, sq8, 0, 0)
    assert (k.team, k.threads, k.lds_bytes) == (1, 64, HEAPS + (0 if sq8 else 256 * nb_sorted))
    assert (k.vis_lds, k.vis_hash_log2, k.nbl_off, k.spec_off) == (0, 0, 0, 0)
    k = search(lib, dim=dim, sq8=sq8, bare=bare, blocks=4096, sorted=0, vis_hash_log2=15)
    assert (k.family, k.nb, k.sorted, k.del_, k.sq8, k.latency, k.global_cand) == (SEARCH, nb_heap, 0, 0, sq8, 0, 0)
    assert (k.threads, k.lds_bytes, k.vis_lds, k.vis_hash_log2) == (64, HEAPS + (0 if sq8 else 256 * nb_heap), 0, 15)
    # the candidate heap in global scratch: the sorted list is not taken even where the caller allows it, and the LDS heap area is the result heap alone
    k = search(lib, dim=dim, sq8=sq8, bare=bare, blocks=4096, global_cand=1)
    assert (k.family, k.nb, k.sorted, k.del_, k.global_cand, k.latency) == (SEARCH, nb_heap, 0, 0, 1, 0)
    assert k.lds_bytes == 1024 + (0 if sq8 else 256 * nb_heap)


@pytest.mark.parametrize("sq8", [0, 1])
@pytest.mark.parametrize("ef,bare_slots,del_slots", [(96, 2, 2), (97, 2, 3), (128, 2, 3), (129, 4, 3), (160, 4, 3), (161, 4, 4), (224, 4, 4)])
def test_sorted_list_entries_a_lane_by_ef(lib, sq8, ef, bare_slots, del_slots):
    for blocks in (1, 4096):   # the team form and the batch form
        assert search(lib, ef=ef, sq8=sq8, blocks=blocks).sorted == bare_slots
        k = search(lib, ef=ef, sq8=sq8, bare=0, blocks=blocks)
        assert (k.sorted, k.del_) == (del_slots, 1)
    assert search(lib, ef=ef, sq8=sq8, sorted=0).sorted == 0


# (dim, blocks) -> family, latency, visited set in LDS; floats over a bare graph, team_max = 256
@pytest.mark.parametrize("dim,blocks,family,latency,vis_lds", [
    (768, 256, TEAM, 1, 1), (768, 257, SEARCH, 1, 1), (768, 512, SEARCH, 1, 1), (768, 513, SEARCH, 1, 0), (768, 1024, SEARCH, 1, 0), (768, 1025, SEARCH, 1, 0),
    (768, 3072, SEARCH, 1, 0), (768, 3073, SEARCH, 0, 0),
    (1024, 256, TEAM, 1, 1), (1024, 257, SEARCH, 1, 1), (1024, 1025, SEARCH, 1, 0), (1024, 3072, SEARCH, 1, 0), (1024, 3073, SEARCH, 0, 0),
    (1536, 256, TEAM, 1, 1), (1536, 257, SEARCH, 1, 1), (1536, 512, SEARCH, 1, 1), (1536, 513, SEARCH, 1, 0), (1536, 1024, SEARCH, 1, 0), (1536, 1025, SEARCH, 0, 0),
    (1536, 3072, SEARCH, 0, 0),
    (512, 256, TEAM, 1, 1), (512, 257, SEARCH, 0, 0), (512, 1024, SEARCH, 0, 0), (128, 256, TEAM, 1, 1), (128, 257, SEARCH, 0, 0),
    (384, 1, SEARCH, 0, 0), (384, 512, SEARCH, 0, 0), (100, 1, SEARCH, 0, 0)])
def test_search_form_by_launch_size(lib, dim, blocks, family, latency, vis_lds):
    nb = NB_FLOAT[dim]
    for bare in (1, 0):
        k = search(lib, dim=dim, blocks=blocks, bare=bare)
        assert (k.family, k.nb, k.latency, k.vis_lds) == (family, nb, latency, vis_lds)
        assert (k.team, k.threads) == ((4, 256) if family == TEAM else (1, 64))
        # a team takes the set one size up (2^14 words), the latency form as allowed (2^13)
        vis = (65536 if family == TEAM else 32768) if vis_lds else 0
        assert k.lds_bytes == HEAPS + 256 * nb + vis and k.vis_hash_log2 == ((14 if family == TEAM else 13) if vis_lds else 0)
        assert k.needs_raised_lds == (family == TEAM)   # 5824 + 256 nb + 65536 > 60 KB
    # the heap search of the same launch: never a team; the latency form by the same thresholds
    k = search(lib, dim=dim, blocks=blocks, sorted=0)
    assert (k.family, k.latency, k.sorted, k.threads) == (SEARCH, int(nb > 8 and blocks <= (1024 if nb > 16 else 3072)), 0, 64)
    assert k.vis_lds == int(k.latency and blocks <= 512)
    # ... with its candidate heap in global scratch: the visited set stays in HBM
    k = search(lib, dim=dim, blocks=blocks, sorted=0, global_cand=1, vis_hash_log2=15)
    assert (k.family, k.latency, k.vis_lds, k.vis_hash_log2, k.lds_bytes) == (SEARCH, int(nb > 8 and blocks <= (1024 if nb > 16 else 3072)), 0, 15, 1024 + 256 * nb)
    # over codes there is neither a team nor a latency form
    for bare in (1, 0):
        k = search(lib, dim=dim, blocks=blocks, sq8=1, bare=bare)
        assert (k.family, k.latency, k.vis_lds, k.team, k.threads, k.lds_bytes) == (SEARCH, 0, 0, 1, 64, HEAPS)


def test_team_needs_more_than_one_wavefront_and_few_searches(lib):
    assert search(lib, team=1).family == SEARCH and search(lib, team=0).family == SEARCH
    assert search(lib, team=2).team == 4   # (the one team form has four wavefronts)
    assert search(lib, team_max=0).family == SEARCH and search(lib, blocks=8, team_max=8).family == TEAM and search(lib, blocks=9, team_max=8).family == SEARCH
    assert search(lib, sorted=0).family == SEARCH


@pytest.mark.parametrize("log2,team_log2,team_lds,lat_log2,lat_lds", [
    (0, None, 8896, None, 8896), (11, 11, 8896 + 8192, 11, 8896 + 8192), (12, 13, 8896 + 32768, 12, 8896 + 16384), (13, 14, 8896 + 65536, 13, 8896 + 32768),
    (14, 14, 8896 + 65536, None, 8896), (15, None, 8896, None, 8896)])
def test_visited_set_in_lds_by_allowed_size(lib, log2, team_log2, team_lds, lat_log2, lat_lds):
    """768 floats: 5824 bytes of heaps + 3072 of query fragment = 8896; a team goes one size up from 2^12 and 2^13 within 64 KB, the latency form
    takes the size as allowed up to 32 KB; where the set stays in HBM the caller's vis_hash_log2 passes through"""
    k = search(lib, blocks=1, vis_lds_log2=log2, vis_hash_log2=16)
    assert (k.family, k.vis_lds, k.vis_hash_log2, k.lds_bytes) == (TEAM, int(team_log2 is not None), team_log2 or 16, team_lds)
    assert k.needs_raised_lds == (team_lds > K60)
    k = search(lib, blocks=300, vis_lds_log2=log2, vis_hash_log2=16)
    assert (k.family, k.latency, k.vis_lds, k.vis_hash_log2, k.lds_bytes) == (SEARCH, 1, int(lat_log2 is not None), lat_log2 or 16, lat_lds)
    assert not k.needs_raised_lds


def test_latency_form_keeps_dynamic_lds_under_60k(lib):
    # ef = 1024 on the heaps: (1024 + 2048) * 8 = 24576; 768 floats: + 3072 + 32768 = 60416 fits, 1536 floats: + 6144 + 32768 = 63488 does not
    k = search(lib, sorted=0, ef=1024, ef_cap=1024, lds_cand_cap=2048, blocks=300)
    assert (k.latency, k.vis_lds, k.lds_bytes, k.needs_raised_lds) == (1, 1, 60416, 0)
    k = search(lib, sorted=0, ef=1024, ef_cap=1024, lds_cand_cap=2048, blocks=300, dim=1536)
    assert (k.latency, k.vis_lds, k.lds_bytes, k.needs_raised_lds) == (1, 0, 30720, 0)
    # the search family past 60 KB (codes, the largest heaps and more): 7680 entries are 61440 bytes, 7744 are 61952
    assert not search(lib, sq8=1, sorted=0, ef=4096, ef_cap=4096, lds_cand_cap=3584).needs_raised_lds
    k = search(lib, sq8=1, sorted=0, ef=4096, ef_cap=4096, lds_cand_cap=3648)
    assert (k.lds_bytes, k.needs_raised_lds) == (61952, 1)


@pytest.mark.parametrize("bare", [1, 0])
@pytest.mark.parametrize("nbl,spec,maxM0", [(0, 0, 32), (1, 0, 32), (1, 0, 64), (0, 1, 32), (0, 1, 64), (1, 1, 32), (1, 1, 64), (1, 0, 128), (0, 1, 128),
                                            (1, 1, 128)])
def test_team_areas(lib, bare, nbl, spec, maxM0):
    at = 8896 + 65536   # 74432: heaps, query fragment, the 2^14-word set
    want_nbl = at if (nbl and not spec and maxM0 == 32) else 0
    want_spec = at if (spec and bare and maxM0 == 32) else 0   # (never both: the look-ahead keeps link blocks of its own)
    k = search(lib, bare=bare, nbl=nbl, spec=spec, maxM0=maxM0, ef=96)
    assert (k.family, k.nbl_off, k.spec_off, k.lds_bytes) == (TEAM, want_nbl, want_spec, at + (NBL if want_nbl else 0) + (SPEC if want_spec else 0))
    # not a team: no areas
    k = search(lib, bare=bare, nbl=nbl, spec=spec, maxM0=maxM0, ef=96, blocks=300)
    assert (k.family, k.nbl_off, k.spec_off, k.lds_bytes) == (SEARCH, 0, 0, 8896 + 32768)


def test_team_areas_stay_under_150k(lib):
    # (128 + 9000) * 8 + 3072 + 65536 = 141632: + 8192 = 149824 fits, + 17664 = 159296 does not; with 10000 entries 149632 + 8192 = 157824 does not
    k = search(lib, lds_cand_cap=9000, nbl=1)
    assert (k.family, k.nbl_off, k.lds_bytes, k.needs_raised_lds) == (TEAM, 141632, 149824, 1)
    k = search(lib, lds_cand_cap=9000, spec=1)
    assert (k.spec_off, k.lds_bytes) == (0, 141632)
    k = search(lib, lds_cand_cap=10000, nbl=1)
    assert (k.nbl_off, k.lds_bytes) == (0, 149632)
    assert 149632 + NBL > K150 >= 149824


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("ef_cap,heaps", [(128, 17408), (256, 18432)])   # (ef_cap + 2048) * 8
def test_helper(lib, dim, ef_cap, heaps):
    for bare in (1, 0):
        k = pick(lib, 1, dim=dim, ef_cap=ef_cap, lds_cand_cap=2048, sorted=0, bare=bare, blocks=8)
        nb = NB_HELPER[dim]   # floats: 512 has no helper form of its own
        assert (k.family, k.nb, k.sq8, k.sorted, k.del_, k.global_cand, k.latency, k.team, k.threads) == (HELPER, nb, 0, 0, 0, 0, int(nb > 8), 1, 64)
        assert (k.lds_bytes, k.needs_raised_lds, k.exists, k.nbl_off, k.spec_off, k.vis_lds) == (heaps + 256 * nb, 0, 1, 0, 0, 0)
        k = pick(lib, 1, dim=dim, ef_cap=ef_cap, lds_cand_cap=2048, sorted=0, bare=bare, sq8=1, blocks=8)
        nb = NB_SQ8_DEL[dim]   # codes: the two sizes every SQ8 graph has a fixed form for
        assert (k.family, k.nb, k.sq8, k.sorted, k.del_, k.latency, k.threads, k.lds_bytes, k.exists) == (HELPER, nb, 1, 0, 0, 0, 64, heaps, 1)


def test_helper_past_60k(lib):
    assert not pick(lib, 1, sq8=1, ef_cap=4096, lds_cand_cap=3584).needs_raised_lds   # 61440
    k = pick(lib, 1, sq8=1, ef_cap=4096, lds_cand_cap=4096)
    assert (k.lds_bytes, k.needs_raised_lds) == (65536, 1)


# the two classes of resident kernel: ef_cap = 128 with the 2^14-word set in LDS, ef_cap = 256 with the set of a slot in HBM
CLASS0 = dict(ef_cap=128, lds_cand_cap=1024, vis_lds=1, vis_lds_log2=14, vis_hash_log2=14, blocks=16)   # heaps 9216, set 65536
CLASS1 = dict(ef_cap=256, lds_cand_cap=1024, vis_lds=0, vis_lds_log2=0, vis_hash_log2=14, blocks=16)    # heaps 10240


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("bare", [1, 0])
def test_server_by_dim(lib, dim, bare):
    for cls, slots, fixed in ((CLASS0, 2, 9216 + 65536), (CLASS1, 4, 10240)):
        k = pick(lib, 2, dim=dim, bare=bare, **cls)
        nb = NB_FLOAT[dim]
        assert k.served == int(nb > 0)
        if k.served:
            assert (k.family, k.nb, k.sorted, k.del_, k.sq8, k.team, k.threads, k.exists) == (SERVER_WIDE if nb > 12 else SERVER, nb, slots, 1 - bare, 0, 4, 256, 1)
            assert (k.lds_bytes, k.needs_raised_lds, k.nbl_off, k.spec_off) == (fixed + 256 * nb, int(cls is CLASS0), 0, 0)
            assert (k.vis_lds, k.vis_hash_log2) == (cls["vis_lds"], 14)
        k = pick(lib, 2, dim=dim, bare=bare, sq8=1, **cls)
        nb = (NB_SQ8 if bare else NB_SQ8_DEL)[dim]
        assert k.served == int(nb > 0)
        if k.served:   # one wavefront a slot, no query fragment
            assert (k.family, k.nb, k.sorted, k.del_, k.sq8, k.team, k.threads, k.exists) == (SERVER_SQ8, nb, slots, 1 - bare, 1, 1, 64, 1)
            assert (k.lds_bytes, k.needs_raised_lds, k.nbl_off, k.spec_off) == (fixed, int(cls is CLASS0), 0, 0)


@pytest.mark.parametrize("sq8", [0, 1])
def test_server_gates(lib, sq8):
    assert pick(lib, 2, sq8=sq8, **CLASS0).served and pick(lib, 2, sq8=sq8, **CLASS1).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS0, "sorted": 0}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS0, "vis_lds": 0}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS0, "vis_lds_log2": 15}).served
    assert pick(lib, 2, sq8=sq8, **{**CLASS0, "vis_lds_log2": 13}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS1, "vis_lds": 1}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS1, "vis_lds_log2": 13}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS1, "has_visited": 0}).served
    assert not pick(lib, 2, sq8=sq8, **{**CLASS1, "vis_hash_log2": 13}).served
    assert pick(lib, 2, sq8=sq8, **{**CLASS0, "sq8_query": 0}).served == 1 - sq8   # the arrays of the mailbox over codes
    assert pick(lib, 2, sq8=sq8, **{**CLASS0, "ef_cap": 129}).served == 0 and pick(lib, 2, sq8=sq8, **{**CLASS1, "ef_cap": 129}).sorted == 4


def test_server_lds_gate_and_areas(lib):
    # floats: (128 + 10000) * 8 + 3072 + 65536 = 149632 is served, (128 + 11000) * 8 + ... = 157632 is not
    k = pick(lib, 2, **{**CLASS0, "lds_cand_cap": 10000})
    assert (k.served, k.lds_bytes) == (1, 149632)
    assert not pick(lib, 2, **{**CLASS0, "lds_cand_cap": 11000}).served
    # codes: the gate measures the float layout (query fragment included), the launch gets the layout without it
    k = pick(lib, 2, sq8=1, **{**CLASS0, "lds_cand_cap": 10490})   # 84944 + 3072 + 65536 = 153552 <= 153600
    assert (k.served, k.lds_bytes) == (1, 84944 + 65536)
    assert not pick(lib, 2, sq8=1, **{**CLASS0, "lds_cand_cap": 10500}).served   # 85024 + 3072 + 65536 = 153632
    at = 9216 + 3072 + 65536   # 77824
    k = pick(lib, 2, nbl=1, **CLASS0)
    assert (k.nbl_off, k.spec_off, k.lds_bytes) == (at, 0, at + NBL)
    k = pick(lib, 2, spec=1, nbl=1, **CLASS0)
    assert (k.nbl_off, k.spec_off, k.lds_bytes) == (0, at, at + SPEC)
    assert pick(lib, 2, spec=1, bare=0, **CLASS0).lds_bytes == at and pick(lib, 2, nbl=1, maxM0=64, **CLASS0).lds_bytes == at
    k = pick(lib, 2, nbl=1, bare=0, **CLASS0)
    assert (k.nbl_off, k.del_) == (at, 1)
    k = pick(lib, 2, sq8=1, nbl=1, spec=1, **CLASS0)   # a slot over codes is one wavefront: no areas
    assert (k.nbl_off, k.spec_off, k.lds_bytes) == (0, 0, 9216 + 65536)
    # past 150 KB the optional area is dropped and the kernel still serves
    k = pick(lib, 2, nbl=1, **{**CLASS0, "lds_cand_cap": 9000})
    assert (k.served, k.nbl_off, k.lds_bytes) == (1, 141632, 149824)
    k = pick(lib, 2, nbl=1, **{**CLASS0, "lds_cand_cap": 10000})
    assert (k.served, k.nbl_off, k.lds_bytes) == (1, 0, 149632)
