"""-m gpu: every HNSW kernel over level-0 lists of 63 to 128 links.  A list is 1 + maxM0 words and a wavefront reads 64 words a pass, so
every kernel loops over a list in passes of 64; a second pass runs only on a list of 64 links or more, a third only on one of exactly 128,
and no built graph of a test's size holds such lists.  The graphs here are constructed (tests/hnsw_long_list_cases.py: every list of a
graph has the one length c its class names; tests/test_hnsw_long_list_cases.py proves on the CPU what the cases rely on).

Bar: the one of tests/test_gpu_row_layout.py — on the same flat graph the device returns exactly the labels and the distance bits of the
restated engine (oracle_hnsw_search_knn, OracleHnswStream, oracle_hnsw_search_knn_sq8), over an owned index and over adopted rows at a
padded stride whose pads are NaN.  No expectation is taken from the code under test.  Lists are in ascending order of distance; the
"nearest_last" cases rotate them by one, so that the one word of a last pass is the link a search needs most.  The launched searches are
held to the engine's hops and distance evaluations as well: these graphs are dense enough for a skipped link to be reached through
another list with the same answer in the end: answers alone can miss a dropped last word.

test                                     kernel family                                               list classes (M, c)
launched, d = 128 / 768                  fixed-dimension sorted-list search: team (nq = 1), batch     all seven
launched, inner product                  the same, metric 1                                           (64, 128)
launched, d = 100 / 1024 / 1536          generic batch; wide-chunk fixed kernels                      (64, 128), (32, 64)
heaps only / global candidate heap       the heap search, candidate heap in LDS / in global scratch   (64, 128), (32, 64) at d = 768
300 deleted                              the deleting sorted list (ef <= 224), the heaps above        (64, 128), (32, 64) at d = 768
team gates (NBL = 1, SPEC = 1)           team search whose link-block / look-ahead areas must stay off (64, 128), (32, 64) at d = 768
mailbox                                  resident search kernels, both ef classes                     (64, 64), (64, 65), (64, 128)
streaming                                hnsw_stream, LDS and global heaps                            (64, 64), (64, 65), (64, 128)
streaming, 6000 rows                     hnsw_stream leaving the LDS staging in the middle of a call   (64, 64), (64, 65), (64, 128)
range                                    hnsw_range_kernel: ef-search + closure                       (64, 64), (64, 128)
SQ8                                      search over codes, launched and resident                     (64, 64), (64, 128)
"""
import ctypes as C

import numpy as np
import pytest

from . import hnsw_long_list_cases as cases
from .conftest import make_corpus
from .test_gpu_row_layout import _check_hnsw, _hnsw_layouts, bits

pytestmark = pytest.mark.gpu
LAYOUTS = ("owned", "padded20")
ERR_OVERFLOW = -8
_cache = {}


def _shape(oracle, shape):
    """(graph, rows, inv_norms, 12 queries) of a case"""
    metric, M, d, c, deleted = shape[:5]
    return cases.full_graph(*shape), cases.rows_of(d), cases.inv_norms_of(oracle, metric, d), cases.queries_of(oracle, metric, d)


def _wants(oracle, shape, k, ef):
    metric, M, d, c, deleted = shape[:5]
    return [(wd, wl) for wd, wl, _, _ in cases.wants_of(oracle, metric, M, d, c, k, ef, deleted, *shape[5:])]


def _stats(oracle, shape, k, ef):
    """(distance evaluations, hops) of the restated engine over the 12 queries of a plan"""
    metric, M, d, c, deleted = shape[:5]
    w = cases.wants_of(oracle, metric, M, d, c, k, ef, deleted, *shape[5:])
    return sum(nd for _, _, nd, _ in w), sum(nh for _, _, _, nh in w)


def _counters(ix):
    """(distance evaluations, hops) the search kernels counted since the last call; None where a search started over on the heaps or was
    run again (such a search is counted more than once)"""
    evals, hops, restarts, _ = ix.hnsw_read_stats4()
    reruns = ix.hnsw_read_tie_reruns() + ix.hnsw_read_lds_reruns()
    return None if restarts or reruns else (evals, hops)


def _launched(rxgpu, oracle, monkeypatch, shape, what, **env):
    """12 single queries, then one call of 300, under every plan and layout, on the launch path.  Besides the answers, the traversal: a
    search pops as many nodes and evaluates as many distances as the restated engine (every node at most once, the entry point twice), so
    a link that is skipped and reached through another list later still shows, in the hops."""
    g, rows, inv, q = _shape(oracle, shape)
    monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    batch = np.tile(q, (25, 1))
    compared = {name: 0 for name in LAYOUTS}
    with _hnsw_layouts(rxgpu, shape[0], g, rows, inv, LAYOUTS) as ixs:
        for k, ef in cases.PLANS:
            wants = _wants(oracle, shape, k, ef)
            evals, hops = _stats(oracle, shape, k, ef)
            for name, ix in ixs.items():
                _counters(ix)
                for i in range(12):
                    _check_hnsw(g, ix.hnsw_search_knn(q[i][None, :], k, ef), wants[i:i + 1], (what, "nq = 1", name) + shape + (k, ef, i))
                single = _counters(ix)
                _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 25, (what, "nq = 300", name) + shape + (k, ef))
                many = _counters(ix)
                print(what, name, cases.case_id(shape), "k", k, "ef", ef, "evaluations, hops: engine", (evals, hops), "nq = 1", single, "nq = 300 / 25",
                      many and (many[0] / 25, many[1] / 25))
                if "RXGPU_HNSW_LDS_CAND_CAP" in env:   # every search outgrows its heap area and runs again on the tiers behind it: counted twice
                    continue
                assert single is None or single == (evals, hops), (what, "nq = 1", name) + shape + (k, ef, single, (evals, hops))
                assert many is None or many == (25 * evals, 25 * hops), (what, "nq = 300", name) + shape + (k, ef, many, (25 * evals, 25 * hops))
                compared[name] += int(single is not None) + int(many is not None)
    if "RXGPU_HNSW_LDS_CAND_CAP" not in env:   # the traversal was compared under at least one plan on every index: the check is not empty
        assert all(compared.values()), (what,) + shape + (compared,)


# ---------------------------------------------------------------------------------------------------------------- launched searches
@pytest.mark.parametrize("shape", cases.LAUNCHED + cases.INNER_PRODUCT + cases.LAUNCHED_NEAREST_LAST, ids=cases.case_id)
def test_fixed_dimension_kernels_over_every_list_class(rxgpu, oracle, monkeypatch, pick_lib, shape):
    """nq = 1 is the team form, nq = 300 the batch form of the sorted-list search: the pick for these launches says so"""
    from . import test_hnsw_kernel_pick as kp
    metric, M, d, c, deleted = shape[:5]
    for k, ef in cases.PLANS:
        one = kp.pick(pick_lib, 0, dim=d, ef=ef, ef_cap=max(ef, 128), bare=1, maxM0=2 * M, blocks=1)
        many = kp.pick(pick_lib, 0, dim=d, ef=ef, ef_cap=max(ef, 128), bare=1, maxM0=2 * M, blocks=300)
        assert (one.family, one.team, one.nb, many.family, many.team, many.nb) == (kp.TEAM, 4, d // 64, kp.SEARCH, 1, d // 64), shape + (k, ef)
        assert one.sorted and many.sorted, shape + (k, ef)
    _launched(rxgpu, oracle, monkeypatch, shape, "fixed")


@pytest.mark.parametrize("shape", cases.OTHER_DIMS, ids=cases.case_id)
def test_generic_and_wide_chunk_kernels_over_full_lists(rxgpu, oracle, monkeypatch, shape):
    _launched(rxgpu, oracle, monkeypatch, shape, "generic / wide")


@pytest.mark.parametrize("shape", cases.AT_768 + cases.AT_768_NEAREST_LAST, ids=cases.case_id)
def test_heap_search_over_full_lists(rxgpu, oracle, monkeypatch, shape):
    _launched(rxgpu, oracle, monkeypatch, shape, "heaps only", RXGPU_HNSW_SORTED=0)


@pytest.mark.parametrize("shape", cases.AT_768, ids=cases.case_id)
def test_global_candidate_heap_over_full_lists(rxgpu, oracle, monkeypatch, shape):
    _launched(rxgpu, oracle, monkeypatch, shape, "global candidate heap", RXGPU_HNSW_LDS_CAND_CAP=4)


@pytest.mark.parametrize("form", ["sorted", "heaps_only", "global_candidate_heap"])
@pytest.mark.parametrize("shape", cases.AT_768_DELETED, ids=cases.case_id)
def test_deleted_nodes_over_full_lists(rxgpu, oracle, monkeypatch, shape, form):
    env = {"sorted": {}, "heaps_only": {"RXGPU_HNSW_SORTED": 0}, "global_candidate_heap": {"RXGPU_HNSW_LDS_CAND_CAP": 4}}[form]
    _launched(rxgpu, oracle, monkeypatch, shape, "300 deleted, " + form, **env)


# ---------------------------------------------------------------------------------------------------------------- the team's gates
@pytest.fixture(scope="module")
def pick_lib():
    from . import test_hnsw_kernel_pick as kp
    if not kp.LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(kp.LIB))
    L.hnsw_pick_cpu.restype = None
    L.hnsw_pick_cpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("switch", ["RXGPU_HNSW_NBL", "RXGPU_HNSW_SPEC"])
@pytest.mark.parametrize("shape", cases.AT_768, ids=cases.case_id)
def test_team_areas_stay_off_at_long_lists(rxgpu, oracle, monkeypatch, pick_lib, shape, switch):
    """The link-block area and the look-ahead area of a team hold 64 words a list: from maxM0 = 64 on the pick gives neither, whatever
    the switches ask for, and the answers are those of the plain team search."""
    from . import test_hnsw_kernel_pick as kp
    metric, M, d, c, deleted = shape[:5]
    for k, ef in cases.PLANS:
        for bare in (1, 0):
            got = kp.pick(pick_lib, 0, dim=d, ef=ef, ef_cap=max(ef, 128), bare=bare, maxM0=2 * M, blocks=1,
                          nbl=int(switch.endswith("NBL")), spec=int(switch.endswith("SPEC")))
            assert (got.nbl_off, got.spec_off) == (0, 0) and got.exists and got.served, (shape, k, ef, bare, got.family, got.nbl_off, got.spec_off)
            if bare:   # (with delete marks the sorted list, and with it the team, ends at ef = 224)
                assert got.family == kp.TEAM, (shape, k, ef, got.family)
    _launched(rxgpu, oracle, monkeypatch, shape, switch, **{switch: 1})


# ---------------------------------------------------------------------------------------------------------------- the mailbox
@pytest.mark.parametrize("shape", cases.MAILBOX + cases.MAILBOX_NEAREST_LAST, ids=cases.case_id)
def test_posted_search_over_long_lists(rxgpu, oracle, monkeypatch, shape):
    """a served call is checked against the engine; a declined or flagged one is answered by rxgpu_hnsw_search_knn, the caller's next step,
    and checked the same way.  ef above 256 (224 on a graph with deleted nodes) is declined by the mailbox's documented limits."""
    g, rows, inv, q = _shape(oracle, shape)
    limit = 224 if shape[4] else 256
    monkeypatch.delenv("RXGPU_HNSW_SERVER", raising=False)
    with _hnsw_layouts(rxgpu, shape[0], g, rows, inv, LAYOUTS) as ixs:
        for name, ix in ixs.items():
            served = asked = 0
            for k, ef in cases.PLANS:
                wants = _wants(oracle, shape, k, ef)
                for i in range(12):
                    pd, pr, pc, ok = ix.hnsw_search_knn_posted(q[i], k, ef)
                    if ef > limit:
                        assert not ok, (name,) + shape + (k, ef, i)
                    else:
                        asked += 1
                    if ok:
                        served += 1
                        got = (pd[None, :], pr[None, :], np.array([pc]))
                    else:
                        got = ix.hnsw_search_knn(q[i][None, :], k, ef)
                    _check_hnsw(g, got, wants[i:i + 1], ("posted", ok, name) + shape + (k, ef, i))
            print(f"mailbox {cases.case_id(shape)} {name}: served {served} of {asked} calls within the limits ({served / asked:.3f})")
            assert served >= 1, (name,) + shape


# ---------------------------------------------------------------------------------------------------------------- streaming
STREAM_PLANS = [(0, [10] * 6), (16, [5, 40, 1, 300, 7]), (64, [64] * 12), (3, [1] * 20 + [5000]), (100, [1000, 1000, 1000, 1000]),   # tests/test_gpu_hnsw.py
                (64, [64] * 60), (200, [1000] * 7)]   # ... and its deep sessions: every node is evaluated on the way


class _Stream:
    """rxgpu_hnsw_stream_begin / _continue / _end on a device index"""

    def __init__(self, rxgpu, ix, q, ef):
        self.rxgpu, self.L, self.n = rxgpu, rxgpu.lib(), int(ix.count)
        self.q = np.ascontiguousarray(q, np.float32)
        self.s = C.c_void_p()
        rxgpu._check(self.L.rxgpu_hnsw_stream_begin(ix._h, self.q.ctypes.data, ef, C.byref(self.s)))

    def next(self, batch):
        cap = max(1, min(batch, self.n))
        od, orow = np.empty(cap, np.float32), np.empty(cap, np.uint32)
        cnt, ex = C.c_uint32(0), C.c_int(0)
        self.rxgpu._check(self.L.rxgpu_hnsw_stream_continue(self.s, batch, od.ctypes.data, orow.ctypes.data, C.byref(cnt), C.byref(ex)))
        return od[:cnt.value].copy(), orow[:cnt.value].copy(), bool(ex.value)

    def close(self):
        if self.s:
            self.L.rxgpu_hnsw_stream_end(self.s)
            self.s = C.c_void_p()


def _sorted_pairs(dist, labels):
    order = np.lexsort((labels, dist))
    return bits(dist[order]), labels[order]


def _same_batch(g, got, want, what):
    """one Continue: the same (dist, label) pairs, `exhausted` alike"""
    (gd, gr, gex), (wd, wl, wex) = got, want
    assert gex == wex and len(gd) == len(wd), what + (len(gd), len(wd), gex, wex)
    a, w = _sorted_pairs(gd, g["labels"][gr]), _sorted_pairs(wd, wl)
    assert np.array_equal(a[1], w[1]), what + ("labels",)
    assert np.array_equal(a[0], w[0]), what + ("distance bits",)


@pytest.mark.parametrize("heaps", ["lds", "global"])
@pytest.mark.parametrize("shape", cases.STREAMING + cases.STREAMING_NEAREST_LAST, ids=cases.case_id)
def test_streaming_sessions_over_long_lists(rxgpu, oracle, monkeypatch, shape, heaps):
    """Whole sessions against OracleHnswStream batch for batch; "global": every call on the HBM-resident heaps (RXGPU_HNSW_STREAM_GLOBAL).
    The profile slots tell which kernel ran: a call with a batch above 1024 entries starts on the global heaps, and a call in which both
    slots count left the LDS staging on the way (kStreamNeedGlobal).  Over 3000 rows no call does: the candidate set would have to pass
    3072 - maxM0 = 2944 entries, and the restated engine's peaks near 2300 (tests/hnsw_long_list_cases.py); the 6000-row graphs of
    test_streaming_call_leaves_the_lds_staging are there for that.
    The sessions of an index end after its profile was read for the last time: the profile's events are recorded on a session's own stream,
    which rxgpu_hnsw_stream_end destroys, and rxgpu_profile_read waits on every event of a slot."""
    from oracle.pyoracle import OracleHnswStream
    metric, M, d, c, deleted = shape[:5]
    g, rows, inv, _ = _shape(oracle, shape)
    if heaps == "global":
        monkeypatch.setenv("RXGPU_HNSW_STREAM_GLOBAL", "1")
    else:
        monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, LAYOUTS) as ixs:
        for name, ix in ixs.items():
            ix.profile_enable(True)
            handovers = in_lds = in_global = 0
            before = (0, 0)
            sessions = []
            for qi, (ef, batches) in enumerate(STREAM_PLANS):
                q = make_corpus(900 + qi, 1, d)[0]
                if metric == 2:
                    q, _ = oracle.normalize_copy(q)
                gs, ws = _Stream(rxgpu, ix, q, ef), OracleHnswStream(oracle, g, q, ef, inv)
                sessions.append(gs)
                for step, b in enumerate(batches):
                    got = gs.next(b)
                    after = (ix.profile_read("hnsw_stream")[0], ix.profile_read("hnsw_stream_global")[0])
                    _same_batch(g, got, ws.next(b), (name,) + shape + (qi, step, b))
                    in_lds += after[0] - before[0]
                    in_global += after[1] - before[1]
                    handovers += int(after[0] > before[0] and after[1] > before[1])
                    before = after
                ws.close()
            ix.profile_enable(False)
            for gs in sessions:
                gs.close()
            print(f"streaming {cases.case_id(shape)} {name} {heaps}: {in_lds} launches on LDS heaps, {in_global} on global heaps, {handovers} calls handed over")
            if heaps == "global":
                assert in_lds == 0 and in_global >= 1, (name,) + shape
            else:
                assert in_lds >= 1 and in_global >= 1, (name,) + shape   # batch 5000 > 1024 entries: that call cannot stage its heaps in LDS


@pytest.mark.parametrize("shape", cases.HANDOVER, ids=lambda s: "metric%d-M%d-d%d-c%d" % s)
def test_streaming_call_leaves_the_lds_staging(rxgpu, oracle, monkeypatch, shape):
    """The deep session over 6000 rows: its candidate set passes 3072 - maxM0 entries in the middle of a call (the restated engine says in
    which: tests/test_hnsw_long_list_cases.py proves there is one), so that call stops at a step boundary with kStreamNeedGlobal and is
    resumed on the global heaps, and the calls behind it start there.  Per call: the kernels that ran, and the batch."""
    metric, M, d, c = shape
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.full_graph(metric, M, d, c, n=cases.HANDOVER_N)
    rows = g["vectors"]
    inv = oracle.l2_modules(rows) if metric == 2 else None
    calls = cases.handover_calls(oracle, metric, M, d, c)
    assert sum(handed for _, _, _, _, handed, _ in calls) >= 1
    ef, batches = cases.HANDOVER_PLAN
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, LAYOUTS) as ixs:
        for name, ix in ixs.items():
            ix.profile_enable(True)
            gs = _Stream(rxgpu, ix, cases.handover_query(oracle, metric, d), ef)
            before, handovers = (0, 0), 0
            for step, (b, (wd, wl, wex, in_lds, handed, sizes)) in enumerate(zip(batches, calls)):
                got = gs.next(b)
                after = (ix.profile_read("hnsw_stream")[0], ix.profile_read("hnsw_stream_global")[0])
                ran = (after[0] - before[0], after[1] - before[1])
                assert ran == ((1, 1) if handed else (1, 0) if in_lds else (0, 1)), (name,) + shape + (step, ran, in_lds, handed, sizes)
                _same_batch(g, got, (wd, wl, wex), (name,) + shape + (step, b))
                handovers += int(ran == (1, 1))
                before = after
            ix.profile_enable(False)
            gs.close()
            print(f"streaming {name} {shape}: {handovers} calls handed over, {before[0]} launches on LDS heaps, {before[1]} on global heaps")
            assert handovers >= 1, (name,) + shape


# ---------------------------------------------------------------------------------------------------------------- range search
def _range_call(rxgpu, ix, q, radius, ef, cap):
    od, orow = np.empty(cap, np.float32), np.empty(cap, np.uint32)
    total = C.c_uint64(0)
    rc = rxgpu.lib().rxgpu_hnsw_search_range(ix._h, q.ctypes.data, C.c_float(radius), ef, od.ctypes.data, orow.ctypes.data, cap, C.byref(total))
    return rc, od, orow, int(total.value)


def _want_range(oracle, g, q, inv, all_d, radius, ef):
    """SearchRange restated: the engine's ef results with dist < radius, closed under level-0 links through nodes with dist < radius"""
    from oracle.pyoracle import oracle_hnsw_search_knn
    _, labels = oracle_hnsw_search_knn(oracle, g, q, ef, ef, inv)
    seeds = (labels >> np.uint64(32)).astype(np.int64)
    inside = all_d < np.float32(radius)
    found = set(int(r) for r in seeds if inside[r])
    todo = sorted(found)
    links0 = g["links0"]
    while todo:
        node = todo.pop()
        for nb in links0[node, 1:1 + int(links0[node, 0])]:
            nb = int(nb)
            if inside[nb] and nb not in found:
                found.add(nb)
                todo.append(nb)
    return found, len(seeds)


@pytest.mark.parametrize("shape", cases.RANGE + cases.RANGE_NEAREST_LAST, ids=cases.case_id)
def test_range_search_over_long_lists(rxgpu, oracle, shape):
    metric, M, d, c, deleted = shape[:5]
    g, rows, inv, q = _shape(oracle, shape)
    ef = 64
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, LAYOUTS) as ixs:
        for i in range(12):
            all_d = oracle.dist_many(metric, q[i], rows, inv)
            radius = float(np.sort(all_d)[39])   # the 40th smallest exact distance: 39 rows lie inside
            want, seeds = _want_range(oracle, g, q[i], inv, all_d, radius, ef)
            assert seeds == ef and 1 <= len(want) <= 39, shape + (i, seeds, len(want))
            for name, ix in ixs.items():
                what = (name,) + shape + (i,)
                rc, od, orow, total = _range_call(rxgpu, ix, q[i], radius, ef, 64)   # (at most 39 hits: room enough)
                assert rc == 0, what + (rc,)
                got = orow[:total]
                assert total == len(want) and set(int(r) for r in got) == want, what + (total, len(want))
                assert np.array_equal(bits(od[:total]), bits(all_d[got])), what + ("distance bits",)
                if len(want) > 8:   # the overflow answer: not enough room, every hit counted all the same, then the retry with room
                    rc, _, _, seen = _range_call(rxgpu, ix, q[i], radius, ef, 8)
                    assert rc == ERR_OVERFLOW and seen == len(want), what + (rc, seen, len(want))
                    rc, od, orow, total = _range_call(rxgpu, ix, q[i], radius, ef, 64)
                    assert rc == 0 and set(int(r) for r in orow[:total]) == want, what + ("after the overflow",)


# ---------------------------------------------------------------------------------------------------------------- SQ8
def _sq8_case(oracle, metric, d):
    """(sq dict, float queries, norms, query codes, corrective offsets, normCoefs) of a shape's rows and queries, computed once"""
    key = ("sq8", metric, d)
    if key not in _cache:
        from oracle.pyoracle import Sq8Oracle
        from .test_gpu_hnsw_server_sq8 import quantise_queries, quantise_rows
        min_q, max_q, sq = quantise_rows(Sq8Oracle(oracle), metric, cases.rows_of(d))
        _cache[key] = (sq,) + quantise_queries(oracle, metric, min_q, max_q, make_corpus(700 + d, 12, d))
    return _cache[key]


@pytest.mark.parametrize("shape", cases.SQ8, ids=cases.case_id)
def test_sq8_search_over_long_lists(rxgpu, oracle, monkeypatch, shape):
    """over codes: 12 single queries and one call of 300 on the launch path, then the 12 through the mailbox"""
    from oracle.pyoracle import oracle_hnsw_search_knn_sq8
    metric, M, d, c, deleted = shape[:5]
    g, rows, inv, _ = _shape(oracle, shape)
    sq, qs, norms, qc, qo, qn = _sq8_case(oracle, metric, d)
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, LAYOUTS) as ixs:
        for ix in ixs.values():
            ix.hnsw_attach_sq8(sq["codes"], sq["corr"], float(sq["alpha_2"]))
        served_by = {name: 0 for name in ixs}
        for k, ef in cases.PLANS:
            wants = [oracle_hnsw_search_knn_sq8(oracle, g, sq, qs[i], k, ef, inv, norms[i]) for i in range(12)]
            for name, ix in ixs.items():
                what = (name,) + shape + (k, ef)
                monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")
                for i in range(12):
                    _check_hnsw(g, ix.hnsw_search_knn_sq8(qc[i][None, :], qo[i:i + 1], qn[i:i + 1], k, ef), wants[i:i + 1], ("sq8, nq = 1",) + what + (i,))
                _check_hnsw(g, ix.hnsw_search_knn_sq8(np.tile(qc, (25, 1)), np.tile(qo, 25), np.tile(qn, 25), k, ef), wants * 25, ("sq8, nq = 300",) + what)
                monkeypatch.delenv("RXGPU_HNSW_SERVER")
                served = 0
                for i in range(12):
                    pd, pr, pc, ok = ix.hnsw_search_knn_sq8_posted(qc[i], qo[i], qn[i], k, ef)
                    served += int(ok)
                    got = (pd[None, :], pr[None, :], np.array([pc])) if ok else ix.hnsw_search_knn_sq8(qc[i][None, :], qo[i:i + 1], qn[i:i + 1], k, ef)
                    _check_hnsw(g, got, wants[i:i + 1], ("sq8, posted", ok) + what + (i,))
                print(f"sq8 mailbox {cases.case_id(shape)} {name} k={k} ef={ef}: {served} of 12 calls answered by the posted call")
                served_by[name] += served
        assert all(n >= 1 for n in served_by.values()), shape + (served_by,)   # (otherwise the posted half is the launched half once more)
