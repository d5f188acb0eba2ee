"""-m gpu: WHICH ROUTE an ft_fast call takes.  The results of every path are pinned bit for bit elsewhere (tests/test_gpu_ft_*.py); a call that
took another route — a batch run query by query, a sharded merge that skipped an exchange, a packed upload whose pool was carved otherwise —
would leave all of them equal.  So this file reads the library's own counters around small calls: rxgpu_ft_read_batch_stats (launch trains and
the merges they carried), rxgpu_ft_read_train_stats (merges by train), rxgpu_ft_shard_collectives (exchanges between the shards) and
rxgpu_ft_read_packed_stats (stream bytes read, pool bytes carved).  Fixtures: those of test_gpu_ft_batch.py::test_batch_with_phrases_inside."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from oracle.pyoracle import FtOracle
from .ft_pack import pack_postings
from .test_bm25_oracle import _multi_case, make_pos_postings

pytestmark = pytest.mark.gpu

NF, TOTAL, LIMIT = 2, 3000, 20000
PLAN_LIB = Path(__file__).resolve().parent / "cpp" / "libft_packed_plan_cpu.so"


@pytest.fixture(scope="module")
def hostapi(rxgpu):
    from reindexer_amd import hostapi as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def case(oracle):
    """The index (3 OR terms of 1..3 words with 400..1500 postings each over 3000 documents) and the five queries of the batch."""
    _, words, avg, removed, _, terms, store = _multi_case(103, NF, TOTAL, LIMIT, (1, 1, 1), False, None, sizes=(400, 1500), nsub_range=(1, 4))
    plain = [dict(op=t["op"], opts=t["opts"], subs=[(s["word"], s["proc"]) for s in t["subs"]]) for t in terms]
    phrase = [dict(plain[0]), dict(plain[1], phrase=0, distance=1), dict(plain[2], phrase=0, distance=10)]
    return dict(words=words, avg=avg, removed=removed, terms=terms, store=store, plain=plain,
                queries=[phrase, plain[:1], plain[:2], phrase, plain[1:]], ft=FtOracle(oracle))


def _merger(hostapi, case, devices=None):
    m = hostapi.GpuFtMerger(NF, devices=devices)
    m.set_docs(case["words"], case["avg"], case["removed"])   # first: the cut of a sharded index follows the documents
    for s in case["store"]:
        m.set_word_fpos(s["word"], s)
    return m


def _batch_stats(rxgpu, m):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert rxgpu.lib().rxgpu_ft_read_batch_stats(m.device_index, C.byref(a), C.byref(b)) == 0
    return np.array([a.value, b.value], np.int64)


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
            and np.array_equal(a[3], b[3]) and a[4] == b[4])


def test_batch_with_phrases_takes_one_train_for_its_plain_queries(rxgpu, hostapi, case):
    """[phrase, plain, plain, phrase, plain]: the phrases run one by one, the three plain queries share ONE train; Empty() queries carry no merge."""
    m = _merger(hostapi, case)
    cfg = case["ft"].default_config(NF, merge_limit=LIMIT, min_rank=5)
    queries = case["queries"]
    s0 = _batch_stats(rxgpu, m)
    m.read_train_stats()
    batch = m.merge_query_batch(cfg, queries, sort_by_rank=False)
    assert [len(b[0]) > 0 for b in batch] == [True] * 5
    assert (_batch_stats(rxgpu, m) - s0).tolist() == [1, 3]
    assert sum(m.read_train_stats()) == 5
    lone_not = [dict(case["plain"][0], op=3)]
    s0 = _batch_stats(rxgpu, m)
    more = m.merge_query_batch(cfg, queries[:2] + [[]] + queries[2:4] + [lone_not] + queries[4:], sort_by_rank=False)
    assert [len(b[0]) > 0 for b in more] == [True, True, False, True, True, False, True]
    assert (_batch_stats(rxgpu, m) - s0).tolist() == [1, 3]
    m.close()


def test_batch_longer_than_one_train_is_cut_at_64(rxgpu, hostapi, case):
    m = _merger(hostapi, case)
    cfg = case["ft"].default_config(NF, merge_limit=LIMIT, min_rank=5)
    plain = case["plain"]
    shapes = [plain[:1], plain[1:2], plain[2:], plain[:2], plain[1:], plain, [plain[0], plain[2]]]
    queries = [shapes[i % len(shapes)] for i in range(70)]
    for i, q in enumerate(queries):
        assert len(m.merge_query(cfg, q, None, sort_by_rank=False)[0]) > 0, i
    s0 = _batch_stats(rxgpu, m)
    batch = m.merge_query_batch(cfg, queries, sort_by_rank=False)
    assert len(batch) == 70 and all(len(b[0]) > 0 for b in batch)
    assert (_batch_stats(rxgpu, m) - s0).tolist() == [2, 70]   # kFtBatchMax = 64: trains of 64 and 6
    m.close()


def test_sharded_merger_runs_a_batch_merge_by_merge_and_exchanges_per_merge(rxgpu, hostapi, case, monkeypatch):
    """Two shards on one device.  A batch never enters the batch train (every shard's handle runs one train and its exchanges at a time); the
    shards' launch trains are not the handle's (its train counters stay where they are).  One exchange per merge for the tables of first-met
    documents, one more for the pre-score histograms when the host half of the 2-phase gate held (FtMergePlan::prescore, ft_merge_plan.h)."""
    monkeypatch.delenv("RXGPU_SHARD_MERGE", raising=False)   # (=host would send the pieces through the host: no collective is counted)
    one = _merger(hostapi, case)
    many = _merger(hostapi, case, devices=[0, 0])
    assert rxgpu.lib().rxgpu_ft_shard_count(many.device_index) == 2
    cfg = case["ft"].default_config(NF, merge_limit=LIMIT, min_rank=5)
    s0 = _batch_stats(rxgpu, many)
    many.read_train_stats()
    got = many.merge_query_batch(cfg, case["queries"], sort_by_rank=False)
    want = one.merge_query_batch(cfg, case["queries"], sort_by_rank=False)
    assert (_batch_stats(rxgpu, many) - s0).tolist() == [0, 0]
    assert many.read_train_stats() == (0, 0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert len(a[0]) > 0 and _same(a, b), i

    def collectives():
        return int(rxgpu.lib().rxgpu_ft_shard_collectives(many.device_index))

    query = case["plain"]
    total_or_vids = sum(len(s["doc"]) for t in case["terms"] for s in t["subs"])
    # mergeLimit above totalORVids: min(est_or, est_and, N) > mergeLimit cannot hold — prescore == 0, the adder tables alone travel
    c0 = collectives()
    r = many.merge_query(case["ft"].default_config(NF, merge_limit=total_or_vids + 1, min_rank=5), query, None, sort_by_rank=False)
    assert len(r[0]) > 0 and not r[4]
    assert collectives() - c0 == 1
    # mergeLimit below every OR term's postings (>= 400) and below N = 3000: prescore == 1, the histograms travel too
    c0 = collectives()
    r = many.merge_query(case["ft"].default_config(NF, merge_limit=300, min_rank=5), query, None, sort_by_rank=False)
    assert len(r[0]) > 0 and r[4]
    assert collectives() - c0 == 2
    one.close()
    many.close()


def _plan_pool_bytes(counts):
    """The pool of a packed upload as csrc/ft_packed_plan.h lays it out (compiled for the host: tests/cpp/ft_packed_plan_cpu.cc)."""
    if not PLAN_LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(PLAN_LIB))
    L.ft_packed_pool_cpu.restype = C.c_uint64
    L.ft_packed_pool_cpu.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(counts, np.uint32).reshape(-1, 4)
    return int(L.ft_packed_pool_cpu(c.shape[0], c.ctypes.data, None, None))


def test_packed_upload_reads_every_stream_once_and_carves_the_planned_pool(hostapi):
    """~50 words, among them an empty stream, one of exactly kFtPackedSegBytes = 1024 bytes (one piece, full) and one longer (two pieces).  The
    pool bytes the device path reports equal the CPU plan's layout over the counts the DEVICE decoded (read back with rxgpu_ft_get_word)."""
    rng = np.random.default_rng(9)
    one_pos = lambda n: dict(doc=np.arange(1, n + 1, dtype=np.uint32), pos_off=np.arange(n + 1, dtype=np.uint32), fpos=np.ones(n, np.uint64))
    words = [(0, np.zeros(0, np.uint8), 0)]
    words.append((1,) + pack_postings(**one_pos(512)))   # 2 bytes per posting (id delta 1, head of position 1)
    words.append((2,) + pack_postings(**one_pos(700)))
    assert len(words[1][1]) == 1024 and len(words[2][1]) > 1024
    for wid in range(3, 50):
        s = make_pos_postings(rng, int(rng.choice([4000, 70_000])), NF, int(rng.choice([1, 2, 7, 64, 300])), 1.0, array_fields=bool(wid % 3 == 0))
        words.append((wid,) + pack_postings(s["doc"], s["pos_off"], s["fpos"]))
    m = hostapi.GpuFtMerger(NF)
    m.set_docs(np.ones((70_001, NF), np.float32), np.ones(NF, np.float32), np.zeros(70_001, np.uint8))
    m.read_packed_stats()
    m.set_words_packed(words)
    stats = m.read_packed_stats()
    assert stats[2] == sum(len(w[1]) for w in words)
    counts = []
    for wid, _, _ in words:
        g = m.get_word(wid)
        n = len(g["doc"])
        counts.append((n, len(g["fpos"]), len(g["ent_field"]), int(g["doc"][-1]) if n else 0))
    assert counts[0][0] == 0 and counts[1][0] == 512 and counts[2][0] == 700
    assert stats[3] == _plan_pool_bytes(counts)
    m.close()
