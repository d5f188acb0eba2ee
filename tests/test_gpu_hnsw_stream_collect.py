"""-m gpu: a streaming HNSW session collected under an allowed-rows bitmap in one device call — rxgpu_hnsw_stream_collect
(hnsw_stream_collect.hip), the one-shot rxgpu_hnsw_collect_knn / _sq8 on a leased search context, GpuHnswMap::CollectStreaming / SearchKnnStreamed and their Python bindings.

Every comparison is exact.  A collection is compared with (1) the rule of csrc/hnsw_stream_collect_plan.h restated in Python
(tests/hnsw_stream_collect_cases.py: run_rule) over the product's own rxgpu_hnsw_stream_continue on a second session — rows and distance bits
in delivery order, per-call (batch, emitted, accepted), calls, presented, exhausted — and (2) the same rule over the restated engine
(OracleHnswStream), which does not run the product's stream kernel: per call the accepted (distance bits, label) pairs as sorted pairs (the
engine's order inside a batch is the heap's, the rule does not read it) and the same counters.  tests/test_hnsw_stream_collect_cases.py shows
on the CPU on which side of the LDS limits each case lies."""
import threading

import numpy as np
import pytest

from . import hnsw_stream_collect_cases as cases
from .test_gpu_hnsw import bits

pytestmark = pytest.mark.gpu


class _Index:
    """a device index with the case's graph attached"""

    def __init__(self, rxgpu, oracle, g):
        self.g = g
        self.inv = oracle.l2_modules(g["vectors"]) if g["metric"] == 2 else None
        self.ix = rxgpu.VectorIndex(g["metric"], g["dim"], g["n"])
        self.ix.upload_rows(0, g["vectors"], self.inv)
        self.ix.hnsw_attach_graph(g)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ix.close()


def _flat(per_call):
    d = np.concatenate([np.asarray(x[0], np.float32) for x in per_call]) if per_call else np.zeros(0, np.float32)
    r = np.concatenate([np.asarray(x[1]) for x in per_call]) if per_call else np.zeros(0, np.uint32)
    return d, r


def _sorted_pairs(dist, labels):
    order = np.lexsort((labels, dist))
    return bits(np.asarray(dist, np.float32)[order]), np.asarray(labels)[order]


def check_against_rule(got, want, tag):
    """the product's own Continue under the Python rule: delivery order and all"""
    assert [tuple(int(x) for x in c) for c in got["calls"]] == want["calls"], tag + (got["calls"].tolist(), want["calls"])
    assert (got["presented"], got["accepted"], got["exhausted"]) == (want["presented"], want["accepted"], want["exhausted"]), tag
    wd, wr = _flat(want["per_call"])
    assert np.array_equal(got["row"], wr), tag + ("rows",)
    assert np.array_equal(bits(got["dist"]), bits(wd)), tag + ("distance bits",)


def check_against_oracle(got, want, labels, tag):
    assert [tuple(int(x) for x in c) for c in got["calls"]] == want["calls"], tag + (got["calls"].tolist(), want["calls"])
    assert (got["presented"], got["accepted"], got["exhausted"]) == (want["presented"], want["accepted"], want["exhausted"]), tag
    at = 0
    for c, (wd, wl) in enumerate(want["per_call"]):
        end = int(got["calls"][c][2])
        a, w = _sorted_pairs(got["dist"][at:end], labels[got["row"][at:end]]), _sorted_pairs(wd, wl)
        assert np.array_equal(a[1], w[1]), tag + (c, "labels")
        assert np.array_equal(a[0], w[0]), tag + (c, "distance bits")
        at = end
    assert at == got["accepted"]


def collect_three_ways(rxgpu, oracle, dev, q, allowed, needed, ef, first_batch, tag, max_calls=cases.MAX_CALLS, words=None):
    """collect on one session; the Python rule over Continue on a second; the rule over the restated engine.  Returns (got, oracle's run)."""
    g = dev.g
    with dev.ix.hnsw_stream(q, ef) as s:
        got = s.collect(cases.words_of(allowed) if words is None else words, needed, first_batch, max_calls)
    with dev.ix.hnsw_stream(q, ef) as s:
        rule = cases.run_rule(s, lambda rows: allowed[rows], needed, first_batch, max_calls)
    check_against_rule(got, rule, tag)
    # the one-shot call on a leased context: the same rows, bits, positions, records and launches as begin -> collect -> end
    one = dev.ix.hnsw_collect_knn(q, ef, cases.words_of(allowed) if words is None else words, needed, first_batch, max_calls)
    for k in ("row", "pos", "calls"):
        assert np.array_equal(one[k], got[k]), tag + ("one-shot", k)
    assert np.array_equal(bits(one["dist"]), bits(got["dist"])), tag + ("one-shot",)
    assert all(one[k] == got[k] for k in ("presented", "accepted", "exhausted", "launches")), tag + ("one-shot",)
    # a row's position in its call: the call delivers worst first, so ascending positions are descending distances
    at = 0
    for _, emitted, end in got["calls"]:
        pos = got["pos"][at:end].astype(np.int64)
        assert np.all(np.diff(pos) > 0) and (len(pos) == 0 or pos[-1] < emitted), tag + ("positions",)
        at = int(end)
    want = cases.oracle_rule(oracle, g, q, dev.inv, allowed, needed, ef, first_batch, max_calls)
    check_against_oracle(got, want, g["labels"], tag)
    return got, want


# ------------------------------------------------------------------------------------------------ A. everything stays in LDS
@pytest.mark.parametrize("deleted", [0, cases.A_DELETED])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_collect_equals_the_rule_over_continue_and_over_the_engine(rxgpu, oracle, monkeypatch, metric, deleted):
    """3000 x 48, M = 8: shares 1 .. 0 x needed 1 / 10 / 150 x ef = first_batch 100 / 16, with and without 200 deleted labels.  One launch
    each: the candidate set stays below kStreamLdsCand - maxM0 (the CPU test of the cases says so).  ef 16 parks nodes in the extras; the
    selective shares at needed 150 exhaust the session; share 0 walks the batch ladder."""
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.A, metric, deleted)
    q = cases.query(oracle, metric, g["dim"])
    most = 0
    with _Index(rxgpu, oracle, g) as dev:
        for share in cases.A_SHARES:
            allowed = cases.allowed_rows(g["n"], share)
            for needed in cases.A_NEEDED:
                for ef in cases.A_EF:
                    tag = (metric, deleted, share, needed, ef)
                    got, want = collect_three_ways(rxgpu, oracle, dev, q, allowed, needed, ef, ef, tag)
                    assert got["launches"] == 1, tag
                    most = max(most, len(want["calls"]))
                    if share == 0:
                        assert got["accepted"] == 0 and got["exhausted"], tag
    print(f"collect A metric {metric} deleted {deleted}: up to {most} calls in one launch")


# ------------------------------------------------------------------------------------------------ B. the handover
@pytest.mark.parametrize("heaps", ["lds", "global"])
@pytest.mark.parametrize("case", cases.B_CASES, ids=lambda c: "share%s-needed%d-ef%d" % c)
def test_collect_leaves_the_lds_staging(rxgpu, oracle, monkeypatch, case, heaps):
    """6000 x 32, M = 16 (maxM0 32): a collection whose candidate set passes kStreamLdsCand - maxM0 = 3040 entries stops at that step
    boundary and is resumed once on the global heaps — two launches, the same answer; one that stays below takes one.  The restated engine
    says on which side the case is.  "global": the same cases with every heap in HBM from the start (RXGPU_HNSW_STREAM_GLOBAL), one launch."""
    share, needed, ef = case
    g = cases.graph(cases.B, 0)
    q = cases.query(oracle, 0, g["dim"])
    if heaps == "global":
        monkeypatch.setenv("RXGPU_HNSW_STREAM_GLOBAL", "1")
    else:
        monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    allowed = cases.allowed_rows(g["n"], share)
    with _Index(rxgpu, oracle, g) as dev:
        got, want = collect_three_ways(rxgpu, oracle, dev, q, allowed, needed, ef, ef, case + (heaps,))
    outgrows = want["peak_cand"] > cases.STREAM_LDS_CAND - g["maxM0"] or want["peak_ext"] + 1 > cases.STREAM_LDS_TOP
    assert outgrows == (share != 1), (case, want["peak_cand"], want["peak_ext"])   # the case is on the side it is here for
    print(f"collect B {case} {heaps}: candidate_set peaks at {want['peak_cand']}, extras at {want['peak_ext']}, {got['launches']} launches")
    assert got["launches"] == (2 if outgrows and heaps == "lds" else 1), (case, heaps, got["launches"])


def test_collect_with_a_first_batch_above_the_lds_heaps(rxgpu, oracle, monkeypatch):
    """ef = first_batch = 1200 > kStreamLdsTop: global heaps from the first call, one launch, the same results"""
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.B, 0)
    q = cases.query(oracle, 0, g["dim"])
    allowed = cases.allowed_rows(g["n"], 0.1)
    with _Index(rxgpu, oracle, g) as dev:
        got, _ = collect_three_ways(rxgpu, oracle, dev, q, allowed, 150, 1200, 1200, ("ef1200",))
    assert got["launches"] == 1 and got["calls"][0][0] == 1200


# ------------------------------------------------------------------------------------------------ C. SQ8, through a quantised Map
@pytest.mark.parametrize("metric", [0, 2])
def test_collect_over_a_quantised_map(rxgpu, oracle, monkeypatch, metric):
    """2000 x 64 quantised to SQ8: the device collection against the Map's host loop (RXGPU_HNSW_COLLECT=host: the plan functions over
    ContinueStreamingSearch of the SQ8 session) and against the Python rule over the session's next().  OracleHnswStream walks float rows
    only — it takes no codes — so the engine-side check of the quantised walk stays with tests/test_gpu_sq8.py's streaming sessions."""
    from reindexer_amd import hostapi
    n, d = 2000, 64
    rows = cases.make_corpus(64, n, d)
    labels = cases.labels_of(n)
    m = hostapi.GpuHnswMap(metric, d, n, M=8, ef_construction=100)
    m.add(rows, labels)
    m.quantize(float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995)))
    q, norm = cases.make_corpus(900, 1, d)[0], None
    if metric == 2:
        q, k_ = oracle.normalize_copy(q)
        norm = float(np.float32(1.0) / np.float32(k_))
    for share in (0.5, 0.02):
        allowed = cases.allowed_rows(n, share)
        al = labels[allowed]
        al_set = set(al.tolist())
        for needed, ef in ((10, 100), (150, 16)):
            tag = (metric, share, needed, ef)
            monkeypatch.delenv("RXGPU_HNSW_COLLECT", raising=False)
            s = m.stream(q, ef, norm=norm)
            got = s.collect(al, needed, ef)
            s.close()
            assert got["launches"] >= 1, tag
            monkeypatch.setenv("RXGPU_HNSW_COLLECT", "host")
            s = m.stream(q, ef, norm=norm)
            host = s.collect(al, needed, ef)
            s.close()
            assert host["launches"] == 0, tag
            s = m.stream(q, ef, norm=norm)
            want = cases.run_rule(s, lambda labs: np.fromiter((int(x) in al_set for x in labs), bool, len(labs)), needed, ef)
            s.close()
            wd, wl = cases.best_first(want["per_call"], needed)
            monkeypatch.delenv("RXGPU_HNSW_COLLECT")
            one = m.search_knn_streamed(q, needed, ef, al, norm=norm)   # rxgpu_hnsw_collect_knn_sq8: the one-shot call over the codes
            assert one["launches"] >= 1, tag
            for name, r in (("device", got), ("host", host), ("one-shot", one)):
                assert r["presented_at_cut"] == cases.presented_at_cut(want, needed), tag + (name, r["presented_at_cut"])
                prev, per = 0, []
                for b, e, acc in want["calls"]:
                    per.append((b, e, acc - prev))
                    prev = acc
                assert [tuple(int(x) for x in c) for c in r["calls"]] == per, tag + (name,)
                assert (r["presented"], r["accepted"], r["exhausted"]) == (want["presented"], want["accepted"], want["exhausted"]), tag + (name,)
                assert np.array_equal(r["labels"], wl) and np.array_equal(bits(r["dist"]), bits(wd)), tag + (name,)
    m.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_c_abi_sq8_one_shot_equals_the_sq8_session(rxgpu, oracle, monkeypatch, metric):
    """rxgpu_hnsw_collect_knn_sq8 through its own binding (VectorIndex.hnsw_collect_knn_sq8), on codes attached by hand: rows, distance bits,
    positions, records and launches of rxgpu_hnsw_stream_begin_sq8 + collect + end, which in turn equal the Python rule over the SQ8
    session's Continue."""
    from reindexer_amd.hostapi import sq8_quantize, sq8_quantize_many
    from oracle.pyoracle import Sq8Oracle
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.A, metric)
    rows, n, d = g["vectors"], g["n"], g["dim"]
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))
    alpha_2 = float(Sq8Oracle(oracle).params(min_q, max_q, d)["alpha_2"])
    codes, corr = sq8_quantize_many(metric, min_q, max_q, rows)
    q, coef = cases.make_corpus(900, 1, d)[0], np.float32(1.0)
    if metric == 2:
        q, k_ = oracle.normalize_copy(q)
        coef = np.float32(k_)   # normCoef = 1 / norm
    qc, qo, _ = sq8_quantize(metric, min_q, max_q, q, float(np.float32(1.0) / coef))   # prepareData: norm = 1.f / normCoef
    with _Index(rxgpu, oracle, g) as dev:
        ix = dev.ix
        ix.hnsw_attach_sq8(codes, corr, alpha_2)
        for share, needed, ef in ((0.5, 10, 100), (0.02, 150, 16), (1, 150, 100)):
            allowed = cases.allowed_rows(n, share)
            words = cases.words_of(allowed)
            with ix.hnsw_stream_sq8(qc, float(qo), float(coef), ef) as s:
                got = s.collect(words, needed, ef)
            with ix.hnsw_stream_sq8(qc, float(qo), float(coef), ef) as s:
                check_against_rule(got, cases.run_rule(s, lambda r: allowed[r], needed, ef), (metric, share, needed, ef))
            one = ix.hnsw_collect_knn_sq8(qc, float(qo), float(coef), ef, words, needed, ef)
            for k in ("row", "pos", "calls"):
                assert np.array_equal(one[k], got[k]), (metric, share, needed, ef, k)
            assert np.array_equal(bits(one["dist"]), bits(got["dist"]))
            assert all(one[k] == got[k] for k in ("presented", "accepted", "exhausted", "launches"))
            assert got["accepted"] > 0


# ------------------------------------------------------------------------------------------------ D. edges
def test_collect_edges(rxgpu, oracle, monkeypatch):
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.A, 0)
    n = g["n"]
    q = cases.query(oracle, 0, g["dim"])
    with _Index(rxgpu, oracle, g) as dev:
        ix = dev.ix
        allowed = cases.allowed_rows(n, 0.1)
        # needed 0 / first_batch 0: nothing runs, whatever the buffers
        with ix.hnsw_stream(q, 100) as s:
            for needed, fb in ((0, 100), (10, 0)):
                r = s.collect(cases.words_of(allowed), needed, fb, cap=0, calls_cap=0)
                assert (len(r["calls"]), r["presented"], r["accepted"], r["exhausted"], r["launches"]) == (0, 0, 0, False, 0)
            # ... and the session is untouched: a collection behind them equals one on a fresh session
            after = s.collect(cases.words_of(allowed), 10, 100)
        with ix.hnsw_stream(q, 100) as s:
            fresh = s.collect(cases.words_of(allowed), 10, 100)
        assert np.array_equal(after["row"], fresh["row"]) and np.array_equal(after["calls"], fresh["calls"])
        # a NULL bitmap = all ones; bits at and above the count are ignored
        everything = np.ones(n, bool)
        with ix.hnsw_stream(q, 100) as s:
            null = s.collect(None, 150, 100)
        with ix.hnsw_stream(q, 100) as s:
            ones = s.collect(cases.words_of(everything), 150, 100)
        for k in ("row", "calls"):
            assert np.array_equal(null[k], ones[k]), k
        assert np.array_equal(bits(null["dist"]), bits(ones["dist"])) and null["accepted"] == null["presented"] >= 150
        with ix.hnsw_stream(q, 100) as s:
            dirty = s.collect(cases.words_of(allowed, extra_words=3, garbage=True), 150, 100)
        with ix.hnsw_stream(q, 100) as s:
            clean = s.collect(cases.words_of(allowed), 150, 100)
        assert np.array_equal(dirty["row"], clean["row"]) and np.array_equal(dirty["calls"], clean["calls"]) and dirty["accepted"] == clean["accepted"]
        # short n_words, short cap, short calls_cap: refused before anything runs
        words = cases.words_of(allowed)
        bound = int(rxgpu.lib().rxgpu_hnsw_stream_collect_bound(n, 150, 100))
        assert bound == 150 - 1 + 800
        with ix.hnsw_stream(q, 100) as s:
            for kw in (dict(n_words=words.size - 1), dict(cap=bound - 1), dict(calls_cap=999)):
                with pytest.raises(rxgpu.RxGpuError):
                    s.collect(words, 150, 100, **kw)
            ok = s.collect(words, 150, 100, cap=bound, calls_cap=1000)   # the session was not touched by the refused calls
        assert np.array_equal(ok["row"], clean["row"]) and np.array_equal(ok["calls"], clean["calls"])
        # max_calls 2 on a collection that needs more: stops after 2, not exhausted
        sparse = cases.allowed_rows(n, 0.01)
        full = cases.oracle_rule(oracle, g, q, None, sparse, 150, 100, 100)
        assert len(full["calls"]) == 5
        got, want = collect_three_ways(rxgpu, oracle, dev, q, sparse, 150, 100, 100, ("max_calls",), max_calls=2)
        assert len(got["calls"]) == 2 and not got["exhausted"] and got["accepted"] < 150
        # the session afterwards is in the state behind its last Continue: next(50) equals the engine's next(50) behind the same calls
        with ix.hnsw_stream(q, 100) as s:
            s.collect(cases.words_of(sparse), 150, 100, 2)
            gd, gr, gex = s.next(50)
            again = s.collect(cases.words_of(sparse), 10, 100)   # ... and it takes a further collection
        want = cases.oracle_rule(oracle, g, q, None, sparse, 150, 100, 100, max_calls=2, keep_session=True)
        wd, wl, wex = want["session"].next(50)
        a, w = _sorted_pairs(gd, g["labels"][gr]), _sorted_pairs(wd, wl)
        assert gex == wex and np.array_equal(a[1], w[1]) and np.array_equal(a[0], w[0])
        row_of = {int(lab): i for i, lab in enumerate(g["labels"])}
        more = cases.run_rule(want["session"], lambda labs: sparse[np.fromiter((row_of[int(x)] for x in labs), np.int64, len(labs))], 10, 100)
        want["session"].close()
        check_against_oracle(again, more, g["labels"], ("collect behind next",))
        # a graph mutated under the session
        with ix.hnsw_stream(q, 100) as s:
            ix.truncate(n - 1)
            with pytest.raises(rxgpu.RxGpuError):
                s.collect(words, 10, 100)


def test_collect_on_an_empty_graph(rxgpu):
    with rxgpu.VectorIndex(0, 16, 8) as ix:
        with ix.hnsw_stream(np.zeros(16, np.float32), 100) as s:
            r = s.collect(None, 10, 100, cap=0, calls_cap=0)
    assert (len(r["calls"]), r["presented"], r["accepted"], r["exhausted"], r["launches"]) == (0, 0, 0, True, 0)


def test_collect_exhausts_inside_a_call(rxgpu, oracle, monkeypatch):
    """200 x 16: the second call asks for more rows than the graph has left and delivers what there is"""
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.SMALL, 0)
    q = cases.query(oracle, 0, g["dim"])
    allowed = cases.allowed_rows(g["n"], 0.3)
    with _Index(rxgpu, oracle, g) as dev:
        got, want = collect_three_ways(rxgpu, oracle, dev, q, allowed, 70, 100, 100, ("small",))
    assert got["exhausted"] and len(got["calls"]) == 2 and got["calls"][1][0] > got["calls"][1][1], got["calls"]
    print("collect small:", got["calls"].tolist())


# ------------------------------------------------------------------------------------------------ E. the Map: one-shot, threads, shards
def test_map_one_shot_equals_begin_collect_end(rxgpu, oracle, monkeypatch):
    """GpuHnswMap::SearchKnnStreamed == BeginStreamingSearch + CollectStreaming + the session's end == the host loop (RXGPU_HNSW_COLLECT=host)
    == the rule over the restated engine with its best-first cut; four threads with bitmaps of their own against the serial answers."""
    from reindexer_amd import hostapi
    monkeypatch.delenv("RXGPU_HNSW_COLLECT", raising=False)
    monkeypatch.delenv("RXGPU_HNSW_STREAM_GLOBAL", raising=False)
    g = cases.graph(cases.A, 2)
    n, d = g["n"], g["dim"]
    labels = cases.labels_of(n)
    m = hostapi.GpuHnswMap(2, d, n, M=cases.A["M"], ef_construction=cases.A["efc"])
    m.add(g["vectors"], labels)
    inv = oracle.l2_modules(g["vectors"])
    q = cases.query(oracle, 2, d)
    serial = {}
    for share in (0.5, 0.1, 0.02, 0.3):
        allowed = cases.allowed_rows(n, share) if share != 0.3 else np.random.default_rng(11).random(n) < share
        al = labels[allowed]
        for needed, ef in ((10, 100), (150, 16)):
            tag = (share, needed, ef)
            one = m.search_knn_streamed(q, needed, ef, al)
            s = m.stream(q, ef)
            two = s.collect(al, needed, ef)
            s.close()
            monkeypatch.setenv("RXGPU_HNSW_COLLECT", "host")
            host = m.search_knn_streamed(q, needed, ef, al)
            monkeypatch.delenv("RXGPU_HNSW_COLLECT")
            want = cases.oracle_rule(oracle, g, q, inv, allowed, needed, ef, ef)
            wd, wl = cases.best_first(want["per_call"], needed)
            assert one["launches"] >= 1 and host["launches"] == 0, tag
            cut = cases.presented_at_cut(want, needed)
            assert cut <= want["presented"] and (want["accepted"] >= needed or cut == want["presented"]), tag
            for name, r in (("one-shot", one), ("begin+collect", two), ("host", host)):
                assert r["presented_at_cut"] == cut, tag + (name, r["presented_at_cut"], cut)
                assert np.array_equal(r["labels"], wl) and np.array_equal(bits(r["dist"]), bits(wd)), tag + (name,)
                assert (r["n_calls"], r["presented"], r["accepted"], r["exhausted"]) == (len(want["calls"]), want["presented"], want["accepted"],
                                                                                         want["exhausted"]), tag + (name,)
                assert np.array_equal(np.cumsum(r["calls"][:, 2]), [c[2] for c in want["calls"]]), tag + (name,)
            serial[tag] = (al, one)
    errors = []

    def worker(tag):
        try:
            al, want = serial[tag]
            for _ in range(5):
                r = m.search_knn_streamed(q, tag[1], tag[2], al)
                assert np.array_equal(r["labels"], want["labels"]) and np.array_equal(bits(r["dist"]), bits(want["dist"])) and \
                    np.array_equal(r["calls"], want["calls"]), tag
        except Exception as e:   # noqa: BLE001
            errors.append((tag, repr(e)))

    threads = [threading.Thread(target=worker, args=(tag,)) for tag in [(0.5, 10, 100), (0.1, 150, 16), (0.02, 10, 100), (0.3, 150, 16)]]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    m.close()


def test_empty_map_and_sharded_handle(rxgpu, monkeypatch):
    """An empty Map: 0 calls, exhausted — from the device call and from the host loop alike.  The one-shot call on a sharded handle:
    RXGPU_ERR_LOGIC, like rxgpu_hnsw_stream_begin."""
    from reindexer_amd import hostapi
    m = hostapi.GpuHnswMap(0, 16, 64, M=8, ef_construction=100)
    q = np.zeros(16, np.float32)
    for mode in (None, "host"):
        if mode:
            monkeypatch.setenv("RXGPU_HNSW_COLLECT", mode)
        else:
            monkeypatch.delenv("RXGPU_HNSW_COLLECT", raising=False)
        for r in (m.search_knn_streamed(q, 10, 100, [1, 2]), ):
            assert (r["n_calls"], r["presented"], r["presented_at_cut"], r["accepted"], r["exhausted"], len(r["labels"])) == (0, 0, 0, 0, True, 0), mode
        s = m.stream(q, 100)
        r = s.collect([1, 2], 10, 100)
        s.close()
        assert (r["n_calls"], r["presented"], r["accepted"], r["exhausted"]) == (0, 0, 0, True), mode
    m.close()
    with rxgpu.ShardedVectorIndex(1, 16, 256, [0, 0]) as sx:
        with pytest.raises(rxgpu.RxGpuError) as e:
            sx.hnsw_collect_knn(q, 100, None, 10, 100)
        assert e.value.code == rxgpu.RXGPU_ERR_LOGIC


def test_map_over_two_shards_runs_the_host_loop(rxgpu, oracle, monkeypatch):
    """A Map over a device list (two shards on one device) always takes the host loop: the plan functions over its merged
    ContinueStreamingSearch — checked against the Python rule over the same Map's next()."""
    from reindexer_amd import hostapi
    monkeypatch.delenv("RXGPU_HNSW_COLLECT", raising=False)
    n, d = 2000, 32
    rows = cases.make_corpus(65, n, d)
    labels = cases.labels_of(n)
    m = hostapi.GpuHnswMap(0, d, n, M=8, ef_construction=100, devices=[0, 0])
    m.add(rows, labels)
    q = cases.make_corpus(900, 1, d)[0]
    for share, needed, ef in ((0.5, 10, 100), (0.02, 150, 16)):
        al = labels[cases.allowed_rows(n, share)]
        al_set = set(al.tolist())
        got = m.search_knn_streamed(q, needed, ef, al)
        s = m.stream(q, ef)
        want = cases.run_rule(s, lambda labs: np.fromiter((int(x) in al_set for x in labs), bool, len(labs)), needed, ef)
        s.close()
        wd, wl = cases.best_first(want["per_call"], needed)
        assert got["launches"] == 0 and got["presented_at_cut"] == cases.presented_at_cut(want, needed)
        assert np.array_equal(got["labels"], wl) and np.array_equal(bits(got["dist"]), bits(wd)), (share, needed, ef)
        assert (got["n_calls"], got["presented"], got["accepted"], got["exhausted"]) == (len(want["calls"]), want["presented"], want["accepted"],
                                                                                         want["exhausted"])
    m.close()
