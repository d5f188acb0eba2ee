"""-m gpu: the RESIDENT HNSW search kernel over SQ8 codes (hnsw_server_sq8_kernel, hnsw_server.hip; host side rxgpu_hnsw_server.hip): ONE
quantised query per call, the planner's concurrency model over a quantised graph.
Bar: a query answered through the mailbox over codes returns exactly what the launching path returns (the same device code, itself pinned to
the reference's quantised engine in test_gpu_sq8.py), what the restated quantised engine returns and what the real one (RefHnswQ) returns —
whatever the threads, the generations of the kernel and the mutations of the index in between.
The share of served queries is not a fixed number here: equal keys are more frequent over integer codes than over floats.  The rule is per
query — what the launches answer without a re-run, the mailbox serves — and the launch-flagged queries may be at most kFlaggedCap of a case."""
import threading
import time

import numpy as np
import pytest

from .conftest import make_corpus
from .test_gpu_hnsw_server import Env, bits, build, pairs, queries_for

pytestmark = pytest.mark.gpu

kFlaggedCap = 0.25   # non-vacuity: so many of a case's queries, at most, may need a re-run on the launch path


@pytest.fixture(scope="module")
def sq8(oracle):
    from oracle.pyoracle import Sq8Oracle
    return Sq8Oracle(oracle)


def quantise_rows(sq8, metric, vecs):
    """The code table of the rows as the restated quantiser makes it: (min_q, max_q, sq dict for oracle_hnsw_search_knn_sq8)."""
    vecs = np.asarray(vecs)
    min_q, max_q = float(np.quantile(vecs, 0.005)), float(np.quantile(vecs, 0.995))
    p = sq8.params(min_q, max_q, vecs.shape[1])
    stored = [sq8.quantize(metric, p, x) for x in vecs]
    sq = dict(min_q=p["min_q"], alpha=p["alpha"], alpha_2=p["alpha_2"], delta=p["delta"], codes=np.stack([c for c, _ in stored]),
              corr=np.array([o for _, o in stored], np.float32))
    return min_q, max_q, sq


def quantise_queries(oracle, metric, min_q, max_q, raw):
    """prepareData for every query: (float queries as SearchKnn gets them, norms as query_data_norm (None: not cosine), codes, corr, normCoef)."""
    from reindexer_amd.hostapi import sq8_quantize
    qs, norms, qc, qo, qn = [], [], [], [], []
    for q in raw:
        norm = None
        coef = np.float32(1.0)
        if metric == 2:
            q, k_ = oracle.normalize_copy(q)
            norm = float(np.float32(1.0) / np.float32(k_))
            coef = np.float32(1.0) / np.float32(norm)
        c, o, _ = sq8_quantize(metric, min_q, max_q, q, float(np.float32(1.0) / coef))   # norm = 1.f / normCoef (hnswalg.h:510-529)
        qs.append(q), norms.append(norm), qc.append(c), qo.append(o), qn.append(coef)
    return np.stack(qs), norms, np.stack(qc), np.array(qo, np.float32), np.array(qn, np.float32)


class Case:
    """A graph built by GpuHnswMap, exported, with its SQ8 code table and quantised queries; attach(ix) makes a device index of it."""

    def __init__(self, oracle, sq8, metric, d, deleted, n=None, nq=48, M=8, efc=100, seed=5):
        self.metric, self.d = metric, d
        self.n = n or (6000 if d > 128 else 12000)
        self.m, self.g, _ = build(oracle, metric, self.n, d, M=M, efc=efc, seed=seed, deleted=deleted)
        self.vecs = np.array(self.g["vectors"])
        self.inv = oracle.l2_modules(self.vecs) if metric == 2 else None
        self.min_q, self.max_q, self.sq = quantise_rows(sq8, metric, self.vecs)
        self.q, self.norms, self.qc, self.qo, self.qn = quantise_queries(oracle, metric, self.min_q, self.max_q, make_corpus(700, nq, d))

    def attach(self, ix):
        ix.upload_rows(0, self.g["vectors"], self.g["inv_norms"] if self.metric == 2 else None)
        ix.hnsw_attach_graph(self.g)
        ix.hnsw_attach_sq8(self.sq["codes"], self.sq["corr"], float(self.sq["alpha_2"]))

    def launched(self, ix, qi, k, ef):
        """(dist, row, count, flagged) of query qi on the launch path: flagged = it needed a re-run there (a tie or LDS re-run, counted by the
        library around this one call)."""
        with Env(RXGPU_HNSW_SERVER=0):
            ix.hnsw_read_tie_reruns(), ix.hnsw_read_lds_reruns()
            ld, lr, lc = ix.hnsw_search_knn_sq8(self.qc[qi][None, :], self.qo[qi:qi + 1], self.qn[qi:qi + 1], k, ef)
            flagged = ix.hnsw_read_tie_reruns() + ix.hnsw_read_lds_reruns()
        return ld[0], lr[0], int(lc[0]), flagged > 0

    def posted(self, ix, qi, k, ef):
        """(dist, row, count, ok, by the mailbox itself): ok = the posted call answered; the last = the resident kernel's own answer, not the
        re-run tiers behind a flagged search."""
        s0 = ix.hnsw_server_stats()[0]
        pd, pr, pc, ok = ix.hnsw_search_knn_sq8_posted(self.qc[qi], self.qo[qi], self.qn[qi], k, ef)
        return pd, pr, pc, ok, ix.hnsw_server_stats()[0] > s0

    def restated(self, oracle, qi, k, ef):
        from oracle.pyoracle import oracle_hnsw_search_knn_sq8
        return oracle_hnsw_search_knn_sq8(oracle, self.g, self.sq, self.q[qi], k, ef, self.inv, self.norms[qi])

    def close(self):
        self.m.close()


CASES = [(0, 128, 0), (1, 768, 0), (2, 768, 0), (2, 512, 0), (0, 128, 300), (2, 768, 200), (1, 384, 0)]
_cases = {}


@pytest.fixture(scope="module")
def case_of(oracle, sq8):
    """The cases of the two tests below, built once (the graph build is most of a case's time)."""
    def get(metric, d, deleted):
        key = (metric, d, deleted)
        if key not in _cases:
            _cases[key] = Case(oracle, sq8, metric, d, deleted)
        return _cases[key]
    yield get
    for c in _cases.values():
        c.close()
    _cases.clear()


def plans_of(deleted):
    return ((10, 128 if not deleted else 96), (10, 10), (1, 0), (40, 64), (10, 256 if not deleted else 224), (60, 200))   # the last two: the second mailbox over codes


def same_answer(a_dist, a_row, b_dist, b_row):
    a, b = pairs(a_dist, a_row), pairs(b_dist, b_row)
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("metric,d,deleted", CASES)
def test_posted_equals_launched_restated_and_real_engine(rxgpu, oracle, case_of, metric, d, deleted):
    c = case_of(metric, d, deleted)
    with rxgpu.VectorIndex(metric, d, c.n) as ix:
        c.attach(ix)
        served = 0
        for k, ef in plans_of(deleted):
            for qi in range(c.q.shape[0]):
                pd, pr, pc, ok, _ = c.posted(ix, qi, k, ef)
                ld, lr, lc, _ = c.launched(ix, qi, k, ef)
                if ok:
                    served += 1
                    assert pc == lc, (k, ef, qi)
                    assert same_answer(pd[:pc], pr[:pc], ld[:pc], lr[:pc]), (k, ef, qi)
                if qi < 6:   # ... and the restated quantised engine, whoever answered
                    wd, wl = c.restated(oracle, qi, k, ef)
                    gd, gr = (pd[:pc], pr[:pc]) if ok else (ld[:lc], lr[:lc])
                    assert np.array_equal(np.sort(c.g["labels"][gr]), np.sort(wl)), (k, ef, qi)
                    assert np.array_equal(np.sort(bits(gd)), np.sort(bits(wd))), (k, ef, qi)
        got, gens = ix.hnsw_server_stats()
        assert 0 < got <= served and gens >= 1, (got, served, gens)
        # what the mailbox over codes does not take: the correct answer still comes from the launches
        wd, wl = c.restated(oracle, 0, 10, 300)
        for env, ef in (({}, 300), (dict(RXGPU_HNSW_SERVER=0), 64), (dict(RXGPU_HNSW_SERVER_SQ8=0), 64)):
            with Env(**env):
                s0 = ix.hnsw_server_stats()[0]
                _, _, _, ok = ix.hnsw_search_knn_sq8_posted(c.qc[0], c.qo[0], c.qn[0], 10, ef)
                assert not ok, (env, ef)
                ld, lr, lc = ix.hnsw_search_knn_sq8(c.qc[0][None, :], c.qo[:1], c.qn[:1], 10, ef)
                assert ix.hnsw_server_stats()[0] == s0, (env, ef)
            want = (wd, wl) if ef == 300 else c.restated(oracle, 0, 10, ef)
            assert np.array_equal(np.sort(c.g["labels"][lr[0, :int(lc[0])]]), np.sort(want[1])) and \
                np.array_equal(np.sort(bits(ld[0, :int(lc[0])])), np.sort(bits(want[0]))), (env, ef)


def test_a_dimension_without_a_fixed_sq8_form_keeps_the_launches(rxgpu, oracle, sq8):
    """dim 96 runs the generic SQ8 distance batch, which re-reads the query codes at every batch: declined by the mailbox on the host."""
    c = Case(oracle, sq8, 0, 96, 0, n=3000, nq=4)
    with rxgpu.VectorIndex(0, 96, c.n) as ix:
        c.attach(ix)
        for qi in range(4):
            _, _, _, ok = ix.hnsw_search_knn_sq8_posted(c.qc[qi], c.qo[qi], c.qn[qi], 10, 64)
            assert not ok
            ld, lr, lc = ix.hnsw_search_knn_sq8(c.qc[qi][None, :], c.qo[qi:qi + 1], c.qn[qi:qi + 1], 10, 64)
            wd, wl = c.restated(oracle, qi, 10, 64)
            assert np.array_equal(np.sort(c.g["labels"][lr[0, :int(lc[0])]]), np.sort(wl)) and np.array_equal(np.sort(bits(ld[0, :int(lc[0])])), np.sort(bits(wd)))
        assert ix.hnsw_server_stats() == (0, 0)
    c.close()


@pytest.mark.parametrize("metric,d,deleted", CASES)
def test_what_the_launches_answer_without_a_rerun_the_mailbox_serves(rxgpu, case_of, metric, d, deleted):
    """Per query: the launch path needed no re-run (no tie re-run, no LDS re-run around its single-query call) => the resident kernel itself
    answers it.  The resident form runs the launch kernel's search with a visited set and a restart area at least as large, so it flags no
    class of search the launches do not; if it ever does, this is where it shows.  Non-vacuity: at most kFlaggedCap of the queries of a case
    are launch-flagged."""
    c = case_of(metric, d, deleted)
    with rxgpu.VectorIndex(metric, d, c.n) as ix:
        c.attach(ix)
        total = flagged = by_mailbox = 0
        broken = []
        for k, ef in plans_of(deleted):
            flags = [c.launched(ix, qi, k, ef)[3] for qi in range(c.q.shape[0])]   # (first: reading the counters makes a resident kernel leave)
            for qi, fl in enumerate(flags):
                _, _, _, ok, mailbox = c.posted(ix, qi, k, ef)
                total += 1
                flagged += int(fl)
                by_mailbox += int(mailbox)
                if not fl and not (ok and mailbox):
                    broken.append((k, ef, qi))
        msg = f"queries {total}, launch-flagged {flagged}, served by the resident kernel {by_mailbox}, unflagged but not served {broken[:8]}"
        print(msg)
        assert not broken, msg
        assert flagged <= kFlaggedCap * total, msg


@pytest.mark.parametrize("slots", [64, 3])
def test_sixteen_threads_one_quantised_query_each(rxgpu, oracle, sq8, slots):
    """The reference's runMultithreadQueries shape over codes: T threads, one SearchKnn each at a time, over one index.  With 3 slots most calls
    find the mailbox full and take a launch: same answers."""
    T, per = 16, 40
    c = Case(oracle, sq8, 2, 128, 0, n=20000, nq=64, M=16, efc=200)
    with Env(RXGPU_HNSW_SERVER_SLOTS=slots):
        with rxgpu.VectorIndex(2, 128, c.n) as ix:
            c.attach(ix)
            want = [c.launched(ix, qi, 10, 128) for qi in range(c.q.shape[0])]
            errors = []

            def worker(t):
                try:
                    for j in range(per):
                        qi = (t * per + j) % c.q.shape[0]
                        d_, r_, c_ = ix.hnsw_search_knn_sq8(c.qc[qi][None, :], c.qo[qi:qi + 1], c.qn[qi:qi + 1], 10, 128)
                        w = want[qi]
                        if int(c_[0]) != w[2] or not same_answer(d_[0], r_[0], w[0], w[1]):
                            errors.append((t, j))
                except Exception as e:   # noqa: BLE001
                    errors.append((t, repr(e)))

            th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert not errors, errors[:4]
            served, _ = ix.hnsw_server_stats()
            assert served > 0
            if slots == 64:   # every thread finds a slot: the per-query rule holds for the whole run
                unflagged = sum(1 for t in range(T) for j in range(per) if not want[(t * per + j) % c.q.shape[0]][3])
                flagged = T * per - unflagged
                msg = f"calls {T * per}, launch-flagged {flagged}, served by the resident kernel {served}"
                print(msg)
                assert served >= unflagged, msg
                assert flagged <= kFlaggedCap * T * per, msg
    c.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_quantised_map_equals_the_real_quantised_engine_through_the_mailbox(rxgpu, ref, oracle, metric):
    """RefHnsw + RefHnswQ and GpuHnswMap built from the same inserts, with deletes, quantised with the range the reference sampled: the Map's
    single queries now travel through the mailbox over codes and still equal the real engine in labels and distance bits."""
    from oracle.pyoracle import RefHnsw, RefHnswQ
    from reindexer_amd import hostapi
    n, d, nq = 4000, 128, 24
    rows = make_corpus(183 + metric, n, d)
    labels = (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(2)
    rf = RefHnsw(ref, metric, d, n, M=12, ef_construction=80)
    rf.add(rows, labels)
    m = hostapi.GpuHnswMap(metric, d, n, M=12, ef_construction=80)
    m.add(rows, labels)
    for lab in labels[np.random.default_rng(4).choice(n, 120, replace=False)]:
        rf.mark_delete(lab)
        m.mark_delete(lab)
    rq = RefHnswQ(rf, sample_size=n)
    prm = rq.export()
    m.quantize(float(prm["min_q"]), float(prm["max_q"]))
    asks = []
    for qi in range(nq):
        q = make_corpus(3300 + qi, 1, d)[0]
        norm = None
        if metric == 2:
            q, k_ = oracle.normalize_copy(q)
            norm = float(np.float32(1.0) / np.float32(k_))
        asks.append((q, norm))
    unflagged = 0
    with Env(RXGPU_HNSW_SERVER=0):   # which of them the launches answer without a re-run
        for q, norm in asks:
            m.tie_reruns(), m.lds_reruns()
            m.search_knn_norm(q, 40, 64, norm)
            unflagged += int(m.tie_reruns() + m.lds_reruns() == 0)
    p0 = m.posted_queries()
    for qi, (q, norm) in enumerate(asks):
        wd, wl = rq.search_knn(q, 40, 64, norm)
        gd, gl = m.search_knn_norm(q, 40, 64, norm)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gd), bits(wd)), (metric, qi)
    msg = f"queries {nq}, answered by the launches without a re-run {unflagged}, posted {m.posted_queries() - p0}"
    print(msg)
    assert m.posted_queries() - p0 >= unflagged, msg
    assert nq - unflagged <= kFlaggedCap * nq, msg
    rq.close()
    rf.close()
    m.close()


def test_quantised_map_mutations_between_posted_queries(rxgpu, oracle, sq8):
    """Upserts, deletes and a resize of a QUANTISED Map between single queries: every upload of code rows (and the new code table behind a
    resize) makes the resident kernel over the codes leave first, and the next query sees the new graph and the new codes — equal to the
    restated quantised engine over the Map's exported graph each time."""
    from oracle.pyoracle import oracle_hnsw_search_knn_sq8
    from reindexer_amd import hostapi
    n, d = 6000, 128
    rows = make_corpus(11, n, d)
    labels = np.arange(n, dtype=np.uint64) << np.uint64(32)
    m = hostapi.GpuHnswMap(0, d, 3000, M=8, ef_construction=100)
    q = queries_for(oracle, 0, d, 12)
    min_q, max_q = float(np.quantile(rows, 0.005)), float(np.quantile(rows, 0.995))
    p = sq8.params(min_q, max_q, d)
    at = 0
    for step, upto in enumerate((1500, 3000, 4500, 6000)):
        if step == 2:
            m.resize(n)
        m.add(rows[at:upto], labels[at:upto])
        at = upto
        if step == 0:
            m.quantize(min_q, max_q)
        if step == 3:
            for lab in labels[100:160]:
                m.mark_delete(lab)
        g = m.export_graph(with_views=True)
        stored = [sq8.quantize(0, p, x) for x in np.array(g["vectors"])]
        sq = dict(min_q=p["min_q"], alpha=p["alpha"], alpha_2=p["alpha_2"], delta=p["delta"], codes=np.stack([c for c, _ in stored]),
                  corr=np.array([o for _, o in stored], np.float32))
        for x in q:
            gd, gl = m.search_knn_norm(x, 10, 64, None)
            wd, wl = oracle_hnsw_search_knn_sq8(oracle, g, sq, x, 10, 64, None, None)
            assert np.array_equal(gl, wl), step
            assert np.array_equal(bits(gd), bits(wd)), step
    assert m.posted_queries() >= 36, m.posted_queries()   # the queries did go through the mailbox (48 asked; the cap of the flagged share leaves 36)
    m.close()


def test_generations_idle_exit_and_restart_over_codes(rxgpu, oracle, sq8):
    c = Case(oracle, sq8, 0, 128, 0, n=8000, nq=8)
    with Env(RXGPU_HNSW_SERVER_IDLE_US=300, RXGPU_HNSW_SERVER_LIFE_MS=5):
        with rxgpu.VectorIndex(0, 128, c.n) as ix:
            c.attach(ix)
            ask = lambda qi: ix.hnsw_search_knn_sq8_posted(c.qc[qi], c.qo[qi], c.qn[qi], 10, 64)   # noqa: E731
            want = [ask(qi) for qi in range(8)]
            assert all(w[3] for w in want)
            g0 = ix.hnsw_server_stats()[1]
            for rnd in range(6):   # the kernel has left by itself each time: the next query launches the next generation
                time.sleep(0.02)
                for qi, w in enumerate(want):
                    pd, pr, pc, ok = ask(qi)
                    assert ok and pc == w[2] and same_answer(pd, pr, w[0], w[1])
            assert ix.hnsw_server_stats()[1] >= g0 + 6
            # ... and a stream of queries longer than the lifetime crosses generations without a gap in the answers
            t0 = time.perf_counter()
            cnt = 0
            while time.perf_counter() - t0 < 0.06:
                pd, pr, pc, ok = ask(cnt % 8)
                w = want[cnt % 8]
                assert pc == w[2] and same_answer(pd, pr, w[0], w[1])
                cnt += 1
            assert ix.hnsw_server_stats()[1] >= g0 + 8
    c.close()


def test_a_float_and_a_code_mailbox_and_a_scan_side_by_side(rxgpu, oracle, sq8):
    """The resident kernel of a float index and the one over another index's codes alive at once, a brute-force scan and a batch launch beside
    them: nothing waits for a kernel that waits for the host."""
    n, d = 8000, 128
    ma, ga, _ = build(oracle, 0, n, d, seed=21)
    cb = Case(oracle, sq8, 1, d, 0, n=n, nq=16, seed=22)
    q = queries_for(oracle, 0, d, 16)
    with rxgpu.VectorIndex(0, d, n) as a, rxgpu.VectorIndex(1, d, n) as b:
        a.upload_rows(0, ga["vectors"], None)
        a.hnsw_attach_graph(ga)
        cb.attach(b)
        t0 = time.perf_counter()
        for qi, x in enumerate(q):
            ra = a.hnsw_search_knn_posted(x, 10, 64)
            rb = b.hnsw_search_knn_sq8_posted(cb.qc[qi], cb.qo[qi], cb.qn[qi], 10, 64)
            sd, sr, _ = a.search_knn(x, 11)                                        # a scan on an ordinary stream while both resident kernels are alive
            bd, br, bc = b.hnsw_search_knn_sq8(cb.qc[:8], cb.qo[:8], cb.qn[:8], 10, 64)   # ... and a batch launch over the codes
            assert ra[3] and rb[3]
            assert set(rb[1][:rb[2]].tolist()) <= set(range(n)) and sr.shape[1] == 11 and int(bc[0]) == 10
        assert time.perf_counter() - t0 < 5.0
        assert a.hnsw_server_stats()[0] > 0 and b.hnsw_server_stats()[0] > 0
    ma.close()
    cb.close()
