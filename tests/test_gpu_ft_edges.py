"""-m gpu: every BM25 merge train at the edges of its geometry — the cases of tests/ft_edge_cases.py (documents PLACED on both sides of every
8192-document range boundary, on the last document, on the sparse train's lane-wrap offsets; range segments of exactly 256 / 512 / 1024
postings and one more or less; a full range of 32 staged blocks and a 33rd; an empty segment between two filled ones; words whose range
index ends before the index does; 4 .. 17 sub-terms; the preselect cut ON a boundary; an index grown across boundaries), which
tests/test_ft_edge_cases.py has shown on the CPU to be non-vacuous and on which the restated merger equals the real ft::Merger.

Bar, everywhere: the merged documents IN MERGE ORDER, raw rank bits, fields, terms counters / uint8 ranks and the preselect flag, and the
(document -> rank, field) map of the rank-sorted flavour.  No tolerances.  The dense train (ft_merge.hip and its kernel units) and the sparse
train (ft_sparse.hip) run every case they are eligible for — rxgpu_ft_read_train_stats says which one ran — and must equal each other and
the restated merger; so must merge() over the flat entries, words uploaded packed and decoded on the device, batches, document-range shards
whose cuts fall on the planted boundaries, and phrases (against the real merger)."""
import numpy as np
import pytest

from oracle.pyoracle import FtOracle, ref_ft_or_none
from . import ft_edge_cases as ec
from .ft_pack import flat_entries, pack_postings

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ft(oracle):
    return FtOracle(oracle)


@pytest.fixture()
def hostapi(rxgpu):
    from reindexer_amd import hostapi as h
    h.lib()
    yield h
    h.set_ft_train_mode(-1)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
            and np.array_equal(a[3], b[3]) and a[4] == b[4])


def assert_oracle(g, w, what):
    assert g[4] == w[4], what
    assert np.array_equal(g[0], w[0].astype(np.int32)), (what, len(g[0]), len(w[0]), np.setxor1d(g[0], w[0].astype(np.int32))[:8])
    assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), what
    assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), what


def assert_sorted_flavour(m, cfg, gterms, exc, g, what):
    """rank-sorted flavour: the same (document -> rank, field) map, non-increasing ranks"""
    sd, _, sf, sn, _ = m.merge_query(cfg, gterms, exc, sort_by_rank=True)
    assert np.all(np.diff(sn.astype(int)) <= 0), what
    o1, o2 = np.argsort(sd, kind="stable"), np.argsort(g[0], kind="stable")
    assert np.array_equal(sd[o1], g[0][o2]) and np.array_equal(sn[o1], g[3][o2]) and np.array_equal(sf[o1], g[2][o2]), what


class Pair:
    """Two mergers over the same index: one only ever runs the dense train, the other the sparse one whenever the query is eligible — a train
    never finds the other's result of the same query in its output buffers."""

    def __init__(self, hostapi, nf):
        self.dense, self.sparse = self.ms = [hostapi.GpuFtMerger(nf) for _ in range(2)]

    def set_docs(self, words, avg, removed):
        for m in self.ms:
            m.set_docs(words, avg, removed)

    def upload(self, store):
        for m in self.ms:
            for s in store:
                m.set_word_fpos(s["word"], s)

    def close(self):
        for m in self.ms:
            m.close()


def both_trains(hostapi, pair, cfg, gterms, exc, expect_sparse):
    hostapi.set_ft_train_mode(1)
    pair.sparse.read_train_stats()
    s = pair.sparse.merge_query(cfg, gterms, exc, sort_by_rank=False)
    assert pair.sparse.read_train_stats() == ((0, 1) if expect_sparse else (1, 0))
    hostapi.set_ft_train_mode(0)
    pair.dense.read_train_stats()
    d = pair.dense.merge_query(cfg, gterms, exc, sort_by_rank=False)
    assert pair.dense.read_train_stats() == (1, 0)
    return d, s


_entries = {}


def entries_of(s):
    """the flat (field, tf, first position) entries of a sub-term, as merge() and the restated mergeSimple read them"""
    key = id(s)
    if key not in _entries:
        eo, ef, et, e1, ro = flat_entries(s["doc"], s["pos_off"], s["fpos"])
        _entries[key] = (s, dict(doc=s["doc"], ent_off=eo, ent_field=ef, ent_tf=et, ent_first_pos=e1, proc=s["proc"]), ro)
    return _entries[key][1:]


def run_queries(hostapi, ft, pair, case, total, words, avg, queries, variants):
    """every query x flag variant on both trains, against each other and the restated merger; single OR terms through merge() as well"""
    nf = case["nf"]
    for vname, removed, excluded in variants:
        pair.set_docs(words, avg, removed)
        for q in queries:
            name, terms = q[0], q[1]
            what = (case["name"], name, vname)
            cfg = ft.default_config(nf, merge_limit=q[2] if len(q) > 2 else case["limit"])
            gterms = ec.gpu_terms(terms)
            w = ft.merge_query(cfg, terms, total, words, avg, removed, excluded, sort_by_rank=False)
            d, s = both_trains(hostapi, pair, cfg, gterms, excluded, expect_sparse=0 < ec.n_live_subs(terms) <= ec.SPARSE_SUBS)
            assert same(d, s), (what, len(d[0]), len(s[0]), np.setxor1d(d[0], s[0])[:8])
            assert_oracle(s, w, what)
            assert_sorted_flavour(pair.dense, cfg, gterms, excluded, d, what)
            hostapi.set_ft_train_mode(1)
            assert_sorted_flavour(pair.sparse, cfg, gterms, excluded, s, what)
            if len(terms) == 1 and terms[0]["op"] == ec.OR:     # Simple(): merge() over the flat entries
                osubs = [entries_of(x)[0] for x in terms[0]["subs"]]
                wd, wp, wf, wn = ft.merge_simple(cfg, terms[0]["opts"], total, words, avg, removed, excluded, osubs, sort_by_rank=False)
                hostapi.set_ft_train_mode(-1)
                gd, gp, gf, gn = pair.dense.merge(cfg, terms[0]["opts"], gterms[0]["subs"], excluded, sort_by_rank=False)
                assert np.array_equal(gd, wd.astype(np.int32)) and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), what
                assert np.array_equal(gf, wf) and np.array_equal(gn, wn), what
                assert np.array_equal(gd, d[0]) and np.array_equal(gp.view(np.uint32), d[1].view(np.uint32)), what


# ------------------------------------------------------------------------------------------------------------------------ both trains
@pytest.mark.parametrize("total", ec.TOTALS)
def test_case_a_totals_on_both_trains(hostapi, ft, total):
    """ONE pair of mergers runs every query shape x flag variant of the total in sequence: the kept-clean tables are handed from edge case
    to edge case."""
    case = ec.case_a(total)
    pair = Pair(hostapi, case["nf"])
    try:
        pair.set_docs(case["words"], case["avg"], None)
        pair.upload(case["store"])
        run_queries(hostapi, ft, pair, case, total, case["words"], case["avg"], case["queries"], case["variants"])
    finally:
        pair.close()


@pytest.mark.parametrize("group", ["count", "pair", "gap", "full", "early"])
def test_case_b_posting_counts_on_both_trains(hostapi, ft, group):
    case = ec.case_b()
    queries = [q for q in case["queries"] if q[0].startswith(group)]
    assert queries
    pair = Pair(hostapi, case["nf"])
    try:
        pair.set_docs(case["words"], case["avg"], None)
        pair.upload(case["store"])
        run_queries(hostapi, ft, pair, case, case["total"], case["words"], case["avg"], queries, case["variants"])
    finally:
        pair.close()


def test_case_c_sub_term_counts_pick_the_train(hostapi, ft):
    """4, 5, 8, 9 and 16 sub-terms: the sparse train must run (run_queries asserts the train from the count); 17: the dense one."""
    case = ec.case_c()
    assert [0 < ec.n_live_subs(t) <= ec.SPARSE_SUBS for _, t in case["queries"]] == [True] * 5 + [False]
    pair = Pair(hostapi, case["nf"])
    try:
        pair.set_docs(case["words"], case["avg"], None)
        pair.upload(case["store"])
        run_queries(hostapi, ft, pair, case, case["total"], case["words"], case["avg"], case["queries"], case["variants"])
    finally:
        pair.close()


def test_case_d_preselect_cut_on_the_boundary(hostapi, ft):
    case = ec.case_d(ft)
    pair = Pair(hostapi, case["nf"])
    try:
        pair.set_docs(case["words"], case["avg"], None)
        pair.upload(case["store"])
        run_queries(hostapi, ft, pair, case, case["total"], case["words"], case["avg"], case["queries"], case["variants"])
        hostapi.set_ft_train_mode(-1)
        for name, terms, limit, last, dropped in case["queries"]:
            cfg = ft.default_config(case["nf"], merge_limit=limit)
            for m in pair.ms:
                g = m.merge_query(cfg, ec.gpu_terms(terms), None, sort_by_rank=False)
                kept = np.intersect1d(g[0].astype(np.uint32), case["ties"])
                assert g[4] and len(g[0]) <= limit and kept.max() == last and dropped not in g[0], name
    finally:
        pair.close()


def test_case_e_grown_index(hostapi, ft):
    case = ec.case_e()
    pair = Pair(hostapi, case["nf"])
    try:
        for step in case["steps"]:
            pair.set_docs(step["words"], step["avg"], None)
            pair.upload(step["new"])
            run_queries(hostapi, ft, pair, case, step["total"], step["words"], step["avg"], step["queries"], [("none", None, None)])
    finally:
        pair.close()


# ---------------------------------------------------------------------------------------------------------------------- packed upload
_packed = {}


def packed_words(case):
    if case["name"] not in _packed:
        _packed[case["name"]] = [(s["word"],) + pack_postings(s["doc"], s["pos_off"], s["fpos"]) for s in case["store"]]
    return _packed[case["name"]]


@pytest.mark.parametrize("host_from", [None, 1 << 40], ids=["host_from_default", "all_on_device"])
@pytest.mark.parametrize("which", ["a16385", "b"])
def test_packed_upload_decodes_and_merges_the_same(hostapi, ft, which, host_from):
    case = ec.case_a(2 * ec.R + 1) if which == "a16385" else ec.case_b()
    nf, total, words, avg = case["nf"], case["total"], case["words"], case["avg"]
    m = hostapi.GpuFtMerger(nf)
    try:
        m.set_docs(words, avg, None)
        if host_from is None:
            m.set_words_packed(packed_words(case))
        else:
            m.set_words_packed(packed_words(case), host_from_bytes=host_from)
        for s in case["store"]:
            want, ro = entries_of(s)
            got = m.get_word(s["word"])
            assert np.array_equal(got["doc"], s["doc"]) and np.array_equal(got["pos_off"], s["pos_off"]) and np.array_equal(got["fpos"], s["fpos"])
            assert np.array_equal(got["ent_off"], want["ent_off"]) and np.array_equal(got["ent_field"], want["ent_field"])
            assert np.array_equal(got["ent_tf"], want["ent_tf"]) and np.array_equal(got["ent_first"], want["ent_first_pos"])
            assert np.array_equal(got["range_off"], ro), (s["word"], got["range_off"], ro)
        for vname, removed, excluded in [v for v in case["variants"] if v[0] in ("none", "around+exc")]:
            m.set_docs(words, avg, removed)
            for name, terms in case["queries"]:
                cfg = ft.default_config(nf, merge_limit=case["limit"])
                gterms = ec.gpu_terms(terms)
                w = ft.merge_query(cfg, terms, total, words, avg, removed, excluded, sort_by_rank=False)
                for mode in (0, 1):
                    hostapi.set_ft_train_mode(mode)
                    assert_oracle(m.merge_query(cfg, gterms, excluded, sort_by_rank=False), w, (which, name, vname, mode))
                if len(terms) == 1:
                    osubs = [entries_of(x)[0] for x in terms[0]["subs"]]
                    wd, wp, wf, wn = ft.merge_simple(cfg, terms[0]["opts"], total, words, avg, removed, excluded, osubs, sort_by_rank=False)
                    gd, gp, gf, gn = m.merge(cfg, terms[0]["opts"], gterms[0]["subs"], excluded, sort_by_rank=False)
                    assert np.array_equal(gd, wd.astype(np.int32)) and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), (which, name, vname)
                    assert np.array_equal(gf, wf) and np.array_equal(gn, wn), (which, name, vname)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------------------ batch
@pytest.mark.parametrize("total", [ec.R + 1, 4 * ec.R + 1])
def test_batch_of_every_shape_mixes_both_trains(hostapi, ft, total):
    """Every query shape of the total, a 16- and a 17-sub-term query in ONE merge_query_batch call, per removed-documents variant (a batch
    takes no excluded list: the excluded halves of the variants run in the single-query tests)."""
    case = ec.case_a(total)
    nf, words, avg = case["nf"], case["words"], case["avg"]
    wide = [dict(s, word=100 + s["word"]) for s in ec.case_c(total)["store"]]
    queries = [terms for _, terms in case["queries"]]
    queries.append([ec.term(ec.OR, wide[:8], nf), ec.term(ec.OR, wide[8:16], nf)])
    queries.append([ec.term(ec.OR, wide[:9], nf), ec.term(ec.OR, wide[9:17], nf)])
    m = hostapi.GpuFtMerger(nf)
    try:
        m.set_docs(words, avg, None)
        for s in case["store"] + wide:
            m.set_word_fpos(s["word"], s)
        cfg = ft.default_config(nf, merge_limit=case["limit"])
        for vname, removed, _ in [v for v in case["variants"] if v[0] in ("none", "around", "mirror")]:
            m.set_docs(words, avg, removed)
            hostapi.set_ft_train_mode(1)
            m.read_train_stats()
            got = m.merge_query_batch(cfg, [ec.gpu_terms(q) for q in queries], sort_by_rank=False)
            assert m.read_train_stats() == (1, len(queries) - 1)
            for qi, (terms, g) in enumerate(zip(queries, got)):
                assert_oracle(g, ft.merge_query(cfg, terms, total, words, avg, removed, None, sort_by_rank=False), (total, vname, qi))
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("which", ["a16385", "b", "d"])
def test_shard_cuts_on_planted_boundaries(rxgpu, hostapi, ft, which, shards):
    """Document-range shards over 16385 and 3 * 8192 + 5 documents: the cuts fall on 8192 / 16384 with planted documents on both sides.
    Bit-equal to the single index, and to the restated merger."""
    case = {"a16385": lambda: ec.case_a(2 * ec.R + 1), "b": ec.case_b, "d": lambda: ec.case_d(ft)}[which]()
    nf, total, words, avg = case["nf"], case["total"], case["words"], case["avg"]
    one = hostapi.GpuFtMerger(nf)
    many = hostapi.GpuFtMerger(nf, devices=[0] * shards)
    try:
        assert rxgpu.lib().rxgpu_ft_shard_count(many.device_index) == shards
        for m in (one, many):
            m.set_docs(words, avg, None)   # first: the cut of a sharded index follows the documents
            for s in case["store"]:
                m.set_word_fpos(s["word"], s)
        hostapi.set_ft_train_mode(-1)
        for vname, removed, excluded in [v for v in case["variants"] if v[0] in ("none", "around+exc", "mirror+exc")]:
            for m in (one, many):
                m.set_docs(words, avg, removed)
            for q in case["queries"]:
                name, terms = q[0], q[1]
                cfg = ft.default_config(nf, merge_limit=q[2] if len(q) > 2 else case["limit"])
                gterms = ec.gpu_terms(terms)
                a = one.merge_query(cfg, gterms, excluded, sort_by_rank=False)
                b = many.merge_query(cfg, gterms, excluded, sort_by_rank=False)
                assert same(a, b), (which, name, vname, len(a[0]), len(b[0]), np.setxor1d(a[0], b[0])[:8])
                assert_oracle(b, ft.merge_query(cfg, terms, total, words, avg, removed, excluded, sort_by_rank=False), (which, name, vname))
    finally:
        one.close()
        many.close()


# ---------------------------------------------------------------------------------------------------------------------------- phrases
@pytest.mark.parametrize("distance", [1, 8])
def test_phrases_over_planted_documents_equal_real_merger(hostapi, ft, distance):
    """A two-term phrase that matches in every planted document and in none next to them, as the whole query and as phrase OR term, against
    the real ft::Merger with its PhraseMerger."""
    case = ec.case_phrase(distance)
    nf, words, avg = case["nf"], case["words"], case["avg"]
    real = ref_ft_or_none(nf)
    if real is None:
        pytest.skip("oracle/_ref/libref_ft.so not available")
    m = hostapi.GpuFtMerger(nf)
    try:
        m.set_docs(words, avg, None)
        for s in case["store"]:
            real.set_word_fpos(s["word"], s)
            m.set_word_fpos(s["word"], s)
        cfg = ft.default_config(nf, merge_limit=case["limit"])
        for vname, removed, excluded in case["variants"]:
            real.set_docs(words, avg, removed)
            real.set_config(cfg)
            m.set_docs(words, avg, removed)
            live = case["planted"]
            for flags in (removed, excluded):
                if flags is not None:
                    live = live[flags[live] == 0]
            for name, q in case["queries"]:
                what = (distance, name, vname)
                wd, wp, wf, wn = real.merge(q, excluded, rank_sort_type=1)
                g = m.merge_query(cfg, q, excluded, sort_by_rank=False)
                assert len(wd) >= len(live) and np.all(np.isin(live, wd)), what      # the case must not pass on empty results
                assert np.array_equal(g[0], wd), (what, len(g[0]), len(wd), np.setxor1d(g[0], wd)[:8])
                assert np.array_equal(g[1].view(np.uint32), wp.view(np.uint32)), what
                assert np.array_equal(g[2], wf) and np.array_equal(g[3], wn), what
                assert_sorted_flavour(m, cfg, q, excluded, g, what)
    finally:
        real.close()
        m.close()
