"""CPU: the cases of tests/ft_edge_cases.py are what they claim to be, BEFORE tests/test_gpu_ft_edges.py holds the kernels to them.

  * the geometry the case module states is the geometry of the kernels (the plan library's constants, and those that only the kernel
    sources carry): a changed constant fails here instead of silently moving the edges away from the cases;
  * every case places what it says: exact segment lengths per document range, planted documents in the sub-terms named, ascending
    unique documents inside the document table;
  * non-vacuity, from the RESTATED merger's output alone: with no limit in reach every planted document that is neither removed, excluded
    nor NOT-ed is merged and every removed or excluded document is absent; case D's limits preselect and cut where they say; case C's
    counts are the sparse train's kernel sizes and one past each;
  * where oracle/_ref/libref_ft.so is built: the restated merger equals the real ft::Merger on every case of A, B, D and E (documents in
    merge order, rank bits, fields, uint8 ranks) — "restated == real" at the edges and not only at total = 3000 — and the phrase cases
    match in exactly the planted documents."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle.pyoracle import FtOracle, ref_ft_or_none
from . import ft_edge_cases as ec

ROOT = Path(__file__).resolve().parent.parent
PLAN_LIB = ROOT / "tests" / "cpp" / "libft_merge_plan_cpu.so"
CSRC = ROOT / "reindexer_amd" / "csrc"


@pytest.fixture(scope="module")
def ft(oracle):
    return FtOracle(oracle)


def _real(nf):
    real = ref_ft_or_none(nf)
    if real is None:
        pytest.skip("oracle/_ref/libref_ft.so not available")
    return real


def _const(path, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*(\d+)", (CSRC / path).read_text())
    assert m, (path, name)
    return int(m.group(1))


def test_stated_geometry_is_the_kernels_geometry():
    if not PLAN_LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(PLAN_LIB))
    L.ft_plan_constants.argtypes = [C.c_void_p]
    c = np.zeros(9, np.uint32)
    L.ft_plan_constants(c.ctypes.data)
    block_postings, pass_items, range_docs, sparse_subs = (int(x) for x in c[:4])
    assert (range_docs, block_postings, sparse_subs) == (ec.R, ec.BLOCK_POSTINGS, ec.SPARSE_SUBS)
    assert block_postings == ec.STAGE_POSTINGS * pass_items
    # what the plan library does not carry, from the kernel sources
    assert _const("ft_ranges.hip", "kFtStageBlocks") == ec.STAGE_BLOCKS and ec.STAGE_BLOCKS * ec.STAGE_POSTINGS == ec.R
    assert _const("ft_ranges.hip", "kFtRangeSubs") == ec.RANGE_SUBS
    assert 1 << _const("rxgpu_internal.h", "kFtRangeShift") == ec.R
    assert 64 * _const("ft_sparse.hip", "kSpLoads") == ec.FLAT_POSTINGS
    assert _const("ft_merge_plan.h", "kFtRankTiles") == 2
    words = ec.R // ec.WORD_DOCS
    assert ec.LANE_WRAP == tuple(k * 64 * ec.WORD_DOCS for k in (1, 2, 3)) and words == 4 * 64   # four words a lane, 64 words apart
    assert 32768 in ec.TOTALS and 32768 // ec.WORD_DOCS == block_postings                        # one block of mask words
    assert ec.B_TOTAL == 3 * ec.R + 5


def _well_formed(case, store=None, total=None):
    total = case["total"] if total is None else total
    for s in case["store"] if store is None else store:
        d = s["doc"].astype(np.int64)
        assert d.shape[0] > 0 and d[0] >= 1 and d[-1] < total and np.all(np.diff(d) > 0), s["word"]
        assert s["pos_off"].shape[0] == d.shape[0] + 1 and s["pos_off"][0] == 0 and s["pos_off"][-1] == s["fpos"].shape[0]
        assert np.all(np.diff(s["pos_off"].astype(np.int64)) > 0)
        assert d.shape[0] <= 10_500


def test_planted_documents_sit_on_the_edges():
    assert ec.planted_docs(2).tolist() == [1]
    assert ec.planted_docs(33).tolist() == [1, 31, 32]
    p = set(ec.planted_docs(16385).tolist())
    assert {1, 31, 32, 33, 8191, 8192, 8193, 16383, 16384} <= p and 16385 not in p
    assert {2047, 2048, 4095, 4096, 6143, 6144, 8192 + 2047, 8192 + 2048, 8192 + 6143, 8192 + 6144} <= p
    assert 16384 not in set(ec.planted_docs(16384).tolist()) and 16383 in set(ec.planted_docs(16384).tolist())
    assert {32767, 32768} <= set(ec.planted_docs(32769).tolist())
    for total in ec.TOTALS:
        names = [v[0] for v in ec.flag_variants(total)]
        assert names == ["none", "none+exc", "around", "around+exc", "mirror", "mirror+exc"]
        for name, rem, exc in ec.flag_variants(total):
            if name == "around+exc":
                assert rem[total - 1] == 1
                for b in range(ec.R, total - 1, ec.R):
                    assert rem[b - 1] == 1 and rem[b] == 0 and exc[b] == 0 and (b + 1 >= total or exc[b + 1] == 1)
            if name == "mirror+exc":
                assert rem[total - 1] == 0 and exc[total - 1] == 0
                for b in range(ec.R, total, ec.R):
                    assert exc[b - 1] == 1 and rem[b] == 0 and exc[b] == 0 and (b + 1 >= total or rem[b + 1] == 1)


def _check_non_vacuous(ft, case, name, terms, total, words, avg, vname, removed, excluded, planted):
    cfg = ft.default_config(case["nf"], merge_limit=case["limit"])
    doc, proc, field, norm, pre = ft.merge_query(cfg, terms, total, words, avg, removed, excluded, sort_by_rank=False)
    assert not pre and doc.shape[0] < case["limit"], (name, vname)
    assert np.unique(doc).shape[0] == doc.shape[0] and (doc.shape[0] == 0 or (doc.min() >= 1 and doc.max() < total))
    want = ec.must_hold(terms, planted, removed, excluded)
    missing = np.setdiff1d(want, doc)
    assert missing.shape[0] == 0, (case["name"], name, vname, missing[:8])
    for flags in (removed, excluded):
        assert flags is None or not flags[doc].any(), (case["name"], name, vname)
    return doc, want


@pytest.mark.parametrize("total", ec.TOTALS)
def test_case_a_places_and_keeps_the_planted_documents(ft, total):
    case = ec.case_a(total)
    _well_formed(case)
    planted = case["planted"]
    assert np.array_equal(planted, ec.planted_docs(total))
    for s in case["store"][:-1]:
        assert np.all(np.isin(planted, s["doc"]))
    neg = case["store"][-1]
    assert np.array_equal(np.intersect1d(neg["doc"], planted), planted[::2])
    assert [[t["op"] for t in q] for _, q in case["queries"]] == [[1, 1], [2, 1], [1, 3, 1], [1], [2, 2]]
    assert [len(t["subs"]) for t in case["queries"][0][1]] == [2, 2] and len(case["queries"][3][1][0]["subs"]) == 3
    held = 0
    for vname, removed, excluded in case["variants"]:
        for name, terms in case["queries"]:
            _, want = _check_non_vacuous(ft, case, name, terms, total, case["words"], case["avg"], vname, removed, excluded, planted)
            held += want.shape[0]
            if name != "or_not_or" and vname == "none":
                assert np.array_equal(want, planted)       # all of them, the last document and both sides of every boundary included
            if name == "or_not_or":
                assert not np.isin(planted[::2], want).any()
    assert held > 0


def test_case_b_places_exact_posting_counts(ft):
    case = ec.case_b()
    _well_formed(case)
    nm = case["named"]
    assert case["total"] == ec.B_TOTAL and tuple(nm["cnt"]) == ec.COUNTS
    for n, s in nm["cnt"].items():
        assert [ec.seg_len(s, r) for r in range(4)] == [0, n, 0, 0]
        assert s["doc"][0] == ec.R and (n == 1 or s["doc"][-1] == 2 * ec.R - 1)     # the first and the last document of the range
    assert ec.seg_len(nm["cnt"][256], 1) + ec.seg_len(nm["c256b"], 1) == ec.FLAT_POSTINGS
    assert ec.seg_len(nm["cnt"][257], 1) + ec.seg_len(nm["c256b"], 1) == ec.FLAT_POSTINGS + 1
    assert not np.array_equal(nm["cnt"][256]["doc"], nm["c256b"]["doc"])
    assert ec.seg_len(nm["gmid"], 0) > 0 and [ec.seg_len(nm["gmid"], r) for r in (1, 2, 3)] == [0, 0, 0]
    for g in (nm["g0"], nm["g2"]):
        assert all(ec.seg_len(g, r) > 0 for r in range(4))
    assert np.array_equal(nm["full"]["doc"], np.arange(ec.R, 2 * ec.R)) and ec.seg_len(nm["full"], 1) == ec.STAGE_BLOCKS * ec.STAGE_POSTINGS
    assert ec.seg_len(nm["one"], 1) == 1 and nm["one"]["doc"].shape[0] == 1
    assert nm["e8191"]["doc"][-1] == ec.R - 1 and nm["e8192"]["doc"][-1] == ec.R and ec.seg_len(nm["e8192"], 1) == 1
    assert nm["elast"]["doc"].tolist() == [case["total"] - 1] and nm["e1"]["doc"].tolist() == [1]
    q = dict(case["queries"])
    assert [s["word"] for s in q["gap_subs"][0]["subs"]] == [nm["g0"]["word"], nm["gmid"]["word"], nm["g2"]["word"]]
    assert {s["word"] for t in q["early_terms"] for s in t["subs"]} == {nm[k]["word"] for k in ("e8191", "e8192", "elast", "e1")}
    # every document of the sub-terms (not only the planted ones) is accounted for: the range-1 words are planted there one by one
    every = np.unique(np.concatenate([s["doc"] for n, s in nm["cnt"].items()] + [case["planted"]]))
    for vname, removed, excluded in case["variants"]:
        for name, terms in case["queries"]:
            _check_non_vacuous(ft, case, name, terms, case["total"], case["words"], case["avg"], vname, removed, excluded, every)
    cfg = ft.default_config(case["nf"], merge_limit=case["limit"])
    full = ft.merge_query(cfg, q["full_subs"], case["total"], case["words"], case["avg"], None, None, sort_by_rank=False)
    assert np.array_equal(np.sort(full[0]), np.arange(ec.R, 2 * ec.R))
    ends = ft.merge_query(cfg, q["early_ends"], case["total"], case["words"], case["avg"], None, None, sort_by_rank=False)
    assert sorted(ends[0].tolist()) == [1, case["total"] - 1]


def test_case_c_counts_are_what_they_claim(ft):
    case = ec.case_c()
    _well_formed(case)
    assert case["total"] == 2 * ec.R + 1
    counts = [ec.n_live_subs(terms) for _, terms in case["queries"]]
    assert counts == list(ec.SUB_COUNTS) == [4, 5, 8, 9, 16, 17]
    assert [c <= ec.SPARSE_SUBS for c in counts] == [True] * 5 + [False]
    for name, terms in case["queries"]:
        assert len(terms) == 2 and all(t["op"] == ec.OR for t in terms)
        assert len({s["word"] for t in terms for s in t["subs"]}) == ec.n_live_subs(terms)
    for s in case["store"]:
        assert np.all(np.isin(case["planted"], s["doc"]))
    for vname, removed, excluded in case["variants"]:
        for name, terms in case["queries"]:
            _check_non_vacuous(ft, case, name, terms, case["total"], case["words"], case["avg"], vname, removed, excluded, case["planted"])


def test_case_d_limits_cut_on_the_boundary(ft):
    case = ec.case_d(ft)
    _well_formed(case)
    a, b = (s["doc"] for s in case["store"])
    for d in (ec.R - 1, ec.R, ec.R + 1):
        assert d in a and d not in b and d in case["ties"]
    assert [q[3:] for q in case["queries"]] == [(ec.R - 1, ec.R), (ec.R, ec.R + 1)]
    both = np.intersect1d(a, b)
    for name, terms, limit, last, dropped in case["queries"]:
        cfg = ft.default_config(case["nf"], merge_limit=limit)
        doc, proc, field, norm, pre = ft.merge_query(cfg, terms, case["total"], case["words"], case["avg"], None, None, sort_by_rank=False)
        assert pre is True and doc.shape[0] <= limit < a.shape[0] + b.shape[0]
        kept = np.intersect1d(doc, case["ties"])
        assert kept.max() == last and dropped not in doc
        assert np.array_equal(kept, case["ties"][: kept.shape[0]])      # a prefix of the ties, in document order
        assert np.all(np.isin(both, doc))                                 # every document above the threshold


def test_case_e_grows_across_the_boundaries(ft):
    case = ec.case_e()
    assert [s["total"] for s in case["steps"]] == [8000, ec.R + 1, 2 * ec.R + 1]
    assert case["steps"][1]["new"][0]["doc"].tolist() == [ec.R - 1, ec.R] and case["steps"][2]["new"][0]["doc"].tolist() == [2 * ec.R - 1, 2 * ec.R]
    up = []
    for step in case["steps"]:
        up += step["new"]
        _well_formed(case, up, step["total"])
        assert np.array_equal(step["words"], case["words"][: step["total"]])
        for name, terms in step["queries"]:
            assert all(any(s is u for u in up) for t in terms for s in t["subs"])
            doc, want = _check_non_vacuous(ft, case, name, terms, step["total"], step["words"], step["avg"], "none", None, None, step["planted"])
            if not any(t["op"] != ec.OR for t in terms):
                assert np.all(np.isin(np.concatenate([s["doc"] for t in terms for s in t["subs"]]), doc))
        if len(up) > 2:
            assert any(s is step["new"][0] for _, terms in step["queries"] for t in terms for s in t["subs"])
            assert any(s is up[0] for _, terms in step["queries"] for t in terms for s in t["subs"])


# ------------------------------------------------------------------------------------------------- the restated merger vs the real one
def _same_as_real(ft, real, case, total, words, avg, queries, variants, limit_of=None):
    n = 0
    for vname, removed, excluded in variants:
        real.set_docs(words, avg, removed)
        for q in queries:
            name, terms = q[0], q[1]
            cfg = ft.default_config(case["nf"], merge_limit=q[2] if len(q) > 2 else case["limit"])
            real.set_config(cfg)
            wd, wp, wf, wn = real.merge(ec.gpu_terms(terms), excluded, rank_sort_type=1)
            gd, gp, gf, gn, _ = ft.merge_query(cfg, terms, total, words, avg, removed, excluded, sort_by_rank=False)
            assert np.array_equal(gd.astype(np.int32), wd), (case["name"], name, vname, len(gd), len(wd))
            assert np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), (case["name"], name, vname)
            assert np.array_equal(gf, wf) and np.array_equal(gn, wn), (case["name"], name, vname)
            n += len(wd)
    return n


@pytest.mark.parametrize("total", ec.TOTALS)
def test_restated_merger_equals_real_merger_on_case_a(ft, total):
    case = ec.case_a(total)
    real = _real(case["nf"])
    real.set_docs(case["words"], case["avg"], None)
    for s in case["store"]:
        real.set_word_fpos(s["word"], s)
    assert _same_as_real(ft, real, case, total, case["words"], case["avg"], case["queries"], case["variants"]) > 0
    real.close()


@pytest.mark.parametrize("which", ["b", "d"])
def test_restated_merger_equals_real_merger_on_cases_b_and_d(ft, which):
    case = ec.case_b() if which == "b" else ec.case_d(ft)
    real = _real(case["nf"])
    real.set_docs(case["words"], case["avg"], None)
    for s in case["store"]:
        real.set_word_fpos(s["word"], s)
    assert _same_as_real(ft, real, case, case["total"], case["words"], case["avg"], case["queries"], case["variants"]) > 0
    real.close()


def test_restated_merger_equals_real_merger_on_case_e(ft):
    case = ec.case_e()
    real = _real(case["nf"])
    for step in case["steps"]:
        real.set_docs(step["words"], step["avg"], None)
        for s in step["new"]:
            real.set_word_fpos(s["word"], s)
        assert _same_as_real(ft, real, case, step["total"], step["words"], step["avg"], step["queries"], [("none", None, None)]) > 0
    real.close()


@pytest.mark.parametrize("distance", [1, 8])
def test_phrase_cases_match_in_exactly_the_planted_documents(ft, distance):
    """The real merger's answer to the phrase alone: every live planted document, none of the documents next to them."""
    case = ec.case_phrase(distance)
    _well_formed(case)
    real = _real(case["nf"])
    for s in case["store"]:
        real.set_word_fpos(s["word"], s)
    for vname, removed, excluded in case["variants"]:
        real.set_docs(case["words"], case["avg"], removed)
        real.set_config(ft.default_config(case["nf"], merge_limit=case["limit"]))
        live = case["planted"]
        for flags in (removed, excluded):
            if flags is not None:
                live = live[flags[live] == 0]
        doc = real.merge(case["queries"][0][1], excluded, rank_sort_type=1)[0]
        assert np.array_equal(np.intersect1d(doc, np.concatenate([case["planted"], case["near"]])), live), vname
        assert np.all(np.isin(doc, np.concatenate([case["planted"], case["hit"]])))
        both = real.merge(case["queries"][1][1], excluded, rank_sort_type=1)[0]
        assert np.all(np.isin(live, both)) and len(both) > len(doc)
    real.close()
