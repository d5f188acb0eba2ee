"""The decisions of one BM25 merge (reindexer_amd/csrc/ft_merge_plan.h), compiled for the host (tests/cpp/ft_merge_plan_cpu.cc) and pinned on
the CPU: query parts, volume, the 2-phase gate's host half, the launch train, the row table, the engine limits and the three layouts.  Inputs
are hand-made; every expected value is worked out here from the rule as the reference states it (selecterimpl.h:482-572 for the parts and
totalORVids, merger.h:239-267 and mergerimpl.h:486-490 for the gate, mergerimpl.h:110-112 / 509-514 for the qp numbering)."""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

LIB = Path(__file__).resolve().parent / "cpp" / "libft_merge_plan_cpu.so"
PARAMS, LOGIC, NOTFOUND, OVERFLOW = -3, -4, -7, -8
OR, AND, NOT = 1, 2, 3
NF = 2
SIZES = (96, 120, 24, 640, 16)   # subterm, term_cfg, syn_job, plan, record: any sizes do, the layouts are functions of them
CAP_ROWS = 70000
P = C.c_void_p

SCALARS = ["nparts", "total_vids", "max_merged", "empty", "any_phrase", "sparse", "est_or", "est_and", "prescore", "query_len", "n_subs", "n_terms",
           "n_grid", "merge_blocks", "merged_postings", "n_rows", "n_part_qp", "n_syns", "n_jobs", "n_job_syns", "sp_empty_and", "nwords", "n_ranges",
           "cfg_floats", "plan_bytes", "state_bytes", "clean_bytes", "out_header", "out_doc", "out_proc", "out_terms_counter", "out_field", "out_bytes",
           "area_hdr_bytes", "area_bytes"]
STATE = ["plan_subs", "plan_terms", "plan_mgrid", "plan_fc", "plan_syns", "plan_jobs", "plan_jsyn", "plan_self", "mask", "synmask", "score", "brec", "boff",
         "adders", "eidx", "efield", "tdoc", "tpos", "tidx"]
CLEAN = ["hist", "lb_pre", "bcnt", "sync", "dbg", "lb_units", "erank"]
ROW = ["term", "src", "row", "attr", "qp", "prev_term_qp", "ord_in_term", "suppressed", "phrase"]


class In(C.Structure):
    _fields_ = [("nterms", C.c_uint32), ("num_fields", C.c_uint32), ("ops", P), ("phrase_num", P), ("sub_off", P), ("boost", P), ("term_len_boost", P),
                ("field_boost", P), ("need_sum", P), ("nsyn", C.c_uint32), ("first_term", C.c_uint32), ("syn_term_off", P), ("part_syn_off", P),
                ("part_syn", P), ("suppressed", P), ("sub_n", P), ("sub_df", P), ("sub_last_doc", P), ("sub_found", P), ("sub_has_pos", P), ("procs", P),
                ("merge_limit", C.c_uint32), ("bm25_type", C.c_int32), ("k1", C.c_double), ("b", C.c_double), ("ratio", C.c_double), ("field_cfg", P),
                ("h_avg", P), ("n_avg", C.c_uint32), ("sh_total", C.c_uint32), ("total_docs", C.c_uint64), ("train_mode", C.c_int32), ("simple", C.c_int32),
                ("resident", C.c_int32), ("have_outs", C.c_int32), ("max_areas", C.c_uint32), ("pad", C.c_uint32), ("cap", C.c_uint64),
                ("phrase_admitted", P), ("phrase_row_off", P), ("phrase_row_n", P), ("sizes", C.c_uint64 * 5)]


class Out(C.Structure):
    _fields_ = [("code", C.c_int32), ("msg", C.c_char * 252), ("scalars", P), ("parts", P), ("term_postings", P), ("rows", P), ("terms", P), ("grid", P),
                ("syns", P), ("jobs", P), ("job_syns", P), ("regions", P), ("cap_rows", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    L = C.CDLL(str(LIB))
    L.ft_merge_plan_cpu.restype = C.c_int
    L.ft_merge_plan_cpu.argtypes = [C.POINTER(In), C.POINTER(Out)]
    L.ft_classify_cpu.argtypes = [C.c_uint32, P, P, P]
    L.ft_out_layout_cpu.argtypes = [C.c_uint64, P]
    L.ft_plan_constants.argtypes = [P]
    return L


def W(n, proc=100.0, df=None, last=10, found=True, pos=True):
    """One sub-term as the dictionary holds its word."""
    return SimpleNamespace(n=n, df=n if df is None else df, last=last, found=found, pos=pos, proc=proc)


def T(op, subs, phrase=-1, boost=1.0, tlb=1.0, fb=(1.0, 1.0), ns=(0, 0)):
    return SimpleNamespace(op=op, subs=subs, phrase=phrase, boost=boost, tlb=tlb, fb=fb, ns=ns)


def plan(L, terms, N=1000, limit=20000, syn=None, mode=-1, simple=False, resident=False, areas=0, sh_total=0, phrases=None, bm25_type=0, k1=2.0, b=0.75,
         ratio=0.0, field_cfg=None, h_avg=(5.0, 7.0), cap=1 << 40, have_outs=True, null_opts=False, suppressed=None):
    """syn = (first_term, syn_term_off, part_syn_off, part_syn); phrases = {part: (admitted, [documents per row])}"""
    keep = []

    def arr(values, dtype):
        a = np.ascontiguousarray(values, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    subs = [w for t in terms for w in t.subs]
    i = In()
    i.nterms, i.num_fields = len(terms), NF
    i.ops = arr([t.op for t in terms], np.int32)
    i.phrase_num = arr([t.phrase for t in terms], np.int32)
    i.sub_off = arr(np.cumsum([0] + [len(t.subs) for t in terms]), np.uint32)
    i.boost = arr([t.boost for t in terms], np.float32)
    i.term_len_boost = arr([t.tlb for t in terms], np.float32)
    i.field_boost = None if null_opts else arr([t.fb for t in terms], np.float32)
    i.need_sum = arr([t.ns for t in terms], np.uint8)
    if syn:
        i.first_term, sto, pso, ps = syn
        i.nsyn = len(sto) - 1
        i.syn_term_off, i.part_syn_off, i.part_syn = arr(sto, np.uint32), arr(pso, np.uint32), arr(ps + [0], np.uint32)
        i.suppressed = arr(suppressed if suppressed is not None else [0] * len(subs), np.uint8)
    i.sub_n = arr([w.n for w in subs] + [0], np.uint64)
    i.sub_df = arr([w.df for w in subs] + [0], np.uint64)
    i.sub_last_doc = arr([w.last for w in subs] + [0], np.uint32)
    i.sub_found = arr([w.found for w in subs] + [0], np.uint8)
    i.sub_has_pos = arr([w.pos for w in subs] + [0], np.uint8)
    i.procs = arr([w.proc for w in subs] + [0], np.float32)
    i.merge_limit, i.bm25_type, i.k1, i.b, i.ratio = limit, bm25_type, k1, b, ratio
    i.field_cfg = arr(field_cfg if field_cfg is not None else [[1.0] * NF, [0.1] * NF, [1.0] * NF, [0.3] * NF, [1.0] * NF, [0.1] * NF], np.float64)
    i.h_avg, i.n_avg = arr(h_avg, np.float32), len(h_avg)
    i.sh_total, i.total_docs, i.train_mode = sh_total, N, mode
    i.simple, i.resident, i.have_outs, i.max_areas, i.cap = int(simple), int(resident), int(have_outs), areas, cap
    if phrases is not None:
        nparts = 1 + max(phrases)
        rows = [phrases.get(p, (0, []))[1] for p in range(nparts)]
        i.phrase_admitted = arr([phrases.get(p, (0, []))[0] for p in range(nparts)], np.uint64)
        i.phrase_row_off = arr(np.cumsum([0] + [len(r) for r in rows]), np.uint32)
        i.phrase_row_n = arr([n for r in rows for n in r] + [0], np.uint64)
    i.sizes = (C.c_uint64 * 5)(*SIZES)
    o = Out()
    buf = dict(scalars=np.full(len(SCALARS) + 1, 0xDEAD, np.uint64), parts=np.zeros((64, 3), np.uint32), term_postings=np.zeros(64, np.uint64),
               rows=np.zeros((CAP_ROWS, 9), np.uint32), terms=np.zeros((CAP_ROWS, 6), np.uint32), grid=np.zeros((CAP_ROWS, 2), np.uint32),
               syns=np.zeros((64, 4), np.uint32), jobs=np.zeros((64, 3), np.uint32), job_syns=np.zeros(64, np.uint32),
               regions=np.zeros((len(STATE) + len(CLEAN), 2), np.uint64))
    for k, a in buf.items():
        setattr(o, k, a.ctypes.data)
    o.cap_rows = CAP_ROWS
    code = L.ft_merge_plan_cpu(C.byref(i), C.byref(o))
    r = SimpleNamespace(code=code, msg=o.msg.decode())
    if code:
        return r
    assert buf["scalars"][-1] == 0xDEAD   # the shim wrote exactly the scalars named here
    for name, v in zip(SCALARS, buf["scalars"]):
        setattr(r, name, int(v))
    r.parts = [tuple(int(x) for x in p) for p in buf["parts"][:r.nparts]]
    r.term_postings = [int(x) for x in buf["term_postings"][:len(terms)]]
    if r.empty:
        return r
    r.rows = [SimpleNamespace(**dict(zip(ROW, (int(x) for x in row)))) for row in buf["rows"][:min(r.n_subs, CAP_ROWS)]]
    r.terms = [tuple(int(x) for x in t) for t in buf["terms"][:r.n_terms]]
    r.grid = [tuple(int(x) for x in g) for g in buf["grid"][:min(r.n_grid, CAP_ROWS)]]
    r.syns = [tuple(int(x) for x in s) for s in buf["syns"][:r.n_syns]]
    r.jobs = [tuple(int(x) for x in j) for j in buf["jobs"][:r.n_jobs]]
    r.job_syns = [int(x) for x in buf["job_syns"][:r.n_job_syns]]
    r.state = {name: (int(a), int(b)) for name, (a, b) in zip(STATE, buf["regions"])}
    r.clean = {name: (int(a), int(b)) for name, (a, b) in zip(CLEAN, buf["regions"][len(STATE):])}
    return r


def a256(v):
    return (v + 255) // 256 * 256


def test_constants_shared_with_the_kernels(lib):
    c = np.zeros(9, np.uint32)
    lib.ft_plan_constants(c.ctypes.data)
    # kFtBlockPostings, kFtPassItems, kFtRangeDocs, kFtSparseSubs, kFtHistCopies, kFtHistStride, kFtSyncWords, kFtBatchMax, ft_pass_blocks(1025)
    assert list(c) == [1024, 4, 8192, 16, 8, 65536 + 1024, 16, 64, 2]


# ------------------------------------------------------------------------------------------------------------------------------ parts
def test_parts_group_consecutive_equal_phrase_numbers(lib):
    terms = [T(OR, [W(5)], phrase=p) for p in (-1, 4, 4, -1, 7)]
    r = plan(lib, terms, phrases={1: (3, [3]), 3: (2, [2])})
    assert r.parts == [(0, 0, 1), (1, 1, 3), (0, 3, 4), (1, 4, 5)]
    assert r.any_phrase and r.query_len == 5   # QueryLength() counts the terms inside phrases one by one


def test_adjacent_phrases_with_different_numbers_stay_two_parts(lib):
    terms = [T(OR, [W(5)], phrase=p) for p in (2, 2, 3, 3)]
    r = plan(lib, terms, phrases={0: (1, [1]), 1: (1, [1])})
    assert r.parts == [(1, 0, 2), (1, 2, 4)]


@pytest.mark.parametrize("ops,phr,want", [
    ([], [], (0, 1, 0)),                       # no terms: Empty()
    ([NOT], [-1], (1, 1, 0)),                  # a single NOT part: Empty()
    ([OR], [-1], (1, 0, 1)),                   # one plain term: Simple()
    ([AND], [-1], (1, 0, 1)),
    ([OR, OR], [5, 5], (1, 0, 0)),             # one phrase: one part, not Simple()
    ([NOT, NOT], [5, 5], (1, 1, 0)),           # Op() of a phrase is its first term's
    ([OR, OR], [-1, -1], (2, 0, 0)),
    ([OR, OR, OR, OR, OR], [-1, 4, 4, -1, 7], (4, 0, 0)),
])
def test_empty_and_simple_classification(lib, ops, phr, want):
    out = np.zeros(3, np.uint32)
    o, p = np.array(ops + [0], np.int32), np.array(phr + [0], np.int32)
    lib.ft_classify_cpu(len(ops), o.ctypes.data, p.ctypes.data, out.ctypes.data)
    assert tuple(out) == want


# ------------------------------------------------------------------------------------------------------------------------------ volume
def test_max_merged_is_the_smaller_of_limit_and_total_vids(lib):
    terms = [T(OR, [W(30), W(12, proc=90)]), T(NOT, [W(8)])]   # totalORVids counts every term, whatever its operator
    r = plan(lib, terms, limit=20000)
    assert r.term_postings == [42, 8] and r.total_vids == 50 and r.max_merged == 50 and not r.empty
    assert plan(lib, terms, limit=49).max_merged == 49


def test_document_frequency_not_fragment_length_counts(lib):   # a document-range shard: limits are facts of the whole index
    r = plan(lib, [T(OR, [W(3, df=40)]), T(OR, [W(0, df=7)])], sh_total=2)
    assert r.term_postings == [40, 7] and r.max_merged == 47


def test_merge_limit_zero_and_all_empty_words_are_empty(lib):
    terms = [T(OR, [W(30)]), T(OR, [W(8)])]
    assert plan(lib, terms, limit=0).empty
    assert plan(lib, [T(OR, [W(0)]), T(AND, [W(0), W(0)])]).empty


def test_output_room_is_checked_against_max_merged(lib):
    terms = [T(OR, [W(30)]), T(OR, [W(8)])]
    assert plan(lib, terms, cap=38).code == 0
    r = plan(lib, terms, cap=37)
    assert (r.code, r.msg) == (OVERFLOW, "plan: output buffers too small")
    assert plan(lib, terms, have_outs=False).code == OVERFLOW
    assert plan(lib, terms, cap=0, have_outs=False, resident=True).code == 0   # a resident merge has no lists


# ------------------------------------------------------------------------------------------------------------------------------ the gate
def test_gate_or_sums_and_compares_with_the_limit(lib):
    below = plan(lib, [T(OR, [W(50)]), T(OR, [W(30), W(20)])], limit=100)
    assert (below.est_or, below.prescore) == (100, 0)          # 100 > 100 is false
    above = plan(lib, [T(OR, [W(50)]), T(OR, [W(30), W(21)])], limit=100)
    assert (above.est_or, above.prescore) == (101, 1)


def test_gate_and_takes_the_minimum(lib):
    r = plan(lib, [T(OR, [W(500)]), T(AND, [W(90)]), T(AND, [W(300)])], limit=100)
    assert (r.est_or, r.est_and, r.prescore) == (500, 90, 0)   # min(500, 90) = 90 <= 100
    r = plan(lib, [T(OR, [W(500)]), T(AND, [W(101)]), T(AND, [W(300)])], limit=100)
    assert (r.est_and, r.prescore) == (101, 1)


def test_gate_skips_not_parts(lib):
    r = plan(lib, [T(OR, [W(60)]), T(NOT, [W(900)])], limit=100)
    assert (r.est_or, r.est_and, r.prescore) == (60, 2 ** 64 - 1, 0)


def test_gate_never_fires_when_the_index_is_not_above_the_limit(lib):
    terms = [T(OR, [W(90)]), T(OR, [W(90)])]
    assert plan(lib, terms, N=100, limit=100, ).prescore == 0   # est 180, but min(est, N) = 100 and N > limit is false
    assert plan(lib, terms, N=101, limit=100).prescore == 1


def test_gate_never_fires_for_a_simple_query(lib):
    assert plan(lib, [T(OR, [W(400)])], limit=100, simple=True).prescore == 0
    assert plan(lib, [T(OR, [W(400)]), T(OR, [W(1)])], limit=100).prescore == 1


def test_gate_counts_a_phrase_by_its_admitted_documents(lib):
    terms = [T(OR, [W(400)], phrase=1), T(OR, [W(400)], phrase=1), T(OR, [W(10)])]
    assert plan(lib, terms, limit=100, phrases={0: (80, [80])}).est_or == 90
    assert plan(lib, terms, limit=100, phrases={0: (95, [95])}).prescore == 1


def test_gate_adds_the_first_term_of_every_synonym_of_the_part(lib):
    # parts: t0 (AND), t1 (OR); synonym 0 = terms 2, 3 (of part 0), synonym 1 = term 4 (of part 1)
    terms = [T(AND, [W(40)]), T(OR, [W(30)]), T(OR, [W(25)]), T(OR, [W(900)]), T(OR, [W(7)])]
    r = plan(lib, terms, limit=100, syn=(2, [0, 2, 3], [0, 1, 2], [0, 1]))
    assert (r.est_and, r.est_or) == (40 + 25, 30 + 7)   # the second term of synonym 0 does not count


# ------------------------------------------------------------------------------------------------------------------------------ the train
def test_density_boundary(lib):
    # sparse iff local_postings * 10 <= N * 3
    assert plan(lib, [T(OR, [W(302)])], N=1007, simple=True).sparse == 1   # 3020 = 3021 - 1
    assert plan(lib, [T(OR, [W(301)])], N=1003, simple=True).sparse == 0   # 3010 = 3009 + 1
    assert plan(lib, [T(OR, [W(300)])], N=1000, simple=True).sparse == 1   # equal
    # the postings on this handle decide, not the document frequency
    assert plan(lib, [T(OR, [W(10, df=900)])], N=1000, simple=True).sparse == 1


def test_train_mode_overrides(lib):
    dense_q, sparse_q = [T(OR, [W(900)])], [T(OR, [W(10)])]
    assert plan(lib, sparse_q, simple=True, mode=0).sparse == 0
    assert plan(lib, dense_q, simple=True, mode=1).sparse == 1
    assert plan(lib, dense_q, simple=True, mode=-1).sparse == 0


ELIGIBLE = dict(terms=[T(OR, [W(10)]), T(AND, [W(10)])], mode=1)


def test_eligible_baseline(lib):
    assert plan(lib, **ELIGIBLE).sparse == 1
    # a NOT term's options are not looked at
    assert plan(lib, [T(OR, [W(10)]), T(NOT, [W(10)], fb=(1.0, 3.0), boost=0.0)], mode=1).sparse == 1


def cfg_with(row, field, value):
    fc = [[1.0] * NF, [0.1] * NF, [1.0] * NF, [0.3] * NF, [1.0] * NF, [0.1] * NF]
    fc[row][field] = value
    return fc


@pytest.mark.parametrize("change", [
    dict(terms=[T(OR, [W(10)], phrase=1), T(OR, [W(10)], phrase=1), T(OR, [W(10)])], phrases={0: (5, [5])}),   # a phrase
    dict(terms=[T(OR, [W(10)]), T(OR, [W(10)]), T(OR, [W(10)])], syn=(2, [0, 1], [0, 1, 1], [0])),              # a multi-word synonym
    dict(areas=4),
    dict(sh_total=2),
    dict(terms=[T(OR, [W(1, proc=100 - i) for i in range(9)]), T(OR, [W(1, proc=100 - i) for i in range(8)])]),   # 17 sub-terms
    dict(bm25_type=1),                                                                                           # classic BM25
    dict(terms=[T(OR, [W(10)], fb=(1.0, 2.0)), T(AND, [W(10)])]),                                                # unequal field boosts
    dict(field_cfg=cfg_with(1, 1, 0.9995)),                                                                      # a weight above 0.999
    dict(terms=[T(OR, [W(10, proc=float("inf"))]), T(AND, [W(10)])]),                                            # a non-finite proc
    dict(terms=[T(OR, [W(10, proc=1e-20)], boost=1e-12), T(AND, [W(10)])]),                                      # the product below 1e-30
    dict(h_avg=(5.0, 0.0)),
    dict(h_avg=(5.0,)),
    dict(k1=-1.0),
    dict(terms=[T(OR, [W(10)], boost=0.0), T(AND, [W(10)])]),
])
def test_each_reason_against_the_sparse_train(lib, change):
    assert plan(lib, **{**ELIGIBLE, **change}).sparse == 0


def test_sixteen_sub_terms_are_still_eligible(lib):
    terms = [T(OR, [W(1, proc=100 - i) for i in range(8)]), T(OR, [W(1, proc=100 - i) for i in range(8)])]
    assert plan(lib, terms, mode=1).sparse == 1
    # words without postings anywhere do not count
    terms[1].subs.append(W(0, proc=1))
    assert plan(lib, terms, mode=1).sparse == 1


def test_sparse_attribute_words(lib):
    # proc16 = uint16(proc * field_boost[0] * boost), capped at 65535 / 4; bit 16 first sub-term of its term, 17 AND, 18 NOT; row << 20
    terms = [T(OR, [W(10, proc=80.0), W(5, proc=70.5)], boost=2.0), T(AND, []), T(NOT, [W(4, proc=50.0)], fb=(3.0, 9.0))]
    r = plan(lib, terms, mode=1)
    assert r.sparse and r.sp_empty_and == 1   # an AND term without postings empties the mask
    assert [x.attr for x in r.rows] == [160 | 1 << 16, 141 | 1 << 20, 150 | 1 << 16 | 1 << 18]
    assert plan(lib, [T(OR, [W(10, proc=30000.0)])], simple=True, mode=1).rows[0].attr == 16383 | 1 << 16


# ------------------------------------------------------------------------------------------------------------------------------ the rows
def test_qp_skips_not_terms_and_not_sub_terms_take_no_row(lib):
    terms = [T(OR, [W(2000), W(30, proc=90)]), T(NOT, [W(9)]), T(AND, [W(1025)])]
    r = plan(lib, terms)
    assert [(x.term, x.src, x.qp, x.row, x.ord_in_term) for x in r.rows] == [(0, 0, 1, 0, 0), (0, 1, 1, 1, 1), (1, 2, 0, 0, 0), (2, 3, 2, 2, 0)]
    assert r.n_rows == 3 and r.n_part_qp == 2 and r.query_len == 3
    # block_base is the running sum of ft_pass_blocks (1024 postings a block) over the merged rows: 2, 1, then 2 blocks
    assert r.grid == [(0, 0), (2, 1), (3, 3)] and r.merge_blocks == 5 and r.merged_postings == 2000 + 30 + 1025
    assert [t[:3] for t in r.terms] == [(0, 2, OR), (2, 3, NOT), (3, 4, AND)]


def test_a_word_without_postings_is_dropped_but_keeps_its_place_in_the_term(lib):
    r = plan(lib, [T(OR, [W(5), W(0, proc=95), W(7, proc=90)]), T(OR, [W(1)])])
    assert [(x.src, x.ord_in_term, x.row) for x in r.rows] == [(0, 0, 0), (2, 2, 1), (3, 0, 2)]
    # a shard keeps the row of a word whose postings lie on other shards (df > 0, n == 0): rows are numbered alike on every shard
    r = plan(lib, [T(OR, [W(5), W(0, proc=95, df=3), W(7, proc=90)]), T(OR, [W(1)])], sh_total=2)
    assert [(x.src, x.row) for x in r.rows] == [(0, 0), (1, 1), (2, 2), (3, 3)] and [g[0] for g in r.grid] == [0, 1, 1, 2]


def test_phrase_rows_carry_the_last_plain_terms_qp(lib):
    terms = [T(OR, [W(9)]), T(NOT, [W(9)]), T(AND, [W(9)]), T(OR, [W(9)], phrase=3), T(OR, [W(9)], phrase=3), T(OR, [W(9)])]
    r = plan(lib, terms, phrases={3: (6, [4, 0, 2])})
    ph = [x for x in r.rows if x.phrase]
    assert [(x.term, x.src, x.qp, x.prev_term_qp, x.ord_in_term, x.row) for x in ph] == [(3, 0, 3, 2, 0, 2), (3, 1, 3, 2, 1, 3), (3, 2, 3, 2, 2, 4)]
    assert [x.prev_term_qp for x in r.rows if not x.phrase] == [0, 0, 0, 0]
    assert r.rows[-1].qp == 4 and r.n_part_qp == 4 and r.terms[3] == (3, 6, OR, 1, 1, 1)
    assert r.merged_postings == 9 + 9 + 4 + 0 + 2 + 9   # the rows' documents, not the phrase's words


def test_a_not_phrase_takes_no_qp_and_no_rows_of_the_grid(lib):
    terms = [T(OR, [W(9)]), T(NOT, [W(9)], phrase=1), T(NOT, [W(9)], phrase=1)]
    r = plan(lib, terms, phrases={1: (5, [5])})
    assert [(x.qp, x.row, x.phrase) for x in r.rows] == [(1, 0, 0), (0, 0, 1)] and r.n_rows == 1 and r.n_part_qp == 1


def test_synonym_terms_all_take_a_qp(lib):
    # parts t0 (AND), t1 (OR); synonym 0 = t2, t3 (NOT) of part 0; synonym 1 = t4 of part 1
    terms = [T(AND, [W(40)]), T(OR, [W(30)]), T(OR, [W(25), W(3, proc=50)]), T(NOT, [W(6)]), T(OR, [W(7)])]
    r = plan(lib, terms, syn=(2, [0, 2, 3], [0, 1, 2], [0, 1]), suppressed=[0, 0, 0, 1, 0, 0])
    assert r.n_part_qp == 2
    assert [(x.term, x.qp, x.row, x.suppressed) for x in r.rows] == [(0, 1, 0, 0), (1, 2, 1, 0), (2, 3, 2, 0), (2, 3, 3, 1), (3, 0, 0, 0), (4, 5, 4, 0)]
    assert r.syns == [(2, 4, 4, 2), (4, 5, 5, 1)]               # term_begin, term_end, end_qp, nterms
    assert [t[2] for t in r.terms] == [AND, OR, OR, OR, OR]      # a synonym's term is scored like an OR term
    assert r.jobs == [(0, 0, 1)] and r.job_syns == [0]           # only the AND part's mask takes its synonyms' masks in


def test_same_boost_and_all_positive_flags(lib):
    r = plan(lib, [T(OR, [W(1)], fb=(2.0, 2.0)), T(OR, [W(1)], fb=(2.0, 0.0)), T(OR, [W(1)], fb=(1.0, 3.0))])
    assert [t[3:5] for t in r.terms] == [(1, 1), (0, 0), (0, 1)]


# ------------------------------------------------------------------------------------------------------------------------------ limits
def test_65535_merged_rows_are_refused(lib):
    def q(last):
        return [T(OR, [W(1, proc=1.0)] * 4096) for _ in range(15)] + [T(OR, [W(1, proc=1.0)] * last)]
    ok = plan(lib, q(4094))
    assert ok.code == 0 and ok.n_rows == 65534
    r = plan(lib, q(4095))
    assert (r.code, r.msg) == (PARAMS, "plan: more than 65534 merged sub-terms in one query (GPU engine limit)")


def test_posting_limits(lib):
    r = plan(lib, [T(OR, [W(5, df=2 ** 31)]), T(OR, [W(5, df=2 ** 31 - 1)])])
    assert (r.code, r.msg) == (PARAMS, "plan: more than 2^32 postings in one merge")
    assert plan(lib, [T(OR, [W(5, df=2 ** 31)]), T(OR, [W(5, df=2 ** 31 - 2)])]).code == 0
    # every list is padded to whole blocks of 1024 postings: 4 x 2^30 padded, 2^32 - 4 unpadded
    r = plan(lib, [T(OR, [W(2 ** 30 - 1)]) for _ in range(4)], N=20000)
    assert (r.code, r.msg) == (PARAMS, "plan: more than 2^32 (padded) postings in one merge")


def test_sub_terms_must_be_sorted_by_proc(lib):
    r = plan(lib, [T(OR, [W(5, proc=50.0), W(5, proc=50.5)]), T(OR, [W(1)])])
    assert (r.code, r.msg) == (PARAMS, "plan: sub-terms must be sorted by proc, descending (SortSubterms)")
    assert plan(lib, [T(OR, [W(5, proc=50.0), W(5, proc=50.0)]), T(OR, [W(1)])]).code == 0


def test_a_list_reaching_past_the_documents_is_refused(lib):
    r = plan(lib, [T(OR, [W(5, last=64)])], N=64, simple=True)
    assert (r.code, r.msg) == (PARAMS, "plan: a posting list holds a document id >= total_docs (rxgpu_ft_set_docs)")
    assert plan(lib, [T(OR, [W(5, last=63)])], N=64, simple=True).code == 0
    assert plan(lib, [T(OR, [W(0, last=64, df=3)])], N=64, simple=True, sh_total=2).code == 0   # an empty fragment has no last document


def test_other_refusals_keep_their_codes_and_order(lib):
    two = [T(OR, [W(5)]), T(OR, [W(5)])]
    assert plan(lib, two, bm25_type=3).msg == "plan: bm25_type must be 0 (rx), 1 (classic) or 2 (wordCount)"
    r = plan(lib, [T(OR, [W(5, found=False, last=10 ** 6)]), T(OR, [W(5)])])
    assert (r.code, r.msg) == (NOTFOUND, "plan: unknown word id")   # before the same word's range check
    r = plan(lib, [T(OR, [W(5, last=10 ** 6)]), T(OR, [W(5, found=False)])])
    assert r.code == PARAMS                                         # sub-term by sub-term
    r = plan(lib, two, simple=True)
    assert (r.code, r.msg) == (LOGIC, "plan: a phrase is not a Simple() query")
    r = plan(lib, [T(OR, [W(5, pos=False)]), T(OR, [W(5)])])
    assert (r.code, r.msg) == (LOGIC, "plan: the word was uploaded without positions (rxgpu_ft_set_word_positions)")
    assert plan(lib, [T(OR, [W(5, pos=False)])], simple=True).code == 0   # mergeSimple reads no positions
    assert plan(lib, two, null_opts=True, mode=0).msg == "plan: null term options"
    assert plan(lib, [T(OR, [W(5)], ns=(1, 1)), T(OR, [W(5)])]).code == 0
    r = plan(lib, [T(OR, [W(1, proc=1.0)] * 4097), T(OR, [W(5)])])
    assert (r.code, r.msg) == (PARAMS, "plan: more than 4096 sub-terms in one term (GPU engine limit)")
    r = plan(lib, two, areas=4, resident=True)
    assert (r.code, r.msg) == (LOGIC, "plan: areas are built for queries of plain terms (no multi-word synonyms, no resident form)")
    r = plan(lib, [T(OR, [W(5)], phrase=1), T(OR, [W(5)], phrase=1), T(OR, [W(5)])], areas=4, phrases={0: (1, [1])})
    assert (r.code, r.msg) == (LOGIC, "plan: a phrase's areas stay on the CPU merger")
    r = plan(lib, [T(OR, [W(1)]), T(OR, [W(1)]), T(OR, [W(1)])], syn=(2, [0, 2], [0, 1, 1], [0]))
    assert (r.code, r.msg) == (PARAMS, "plan: inconsistent synonym tables")
    r = plan(lib, [T(OR, [W(1)]), T(OR, [W(1)]), T(OR, [W(1)])], syn=(2, [0, 1], [0, 1, 1], [1]))
    assert (r.code, r.msg) == (PARAMS, "plan: synonym id out of range")


# ------------------------------------------------------------------------------------------------------------------------------ layouts
def check_layout(regions, total):
    at = 0
    for name, (off, size) in regions.items():
        assert off % 256 == 0, name
        assert off >= at, name   # in order, no overlap
        at = off + size
    assert at <= total and total % 256 == 0


def test_dense_layout(lib):
    terms = [T(OR, [W(2000), W(30, proc=90)]), T(NOT, [W(9)]), T(AND, [W(1025)])]
    r = plan(lib, terms, N=20000, limit=100, mode=0)   # (left to itself the plan takes the sparse train: 3064 postings on 20000 documents)
    assert r.prescore and not r.sparse and r.max_merged == 100 and r.n_rows == 3 and r.n_ranges == 3 and r.nwords == 625
    check_layout(r.state, r.state_bytes)
    check_layout(r.clean, r.clean_bytes)
    assert r.plan_bytes % 256 == 0 and r.plan_bytes == r.state["mask"][0] and r.state["plan_subs"][0] == 0
    sub, tcfg, job, pl, rec = SIZES
    assert r.cfg_floats == 6 * NF + 3 * NF
    want = dict(plan_subs=4 * sub, plan_terms=3 * tcfg, plan_mgrid=3 * 8, plan_fc=r.cfg_floats * 4 + 3 * NF, plan_syns=16, plan_jobs=job, plan_jsyn=4,
                plan_self=pl, mask=625 * 4, synmask=0, score=625 * 32 * 2, brec=(2000 + 30 + 1025) * rec, boff=3 * 4, adders=3 * 3 * 4, eidx=3 * 100 * 4,
                efield=3 * 100, tdoc=0, tpos=0, tidx=0)
    assert {k: v[1] for k, v in r.state.items()} == want
    assert {k: v[1] for k, v in r.clean.items()} == dict(hist=8 * (65536 + 1024) * 4, lb_pre=8, bcnt=12, sync=64, dbg=512, lb_units=24, erank=3 * 100 * 4)
    assert list(r.clean)[-1] == "erank" and r.clean["erank"][0] == max(off for off, _ in r.clean.values())
    # the regions in front of erank depend on the corpus only: a query with more rows leaves them where they are
    more = plan(lib, terms + [T(OR, [W(3)])], N=20000, limit=100, mode=0)
    assert {k: v for k, v in more.clean.items() if k != "erank"} == {k: v for k, v in r.clean.items() if k != "erank"}
    assert plan(lib, terms, N=20000, limit=5000, mode=0).state["score"][1] == 0   # no pre-scores without the gate


def test_sparse_layout(lib):
    r = plan(lib, [T(OR, [W(20), W(3, proc=90)]), T(AND, [W(10)])], N=20000, limit=5, mode=1)   # min(OR 23, AND 10) > 5
    assert r.sparse and r.prescore and r.max_merged == 5
    check_layout(r.state, r.state_bytes)
    check_layout(r.clean, r.clean_bytes)
    sizes = {k: v[1] for k, v in r.state.items()}
    assert [sizes[k] for k in ("mask", "score", "brec", "eidx", "efield")] == [0] * 5 and r.clean["erank"][1] == 0
    assert (sizes["tdoc"], sizes["tpos"], sizes["tidx"]) == (5 * 4, 5 * 4, 5 * 3 * 4)
    dense = plan(lib, [T(OR, [W(20), W(3, proc=90)]), T(AND, [W(10)])], N=20000, limit=5, mode=0)
    assert [dense.state[k][1] for k in ("tdoc", "tpos", "tidx")] == [0, 0, 0]


def test_synonym_masks_in_the_layout(lib):
    terms = [T(AND, [W(40)]), T(OR, [W(30)]), T(OR, [W(25)])]
    r = plan(lib, terms, N=6400, syn=(2, [0, 1], [0, 1, 1], [0]))
    check_layout(r.state, r.state_bytes)
    assert r.state["synmask"][1] == 1 * 200 * 4 and r.state["plan_syns"][1] == 16 and r.state["plan_jsyn"][1] == 4


@pytest.mark.parametrize("M", [1, 63, 1000])
def test_packed_result_layout_is_the_closed_form(lib, M):
    out = np.zeros(6, np.uint64)
    lib.ft_out_layout_cpu(M, out.ctypes.data)
    doc = a256(16)
    proc = doc + a256(M * 4)
    tc = proc + a256(M * 4)
    field = tc + a256(M * 2)
    assert [int(x) for x in out] == [0, doc, proc, tc, field, field + a256(M)]


def test_plan_carries_the_packed_layout_and_the_areas_sizes(lib):
    r = plan(lib, [T(OR, [W(40)]), T(OR, [W(23)])], areas=5)
    assert r.max_merged == 63
    assert (r.out_doc, r.out_proc, r.out_terms_counter, r.out_field, r.out_bytes) == (256, 512, 768, 1024, 1280)
    assert r.area_hdr_bytes == a256(63 * NF * 2 * 4) and r.area_bytes == 63 * NF * 5 * 3 * 4
    assert plan(lib, [T(OR, [W(40)]), T(OR, [W(23)])]).area_bytes == 0


# ------------------------------------------------------------------------------------------------------------------------------ the dense train's launches
LDS_LARGE, LDS_FEW = 48 * 1024, 32 * 1024   # ft_finish: document table + key list / the compact layout
LAUNCH = ["syn_grid", "ranges_grid", "apply_blocks", "rank_blocks", "adders_grid", "bases_grid", "finish_grid", "finish_lds"]


def Q(n_rows, max_merged=100, merge_blocks=1, simple=0, prescore=0, n_ranges=2, range_count=0, nwords=282, n_syn_jobs=0):
    """One host plan as the nine facts ft_train_launch reads (9000 documents: two ranges, 282 mask words)."""
    return (n_rows, max_merged, merge_blocks, simple, prescore, n_ranges, range_count, nwords, n_syn_jobs)


def train(L, plans, phase=-1):
    facts = np.ascontiguousarray(plans, dtype=np.uint64).reshape(-1, 9)
    out = np.full(9, 0xDEAD, np.uint64)
    L.ft_train_launch_cpu.argtypes = [P, C.c_uint32, C.c_int32, P]
    L.ft_train_launch_cpu(facts.ctypes.data, len(plans), phase, out.ctypes.data)
    assert out[8] == 0xDEAD
    return dict(zip(LAUNCH, (int(x) for x in out)))


def launches(syn=0, ranges=0, apply=0, rank=0, adders=0, bases=0, finish=0, lds=0):
    return dict(zip(LAUNCH, (syn, ranges, apply, rank, adders, bases, finish, lds)))


def test_train_constants(lib):
    c = np.zeros(7, np.uint32)
    lib.ft_train_constants.argtypes = [P]
    lib.ft_train_constants(c.ctypes.data)
    # kFtApplyWords, kFtRankTiles, kFtFinishRows, kFtBitmapRows, kFtSparseRecords, kFtSparsePostings, kFtSparseHeads
    assert list(c) == [4, 2, 16, 8, 768, 6, 512]


def test_train_of_a_simple_query(lib):
    # ft_ranges (mask only), ft_rank_all over ceil(3 / 2) workgroups of two tiles, ft_adders, ft_finish in the compact layout
    assert train(lib, [Q(1, merge_blocks=3, simple=1)]) == launches(ranges=2, rank=2, adders=2, finish=2, lds=LDS_FEW)
    # (the gate never holds for a Simple() query: the flag alone launches nothing)
    assert train(lib, [Q(1, merge_blocks=3, simple=1, prescore=1)])["apply_blocks"] == 0
    assert train(lib, []) == launches()


def test_train_of_a_two_term_query_with_pre_score(lib):
    q = Q(2, max_merged=20000, merge_blocks=5, prescore=1, n_ranges=3, nwords=625)
    assert train(lib, [q]) == launches(ranges=3, apply=1, rank=3, adders=3, finish=3, lds=LDS_FEW)
    assert train(lib, [Q(2, max_merged=20000, merge_blocks=5, n_ranges=3, nwords=625)])["apply_blocks"] == 0
    # a query without merged postings (every term a NOT): ft_rank_all is not launched
    assert train(lib, [Q(0, merge_blocks=0)])["rank_blocks"] == 0


@pytest.mark.parametrize("rows,bases,lds", [(8, 0, LDS_FEW), (9, 0, LDS_LARGE), (16, 0, LDS_LARGE), (17, 1, LDS_LARGE)])
def test_train_by_the_number_of_rows(lib, rows, bases, lds):
    # up to 8 rows the bitmaps; up to 16 rows (and 8192 entries) ft_finish sums its own bases
    assert train(lib, [Q(rows, merge_blocks=rows)]) == launches(ranges=2, rank=(rows + 1) // 2, adders=2, bases=bases, finish=2, lds=lds)


def test_train_by_the_size_of_the_table(lib):
    def q(rows, ranges):
        return Q(rows, n_ranges=ranges, nwords=ranges * 256)
    assert train(lib, [q(3, 2730)])["bases_grid"] == 0      # 8190 entries
    assert train(lib, [q(3, 2731)])["bases_grid"] == 1      # 8193
    assert train(lib, [q(16, 512)])["bases_grid"] == 0      # 8192 exactly
    assert train(lib, [q(16, 513)])["bases_grid"] == 1
    assert train(lib, [q(3, 2731)])["finish_lds"] == LDS_FEW   # the layout is a matter of rows and mergeLimit only


def test_train_by_merge_limit(lib):
    # 16-bit slots hold 0 .. 65534 and 0xFFFF for "never merged"
    assert train(lib, [Q(2, max_merged=65534)])["finish_lds"] == LDS_FEW
    assert train(lib, [Q(2, max_merged=65535)])["finish_lds"] == LDS_LARGE


def test_train_of_a_document_range_shard_phase_by_phase(lib):
    # 80000 documents: 10 ranges, 2500 mask words; this shard holds 5 ranges = 1280 words = two workgroups of ft_preselect_apply (the whole
    # index would take three)
    q = Q(2, max_merged=20000, merge_blocks=4, prescore=1, n_ranges=10, range_count=5, nwords=2500)
    assert train(lib, [q], 0) == launches(ranges=5)
    assert train(lib, [q], 1) == launches(apply=2, rank=2, adders=5)
    assert train(lib, [q], 2) == launches(finish=5, lds=LDS_FEW)
    assert train(lib, [q], -1) == launches(ranges=5, apply=2, rank=2, adders=5, finish=5, lds=LDS_FEW)
    whole = Q(2, max_merged=20000, merge_blocks=4, prescore=1, n_ranges=10, nwords=2500)
    assert train(lib, [whole], 1) == launches(apply=3, rank=2, adders=10)
    many = Q(17, max_merged=20000, merge_blocks=17, n_ranges=10, range_count=5, nwords=2500)
    assert train(lib, [many], 2) == launches(bases=1, finish=5, lds=LDS_LARGE)
    assert train(lib, [many], 1)["bases_grid"] == 0


def test_train_with_synonym_masks(lib):
    q = Q(3, merge_blocks=3, n_syn_jobs=1)
    assert train(lib, [q]) == launches(syn=2, ranges=2, rank=2, adders=2, finish=2, lds=LDS_FEW)
    assert train(lib, [q], 0) == launches(syn=2, ranges=2)
    assert train(lib, [q], 1)["syn_grid"] == 0


def test_train_of_a_mixed_batch_takes_the_large_layout_and_the_widest_grid(lib):
    two, nine = Q(2, merge_blocks=2), Q(9, merge_blocks=12, prescore=1)
    assert train(lib, [two, two]) == launches(ranges=2, rank=1, adders=2, finish=2, lds=LDS_FEW)
    for batch in ([two, nine], [nine, two]):
        assert train(lib, batch) == launches(ranges=2, apply=1, rank=6, adders=2, finish=2, lds=LDS_LARGE)
    assert train(lib, [two, Q(17, merge_blocks=17)])["bases_grid"] == 1


@pytest.mark.parametrize("nwords,blocks", [(1023, 1), (1024, 1), (1025, 2)])
def test_apply_blocks_size_the_grid_and_the_look_back_chain(lib, nwords, blocks):
    # 256 threads x 4 mask words per workgroup of ft_preselect_apply; one 8-byte look-back word per workgroup
    lib.ft_apply_blocks_cpu.restype, lib.ft_apply_blocks_cpu.argtypes = C.c_uint64, [C.c_uint64]
    assert lib.ft_apply_blocks_cpu(nwords) == blocks
    ranges = (nwords * 32 + 8191) // 8192
    assert train(lib, [Q(2, prescore=1, n_ranges=ranges, nwords=nwords)])["apply_blocks"] == blocks
    r = plan(lib, [T(OR, [W(50)]), T(OR, [W(60)])], N=nwords * 32, limit=100, mode=0)
    assert r.nwords == nwords and r.prescore and r.clean["lb_pre"][1] == blocks * 8


def test_train_of_a_planned_query(lib):
    terms = [T(OR, [W(2000), W(30, proc=90)]), T(NOT, [W(9)]), T(AND, [W(1025)])]
    r = plan(lib, terms, N=20000, limit=100, mode=0)
    q = Q(r.n_rows, r.max_merged, r.merge_blocks, 0, r.prescore, r.n_ranges, 0, r.nwords, r.n_jobs)
    assert train(lib, [q]) == launches(ranges=3, apply=1, rank=3, adders=3, finish=3, lds=LDS_FEW)   # 5 blocks of postings: 3 workgroups


def test_finish_lds_layouts(lib):
    v = np.zeros(14, np.uint32)
    lib.ft_finish_lds_cpu.argtypes = [P]
    lib.ft_finish_lds_cpu(v.ctypes.data)
    tab, keys, words, slot, bits, pref, words_few, table_large, table_few, sparse_large, sparse_few, sp_head, sp_todo, sp_words = (int(x) for x in v)
    # sorted layout: 8192 halves of document table, 8192 keys; compact: 8192 halves of slots, 8 x 256 bitmap words, 8 x 256 prefixes
    assert (tab, keys, words) == (0, 4096, 12288) and words * 4 == LDS_LARGE
    assert (slot, bits, pref, words_few) == (0, 4096, 6144, 8192) and words_few * 4 == LDS_FEW
    # the table of ft_adders (up to 8192 entries): over the key list / from the start of the compact block
    assert (table_large, table_few) == (4096, 0) and table_large + 8192 <= words and table_few + 8192 <= words_few
    # sparse bucket: 768 records of four words, 512 heads, 768 halves; behind the slots (compact) / behind 768 slots of the key list (sorted)
    assert (sp_head, sp_todo, sp_words) == (3072, 3584, 3968)
    assert sparse_few == bits and sparse_few + sp_words <= words_few
    assert sparse_large >= keys + 768 and sparse_large + sp_words <= words
