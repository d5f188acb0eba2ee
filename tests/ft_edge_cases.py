"""The indexes and queries of the BM25 edge tests, and what each has to show — defined once, so that tests/test_ft_edge_cases.py proves the
conditions on the CPU (over the restated merger, and over the real ft::Merger where it is built) before tests/test_gpu_ft_edges.py lets a card
see them.  Not a test module.

The merge kernels are built around fixed geometry, and every other FT test draws its documents at random, nearly always below 3000:

    R = 8192            documents of one range (kFtRangeDocs): one workgroup of ft_ranges / ft_finish, one unit of the sparse train, the
                        granule of a word's range index (range_off) and of a shard cut
    32                  documents of one mask word; a range has 256 of them
    2048 / 4096 / 6144  in-range offsets at which a lane of the sparse train moves to its next mask word (four words a lane, 64 words apart)
    256                 postings of one staged block of ft_ranges; 32 blocks are staged (kFtStageBlocks), i.e. one full range, then the loop
    512                 postings of one flat pass of the sparse train (64 lanes x 8 loads)
    1024                postings of one block of the posting-side kernels (kFtBlockPostings); a rank workgroup takes two of them
    32768               documents = 1024 mask words = one block of ft_apply_blocks
    128                 sub-terms whose segments ft_ranges stages in LDS (kFtRangeSubs)
    16                  sub-terms of a sparse merge (kFtSparseSubs); 4-, 8- and 16-sub-term instantiations of its kernels

Here the documents are PLACED: on both sides of every one of these edges, with removed and excluded documents next to them.  A case is a dict

    nf, total, words, avg     the document table (words[0] is the empty document)
    store                     every word of the index: positions-format sub-terms (word, doc, pos_off, fpos, proc)
    planted                   the documents that were placed on purpose
    queries                   [(name, terms)]: terms as FtOracle.merge_query takes them, their sub-terms being entries of `store`
    variants                  [(name, removed, excluded)]: removed goes with the document table, excluded with the query
    limit                     mergeLimit (out of reach unless the case is about the cut)
"""
import functools

import numpy as np

from oracle.pyoracle import make_fpos
from .test_bm25_oracle import make_pos_postings

R = 8192
WORD_DOCS = 32
LANE_WRAP = (2048, 4096, 6144)
STAGE_POSTINGS, FLAT_POSTINGS, BLOCK_POSTINGS = 256, 512, 1024
STAGE_BLOCKS = 32
RANGE_SUBS = 128
SPARSE_SUBS = 16
OR, AND, NOT = 1, 2, 3

TOTALS = (2, 33, 8191, 8192, 8193, 16384, 16385, 32768, 32769)
COUNTS = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
B_TOTAL = 3 * R + 5
SUB_COUNTS = (4, 5, 8, 9, 16, 17)
PROCS = (100.0, 85.0, 70.5, 55.0)
NO_LIMIT = 20000


def planted_docs(total):
    """The documents next to every edge of the geometry, inside [1, total)."""
    p = {1, 31, 32, 33, total - 2, total - 1}
    for b in range(R, total, R):
        p |= {b - 1, b, b + 1}
    for r in range(0, total, R):
        for o in LANE_WRAP:
            p |= {r + o - 1, r + o}
    return np.array(sorted(d for d in p if 1 <= d < total), np.uint32)


def doc_table(seed, total, nf):
    rng = np.random.default_rng(seed)
    words = rng.integers(1, 6, (total, nf)).astype(np.float32)
    words[0] = 0
    return words, words[1:].mean(axis=0).astype(np.float32)


def sub_from_docs(rng, docs, nf, proc, word):
    """A positions-format sub-term over an EXPLICIT document list (positions as make_pos_postings draws them)."""
    docs = np.unique(np.asarray(docs, np.uint32))
    n = docs.shape[0]
    assert n > 0 and docs[0] >= 1
    s = make_pos_postings(rng, n + 1, nf, n, proc)   # n postings over the documents 1..n: only their positions are kept
    s["doc"] = docs
    s["word"] = word
    return s


def others(rng, total, avoid, k=300, lo=1, hi=None):
    """Up to k random documents of [lo, hi) that are not in `avoid` (at most half of what there is)."""
    pool = np.setdiff1d(np.arange(lo, total if hi is None else hi, dtype=np.uint32), avoid)
    return rng.choice(pool, min(k, pool.shape[0] // 2), replace=False).astype(np.uint32)


def term(op, subs, nf):
    assert all(a["proc"] >= b["proc"] for a, b in zip(subs, subs[1:]))   # SortSubterms order
    return dict(op=op, opts=dict(boost=1.0, term_len_boost=1.0, field_boost=[1.0] * nf, need_sum_rank=[0] * nf), subs=list(subs))


def gpu_terms(terms):
    return [dict(op=t["op"], opts=t["opts"], subs=[(s["word"], s["proc"]) for s in t["subs"]]) for t in terms]


def flag_variants(total, with_none_arrays=True):
    """No flags; around every range boundary b: b-1 removed, b+1 excluded, b untouched, total-1 removed; the mirror of that with total-1
    live.  Each once without an excluded list and once with it.  (Where total-1 is itself a boundary, 'total-1 removed' wins in the second
    form; the third keeps that boundary live.)"""
    def zeros():
        return np.zeros(total, np.uint8)
    rem_a, exc_a, rem_m, exc_m = zeros(), zeros(), zeros(), zeros()
    for b in range(R, total, R):
        rem_a[b - 1] = exc_m[b - 1] = 1
        if b + 1 < total:
            exc_a[b + 1] = rem_m[b + 1] = 1
    rem_a[total - 1] = 1
    out = [("none", None, None)]
    if with_none_arrays:
        out.append(("none+exc", zeros(), zeros()))
    out += [("around", rem_a, None), ("around+exc", rem_a, exc_a), ("mirror", rem_m, None), ("mirror+exc", rem_m, exc_m)]
    return out


def must_hold(terms, planted, removed, excluded):
    """The planted documents every merge of `terms` has to return when no limit is in reach: in every AND term, in no NOT term, in some
    merged term, and neither removed nor excluded."""
    def union(t):
        return np.unique(np.concatenate([s["doc"] for s in t["subs"]])) if t["subs"] else np.zeros(0, np.uint32)
    keep = np.zeros(0, np.uint32)
    for t in terms:
        if t["op"] != NOT:
            keep = np.union1d(keep, union(t))
    for t in terms:
        if t["op"] == AND:
            keep = np.intersect1d(keep, union(t))
        elif t["op"] == NOT:
            keep = np.setdiff1d(keep, union(t))
    keep = np.intersect1d(keep, planted)
    for flags in (removed, excluded):
        if flags is not None:
            keep = keep[flags[keep] == 0]
    return keep


def seg_len(s, rng_no):
    """Postings of the sub-term inside document range rng_no."""
    return int(np.count_nonzero(s["doc"] // R == rng_no))


def n_live_subs(terms):
    return sum(1 for t in terms for s in t["subs"] if len(s["doc"]))


def _freeze(case):
    for s in case["store"]:
        for k in ("doc", "pos_off", "fpos"):
            s[k].setflags(write=False)
    case["words"].setflags(write=False)
    return case


# --------------------------------------------------------------------------------------------------------------------------- A: totals
@functools.lru_cache(maxsize=None)
def case_a(total):
    nf = 2
    rng = np.random.default_rng(9000 + total)
    words, avg = doc_table(9100 + total, total, nf)
    planted = planted_docs(total)
    w = []
    for i, proc in enumerate((100.0, 85.0, 100.0, 70.5, 100.0, 85.0, 55.0)):
        w.append(sub_from_docs(rng, np.concatenate([planted, others(rng, total, planted)]), nf, proc, i))
    neg = sub_from_docs(rng, np.concatenate([planted[::2], others(rng, total, planted, 100)]), nf, 100.0, len(w))   # every second planted document
    queries = [
        ("or2_or2", [term(OR, w[0:2], nf), term(OR, w[2:4], nf)]),
        ("and_or", [term(AND, w[0:1], nf), term(OR, w[2:3], nf)]),
        ("or_not_or", [term(OR, w[0:1], nf), term(NOT, [neg], nf), term(OR, w[2:3], nf)]),
        ("simple3", [term(OR, w[4:7], nf)]),
        ("and_and", [term(AND, w[0:1], nf), term(AND, w[1:2], nf)]),
    ]
    return _freeze(dict(name=f"A{total}", nf=nf, total=total, words=words, avg=avg, store=w + [neg], planted=planted, queries=queries,
                        variants=flag_variants(total), limit=NO_LIMIT))


# ------------------------------------------------------------------------------------------------------------------- B: posting counts
def _range1_docs(rng, n):
    """n documents of range 1, its edges first: the first and last document of the range, the lane-wrap offsets, the first mask words."""
    pri = [R, 2 * R - 1, R + 1, 2 * R - 2] + [R + o + k for o in LANE_WRAP for k in (-1, 0)] + [R + 31, R + 32, R + 33]
    pri = np.array(pri[:n], np.uint32)
    rest = np.setdiff1d(np.arange(R, 2 * R, dtype=np.uint32), pri)
    return np.concatenate([pri, rng.choice(rest, n - pri.shape[0], replace=False)]) if n > pri.shape[0] else pri


@functools.lru_cache(maxsize=None)
def case_b():
    nf, total = 2, B_TOTAL
    rng = np.random.default_rng(9500)
    words, avg = doc_table(9501, total, nf)
    planted = planted_docs(total)
    store = []

    def add(docs, proc):
        store.append(sub_from_docs(rng, docs, nf, proc, len(store)))
        return store[-1]

    cnt = {n: add(_range1_docs(rng, n), 100.0) for n in COUNTS}
    c256b = add(_range1_docs(rng, 256), 85.0)
    spread = np.concatenate([planted, others(rng, total, planted)])
    g0 = add(spread, 100.0)
    gmid = add(np.concatenate([planted[planted < R], others(rng, total, planted, 100, hi=R)]), 85.0)   # nothing in range 1: an empty segment
    g2 = add(np.concatenate([planted, others(rng, total, planted)]), 70.5)                              # between two that are not
    full = add(np.arange(R, 2 * R, dtype=np.uint32), 100.0)                                            # 32 staged blocks ...
    one = add([R + 3808], 85.0)                                                                        # ... and a 33rd
    low = planted[planted < R - 1]
    e8191 = add(np.concatenate([low, others(rng, total, planted, hi=R - 1), [R - 1]]), 100.0)          # range index ends with range 0
    e8192 = add(np.concatenate([low, others(rng, total, planted, hi=R - 1), [R]]), 85.0)               # ... with one posting of range 1
    elast = add([total - 1], 70.5)
    e1 = add([1], 55.0)
    queries = []
    for n in COUNTS:
        queries.append((f"count{n}", [term(OR, [cnt[n]], nf)]))
        queries.append((f"count{n}_or", [term(OR, [cnt[n]], nf), term(OR, [cnt[257 if n != 257 else 256]], nf)]))
    queries += [
        ("pair512_terms", [term(OR, [cnt[256]], nf), term(OR, [c256b], nf)]),
        ("pair513_terms", [term(OR, [c256b], nf), term(OR, [cnt[257]], nf)]),
        ("pair512_subs", [term(OR, [cnt[256], c256b], nf)]),
        ("pair513_subs", [term(OR, [cnt[257], c256b], nf)]),
        ("gap_subs", [term(OR, [g0, gmid, g2], nf)]),
        ("gap_subs_or", [term(OR, [g0, gmid, g2], nf), term(OR, [cnt[255]], nf)]),
        ("gap_and", [term(AND, [g0, gmid, g2], nf), term(OR, [cnt[513]], nf)]),
        ("full_subs", [term(OR, [full, one], nf)]),
        ("full_terms", [term(OR, [full], nf), term(OR, [one], nf)]),
        ("full_and", [term(AND, [full], nf), term(OR, [one], nf), term(OR, [g0], nf)]),
        ("early_terms", [term(OR, [e8191, e8192], nf), term(OR, [elast, e1], nf)]),
        ("early_ends", [term(OR, [e1], nf), term(OR, [elast], nf)]),
        ("early_subs", [term(OR, [e8191, e8192, elast, e1], nf)]),
        ("early_and", [term(AND, [e8192], nf), term(OR, [elast], nf), term(OR, [g0], nf)]),
        ("early_not", [term(OR, [g0], nf), term(NOT, [e8191], nf), term(OR, [elast], nf)]),
    ]
    variants = [v for v in flag_variants(total, False) if v[0] in ("none", "around+exc")]
    named = dict(cnt=cnt, c256b=c256b, g0=g0, gmid=gmid, g2=g2, full=full, one=one, e8191=e8191, e8192=e8192, elast=elast, e1=e1)
    return _freeze(dict(name="B", nf=nf, total=total, words=words, avg=avg, store=store, planted=planted, queries=queries, variants=variants,
                        limit=NO_LIMIT, named=named))


# ------------------------------------------------------------------------------------------------------------------ C: sub-term counts
@functools.lru_cache(maxsize=None)
def case_c(total=2 * R + 1):
    """Two OR terms with 4, 5, 8, 9, 16 and 17 sub-terms in all: the sparse train's 4-, 8- and 16-sub-term kernels filled and one past,
    then one sub-term more than it holds bitmaps for."""
    nf = 2
    rng = np.random.default_rng(9700 + total)
    words, avg = doc_table(9701 + total, total, nf)
    planted = planted_docs(total)
    w = [sub_from_docs(rng, np.concatenate([planted, others(rng, total, planted, 200)]), nf, 100.0 - 2 * i, i) for i in range(max(SUB_COUNTS))]
    queries = []
    for k in SUB_COUNTS:
        h = (k + 1) // 2
        queries.append((f"subs{k}", [term(OR, w[:h], nf), term(OR, w[h:k], nf)]))
    variants = [v for v in flag_variants(total, False) if v[0] in ("none", "around+exc")]
    return _freeze(dict(name=f"C{total}", nf=nf, total=total, words=words, avg=avg, store=w, planted=planted, queries=queries, variants=variants,
                        limit=NO_LIMIT))


# ------------------------------------------------------------------------------------------------------ D: preselect cut on a boundary
_built = {}   # case D takes the restated merger as an argument, so it keeps its own cache


def case_d(ft):
    """One proc and one position for every posting, two OR terms: documents of both terms pre-score 2 p, documents of one term p.  8191, 8192
    and 8193 are documents of term 0 only.  A mergeLimit between the two counts makes p the threshold and keeps a prefix of its ties in
    document order; the two limits found here (by stepping the limit over the restated merger) end that prefix ON 8191 and ON 8192.
    Returns the case with queries = [(name, terms, limit, last kept tie, first dropped tie)]."""
    if "d" in _built:
        return _built["d"]
    nf, total = 1, 2 * R + 1
    rng = np.random.default_rng(9800)
    words = np.ones((total, nf), np.float32) * 5
    words[0] = 0
    avg = words[1:].mean(axis=0).astype(np.float32)
    edge = np.array([R - 1, R, R + 1], np.uint32)
    store = []
    for t in range(2):
        doc = rng.choice(np.setdiff1d(np.arange(1, total, dtype=np.uint32), edge), 6000, replace=False)
        doc = np.unique(np.concatenate([doc, edge])) if t == 0 else np.sort(doc)
        fp = make_fpos(rng.integers(0, 40, doc.shape[0]), np.zeros(doc.shape[0], np.int64)).astype(np.uint64)
        store.append(dict(word=t, doc=doc.astype(np.uint32), pos_off=np.arange(doc.shape[0] + 1, dtype=np.uint32), fpos=fp, proc=100.0))
    terms = [term(OR, [s], nf) for s in store]
    both = np.intersect1d(store[0]["doc"], store[1]["doc"])
    ties = np.setxor1d(store[0]["doc"], store[1]["doc"])
    queries = []
    for last in (R - 1, R):
        guess = both.shape[0] + int(np.searchsorted(ties, last)) + 1
        found = None
        for limit in range(guess - 3, guess + 4):
            cfg = ft.default_config(nf, merge_limit=limit)
            got = ft.merge_query(cfg, terms, total, words, avg, None, None, sort_by_rank=False)
            kept = np.intersect1d(got[0], ties)
            if got[4] and kept.shape[0] and kept.max() == last:
                found = limit
                break
        assert found is not None, (last, guess)
        queries.append((f"cut_after_{last}", terms, found, last, last + 1))
    _built["d"] = _freeze(dict(name="D", nf=nf, total=total, words=words, avg=avg, store=store, planted=edge, queries=queries, ties=ties,
                               variants=[("none", None, None)]))
    return _built["d"]


# ---------------------------------------------------------------------------------------------------------------------- E: grown index
@functools.lru_cache(maxsize=None)
def case_e():
    """An index that grows across a range boundary: set_docs with 8000 documents, again with 8193 and a word on 8191 and 8192, again with
    16385 and a word on 16383 and 16384.  The words of the earlier steps stay as they were uploaded: their range indexes end ranges before
    the grown index does.  steps = [dict(total, words, avg, new (sub-terms uploaded at this step), planted, queries)]."""
    nf = 2
    rng = np.random.default_rng(9900)
    base, _ = doc_table(9901, 2 * R + 1, nf)
    p0 = planted_docs(8000)
    w0 = sub_from_docs(rng, np.concatenate([p0, others(rng, 8000, p0)]), nf, 100.0, 0)
    w1 = sub_from_docs(rng, np.concatenate([p0, others(rng, 8000, p0)]), nf, 85.0, 1)
    w2 = sub_from_docs(rng, [R - 1, R], nf, 70.5, 2)
    w3 = sub_from_docs(rng, [2 * R - 1, 2 * R], nf, 55.0, 3)
    steps = []
    for total, new, queries in (
        (8000, [w0, w1], [("or_or", [term(OR, [w0], nf), term(OR, [w1], nf)]), ("simple", [term(OR, [w0, w1], nf)])]),
        (R + 1, [w2], [("old_or_new", [term(OR, [w0], nf), term(OR, [w2], nf)]), ("old2_or_new", [term(OR, [w0, w1], nf), term(OR, [w2], nf)]),
                       ("simple", [term(OR, [w0, w1, w2], nf)]), ("new_and_old", [term(AND, [w2], nf), term(OR, [w0], nf)])]),
        (2 * R + 1, [w3], [("three_terms", [term(OR, [w0], nf), term(OR, [w2], nf), term(OR, [w3], nf)]),
                           ("old2_or_new2", [term(OR, [w0, w1], nf), term(OR, [w2, w3], nf)]), ("simple", [term(OR, [w0, w1, w2, w3], nf)]),
                           ("old_not_new", [term(OR, [w0], nf), term(NOT, [w2], nf), term(OR, [w3], nf)])]),
    ):
        words = base[:total].copy()
        planted = np.unique(np.concatenate([p0] + [s["doc"] for s in (w2, w3)[:len(steps)]]))
        steps.append(dict(total=total, words=words, avg=words[1:].mean(axis=0).astype(np.float32), new=new, planted=planted, queries=queries))
    case = dict(name="E", nf=nf, total=2 * R + 1, words=base, avg=None, store=[w0, w1, w2, w3], steps=steps, limit=NO_LIMIT)
    return _freeze(case)


# -------------------------------------------------------------------------------------------------------------------------- phrases
@functools.lru_cache(maxsize=None)
def case_phrase(distance):
    """A two-term phrase at total 16385.  Both words stand in every planted document, `distance` apart in one field (the widest gap that
    still matches), and in the documents next to the planted ones distance + 1 apart, with a second occurrence at the matching place in
    the OTHER field: there the phrase must not match.  A few hundred other documents hold it or miss it at random."""
    nf, total = 2, 2 * R + 1
    rng = np.random.default_rng(9950 + distance)
    words, avg = doc_table(9951, total, nf)
    planted = planted_docs(total)
    near = np.setdiff1d(np.concatenate([planted - 1, planted + 1]), planted)
    near = near[(near >= 1) & (near < total)].astype(np.uint32)
    rest = others(rng, total, np.concatenate([planted, near]))
    hit = rest[: rest.shape[0] // 2]
    docs = np.unique(np.concatenate([planted, near, rest]))
    kind = np.where(np.isin(docs, planted), 0, np.where(np.isin(docs, near), 1, np.where(np.isin(docs, hit), 2, 3)))
    store = [dict(word=k, doc=docs, proc=100.0, pos_off=[0], fpos=[]) for k in range(2)]
    for d, k in zip(docs, kind):
        f, at = int(rng.integers(0, nf)), int(rng.integers(0, 20))
        gap = (distance, distance + 1, int(rng.integers(1, distance + 1)), distance + int(rng.integers(1, 6)))[k]
        second = [(f, at + gap)] + ([(1 - f, at + distance)] if k == 1 else [])
        for s, occ in zip(store, ([(f, at)], sorted(second))):
            s["fpos"].extend(int(make_fpos([p], [fl])[0]) for fl, p in occ)
            s["pos_off"].append(len(s["fpos"]))
    for s in store:
        s["pos_off"], s["fpos"] = np.array(s["pos_off"], np.uint32), np.array(s["fpos"], np.uint64)
    noise = sub_from_docs(rng, np.concatenate([planted[1::2], others(rng, total, planted)]), nf, 85.0, 2)
    store.append(noise)
    o = dict(boost=1.0, term_len_boost=1.0, field_boost=[1.0] * nf, need_sum_rank=[0] * nf)
    phrase = [dict(op=OR, opts=o, subs=[(k, 100.0)], phrase=0, distance=(1 if k == 0 else distance)) for k in range(2)]
    queries = [("phrase", phrase), ("phrase_or_term", phrase + [dict(op=OR, opts=o, subs=[(2, 85.0)], phrase=-1, distance=1)])]
    variants = [v for v in flag_variants(total, False) if v[0] in ("none", "around+exc", "mirror+exc")]
    return _freeze(dict(name=f"P{distance}", nf=nf, total=total, words=words, avg=avg, store=store, planted=planted, near=near, hit=hit,
                        queries=queries, variants=variants, limit=NO_LIMIT))
