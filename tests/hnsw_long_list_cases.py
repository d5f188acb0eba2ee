"""The graphs of the long-list HNSW tests, and what each has to show — defined once, so that tests/test_hnsw_long_list_cases.py proves the
conditions on the CPU (over the restated engine) before tests/test_gpu_hnsw_long_lists.py lets a card see them.  Not a test module.

A level-0 list is 1 + maxM0 words and a wavefront reads 64 of them a pass, so a kernel takes a second pass over a list of 64 links or more
and a third over one of exactly 128.  selectNeighbors prunes far too hard for a built graph of a few thousand rows to hold such lists, so
they are constructed: every level-0 list of a graph holds the node's c nearest other rows and every level-1 list is filled, whence every
pop of every search reads lists of one known length.

classes   M = 64 (maxM0 = 128): c = 63 (the last word of pass 1), 64 (the first word of pass 2 alone), 65 (pass 2 partly filled),
                                127 (the last word of pass 2), 128 (pass 3 holds one word)
          M = 32 (maxM0 = 64):  c = 63, 64 (the full list of a graph whose maxM0 switches the team's look-ahead areas off)

Lists are in ascending order of distance, so the one word a last pass holds is the farthest link of the list, the one a search misses
least.  The "nearest last" form of a graph rotates every level-0 list by one: the nearest row moves to the last word, and a kernel that
drops that word loses the link every search needs most.
"""
import numpy as np

from .conftest import make_corpus

N = 3000
CLASSES = ((64, 63), (64, 64), (64, 65), (64, 127), (64, 128), (32, 63), (32, 64))   # (M, c)
PLANS = ((10, 128), (10, 10), (40, 64), (60, 250))   # (k, ef): those of tests/test_gpu_row_layout.py
DELETED = 300

_cache = {}


HANDOVER_N = 6000   # rows of the streaming graphs whose candidate set outgrows the LDS staging (3000 rows cannot: see handover_calls)
STREAM_LDS_CAND = 3072   # kStreamLdsCand: entries of candidate_set a streaming call stages in LDS


def labels_of(n=N):
    return (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(3)


def rows_of(d, n=N):
    key = ("rows", d, n)
    if key not in _cache:
        rows = make_corpus(600 + d, n, d)
        rows.setflags(write=False)
        _cache[key] = rows
    return _cache[key]


def nearest_ids(metric, rows, among=None, keep=128):
    """[len(among)][keep] ids: for every listed row its nearest other listed rows, ascending float64 distance, ties by id."""
    ids = np.arange(rows.shape[0]) if among is None else np.asarray(among, np.int64)
    x = rows[ids].astype(np.float64)
    dots = x @ x.T
    if metric == 0:
        sq = np.einsum("ij,ij->i", x, x)
        dist = sq[:, None] + sq[None, :] - 2.0 * dots
    elif metric == 1:
        dist = -dots
    else:
        nrm = np.sqrt(np.einsum("ij,ij->i", x, x))
        dist = -dots / (nrm[:, None] * nrm[None, :])
    np.fill_diagonal(dist, np.inf)
    keep = min(keep, ids.size - 1)
    order = np.argsort(dist, axis=1, kind="stable")[:, :keep]   # stable: among equal distances the smaller id first
    return ids[order].astype(np.uint32)


def _host_export(metric, M, d, n=N):
    """levels, upper lists, entry point and top level of the host builder over the rows (its level-0 lists are replaced)"""
    key = ("host", metric, M, d, n)
    if key not in _cache:
        from reindexer_amd import hostapi
        g = hostapi.HnswGraph(metric, d, n, M=M, ef_construction=100)
        g.add(rows_of(d, n), labels_of(n))
        e = g.export()
        g.close()
        assert e["n"] == n and e["M"] == M and e["maxM0"] == 2 * M
        level1 = np.flatnonzero(e["levels"] >= 1)
        near1 = nearest_ids(metric, rows_of(d, n), level1, keep=M)
        fill = near1.shape[1]
        assert fill == min(M, level1.size - 1) and fill >= 1
        upper = e["upper"].copy()
        at = e["upper_off"][level1].astype(np.int64)   # the block of level 1 is the first of a node's blocks
        upper[at, 0] = fill
        upper[at, 1:1 + fill] = near1
        upper[at, 1 + fill:] = 0
        e["upper"] = upper
        _cache[key] = (e, fill)
    return _cache[key]


def _nearest0(metric, d, n=N):
    key = ("near0", metric, d, n)
    if key not in _cache:
        _cache[key] = nearest_ids(metric, rows_of(d, n), keep=128)
    return _cache[key]


def full_graph(metric, M, d, c, deleted=0, nearest_last=False, n=N):
    """The flat graph (the rows as its vectors) in which every level-0 list holds the node's c nearest other rows and every level-1 list
    its min(M, level-1 nodes - 1) nearest other level-1 nodes; `deleted` delete marks drawn like those of tests/test_gpu_row_layout.py.
    nearest_last: the same lists rotated by one, the nearest row in the last word.  Made once per shape and shared: read-only."""
    key = ("graph", metric, M, d, c, deleted, bool(nearest_last), n)
    if key not in _cache:
        e, fill = _host_export(metric, M, d, n)
        max_m0 = 2 * M
        keep = min(c, max_m0)
        links0 = np.zeros((n, 1 + max_m0), np.uint32)
        links0[:, 0] = c
        links0[:, 1:1 + keep] = np.roll(_nearest0(metric, d, n)[:, :keep], -1 if nearest_last else 0, axis=1)
        flags = np.zeros(n, np.uint8)
        if deleted:
            flags[np.random.default_rng(d).choice(n, deleted, replace=False)] = 1
        g = dict(e, links0=links0, deleted=flags, num_deleted=int(deleted), vectors=rows_of(d, n), level1_fill=fill)
        for a in (links0, flags, g["upper"]):
            a.setflags(write=False)
        _cache[key] = g
    return _cache[key]


def queries_of(orc, metric, d):
    """the 12 queries of a shape, normalised for cosine"""
    q = make_corpus(700 + d, 12, d)
    if metric == 2:
        q = np.stack([orc.normalize_copy(v)[0] for v in q])
    return q


def inv_norms_of(orc, metric, d):
    key = ("inv", metric, d)
    if key not in _cache:
        _cache[key] = orc.l2_modules(rows_of(d)) if metric == 2 else None
    return _cache[key]


def wants_of(orc, metric, M, d, c, k, ef, deleted=0, nearest_last=False):
    """the restated engine's (dist, labels, distance evaluations, hops) of the 12 queries under one plan, computed once"""
    key = ("wants", metric, M, d, c, deleted, bool(nearest_last), k, ef)
    if key not in _cache:
        from oracle.pyoracle import oracle_hnsw_search_knn
        g = full_graph(metric, M, d, c, deleted, nearest_last)
        inv = inv_norms_of(orc, metric, d)
        _cache[key] = [oracle_hnsw_search_knn(orc, g, v, k, ef, inv, with_stats=True) for v in queries_of(orc, metric, d)]
    return _cache[key]


def check_structure(g, M, c):
    """every list of the graph has the length its class names: the count word, no self link, no link twice, ids in range"""
    max_m0, n = 2 * M, g["n"]
    assert g["M"] == M and g["maxM0"] == max_m0 and c <= max_m0 <= 128
    l0 = g["links0"]
    assert l0.shape == (n, 1 + max_m0) and (l0[:, 0] == c).all()
    body = l0[:, 1:1 + c].astype(np.int64)
    assert (body < n).all() and (body != np.arange(n)[:, None]).all()
    assert (np.diff(np.sort(body, axis=1), axis=1) > 0).all()
    assert (l0[:, 1 + c:] == 0).all()
    level1 = np.flatnonzero(g["levels"] >= 1)
    fill = g["level1_fill"]
    lists1 = g["upper"][g["upper_off"][level1].astype(np.int64)]
    assert fill == min(M, level1.size - 1) and (lists1[:, 0] == fill).all()
    assert np.isin(lists1[:, 1:1 + fill], level1).all() and (lists1[:, 1:1 + fill] != level1[:, None]).all()
    assert g["maxlevel"] >= 1 and g["levels"][g["entry"]] == g["maxlevel"]
    assert int(np.count_nonzero(g["deleted"])) == g["num_deleted"]


def check_conditions(orc, metric, M, d, c, deleted=0, nearest_last=False):
    """What the GPU cases of this graph rely on; a graph that misses one is changed, the condition is not.
    -> (fewest hops, most hops, fewest distance evaluations, most distance evaluations) over the plans and queries"""
    g = full_graph(metric, M, d, c, deleted, nearest_last)
    check_structure(g, M, c)
    if nearest_last:
        assert np.array_equal(g["links0"][:, c], _nearest0(metric, d)[:, 0]) and c >= 2
    live = g["labels"][g["deleted"] == 0]
    hops, evals = [], []
    for k, ef in PLANS:
        for i, (wd, wl, nd, nh) in enumerate(wants_of(orc, metric, M, d, c, k, ef, deleted, nearest_last)):
            what = (metric, M, d, c, deleted, nearest_last, k, ef, i)
            assert nh >= min(ef, 10), what + ("hops", nh)
            # level 0 starts with the entry point of the descent as the one visited node, and no list names its own node: the first hop
            # evaluates every one of the c links of that node's list
            assert nd >= c + 1, what + ("distance evaluations", nd)
            if c > 64:
                assert g["links0"][:, 0].min() > 64 and nd > 64, what
            assert wd.size == wl.size == k, what + ("results", wd.size)
            assert np.unique(wl).size == k and np.isin(wl, live).all(), what
            hops.append(nh)
            evals.append(nd)
    return min(hops), max(hops), min(evals), max(evals)


# ---------------------------------------------------------------------------------------------------------------- what the GPU tests run
# (metric, M, d, c, deleted[, nearest last]) of every graph tests/test_gpu_hnsw_long_lists.py attaches, by the test that does
FULL = ((64, 128), (32, 64))                      # c = maxM0 for both values of M
LAUNCHED = [(metric, M, d, c, 0) for metric in (0, 2) for d in (128, 768) for M, c in CLASSES]   # the fixed-dimension kernels, the team form
INNER_PRODUCT = [(1, 64, 128, 128, 0)]
OTHER_DIMS = [(metric, M, d, c, 0) for metric in (0, 2) for d in (100, 1024, 1536) for M, c in FULL]   # generic; wide chunks
AT_768 = [(metric, M, 768, c, 0) for metric in (0, 2) for M, c in FULL]   # heaps only; the global candidate heap; the team's gates
AT_768_DELETED = [(metric, M, 768, c, DELETED) for metric in (0, 2) for M, c in FULL]
MAILBOX = [(metric, 64, d, c, deleted) for metric in (0, 2) for d in (128, 768) for c in (64, 65, 128) for deleted in (0, DELETED)]
STREAMING = [(metric, 64, d, c, 0) for metric in (0, 2) for d in (48, 768) for c in (64, 65, 128)]
RANGE = [(metric, 64, d, c, 0) for metric in (0, 2) for d in (32, 768) for c in (64, 128)]
SQ8 = [(metric, 64, d, c, 0) for metric in (0, 2) for d in (128, 768) for c in (64, 128)]
# nearest last: the classes whose last pass holds one word (in a kernel that counts words: c = 64 and 128; in the streaming kernel, which
# counts links: c = 65), and the full lists
LAUNCHED_NEAREST_LAST = [(metric, M, d, c, 0, True) for metric in (0, 2) for d in (128, 768) for M, c in ((64, 64), (64, 65), (64, 128), (32, 64))]
AT_768_NEAREST_LAST = [(metric, M, 768, c, 0, True) for metric in (0, 2) for M, c in FULL]
MAILBOX_NEAREST_LAST = [(0, 64, d, c, 0, True) for d in (128, 768) for c in (64, 128)]
STREAMING_NEAREST_LAST = [(metric, 64, d, c, 0, True) for metric in (0, 2) for d in (48, 768) for c in (65, 128)]
RANGE_NEAREST_LAST = [(0, 64, d, c, 0, True) for d in (32, 768) for c in (64, 128)]
SHAPES = sorted(set(LAUNCHED + INNER_PRODUCT + OTHER_DIMS + AT_768 + AT_768_DELETED + MAILBOX + STREAMING + RANGE + SQ8 + LAUNCHED_NEAREST_LAST +
                    AT_768_NEAREST_LAST + MAILBOX_NEAREST_LAST + STREAMING_NEAREST_LAST + RANGE_NEAREST_LAST), key=lambda s: s + (False,) * (6 - len(s)))


def case_id(shape):
    metric, M, d, c, deleted = shape[:5]
    return f"metric{metric}-M{M}-d{d}-c{c}" + (f"-del{deleted}" if deleted else "") + ("-nearest_last" if len(shape) > 5 and shape[5] else "")


# ---------------------------------------------------------------------------------------------------------------- leaving the LDS staging
# A streaming call stages candidate_set in LDS while cand_n + maxM0 <= 3072 and, where a step would pass that, stops at the step's boundary
# and is resumed on the global heaps (kStreamNeedGlobal).  candidate_set holds what was evaluated and not yet popped, and at maxM0 = 128 the
# gate lies at 2944 entries: over 3000 rows the restated engine's set peaks near 2000 (c = 64) and 2300 (c = 128), over 6000 rows past 3600.
HANDOVER = [(0, 64, 48, c) for c in (64, 65, 128)]   # (metric, M, d, c) of the 6000-row graphs
HANDOVER_PLAN = (64, [64] * 60)                      # the deep session of tests/test_gpu_hnsw.py: 3840 results, so at least as many pops


def handover_query(orc, metric, d):
    q = make_corpus(905, 1, d)[0]
    return orc.normalize_copy(q)[0] if metric == 2 else q


def handover_calls(orc, metric, M, d, c):
    """The restated engine's session over the 6000-row graph under HANDOVER_PLAN: per call (dist, labels, exhausted, starts on the LDS
    heaps, handed over, (candidate set at the start, its peak in front of a pop, the peak of the extras)); handed over = the call starts with
    its heaps small enough for LDS and its candidate set passes 3072 - maxM0 entries in front of a pop."""
    key = ("handover", metric, M, d, c)
    if key not in _cache:
        from oracle.pyoracle import OracleHnswStream
        g = full_graph(metric, M, d, c, n=HANDOVER_N)
        ef, batches = HANDOVER_PLAN
        os_ = OracleHnswStream(orc, g, handover_query(orc, metric, d), ef, orc.l2_modules(g["vectors"]) if metric == 2 else None)
        gate, out = STREAM_LDS_CAND - g["maxM0"], []
        for b in batches:
            wd, wl, wex = os_.next(b)
            cand0, top0, ext0, cand_peak, ext_peak = os_.last_sizes()
            in_lds = max(ef, b) <= 1024 and top0 <= 1024 and ext0 <= 1024 and cand0 <= gate
            out.append((wd, wl, wex, in_lds, in_lds and (cand_peak > gate or ext_peak + 1 > 1024), (cand0, cand_peak, ext_peak)))
        os_.close()
        _cache[key] = out
    return _cache[key]
