"""The cases of tests/test_gpu_hnsw_stream_collect.py and the CPU side of their expectations: the graphs (the host builder over make_corpus,
labels row << 32 | 5), the bitmaps (default_rng(7).random(n) < share), and the rule of csrc/hnsw_stream_collect_plan.h restated in Python over
any session with .next(batch) — driven over the restated engine (OracleHnswStream) it is the expectation that does not depend on the
product's stream kernel.  tests/test_hnsw_stream_collect_cases.py proves on the CPU that every case is on the side (LDS / handover /
exhaustion / call count) it is there for."""
import numpy as np

from .conftest import make_corpus

LABEL_TAG = 5
A = dict(seed=61, n=3000, d=48, M=8, efc=100)       # everything stays in LDS
B = dict(seed=62, n=6000, d=32, M=16, efc=100)      # candidate_set passes kStreamLdsCand - maxM0 = 3040 in the middle of a collection
SMALL = dict(seed=63, n=200, d=16, M=8, efc=100)    # exhaustion inside a call
A_DELETED = 200
A_SHARES = (1, 0.5, 0.1, 0.02, 0.01, 0)
A_NEEDED = (1, 10, 150)
A_EF = (100, 16)
B_CASES = ((0.1, 150, 100), (0.02, 10, 100), (0.5, 150, 100), (1, 150, 100))   # (share, needed, ef = first_batch)
STREAM_LDS_CAND, STREAM_LDS_TOP = 3072, 1024
MAX_CALLS = 1000

_cache = {}


def labels_of(n):
    return (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(LABEL_TAG)


def deleted_labels(n, count):
    return labels_of(n)[np.random.default_rng(8).choice(n, count, replace=False)]


def graph(shape, metric, deleted=0):
    """the flat graph of the host builder (what GpuHnswMap builds over the same rows in the same order), made once and shared: read-only"""
    key = (shape["seed"], metric, deleted)
    if key not in _cache:
        from reindexer_amd import hostapi
        n, d = shape["n"], shape["d"]
        rows = make_corpus(shape["seed"], n, d)
        hg = hostapi.HnswGraph(metric, d, n, M=shape["M"], ef_construction=shape["efc"])
        hg.add(rows, labels_of(n))
        for lab in deleted_labels(n, deleted) if deleted else ():
            hg.mark_delete(lab)
        g = hg.export()
        hg.close()
        g["vectors"] = rows
        _cache[key] = g
    return _cache[key]


def query(orc, metric, d, seed=900):
    q = make_corpus(seed, 1, d)[0]
    return orc.normalize_copy(q)[0] if metric == 2 else q


def allowed_rows(n, share):
    return np.random.default_rng(7).random(n) < share


def words_of(allowed, extra_words=0, garbage=False):
    n = allowed.shape[0]
    w = np.zeros((n + 31) // 32 + extra_words, np.uint32)
    idx = np.nonzero(allowed)[0]
    np.bitwise_or.at(w, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    if garbage:   # bits at and above n
        if n & 31:
            w[n >> 5] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
        w[(n + 31) // 32:] = 0xFFFFFFFF
    return w


def next_batch(accepted, presented, needed):
    """StreamingKnnEstimator::EstimateBatchSize in Python's doubles (knn_streaming_estimator.h:26-38)"""
    remaining = 1 if accepted >= needed else needed - accepted
    return min(max(int(float(presented) / max(1, accepted) * remaining), 100), 800)


def run_rule(session, is_allowed, needed, first_batch, max_calls=MAX_CALLS, after_call=None):
    """The loop of StreamingKnnIndexIterator::Next over session.next(batch) -> (dist, ids, exhausted); is_allowed(ids) -> bool array.
    Returns dict(calls=[(batch, emitted, accepted so far)], per_call=[(dist, ids) accepted, in delivery order], per_call_seen=[per accepted
    row: the rows a consumer that walks the calls in order, each ascending by (dist, id), has been presented when it reaches the row],
    presented, accepted, exhausted)."""
    calls, per_call, per_call_seen = [], [], []
    presented = accepted = 0
    batch, exhausted = first_batch, False
    while True:
        dist, ids, exhausted = session.next(batch)
        ok = is_allowed(ids) if len(ids) else np.zeros(0, bool)
        rank = np.empty(len(ids), np.int64)
        rank[np.lexsort((ids, dist))] = np.arange(1, len(ids) + 1)
        per_call_seen.append(presented + rank[ok])
        presented += len(ids)
        accepted += int(np.count_nonzero(ok))
        calls.append((batch, len(ids), accepted))
        per_call.append((dist[ok], ids[ok]))
        if after_call is not None:
            after_call(session)
        if accepted >= needed or exhausted or len(calls) >= max_calls:
            break
        batch = next_batch(accepted, presented, needed)
    return dict(calls=calls, per_call=per_call, per_call_seen=per_call_seen, presented=presented, accepted=accepted, exhausted=exhausted)


def oracle_rule(orc, g, q, inv, allowed, needed, ef, first_batch, max_calls=MAX_CALLS, keep_session=False):
    """the rule over the restated engine; also the largest candidate_set / extras any of its calls met in front of a pop"""
    from oracle.pyoracle import OracleHnswStream
    row_of = {int(lab): i for i, lab in enumerate(g["labels"])}
    s = OracleHnswStream(orc, g, q, ef, inv)
    peaks = []
    out = run_rule(s, lambda labs: allowed[np.fromiter((row_of[int(x)] for x in labs), np.int64, len(labs))], needed, first_batch, max_calls,
                   after_call=lambda ses: peaks.append(ses.last_sizes()))
    out["peak_cand"] = max(p[3] for p in peaks)
    out["peak_ext"] = max(p[4] for p in peaks)
    out["start_sizes"] = [p[:3] for p in peaks]
    if keep_session:
        out["session"] = s
    else:
        s.close()
    return out


def best_first(per_call, needed):
    """each call's accepted rows ascending by (dist, id), calls concatenated, cut at needed"""
    ds, ls = [], []
    for dist, ids in per_call:
        order = np.lexsort((ids, dist))
        ds.append(np.asarray(dist, np.float32)[order])
        ls.append(np.asarray(ids)[order])
    d = np.concatenate(ds) if ds else np.zeros(0, np.float32)
    lab = np.concatenate(ls) if ls else np.zeros(0, np.uint64)
    return d[:needed], lab[:needed]


def presented_at_cut(run, needed):
    """StreamingKnnIndexIterator's presented_ when its consumer takes the needed-th accepted row; all that was presented if fewer passed"""
    seen = []
    for (dist, ids), sn in zip(run["per_call"], run["per_call_seen"]):
        seen.append(np.asarray(sn)[np.lexsort((ids, dist))])
    seen = np.concatenate(seen) if seen else np.zeros(0, np.int64)
    return int(seen[needed - 1]) if len(seen) >= needed else run["presented"]
