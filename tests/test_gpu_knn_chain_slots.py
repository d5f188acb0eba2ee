"""-m gpu: the launch sequence of every brute-force KNN chain (rxgpu_knn_chains.hip), as the profile slots show it.

One index of 3 000 x 256 random normal rows per metric (256 lies inside the int8 tier's 128 < D <= 1024 and is a multiple of 64; no ties, so
no gate opens), kk = 10.  After ONE search_knn (or search_knn_subset over 500 ascending rows) with profiling freshly enabled, every slot a
chain can file is read and compared with the table below; slots not listed are 0.  The pruned chains of a single query also record what they
nominated (rxgpu_index_last_candidates): the capacity is pinned and count <= cap says the pruned chain answered, not the exact scan behind
its gate.  Whatever the chain, distances (as bits) and rows equal those of the f32 scan of the same queries, one at a time."""
import numpy as np
import pytest

from .conftest import make_corpus

pytestmark = pytest.mark.gpu

N, D, KK, N_IDS = 3_000, 256, 10, 500
SLOTS = ("scan", "merge", "scan_subset", "scan_bf16", "scan_i8", "scan_i8_subset", "filter_approx", "rescore", "fallback_scan", "gemm_sample", "gemm")
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_BATCH_BF16_MIN")
BATCHED = dict(gemm_sample=1, gemm=1, rescore=1, fallback_scan=1)
# name: (queries, over the row list?, environment, slots that are not 0, capacity of the candidate list or None: nothing is recorded)
CASES = {
    "one-f32": (1, False, dict(RXGPU_SCAN_BF16=0), dict(scan=1, merge=1), None),
    "one-bf16": (1, False, dict(RXGPU_SCAN_BF16=1), dict(scan_bf16=1, filter_approx=1, rescore=1, fallback_scan=1), 3008),
    "one-i8": (1, False, dict(RXGPU_SCAN_I8=1), dict(scan_i8=1, filter_approx=1, rescore=1, fallback_scan=1), 3008),
    "four": (4, False, {}, BATCHED, None),
    "four-f32-nomination": (4, False, dict(RXGPU_BATCH_BF16_MIN=0), BATCHED, None),
    "three-hundred": (300, False, {}, {k: 2 for k in BATCHED}, None),   # chunks of 256 and 44 queries
    "list-f32": (1, True, {}, dict(scan_subset=1, merge=1), None),
    "list-i8": (1, True, dict(RXGPU_SCAN_I8=1), dict(scan_i8_subset=1, filter_approx=1, rescore=1), 512),   # "fallback_scan" counts opened gates here
}


def _env(mp, env):
    for name in ENV:
        mp.delenv(name, raising=False)
    for k, v in env.items():
        mp.setenv(k, str(v))


@pytest.fixture(scope="module", params=[1, 0, 2], ids=["ip", "l2", "cosine"])
def chains(request, rxgpu, oracle):
    """(index, queries, row list, the f32 scan's answer to every query, the f32 subset scan's answer to the first)"""
    metric = request.param
    rows = make_corpus(700 + metric, N, D)
    inv = oracle.l2_modules(rows) if metric == 2 else None
    q = make_corpus(800 + metric, 300, D)
    if metric == 2:
        q = np.stack([oracle.normalize_copy(v)[0] for v in q])
    ids = np.sort(np.random.default_rng(900 + metric).choice(N, N_IDS, replace=False)).astype(np.uint32)
    with rxgpu.VectorIndex(metric, D, N) as ix, pytest.MonkeyPatch.context() as mp:
        ix.upload_rows(0, rows, inv)
        _env(mp, CASES["one-f32"][2])
        one = [ix.search_knn(q[i:i + 1], KK) for i in range(q.shape[0])]
        want = tuple(np.concatenate([r[j] for r in one]) for j in range(3))
        _env(mp, CASES["list-f32"][2])
        want_list = ix.search_knn_subset(q[:1], KK, ids)
        for w in want + want_list:
            w.setflags(write=False)
        _env(mp, {})
        yield ix, q, ids, want, want_list


@pytest.mark.parametrize("case", list(CASES))
def test_slots_of_one_call(chains, monkeypatch, case):
    ix, q, ids, want, want_list = chains
    nq, listed, env, slots, cap = CASES[case]
    _env(monkeypatch, env)
    before = ix.last_candidates()
    ix.profile_enable(True)   # (clears the slots)
    got = ix.search_knn_subset(q[:nq], KK, ids) if listed else ix.search_knn(q[:nq], KK)
    seen = {s: ix.profile_read(s)[0] for s in SLOTS}
    cand = ix.last_candidates()
    ix.profile_enable(False)
    print(case, {s: n for s, n in seen.items() if n}, cand)
    assert seen == {s: slots.get(s, 0) for s in SLOTS}, case
    if cap is None:
        assert cand == before, (case, "a chain without a candidate list recorded one")
    else:
        assert cand[1] == cap and cand[0] <= cap, (case, cand)
    ref = want_list if listed else tuple(w[:nq] for w in want)
    assert np.array_equal(got[2], ref[2]) and int(got[2].min()) == KK, case
    assert np.array_equal(got[1], ref[1]), case
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), case
