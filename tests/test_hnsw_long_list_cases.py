"""CPU: the constructed graphs of tests/hnsw_long_list_cases.py — each proven here, over the restated engine, to hold what its GPU cases in
tests/test_gpu_hnsw_long_lists.py rely on (every list of the length its class names, searches that hop and evaluate enough, k live
results) before a card sees it."""
import numpy as np
import pytest

from . import hnsw_long_list_cases as cases


def test_classes_cover_both_sides_of_every_pass_boundary():
    """a pass reads words 64 p .. 64 p + 63 of a list, word 0 being the count: link j (from 1) lies in pass j // 64"""
    for M in (64, 32):
        cs = sorted(c for m, c in cases.CLASSES if m == M)
        last_pass = {c: c // 64 for c in cs}
        assert 2 * M in cs and 63 in cs and 64 in cs       # the last word of pass 1; the first word of pass 2 alone
        assert last_pass[63] == 0 and last_pass[64] == 1
        if M == 64:
            assert cs == [63, 64, 65, 127, 128] and last_pass[127] == 1 and last_pass[128] == 2
    assert all(c <= 2 * M <= 128 for M, c in cases.CLASSES)


def test_nearest_ids_order_and_ties():
    rows = np.array([[0, 0], [1, 0], [-1, 0], [0, 2], [0, 2]], np.float32)   # rows 1 and 2 at one distance of row 0; rows 3 and 4 equal
    got = cases.nearest_ids(0, rows, keep=4)
    assert got[0].tolist() == [1, 2, 3, 4] and got[3].tolist()[0] == 4 and got[4].tolist()[0] == 3
    assert cases.nearest_ids(0, rows, among=[0, 3, 4], keep=8).tolist() == [[3, 4], [4, 0], [3, 0]]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.case_id)
def test_graph_holds_what_its_gpu_cases_rely_on(oracle, shape):
    lo_h, hi_h, lo_e, hi_e = cases.check_conditions(oracle, *shape)
    print(cases.case_id(shape), "hops", lo_h, "..", hi_h, "distance evaluations", lo_e, "..", hi_e, "of", cases.N)


@pytest.mark.parametrize("shape", cases.HANDOVER, ids=lambda s: "metric%d-M%d-d%d-c%d" % s)
def test_deep_session_over_6000_rows_outgrows_the_lds_staging_mid_call(oracle, shape):
    """what test_streaming_call_leaves_the_lds_staging relies on: one call of the session starts with at most 3072 - maxM0 candidates and
    passes that number in front of a pop; every call emits its 64 results, and the extras never come near their 1024 entries"""
    metric, M, d, c = shape
    g = cases.full_graph(metric, M, d, c, n=cases.HANDOVER_N)
    assert g["n"] == cases.HANDOVER_N
    cases.check_structure(g, M, c)
    calls = cases.handover_calls(oracle, metric, M, d, c)
    gate = cases.STREAM_LDS_CAND - 2 * M
    handed = [i for i, call in enumerate(calls) if call[4]]
    assert len(handed) >= 1, handed
    cand0, peak, _ = calls[handed[0]][5]
    assert cand0 <= gate < peak, (cand0, peak)
    assert all(call[3] for call in calls[:handed[0] + 1]) and not calls[handed[0] + 1][3]   # the next call starts on the global heaps
    assert all(len(call[0]) == 64 and not call[2] for call in calls) and max(call[5][2] for call in calls) < 512
    print(shape, "handed over in call", handed[0], "candidates at its start, at their peak:", cand0, peak)


def test_sessions_over_3000_rows_stay_below_the_gate(oracle):
    """why the 3000-row graphs cannot show the handover: candidate_set (evaluated, not yet popped) peaks far below 2944"""
    from oracle.pyoracle import OracleHnswStream
    from .conftest import make_corpus
    for c in (64, 128):
        g = cases.full_graph(0, 64, 48, c)
        for qi, (ef, batches) in enumerate([(64, [64] * 12), (100, [1000] * 4), (64, [64] * 60), (200, [1000] * 7)]):
            s = OracleHnswStream(oracle, g, make_corpus(900 + qi, 1, 48)[0], ef, None)
            for b in batches:
                s.next(b)
                assert s.last_sizes()[3] < 2600, (c, qi, s.last_sizes())
            s.close()
