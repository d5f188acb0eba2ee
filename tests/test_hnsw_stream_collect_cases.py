"""CPU: the cases of tests/test_gpu_hnsw_stream_collect.py lie where that file says — shown with the restated engine (OracleHnswStream) under
the rule restated in Python (tests/hnsw_stream_collect_cases.py), no GPU: the 3000-row collections stay below kStreamLdsCand - maxM0 and
take 1 - 8 calls, ef 16 parks nodes in the extras, the selective shares exhaust the session, share 0 walks the batch ladder; the 6000-row
collections are on the side of the LDS limit they are there for; the 200-row graph runs out inside a call.  The Python rule equals the
library's estimate on every batch it computes on the way."""
import pytest

from . import hnsw_stream_collect_cases as cases


@pytest.mark.parametrize("metric,deleted", [(0, 0), (2, cases.A_DELETED)])
def test_a_cases_stay_in_lds(oracle, metric, deleted):
    from reindexer_amd import capi
    L = capi.lib()
    g = cases.graph(cases.A, metric, deleted)
    inv = oracle.l2_modules(g["vectors"]) if metric == 2 else None
    q = cases.query(oracle, metric, g["dim"])
    seen_calls, parked, exhausted = set(), 0, 0
    for share in cases.A_SHARES:
        allowed = cases.allowed_rows(g["n"], share)
        for needed in cases.A_NEEDED:
            for ef in cases.A_EF:
                r = cases.oracle_rule(oracle, g, q, inv, allowed, needed, ef, ef)
                assert r["peak_cand"] + g["maxM0"] <= cases.STREAM_LDS_CAND and r["peak_ext"] + 1 <= cases.STREAM_LDS_TOP, (share, needed, ef)
                assert 1 <= len(r["calls"]) <= 8
                seen_calls.add(len(r["calls"]))
                parked += int(ef == 16 and r["peak_ext"] > 0)
                exhausted += int(r["exhausted"])
                presented = 0
                for (b0, e0, a0), (b1, _, _) in zip(r["calls"], r["calls"][1:]):   # the Python rule == the plan header's estimate
                    presented += e0
                    assert b1 == L.rxgpu_hnsw_stream_collect_batch(a0, presented, needed)
                if share <= 0.02 and needed == 150:
                    assert r["exhausted"] and r["presented"] < g["n"]   # some nodes are unreachable
                if share == 0 and needed == 1 and ef == 100:
                    assert [c[0] for c in r["calls"]][:5] == [100, 100, 200, 400, 800]
    assert len(seen_calls) >= 4 and parked >= 10 and exhausted >= 6


def test_b_cases_are_on_their_side_of_the_lds_limit(oracle):
    g = cases.graph(cases.B, 0)
    q = cases.query(oracle, 0, g["dim"])
    limit = cases.STREAM_LDS_CAND - g["maxM0"]
    assert limit == 3040
    for share, needed, ef in cases.B_CASES:
        r = cases.oracle_rule(oracle, g, q, None, cases.allowed_rows(g["n"], share), needed, ef, ef)
        assert (r["peak_cand"] > limit) == (share != 1), (share, needed, ef, r["peak_cand"])
        assert r["start_sizes"][0][0] + g["maxM0"] <= cases.STREAM_LDS_CAND   # every collection STARTS in LDS


def test_small_graph_runs_out_inside_a_call(oracle):
    g = cases.graph(cases.SMALL, 0)
    r = cases.oracle_rule(oracle, g, cases.query(oracle, 0, g["dim"]), None, cases.allowed_rows(g["n"], 0.3), 70, 100, 100)
    assert len(r["calls"]) == 2 and r["exhausted"] and r["calls"][1][0] > r["calls"][1][1] and r["accepted"] < 70
