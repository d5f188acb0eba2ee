"""-m gpu: layout invariance of every vector search.  include/rxgpu.h lets an index run over rows stored as [n][row_stride] floats
(rxgpu_index_adopt_device_rows: row_stride >= dim, row_stride % 4 == 0, 16-byte aligned), and RXGPU_ROW_ALIGN gives an owned index such a
stride as well.  The same logical rows in different layouts must give the same counts, rows and distance bits from every entry point.

The yardstick is the CPU oracle (oracle.dist_many + lex_topk, oracle.bf_search_range, oracle_hnsw_search_knn on the exported graph); an
owned, tight index over the same rows is searched beside the layouts for a clearer message and where the oracle has no form.  Every float of
an adopted buffer that is not one of the dim elements of a live row (pads, guard rows, guard norms) is NaN: a kernel that reads one as data
returns NaN distances or loses rows.

layouts   tight         adopted, stride = dim rounded up to 4
          padded4/20/64 adopted, stride = round4(dim) + 4 / 20 / 64 (20 keeps rows off 64- and 256-byte boundaries)
          guarded       padded20, the adopted pointer 3 rows into a larger buffer with 3 more rows behind the last; the norms alike
          aligned4096 / aligned256   owned under RXGPU_ROW_ALIGN (pads are whatever the allocation held: the oracle comparison alone)
          far           adopted, stride = 2^20 floats, n = 4160: rows from 1024 on start beyond 2^32 bytes, rows from 4096 on beyond 2^32 elements
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from .conftest import lex_topk, make_corpus

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]   # l2, ip, cosine
DIMS = [5, 100, 130, 768]   # tail only with dim % 4 != 0; generic with a tail; generic above 128, inside the int8 tier's range; the fixed kernel
N = 3001
N_TIER = 12_007   # d = 768: gaussian rows stay inside the candidate list (test_gpu_scan_i8.py)
BF16_SHAPES = [(100, N), (768, N_TIER)]   # the bf16 tier serves dimensions that round up (to 64) to 128, 256, 384, 512, 768 or 1024
I8_SHAPES = [(130, N), (768, N_TIER)]     # the int8 tier serves 128 < dim <= 1024
# (d = 64 is in no list: no tier asks for D <= 128.  64 floats round up to a shadow row of 64, which scan_bf16_supported refuses, and the int8
# tier starts above 128; the bf16 tier at its narrowest shadow, 128, is reached through d = 100, which has a tail as well.)
ENV = ("RXGPU_SCAN_BF16", "RXGPU_SCAN_BF16_MIN_BYTES", "RXGPU_SCAN_I8", "RXGPU_SCAN_I8_MIN_BYTES", "RXGPU_SCAN_I8_SUBSET_MIN_BYTES",
       "RXGPU_SCAN_I8_RANGE_MIN_BYTES", "RXGPU_SCAN_I8_WG_PER_CU", "RXGPU_GEMM_SPLIT", "RXGPU_BATCH_BF16_MIN", "RXGPU_SHADOW_BLOCKED")
ADOPTED = ("tight", "padded4", "padded20", "padded64", "guarded")
ALIGNED = ("aligned4096", "aligned256")
LAYOUTS = ADOPTED + ALIGNED
PAD = {"tight": 0, "padded4": 4, "padded20": 20, "padded64": 64, "guarded": 20}
FAR_STRIDE, FAR_N, FAR_D = 1 << 20, 4160, 768
ERR_PARAMS, ERR_LOGIC = -3, -4


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def round4(d):
    return (d + 3) & ~3


def _env(monkeypatch, **kw):
    """the scan and nomination switches: all unset, then RXGPU_SCAN_<k> = v (a key that begins with RXGPU_ is taken as it is)"""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k if k.startswith("RXGPU_") else "RXGPU_SCAN_" + k, str(v))


# ---------------------------------------------------------------------------------------------------------------- data and references
_cache = {}


def _data(oracle, metric, d, n):
    """(rows, inv_norms or None, 256 queries), made once per shape and read-only"""
    key = ("data", metric, d, n)
    if key not in _cache:
        rows = make_corpus(7000 + d, n, d)
        q = make_corpus(8000 + d, 256, d)
        inv = None
        if metric == 2:
            inv = oracle.l2_modules(rows)
            q = np.stack([oracle.normalize_copy(v)[0] for v in q])
        for a in (rows, q, inv):
            if a is not None:
                a.setflags(write=False)
        _cache[key] = (rows, inv, q)
    return _cache[key]


def _dists(oracle, metric, d, n, qi):
    """the oracle's distances of query qi of _data to all rows, computed once"""
    key = ("dist", metric, d, n, qi)
    if key not in _cache:
        rows, inv, q = _data(oracle, metric, d, n)
        out = oracle.dist_many(metric, q[qi], rows, inv)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _check_knn(got, wants, kk, what, ids=None):
    """got = (dist, row, count) of len(wants) queries; wants[i]: the oracle's distances of query i to the rows searched (to rows[ids] with a list)"""
    dist, row, cnt = got
    for i, all_d in enumerate(wants):
        c = min(kk, all_d.shape[0])
        wd, wr = lex_topk(all_d, c)
        if ids is not None:
            wr = ids[wr]
        assert int(cnt[i]) == c, (what, i, int(cnt[i]), c)
        assert np.array_equal(row[i, :c], wr), (what, i, "rows", row[i, :c][:8], wr[:8])
        assert np.array_equal(bits(dist[i, :c]), bits(wd)), (what, i, "distance bits", dist[i, :c][:8], wd[:8])


def _same(a, b, what):
    """two (dist, row, count) results agree in all that the call defines"""
    (da, ra, ca), (db, rb, cb) = a, b
    assert np.array_equal(ca, cb), (what, "counts")
    for i in range(len(ca)):
        c = int(ca[i])
        assert np.array_equal(ra[i, :c], rb[i, :c]), (what, i, "rows")
        assert np.array_equal(bits(da[i, :c]), bits(db[i, :c])), (what, i, "distance bits")


# ---------------------------------------------------------------------------------------------------------------- layouts
def _tensor(a):
    """a device copy of a host array (the shared arrays are read-only, which torch does not take as they are)"""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def device_layout(rows, inv, stride, guard=0):
    """The rows in a torch device buffer of [guard + n + guard][stride] floats, NaN wherever no element of a live row lies.
    -> (ptr of row 0, stride, keepalive, ptr of the norm of row 0 or None); the norms are a tensor of their own, tight, guarded like the rows."""
    import torch
    n, d = rows.shape
    assert stride >= d and stride % 4 == 0
    buf = torch.full((n + 2 * guard, stride), float("nan"), dtype=torch.float32, device="cuda")
    buf[guard:guard + n, :d] = _tensor(rows)
    ptr = buf.data_ptr() + guard * stride * 4
    t_inv, inv_ptr = None, None
    if inv is not None:
        t_inv = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
        t_inv[guard:guard + n] = _tensor(inv)
        inv_ptr = t_inv.data_ptr() + guard * 4
    torch.cuda.synchronize()
    return ptr, stride, (buf, t_inv), inv_ptr


def aligned_stride(d, align):
    return ((round4(d) * 4 + align - 1) & ~(align - 1)) // 4


def open_aligned(rxgpu, metric, d, capacity, align):
    """an owned index created under RXGPU_ROW_ALIGN = align; the variable is set around the constructor only"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RXGPU_ROW_ALIGN", str(align))
        ix = rxgpu.VectorIndex(metric, d, capacity)
    want = aligned_stride(d, align)
    assert ix.row_stride == want, (d, align, ix.row_stride, want)
    assert want > round4(d) or round4(d) * 4 % align == 0
    return ix


def open_layout(rxgpu, name, metric, rows, inv):
    n, d = rows.shape
    if name == "owned":
        ix = rxgpu.VectorIndex(metric, d, n)
        assert ix.row_stride == round4(d)
        ix.upload_rows(0, rows, inv)
    elif name in ALIGNED:
        ix = open_aligned(rxgpu, metric, d, n, int(name[len("aligned"):]))
        ix.upload_rows(0, rows, inv)
    else:
        ptr, stride, keep, inv_ptr = device_layout(rows, inv, round4(d) + PAD[name], guard=3 if name == "guarded" else 0)
        ix = rxgpu.VectorIndex(metric, d)
        ix.adopt_device_rows(ptr, n, stride, inv_ptr, keepalive=keep)
        assert ix.row_stride == stride
    assert ix.count == n
    return ix


@contextlib.contextmanager
def open_layouts(rxgpu, metric, rows, inv, names=("owned",) + LAYOUTS):
    with contextlib.ExitStack() as st:
        yield {name: st.enter_context(open_layout(rxgpu, name, metric, rows, inv)) for name in names}


def _scan_slots(ix, fn, names=("scan", "scan_bf16", "scan_i8")):
    """(result of fn, launches filed under `names`, (candidates, capacity of the list)) with profiling on around fn"""
    ix.profile_enable(True)
    out = fn()
    n = tuple(ix.profile_read(s)[0] for s in names)
    cand = ix.last_candidates()
    ix.profile_enable(False)
    return out, n, cand


DERIVED = ("stats", "row_sq", "rows_bf16", "codes_i8", "side_i8")


def _derived(rxgpu, ix):
    """the bytes of every derived buffer the index has built so far (rxgpu_index_inspect): statistics words, |x|^2 per row, both shadows"""
    out = {}
    for name in DERIVED:
        try:
            out[name] = ix.inspect(name).view(np.uint8).copy()
        except rxgpu.RxGpuError as err:
            assert err.code == ERR_LOGIC, (name, err)   # not built, or a name the metric does not have
    return out


def _same_derived(rxgpu, ix, ref, need, what):
    """what the builders derived from the layout's rows is byte-equal to what they derived from the owned index's: a builder that read a pad
    or a guard row leaves other bytes, even where the exact re-score behind the nomination still returns the right rows"""
    got, want = _derived(rxgpu, ix), _derived(rxgpu, ref)
    assert set(need) <= set(want), (what, "the owned index has not built", set(need) - set(want))
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (what, name)


# ---------------------------------------------------------------------------------------------------------------- 1. single-query k-NN
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_f32_single_query_knn_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    """kk 1, 11, 64: the fused scan; 65, 100, 128: two entries per lane; 300: the distance pass with radix select; kk above n"""
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch, BF16=0)
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for kk in (1, 11, 64, 65, 100, 128, 300, N + 50):
            for qi in range(2):
                ref = ixs["owned"].search_knn(q[qi:qi + 1], kk)
                for name, ix in ixs.items():
                    got = ix.search_knn(q[qi:qi + 1], kk)
                    _check_knn(got, [_dists(oracle, metric, d, N, qi)], kk, (name, metric, d, kk, qi))
                    _same(got, ref, (name, "vs owned", metric, d, kk, qi))


def _reversed_copy(rows, inv):
    return np.ascontiguousarray(rows[::-1]), (np.ascontiguousarray(inv[::-1]) if inv is not None else None)


def _forced_tier(rxgpu, oracle, monkeypatch, metric, d, n, tier):
    want_slots = {"BF16": (0, 1, 0), "I8": (0, 0, 1)}[tier]
    need = {"BF16": ("stats", "rows_bf16"), "I8": ("stats", "codes_i8", "side_i8")}[tier]
    rows, inv, q = _data(oracle, metric, d, n)
    worst = 0

    def check(ix, wants, what, owned=None):
        """-> the candidates of every call.  Where the list holds every row (n = 3001) cand <= cap can fail only for a query without a finite
        bound, and over-nominated rows are re-scored exactly: the count itself has to equal the owned index's, and the shadows theirs."""
        nonlocal worst
        cands = {}
        for kk in (1, 11, 64):
            for qi in range(2):
                _env(monkeypatch, **{tier: 1})
                got, slots, (cand, cap) = _scan_slots(ix, lambda: ix.search_knn(q[qi:qi + 1], kk))
                print(what, "kk", kk, "query", qi, "slots", slots, "candidates", cand, "of", cap)
                assert slots == want_slots, (what, kk, qi, slots)
                assert cand <= cap, (what, kk, qi, "the exact scan behind the gate answered", cand, cap)
                worst = max(worst, cand)
                cands[kk, qi] = (cand, cap)
                _check_knn(got, [wants[qi]], kk, (what, kk, qi))
        if owned is not None:
            assert cands == owned[1], (what, "candidates, capacity by (kk, query): layout, then owned", cands, owned[1])
            _same_derived(rxgpu, ix, owned[0], need, what)
        return cands

    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        wants = [_dists(oracle, metric, d, n, qi) for qi in range(2)]
        owned = (ixs["owned"], check(ixs["owned"], wants, (tier, "owned", metric, d)))
        for name in LAYOUTS:
            check(ixs[name], wants, (tier, name, metric, d), owned)
        # a second adoption, onto the same rows in reverse order at another stride: what was derived from the first storage must go
        rrows, rinv = _reversed_copy(rows, inv)
        rwants = [np.ascontiguousarray(w[::-1]) for w in wants]
        with open_layout(rxgpu, "owned", metric, rrows, rinv) as rix:
            rowned = (rix, check(rix, rwants, (tier, "owned, reversed", metric, d)))
            for name in ADOPTED:
                ptr, stride, keep, inv_ptr = device_layout(rrows, rinv, round4(d) + (4 if PAD[name] == 64 else 64), guard=0 if name == "guarded" else 3)
                assert stride != ixs[name].row_stride
                ixs[name].adopt_device_rows(ptr, n, stride, inv_ptr, keepalive=keep)
                check(ixs[name], rwants, (tier, name, "adopted again", metric, d), rowned)
    print(f"{tier} tier metric={metric} d={d} n={n}: at most {worst} candidates")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", BF16_SHAPES)
def test_forced_bf16_tier_over_every_layout(rxgpu, oracle, monkeypatch, metric, d, n):
    _forced_tier(rxgpu, oracle, monkeypatch, metric, d, n, "BF16")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", I8_SHAPES)
def test_forced_int8_tier_over_every_layout(rxgpu, oracle, monkeypatch, metric, d, n):
    _forced_tier(rxgpu, oracle, monkeypatch, metric, d, n, "I8")


# ---------------------------------------------------------------------------------------------------------------- 2. batched queries
BATCHED_SLOTS = ("gemm_sample", "gemm", "rescore", "scan", "scan_bf16", "scan_i8")   # one chunk of up to 256 queries: one launch of each of the first three
NOMINATION = {"default": {}, "single_ring": {"RXGPU_GEMM_SPLIT": 0}, "f32": {"RXGPU_BATCH_BF16_MIN": 0}, "rowmajor_shadow": {"RXGPU_SHADOW_BLOCKED": 0}}


@pytest.mark.parametrize("form", list(NOMINATION))
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_batched_queries_over_every_layout(rxgpu, oracle, monkeypatch, metric, d, form):
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch, **NOMINATION[form])   # before the indexes exist: the shadow's form is decided when it is built
    wants = [_dists(oracle, metric, d, N, qi) for qi in range(256)]
    # the f32 nomination reads the rows themselves and derives |x|^2 (l2) and the statistics; the others read the bf16 shadow as well
    need = ("stats",) + (("row_sq",) if metric == 0 else ()) + (("rows_bf16",) if form != "f32" else ())
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for nq, kk in ((2, 11), (2, 33), (40, 11), (40, 33), (70, 11), (70, 33), (256, 11), (256, 33)):
            ref = ixs["owned"].search_knn(q[:nq], kk)
            for name, ix in ixs.items():
                got, slots, _ = _scan_slots(ix, lambda: ix.search_knn(q[:nq], kk), BATCHED_SLOTS)
                assert slots == (1, 1, 1, 0, 0, 0), (name, form, metric, d, nq, kk, "the nomination chain did not answer", slots)
                _check_knn(got, wants[:nq], kk, (name, form, metric, d, nq, kk))
                _same(got, ref, (name, "vs owned", form, metric, d, nq, kk))
        # A batch records no candidate count (rxgpu_index_last_candidates is for one query; test_gpu_knn_chain_slots.py pins that), and its
        # list holds every row at this n, so over-nominated rows would be re-scored exactly.  What a nomination reads besides the rows and
        # the norms is compared instead: byte-equal to the owned index's, so the same thresholds and the same rows nominated.
        for name in LAYOUTS:
            _same_derived(rxgpu, ixs[name], ixs["owned"], need, (name, form, metric, d))


# ---------------------------------------------------------------------------------------------------------------- 3. device and resident entry points
def _d2h(rxgpu, ptr, count, dtype):
    """`count` elements at a device pointer of the library (hipMemcpy of the HIP runtime the library is linked to)"""
    fn = rxgpu.lib().hipMemcpy
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, dtype)
    assert fn(out.ctypes.data, ptr, out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def _device_knn(ix, queries, kk, ids=None):
    """rxgpu_search_knn_device / _subset_device on a torch stream of its own -> (dist, row, count)"""
    import torch
    nq = queries.shape[0]
    dq = _tensor(queries)
    od = torch.full((nq, kk), float("inf"), dtype=torch.float32, device="cuda")
    orow = torch.full((nq, kk), -1, dtype=torch.int32, device="cuda")
    oc = torch.zeros(nq, dtype=torch.int32, device="cuda")
    dids = _tensor(ids.astype(np.int32)) if ids is not None else None
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    if ids is None:
        ix.search_knn_device(dq.data_ptr(), nq, kk, od.data_ptr(), orow.data_ptr(), oc.data_ptr(), stream.cuda_stream)
    else:
        ix.search_knn_subset_device(dq.data_ptr(), nq, kk, dids.data_ptr(), ids.size, od.data_ptr(), orow.data_ptr(), oc.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return od.cpu().numpy(), orow.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)


def _resident_knn(rxgpu, ix, query, kk):
    import torch
    dd, dr, dc, _, entries = ix.search_knn_resident(query, kk)
    torch.cuda.synchronize()   # the search was only enqueued
    cnt = _d2h(rxgpu, dc, 1, np.uint32)
    return _d2h(rxgpu, dd, entries, np.float32)[None, :], _d2h(rxgpu, dr, entries, np.uint32)[None, :], cnt


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_device_and_resident_entry_points_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch)
    wants = [_dists(oracle, metric, d, N, qi) for qi in range(40)]
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for name, ix in ixs.items():
            for nq, kk in ((1, 11), (40, 11)):
                _check_knn(_device_knn(ix, q[:nq], kk), wants[:nq], kk, ("search_knn_device", name, metric, d, nq))
            for kk in (11, 100):
                got = _resident_knn(rxgpu, ix, q[3], kk)
                assert got[0].shape[1] == kk
                _check_knn(got, [wants[3]], kk, ("search_knn_resident", name, metric, d, kk))


# ---------------------------------------------------------------------------------------------------------------- 4. row lists
def _lists(n, seed):
    rng = np.random.default_rng(seed)
    one = np.sort(rng.choice(n, max(n // 100, 1), replace=False)).astype(np.uint32)
    half = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)
    return {"1%": one, "50%": half, "100%": np.arange(n, dtype=np.uint32)}


def _bitmap(ids, n):
    words = np.zeros((n + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return words


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_row_lists_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch, BF16=0)
    all_d = _dists(oracle, metric, d, N, 0)
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for lname, ids in _lists(N, d).items():
            words = _bitmap(ids, N)
            for kk in (11, 100, 300):
                ref = ixs["owned"].search_knn_subset(q[:1], kk, ids)
                for name, ix in ixs.items():
                    what = (name, metric, d, lname, kk)
                    got = ix.search_knn_subset(q[:1], kk, ids)
                    _check_knn(got, [all_d[ids]], kk, ("subset",) + what, ids)
                    _same(got, ref, ("subset vs owned",) + what)
                    bd, br, bc, allowed = ix.search_knn_bitmap(q[:1], kk, words)
                    assert allowed == ids.size
                    _check_knn((bd, br, bc), [all_d[ids]], kk, ("bitmap",) + what, ids)
                    if kk <= 128:
                        _check_knn(_device_knn(ix, q[:1], kk, ids), [all_d[ids]], kk, ("subset_device",) + what, ids)
                    else:   # rxgpu_search_knn_subset_device takes kk in [1, 128]: RXGPU_ERR_PARAMS above
                        with pytest.raises(rxgpu.RxGpuError) as err:
                            _device_knn(ix, q[:1], kk, ids)
                        assert err.value.code == ERR_PARAMS, what
                    if lname == "100%":
                        _same(got, ix.search_knn(q[:1], kk), ("the full list vs the unfiltered search",) + what)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", I8_SHAPES)
def test_forced_int8_subset_tier_over_every_layout(rxgpu, oracle, monkeypatch, metric, d, n):
    rows, inv, q = _data(oracle, metric, d, n)
    all_d = _dists(oracle, metric, d, n, 0)
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for lname, ids in _lists(n, d).items():
            for kk in (11, 64):
                for name, ix in ixs.items():
                    _env(monkeypatch, I8=1)
                    got, slots, (cand, cap) = _scan_slots(ix, lambda: ix.search_knn_subset(q[:1], kk, ids), ("scan_subset", "scan_i8_subset", "fallback_scan"))
                    assert slots == (0, 1, 0), (name, metric, d, lname, kk, slots)
                    assert cand <= cap, (name, metric, d, lname, kk, "the exact scan behind the gate answered", cand, cap)
                    if name == "owned":   # (the first of the layouts)
                        owned_cand = (cand, cap)
                    assert (cand, cap) == owned_cand, (name, metric, d, lname, kk, "candidates, capacity: layout, then owned", (cand, cap), owned_cand)
                    _check_knn(got, [all_d[ids]], kk, ("int8 subset", name, metric, d, lname, kk), ids)
        for name in LAYOUTS:
            _same_derived(rxgpu, ixs[name], ixs["owned"], ("stats", "codes_i8", "side_i8"), ("int8 subset", name, metric, d))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [100, 768])
def test_ivf_lists_with_the_coarse_index_on_strided_storage(rxgpu, oracle, monkeypatch, metric, d):
    """set_lists + search_knn_lists / search_range_lists: the coarse index over the centroids is adopted at the layout's stride as well"""
    nlist = 24
    rows, inv, q = _data(oracle, metric, d, N)
    cents = make_corpus(9000 + d, nlist, d)
    cinv = oracle.l2_modules(cents) if metric == 2 else None
    owner = np.random.default_rng(d).integers(0, nlist, N)
    lists = [np.flatnonzero(owner == l).astype(np.uint32) for l in range(nlist)]
    _env(monkeypatch, BF16=0)
    with open_layouts(rxgpu, metric, rows, inv, ("owned", "padded20", "guarded", "aligned4096")) as ixs, \
            open_layouts(rxgpu, metric, cents, cinv, ("owned", "padded20", "guarded", "aligned4096")) as cxs:
        for name, ix in ixs.items():
            ix.set_lists(lists)
            for qi in range(3):
                all_d = _dists(oracle, metric, d, N, qi)
                for nprobe, k in ((1, 10), (4, 100), (24, 33)):
                    _, probed = lex_topk(oracle.dist_many(metric, q[qi], cents, cinv), nprobe)
                    ids = np.sort(np.concatenate([lists[int(l)] for l in probed]))
                    what = (name, metric, d, qi, nprobe, k)
                    gd, gr, scanned = ix.search_knn_lists(cxs[name], q[qi], nprobe, k)
                    assert scanned == ids.size, what
                    _check_knn((gd[None, :], gr[None, :], np.array([gd.size])), [all_d[ids]], k, ("search_knn_lists",) + what, ids)
                    srt = np.sort(all_d[ids])
                    radius = float(srt[min(40, srt.size - 1)])
                    keep = all_d[ids] < radius
                    wd, wpos = lex_topk(np.where(keep, all_d[ids], np.inf), int(keep.sum()))
                    rd, rr, rscanned = ix.search_range_lists(cxs[name], q[qi], nprobe, radius, cap=8)   # cap 8: the overflow retry
                    assert rscanned == ids.size, what
                    assert np.array_equal(rr, ids[wpos]) and np.array_equal(bits(rd), bits(wd)), ("search_range_lists",) + what


# ---------------------------------------------------------------------------------------------------------------- 5. range search
def _radii(all_d):
    """no hit, 40 hits (halfway between ranks 40 and 41), every row"""
    srt = np.sort(all_d)
    mid = np.float32((np.float64(srt[39]) + np.float64(srt[40])) / 2)
    assert srt[39] < mid <= srt[40]
    return [(float(np.nextafter(srt[0], np.float32(-np.inf))), 0), (float(mid), 40), (3.0e38, all_d.size)]


def _want_range(all_d, radius, ids=None):
    d = all_d if ids is None else all_d[ids]
    keep = d < np.float32(radius)
    wd, wpos = lex_topk(np.where(keep, d, np.inf), int(keep.sum()))
    return wd, (wpos if ids is None else ids[wpos])


def _check_range(oracle, ix, metric, rows, inv, query, all_d, ids, what, i8=False):
    for radius, hits in _radii(all_d if ids is None else all_d[ids]):
        wd, wr = _want_range(all_d, radius, ids)
        assert wd.size == hits, (what, radius)
        if ids is None:   # the oracle's own range search as well
            od, ol = oracle.bf_search_range(metric, rows, np.arange(rows.shape[0], dtype=np.uint64), inv, query, radius)
            assert np.array_equal(ol, wr.astype(np.uint64)) and np.array_equal(bits(od), bits(wd)), (what, radius)

        def call():
            return ix.search_range(query, radius, cap=64) if ids is None else ix.search_range_subset(query, radius, ids, cap=64)   # cap 64: the overflow retry
        if i8:
            names = ("range", "range_i8", "range_rescore") if ids is None else ("range_subset", "range_i8_subset", "range_rescore")
            (gd, gr), slots, (cand, ccap) = _scan_slots(ix, call, names)
            assert slots[0] == 0 and slots[1] >= 1, (what, radius, slots)
            assert cand <= ccap, (what, radius, "the f32 kernel behind the tier answered", cand, ccap)
        else:
            gd, gr = call()
        assert np.array_equal(gr, wr), (what, radius, "rows", gr[:8], wr[:8])
        assert np.array_equal(bits(gd), bits(wd)), (what, radius, "distance bits")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_f32_range_search_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch, BF16=0)
    all_d = _dists(oracle, metric, d, N, 0)
    half = _lists(N, d)["50%"]
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for name, ix in ixs.items():
            _check_range(oracle, ix, metric, rows, inv, q[0], all_d, None, ("range", name, metric, d))
            _check_range(oracle, ix, metric, rows, inv, q[0], all_d, half, ("range_subset", name, metric, d))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [130, 768])
def test_forced_int8_range_tier_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    """n = 3001: the candidate list of a range call holds min(n, max(4096, 2 cap)) rows, so the tier itself answers the radius of every row too"""
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch, I8=1)
    all_d = _dists(oracle, metric, d, N, 0)
    half = _lists(N, d)["50%"]
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for name, ix in ixs.items():
            _check_range(oracle, ix, metric, rows, inv, q[0], all_d, None, ("int8 range", name, metric, d), i8=True)
            _check_range(oracle, ix, metric, rows, inv, q[0], all_d, half, ("int8 range_subset", name, metric, d), i8=True)


# ---------------------------------------------------------------------------------------------------------------- 6. row reads and error codes
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_distances_and_download_row_over_every_layout(rxgpu, oracle, metric, d):
    rows, inv, q = _data(oracle, metric, d, N)
    all_d = _dists(oracle, metric, d, N, 0)
    scattered = np.random.default_rng(d).permutation(N)[:300].astype(np.uint32)
    scattered[:3] = (0, N - 1, 0)   # both ends, one row twice
    L = rxgpu.lib()
    with open_layouts(rxgpu, metric, rows, inv) as ixs:
        for name, ix in ixs.items():
            assert np.array_equal(bits(ix.distances(q[0], scattered)), bits(all_d[scattered])), (name, metric, d)
            for r in (0, 1, 1500, N - 1):
                out, norm = np.full(d, np.nan, np.float32), C.c_float(np.nan)
                assert L.rxgpu_index_download_row(ix._h, r, out.ctypes.data, C.byref(norm)) == 0, (name, r)
                assert np.array_equal(bits(out), bits(rows[r])), (name, metric, d, r)
                assert bits(norm.value) == bits(inv[r] if inv is not None else 1.0), (name, metric, d, r)


@pytest.mark.parametrize("metric", METRICS)
def test_error_codes_of_adoption_and_of_mutations_on_adopted_storage(rxgpu, oracle, metric):
    d = 100
    rows, inv, q = _data(oracle, metric, d, N)
    L = rxgpu.lib()
    ptr, stride, keep, inv_ptr = device_layout(rows, inv, d + 20)
    with rxgpu.VectorIndex(metric, d) as ix:
        adopt = lambda p, s, norms: L.rxgpu_index_adopt_device_rows(ix._h, p, N, s, norms)
        assert adopt(ptr, d - 4, inv_ptr) == ERR_PARAMS      # row_stride < dim
        assert adopt(ptr, d + 2, inv_ptr) == ERR_PARAMS      # row_stride % 4 != 0
        assert adopt(ptr + 4, stride, inv_ptr) == ERR_PARAMS   # a pointer off 16 bytes
        assert adopt(ptr + 8, stride, inv_ptr) == ERR_PARAMS
        if metric == 2:
            assert adopt(ptr, stride, None) == ERR_PARAMS    # cosine without norms
        assert ix.count == 0                                 # nothing was adopted
        ix.adopt_device_rows(ptr, N, stride, inv_ptr, keepalive=keep)
        one = np.ascontiguousarray(rows[:1])
        one_inv = np.ascontiguousarray(inv[:1]) if inv is not None else None
        assert L.rxgpu_index_upload_rows(ix._h, 0, 1, one.ctypes.data, one_inv.ctypes.data if one_inv is not None else None) == ERR_LOGIC
        assert L.rxgpu_index_move_row(ix._h, 1, 0) == ERR_LOGIC
        assert L.rxgpu_index_reserve(ix._h, 2 * N) == ERR_LOGIC
        _check_knn(ix.search_knn(q[:1], 11), [_dists(oracle, metric, d, N, 0)], 11, ("after the refused calls", metric))   # and nothing changed


# ---------------------------------------------------------------------------------------------------------------- 7. mutations on strided owned storage
@pytest.mark.parametrize("align", [4096, 256])
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [100, 768])
def test_mutations_on_strided_owned_storage(rxgpu, oracle, monkeypatch, metric, d, align):
    """upload_rows (the 2-D copy), move_row, reserve and the upkeep of the shadows on rows that start every RXGPU_ROW_ALIGN bytes.  The forced
    tiers are asserted through the profile slots where the tier serves the dimension (bf16: 100 and 768, int8: 768); at d = 100 the forced
    int8 call takes what rxgpu_scan_tier names, and equals the oracle like every other."""
    src = make_corpus(500 + d, 3200, d)
    q = _data(oracle, metric, d, N)[2]
    best = np.ascontiguousarray(q[0] * np.float32(1.001))   # overwrites a row in the middle: the new best row of query 0 under every metric
    cur = np.empty((0, d), np.float32)

    def check(ix, step):
        inv = oracle.l2_modules(cur) if metric == 2 else None
        wants = [oracle.dist_many(metric, q[qi], cur, inv) for qi in range(70)]
        for env, tier in (({"BF16": 0}, 0), ({"BF16": 1}, 1), ({"I8": 1}, 2)):
            _env(monkeypatch, **env)
            expect = rxgpu.scan_tier(cur.shape[0], d)
            assert expect == tier or (tier == 2 and d <= 128), (step, env, expect)
            got, slots, (cand, cap) = _scan_slots(ix, lambda: ix.search_knn(q[:1], 11))
            assert slots == tuple(int(t == expect) for t in range(3)), (step, env, slots)
            if expect:
                assert cand <= cap, (step, env, cand, cap)
            _check_knn(got, wants[:1], 11, (step, env, metric, d, align))
        _env(monkeypatch)
        _check_knn(ix.search_knn(q[:70], 11), wants, 11, (step, "batch of 70", metric, d, align))

    def norms(a):
        return oracle.l2_modules(a) if metric == 2 else None

    with open_aligned(rxgpu, metric, d, 2600, align) as ix:
        cur = src[:2000].copy()
        ix.upload_rows(0, cur, norms(cur))
        check(ix, "a prefix")
        cur[1000] = best
        ix.upload_rows(1000, cur[1000:1001], norms(cur[1000:1001]))
        check(ix, "one row overwritten")
        assert int(ix.search_knn(q[:1], 1)[1][0, 0]) == 1000
        cur = np.concatenate([cur, src[2000:2500]])
        ix.upload_rows(2000, src[2000:2500], norms(src[2000:2500]))
        check(ix, "appended")
        ix.move_row(2499, 5)
        ix.truncate(2499)
        cur[5] = cur[2499]
        cur = cur[:2499].copy()
        check(ix, "move_row + truncate")
        ix.reserve(3200)
        assert ix.capacity == 3200 and ix.count == 2499 and ix.row_stride == aligned_stride(d, align)
        check(ix, "reserve past the capacity")
        cur = np.concatenate([cur, src[2500:3200]])[:3200]
        ix.upload_rows(2499, cur[2499:], norms(cur[2499:]))
        assert ix.count == cur.shape[0] > 2600
        check(ix, "appended past the first capacity")


# ---------------------------------------------------------------------------------------------------------------- 8. two shards, two strides
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_two_shards_adopted_at_different_strides(rxgpu, oracle, monkeypatch, metric, d):
    """shard 0 adopts padded memory, shard 1 guarded memory with another pad; the sharded handle answers like one owned index over all rows"""
    rows, inv, q = _data(oracle, metric, d, N)
    _env(monkeypatch)
    wants = [_dists(oracle, metric, d, N, qi) for qi in range(5)]
    half = _lists(N, d)["50%"]
    scattered = np.random.default_rng(d).permutation(N)[:200].astype(np.uint32)
    with rxgpu.ShardedVectorIndex(metric, d, N, [0, 0]) as sx, rxgpu.VectorIndex(metric, d, N) as one:
        one.upload_rows(0, rows, inv)
        cut = sx.shard_rows
        assert cut % 32 == 0 and 0 < cut < N
        a = device_layout(rows[:cut], inv[:cut] if inv is not None else None, round4(d) + 4)
        b = device_layout(rows[cut:], inv[cut:] if inv is not None else None, round4(d) + 64, guard=3)
        sx.shard(0).adopt_device_rows(a[0], cut, a[1], a[3])
        sx.shard(1).adopt_device_rows(b[0], N - cut, b[1], b[3])
        sx.sync_count()
        assert sx.count == N
        for nq in (1, 5):
            for kk in (11, 100):
                got = sx.search_knn(q[:nq], kk)
                _check_knn(got, wants[:nq], kk, ("sharded search_knn", metric, d, nq, kk))
                _same(got, one.search_knn(q[:nq], kk), ("sharded vs one index", metric, d, nq, kk))
        got = sx.search_knn_subset(q[:1], 11, half)
        _check_knn(got, [wants[0][half]], 11, ("sharded search_knn_subset", metric, d), half)
        _same(got, one.search_knn_subset(q[:1], 11, half), ("sharded subset vs one index", metric, d))
        _check_range(oracle, sx, metric, rows, inv, q[0], wants[0], None, ("sharded range", metric, d))
        assert np.array_equal(bits(sx.distances(q[0], scattered)), bits(wants[0][scattered])), (metric, d)
    del a, b


# ---------------------------------------------------------------------------------------------------------------- 9. rows beyond 2^32 elements
def _far_data(oracle, metric):
    """4160 x 768 rows; near-duplicates of queries 0..2 planted in rows 4100..4150, so that each one's 11 best rows lie beyond 2^32 elements (a
    32-bit wrap of row * stride turns row r into row r - 4096: another row, another answer)"""
    key = ("far", metric)
    if key not in _cache:
        rows = make_corpus(4242, FAR_N, FAR_D)
        q = make_corpus(4243, 70, FAR_D)
        noise = make_corpus(4244, 51, FAR_D, scale=0.01)
        for j in range(51):
            rows[4100 + j] = q[j % 3] + noise[j]
        inv = None
        if metric == 2:
            inv = oracle.l2_modules(rows)
            q = np.stack([oracle.normalize_copy(v)[0] for v in q])
        wants = [oracle.dist_many(metric, q[qi], rows, inv) for qi in range(70)]
        for qi in range(3):
            assert lex_topk(wants[qi], 11)[1].min() >= 4100
        _cache[key] = (rows, inv, q, wants)
    return _cache[key]


@pytest.fixture(scope="module")
def far_buffer():
    """the 16.25 GiB buffer of the far layout: one allocation, one fill, freed when the module is done"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device visible")
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip(f"the far layout needs 16.25 GiB in one piece: {free / 2 ** 30:.1f} GiB of device memory are free, 20 GiB are asked for")
    buf = torch.full((FAR_N, FAR_STRIDE), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :FAR_D] = _tensor(make_corpus(4242, FAR_N, FAR_D))   # the rows of _far_data before the planting
    torch.cuda.synchronize()
    state = {"buf": buf}
    yield state
    state.clear()
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("metric", METRICS)
def test_rows_beyond_2_to_the_32_elements(rxgpu, oracle, monkeypatch, far_buffer, metric):
    """one representative of every group over the far layout"""
    import torch
    rows, inv, q, wants = _far_data(oracle, metric)
    buf = far_buffer["buf"]
    buf[4100:4151, :FAR_D] = _tensor(rows[4100:4151])
    t_inv = _tensor(inv) if inv is not None else None
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0 and 4096 * FAR_STRIDE == 1 << 32
    rng = np.random.default_rng(5)
    half = np.flatnonzero(rng.random(FAR_N) < 0.5).astype(np.uint32)
    half = np.union1d(half, np.arange(4096, FAR_N)).astype(np.uint32)
    scattered = np.concatenate([rng.permutation(FAR_N)[:100], [0, 1023, 1024, 4095, 4096, 4100, 4150, FAR_N - 1]]).astype(np.uint32)
    with rxgpu.VectorIndex(metric, FAR_D) as ix:
        ix.adopt_device_rows(buf.data_ptr(), FAR_N, FAR_STRIDE, t_inv.data_ptr() if t_inv is not None else None, keepalive=(buf, t_inv))
        assert ix.row_stride == FAR_STRIDE
        what = ("far", metric)
        _env(monkeypatch, BF16=0)                                                 # the f32 scan, the radix select, kk above n
        for kk in (11, 100, 300, FAR_N + 5):
            for qi in range(3):
                _check_knn(ix.search_knn(q[qi:qi + 1], kk), [wants[qi]], kk, what + ("f32 scan", kk, qi))
        for tier, want_slots in (("BF16", (0, 1, 0)), ("I8", (0, 0, 1))):        # both forced tiers
            for qi in range(3):
                _env(monkeypatch, **{tier: 1})
                got, slots, (cand, cap) = _scan_slots(ix, lambda: ix.search_knn(q[qi:qi + 1], 11))
                assert slots == want_slots and cand <= cap, what + (tier, slots, cand, cap)
                _check_knn(got, [wants[qi]], 11, what + (tier, qi))
        _env(monkeypatch)                                                         # batched, both nominations
        _check_knn(ix.search_knn(q[:70], 11), wants, 11, what + ("batch of 70",))
        _check_knn(ix.search_knn(q[:40], 33), wants[:40], 33, what + ("batch of 40",))
        _env(monkeypatch, RXGPU_BATCH_BF16_MIN=0)
        _check_knn(ix.search_knn(q[:70], 11), wants, 11, what + ("batch of 70, f32 nomination",))
        _env(monkeypatch)                                                         # device and resident entry points
        _check_knn(_device_knn(ix, q[:1], 11), wants[:1], 11, what + ("search_knn_device",))
        _check_knn(_resident_knn(rxgpu, ix, q[1], 100), [wants[1]], 100, what + ("search_knn_resident",))
        _env(monkeypatch, BF16=0)                                                 # row lists
        for kk in (11, 300):
            _check_knn(ix.search_knn_subset(q[:1], kk, half), [wants[0][half]], kk, what + ("subset", kk), half)
        bd, br, bc, allowed = ix.search_knn_bitmap(q[:1], 11, _bitmap(half, FAR_N))
        _check_knn((bd, br, bc), [wants[0][half]], 11, what + ("bitmap",), half)
        _check_knn(_device_knn(ix, q[:1], 11, half), [wants[0][half]], 11, what + ("subset_device",), half)
        _env(monkeypatch, I8=1)
        got, slots, (cand, cap) = _scan_slots(ix, lambda: ix.search_knn_subset(q[:1], 11, half), ("scan_subset", "scan_i8_subset", "fallback_scan"))
        assert slots == (0, 1, 0) and cand <= cap, what + ("int8 subset", slots, cand, cap)
        _check_knn(got, [wants[0][half]], 11, what + ("int8 subset",), half)
        _env(monkeypatch, BF16=0)                                                 # range, both tiers
        _check_range(oracle, ix, metric, rows, inv, q[0], wants[0], None, what + ("range",))
        _check_range(oracle, ix, metric, rows, inv, q[0], wants[0], half, what + ("range_subset",))
        _env(monkeypatch, I8=1)
        for radius, hits in _radii(wants[0])[:2]:   # (the radius of every row: 4160 candidates against a list of 4096, the f32 kernel by design)
            wd, wr = _want_range(wants[0], radius)
            (gd, gr), slots, (cand, ccap) = _scan_slots(ix, lambda: ix.search_range(q[0], radius, cap=64), ("range", "range_i8", "range_rescore"))
            assert slots == (0, 1, 1) and cand <= ccap, what + ("int8 range", radius, slots, cand, ccap)
            assert wd.size == hits and np.array_equal(gr, wr) and np.array_equal(bits(gd), bits(wd)), what + ("int8 range", radius)
            wd, wr = _want_range(wants[0], radius, half)
            (gd, gr), slots, (cand, ccap) = _scan_slots(ix, lambda: ix.search_range_subset(q[0], radius, half, cap=64),
                                                       ("range_subset", "range_i8_subset", "range_rescore"))
            assert slots == (0, 1, 1) and cand <= ccap, what + ("int8 range_subset", radius, slots, cand, ccap)
            assert np.array_equal(gr, wr) and np.array_equal(bits(gd), bits(wd)), what + ("int8 range_subset", radius)
        assert np.array_equal(bits(ix.distances(q[0], scattered)), bits(wants[0][scattered])), what + ("distances",)


# ---------------------------------------------------------------------------------------------------------------- 10. HNSW
HNSW_N = 3000
PLANS = ((10, 128), (10, 10), (40, 64), (60, 250))


def _graph(oracle, metric, d, deleted=0):
    """(flat graph with the rows as its vectors, rows, inv_norms, 12 queries) of a GpuHnswMap build, made once per shape"""
    key = ("hnsw", metric, d, deleted)
    if key not in _cache:
        from reindexer_amd import hostapi
        rows = make_corpus(600 + d, HNSW_N, d)
        labels = (np.arange(HNSW_N, dtype=np.uint64) << np.uint64(32)) | np.uint64(3)
        m = hostapi.GpuHnswMap(metric, d, HNSW_N, M=16, ef_construction=100)
        m.add(rows, labels)
        for lab in labels[np.random.default_rng(d).choice(HNSW_N, deleted, replace=False)] if deleted else ():
            m.mark_delete(lab)
        g = m.export_graph()
        m.close()
        g["vectors"] = rows
        assert int(np.count_nonzero(g["deleted"])) == deleted
        inv = oracle.l2_modules(rows) if metric == 2 else None
        q = make_corpus(700 + d, 12, d)
        if metric == 2:
            q = np.stack([oracle.normalize_copy(v)[0] for v in q])
        _cache[key] = (g, rows, inv, q)
    return _cache[key]


def _pairs(dist, labels):
    order = np.lexsort((labels, dist))
    return bits(dist[order]), labels[order]


def _check_hnsw(g, got, wants, what):
    """got = (dist, row, count) of len(wants) queries; wants[i] = the restated engine's (dist, labels)"""
    dist, row, cnt = got
    for i, (wd, wl) in enumerate(wants):
        c = int(cnt[i])
        assert c == wd.size, (what, i, c, wd.size)
        a, b = _pairs(dist[i, :c], g["labels"][row[i, :c]]), _pairs(wd, wl)
        assert np.array_equal(a[1], b[1]), (what, i, "labels")
        assert np.array_equal(a[0], b[0]), (what, i, "distance bits")


def _hnsw_wants(oracle, metric, d, k, ef, deleted=0):
    """the restated engine's (dist, labels) of the 12 queries of _graph under one plan, computed once"""
    key = ("hnsw wants", metric, d, deleted, k, ef)
    if key not in _cache:
        from oracle.pyoracle import oracle_hnsw_search_knn
        g, _, inv, q = _graph(oracle, metric, d, deleted)
        _cache[key] = [oracle_hnsw_search_knn(oracle, g, v, k, ef, inv) for v in q]
    return _cache[key]


@contextlib.contextmanager
def _hnsw_layouts(rxgpu, metric, g, rows, inv, names=("owned", "padded20", "aligned4096")):
    with open_layouts(rxgpu, metric, rows, inv, names) as ixs:
        for ix in ixs.values():
            ix.hnsw_attach_graph(g)
        yield ixs


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [100, 384, 128, 768])   # 100 and 384: the generic kernel; 128 and 768: the fixed one
def test_hnsw_search_over_every_layout(rxgpu, oracle, monkeypatch, metric, d):
    g, rows, inv, q = _graph(oracle, metric, d)
    batch = np.tile(q, (25, 1))   # 300 queries: the batch form
    with _hnsw_layouts(rxgpu, metric, g, rows, inv) as ixs:
        for k, ef in PLANS:
            wants = _hnsw_wants(oracle, metric, d, k, ef)
            ref = None
            for name, ix in ixs.items():
                what = (name, metric, d, k, ef)
                monkeypatch.delenv("RXGPU_HNSW_SERVER", raising=False)
                single = [ix.hnsw_search_knn(v[None, :], k, ef) for v in q]
                monkeypatch.setenv("RXGPU_HNSW_SERVER", "0")   # the launched form of one query (without it the resident kernel serves 128 and 768)
                launched = [ix.hnsw_search_knn(v[None, :], k, ef) for v in q]
                monkeypatch.delenv("RXGPU_HNSW_SERVER")
                for i in range(12):
                    _check_hnsw(g, single[i], wants[i:i + 1], ("nq = 1",) + what + (i,))
                    _check_hnsw(g, launched[i], wants[i:i + 1], ("nq = 1, launched",) + what + (i,))
                many = ix.hnsw_search_knn(batch, k, ef)
                _check_hnsw(g, many, wants * 25, ("nq = 300",) + what)
                if ref is None:
                    ref = (single, launched, many)
                else:
                    for i in range(12):
                        _same(single[i], ref[0][i], ("nq = 1 vs owned",) + what + (i,))
                        _same(launched[i], ref[1][i], ("nq = 1, launched, vs owned",) + what + (i,))
                    _same(many, ref[2], ("nq = 300 vs owned",) + what)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("d", [100, 384, 128, 768])
def test_hnsw_posted_search_over_every_layout(rxgpu, oracle, metric, d):
    """the resident kernel serves 128 and 768 floats per row, on strided rows too; at 100 and 384 the mailbox declines and rxgpu_hnsw_search_knn,
    the caller's next step, returns the same result"""
    g, rows, inv, q = _graph(oracle, metric, d)
    with _hnsw_layouts(rxgpu, metric, g, rows, inv) as ixs:
        for name, ix in ixs.items():
            served = 0
            for k, ef in PLANS:
                wants = _hnsw_wants(oracle, metric, d, k, ef)
                for i in range(12):
                    pd, pr, pc, ok = ix.hnsw_search_knn_posted(q[i], k, ef)
                    if d in (100, 384):
                        assert not ok, (name, metric, d, k, ef, i)
                    if ok:
                        served += 1
                        got = (pd[None, :], pr[None, :], np.array([pc]))
                    else:
                        got = ix.hnsw_search_knn(q[i][None, :], k, ef)
                    _check_hnsw(g, got, wants[i:i + 1], ("posted", ok, name, metric, d, k, ef, i))
            if d in (128, 768):
                assert served >= 0.9 * 12 * len(PLANS), (name, metric, d, served)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("case", ["heaps_only", "global_candidate_heap", "300_deleted"])
def test_hnsw_generic_kernel_at_384_on_padded_rows(rxgpu, oracle, monkeypatch, metric, case):
    d = 384
    deleted = 300 if case == "300_deleted" else 0
    g, rows, inv, q = _graph(oracle, metric, d, deleted)
    if case == "heaps_only":
        monkeypatch.setenv("RXGPU_HNSW_SORTED", "0")
    if case == "global_candidate_heap":
        monkeypatch.setenv("RXGPU_HNSW_LDS_CAND_CAP", "4")
    batch = np.tile(q, (25, 1))
    with _hnsw_layouts(rxgpu, metric, g, rows, inv, ("owned", "padded20")) as ixs:
        for k, ef in PLANS:
            wants = _hnsw_wants(oracle, metric, d, k, ef, deleted)
            for name, ix in ixs.items():
                for i in range(12):
                    _check_hnsw(g, ix.hnsw_search_knn(q[i][None, :], k, ef), wants[i:i + 1], (case, "nq = 1", name, metric, k, ef, i))
                _check_hnsw(g, ix.hnsw_search_knn(batch, k, ef), wants * 25, (case, "nq = 300", name, metric, k, ef))
