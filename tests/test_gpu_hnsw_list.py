"""GPU: hnsw's flat search with one allow list per query, served in list order
(wv_index_hnsw_flat_search_multi_allow): k_list_dist computes the
compressor distance of every (query, listed row), k_list_heap runs the worker
heap over the compact lists.  Every row must equal, bit for bit, the one-query
wv_index_hnsw_flat_search under its own list -- ids, distances as uint32 bit
patterns, counts -- for BQ, PQ, SQ, rq-8 and rq-1, and last_scan_rows must be the
lists' size (a loop over the old entry point cannot pass that).  BQ is also
checked against the oracle's restatement directly."""
from concurrent.futures import ThreadPoolExecutor
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 24
ROUTE_LIST_SCAN = 12  # WV_ROUTE_LIST_SCAN
COMPS = ["bq", "pq", "sq", "rq8", "rq1"]

# (metric, variant, gen_matrix kind, n, d, k, PQ (segments, centroids)): what each reaches
SHAPES = {
    # integer data: total compressor ties (BQ codes all equal, SQ / RQ integer
    # ties), list order alone decides; SQ code padding (70 -> 80 bytes); PQ LUT
    # of 35 segments = one PQ_CH = 32 chunk + a 3-segment tail; 3037 = 11 * 256 + 221
    "int": ("l2-squared", "avx512", 1, 3037, 70, 8, (35, 32)),
    # normalisation; PQ ks = 256 with whole 16-segment groups
    "flt": ("cosine", "avx256", 0, 5005, 128, 10, (16, 256)),
    # lists of more than 64 chunks: k_list_heap's second window of chunk minima and its skip
    "long": ("dot", "avx256", 0, 20011, 64, 5, (16, 32)),
}
CASES = [(s, c) for s in ("int", "flt") for c in COMPS] + [("long", c) for c in ("bq", "sq", "rq8")]
RESCORE_LIMIT = 20  # SQ / RQ: >= k, so the trim applies; the worker heap's limit is searchTimeEF(k) = 100


def _raw_list(wv, ids):
    """an allow list handed over as given (AllowList() sorts and dedupes)"""
    a = wv.AllowList()
    a.ids = np.asarray(ids, dtype=np.uint64)
    return a


def _allow_lists(wv, name, n, k, deleted, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(NQ):
        kind = i % 15
        if kind == 0:
            out.append(None)
        elif kind == 1:  # every second id
            out.append(wv.AllowList(range(i % 2, n, 2)))
        elif kind == 2:  # a contiguous window of 800
            out.append(wv.AllowList(range(100, 900)))
        elif kind == 3:
            out.append(wv.AllowList(rng.choice(n, 30, replace=False)))
        elif kind == 4:
            out.append(wv.AllowList([int(rng.integers(0, n))]))
        elif kind == 5:  # only deleted and absent ids (at and past the high-water mark): count 0
            out.append(wv.AllowList(list(deleted[:4]) + [n, n + 10, n + 500]))
        elif kind == 6:  # the empty list
            out.append(wv.AllowList())
        elif kind == 7:  # 70 entries with duplicates, unsorted, one id past the rows
            v = rng.choice(n, 45, replace=False)
            out.append(_raw_list(wv, np.concatenate([v, v[::-1][:20], v[:4], [n + 3]])))
        elif kind == 8:  # more than k, fewer than the limit (100): the heap never fills
            out.append(wv.AllowList(rng.choice(n, 40, replace=False)))
        elif kind == 9:  # fewer than k
            out.append(wv.AllowList(rng.choice(n, max(k - 3, 1), replace=False)))
        elif kind in (10, 11, 12, 13):  # chunk edges
            out.append(wv.AllowList(rng.choice(n, {10: 255, 11: 256, 12: 257, 13: 600}[kind], replace=False)))
        else:  # ends in the last, partial code tile
            out.append(wv.AllowList(range(n - 300, n)))
    if name == "long":  # > 64 chunks of 256 entries
        out[3] = wv.AllowList(i for i in range(n) if i % 97 != 0)
        out[8] = wv.AllowList(rng.choice(n, 16500, replace=False))
        out[9] = wv.AllowList(rng.choice(n, 17000, replace=False))
    return out


def _make(wv, name, comp, rescore_limit=RESCORE_LIMIT):
    metric, variant, kind, n, d, k, pq = SHAPES[name]
    kw = dict(distance=metric, variant=variant)
    if comp == "bq":
        kw["bq"] = True
    elif comp == "sq":
        kw.update(sq=True, rescore_limit=rescore_limit)
    elif comp in ("rq8", "rq1"):
        kw.update(rq={"bits": 8 if comp == "rq8" else 1}, rescore_limit=rescore_limit)
    else:
        kw["pq"] = {"segments": pq[0], "centroids": pq[1], "trainingLimit": 100000, "rescore": True}
    return wv.FlatIndex(**kw)


def _fill(wv, oracle, idx, name, comp, fit=True):
    """rows added, quantizer fitted, some rows deleted, a few upserted"""
    metric, variant, kind, n, d, k, pq = SHAPES[name]
    data = _DATA.setdefault(name, oracle.gen_matrix(kind, 900 + d, 0, n, d))
    idx.add_batch(np.arange(n, dtype=np.uint64), data)
    if fit and comp == "sq":
        idx.sq_fit(0)
    elif fit and comp == "pq":
        idx.pq_fit(seed=9)
    deleted = list(range(5, n, 97))
    idx.delete(*deleted)
    up = oracle.gen_matrix(kind, 902 + d, 0, 3, d)
    for j, row in enumerate((1234, 17, n - 2)):
        idx.add(row, up[j])
    return data, deleted, up


_DATA = {}
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c["idx"].close()
    _CASES.clear()
    _DATA.clear()


def _one_query_rows(idx, queries, k, allows):
    return [idx.hnsw_flat_search(queries[i:i + 1], k, allow=allows[i]) for i in range(len(allows))]


def _case(wv, oracle, name, comp):
    """index of a (shape, compressor), its 24 queries and lists, and the rows of
    the one-query calls under the default options -- built once, read only"""
    if (name, comp) in _CASES:
        return _CASES[(name, comp)]
    metric, variant, kind, n, d, k, pq = SHAPES[name]
    idx = _make(wv, name, comp)
    data, deleted, up = _fill(wv, oracle, idx, name, comp)
    queries = oracle.gen_matrix(kind, 901 + d, 0, NQ, d)
    allows = _allow_lists(wv, name, n, k, deleted, 900 + d)
    one = _one_query_rows(idx, queries, k, allows)
    c = dict(idx=idx, queries=queries, allows=allows, one=one, k=k, n=n, d=d, data=data, deleted=deleted, up=up)
    _CASES[(name, comp)] = c
    return c


def _scan_rows(allows, n):
    """the sum over listed queries of distinct in-range ids, present or not"""
    return sum(int(np.unique(a.ids[a.ids < n]).size) for a in allows if a is not None)


def _check_rows(res, one, tag, sel=None):
    ids, dists, counts = res
    for j, i in enumerate(range(len(one)) if sel is None else sel):
        ei, ed, ec = one[i]
        m = int(counts[j])
        assert m == int(ec[0]), f"{tag} q{i}: count {m} vs one-query {int(ec[0])}"
        np.testing.assert_array_equal(ids[j, :m], ei[0, :m], err_msg=f"{tag} q{i} ids")
        np.testing.assert_array_equal(dists[j, :m].view(np.uint32), ed[0, :m].view(np.uint32), err_msg=f"{tag} q{i} dists")


@pytest.mark.parametrize("name,comp", CASES)
def test_list_search_equals_one_query_calls(wv, oracle, name, comp):
    c = _case(wv, oracle, name, comp)
    idx = c["idx"]
    res = idx.hnsw_flat_search_multi_allow(c["queries"], c["k"], c["allows"])
    st = idx.stats()
    _check_rows(res, c["one"], f"{name} {comp}")
    assert st["last_route"] == ROUTE_LIST_SCAN
    assert st["last_scan_rows"] == _scan_rows(c["allows"], c["n"])
    # the lists' kinds did what they are there for
    counts = res[2]
    for i in range(NQ):
        if i % 15 in (5, 6):
            assert counts[i] == 0
        elif i % 15 == 4:
            assert counts[i] <= 1
    assert counts[0] == c["k"]


@pytest.mark.parametrize("name", ["int", "flt"])
@pytest.mark.parametrize("comp", COMPS)
def test_list_search_settings(wv, oracle, name, comp):
    """ef = 16 (the worker heap's limit drops from 100 to 16: the heap fills and
    the chunk skip runs on every list) and hnsw_rescore = 0 (limit = k,
    compressor distances returned), against the one-query calls under the same
    options; for SQ / RQ also rescore_limit 0, where no rescoring happens (the
    shared index has rescore_limit 20 >= k, where the trim applies)"""
    c = _case(wv, oracle, name, comp)
    idx, k = c["idx"], c["k"]
    for opt, val, back in (("ef", 16, -1), ("hnsw_rescore", 0, 1)):
        idx.set_option(opt, val)
        try:
            one = _one_query_rows(idx, c["queries"], k, c["allows"])
            res = idx.hnsw_flat_search_multi_allow(c["queries"], k, c["allows"])
            assert idx.stats()["last_route"] == ROUTE_LIST_SCAN
        finally:
            idx.set_option(opt, back)
        _check_rows(res, one, f"{name} {comp} {opt}={val}")
        if opt == "hnsw_rescore":  # other distances than the rescored ones, or the setting did nothing
            assert any(not np.array_equal(res[1][i].view(np.uint32), c["one"][i][1][0].view(np.uint32)) for i in (1, 2))
    if comp in ("sq", "rq8", "rq1"):
        idx0 = _make(wv, name, comp, rescore_limit=0)
        try:
            _fill(wv, oracle, idx0, name, comp)
            one = _one_query_rows(idx0, c["queries"], k, c["allows"])
            res = idx0.hnsw_flat_search_multi_allow(c["queries"], k, c["allows"])
            _check_rows(res, one, f"{name} {comp} rescore_limit=0")
        finally:
            idx0.close()


def test_list_search_bq_equals_oracle(wv, oracle):
    """BQ on the float shape against the oracle itself: hamming distances from
    oracle.bq_encode + oracle.hamming_bitwise, exact ones from
    oracle.single_dist, the rows from oracle.hnsw_flat_search.  At least one of
    the four listed queries has equal hamming distances at places limit and
    limit + 1 of its own list, where the heap's order decides who stays."""
    name, comp = "flt", "bq"
    c = _case(wv, oracle, name, comp)
    metric, variant, kind, n, d, k, pq = SHAPES[name]
    m = oracle.METRIC[metric]
    store = c["data"].copy()
    present = np.ones(n, np.uint8)
    present[c["deleted"]] = 0
    for j, row in enumerate((1234, 17, n - 2)):
        store[row] = c["up"][j]
        present[row] = 1
    store = np.stack([oracle.normalize(x) for x in store])
    codes = [oracle.bq_encode(x) for x in store]
    sel = [1, 2, 16, 17]  # every second id (both parities) and the window of 800
    limit = oracle.search_time_ef(k)
    assert limit == 100
    tie = []
    res = c["idx"].hnsw_flat_search_multi_allow(c["queries"][sel], k, [c["allows"][i] for i in sel])
    for j, i in enumerate(sel):
        qn = oracle.normalize(c["queries"][i])
        cq = oracle.bq_encode(qn)
        cd = np.array([oracle.hamming_bitwise(cq, x) for x in codes], np.float32)
        ed = np.array([oracle.single_dist(m, oracle.AVX256, x, qn) for x in store], np.float32)
        own = np.zeros(n, np.uint8)
        own[c["allows"][i].ids.astype(np.int64)] = 1
        own &= present
        assert own.sum() > limit
        srt = np.sort(cd[own.astype(bool)])
        tie.append(bool(srt[limit - 1] == srt[limit]))
        ei, ed_ = oracle.hnsw_flat_search(cd, ed, own, k, limit, True, 0)
        cnt = int(res[2][j])
        assert cnt == len(ei)
        np.testing.assert_array_equal(res[0][j, :cnt], ei, err_msg=f"q{i} ids vs oracle")
        np.testing.assert_array_equal(res[1][j, :cnt].view(np.uint32), ed_.view(np.uint32), err_msg=f"q{i} dists vs oracle")
    assert any(tie), tie


@pytest.mark.parametrize("comp", ["bq", "sq", "rq8"])
def test_list_search_launch_groups(wv, oracle, comp):
    """hnsw_list_rows = 4096 on the long shape: several launch groups, both
    distance buffers reused, and three lists longer than the budget that get a
    group each.  The rows do not change."""
    c = _case(wv, oracle, "long", comp)
    idx = c["idx"]
    sizes = [np.unique(a.ids[a.ids < c["n"]]).size for a in c["allows"] if a is not None]
    assert sum(s > 4096 for s in sizes) >= 3 and sum(-(-s // 256) * 256 for s in sizes) > 6 * 4096
    idx.set_option("hnsw_list_rows", 4096)
    try:
        res = idx.hnsw_flat_search_multi_allow(c["queries"], c["k"], c["allows"])
        st = idx.stats()
    finally:
        idx.set_option("hnsw_list_rows", 0)
    _check_rows(res, c["one"], f"long {comp} groups")
    assert st["last_route"] == ROUTE_LIST_SCAN and st["last_scan_rows"] == _scan_rows(c["allows"], c["n"])


@pytest.mark.parametrize("comp", COMPS)
def test_hnsw_list_option_same_bits(wv, oracle, comp):
    """the existing one-list call with option hnsw_list 0 and 1: identical bits,
    and 1 reports the list route with one stored list scanned per query"""
    c = _case(wv, oracle, "flt", comp)
    idx, k, n = c["idx"], c["k"], c["n"]
    rng = np.random.default_rng(5)
    allow = _raw_list(wv, np.concatenate([rng.choice(n, 1500, replace=False), np.arange(200, 700), [n + 7]]))
    idx.hnsw_flat_search_multi_allow(c["queries"][:1], k, [wv.AllowList([3, 4])])
    assert idx.stats()["last_scan_rows"] == 2
    a = idx.hnsw_flat_search(c["queries"], k, allow=allow)
    assert idx.stats()["last_scan_rows"] == 2  # option 0: not the list path, which would have counted its entries
    idx.set_option("hnsw_list", 1)
    try:
        b = idx.hnsw_flat_search(c["queries"], k, allow=allow)
        st = idx.stats()
    finally:
        idx.set_option("hnsw_list", 0)
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert st["last_route"] == ROUTE_LIST_SCAN
    assert st["last_scan_rows"] == NQ * np.unique(allow.ids[allow.ids < n]).size


def _raw_call(idx, queries, k, allows):
    """the C entry with sentinel-filled outputs -> (rc, ids, dists, counts)"""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    nq, d = q.shape
    kk = max(k, 1)
    ids = np.full((nq, kk), 0xABCD, np.uint64)
    dists = np.full((nq, kk), -7.0, np.float32)
    counts = np.full(nq, -3, np.int32)
    modes = np.array([0 if a is None else 1 for a in allows], dtype=np.int32)
    parts = [np.asarray(a.ids, dtype=np.uint64) for a in allows if a is not None]
    aids = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.uint64)]))
    off = np.zeros(nq + 1, dtype=np.int64)
    off[1:] = np.cumsum([0 if a is None else a.ids.size for a in allows])
    rc = idx._l.wv_index_hnsw_flat_search_multi_allow(
        idx._h, q.ctypes.data_as(C.POINTER(C.c_float)), nq, d, int(k), aids.ctypes.data_as(C.POINTER(C.c_uint64)),
        off.ctypes.data_as(C.c_void_p), modes.ctypes.data_as(C.POINTER(C.c_int32)),
        ids.ctypes.data_as(C.POINTER(C.c_uint64)), dists.ctypes.data_as(C.POINTER(C.c_float)),
        counts.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, ids, dists, counts


def _same_error(wv, idx, queries, k, allows):
    """the batch fails with the one-query call's code and text, no output written"""
    with pytest.raises(wv.WeaviateError) as one:
        idx.hnsw_flat_search(queries[:1], k, allow=allows[0])
    rc, ids, dists, counts = _raw_call(idx, queries, k, allows)
    assert rc == one.value.code and rc != 0
    assert idx._l.wv_last_error().decode() == str(one.value)
    assert (ids == 0xABCD).all() and (dists == -7.0).all() and (counts == -3).all()
    with pytest.raises(wv.WeaviateError) as multi:
        idx.hnsw_flat_search_multi_allow(queries, k, allows)
    assert multi.value.code == one.value.code and str(multi.value) == str(one.value)
    return str(one.value)


def test_list_search_errors(wv, oracle):
    c = _case(wv, oracle, "flt", "sq")
    n, d = c["n"], c["d"]
    allows = [wv.AllowList(range(10, 400)), wv.AllowList(range(0, n, 3)), wv.AllowList([5, 6])]
    q = c["queries"][:3]
    assert "vector lengths don't match" in _same_error(wv, c["idx"], np.ascontiguousarray(q[:, :d - 1]), 5, allows)
    assert "k must be positive" in _same_error(wv, c["idx"], q, 0, allows)
    for comp in ("pq", "sq"):  # untrained PQ / unfitted SQ
        idx = _make(wv, "flt", comp)
        try:
            _fill(wv, oracle, idx, "flt", comp, fit=False)
            assert "quantizer not initialized" in _same_error(wv, idx, q, 5, allows)
        finally:
            idx.close()
    metric, variant, kind, _, _, _, _ = SHAPES["flt"]
    plain = wv.FlatIndex(distance=metric, variant=variant)
    try:
        plain.add_batch(np.arange(50, dtype=np.uint64), c["data"][:50])
        assert "not compressed" in _same_error(wv, plain, q, 5, allows)
    finally:
        plain.close()


def test_list_search_threads(wv, oracle):
    """four threads on one index, each with its own batch: each gets what it gets alone"""
    c = _case(wv, oracle, "flt", "rq8")
    idx, k = c["idx"], c["k"]
    parts = [list(range(t, NQ, 4)) for t in range(4)]

    def run(sel):
        return idx.hnsw_flat_search_multi_allow(c["queries"][sel], k, [c["allows"][i] for i in sel])

    alone = [run(sel) for sel in parts]
    for sel, res in zip(parts, alone):
        _check_rows(res, c["one"], "alone", sel)
    for _ in range(3):
        with ThreadPoolExecutor(4) as ex:
            got = list(ex.map(run, parts))
        for sel, res, ref in zip(parts, got, alone):
            _check_rows(res, c["one"], "threads", sel)
            np.testing.assert_array_equal(res[2], ref[2])
