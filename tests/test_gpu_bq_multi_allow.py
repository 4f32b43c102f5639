"""GPU: per-query allow lists on a flat + BQ index share one launch (option
pqa_bq).  The block minima run once over the union of the
batch's lists; each query's R-heap replay (k_bq_replay<..., PQA>) reads its own
bitmap.  Every query must get, bit for bit, what the one-query call under its
own list gives and what the oracle's searchByVectorQuantized gives -- ids and
distances, hamming ties at the R-th place included."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 24

# (metric, gen_matrix kind, n, d, k, rescore_limit, shift): what each reaches
SHAPES = {
    # 1 word, VALU 256-row minima, NW = 2.  gen_matrix kind 1 is U{0..127}: no
    # negative component, every code 0, every hamming distance 0 -- the R-heap is
    # decided by the tie order alone (the first R own rows, by id)
    "w1_valu": ("l2-squared", 1, 3037, 64, 8, 40, 0.0),
    # the same integers centred (U{-64..63}): hamming distances 0..64 over 3000
    # rows, so ties at every place and blocks the heap's top lets the replay skip
    "w1_cent": ("l2-squared", 1, 3037, 64, 8, 40, 64.0),
    "w8_int8": ("cosine", 0, 5005, 512, 10, 64, 0.0),      # 8 words, int8 32-row minima, pipelined replay
    "w16_pad": ("dot", 0, 4100, 1000, 10, 30, 0.0),        # 16 words, zero-padded plane columns
    "w33_gen": ("l2-squared", 0, 2100, 2112, 5, 20, 0.0),  # 33 words: the generic NW = 0 kernels
}


def _raw_list(wv, ids):
    """an allow list handed over as given (AllowList() sorts and dedupes)"""
    a = wv.AllowList()
    a.ids = np.asarray(ids, dtype=np.uint64)
    return a


def _allow_lists(wv, n, nq, k, R, deleted, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nq):
        kind = i % 10
        if kind == 0:
            out.append(None)
        elif kind == 1:  # every second id
            out.append(wv.AllowList(range(i % 2, n, 2)))
        elif kind == 2:  # a contiguous window
            out.append(wv.AllowList(range(100, 900)))
        elif kind == 3:  # 30 random ids
            out.append(wv.AllowList(rng.choice(n, 30, replace=False)))
        elif kind == 4:  # one id
            out.append(wv.AllowList([int(rng.integers(0, n))]))
        elif kind == 5:  # only deleted and absent ids: count 0
            out.append(wv.AllowList(list(deleted[:4]) + [n + 10, n + 500]))
        elif kind == 6:  # the empty list: count 0 (flat/index.go:590-594)
            out.append(wv.AllowList())
        elif kind == 7:  # duplicates, unsorted
            v = rng.choice(n, 50, replace=False)
            out.append(_raw_list(wv, np.concatenate([v, v[::-1][:20], v[:5]])))
        elif kind == 8:  # shorter than R: the heap never fills
            out.append(wv.AllowList(rng.choice(n, max(R // 2, k + 1), replace=False)))
        else:  # shorter than k
            out.append(wv.AllowList(rng.choice(n, max(k - 3, 1), replace=False)))
    return out


def _ids_of(a):
    return None if a is None else [int(x) for x in a.ids]


def _distinct(allows):
    return len({None if a is None else a.ids.tobytes() for a in allows})


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c["idx"].close()
    _CASES.clear()


def _case(wv, oracle, name):
    """index + oracle of a shape, its 24 queries and lists, and the expected
    rows from both references -- built once, shared by the tests, read only"""
    if name in _CASES:
        return _CASES[name]
    metric, kind, n, d, k, R, shift = SHAPES[name]
    seed = 900 + d
    data = oracle.gen_matrix(kind, seed, 0, n, d) - np.float32(shift)
    queries = oracle.gen_matrix(kind, seed + 1, 0, NQ, d) - np.float32(shift)
    ids = np.arange(n, dtype=np.uint64)
    idx = wv.FlatIndex(distance=metric, variant="avx256", bq=True, rescore_limit=R)
    idx.add_batch(ids, data)
    orc = oracle.OracleFlatBQ(oracle.METRIC[metric], oracle.AVX256, d, n, R)
    orc.add_batch(ids, data)
    deleted = list(range(5, n, 97))
    idx.delete(*deleted)
    orc.delete(deleted)
    up = oracle.gen_matrix(kind, seed + 2, 0, 1, d) - np.float32(shift)  # one upserted row
    idx.add(1234, up[0])
    orc.add_batch([1234], up)
    allows = _allow_lists(wv, n, NQ, k, max(R, k), deleted, seed)
    assert _distinct(allows) >= 6
    idx.set_option("pqa_bq", 0)
    one = [idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i]) for i in range(NQ)]
    idx.set_option("pqa_bq", 1)
    orows = []
    for i in range(NQ):
        rc, oi, od = orc.search(queries[i], k, _ids_of(allows[i]))
        assert rc == 0
        orows.append((oi, od))
    c = dict(idx=idx, orc=orc, queries=queries, allows=allows, one=one, orows=orows, k=k, R=max(R, k), n=n, d=d)
    _CASES[name] = c
    return c


def _check(c, res, sel=None):
    ids, dists, counts = res
    for j, i in enumerate(range(NQ) if sel is None else sel):
        ei, ed, ec = c["one"][i]
        oi, od = c["orows"][i]
        m = int(counts[j])
        assert m == ec[0] == len(oi), f"q{i}: {m} vs one-query {ec[0]} vs oracle {len(oi)}"
        np.testing.assert_array_equal(ids[j, :m], ei[0, :m], err_msg=f"q{i} vs one-query")
        np.testing.assert_array_equal(dists[j, :m].view(np.uint32), ed[0, :m].view(np.uint32), err_msg=f"q{i} vs one-query")
        np.testing.assert_array_equal(ids[j, :m], oi, err_msg=f"q{i} vs oracle")
        np.testing.assert_array_equal(dists[j, :m].view(np.uint32), od.view(np.uint32), err_msg=f"q{i} vs oracle")
    for i in range(NQ):
        if i % 10 in (5, 6):
            assert len(c["orows"][i][0]) == 0


@pytest.mark.parametrize("name,opts", [("w1_valu", {}), ("w1_cent", {}), ("w8_int8", {}), ("w8_int8", {"bq8": 0}), ("w16_pad", {}),
                                       ("w33_gen", {})])
def test_bq_multi_allow_equals_one_query_and_oracle(wv, oracle, name, opts):
    c = _case(wv, oracle, name)
    idx = c["idx"]
    for kk, vv in opts.items():
        idx.set_option(kk, vv)
    try:
        b0 = idx.stats()["batches"]
        res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
        assert idx.stats()["batches"] - b0 == 1
    finally:
        for kk in opts:
            idx.set_option(kk, 1)
    _check(c, res)


@pytest.mark.parametrize("name", ["w1_valu", "w1_cent"])
def test_bq_multi_allow_tie_at_rth_place(wv, oracle, name):
    """a property of the integer shapes' inputs: some query has, inside its own
    list, a hamming tie at the R-th place -- which of the tied rows the R-heap
    keeps is then decided by the replay's insertion order"""
    c = _case(wv, oracle, name)
    orc, R = c["orc"], c["R"]
    tied = 0
    for i in range(NQ):
        al = _ids_of(c["allows"][i])
        rows = [r for r in (range(c["n"]) if al is None else sorted(set(al))) if r < c["n"] and orc.present[r]]
        if len(rows) <= R:
            continue
        qc = oracle.bq_encode(c["queries"][i])
        h = sorted(oracle.hamming_bitwise(qc, orc.codes[r]) for r in rows)
        tied += h[R - 1] == h[R]
    assert tied >= 1


@pytest.mark.parametrize("name", ["w1_valu", "w1_cent", "w8_int8"])
def test_bq_multi_allow_shares_one_launch(wv, oracle, name):
    """pqa_bq = 1: one search_bq batch for the 24 queries; 0: one per distinct list"""
    c = _case(wv, oracle, name)
    idx = c["idx"]
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
    assert idx.stats()["batches"] - b0 == 1
    _check(c, res)
    idx.set_option("pqa_bq", 0)
    try:
        b0 = idx.stats()["batches"]
        res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
        grouped = idx.stats()["batches"] - b0
    finally:
        idx.set_option("pqa_bq", 1)
    # lists that resolve to no row answer without a search (kinds 5 and 6)
    nolaunch = _distinct([a for i, a in enumerate(c["allows"]) if i % 10 in (5, 6)])
    assert grouped == _distinct(c["allows"]) - nolaunch
    _check(c, res)


@pytest.mark.parametrize("name", ["w1_valu", "w8_int8", "w33_gen"])
def test_bq_multi_allow_bitmap_form(wv, oracle, name):
    c = _case(wv, oracle, name)
    idx = c["idx"]
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"], bitmap=True)
    assert idx.stats()["batches"] - b0 == 1
    _check(c, res)


def test_bq_multi_allow_budget_splits(wv, oracle):
    """pqa_budget_mb = 1: 150 bitmaps of 15 KB pass the budget (69 fit), so the
    batch runs as consecutive sub-batches (offsets q0 * k); results stay equal"""
    metric, n, d, k, R, nq = "l2-squared", 120000, 64, 8, 40, 150
    data = oracle.gen_matrix(1, 977, 0, n, d) - np.float32(64)  # centred integers: ties, not all of them
    queries = oracle.gen_matrix(1, 978, 0, nq, d) - np.float32(64)
    ids = np.arange(n, dtype=np.uint64)
    idx = wv.FlatIndex(distance=metric, variant="avx256", bq=True, rescore_limit=R)
    idx.add_batch(ids, data)
    orc = oracle.OracleFlatBQ(oracle.METRIC[metric], oracle.AVX256, d, n, R)
    orc.add_batch(ids, data)
    deleted = list(range(5, n, 97))
    idx.delete(*deleted)
    orc.delete(deleted)
    allows = _allow_lists(wv, n, nq, k, R, deleted, 979)
    idx.set_option("pqa_budget_mb", 1)
    qmax = (1 << 20) // ((n + 255) // 256 * 8 * 4)
    assert 1 < qmax < nq
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(queries, k, allows)
    assert idx.stats()["batches"] - b0 == -(-nq // qmax)
    bres = idx.search_by_vector_batch_multi_allow(queries, k, allows, bitmap=True)
    idx.set_option("pqa_bq", 0)
    for i in range(nq):
        ei, ed, ec = idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i])
        rc, oi, od = orc.search(queries[i], k, _ids_of(allows[i]))
        assert rc == 0
        for ri, rd, rn in (res, bres):
            m = int(rn[i])
            assert m == ec[0] == len(oi), f"q{i}"
            np.testing.assert_array_equal(ri[i, :m], ei[0, :m], err_msg=f"q{i}")
            np.testing.assert_array_equal(rd[i, :m].view(np.uint32), ed[0, :m].view(np.uint32), err_msg=f"q{i}")
            np.testing.assert_array_equal(ri[i, :m], oi, err_msg=f"q{i} vs oracle")
            np.testing.assert_array_equal(rd[i, :m].view(np.uint32), od.view(np.uint32), err_msg=f"q{i} vs oracle")
    idx.close()


def test_bq_batcher_coalesces_distinct_allow_lists(wv, oracle):
    """48 concurrent one-query callers on the d = 512 index, 40 of them with
    pairwise distinct lists: the micro-batcher's launches go through the shared
    BQ form with no code of its own -- every caller gets its one-query result,
    launches < calls, fewer search_bq batches than distinct lists, and a
    caller with a wrong dimension fails alone with the one-query error"""
    c = _case(wv, oracle, "w8_int8")
    idx, k, n, d = c["idx"], c["k"], c["n"], c["d"]
    rng = np.random.default_rng(41)
    ncall = 48
    queries = oracle.gen_matrix(0, 990, 0, ncall, d)
    allows = []
    for i in range(ncall):
        if i < 40:  # pairwise distinct: sizes from 1 to dense
            sz = [1, 7, 30, 200, n // 2][i % 5] + i
            allows.append(wv.AllowList(rng.choice(n, sz, replace=False)))
        else:
            allows.append(None)
    assert _distinct(allows[:40]) == 40
    exp = [idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i]) for i in range(ncall)]
    for i in range(0, ncall, 5):
        rc, oi, od = c["orc"].search(queries[i], k, _ids_of(allows[i]))
        np.testing.assert_array_equal(exp[i][0][0, :exp[i][2][0]], oi)
        np.testing.assert_array_equal(exp[i][1][0, :exp[i][2][0]].view(np.uint32), od.view(np.uint32))
    try:
        idx.search_by_vector_batch(np.ones((1, d + 64), np.float32), k)
        one_err = None
    except wv.WeaviateError as e:
        one_err = str(e)
    assert one_err is not None
    idx.set_option("batch_window_us", 3000)
    s0, b0 = idx.batcher_stats(), idx.stats()["batches"]

    def one(i):
        if i == ncall:  # wrong dimension: fails alone
            try:
                idx.search_by_vector(np.ones(d + 64, np.float32), k)
            except wv.WeaviateError as e:
                return str(e)
            return None
        return idx.search_by_vector(queries[i], k, allow=allows[i])

    with ThreadPoolExecutor(ncall + 1) as ex:
        res = list(ex.map(one, range(ncall + 1)))
    s1, b1 = idx.batcher_stats(), idx.stats()["batches"]
    idx.set_option("batch_window_us", 1000)  # the default
    assert res[ncall] == one_err
    for i in range(ncall):
        ei, ed, ec = exp[i]
        np.testing.assert_array_equal(res[i][0], ei[0, :ec[0]], err_msg=f"q{i}")
        np.testing.assert_array_equal(res[i][1].view(np.uint32), ed[0, :ec[0]].view(np.uint32), err_msg=f"q{i}")
    assert s1["launches"] - s0["launches"] < s1["calls"] - s0["calls"], (s0, s1)
    assert b1 - b0 < 40, (b0, b1)
