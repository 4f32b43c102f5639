"""GPU: per-query allow lists on a flat rq-8 / rq-1 index share one launch
(option pqa_rq).  The exact 32-row block minima (k_rq8_keys) and
the select run once over the union of the batch's lists; each query's
candidates (k_rq8_cand<.., PQA>) and, where they do not prove its R-list, its
R-heap replay (k_rq8_replay<.., PQA>) read its own bitmap.  Every query must
get, bit for bit, what the one-query call under its own list gives and what the
oracle's searchByVectorQuantized gives -- ids and distances, quantized ties at
the R-th place included."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 24

# (metric, gen_matrix kind, n, d, k, rescore_limit): what each reaches
SHAPES = {
    # integer data: quantized ties, so the replay's insertion order decides;
    # NC = 1, RT = 2, a partial last block (3037 = 94 * 32 + 29)
    "int": ("l2-squared", 1, 3037, 64, 8, 40),
    # odd chunk count (NC = 5), RT = 4; unlisted queries share the batch with
    # listed ones, so the union is every present row
    "flt": ("cosine", 0, 5005, 320, 10, 100),
    # two 512-block windows in k_rq8_replay (626 blocks): the window-minimum
    # skip and the second window run; the tail block is partial
    "two": ("dot", 0, 20011, 64, 5, 20),
}
CASES = [(name, bits) for name in SHAPES for bits in (8, 1)]
# gen_matrix seeds (data: seed, queries: seed + 1, the upsert: seed + 2; the
# lists' rng too).  The integer shape's give a listed query a quantized tie
# exactly at the R-th place of its own list: test_rq_multi_allow_tie_at_rth_place
# asserts it.
SEEDS = {("int", 8): 69, ("int", 1): 2600}


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


def _grouped_batches(allows):
    """pqa_rq = 0: one search per distinct list; lists that resolve to no row
    (kinds 5 and 6) answer without a search"""
    return _distinct(allows) - _distinct([a for i, a in enumerate(allows) if i % 10 in (5, 6)])


def _own_rows(c, i):
    """the present rows query i may see, ascending"""
    al = _ids_of(c["allows"][i])
    rows = range(c["n"]) if al is None else sorted(set(al))
    return [r for r in rows if r < c["n"] and c["orc"].present[r]]


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c["idx"].close()
    _CASES.clear()


def _case(wv, oracle, name, bits):
    """index + oracle of a shape, its 24 queries and lists, and the expected
    rows from both references -- built once, shared by the tests, read only"""
    if (name, bits) in _CASES:
        return _CASES[(name, bits)]
    metric, kind, n, d, k, R = SHAPES[name]
    seed = SEEDS.get((name, bits), 700 + d)
    data = oracle.gen_matrix(kind, seed, 0, n, d)
    queries = oracle.gen_matrix(kind, seed + 1, 0, NQ, d)
    ids = np.arange(n, dtype=np.uint64)
    idx = wv.FlatIndex(distance=metric, variant="avx256", rq={"bits": bits}, rescore_limit=R)
    idx.add_batch(ids, data)
    orc = oracle.OracleFlatRQ(bits, oracle.METRIC[metric], oracle.AVX256, d, n, R)
    orc.add_batch(ids, data)
    deleted = list(range(5, n, 97))
    idx.delete(*deleted)
    orc.delete(deleted)
    up = oracle.gen_matrix(kind, seed + 2, 0, 1, d)  # one upserted row
    idx.add(1234, up[0])
    orc.add_batch([1234], up)
    allows = _allow_lists(wv, n, NQ, k, max(R, k), deleted, seed)
    assert _distinct(allows) >= 6
    idx.set_option("pqa_rq", 0)
    one = [idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i]) for i in range(NQ)]
    idx.set_option("pqa_rq", 1)
    orows = []
    for i in range(NQ):
        rc, oi, od = orc.search(queries[i], k, _ids_of(allows[i]))
        assert rc == 0
        orows.append((oi, od))
    c = dict(idx=idx, orc=orc, queries=queries, allows=allows, one=one, orows=orows, k=k, R=max(R, k), n=n, d=d)
    _CASES[(name, bits)] = c
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


@pytest.mark.parametrize("name,bits", CASES)
def test_rq_multi_allow_equals_one_query_and_oracle(wv, oracle, name, bits):
    c = _case(wv, oracle, name, bits)
    idx = c["idx"]
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
    st = idx.stats()
    assert st["last_route"] == 10  # WV_ROUTE_RQ8_INT8
    assert st["batches"] - b0 == 1
    _check(c, res)


@pytest.mark.parametrize("name,bits", CASES)
def test_rq_multi_allow_shares_one_launch(wv, oracle, name, bits):
    """pqa_rq = 1: one search_rq batch for the 24 queries; 0: one per distinct list"""
    c = _case(wv, oracle, name, bits)
    idx = c["idx"]
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
    assert idx.stats()["batches"] - b0 == 1
    _check(c, res)
    idx.set_option("pqa_rq", 0)
    try:
        b0 = idx.stats()["batches"]
        res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
        grouped = idx.stats()["batches"] - b0
    finally:
        idx.set_option("pqa_rq", 1)
    assert grouped == _grouped_batches(c["allows"])
    _check(c, res)


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_multi_allow_proves_some_replays_some(wv, oracle, bits):
    """float shape, R = 100: a query whose list holds at most R present rows can
    never be proven from the union's keys (its (R+1)-th own candidate does not
    exist) and is replayed; an unlisted query whose R + 1 smallest quantized
    distances are distinct has the union as its own rows and must be proven"""
    c = _case(wv, oracle, "flt", bits)
    idx, orc, R = c["idx"], c["orc"], c["R"]
    short = sum(len(_own_rows(c, i)) <= R for i in range(NQ))
    assert 1 <= short < NQ
    present = np.flatnonzero(orc.present)
    provable = 0
    for i in range(NQ):
        if c["allows"][i] is None:
            dq = np.sort(orc.query_distances(c["queries"][i])[present])[: R + 1]
            provable += len(dq) == R + 1 and len(np.unique(dq)) == R + 1 and not np.isnan(dq).any()
    assert provable >= 1
    r0 = idx.stats()["replayed_queries"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
    rep = idx.stats()["replayed_queries"] - r0
    _check(c, res)
    assert rep >= short
    assert rep < NQ


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_multi_allow_listed_and_proven(wv, oracle, bits):
    """every query listed, all under the same dense window (800 ids, > R): the
    union is each query's own rows, so a query whose R + 1 smallest own
    quantized distances are distinct has R + 1 own candidates within M and must
    be proven by k_rq8_cand<.., PQA> -- no replay for it"""
    c = _case(wv, oracle, "flt", bits)
    idx, orc, R, k = c["idx"], c["orc"], c["R"], c["k"]
    window = wv.AllowList(range(100, 900))
    allows = [window] * NQ
    rows = [r for r in range(100, 900) if orc.present[r]]
    assert len(rows) > R + 1
    provable = 0
    for i in range(NQ):
        dq = np.sort(orc.query_distances(c["queries"][i])[rows])[: R + 1]
        provable += len(np.unique(dq)) == R + 1 and not np.isnan(dq).any()
    assert provable >= NQ // 2
    r0, b0 = idx.stats()["replayed_queries"], idx.stats()["batches"]
    ids, dists, counts = idx.search_by_vector_batch_multi_allow(c["queries"], k, allows)
    st = idx.stats()
    assert st["batches"] - b0 == 1 and st["last_route"] == 10
    assert st["replayed_queries"] - r0 <= NQ - provable
    for i in range(NQ):
        rc, oi, od = orc.search(c["queries"][i], k, list(range(100, 900)))
        assert rc == 0 and counts[i] == len(oi) == k
        np.testing.assert_array_equal(ids[i, :k], oi, err_msg=f"q{i} vs oracle")
        np.testing.assert_array_equal(dists[i, :k].view(np.uint32), od.view(np.uint32), err_msg=f"q{i} vs oracle")


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_multi_allow_tie_at_rth_place(wv, oracle, bits):
    """a property of the integer shape's inputs: some listed query with more
    than R present rows has, inside its own list, equal R-th and (R+1)-th
    quantized distances -- which of the tied rows the R-heap keeps is then
    decided by the replay's insertion order"""
    c = _case(wv, oracle, "int", bits)
    orc, R = c["orc"], c["R"]
    tied = 0
    for i in range(NQ):
        if c["allows"][i] is None:
            continue
        rows = _own_rows(c, i)
        if len(rows) <= R:
            continue
        dq = np.sort(orc.query_distances(c["queries"][i])[rows])
        tied += dq[R - 1] == dq[R]
    assert tied >= 1


@pytest.mark.parametrize("name,bits", CASES)
def test_rq_multi_allow_bitmap_form(wv, oracle, name, bits):
    c = _case(wv, oracle, name, bits)
    idx = c["idx"]
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"], bitmap=True)
    assert idx.stats()["batches"] - b0 == 1
    _check(c, res)


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_multi_allow_budget_splits(wv, oracle, bits):
    """pqa_budget_mb = 1: 200 bitmaps of 7.5 KB pass the budget (139 fit), so
    the batch runs as consecutive sub-batches (offsets q0 * k), one search_rq
    each; results stay equal"""
    metric, n, d, k, R, nq = "l2-squared", 60000, 64, 8, 40, 200
    data = oracle.gen_matrix(1, 977, 0, n, d)
    queries = oracle.gen_matrix(1, 978, 0, nq, d)
    ids = np.arange(n, dtype=np.uint64)
    idx = wv.FlatIndex(distance=metric, variant="avx256", rq={"bits": bits}, rescore_limit=R)
    idx.add_batch(ids, data)
    orc = oracle.OracleFlatRQ(bits, oracle.METRIC[metric], oracle.AVX256, d, n, R)
    orc.add_batch(ids, data)
    deleted = list(range(5, n, 97))
    idx.delete(*deleted)
    orc.delete(deleted)
    allows = _allow_lists(wv, n, nq, k, R, deleted, 979)
    idx.set_option("pqa_budget_mb", 1)
    qmax = (1 << 20) // ((n + 255) // 256 * 8 * 4)
    assert 1 < qmax < nq and nq % qmax > 1
    b0 = idx.stats()["batches"]
    res = idx.search_by_vector_batch_multi_allow(queries, k, allows)
    assert idx.stats()["batches"] - b0 == -(-nq // qmax)
    bres = idx.search_by_vector_batch_multi_allow(queries, k, allows, bitmap=True)
    idx.set_option("pqa_rq", 0)
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


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_multi_allow_fallbacks(wv, oracle, bits):
    """what the shared launch does not serve stays grouped and correct: the
    distance-matrix route (rq_mfma = 0) and k = 0, which reports the
    one-query call's error"""
    c = _case(wv, oracle, "flt", bits)
    idx = c["idx"]
    idx.set_option("rq_mfma", 0)
    try:
        b0 = idx.stats()["batches"]
        res = idx.search_by_vector_batch_multi_allow(c["queries"], c["k"], c["allows"])
        st = idx.stats()
    finally:
        idx.set_option("rq_mfma", 1)
    assert st["last_route"] != 10
    assert st["batches"] - b0 == _grouped_batches(c["allows"])
    _check(c, res)
    with pytest.raises(wv.WeaviateError) as one:
        idx.search_by_vector_batch(c["queries"][:1], 0)
    with pytest.raises(wv.WeaviateError) as many:
        idx.search_by_vector_batch_multi_allow(c["queries"], 0, c["allows"])
    assert str(many.value) == str(one.value)


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_batcher_coalesces_distinct_allow_lists(wv, oracle, bits):
    """48 concurrent one-query callers on the d = 320 index, 40 of them with
    pairwise distinct lists: the micro-batcher's launches go through the shared
    rq form with no code of its own -- every caller gets its one-query result,
    launches < calls, fewer search_rq batches than distinct lists, and a
    caller with a wrong dimension fails alone with the one-query error"""
    c = _case(wv, oracle, "flt", bits)
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
    idx.set_option("pqa_rq", 0)
    exp = [idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i]) for i in range(ncall)]
    idx.set_option("pqa_rq", 1)
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
