"""hnsw flat search over SQ by exact block minima on the integer matrix cores
(option sq_keys = 1, route sq_int8) against today's
distance-matrix route (sq_keys = 0), bit for bit on every query, and against
the oracle's hnsw.flatSearch over oracle.SQ distances on six of them.
MI355X only (marker gpu).

The seeds were checked on the CPU with oracle.SQ: on the float data at least
243 of the 260 queries of every (shape, metric, ef) cell have strictly
increasing R + 1 smallest SQ distances over the allowed rows, so a key pass
that flags more than half of them is broken, not unlucky."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, K = 260, 10
SHAPES = [(3000, 64), (2075, 200), (1300, 1024)]  # NC = 1, a width off 16 and 64, NC = 16; partial last blocks
METRICS = ["l2-squared", "dot", "cosine"]
ORACLE_Q = (0, 1, 130, 255, 256, 259)


def corpus(oracle, kind, n, d):
    """data, queries, the allow list and the rows it leaves after two deletes:
    ids [64, 200) are outside the list (empty blocks and partly valid ones)"""
    data = oracle.gen_matrix(kind, 71, 0, n, d)
    queries = oracle.gen_matrix(kind, 72, 0, NQ, d)
    rng = np.random.default_rng(n + d)
    ids = np.arange(n)
    allow = np.sort(rng.choice(ids[(ids < 64) | (ids >= 200)], (n * 3) // 4, replace=False)).astype(np.uint64)
    deleted = (int(allow[5]), int(allow[-1]))
    present = np.zeros(n, np.uint8)
    present[allow.astype(np.int64)] = 1
    present[list(deleted)] = 0
    return data, queries, allow, deleted, present


def make(wv, metric, data, allow, deleted, rescore_limit=20):
    idx = wv.FlatIndex(distance=metric, variant="avx256", sq=True, rescore_limit=rescore_limit)
    idx.add_batch(np.arange(len(data), dtype=np.uint64), data)
    idx.sq_fit(0)
    idx.delete(*deleted)
    return idx, wv.AllowList(allow.tolist())


def both_routes(wv, idx, queries, allow):
    """(ids, distance bits, counts) of sq_keys = 0 and 1, and the queries the new route replayed"""
    out = []
    for arm in (0, 1):
        idx.set_option("sq_keys", arm)
        before = idx.stats()["replayed_queries"]
        ids, dists, counts = idx.hnsw_flat_search(queries, K, allow=allow)
        out.append((ids.copy(), dists.view(np.uint32).copy(), counts.copy()))
    assert wv._lib.ROUTES[idx.stats()["last_route"]] == "sq_int8"
    for a, b, what in zip(out[0], out[1], ("ids", "distances", "counts")):
        np.testing.assert_array_equal(b, a, err_msg=what)
    return out[1], idx.stats()["replayed_queries"] - before


def oracle_distances(oracle, metric, idx, data, queries):
    """per checked query: SQ distances and rescoring distances of every row"""
    m = oracle.METRIC[metric]
    norm = (lambda v: oracle.normalize(v)) if m == oracle.COSINE else (lambda v: v)
    store = [norm(x) for x in data]
    info = idx.sq_info()
    sq = oracle.SQ(a=info["a"], b=info["b"], d=data.shape[1])
    codes = [sq.encode(x) for x in store]
    res = {}
    for qi in ORACLE_Q:
        qn = norm(queries[qi])
        cq = sq.encode(qn)
        res[qi] = (np.array([sq.distance(m, cq, c) for c in codes], np.float32),
                   np.array([oracle.single_dist(m, 1, x, qn) for x in store], np.float32))
    return res


def check_oracle(oracle, got, od, present, rescore_limit, ef, rescore_on=True):
    ids, bits, counts = got
    rescore = rescore_on and rescore_limit != 0
    limit = oracle.search_time_ef(K, ef) if rescore else K
    trim = rescore_limit if rescore_limit >= K else 0
    for qi, (cd, ed) in od.items():
        ei, ed_ = oracle.hnsw_flat_search(cd, ed, present, K, limit, rescore, trim)
        assert counts[qi] == len(ei), qi
        np.testing.assert_array_equal(ids[qi, :len(ei)], ei, err_msg=f"q{qi}")
        np.testing.assert_array_equal(bits[qi, :len(ei)], ed_.view(np.uint32), err_msg=f"q{qi}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_sq_keys_equal_matrix_route_and_oracle(wv, oracle, metric, n, d):
    data, queries, allow, deleted, present = corpus(oracle, 0, n, d)
    idx, al = make(wv, metric, data, allow, deleted)
    od = oracle_distances(oracle, metric, idx, data, queries)
    for ef in (-1, 16):
        idx.set_option("ef", ef)
        got, replayed = both_routes(wv, idx, queries, al)
        print(f"{metric} {n}x{d} ef{ef}: replayed {replayed} of {NQ}")
        assert replayed <= NQ // 2  # the key pass and the candidates prove the others
        check_oracle(oracle, got, od, present, 20, ef)
    idx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_sq_keys_ties_are_replayed(wv, oracle, metric):
    n, d = 2075, 200
    data, queries, allow, deleted, present = corpus(oracle, 1, n, d)  # integer data: ties in every distance
    idx, al = make(wv, metric, data, allow, deleted)
    got, replayed = both_routes(wv, idx, queries, al)
    assert replayed > 0
    check_oracle(oracle, got, oracle_distances(oracle, metric, idx, data, queries), present, 20, -1)
    idx.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("rescore_limit,rescore_on", [(-1, False), (0, True), (300, True)])
def test_sq_keys_rescore_variants(wv, oracle, metric, rescore_limit, rescore_on):
    """doNotRescore (limit = k, SQ distances returned), rescore limit 0, trimming"""
    n, d = 2075, 200
    data, queries, allow, deleted, present = corpus(oracle, 0, n, d)
    idx, al = make(wv, metric, data, allow, deleted, rescore_limit)
    idx.set_option("hnsw_rescore", int(rescore_on))
    got, _ = both_routes(wv, idx, queries, al)
    check_oracle(oracle, got, oracle_distances(oracle, metric, idx, data, queries), present, rescore_limit, -1,
                 rescore_on)
    idx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_sq_keys_plane_follows_writes_and_growth(wv, oracle, metric):
    """the signed plane is built at the first search; rows rewritten in place
    and rows added past the first capacity reach it before the next one"""
    n, d = 2075, 200
    data, queries, allow, deleted, _ = corpus(oracle, 0, n, d)
    idx, _ = make(wv, metric, data, allow, deleted)
    both_routes(wv, idx, queries, None)
    idx.add_batch(np.arange(300, 340, dtype=np.uint64), oracle.gen_matrix(0, 73, 0, 40, d))
    both_routes(wv, idx, queries, None)
    more = oracle.gen_matrix(0, 74, 0, 3000, d)
    idx.add_batch(np.arange(n, n + 3000, dtype=np.uint64), more)
    got, _ = both_routes(wv, idx, queries, None)
    assert (got[0][:, :K] >= n).any()  # the new rows are found
    idx.close()
