"""GPU: rq-8 / rq-1 above 1024 rotated dims on the integer matrix cores
(k_rq8_keys_cp: block keys in column parts, option rq_wide).
The route's results equal the distance-matrix route's (rq_wide 0) and the
oracle's searchByVectorQuantized bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32),
                                  err_msg=msg)


def build(wv, oracle, bits, metric, data, rescore):
    n, d = data.shape
    ids = np.arange(n, dtype=np.uint64)
    idx = wv.FlatIndex(distance=metric, variant="avx256", rq={"bits": bits}, rescore_limit=rescore)
    idx.add_batch(ids, data)
    idx.set_option("rq_wide", 1)
    orc = oracle.OracleFlatRQ(bits, oracle.METRIC[metric], 1, d, n, rescore)
    orc.add_batch(ids, data)
    return idx, orc


def check_oracle(orc, queries, qs, k, ids, dists, counts, allow=None):
    for q in qs:
        rc, oi, od = orc.search(queries[q], k, allow=allow)
        assert rc == 0 and counts[q] == len(oi), f"q{q}"
        np.testing.assert_array_equal(ids[q, :counts[q]], oi, err_msg=f"q{q}")
        bits_equal(dists[q, :counts[q]], od, f"q{q}")


@pytest.mark.parametrize("metric,kind,n,d,k,rescore,nq", [
    ("cosine", 0, 3191, 1088, 10, 63, 150),      # NC 17: a full part + a one-chunk part; R + 1 = 64
    ("cosine", 0, 3500, 1500, 10, 200, 150),     # D = 1536: rows padded by the rotation
    ("l2-squared", 1, 3333, 2048, 20, 100, 150), # NC 32, the last of the 128-query form; integer data
    ("dot", 0, 2999, 2112, 5, -1, 150),          # NC 33, the first of the 64-query form
    ("l2-squared", 0, 2501, 4000, 10, 63, 100),  # D = 4032, NC 63: the widest, ragged
])
@pytest.mark.parametrize("bits", [8, 1])
def test_rq_wide_route_equals_matrix_route_and_oracle(wv, oracle, bits, metric, kind, n, d, k, rescore, nq):
    data = oracle.gen_matrix(kind, 71, 0, n, d)
    queries = oracle.gen_matrix(kind, 72, 0, nq, d)
    queries[1] = data[17]  # a stored row
    queries[2] = 0         # the zero query
    idx, orc = build(wv, oracle, bits, metric, data, rescore)
    ids, dists, counts = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] == 10  # WV_ROUTE_RQ8_INT8
    idx.set_option("rq_wide", 0)
    ids0, dists0, counts0 = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] != 10
    np.testing.assert_array_equal(counts, counts0)
    np.testing.assert_array_equal(ids, ids0)
    bits_equal(dists, dists0, "wide vs distance-matrix route")
    check_oracle(orc, queries, range(0, nq, nq // 6), k, ids, dists, counts)
    idx.close()


@pytest.mark.parametrize("bits", [8, 1])
def test_rq_wide_duplicates_deletes_allow(wv, oracle, bits):
    n, d, k = 3001, 1536, 10
    data = oracle.gen_matrix(0, 73, 0, n, d)
    data[1000:1150] = data[999]  # 151 identical rows
    idx, orc = build(wv, oracle, bits, "l2-squared", data, 50)
    queries = np.concatenate([oracle.gen_matrix(0, 74, 0, 20, d), data[999:1000], data[2000:2001]])
    before = idx.stats()["replayed_queries"]
    ids, dists, counts = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] == 10
    assert idx.stats()["replayed_queries"] - before >= 1  # the duplicated row's query
    check_oracle(orc, queries, range(len(queries)), k, ids, dists, counts)
    dele = np.arange(3, n, 11, dtype=np.uint64)
    idx.delete(*dele)
    orc.delete(dele)
    ids, dists, counts = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] == 10
    check_oracle(orc, queries, range(len(queries)), k, ids, dists, counts)
    allow = np.arange(100, 2500, 2, dtype=np.uint64)
    for q in (0, 20, 21):
        gi, gd = idx.search_by_vector(queries[q], k, allow=wv.AllowList(allow))
        rc, oi, od = orc.search(queries[q], k, allow=allow)
        np.testing.assert_array_equal(gi, oi, err_msg=f"allow q{q}")
        bits_equal(gd, od, f"allow q{q}")
    idx.close()


def test_rq_wide_multi_allow_one_batch(wv, oracle):
    n, d, k, nq = 3001, 1536, 10, 12
    data = oracle.gen_matrix(0, 75, 0, n, d)
    queries = oracle.gen_matrix(0, 76, 0, nq, d)
    idx, _ = build(wv, oracle, 8, "cosine", data, 40)
    allows = [None if q % 4 == 0 else wv.AllowList(range(q, n, 2 + q % 3)) for q in range(nq)]
    allows[5] = wv.AllowList(range(50, 70))  # fewer rows than R: replayed
    b0 = idx.stats()["batches"]
    ids, dists, counts = idx.search_by_vector_batch_multi_allow(queries, k, allows)
    assert idx.stats()["batches"] - b0 == 1 and idx.stats()["last_route"] == 10
    for q in range(nq):
        gi, gd = idx.search_by_vector(queries[q], k, allow=allows[q])
        assert counts[q] == len(gi), f"q{q}"
        np.testing.assert_array_equal(ids[q, :counts[q]], gi, err_msg=f"q{q}")
        bits_equal(dists[q, :counts[q]], gd, f"q{q}")
    idx.close()
