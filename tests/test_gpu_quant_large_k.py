"""GPU: the compressed searches' final stages above 64 KiB of dynamic LDS.
k_bq_final holds 12 k + 16 bytes, k_pq_rescore_final 12 (k + 1) + 16 and
k_pq_finish 12 R + 16: all three cross 65,536 at k (or R) = 5,461, where their
launchers have to raise the kernel's dynamic-LDS limit first.  n = 6,000 rows,
d = 64, 3 queries, k = 5,500 with the rescore limit at its default (R = k) are
the smallest shapes that get there.  Every index type is compared with the
oracle as its own tests do (ids and distance bits), and a 2-shard multi index
(multi.hip's launches of the same kernels) with the single index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K, NQ = 6000, 64, 5500, 3


def bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32),
                                  err_msg=msg)


@pytest.fixture(scope="module")
def corpus(oracle):
    data = oracle.gen_matrix(0, 91, 0, N, D)
    queries = oracle.gen_matrix(0, 92, 0, NQ, D)
    data.setflags(write=False)
    queries.setflags(write=False)
    return data, queries


def _index_kw(comp):
    if comp == "bq":
        return dict(distance="cosine", bq=True)
    if comp == "rq8":
        return dict(distance="l2-squared", rq={"bits": 8})
    if comp == "sq":
        return dict(distance="l2-squared", sq=True)
    return dict(distance="l2-squared",
                pq={"segments": D // 4, "centroids": 32, "trainingLimit": 100000, "rescore": comp == "pq_rescore"})


def _single(wv, comp, data):
    idx = wv.FlatIndex(variant="avx256", **_index_kw(comp))
    idx.add_batch(np.arange(N, dtype=np.uint64), data)
    if comp == "sq":
        idx.sq_fit(2000)
    elif comp.startswith("pq"):
        idx.pq_fit(seed=5)
    return idx


def _check(got, qi, ei, ed, tag):
    ids, dists, counts = got
    assert counts[qi] == len(ei) == K, f"{tag} q{qi}"
    np.testing.assert_array_equal(ids[qi, :K], ei, err_msg=f"{tag} q{qi} ids")
    bits_equal(dists[qi, :K], ed, f"{tag} q{qi} dists")


def test_bq_large_k_equals_oracle(wv, oracle, corpus):
    data, queries = corpus
    idx = _single(wv, "bq", data)
    got = idx.search_by_vector_batch(queries, K)
    orc = oracle.OracleFlatBQ(oracle.COSINE, 1, D, N, -1)
    orc.add_batch(np.arange(N), data)
    for qi in range(NQ):
        rc, ei, ed = orc.search(queries[qi], K)
        assert rc == 0
        _check(got, qi, ei, ed, "bq")
    idx.close()


def test_rq8_large_k_equals_oracle(wv, oracle, corpus):
    data, queries = corpus
    idx = _single(wv, "rq8", data)
    got = idx.search_by_vector_batch(queries, K)
    orc = oracle.OracleFlatRQ(8, oracle.L2, 1, D, N, -1)
    orc.add_batch(np.arange(N, dtype=np.uint64), data)
    for qi in range(NQ):
        rc, ei, ed = orc.search(queries[qi], K)
        assert rc == 0
        _check(got, qi, ei, ed, "rq-8")
    idx.close()


def test_sq_rescored_large_k_equals_oracle(wv, oracle, corpus):
    """hnsw's flat branch: limit = searchTimeEF(k) = k here, rescoring on, no trim."""
    data, queries = corpus
    idx = _single(wv, "sq", data)
    got = idx.search_by_vector_batch(queries, K)
    info = idx.sq_info()
    sq = oracle.SQ(a=info["a"], b=info["b"], d=D)
    codes = [sq.encode(x) for x in data]
    present = np.ones(N, np.uint8)
    assert oracle.search_time_ef(K) == K
    for qi in range(NQ):
        cq = sq.encode(queries[qi])
        cd = np.array([sq.distance(oracle.L2, cq, c) for c in codes], np.float32)
        ed = np.array([oracle.single_dist(oracle.L2, 1, x, queries[qi]) for x in data], np.float32)
        ei, ed_ = oracle.hnsw_flat_search(cd, ed, present, K, K, True, 0)
        _check(got, qi, ei, ed_, "sq")
    idx.close()


@pytest.mark.parametrize("rescore", [True, False])
def test_pq_large_k_equals_oracle(wv, oracle, corpus, rescore):
    data, queries = corpus
    idx = _single(wv, "pq_rescore" if rescore else "pq", data)
    got = idx.search_by_vector_batch(queries, K)
    centers, codes = idx.pq_centers(), idx.pq_codes(N)
    present = np.ones(N, np.uint8)
    for qi in range(NQ):
        ei, ed = oracle.pq_flat_search(oracle.L2, 1, centers, codes, data, present, queries[qi], K, K, rescore)
        _check(got, qi, ei, ed, f"pq rescore={rescore}")
    idx.close()


# rq8 as well: its rescoring heap is multi_search_quant's k_bq_final launch (form 1)
@pytest.mark.parametrize("comp", ["bq", "sq", "rq8"])
def test_multi_large_k_equals_single_index(wv, corpus, comp):
    from weaviate_amd.multi import MultiFlatIndex
    data, queries = corpus
    single = _single(wv, comp, data)
    m = MultiFlatIndex(devices=[0, 0], id_stride=N // 2, transport="local", variant="avx256", dims=D, **_index_kw(comp))
    m.add_batch(np.arange(N, dtype=np.uint64), data)
    if comp == "sq":
        info = single.sq_info()
        for s in m.shards:
            s.sq_restore(info["a"], info["b"])
    gi, gd, gn = m.search_by_vector_batch(queries, K)
    ei, ed, en = single.search_by_vector_batch(queries, K)
    np.testing.assert_array_equal(gn, en, err_msg=f"{comp} counts")
    assert (gn == K).all()
    np.testing.assert_array_equal(gi, ei, err_msg=f"{comp} ids")
    bits_equal(gd, ed, f"{comp} dists")
    single.close()
    m.close()
