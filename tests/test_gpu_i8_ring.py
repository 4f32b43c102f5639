"""The edges of the LDS-DMA ring of k_rq8_keys and k_sq_keys (i8_ring_keys,
DESIGN §3.7b / §3.10c): corpora of 1, 3 and 10 32-row blocks
with a partial last block, all in one span, at the ring's two depths (64
columns: 8 slots, 6 blocks ahead; 1024 columns: 4 slots, 2 ahead).  That is
fewer steps than the prologue issues, exactly one step, and a ring that wraps
once at the deep end and twice at the shallow one.  Five queries (one partly
padded group), two deleted rows.  The matrix-core route has to return the ids,
distance bits and counts of the distance-matrix route.  k = 1 with a rescore
limit (and ef) of 1 keeps R + 1 = 2 candidate blocks, fewer than the 3 and 10
blocks of the larger corpora, so a wrong, stale or unwritten key changes the
candidate set and with it the result; the 1-block corpus cannot see one and
only shows that a ring shorter than its prologue neither faults nor returns
garbage.  rq-1 rotates to at
least 256 columns (NC = 4, still 8 slots).  MI355X only (marker gpu)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, K = 5, 1
DIMS = [64, 1024]
ROWS = [20, 70, 300]


def inputs(oracle, n, d):
    return oracle.gen_matrix(0, 81, 0, n, d), oracle.gen_matrix(0, 82, 0, NQ, d), (3, n - 2)


def same(a, b):
    for x, y, what in zip(a, b, ("ids", "distances", "counts")):
        np.testing.assert_array_equal(y, x, err_msg=what)


@pytest.mark.parametrize("metric", ["l2-squared", "cosine"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_sq_ring_edges(wv, oracle, d, n, metric):
    data, queries, deleted = inputs(oracle, n, d)
    idx = wv.FlatIndex(distance=metric, variant="avx256", sq=True, rescore_limit=1)
    idx.add_batch(np.arange(n, dtype=np.uint64), data)
    idx.sq_fit(0)
    idx.delete(*deleted)
    idx.set_option("ef", 1)
    out = []
    for arm in (0, 1):
        idx.set_option("sq_keys", arm)
        ids, dists, counts = idx.hnsw_flat_search(queries, K)
        out.append((ids.copy(), dists.view(np.uint32).copy(), counts.copy()))
    assert wv._lib.ROUTES[idx.stats()["last_route"]] == "sq_int8"
    assert (out[0][2] == K).all()
    same(out[0], out[1])
    idx.close()


@pytest.mark.parametrize("metric", ["l2-squared", "dot"])
@pytest.mark.parametrize("bits", [8, 1])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_rq_ring_edges(wv, oracle, d, n, bits, metric):
    data, queries, deleted = inputs(oracle, n, d)
    idx = wv.FlatIndex(distance=metric, variant="avx256", rq={"bits": bits}, rescore_limit=1)
    idx.add_batch(np.arange(n, dtype=np.uint64), data)
    assert idx.rq_info()["output_dim"] == (d if bits == 8 else max(d, 256))
    idx.delete(*deleted)
    out = []
    for arm in (0, 1):
        idx.set_option("rq_mfma", arm)
        ids, dists, counts = idx.search_by_vector_batch(queries, K)
        out.append((ids.copy(), dists.view(np.uint32).copy(), counts.copy()))
    assert wv._lib.ROUTES[idx.stats()["last_route"]] == "rq8_int8"
    assert (out[0][2] == K).all()
    same(out[0], out[1])
    idx.close()
