"""GPU: the multi-vector flat search (wv_mv_search_batch, k_mv_maxsim /
k_mv_simple + k_list_heap) against hnsw.flatMultiSearch restated with the
oracle's pieces: computeScore (hnsw/search.go:954-1006) as a float32 loop over
oracle.single_dist(DOT, variant, q, t) -- minimum by `<` from MaxFloat32, one
sequential float32 sum -- and oracle.heap_scan over the candidates' scores in
ascending id order.  Ids and distances are compared bit for bit."""
import functools

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

MAXF = np.float32(np.finfo(np.float32).max)
LENS = (1, 7, 8, 9, 17, 70)  # tokens per document, around the kernel's 16-row step
VARIANTS = {"avx256": orc.AVX256, "avx512": orc.AVX512}


def score(variant, Q, D):
    """computeScore of one (prepared) query against one (prepared) document."""
    s = np.float32(0.0)
    for q in Q:
        m = MAXF
        for t in D:
            dist = np.float32(orc.single_dist(orc.DOT, variant, q, t))
            if dist < m:
                m = dist
        s = np.float32(s + m)
    return s


def make_docs(seed, ndocs, d):
    lens = [LENS[i % len(LENS)] for i in range(ndocs)]
    rows = orc.gen_matrix(0, seed, 0, sum(lens), d)
    cuts = np.cumsum([0] + lens)
    return [rows[cuts[i]:cuts[i + 1]] for i in range(ndocs)]


@functools.lru_cache(maxsize=None)
def dataset(d, nqv, ndocs, variant):
    """Documents with ids 2 i + 5, one query and its reference scores (shared by the tests, read only)."""
    docs = make_docs(d, ndocs, d)
    Q = orc.gen_matrix(0, 1000 + d, 0, nqv, d)
    ids = np.arange(ndocs, dtype=np.uint64) * 2 + 5
    return docs, Q, ids, np.array([score(VARIANTS[variant], Q, D) for D in docs], np.float32)


def expect(cand_ids, cand_scores, k):
    """The reference heap over the candidates in ascending id order."""
    order = np.argsort(cand_ids, kind="stable")
    pos, dd = orc.heap_scan(np.asarray(cand_scores, np.float32)[order], k)
    return np.asarray(cand_ids, np.uint64)[order][pos.astype(np.int64)], dd


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (got[1], want[1])


def index(wv, distance, variant, tile, ids, docs, **opts):
    idx = wv.MultiVectorIndex(distance=distance, variant=variant)
    idx.set_option("mv_tile", tile)
    for key, v in opts.items():
        idx.set_option(key, v)
    idx.add_multi_batch(ids, docs)
    return idx


# d: scalar path; 8 + tail; 32 + 8; below the AVX-512 switch; at it; 128 + 32; 128 + 64 + 8
# query vectors around QT, documents around LIST_CHUNK
CASES = [(5, 1, 1), (13, 8, 255), (40, 9, 257), (96, 33, 40), (128, 9, 600), (160, 8, 30), (200, 4, 60)]


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("variant", ["avx256", "avx512"])
@pytest.mark.parametrize("d,nqv,ndocs", CASES)
def test_search_matches_reference(wv, d, nqv, ndocs, variant, tile):
    docs, Q, ids, scores = dataset(d, nqv, ndocs, variant)
    with index(wv, "dot", variant, tile, ids, docs) as idx:
        for k in (1, 10, ndocs + 3):
            same(idx.search_by_multi_vector(Q, k), expect(ids, scores, k))
        st = idx.stats()
        assert st["last_route"] == 15 and st["last_scan_rows"] == ndocs
        assert st["last_token_rows"] == sum(len(D) for D in docs)
        assert idx.multivector() and idx.contains_doc(int(ids[0])) and not idx.contains_doc(4)


@pytest.mark.parametrize("tile", [0, 1])
def test_ties_follow_the_reference_heap(wv, tile):
    """Small-integer vectors, groups of documents holding one token set in different orders: equal scores."""
    rng = np.random.default_rng(7)
    base = [rng.integers(-2, 3, size=(5, 16)).astype(np.float32) for _ in range(4)]
    docs = [base[i % 4][rng.permutation(5)] for i in range(20)]
    ids = np.arange(20, dtype=np.uint64) + 100
    Q = rng.integers(-2, 3, size=(6, 16)).astype(np.float32)
    scores = [score(orc.AVX256, Q, D) for D in docs]
    assert len(set(float(s) for s in scores)) <= 4
    with index(wv, "dot", "avx256", tile, ids, docs) as idx:
        for k in (1, 3, 10):
            same(idx.search_by_multi_vector(Q, k), expect(ids, scores, k))


@pytest.mark.parametrize("tile", [0, 1])
def test_allow_lists_in_one_batch(wv, tile):
    docs, Q, ids, scores = dataset(40, 9, 257, "avx256")
    gone = ids[[3, 100, 256]]
    allows = [  # raw id arrays: an AllowList would sort them and drop the duplicates
        # unsorted, duplicates, deleted ids, never-stored ids, an id past the high-water mark
        np.concatenate([ids[::-3], ids[10:14], gone, np.array([4, 6, 1 << 40], np.uint64)]),
        np.zeros(0, np.uint64),
        None,
        ids[[200, 7, 7, 100, 31]],
        ids[:5][::-1],
    ]
    queries = [Q, Q, Q, Q, Q[:4]]
    with index(wv, "dot", "avx256", tile, ids, docs, mv_list_rows=256) as idx:  # several launch groups
        idx.delete_multi(*gone)
        bi, bd, bn = idx.search_by_multi_vector_batch(queries, 10, allows)
        scanned = idx.stats()["last_scan_rows"]
        live = ~np.isin(ids, gone)
        for r, (q, a) in enumerate(zip(queries, allows)):
            same((bi[r, :bn[r]], bd[r, :bn[r]]), idx.search_by_multi_vector(q, 10, a))
            cand = live if a is None else live & np.isin(ids, a)
            sc = scores[cand] if q is Q else [score(orc.AVX256, q, docs[i]) for i in np.flatnonzero(cand)]
            same((bi[r, :bn[r]], bd[r, :bn[r]]), expect(ids[cand], sc, 10))
        assert bn[1] == 0 and bn[2] == 10
        # listed slots below the high-water mark, distinct; deleted and never-stored ones are skipped by the kernel
        assert scanned == sum(live.sum() if a is None else np.unique(a[a <= ids.max()]).size for a in allows)


@pytest.mark.parametrize("tile", [0, 1])
def test_distance_only_decides_normalisation(wv, tile):
    """An l2-squared index scores with -dot as a dot index does; cosine-dot normalises documents and queries."""
    docs, Q, ids, scores = dataset(40, 9, 257, "avx256")
    docs, ids, scores = docs[:30], ids[:30], scores[:30]
    with index(wv, "dot", "avx256", tile, ids, docs) as a, index(wv, "l2-squared", "avx256", tile, ids, docs) as b:
        same(b.search_by_multi_vector(Q, 10), a.search_by_multi_vector(Q, 10))
        same(b.search_by_multi_vector(Q, 10), expect(ids, scores, 10))
    ndocs = [np.stack([orc.normalize(t) for t in D]) for D in docs]
    nQ = np.stack([orc.normalize(q) for q in Q])
    with index(wv, "cosine", "avx256", tile, ids, docs) as c, index(wv, "dot", "avx256", tile, ids, ndocs) as e:
        same(c.search_by_multi_vector(Q, 10), e.search_by_multi_vector(nQ, 10))
        same(c.search_by_multi_vector(Q, 10), expect(ids, [score(orc.AVX256, nQ, D) for D in ndocs], 10))


@pytest.mark.parametrize("tile", [0, 1])
def test_query_staged_in_tiles(wv, tile):
    """300 query vectors at d = 40 are more than 32 KiB of staging: the sums are carried across the tiles."""
    docs = make_docs(3, 6, 40)
    ids = np.arange(6, dtype=np.uint64)
    Q = orc.gen_matrix(0, 77, 0, 300, 40)
    with index(wv, "dot", "avx256", tile, ids, docs) as idx:
        same(idx.search_by_multi_vector(Q, 6), expect(ids, [score(orc.AVX256, Q, D) for D in docs], 6))


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("variant,d", [("avx256", 40), ("avx512", 160)])
def test_nan_is_never_the_minimum(wv, variant, d, tile):
    docs = [D.copy() for D in make_docs(5, 12, d)]
    docs[4][3, d - 1] = np.nan  # a 17-token document
    docs[5][0, 0] = np.nan      # a 70-token document
    Q = orc.gen_matrix(0, 9, 0, 5, d)
    Qn = Q.copy()
    Qn[2, 1] = np.nan  # every distance of this query vector is NaN: MaxFloat32 is summed
    ids = np.arange(12, dtype=np.uint64)
    with index(wv, "dot", variant, tile, ids, docs) as idx:
        for q in (Q, Qn):
            same(idx.search_by_multi_vector(q, 12), expect(ids, [score(VARIANTS[variant], q, D) for D in docs], 12))


@pytest.mark.parametrize("tile", [0, 1])
def test_delete_readd_and_query_distances(wv, tile):
    docs, Q, ids, scores = dataset(96, 33, 40, "avx512")
    with index(wv, "dot", "avx512", tile, ids, docs) as idx:
        idx.delete_multi(int(ids[2]), int(ids[9]))
        with pytest.raises(wv.WeaviateError, match="already stored"):
            idx.add_multi(int(ids[3]), docs[3])
        idx.add_multi(1000, docs[2])  # the deleted document under a new id, its rows at the tail
        nids = np.concatenate([np.delete(ids, [2, 9]), [1000]]).astype(np.uint64)
        nsc = np.concatenate([np.delete(scores, [2, 9]), scores[2:3]])
        same(idx.search_by_multi_vector(Q, 10), expect(nids, nsc, 10))
        order = np.array([38, 0, 38, 5])  # caller order, a duplicate
        got = idx.query_multi_vector_distances(Q, nids[order])
        assert np.array_equal(got.view(np.uint32), nsc[order].view(np.uint32))
        assert idx.query_multi_vector_distancer(Q)(1000) == float(scores[2])
        with pytest.raises(wv.WeaviateError, match=f"docID {int(ids[9])} is not in the vector index"):
            idx.query_multi_vector_distances(Q, [int(ids[9])])
