"""GPU: the key route of the multi-vector flat search (k_mv_keys + k_mv_cut, then
the exact kernel on the survivors) against hnsw.flatMultiSearch
restated as in tests/test_gpu_mv.py: computeScore as a float32 loop over
oracle.single_dist(DOT, variant, q, t), oracle.heap_scan over the candidates in
ascending id order.  Ids and distances are compared bit for bit; every index
sets mv_keys = 1 and mv_keys_min = 0."""
import functools

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

MAXF = np.float32(np.finfo(np.float32).max)
LENS = (1, 7, 31, 32, 33, 70)  # tokens per document, around the kernel's 32-row tile
VARIANTS = {"avx256": orc.AVX256, "avx512": orc.AVX512}
# dpad 32 / 64 / 96 / 128: token fragments in registers; 160: streamed.  Query vectors around the 32-vector
# group, documents around LIST_CHUNK
SHAPES = [(5, 1, 40), (40, 31, 255), (96, 33, 257), (128, 32, 600), (160, 40, 64)]


def score(variant, Q, D):
    s = np.float32(0.0)
    for q in Q:
        m = MAXF
        for t in D:
            dist = np.float32(orc.single_dist(orc.DOT, variant, q, t))
            if dist < m:
                m = dist
        s = np.float32(s + m)
    return s


def scores(variant, Q, docs):
    return np.array([score(VARIANTS[variant], Q, D) for D in docs], np.float32)


def prepared(distance, rows):
    return np.stack([orc.normalize(r) for r in rows]) if distance == "cosine" else rows


def make_docs(seed, ndocs, d):
    lens = [LENS[i % len(LENS)] for i in range(ndocs)]
    rows = orc.gen_matrix(0, seed, 0, sum(lens), d)
    cuts = np.cumsum([0] + lens)
    return [rows[cuts[i]:cuts[i + 1]] for i in range(ndocs)]


@functools.lru_cache(maxsize=None)
def dataset(d, nqv, ndocs, variant, distance="dot"):
    """Documents with ids 2 i + 5, one query, the reference scores of the prepared vectors (read only)."""
    docs = make_docs(d, ndocs, d)
    Q = orc.gen_matrix(0, 1000 + d, 0, nqv, d)
    ids = np.arange(ndocs, dtype=np.uint64) * 2 + 5
    return docs, Q, ids, scores(variant, prepared(distance, Q), [prepared(distance, D) for D in docs])


def expect(cand_ids, cand_scores, k):
    order = np.argsort(cand_ids, kind="stable")
    pos, dd = orc.heap_scan(np.asarray(cand_scores, np.float32)[order], k)
    return np.asarray(cand_ids, np.uint64)[order][pos.astype(np.int64)], dd


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (got[1], want[1])


def index(wv, distance, variant, ids, docs, **opts):
    idx = wv.MultiVectorIndex(distance=distance, variant=variant)
    for key, v in {"mv_keys": 1, "mv_keys_min": 0, **opts}.items():
        idx.set_option(key, v)
    idx.add_multi_batch(ids, docs)
    return idx


@pytest.mark.parametrize("distance", ["dot", "cosine"])
@pytest.mark.parametrize("variant", ["avx256", "avx512"])
@pytest.mark.parametrize("d,nqv,ndocs", SHAPES)
def test_search_matches_reference(wv, d, nqv, ndocs, variant, distance):
    docs, Q, ids, sc = dataset(d, nqv, ndocs, variant, distance)
    with index(wv, distance, variant, ids, docs) as idx:
        for k in (1, 10):
            top = np.sort(sc)[:k + 1]
            assert np.unique(top).size == top.size  # the precondition of a search without fallback
            same(idx.search_by_multi_vector(Q, k), expect(ids, sc, k))
            st = idx.stats()
            assert st["last_route"] == 16 and st["last_key_queries"] == 1 and st["last_fallback_queries"] == 0
            assert k + 1 <= st["last_candidates"] <= ndocs


@pytest.mark.parametrize("d,nqv,ndocs", [SHAPES[1], SHAPES[4]])
def test_keys_within_their_bound(wv, d, nqv, ndocs):
    docs, Q, ids, sc = dataset(d, nqv, ndocs, "avx256")
    with index(wv, "dot", "avx256", ids, docs) as idx:
        idx.search_by_multi_vector(Q, 10)
        keys, eps, kid = idx.debug_keys(0)
    assert np.array_equal(kid, ids)
    assert np.all(eps > 0) and np.all(np.isfinite(eps)) and np.all(np.isfinite(keys))
    s64 = np.array([-(Q.astype(np.float64) @ D.astype(np.float64).T).max(axis=1).sum() for D in docs])
    for name, s in (("float64 MaxSim", s64), ("reference fp32", sc.astype(np.float64))):
        err = np.abs(keys.astype(np.float64) - s)
        print(f"d={d}: max |key - {name}| / eps = {(err / eps).max():.4f}")
        assert np.all(err <= eps), name


@pytest.mark.parametrize("case", ["duplicates", "cap", "tiny", "nan"])
def test_fallbacks_stay_exact(wv, case):
    docs, Q, ids, sc = dataset(40, 31, 255, "avx256")
    docs, ids, sc, opts = docs[:60], ids[:60], sc[:60], {}
    if case == "duplicates":  # every document twice under two ids: the top scores tie
        docs, ids, sc = docs + docs, np.concatenate([ids, ids + 1000]), np.concatenate([sc, sc])
    elif case == "cap":
        opts = {"mv_keys_cap": 1}
    elif case == "tiny":  # norms below the guard's 2^-60
        docs, Q = [D * np.float32(1e-25) for D in docs], Q * np.float32(1e-25)
        sc = scores("avx256", Q, docs)
    elif case == "nan":
        Q = Q.copy()
        Q[2, 1] = np.nan
        sc = scores("avx256", Q, docs)
    with index(wv, "dot", "avx256", ids, docs, **opts) as idx:
        same(idx.search_by_multi_vector(Q, 10), expect(ids, sc, 10))
        st = idx.stats()
        assert st["last_route"] == 16 and st["last_key_queries"] == 1 and st["last_fallback_queries"] == 1


def test_mixed_batch(wv):
    docs, Q, ids, sc = dataset(40, 31, 255, "avx256")
    gone = ids[[3, 100, 256 - 2]]
    allows = [  # raw id arrays: an AllowList would sort them and drop the duplicates
        np.concatenate([ids[::-3], ids[10:14], gone, np.array([4, 6, 1 << 40], np.uint64)]),  # keys
        np.zeros(0, np.uint64),                                                                # below mv_keys_min
        None,                                                                                  # keys: every document
        ids[[200, 7, 7, 100, 31]],                                                             # below mv_keys_min
        ids[20:90:2],                                                                          # keys
    ]
    queries = [Q, Q, Q, Q, Q[:4]]
    with index(wv, "dot", "avx256", ids, docs, mv_keys_min=6, mv_list_rows=256) as idx:  # several launch groups
        idx.delete_multi(*gone)
        bi, bd, bn = idx.search_by_multi_vector_batch(queries, 10, allows)
        st = idx.stats()
        assert st["last_route"] == 16 and st["last_key_queries"] == 3 and st["last_fallback_queries"] == 0
        idx.set_option("mv_keys", 0)
        for r, (q, a) in enumerate(zip(queries, allows)):
            same((bi[r, :bn[r]], bd[r, :bn[r]]), idx.search_by_multi_vector(q, 10, a))
            assert idx.stats()["last_route"] == 15
        live = ~np.isin(ids, gone)
        same((bi[2, :bn[2]], bd[2, :bn[2]]), expect(ids[live], sc[live], 10))
        assert bn[1] == 0 and bn[0] == 10


def test_query_staged_in_tiles(wv):
    """300 query vectors at d = 128 are four LDS tiles of 96: the documents' sums are carried across them."""
    docs = make_docs(3, 12, 128)
    ids = np.arange(12, dtype=np.uint64)
    Q = orc.gen_matrix(0, 77, 0, 300, 128)
    with index(wv, "dot", "avx256", ids, docs) as idx:
        same(idx.search_by_multi_vector(Q, 5), expect(ids, scores("avx256", Q, docs), 5))
        st = idx.stats()
        assert st["last_route"] == 16 and st["last_fallback_queries"] == 0
