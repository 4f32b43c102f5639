"""CPU: the multi-vector index's refusals that come before any device call,
each with its error text, and the public header's new route define."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("distance", ["hamming", "manhattan"])
def test_create_refuses_hamming_and_manhattan(wv, distance):
    with pytest.raises(wv.WeaviateError, match=f"multivector: the {distance} distance is not supported") as e:
        wv.MultiVectorIndex(distance=distance, dims=16)
    assert e.value.code == -5


def test_add_refusals(wv):
    with wv.MultiVectorIndex(distance="dot", dims=8) as idx:
        with pytest.raises(wv.WeaviateError, match="addMultiBatch called with empty lists") as e:
            idx.add_multi_batch([], [])
        assert e.value.code == -3
        with pytest.raises(wv.WeaviateError, match="multi vector of document 7 has no vectors") as e:
            idx.add_multi_batch([3, 7], [np.ones((2, 8), np.float32), np.zeros((0, 8), np.float32)])
        assert e.value.code == -3
        with pytest.raises(wv.WeaviateError, match="addMultiBatch called with vectors of different lengths"):
            idx.add_multi_batch([3, 7], [np.ones((2, 8), np.float32), np.ones((1, 9), np.float32)])
        with pytest.raises(wv.WeaviateError, match="new node has a multi vector with length 9 at position 0. "
                                                   "Existing nodes have vectors with length 8"):
            idx.add_multi(3, np.ones((2, 9), np.float32))
        assert not idx.contains_doc(3) and idx.stats()["documents"] == 0


def test_search_refusals(wv):
    from weaviate_amd import _lib
    import ctypes as C
    q = np.ones((2, 8), np.float32)
    with wv.MultiVectorIndex(distance="l2-squared", dims=8) as idx:
        for k in (0, -1):
            with pytest.raises(wv.WeaviateError, match="k must be positive"):
                idx.search_by_multi_vector(q, k)
        with pytest.raises(wv.WeaviateError, match="multi vector query 1 has no vectors"):
            idx.search_by_multi_vector_batch([q, np.zeros((0, 8), np.float32)], 3)
        with pytest.raises(wv.WeaviateError, match="9 vs 8: vector lengths don't match") as e:
            idx.search_by_multi_vector(np.ones((2, 9), np.float32), 3)
        assert e.value.code == -2
        with pytest.raises(wv.WeaviateError, match="multi vector query 0 has no vectors"):
            idx.query_multi_vector_distances(np.zeros((0, 8), np.float32), [1])
        off = np.array([0, 2, 1], np.int64)  # non-monotone offsets reach the C ABI only
        cnt = np.zeros(2, np.int32)
        rc = _lib.load().wv_mv_search_batch(idx._h, q.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data, 2, 8, 3,
                                           None, None, None, None, None, cnt.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == _lib.WV_ERR_INVALID and _lib.load().wv_last_error() == b"query offsets must not decrease"
        # an index without documents answers without a device
        ids, dists = idx.search_by_multi_vector(q, 3)
        assert ids.size == 0 and idx.stats()["last_route"] == 15


def test_header_route_has_a_name():
    src = open(os.path.join(REPO, "include", "wv_knn.h")).read()
    defs = dict(re.findall(r"^#define\s+(WV_[A-Z0-9_]+)\s+(-?\d+)\b", src, flags=re.M))
    from weaviate_amd import _lib
    assert defs["WV_ROUTE_MV_MAXSIM"] == "15" and _lib.ROUTES[15] == "mv_maxsim"
    assert sorted(int(v) for k, v in defs.items() if k.startswith("WV_ROUTE_")) == sorted(_lib.ROUTES)
