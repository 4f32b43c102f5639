"""Host-side mirror of the multi-vector methods of the reference's
`db.VectorIndex` (vector_index.go:25-54; hnsw: AddMulti / AddMultiBatch
insert.go:219-277, DeleteMulti delete.go:105-135, SearchByMultiVector's flat
branch hnsw/flat_search.go:143-212, QueryMultiVectorDistancer
search.go:1033-1045), backed by the gfx950 late-interaction kernel through the
wv_mv_* entry points of the C ABI.

A document and a query are lists of float32 vectors of one dimension; doc ids
are uint64.  The score is the reference's computeScore: the sum over the
query's vectors of the smallest -dot to any of the document's vectors.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import WeaviateError, check
from .flat import DISTANCES, PROVIDER_TYPE, VARIANTS, AllowList, _fptr, _iptr, _uptr


def _ragged(docs, what: str):
    """A list of [n_i][d] arrays -> (rows [sum n_i][d], offsets [len + 1]); the
    reference's error for vectors of different lengths."""
    mats = [np.asarray(v, dtype=np.float32) for v in docs]
    mats = [m.reshape(0, 0) if m.size == 0 else (m[None, :] if m.ndim == 1 else m) for m in mats]
    dims = {m.shape[1] for m in mats if m.shape[0]}
    if len(dims) > 1:
        raise WeaviateError(_lib.WV_ERR_INSERT, f"{what} called with vectors of different lengths")
    d = dims.pop() if dims else 0
    off = np.zeros(len(mats) + 1, dtype=np.int64)
    off[1:] = np.cumsum([m.shape[0] for m in mats])
    full = [m for m in mats if m.shape[0]]
    rows = np.ascontiguousarray(np.concatenate(full) if full else np.zeros((1, max(d, 1)), np.float32))
    return rows, off, d


class MultiVectorIndex:
    """The multi-vector VectorIndex surface over one GPU: AddMulti,
    AddMultiBatch, DeleteMulti, ContainsDoc, SearchByMultiVector (the flat
    branch: filtered brute force), QueryMultiVectorDistancer."""

    def __init__(self, distance: str = "cosine", dims: int = 0, device: int = 0, variant: str = "auto",
                 id_base: int = 0):
        if distance not in DISTANCES:
            raise WeaviateError(_lib.WV_ERR_INVALID, f"unrecognized or unsupported distance metric {distance!r}")
        self._l = _lib.load()
        cfg = _lib.WvMvConfig(DISTANCES[distance], int(dims), int(device), VARIANTS[variant], int(id_base))
        h = C.c_void_p()
        check(self._l.wv_mv_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.metric = DISTANCES[distance]
        self.device = device
        self.id_base = id_base

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._l.wv_mv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def multivector(self) -> bool:
        return True

    def distancer_type(self) -> str:  # the index's provider; pairs are always scored with -dot
        return PROVIDER_TYPE[self.metric]

    def set_option(self, key: str, value: int) -> None:
        check(self._l.wv_mv_set_option(self._h, key.encode(), int(value)))

    def stats(self) -> dict:
        s = _lib.WvMvStats()
        check(self._l.wv_mv_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def debug_keys(self, q: int = 0):
        """Diagnostic hook of the key route: (keys, eps, doc ids) of batch row q
        of the last search that took keys, one entry per listed slot."""
        n = C.c_int64(0)
        check(self._l.wv_mv_debug_keys(self._h, int(q), None, None, None, C.byref(n)))
        keys = np.zeros(max(n.value, 1), dtype=np.float32)
        eps = np.zeros_like(keys)
        slots = np.zeros(keys.size, dtype=np.uint32)
        check(self._l.wv_mv_debug_keys(self._h, int(q), _fptr(keys), _fptr(eps),
                                       slots.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
        return keys[: n.value], eps[: n.value], slots[: n.value].astype(np.uint64) + np.uint64(self.id_base)

    # -- insert path ------------------------------------------------------
    def add_multi(self, doc_id: int, vectors) -> None:
        self.add_multi_batch([doc_id], [vectors])

    def add_multi_batch(self, doc_ids: Sequence[int], vectors) -> None:  # insert.go:219-277
        if len(doc_ids) != len(vectors):
            raise WeaviateError(_lib.WV_ERR_INSERT, "ids and vectors sizes does not match")
        rows, off, d = _ragged(vectors, "addMultiBatch")
        ids = np.ascontiguousarray(doc_ids, dtype=np.uint64)
        check(self._l.wv_mv_add_batch(self._h, _uptr(ids), off.ctypes.data_as(C.c_void_p), _fptr(rows), ids.size,
                                      d if d else rows.shape[1]))

    def delete_multi(self, *doc_ids: int) -> None:  # delete.go:105-135
        a = np.ascontiguousarray(doc_ids, dtype=np.uint64)
        check(self._l.wv_mv_delete(self._h, _uptr(a), a.size))

    def contains_doc(self, doc_id: int) -> bool:  # index.go:767-773
        return bool(self._l.wv_mv_contains_doc(self._h, int(doc_id)))

    # -- search -----------------------------------------------------------
    def search_by_multi_vector_batch(self, queries, k: int, allows=None):
        """flatMultiSearch for every query (a [n_q][d] array each), query i
        under allows[i] (an AllowList, or None: every stored document).
        Returns (ids[nq,k], dists[nq,k], counts[nq]); row i equals the
        one-query call."""
        queries = list(queries)
        nq = len(queries)
        allows = [None] * nq if allows is None else list(allows)
        if len(allows) != nq:
            raise WeaviateError(_lib.WV_ERR_INVALID, f"{len(allows)} allow lists for {nq} queries")
        rows, qoff, d = _ragged(queries, "SearchByMultiVector")
        kk = max(int(k), 1)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        dists = np.zeros((nq, kk), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.int32)
        modes = np.array([0 if a is None else 1 for a in allows], dtype=np.int32)
        parts = [np.asarray(a.ids if isinstance(a, AllowList) else a, dtype=np.uint64) for a in allows if a is not None]
        aids = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(1, np.uint64), dtype=np.uint64)
        aoff = np.zeros(nq + 1, dtype=np.int64)
        sizes = iter(p.size for p in parts)
        aoff[1:] = np.cumsum([0 if a is None else next(sizes) for a in allows])
        check(self._l.wv_mv_search_batch(self._h, _fptr(rows), qoff.ctypes.data_as(C.c_void_p), nq,
                                         d if d else rows.shape[1], int(k), _uptr(aids),
                                         aoff.ctypes.data_as(C.c_void_p), _iptr(modes), _uptr(ids), _fptr(dists),
                                         _iptr(counts)))
        return ids, dists, counts

    def search_by_multi_vector(self, vectors, k: int, allow: Optional[AllowList] = None):
        """SearchByMultiVector's flat branch for one query: (ids, dists)."""
        ids, dists, counts = self.search_by_multi_vector_batch([vectors], k, [allow])
        return ids[0, : counts[0]], dists[0, : counts[0]]

    def query_multi_vector_distances(self, vectors, doc_ids) -> np.ndarray:
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        ids = np.ascontiguousarray(doc_ids, dtype=np.uint64)
        out = np.zeros(max(ids.size, 1), dtype=np.float32)
        check(self._l.wv_mv_query_distances(self._h, _fptr(q), q.shape[0] if q.size else 0, q.shape[1], _uptr(ids),
                                            ids.size, _fptr(out)))
        return out[: ids.size]

    def query_multi_vector_distancer(self, vectors):
        """QueryMultiVectorDistancer (search.go:1033-1045): fn(doc_id) -> score,
        raising "docID .. is not in the vector index" for an unknown id."""
        return lambda doc_id: float(self.query_multi_vector_distances(vectors, [doc_id])[0])
