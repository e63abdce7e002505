"""Thin object wrapper over the anr_index_graph_* C ABI.

``GraphIndex`` is what the drop-in ``vector_store.VectorIndex`` holds for ``index_type`` HNSW when the config key
``anorag_hip.graph`` is true (reference vector_store/vector_index.py:94-99 builds a ``faiss.IndexHNSWFlat`` there): a
``FlatIndex`` whose ``search`` walks a fixed-degree graph with a beam of ``ef_search`` entries instead of scanning every
row.  The graph is built from the index's own exact kNN lists on the first search (or ``build_graph``) and rebuilt on the
first search after an ``add`` or ``reset``.  ``exact_search`` is the flat index's exact scan; the device-output forms
(``search_device`` / ``search_device_async``) stay exact too, and so does a search for more than ``MAX_GRAPH_K`` results
(the beam holds at most 256 entries; the exact scan is what such a call got before the graph existed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import METRIC_IP, GraphStats
from .flat_index import FlatIndex, _f32_matrix


class GraphIndex(FlatIndex):
    """Graph (one-level HNSW-like) index over the rows of a FlatIndex on one MI355X."""

    MAX_GRAPH_K = 256

    def __init__(self, d: int, metric: int = METRIC_IP, normalize: bool = False, device: int = 0, R: int = 64,
                 build_degree: int = 128, ef_search: int = 100, keep_knn: bool = False):
        super().__init__(d, metric, normalize=normalize, device=device)
        self.R = int(R)
        self.build_degree = int(build_degree)
        self.ef_search = int(ef_search)
        self.keep_knn = bool(keep_knn)  # keep the pre-prune kNN lists (knn_lists): n * build_degree int32 of host memory

    def build_graph(self, R: int = None, build_degree: int = None) -> None:
        if R is not None:
            self.R = int(R)
        if build_degree is not None:
            self.build_degree = int(build_degree)
        _lib.check(self._lib.anr_index_graph_build(self._h, self.R, self.build_degree, int(self.keep_knn)),
                   "anr_index_graph_build")

    def graph_stats(self) -> dict:
        st = GraphStats()
        _lib.check(self._lib.anr_index_graph_stats(self._h, C.byref(st)), "anr_index_graph_stats")
        return st.as_dict()

    def _ensure_graph(self) -> None:
        if not self.graph_stats()["has_graph"]:
            self.build_graph()

    def has_fresh_graph(self) -> bool:
        """a graph exists and matches the rows (nothing added or reset since it was built or set)"""
        st = self.graph_stats()
        return bool(st["has_graph"]) and not st["stale"]

    def search(self, q, k: int, ef: int = None):
        q = _f32_matrix(q, self.d, "search")
        if k > self.MAX_GRAPH_K:
            return self.exact_search(q, k)
        self._ensure_graph()
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _lib.check(self._lib.anr_index_graph_search(self._h, q.ctypes.data, nq, int(k), int(ef or self.ef_search),
                                                    D.ctypes.data, I.ctypes.data), "anr_index_graph_search")
        return D, I

    def search_device_queries(self, q_ptr: int, nq: int, k: int, ef: int = None):
        if k > self.MAX_GRAPH_K:
            return FlatIndex.search_device_queries(self, q_ptr, nq, k)
        self._ensure_graph()
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _lib.check(self._lib.anr_index_graph_search_devq(self._h, C.c_void_p(q_ptr), int(nq), int(k),
                                                         int(ef or self.ef_search), D.ctypes.data, I.ctypes.data),
                   "anr_index_graph_search_devq")
        return D, I

    def exact_search(self, q, k: int):
        return FlatIndex.search(self, q, k)

    def adjacency(self) -> np.ndarray:
        """[ntotal, R] int32 neighbour lists, -1 padded (built or rebuilt first when needed)"""
        self._ensure_graph()
        R = self.graph_stats()["R"]
        out = np.empty((self.ntotal, R), dtype=np.int32)
        _lib.check(self._lib.anr_index_graph_get(self._h, out.ctypes.data, out.shape[0], R), "anr_index_graph_get")
        return out

    def set_adjacency(self, adj) -> None:
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        if adj.ndim != 2:
            raise ValueError("adjacency must be [ntotal, R]")
        _lib.check(self._lib.anr_index_graph_set(self._h, adj.ctypes.data, adj.shape[0], adj.shape[1]),
                   "anr_index_graph_set")
        self.R = int(adj.shape[1])

    def knn_lists(self) -> np.ndarray:
        """[ntotal, build_degree] int32: the pre-prune lists of the last build (keep_knn; a stale graph is rebuilt)"""
        K = self.graph_stats()["build_degree"]
        out = np.empty((self.ntotal, K), dtype=np.int32)
        _lib.check(self._lib.anr_index_graph_knn(self._h, out.ctypes.data, out.shape[0], K), "anr_index_graph_knn")
        return out

    def traversal_image(self, ids) -> np.ndarray:
        """rows of the int8 traversal image, decoded to float32 (exact)"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        out = np.empty((len(ids), self.d), dtype=np.float32)
        _lib.check(self._lib.anr_index_graph_image(self._h, ids.ctypes.data, len(ids), out.ctypes.data),
                   "anr_index_graph_image")
        return out


__all__ = ["GraphIndex"]
