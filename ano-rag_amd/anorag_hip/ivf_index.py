"""Thin object wrapper over the anr_ivf_* C ABI.

``IVFIndex`` is what the drop-in ``vector_store.VectorIndex`` holds for ``index_type`` IVFFlat / IVFPQ when the config
key ``anorag_hip.ivf`` is true (reference vector_store/vector_index.py:81-95 builds a ``faiss.IndexIVFFlat`` there): the
``train`` / ``add`` / ``search`` / ``remove_ids`` surface of faiss's IVF indexes, with ``nprobe`` passed per search.
Results are the exact top-k of the probed lists (see include/anorag.h).  With ``pq_m`` the handle is an IVF-PQ index
(faiss's ``IndexIVFPQ(quantizer, d, nlist, pq_m, 8)``): rows are stored as ``pq_m`` one-byte codes of their residuals and
a search returns the ADC top-k of the probed lists.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import METRIC_IP, METRIC_L2, AnoragError  # noqa: F401
from .flat_index import _f32_matrix, _settle_interpreter_heap


class IVFIndex:
    """IVF-Flat (or, with ``pq_m``, IVF-PQ) inner-product / squared-L2 index resident on one MI355X."""

    def __init__(self, d: int, nlist: int, metric: int = METRIC_IP, normalize: bool = False, device: int = 0,
                 spherical: bool = False, pq_m: int = None):
        self._lib = _lib.load()
        _settle_interpreter_heap()
        self.d = int(d)
        self.nlist = int(nlist)
        self.metric = int(metric)
        self.normalize = bool(normalize)
        self.device = int(device)
        self.nprobe = 1
        self.pq_m = None if pq_m is None else int(pq_m)
        h = C.c_void_p()
        self._h = None
        if self.pq_m is None:
            _lib.check(self._lib.anr_ivf_create(self.d, self.metric, int(self.normalize), self.nlist, self.device,
                                                C.byref(h)), "anr_ivf_create")
        else:
            _lib.check(self._lib.anr_ivf_create_pq(self.d, self.metric, int(self.normalize), self.nlist, self.pq_m, 8,
                                                   self.device, C.byref(h)), "anr_ivf_create_pq")
        self._h = h
        if spherical:
            self.set_spherical(True)

    def set_spherical(self, on: bool) -> None:
        """True: spherical k-means (centroids normalised after every update), what faiss's IVF uses for inner product"""
        _lib.check(self._lib.anr_ivf_set_spherical(self._h, int(bool(on))), "anr_ivf_set_spherical")

    def assignments(self, ids) -> np.ndarray:
        """list of each given global id"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        out = np.empty((len(ids),), dtype=np.int32)
        _lib.check(self._lib.anr_ivf_assignments(self._h, ids.ctypes.data, len(ids), out.ctypes.data),
                   "anr_ivf_assignments")
        return out

    def last_search_stats(self) -> dict:
        """{'n_queries', 'n_exact_rescan'} of the last search: queries re-scored exactly after a failed certificate"""
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.anr_ivf_last_search_stats(self._h, C.byref(a), C.byref(b)), "anr_ivf_last_search_stats")
        return {"n_queries": int(a.value), "n_exact_rescan": int(b.value)}

    @property
    def ntotal(self) -> int:
        return int(self._lib.anr_ivf_ntotal(self._h)) if self._h else 0

    @property
    def is_trained(self) -> bool:
        return bool(self._lib.anr_ivf_is_trained(self._h)) if self._h else False

    def train(self, x, niter: int = 25, seed: int = 1234) -> None:
        """k-means on at most 256 * nlist of the rows (device; deterministic for a given seed)"""
        x = _f32_matrix(x, self.d, "train")
        _lib.check(self._lib.anr_ivf_train(self._h, x.ctypes.data, x.shape[0], int(niter), int(seed)), "anr_ivf_train")

    def train_from(self, x, niter: int) -> None:
        """``niter`` Lloyd iterations over all rows of ``x``, starting from the current centroids"""
        x = _f32_matrix(x, self.d, "train_from")
        _lib.check(self._lib.anr_ivf_train_from_centroids(self._h, x.ctypes.data, x.shape[0], int(niter)),
                   "anr_ivf_train_from_centroids")

    @property
    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.d), dtype=np.float32)
        _lib.check(self._lib.anr_ivf_get_centroids(self._h, out.ctypes.data), "anr_ivf_get_centroids")
        return out

    def set_centroids(self, c) -> None:
        c = _f32_matrix(c, self.d, "set_centroids")
        if c.shape[0] != self.nlist:
            raise ValueError(f"set_centroids: expected {self.nlist} rows, got {c.shape[0]}")
        _lib.check(self._lib.anr_ivf_set_centroids(self._h, c.ctypes.data), "anr_ivf_set_centroids")

    # ---- IVF-PQ (pq_m given) ----
    @property
    def codebooks(self) -> np.ndarray:
        """[pq_m, 256, d / pq_m] float32"""
        out = np.empty((self.pq_m or 0, 256, self.d // (self.pq_m or 1)), dtype=np.float32)
        _lib.check(self._lib.anr_ivf_get_codebooks(self._h, out.ctypes.data), "anr_ivf_get_codebooks")
        return out

    def set_codebooks(self, cb) -> None:
        """[pq_m, 256, d / pq_m] float32; rows already in the index are re-encoded"""
        shape = (self.pq_m or 0, 256, self.d // (self.pq_m or 1))
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        if cb.shape != shape:
            raise ValueError(f"set_codebooks: expected shape {shape}, got {cb.shape}")
        _lib.check(self._lib.anr_ivf_set_codebooks(self._h, cb.ctypes.data), "anr_ivf_set_codebooks")

    def pq_train_from(self, x, niter: int) -> None:
        """``niter`` Lloyd iterations of every sub-space over the residuals of all rows of ``x``, from the current
        codebooks"""
        x = _f32_matrix(x, self.d, "pq_train_from")
        _lib.check(self._lib.anr_ivf_pq_train_from_codebooks(self._h, x.ctypes.data, x.shape[0], int(niter)),
                   "anr_ivf_pq_train_from_codebooks")

    def codes(self, ids):
        """(lists int32 [n], codes uint8 [n, pq_m]) of the given global ids"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        lists = np.empty((len(ids),), dtype=np.int32)
        codes = np.empty((len(ids), self.pq_m or 0), dtype=np.uint8)
        _lib.check(self._lib.anr_ivf_codes(self._h, ids.ctypes.data, len(ids), lists.ctypes.data, codes.ctypes.data),
                   "anr_ivf_codes")
        return lists, codes

    def decode(self, ids) -> np.ndarray:
        """c_list + the codebook entries of each id's codes (what an ADC key scores)"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        out = np.empty((len(ids), self.d), dtype=np.float32)
        _lib.check(self._lib.anr_ivf_decode(self._h, ids.ctypes.data, len(ids), out.ctypes.data), "anr_ivf_decode")
        return out

    def memory(self) -> dict:
        """{'device_bytes', 'host_bytes'}: the persistent storage of the index (search scratch excluded)"""
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.anr_ivf_memory(self._h, C.byref(a), C.byref(b)), "anr_ivf_memory")
        return {"device_bytes": int(a.value), "host_bytes": int(b.value)}

    def add(self, x) -> None:
        x = _f32_matrix(x, self.d, "add")
        _lib.check(self._lib.anr_ivf_add(self._h, x.ctypes.data, x.shape[0]), "anr_ivf_add")

    def set_add_raw(self, raw: bool) -> None:
        """True: later adds store rows as given (already preprocessed, e.g. reloaded from a saved index)"""
        _lib.check(self._lib.anr_ivf_set_add_raw(self._h, int(bool(raw))), "anr_ivf_set_add_raw")

    def add_device(self, x_ptr: int, n: int) -> None:
        _lib.check(self._lib.anr_ivf_add_dev(self._h, C.c_void_p(x_ptr), int(n)), "anr_ivf_add_dev")

    def search(self, q, k: int, nprobe: int = None):
        q = _f32_matrix(q, self.d, "search")
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _lib.check(self._lib.anr_ivf_search(self._h, q.ctypes.data, nq, int(k), int(nprobe or self.nprobe),
                                            D.ctypes.data, I.ctypes.data), "anr_ivf_search")
        return D, I

    def search_device_queries(self, q_ptr: int, nq: int, k: int, nprobe: int = None):
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _lib.check(self._lib.anr_ivf_search_devq(self._h, C.c_void_p(q_ptr), int(nq), int(k), int(nprobe or self.nprobe),
                                                 D.ctypes.data, I.ctypes.data), "anr_ivf_search_devq")
        return D, I

    def list_sizes(self) -> np.ndarray:
        out = np.empty((self.nlist,), dtype=np.int64)
        _lib.check(self._lib.anr_ivf_list_sizes(self._h, out.ctypes.data), "anr_ivf_list_sizes")
        return out

    def reconstruct(self, ids) -> np.ndarray:
        """stored (preprocessed) rows of the given global ids"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        out = np.empty((len(ids), self.d), dtype=np.float32)
        _lib.check(self._lib.anr_ivf_reconstruct(self._h, ids.ctypes.data, len(ids), out.ctypes.data),
                   "anr_ivf_reconstruct")
        return out

    def reconstruct_n(self, i0: int, n: int) -> np.ndarray:
        return self.reconstruct(np.arange(int(i0), int(i0) + int(n), dtype=np.int64))

    def remove_ids(self, ids) -> int:
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        n = C.c_int64(0)
        _lib.check(self._lib.anr_ivf_remove(self._h, ids.ctypes.data, len(ids), C.byref(n)), "anr_ivf_remove")
        return int(n.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.anr_ivf_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


__all__ = ["IVFIndex"]
