"""The note graph's scores on the device: the `graph` source of ``HybridSearcher.fuse``.

* ``NoteGraph.pagerank`` replaces ``nx.pagerank(graph, weight="weight")`` of ``GraphIndex.build_index``
  (graph/graph_index.py:43-49): weighted PageRank, float64, reproducible bit for bit.
* ``NoteGraph.retrieve`` / ``graph_retrieve`` replace ``GraphRetriever.retrieve`` (graph/graph_retriever.py:61-92): per
  seed a shortest-path search bounded by a DISTANCE cutoff (``k_hop``), merged in seed order, scored
  ``(centrality / (dist + 1e-5)) * importance`` and sorted best first — for a batch of seed lists at once.
* ``NoteGraph.components`` / ``hop_histogram`` / ``quality_metrics`` replace ``compute_metrics``
  (graph/graph_quality.py:5-46): connected components and the average shortest path length of the largest one, from
  integer counts, equal to the reference's dict in every value.
* ``NoteGraph.retrieve_device`` leaves the rows on the device; ``NoteGraph.to_array`` turns them into the NaN-filled
  ``DeviceArray`` that ``fuse_dense`` takes as its ``graph`` source.

The reference's fallbacks for graphs networkx cannot weigh (unweighted PageRank, hop-count BFS) are out of scope: a
self-loop, a negative or non-finite weight is an error.  Fails loudly when the HIP library is missing; there is no CPU
path here (a numpy restatement lives in tests/notegraph_ref.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .fusion import DeviceArray, SparseRows


class PageRankNotConverged(_lib.AnoragError):
    """the power iteration did not converge in max_iter steps (networkx: PowerIterationFailedConvergence)"""


class NoteGraph:
    """Undirected weighted graph over ``n_nodes`` notes: ``src[e] -- dst[e]`` with ``weight[e]``, distinct pairs."""

    def __init__(self, n_nodes: int, src, dst, weight, device: int = 0):
        self._h = None
        self._lib = _lib.load()
        src = np.ascontiguousarray(src, dtype=np.int64).reshape(-1)
        dst = np.ascontiguousarray(dst, dtype=np.int64).reshape(-1)
        weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        if not (len(src) == len(dst) == len(weight)):
            raise ValueError("src, dst and weight must have one entry per edge")
        self.n, self.n_edges, self.device = int(n_nodes), len(src), int(device)
        self.k_hop = 2  # GraphRetriever's default cutoff (graph_retriever.py:12)
        self.note_ids: Optional[List[Any]] = None
        self.note_index: Dict[Any, int] = {}
        self.nodes: Optional[List[Dict[str, Any]]] = None
        self._centrality = np.zeros(self.n, dtype=np.float64)
        h = C.c_void_p()
        _lib.check(self._lib.anr_notegraph_create(self.device, self.n, self.n_edges, src.ctypes.data, dst.ctypes.data,
                                                  weight.ctypes.data, C.byref(h)), "anr_notegraph_create")
        self._h = h

    # ---- build time ----
    def pagerank(self, alpha: float = 0.85, max_iter: int = 100, tol: float = 1e-6) -> np.ndarray:
        """nx.pagerank(G, alpha, max_iter=max_iter, tol=tol, weight="weight") as an array in node order; becomes the
        centrality ``retrieve`` uses.  ``last_iterations``: the steps it took."""
        out = np.empty(self.n, dtype=np.float64)
        it = C.c_int32(0)
        rc = self._lib.anr_notegraph_pagerank(self._h, float(alpha), int(max_iter), float(tol), out.ctypes.data, C.byref(it))
        self.last_iterations = int(it.value)
        if rc == _lib.ANR_ENOCONV:
            raise PageRankNotConverged(_lib.last_error())
        _lib.check(rc, "anr_notegraph_pagerank")
        self._centrality = out
        return out

    def set_centrality(self, centrality) -> None:
        c = np.ascontiguousarray(centrality, dtype=np.float64).reshape(-1)
        if len(c) != self.n:
            raise ValueError(f"expected {self.n} centralities")
        _lib.check(self._lib.anr_notegraph_set_centrality(self._h, c.ctypes.data), "anr_notegraph_set_centrality")
        self._centrality = c.copy()

    def centrality(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        _lib.check(self._lib.anr_notegraph_get_centrality(self._h, out.ctypes.data), "anr_notegraph_get_centrality")
        return out

    def set_importance(self, importance) -> None:
        imp = np.ascontiguousarray(importance, dtype=np.float64).reshape(-1)
        if len(imp) != self.n:
            raise ValueError(f"expected {self.n} importance scores")
        _lib.check(self._lib.anr_notegraph_set_importance(self._h, imp.ctypes.data), "anr_notegraph_set_importance")

    def set_max_slots(self, slots: int) -> None:
        """bound the (query, seed) searches in flight (0 = sized from free device memory); results do not depend on it"""
        _lib.check(self._lib.anr_notegraph_set_option(self._h, _lib.NOTEGRAPH_OPT_MAX_SLOTS, int(slots)),
                   "anr_notegraph_set_option")

    # ---- graph quality (graph/graph_quality.py) ----
    def set_bfs_words(self, words: int) -> None:
        """64-bit words per node and pass of ``hop_histogram`` (1, 2, 4, 8, 16; 0 = default): a pass walks 64 * words
        sources; results do not depend on it"""
        _lib.check(self._lib.anr_notegraph_set_option(self._h, _lib.NOTEGRAPH_OPT_BFS_WORDS, int(words)),
                   "anr_notegraph_set_option")

    def components(self) -> Tuple[np.ndarray, List[int]]:
        """(labels int64 [n], sizes): labels[v] = the smallest node index of v's component; sizes in the order
        ``nx.connected_components`` yields the components (by first node = ascending label)"""
        lab = np.empty(self.n, dtype=np.int32)
        nc = C.c_int64(0)
        _lib.check(self._lib.anr_notegraph_components(self._h, lab.ctypes.data, C.byref(nc)), "anr_notegraph_components")
        labels = lab.astype(np.int64)
        roots = np.flatnonzero(labels == np.arange(self.n))
        if len(roots) != nc.value:
            raise _lib.AnoragError(f"components: {nc.value} roots counted on the device, {len(roots)} in the labels")
        sizes = np.bincount(labels, minlength=self.n)[roots]
        return labels, [int(s) for s in sizes]

    def hop_histogram(self, sources=None) -> np.ndarray:
        """counts[l] = the (source, node) pairs at hop distance l (int64; counts[0] = the sources); ``sources`` = node
        indices, default all nodes.  ``last_bfs_stats``: sources per pass, passes, levels walked, scratch bytes, words,
        microseconds by HIP events."""
        if sources is None:
            ns, ptr, src = self.n, None, None
        else:
            src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
            ns, ptr = len(src), src.ctypes.data
            if ns == 0:  # no pairs to count (and no pointer to tell from "all nodes")
                return np.zeros(0, dtype=np.int64)
        counts = np.zeros(max(self.n, 1), dtype=np.int64)
        nl = C.c_int64(0)
        stats = np.zeros(8, dtype=np.int64)
        _lib.check(self._lib.anr_notegraph_hop_histogram(self._h, ns, ptr, len(counts), counts.ctypes.data, C.byref(nl),
                                                         stats.ctypes.data), "anr_notegraph_hop_histogram")
        self.last_bfs_stats = dict(sources_per_pass=int(stats[0]), passes=int(stats[1]), levels=int(stats[2]),
                                   scratch_bytes=int(stats[3]), words=int(stats[4]), sources=int(stats[5]),
                                   event_us=int(stats[6]))
        return counts[:nl.value].copy()

    def quality_metrics(self, self_loops: int = 0) -> Dict[str, Any]:
        """compute_metrics(G) of graph/graph_quality.py for this graph: the same keys in the same order, floats for the
        three counts, ``component_sizes`` a list of ints.  ``self_loops``: self-loops the nx.Graph has and this graph
        cannot hold; G.degree() counts each twice."""
        labels, sizes = self.components()
        largest = max(sizes)
        root = np.flatnonzero(labels == np.arange(self.n))[sizes.index(largest)]  # the first of the largest
        if largest > 1:
            counts = self.hop_histogram(np.flatnonzero(labels == root))
            total = sum(l * int(c) for l, c in enumerate(counts))
            aspl = total / (largest * (largest - 1))  # nx.average_shortest_path_length's own last line
        else:
            aspl = 0.0
        return {
            "average_degree": (2 * self.n_edges + 2 * int(self_loops)) / float(self.n),
            "num_components": float(len(sizes)),
            "largest_component_size": float(largest),
            "average_shortest_path_length": aspl,
            "component_sizes": sizes,
        }

    # ---- query time ----
    @staticmethod
    def _pack(seed_lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        offs = np.zeros(len(seed_lists) + 1, dtype=np.int64)
        for i, s in enumerate(seed_lists):
            offs[i + 1] = offs[i] + len(s)
        seeds = (np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1) for s in seed_lists])
                 if offs[-1] else np.zeros(0, dtype=np.int64))
        return offs, np.ascontiguousarray(seeds)

    def retrieve_raw(self, seed_lists, cutoff: float = 2.0, cap: Optional[int] = None):
        """(ids [nq, cap] int64 (-1 padded), dist, score [nq, cap] float64, seed_pos [nq, cap] int32, found [nq] int32)"""
        nq = len(seed_lists)
        cap = int(cap or self.n)
        offs, seeds = self._pack(seed_lists)
        ids = np.empty((nq, cap), dtype=np.int64)
        dist = np.empty((nq, cap), dtype=np.float64)
        score = np.empty((nq, cap), dtype=np.float64)
        pos = np.empty((nq, cap), dtype=np.int32)
        cnt = np.zeros(nq, dtype=np.int32)
        _lib.check(self._lib.anr_notegraph_retrieve(self._h, nq, offs.ctypes.data, seeds.ctypes.data, float(cutoff), cap,
                                                    ids.ctypes.data, dist.ctypes.data, score.ctypes.data, pos.ctypes.data,
                                                    cnt.ctypes.data), "anr_notegraph_retrieve")
        return ids, dist, score, pos, cnt

    def retrieve(self, seed_lists, cutoff: float = 2.0, cap: Optional[int] = None) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """per seed list (node indices, list order matters): (ids, dist, score) of the nodes GraphRetriever.retrieve
        returns, best first; at most ``cap`` of them (default: all)"""
        ids, dist, score, _, cnt = self.retrieve_raw(seed_lists, cutoff, cap)
        out = []
        for q in range(len(seed_lists)):
            m = min(int(cnt[q]), ids.shape[1])
            out.append((ids[q, :m].copy(), dist[q, :m].copy(), score[q, :m].copy()))
        return out

    def retrieve_device(self, seed_lists, cutoff: float = 2.0, cap: int = 8192) -> SparseRows:
        """the best ``cap`` nodes per seed list left on the device, rows ascending by id (``counts``: the row lengths,
        ``found``: the nodes found before the cap).  NOT a fuse_dense source as it stands — unlisted ids would read as
        0.0, not as absent: pass it through ``to_array``."""
        nq = len(seed_lists)
        offs, seeds = self._pack(seed_lists)
        rows = SparseRows(nq, self.n, int(cap), self.device)
        found = np.zeros(nq, dtype=np.int32)
        _lib.check(self._lib.anr_notegraph_retrieve_dev(self._h, nq, offs.ctypes.data, seeds.ctypes.data, float(cutoff),
                                                        int(cap), C.c_void_p(rows.ids_ptr), C.c_void_p(rows.scores_ptr),
                                                        C.c_void_p(rows.count_ptr), found.ctypes.data),
                   "anr_notegraph_retrieve_dev")
        rows.found = found
        rows.counts = np.minimum(found, int(cap)).astype(np.int32)
        return rows

    def to_array(self, rows: SparseRows) -> DeviceArray:
        """[nq, n] float64 on the device, NaN where a node was not reached: the ``graph`` source of ``fuse_dense``"""
        arr = DeviceArray(rows.nq, self.n, np.float64, self.device)
        _lib.check(self._lib.anr_notegraph_rows_to_array_dev(self._h, rows.nq, rows.cap, C.c_void_p(rows.ids_ptr),
                                                             C.c_void_p(rows.scores_ptr), C.c_void_p(rows.count_ptr),
                                                             C.c_void_p(arr.ptr)), "anr_notegraph_rows_to_array_dev")
        return arr

    # ---- the reference's shapes ----
    @staticmethod
    def edges_from_relations(atomic_notes: Sequence[Dict[str, Any]], relations: Sequence[Dict[str, Any]]):
        """host half of ``from_relations`` (no device): (note_ids, node dicts, src, dst, weight, importance) of the graph
        GraphBuilder.build_graph makes (graph/graph_builder.py:21-35).  A node's index is its position in the nx.Graph:
        the notes that carry a note_id in list order — graph_index.py:28-35's mapping when every note has a distinct id —
        then any relation endpoint not among them, as add_edge appends it.  A pair related more than once keeps the LAST
        weight (nx.Graph.add_edge overwrites), at the position of its first mention."""
        index: Dict[Any, int] = {}
        nodes: List[Dict[str, Any]] = []
        for note in atomic_notes:
            nid = note.get("note_id")
            if not nid:
                continue
            if nid in index:
                nodes[index[nid]].update(note)
            else:
                index[nid] = len(nodes)
                nodes.append(dict(note))
        edges: Dict[Tuple[int, int], float] = {}
        for rel in relations:
            s, t = rel.get("source_id"), rel.get("target_id")
            if not (s and t):
                continue
            for nid in (s, t):
                if nid not in index:
                    index[nid] = len(nodes)
                    nodes.append({})
            a, b = index[s], index[t]
            if a == b:
                raise ValueError(f"relation {s!r} -> {t!r} is a self-loop: out of scope for NoteGraph")
            edges[(min(a, b), max(a, b))] = float(rel.get("weight", 1.0))
        pairs = np.asarray(list(edges.keys()), dtype=np.int64).reshape(-1, 2)
        w = np.asarray(list(edges.values()), dtype=np.float64)
        imp = np.asarray([float(nd.get("importance_score", 1.0)) for nd in nodes], dtype=np.float64)
        return list(index.keys()), nodes, pairs[:, 0].copy(), pairs[:, 1].copy(), w, imp

    @classmethod
    def from_relations(cls, atomic_notes: Sequence[Dict[str, Any]], relations: Sequence[Dict[str, Any]],
                       device: int = 0) -> "NoteGraph":
        """The note graph of ``edges_from_relations`` on the device; ``importance_score`` of the notes becomes the
        importance.  ``graph_scans.semantic_similarity_relations`` output goes in as it is."""
        note_ids, nodes, src, dst, w, imp = cls.edges_from_relations(atomic_notes, relations)
        if not nodes:
            raise ValueError("NoteGraph.from_relations: the graph has no nodes")
        g = cls(len(nodes), src, dst, w, device)
        g.note_ids = note_ids
        g.note_index = {nid: i for i, nid in enumerate(note_ids)}
        g.nodes = nodes
        if (imp != 1.0).any():
            g.set_importance(imp)
        return g

    def graph_retrieve(self, seed_note_ids: Sequence[Any]) -> List[Dict[str, Any]]:
        """GraphRetriever.retrieve (graph/graph_retriever.py:61-92) on a graph made by ``from_relations``: the reached
        nodes' dicts plus graph_distance, centrality, graph_score and paragraph_idxs, best graph_score first; ``k_hop``
        stays the distance cutoff it is there."""
        if self.nodes is None:
            raise ValueError("graph_retrieve needs the note dicts: build the graph with NoteGraph.from_relations")
        seeds = [self.note_index.get(s, -1) for s in seed_note_ids]
        ids, dist, score, _, cnt = self.retrieve_raw([seeds], float(self.k_hop), self.n)
        out = []
        for i, d, sc in zip(ids[0, :cnt[0]].tolist(), dist[0].tolist(), score[0].tolist()):
            data = dict(self.nodes[i])
            data["graph_distance"] = d
            data["centrality"] = float(self._centrality[i])
            data["graph_score"] = sc
            data["paragraph_idxs"] = self.nodes[i].get("paragraph_idxs", [])
            out.append(data)
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.anr_notegraph_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass
