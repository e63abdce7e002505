// What the side files need of the flat index in index.hip.  graph.hip (the anr_index_graph_* entry points): the graph
// lives on the anr_index handle and reads its stored float32 rows; it keeps no copy of the corpus.  diversity.hip,
// cluster_quality.hip, kmeans.hip, khop.hip and cluster.hip: the same rows (IndexCore), and for the first four the arenas they keep
// on the handle between calls (IndexScratch).
#pragma once
#include <mutex>

#include "common.hpp"

struct anr_graph;  // graph.hip

namespace anr {

struct IndexCore {
  const float *x32;  // [ntotal][dim] stored (preprocessed) rows
  int64_t ntotal;
  int dim, metric, normalize, device;
  int64_t id_offset;
  hipStream_t stream;  // the handle's own stream (adds, copies)
  std::mutex *mu;      // the handle's lock: held while a graph kernel reads x32
};

// the grow-on-demand device arenas that the analytics calls keep on the handle between calls
struct IndexScratch {
  DevBuf<unsigned char> div_sim;    // anr_index_diversify: the per-query similarity matrices, float64
  DevBuf<unsigned char> div_arena;  // ... every small input and output array of one call
  DevBuf<unsigned char> cq_arena;   // anr_index_cluster_quality: every array of one call
  DevBuf<unsigned char> km_arena;   // anr_index_kmeans: every array of one call
  DevBuf<unsigned char> khop_sim;   // anr_index_cluster_suppress: the per-query Gram matrices, float64
  DevBuf<unsigned char> khop_arena; // anr_index_khop_rerank, anr_index_cluster_suppress: every small array of one call
};

IndexCore index_core(anr_index *h);     // index.hip
IndexScratch &index_scratch(anr_index *h);  // index.hip; touched under the handle's lock
anr_graph *&index_graph(anr_index *h);  // index.hip: the handle's graph state (nullptr until the first graph call)
void graph_mark_stale(anr_graph *g);    // graph.hip: an add or a reset changed the rows (no lock taken)
void graph_free(anr_graph *g);          // graph.hip

}  // namespace anr
