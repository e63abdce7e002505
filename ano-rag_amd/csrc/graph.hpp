// What graph.hip (the anr_index_graph_* entry points) needs of the flat index in index.hip.  The graph lives on the
// anr_index handle and reads its stored float32 rows; it keeps no copy of the corpus.
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

IndexCore index_core(anr_index *h);     // index.hip
anr_graph *&index_graph(anr_index *h);  // index.hip: the handle's graph state (nullptr until the first graph call)
void graph_mark_stale(anr_graph *g);    // graph.hip: an add or a reset changed the rows (no lock taken)
void graph_free(anr_graph *g);          // graph.hip

}  // namespace anr
