// What cluster_quality.hip (anr_index_cluster_quality) needs of the flat index in index.hip: the stored float32 rows
// (IndexCore, graph.hpp) and a slot on the handle for the scratch it keeps between calls.
#pragma once
#include "graph.hpp"

struct anr_cluster_quality;  // cluster_quality.hip

namespace anr {

anr_cluster_quality *&index_cluster_quality(anr_index *h);  // index.hip: the handle's scratch (nullptr until the first call)
void cluster_quality_free(anr_cluster_quality *q);          // cluster_quality.hip

}  // namespace anr
