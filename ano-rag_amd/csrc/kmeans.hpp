// What kmeans.hip (anr_index_kmeans) needs of the flat index in index.hip: the stored float32 rows (IndexCore, graph.hpp)
// and a slot on the handle for the scratch it keeps between calls.
#pragma once
#include "graph.hpp"

struct anr_kmeans;  // kmeans.hip

namespace anr {

anr_kmeans *&index_kmeans(anr_index *h);  // index.hip: the handle's scratch (nullptr until the first call)
void kmeans_free(anr_kmeans *q);          // kmeans.hip

}  // namespace anr
