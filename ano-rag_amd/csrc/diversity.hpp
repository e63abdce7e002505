// What diversity.hip (anr_index_diversify) needs of the flat index in index.hip: the stored float32 rows (IndexCore,
// graph.hpp) and a slot on the handle for the scratch it keeps between calls.
#pragma once
#include "graph.hpp"

struct anr_diversity;  // diversity.hip

namespace anr {

anr_diversity *&index_diversity(anr_index *h);  // index.hip: the handle's scratch (nullptr until the first call)
void diversity_free(anr_diversity *d);          // diversity.hip

}  // namespace anr
