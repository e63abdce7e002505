// What cluster.hip (anr_index_dbscan) needs of the flat index in index.hip: the blocked f16 image the self join
// multiplies, the float32 rows behind it and the statistics that bound the image's error.
#pragma once
#include <mutex>

#include "common.hpp"

namespace anr {

struct JoinView {
  const float *x32;       // [ntotal][dim] stored (preprocessed) rows
  const uint4 *x16;       // the blocked f16 image (index_kernels.hpp)
  const float *rowbias;   // L2: -0.5 ||x||^2 per row; nullptr on an inner-product index
  int64_t ntotal;
  int dim, dimp, kb, metric, normalize, n_cu;
  float xmax, xerr;       // max ||x||, max ||x16 - x|| over the stored rows
  bool f16_unusable;      // a stored value left the f16 range
  hipStream_t stream;
};

// index.hip; the caller holds the handle's lock (index_core(h).mu): retires the batches in flight, refreshes the statistics
int index_join_view(anr_index *h, JoinView *out);

}  // namespace anr
