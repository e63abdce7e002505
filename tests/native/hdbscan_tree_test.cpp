// Stand-alone driver of csrc/hdbscan_tree.hpp (host-only, no HIP), built by tests/test_hdbscan_cpu.py with
// -fsanitize=address,undefined.  Reads trees from stdin, one per block:
//   n min_cluster_size eps        (eps as a C hexadecimal float)
//   src dst w                     (n - 1 lines; w as a hexadecimal float)
// and prints per tree one line: "ok <n_clusters> <label> ..." or "error <message>".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hdbscan_tree.hpp"

int main() {
  long long n;
  int mcs;
  char eps_text[64];
  while (std::scanf("%lld %d %63s", &n, &mcs, eps_text) == 3) {
    const double eps = std::strtod(eps_text, nullptr);
    const size_t m = n > 1 ? (size_t)(n - 1) : 0;
    std::vector<int64_t> src(m), dst(m);
    std::vector<double> w(m);
    for (size_t i = 0; i < m; ++i) {
      long long a, b;
      char wt[64];
      if (std::scanf("%lld %lld %63s", &a, &b, wt) != 3) return 2;
      src[i] = a, dst[i] = b, w[i] = std::strtod(wt, nullptr);
    }
    std::vector<int32_t> labels(n > 0 ? (size_t)n : 0);
    int64_t stats[8];
    std::string err;
    if (anr::hdbscan_labels_host(n, src.data(), dst.data(), w.data(), mcs, eps, labels.data(), stats, &err) != 0) {
      std::printf("error %s\n", err.c_str());
      continue;
    }
    std::printf("ok %lld", (long long)stats[0]);
    for (int32_t v : labels) std::printf(" %d", v);
    std::printf("\n");
  }
  return 0;
}
