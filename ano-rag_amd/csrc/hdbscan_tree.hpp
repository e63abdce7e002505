// The tree stage of HDBSCAN (anr_hdbscan_labels, include/anorag.h): from the N - 1 edges of the mutual-reachability
// spanning tree to labels.  Host-only C++ (no HIP): O(N log N) sequential pointer work; tests/native/hdbscan_tree_test.cpp
// drives it under g++ with the sanitizers, hdbscan.hip exports it.  The steps are sklearn 1.7's for
// HDBSCAN(min_cluster_size, cluster_selection_epsilon, cluster_selection_method='eom', allow_single_cluster=False), restated
// in tests/hdbscan_ref.py (labels_from_mst, tie_order='stable'), with ONE order for edges of equal weight where sklearn's
// np.argsort leaves it open: they keep the order they were given in (Prim's).
//   1. std::stable_sort of the edges by weight.
//   2. Single linkage by union-find: merge i makes node n + i of the two nodes holding the edge's ends, sizes added.
//   3. Condensed tree, breadth-first from the last merge with lambda = 1 / weight (inf at weight 0): where both sides have
//      min_cluster_size rows two new clusters are born (left, then right, ids ascending); otherwise the rows of a side below
//      min_cluster_size leave the cluster at that lambda and the other side carries the cluster's id on.
//   4. Stability: the sum of (lambda - lambda_birth) * size over what leaves a cluster, one row at a time, in that order
//      (float64 sums are not associative; this is the order sklearn adds in).
//   5. Excess of mass from the highest id down: a cluster whose children's stabilities add to more than its own is given
//      up for them (and takes that sum), otherwise everything below it is given up.  The root is never a cluster.
//   6. eps != 0: a chosen cluster born at a distance 1 / lambda < eps gives way to its first ancestor born above eps,
//      or to its ancestor just below the root.
//   7. A row takes the first chosen cluster at or above the cluster it left; none: noise, -1.  Labels number the chosen
//      clusters by ascending id.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

namespace anr {

// 0, or -1 with *err set.  stats (may be null): n_clusters, n_noise, condensed clusters (the root included), tied edges,
// true splits, rows that took an ancestor's label through eps, 0, 0.
inline int hdbscan_labels_host(int64_t n, const int64_t *src, const int64_t *dst, const double *w, int32_t min_cluster_size,
                               double eps, int32_t *labels, int64_t *stats, std::string *err) {
  auto bad = [&](const std::string &m) {
    if (err) *err = m;
    return -1;
  };
  if (n < 2) return bad("hdbscan labels: n = " + std::to_string(n) + ", at least 2 rows are needed");
  if (n > (int64_t)1 << 30) return bad("hdbscan labels: too many rows for one call");
  if (!src || !dst || !w || !labels) return bad("hdbscan labels: null src, dst, w or labels");
  if (min_cluster_size < 2) return bad("hdbscan labels: min_cluster_size = " + std::to_string(min_cluster_size) + ", at least 2 is needed");
  if (!(eps >= 0.0)) return bad("hdbscan labels: cluster_selection_epsilon must not be negative");
  const int64_t m = n - 1;
  for (int64_t i = 0; i < m; ++i) {
    if (src[i] < 0 || src[i] >= n || dst[i] < 0 || dst[i] >= n)
      return bad("hdbscan labels: edge " + std::to_string(i) + " names a row outside 0 .. n - 1");
    if (!(w[i] >= 0.0) || std::isinf(w[i])) return bad("hdbscan labels: the weight of edge " + std::to_string(i) + " is not a finite non-negative number");
  }

  std::vector<int64_t> order((size_t)m);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return w[a] < w[b]; });
  int64_t ties = 0;
  for (int64_t i = 1; i < m; ++i) ties += w[order[(size_t)i]] == w[order[(size_t)i - 1]];

  // single linkage
  std::vector<int64_t> up((size_t)(2 * n - 1)), size((size_t)(2 * n - 1), 1), left((size_t)m), right((size_t)m);
  std::vector<double> height((size_t)m);
  std::iota(up.begin(), up.end(), (int64_t)0);
  auto find = [&](int64_t a) {
    int64_t r = a;
    while (up[(size_t)r] != r) r = up[(size_t)r];
    while (up[(size_t)a] != r) {
      const int64_t next = up[(size_t)a];
      up[(size_t)a] = r;
      a = next;
    }
    return r;
  };
  for (int64_t i = 0; i < m; ++i) {
    const int64_t e = order[(size_t)i];
    const int64_t a = find(src[e]), b = find(dst[e]);
    if (a == b) return bad("hdbscan labels: the edges do not form a spanning tree (edge " + std::to_string(e) + " closes a cycle)");
    left[(size_t)i] = a, right[(size_t)i] = b, height[(size_t)i] = w[e];
    size[(size_t)(n + i)] = size[(size_t)a] + size[(size_t)b];
    up[(size_t)a] = up[(size_t)b] = n + i;
  }

  // condensed tree; cluster c is index c - n of these
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<int64_t> parent_of{0}, child0{-1};  // a cluster has no children or two, with consecutive indices
  std::vector<double> birth{0.0}, stability{0.0};
  std::vector<int64_t> point_cluster((size_t)n, 0);
  std::vector<std::pair<int64_t, int64_t>> queue;  // (node, cluster index), first in first out
  queue.reserve((size_t)m);
  queue.emplace_back(2 * n - 2, 0);
  std::vector<int64_t> stack;
  int64_t splits = 0;
  for (size_t head = 0; head < queue.size(); ++head) {
    const int64_t node = queue[head].first, c = queue[head].second;
    const int64_t side[2] = {left[(size_t)(node - n)], right[(size_t)(node - n)]};
    const double dd = height[(size_t)(node - n)];
    const double lam = dd > 0.0 ? 1.0 / dd : inf;
    const bool big[2] = {size[(size_t)side[0]] >= min_cluster_size, size[(size_t)side[1]] >= min_cluster_size};
    if (big[0] && big[1]) {
      ++splits;
      child0[(size_t)c] = (int64_t)parent_of.size();
      for (int s = 0; s < 2; ++s) {
        const int64_t cc = (int64_t)parent_of.size();
        parent_of.push_back(c), child0.push_back(-1), birth.push_back(lam), stability.push_back(0.0);
        stability[(size_t)c] += (lam - birth[(size_t)c]) * (double)size[(size_t)side[s]];
        queue.emplace_back(side[s], cc);
      }
    } else {
      for (int s = 0; s < 2; ++s) {
        if (big[s]) {
          queue.emplace_back(side[s], c);
          continue;
        }
        stack.assign(1, side[s]);
        while (!stack.empty()) {
          const int64_t v = stack.back();
          stack.pop_back();
          if (v < n) {
            point_cluster[(size_t)v] = c;
            stability[(size_t)c] += (lam - birth[(size_t)c]) * 1.0;
          } else {
            stack.push_back(left[(size_t)(v - n)]);
            stack.push_back(right[(size_t)(v - n)]);
          }
        }
      }
    }
  }
  const int64_t n_cl = (int64_t)parent_of.size();

  // every cluster below c
  auto below = [&](int64_t c, auto &&f) {
    stack.clear();
    if (child0[(size_t)c] >= 0) stack.push_back(child0[(size_t)c]), stack.push_back(child0[(size_t)c] + 1);
    while (!stack.empty()) {
      const int64_t v = stack.back();
      stack.pop_back();
      f(v);
      if (child0[(size_t)v] >= 0) stack.push_back(child0[(size_t)v]), stack.push_back(child0[(size_t)v] + 1);
    }
  };

  std::vector<char> selected((size_t)n_cl, 1);
  selected[0] = 0;
  for (int64_t c = n_cl - 1; c >= 1; --c) {
    double sub = 0.0;
    if (child0[(size_t)c] >= 0) {
      sub = sub + stability[(size_t)child0[(size_t)c]];
      sub = sub + stability[(size_t)child0[(size_t)c] + 1];
    }
    if (sub > stability[(size_t)c]) {
      selected[(size_t)c] = 0;
      stability[(size_t)c] = sub;
    } else {
      below(c, [&](int64_t v) { selected[(size_t)v] = 0; });
    }
  }

  std::vector<char> climbed((size_t)n_cl, 0);
  if (eps != 0.0 && n_cl > 1) {
    std::vector<char> chosen((size_t)n_cl, 0), done((size_t)n_cl, 0);
    for (int64_t c = n_cl - 1; c >= 1; --c) {
      if (!selected[(size_t)c]) continue;
      if (1.0 / birth[(size_t)c] < eps) {
        if (done[(size_t)c]) continue;
        int64_t v = c;
        for (;;) {
          const int64_t p = parent_of[(size_t)v];
          if (p == 0) break;
          v = p;
          if (1.0 / birth[(size_t)p] > eps) break;
        }
        chosen[(size_t)v] = 1;
        if (v != c) climbed[(size_t)v] = 1;
        below(v, [&](int64_t u) { done[(size_t)u] = 1; });
      } else {
        chosen[(size_t)c] = 1;
      }
    }
    selected = chosen;
  }

  std::vector<int32_t> number((size_t)n_cl, -1);
  int32_t n_clusters = 0;
  for (int64_t c = 1; c < n_cl; ++c)
    if (selected[(size_t)c]) number[(size_t)c] = n_clusters++;
  int64_t n_noise = 0, n_climbed = 0;
  for (int64_t p = 0; p < n; ++p) {
    int64_t c = point_cluster[(size_t)p];
    while (c != 0 && !selected[(size_t)c]) c = parent_of[(size_t)c];
    labels[p] = c != 0 ? number[(size_t)c] : -1;
    n_noise += c == 0;
    n_climbed += c != 0 && climbed[(size_t)c];
  }
  if (stats) {
    std::fill(stats, stats + 8, (int64_t)0);
    stats[0] = n_clusters, stats[1] = n_noise, stats[2] = n_cl, stats[3] = ties, stats[4] = splits, stats[5] = n_climbed;
  }
  return 0;
}

}  // namespace anr
