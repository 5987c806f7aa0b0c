// A "hub" column for the layout checks (layout_check.cpp, tile_sweep_check.cpp):
// the last neighbour of random later rows is rewired to location `hub` until
// the location appears in exactly H entries of the NNarray (its own row
// counted, as capi.hip's max_column_length counts it), then the graph is
// recoloured.  The same construction as hub_problem() of
// tests/test_gpu_irregular_graphs.py: a column of B of H entries in a graph
// whose other columns stay a small multiple of m + 1.
#pragma once
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "graph_prep.h"

// nn: row-major 0-based, -1 = NA (graph_prep.h).  Returns the column length
// reached (H when the graph has enough rows to rewire), K through *K_out.
inline int add_hub_column(std::vector<int>& nn, int n, int b, int H, std::mt19937_64& g, std::vector<int>& col,
                          int* K_out, int hub = 7) {
  const int m = b - 1;
  int have = 0;
  std::vector<int> cand;
  for (int k = 0; k < n; ++k) {
    bool has = false;
    for (int u = 0; u < b; ++u) has = has || nn[(size_t)k * b + u] == hub;
    have += has;
    if (!has && k > std::max(hub, m)) cand.push_back(k);
  }
  std::shuffle(cand.begin(), cand.end(), g);
  for (size_t q = 0; q < cand.size() && have < H; ++q, ++have) nn[(size_t)cand[q] * b + m] = hub;
  *K_out = nngp::greedy_coloring(nn.data(), n, b, col);
  return have;
}
