// Host check of build_predict_plan (graph_prep.h): the plan of the batched
// prediction from the stacked NNarray.  No arguments: the plans of dense
// uniform new points over few observed ones (m = 5 and 15), a line of new
// points (depth = n_pred) and n = 3 with NA padding (also one new location)
// are checked against their defining properties, and bad tables are rejected.
// `dump n n_pred b in out`: the plan of the int32 column-major table in file
// `in`, written to `out` as int32 {n_support, n_levels, support, nn,
// level_ptr, level_rows} (compared with numpy by tests/test_predict_plan.py).
// Built with -fsanitize=address,undefined together with graph_prep.cpp.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "graph_prep.h"

using namespace nngp;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++fails;                                                     \
    }                                                              \
  } while (0)

// stacked table (column-major, 1-based, NA = INT_MIN) of observed + new points
static std::vector<int> stacked_table(const std::vector<double>& xy, int N, int m) {
  std::vector<int> rm;
  find_ordered_nn(xy.data(), N, 2, m, rm);
  const int b = m + 1;
  std::vector<int> cm((size_t)N * b);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < b; ++j) cm[i + (size_t)j * N] = rm[(size_t)i * b + j] < 0 ? INT_MIN : rm[(size_t)i * b + j] + 1;
  return cm;
}

static void check_plan(const std::vector<int>& cm, int n, int n_pred, int b, int want_depth) {
  PredictPlan P;
  std::string err;
  const size_t N = (size_t)n + n_pred;
  CHECK(build_predict_plan(cm.data(), n, n_pred, b, P, err));
  if (fails) return;
  // support: sorted, unique, exactly the observed indices the new rows name
  std::set<int> named;
  for (int r = 0; r < n_pred; ++r)
    for (int j = 1; j < b; ++j) {
      const int v = cm[n + r + (size_t)j * N];
      if (v != INT_MIN && v <= n) named.insert(v - 1);
    }
  CHECK(P.n_support == (int)named.size() && (int)P.support.size() == P.n_support);
  CHECK(std::is_sorted(P.support.begin(), P.support.end()));
  CHECK(std::adjacent_find(P.support.begin(), P.support.end()) == P.support.end());
  CHECK(std::equal(P.support.begin(), P.support.end(), named.begin()));
  // the remapped table round-trips to the original
  CHECK(P.nn.size() == (size_t)n_pred * b);
  for (int r = 0; r < n_pred; ++r)
    for (int j = 0; j < b; ++j) {
      const int v = cm[n + r + (size_t)j * N], e = P.nn[(size_t)r * b + j];
      if (v == INT_MIN) {
        CHECK(e == -1);
      } else {
        CHECK(e >= 0 && e < P.n_support + n_pred);
        const int back = e < P.n_support ? P.support[e] : n + (e - P.n_support);
        CHECK(back == v - 1);
      }
    }
  // levels: a partition of the new rows; new-row neighbours in strictly
  // earlier levels; level = 1 + the largest of them
  CHECK((int)P.level_ptr.size() == P.n_levels + 1 && P.level_ptr[0] == 0 && P.level_ptr[P.n_levels] == n_pred);
  std::vector<int> level(n_pred, 0);
  for (int l = 0; l < P.n_levels; ++l) {
    CHECK(P.level_ptr[l + 1] > P.level_ptr[l]);
    for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
      const int r = P.level_rows[q];
      CHECK(r >= 0 && r < n_pred && level[r] == 0);
      level[r] = l + 1;
    }
  }
  for (int r = 0; r < n_pred; ++r) {
    int want = 1;
    for (int j = 1; j < b; ++j) {
      const int e = P.nn[(size_t)r * b + j];
      if (e >= P.n_support) {
        CHECK(level[e - P.n_support] < level[r]);
        want = std::max(want, level[e - P.n_support] + 1);
      }
    }
    CHECK(level[r] == want);
  }
  if (want_depth > 0) CHECK(P.n_levels == want_depth);
  std::printf("n=%d n_pred=%d b=%d: support %d, depth %d\n", n, n_pred, b, P.n_support, P.n_levels);
}

static std::vector<double> points(int n, int n_pred, unsigned seed, bool line) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  const int N = n + n_pred;
  std::vector<double> xy((size_t)N * 2);
  for (int i = 0; i < N; ++i) {
    xy[i] = u(g);
    xy[i + (size_t)N] = u(g);
    if (line && i >= n) {
      xy[i] = 0.1 + 0.8 * (i - n) / (double)(n_pred - 1);
      xy[i + (size_t)N] = 0.5;
    }
  }
  return xy;
}

static int dump(int n, int n_pred, int b, const char* in, const char* out) {
  const size_t N = (size_t)n + n_pred;
  std::vector<int> cm(N * b);
  FILE* f = std::fopen(in, "rb");
  if (!f || std::fread(cm.data(), sizeof(int), cm.size(), f) != cm.size()) return 2;
  std::fclose(f);
  PredictPlan P;
  std::string err;
  if (!build_predict_plan(cm.data(), n, n_pred, b, P, err)) {
    std::printf("%s\n", err.c_str());
    return 3;
  }
  f = std::fopen(out, "wb");
  if (!f) return 2;
  const int head[2] = {P.n_support, P.n_levels};
  std::fwrite(head, sizeof(int), 2, f);
  std::fwrite(P.support.data(), sizeof(int), P.support.size(), f);
  std::fwrite(P.nn.data(), sizeof(int), P.nn.size(), f);
  std::fwrite(P.level_ptr.data(), sizeof(int), P.level_ptr.size(), f);
  std::fwrite(P.level_rows.data(), sizeof(int), P.level_rows.size(), f);
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && std::string(argv[1]) == "dump")
    return dump(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), argv[5], argv[6]);
  check_plan(stacked_table(points(300, 1500, 1, false), 1800, 5), 300, 1500, 6, 0);
  check_plan(stacked_table(points(300, 1500, 2, false), 1800, 15), 300, 1500, 16, 0);
  check_plan(stacked_table(points(500, 600, 3, true), 1100, 5), 500, 600, 6, 600);
  check_plan(stacked_table(points(3, 10, 4, false), 13, 5), 3, 10, 6, 0);
  check_plan(stacked_table(points(3, 1, 5, false), 4, 5), 3, 1, 6, 1);
  // rejected: a new row naming a later row, itself beyond column 0, a wrong column 0
  {
    const int n = 3, n_pred = 10, b = 6, N = 13;
    const std::vector<int> good = stacked_table(points(n, n_pred, 4, false), N, 5);
    PredictPlan P;
    std::string err;
    std::vector<int> t = good;
    t[(n + 2) + (size_t)1 * N] = n + 5;  // row n+2 (0-based) names the later row n+4
    CHECK(!build_predict_plan(t.data(), n, n_pred, b, P, err) && !err.empty());
    t = good;
    t[(n + 2) + (size_t)2 * N] = n + 3;  // itself beyond column 0
    CHECK(!build_predict_plan(t.data(), n, n_pred, b, P, err));
    t = good;
    t[(n + 2) + (size_t)0 * N] = n + 2;  // column 0 is not the row itself
    CHECK(!build_predict_plan(t.data(), n, n_pred, b, P, err));
    t = good;
    t[(n + 2) + (size_t)1 * N] = 0;  // index < 1
    CHECK(!build_predict_plan(t.data(), n, n_pred, b, P, err));
    t = good;
    t[0] = 99;  // rows of the observed locations are not read
    CHECK(build_predict_plan(t.data(), n, n_pred, b, P, err));
    CHECK(!build_predict_plan(good.data(), n, 0, b, P, err));
  }
  std::printf(fails ? "predict_plan_check: %d failures\n" : "predict_plan_check ok\n", fails);
  return fails ? 1 : 0;
}
