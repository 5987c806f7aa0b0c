// CPU check of nngp::summary_select / summary_column (csrc/summary_select.h, the
// per-column selection loop of the device get_summary) against
// std::nth_element: every wanted rank x_(j) and its successor x_(j+1) bitwise,
// for both digit widths the kernel is instantiated with.  nth_element runs
// under the key's own total order (operator< refined by -0.0 < +0.0), which
// is one of the answers operator< allows and the only one that is defined
// bit for bit on columns mixing the two zeros.  Test infrastructure
// (tests/test_summary_select.py builds and runs it with hipcc, host only).
#include "summary_select.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool total_less(double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }

static int failures = 0;

template <int BITS>
static void check_column(const char* what, const std::vector<double>& x) {
  const long long S = (long long)x.size();
  const double q[3] = {0.025, 0.5, 0.975};
  long long j[3];
  double g[3], lo[3], hi[3];
  for (int r = 0; r < 3; ++r) nngp::summary_rank(q[r], S, &j[r], &g[r]);
  auto load = [&](long long s) { return x[(size_t)s]; };
  nngp::summary_select<BITS>(load, S, j, true, lo, hi);
  for (int r = 0; r < 3; ++r) {
    std::vector<double> y = x;
    std::nth_element(y.begin(), y.begin() + j[r], y.end(), total_less);
    const double a = y[(size_t)j[r]];
    const long long j1 = j[r] + 1 < S ? j[r] + 1 : j[r];
    std::nth_element(y.begin(), y.begin() + j1, y.end(), total_less);
    const double b = y[(size_t)j1];
    if (!same(lo[r], a) || !same(hi[r], b)) {
      ++failures;
      std::printf("FAIL %s bits=%d S=%lld rank %lld: got %a, %a want %a, %a\n", what, BITS, S, j[r], lo[r], hi[r], a, b);
    }
  }
  // the whole column summary: quantiles by the same ranks, mean and sd as stated
  double out[5];
  nngp::summary_column<BITS>(load, S, out);
  double sum = 0;
  for (double v : x) sum += v;
  const double mean = sum / (double)S;
  if (!same(out[0], mean)) {
    ++failures;
    std::printf("FAIL %s bits=%d S=%lld mean\n", what, BITS, S);
  }
  for (int r = 0; r < 3; ++r) {
    const double want = nngp::summary_lerp(lo[r], hi[r], g[r]);
    if (!same(out[1 + r], want) || !(out[1 + r] >= lo[r] && out[1 + r] <= hi[r]) || (g[r] == 0.0 && !same(out[1 + r], lo[r]))) {
      ++failures;
      std::printf("FAIL %s bits=%d S=%lld quantile %d\n", what, BITS, S, r);
    }
  }
  if ((S == 1) != (out[4] != out[4])) {
    ++failures;
    std::printf("FAIL %s bits=%d S=%lld sd %g\n", what, BITS, S, out[4]);
  }
}

static void check(const char* what, const std::vector<double>& x) {
  check_column<2>(what, x);
  check_column<4>(what, x);
}

int main() {
  // the key is a bijection that keeps the order
  const double pts[] = {-1e300, -1.0, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1e300};
  for (size_t i = 0; i < sizeof pts / sizeof *pts; ++i) {
    if (!same(nngp::summary_unkey(nngp::summary_key(pts[i])), pts[i])) ++failures;
    if (i && !(nngp::summary_key(pts[i - 1]) < nngp::summary_key(pts[i]))) ++failures;
  }
  std::mt19937_64 gen(20240);
  std::normal_distribution<double> normal(0.0, 1.0);
  int columns = 0;
  for (long long S : {1, 2, 3, 41, 64, 65, 1000}) {
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<double> x((size_t)S);
      for (double& v : x) v = 3.0 + 2.0 * normal(gen);
      check("normal", x);
      for (double& v : x) v = -0.7;
      check("all-equal", x);
      const double three[3] = {-2.0, 0.0, 5.0};
      for (double& v : x) v = three[gen() % 3];
      check("three-valued", x);
      for (double& v : x) v = (gen() & 1) ? 0.0 : -0.0;
      check("signed zeros", x);
      for (double& v : x) {
        const unsigned k = (unsigned)(gen() % 6);
        const double sub = (double)(1 + gen() % 1000) * 4.9406564584124654e-324;
        v = k == 0 ? 1e300 : k == 1 ? -1e300 : (k & 1) ? sub : -sub;
      }
      check("subnormals and 1e300", x);
      for (long long s = 0; s < S; ++s) x[(size_t)s] = 1e3 - 0.37 * (double)s - (double)rep;
      check("decreasing", x);
      columns += 6;
    }
  }
  // a NaN anywhere in a column: five NaNs
  {
    std::vector<double> x(41, 1.0);
    x[17] = std::nan("");
    double out[5];
    nngp::summary_column<2>([&](long long s) { return x[(size_t)s]; }, 41, out);
    for (double v : out)
      if (v == v) ++failures;
  }
  std::printf("%s columns %d failures %d\n", failures ? "FAILED" : "ok", columns, failures);
  return failures ? 1 : 0;
}
