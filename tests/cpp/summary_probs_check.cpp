// CPU check of nngp::summary_column_probs (csrc/summary_select.h, the general
// per-column summary behind nngp_summary_probs) against std::sort under the
// key's own total order (operator< refined by -0.0 < +0.0), for both digit
// widths: every quantile bitwise summary_lerp of the sorted neighbours at the
// rank summary_rank gives (so an exact rank is the sorted value itself), mean
// and sd as stated, every exceedance fraction bitwise the plain count / S, a
// quantile's bits independent of what else was asked, the default request
// bitwise summary_column, and a NaN column all NaN.  Test infrastructure
// (tests/test_summary_probs.py builds and runs it with hipcc, host only, once
// plain and once with the address and undefined-behaviour sanitizers).
#include "summary_select.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool total_less(double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }

static int failures = 0;
static long long checked = 0;

static void fail(const char* what, int bits, long long S, int Q, int K, const char* which, int i, double got,
                 double want) {
  if (++failures <= 40)
    std::printf("FAIL %s bits=%d S=%lld Q=%d K=%d %s %d: got %a want %a\n", what, bits, S, Q, K, which, i, got, want);
}

// Q probabilities that cover 0, 1, a repeat and a descending stretch once Q allows it
static std::vector<double> make_probs(int Q, std::mt19937_64& gen) {
  const double fixed[] = {1.0, 0.0, 0.975, 0.5, 0.5, 0.25, 0.025, 0.9, 0.75, 0.05};
  std::uniform_real_distribution<double> unif(0.0, 1.0);
  std::vector<double> p((size_t)Q);
  for (int i = 0; i < Q; ++i) p[(size_t)i] = i < 10 ? fixed[i] : unif(gen);
  return p;
}

template <int BITS>
static void check_column(const char* what, const std::vector<double>& x, const std::vector<double>& probs,
                         const std::vector<double>& thr) {
  const long long S = (long long)x.size();
  const int Q = (int)probs.size(), K = (int)thr.size();
  auto load = [&](long long s) { return x[(size_t)s]; };
  const double mark = -12345.678;
  std::vector<double> out((size_t)(2 + Q + K) + 1, mark);
  nngp::summary_column_probs<BITS>(load, S, probs.data(), Q, thr.data(), K, out.data(), 1);
  if (!same(out.back(), mark)) fail(what, BITS, S, Q, K, "wrote past the end", 0, out.back(), mark);
  std::vector<double> y = x;
  std::sort(y.begin(), y.end(), total_less);
  double sum = 0;
  for (double v : x) sum += v;
  const double mean = sum / (double)S;
  if (!same(out[0], mean)) fail(what, BITS, S, Q, K, "mean", 0, out[0], mean);
  double ss = 0;
  for (double v : x) {
#pragma clang fp contract(off)  // the two-pass sum as stated: product rounded, then added
    const double d = v - mean;
    ss += d * d;
  }
  const double sd = std::sqrt(ss / (double)(S - 1));
  if (S == 1 ? out[(size_t)(1 + Q)] == out[(size_t)(1 + Q)] : !same(out[(size_t)(1 + Q)], sd))
    fail(what, BITS, S, Q, K, "sd", 0, out[(size_t)(1 + Q)], sd);
  for (int i = 0; i < Q; ++i) {
    long long j;
    double g;
    nngp::summary_rank(probs[(size_t)i], S, &j, &g);
    const double a = y[(size_t)j], b = y[(size_t)(j + 1 < S ? j + 1 : j)];
    const double want = nngp::summary_lerp(a, b, g);
    const double got = out[(size_t)(1 + i)];
    if (!same(got, want) || (g == 0.0 && !same(got, a))) fail(what, BITS, S, Q, K, "quantile", i, got, want);
    if (probs[(size_t)i] == 0.0 && !same(got, y.front())) fail(what, BITS, S, Q, K, "minimum", i, got, y.front());
    if (probs[(size_t)i] == 1.0 && !same(got, y.back())) fail(what, BITS, S, Q, K, "maximum", i, got, y.back());
    // the same q asked alone, without thresholds: the same bits
    double alone[3];
    nngp::summary_column_probs<BITS>(load, S, &probs[(size_t)i], 1, nullptr, 0, alone, 1);
    if (!same(alone[1], got)) fail(what, BITS, S, Q, K, "quantile asked alone", i, alone[1], got);
    ++checked;
  }
  for (int k = 0; k < K; ++k) {
    long long count = 0;
    for (double v : x) count += v > thr[(size_t)k];
    const double want = (double)count / (double)S;
    if (!same(out[(size_t)(2 + Q + k)], want)) fail(what, BITS, S, Q, K, "exceedance", k, out[(size_t)(2 + Q + k)], want);
    ++checked;
  }
}

template <int BITS>
static void check_default(const char* what, const std::vector<double>& x) {
  const long long S = (long long)x.size();
  auto load = [&](long long s) { return x[(size_t)s]; };
  const double q[3] = {0.025, 0.5, 0.975};
  double five[5], got[5];
  nngp::summary_column<BITS>(load, S, five);
  nngp::summary_column_probs<BITS>(load, S, q, 3, nullptr, 0, got, 1);
  for (int i = 0; i < 5; ++i)
    if (!same(five[i], got[i])) fail(what, BITS, S, 3, 0, "parity with summary_column", i, got[i], five[i]);
}

static void check(const char* what, const std::vector<double>& x, std::mt19937_64& gen) {
  const double inf = std::numeric_limits<double>::infinity();
  // thresholds: a data value, both infinities, both zeros, values inside the data's range
  const double all_thr[8] = {x[x.size() / 2], -inf, inf, 0.0, -0.0, 3.0, x[0], -0.7};
  for (int Q : {0, 1, 2, 3, 4, 6, 7, 16}) {
    const std::vector<double> probs = make_probs(Q, gen);
    const int K = Q % 3 == 0 ? 8 : Q % 3 == 1 ? 0 : 3;
    const std::vector<double> thr(all_thr, all_thr + K);
    check_column<2>(what, x, probs, thr);
    check_column<4>(what, x, probs, thr);
  }
  // every threshold count 0..8 once per column, with the default probabilities
  for (int K = 0; K <= 8; ++K) check_column<4>(what, x, {0.025, 0.5, 0.975}, std::vector<double>(all_thr, all_thr + K));
  check_default<2>(what, x);
  check_default<4>(what, x);
}

int main() {
  std::mt19937_64 gen(20261);
  std::normal_distribution<double> normal(0.0, 1.0);
  int columns = 0;
  for (long long S : {1, 2, 3, 5, 41, 64, 65, 257}) {
    std::vector<double> x((size_t)S);
    for (double& v : x) v = 3.0 + 2.0 * normal(gen);
    check("normal", x, gen);
    for (double& v : x) v = -0.7;
    check("all-equal", x, gen);
    const double three[3] = {-2.0, 0.0, 5.0};
    for (double& v : x) v = three[gen() % 3];
    check("three-valued", x, gen);
    for (double& v : x) v = (gen() & 1) ? 0.0 : -0.0;
    check("signed zeros", x, gen);
    for (double& v : x) v = (gen() % 5 == 0) ? ((gen() & 1) ? 1e300 : -1e300) : normal(gen) * 4.9406564584124654e-324 * 1000.0;
    check("subnormals and 1e300", x, gen);
    for (long long s = 0; s < S; ++s) x[(size_t)s] = 1e3 - 0.37 * (double)s;
    check("decreasing", x, gen);
    columns += 6;
  }
  // signed zeros against the threshold 0.0: neither zero exceeds it
  {
    const std::vector<double> x = {-0.0, 0.0, 0.0, -0.0, 1.0};
    const double thr[2] = {0.0, -0.0};
    double out[4];
    nngp::summary_column_probs<4>([&](long long s) { return x[(size_t)s]; }, 5, nullptr, 0, thr, 2, out, 1);
    if (!same(out[2], 0.2) || !same(out[3], 0.2)) fail("zeros", 4, 5, 0, 2, "exceedance", 0, out[2], 0.2);
  }
  // infinite entries: ranks and counts are exact, +inf never exceeds +inf
  {
    const double inf = std::numeric_limits<double>::infinity();
    const std::vector<double> x = {inf, -1.0, -inf, 2.0, inf};
    const double probs[3] = {0.0, 0.5, 1.0}, thr[3] = {inf, -inf, 2.0};
    double out[8];
    nngp::summary_column_probs<2>([&](long long s) { return x[(size_t)s]; }, 5, probs, 3, thr, 3, out, 1);
    const double want[3] = {-inf, 2.0, inf}, frac[3] = {0.0, 0.8, 0.4};
    for (int i = 0; i < 3; ++i) {
      if (!same(out[1 + i], want[i])) fail("infinities", 2, 5, 3, 3, "quantile", i, out[1 + i], want[i]);
      if (!same(out[5 + i], frac[i])) fail("infinities", 2, 5, 3, 3, "exceedance", i, out[5 + i], frac[i]);
    }
  }
  // a NaN anywhere in a column: every output NaN, the strided store touches its own slots only
  for (int Q : {0, 3, 16}) {
    std::vector<double> x(41, 1.0);
    x[17] = std::nan("");
    const std::vector<double> probs = make_probs(Q, gen);
    const double thr[8] = {0.0, 1.0, 2.0, -1.0, 0.5, 1.5, 3.0, -3.0};
    const int cols = 2 + Q + 8;
    std::vector<double> out((size_t)cols * 3, 7.0);
    nngp::summary_column_probs<4>([&](long long s) { return x[(size_t)s]; }, 41, probs.data(), Q, thr, 8, out.data() + 1, 3);
    for (int i = 0; i < cols; ++i) {
      if (out[(size_t)i * 3 + 1] == out[(size_t)i * 3 + 1]) fail("NaN column", 4, 41, Q, 8, "not NaN", i, out[(size_t)i * 3 + 1], 0);
      if (!same(out[(size_t)i * 3], 7.0) || !same(out[(size_t)i * 3 + 2], 7.0)) fail("NaN column", 4, 41, Q, 8, "stride", i, 0, 7.0);
    }
  }
  std::printf("%s columns %d values %lld failures %d\n", failures ? "FAILED" : "ok", columns, checked, failures);
  return failures ? 1 : 0;
}
