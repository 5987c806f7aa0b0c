// CPU check of nngp::field_diag_ess / field_diag_combine (csrc/field_diag.h, the
// per-column part of the device field diagnostics) against a long double
// restatement in this file: AR(1) columns of S in {4, 5, 37, 300, 1000} with
// rho in {0, 0.5, 0.9, 0.99}, and crafted acf arrays.  The order must be the
// restatement's wherever its two lowest AICs lie >= 1e-6 apart (asserted for
// every column here); ess within 8 (S + P) eps / min(1, (1 - sum phi)^2):
// each acf[l] carries at most (S + 2) eps / 2 of acf[0] (recursive summation,
// Cauchy-Schwarz), ess = S acf[0] (1 - sum phi)^2 / v turns an error of sum
// phi into twice that over 1 - sum phi, and the Yule-Walker solve magnifies
// the acf's error into phi by about as much again for a root near 1.
// An a-priori bound: the columns here use at most 0.15 of it (printed).
// Test infrastructure (tests/test_field_diag.py builds and runs it with hipcc,
// host only, once plain and once with the address and undefined sanitizers).
#include "field_diag.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

static int failures = 0;
#define EXPECT(c, ...)          \
  do {                          \
    if (!(c)) {                 \
      ++failures;               \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");        \
    }                           \
  } while (0)

struct Ref {
  long double ess, d;  // d = 1 - sum phi at the selected order
  int order;
  double gap;
};

static Ref ref_ess(const std::vector<long double>& acf, long long S, int P) {
  const long double n = (long double)S;
  Ref r{n, 1.0L, 0, INFINITY};
  if (P < 1 || acf[0] == 0) return r;
  std::vector<long double> phi, aics;
  long double v = acf[0], best_aic = n * std::log(v), best_v = v, best_sum = 0;
  aics.push_back(best_aic);
  for (int k = 1; k <= P; ++k) {
    long double s = 0;
    for (int j = 0; j + 1 < k; ++j) s += phi[j] * acf[k - 1 - j];
    const long double kk = (acf[k] - s) / v;
    std::vector<long double> nw(k);
    for (int j = 0; j + 1 < k; ++j) nw[j] = phi[j] - kk * phi[k - 2 - j];
    nw[k - 1] = kk;
    phi = nw;
    v = v * (1 - kk * kk);
    if (v <= 0) break;
    const long double aic = n * std::log(v) + 2 * k;
    aics.push_back(aic);
    if (aic < best_aic) {
      best_aic = aic;
      best_v = v;
      best_sum = 0;
      for (long double p : phi) best_sum += p;
      r.order = k;
    }
  }
  long double second = INFINITY;
  for (size_t i = 0; i < aics.size(); ++i)
    if ((int)i != r.order && aics[i] < second) second = aics[i];
  r.gap = (double)(second - best_aic);
  r.d = 1 - best_sum;
  const long double spec0 = best_v / (r.d * r.d);
  r.ess = spec0 > 0 ? n * acf[0] / spec0 : n;
  return r;
}

static double run_header(const std::vector<double>& acf, long long S, int P, int* order) {
  std::vector<double> phi((size_t)(P > 0 ? P : 1), 0.0);
  return nngp::field_diag_ess(acf.data(), S, P, phi.data(), order);
}

int main() {
  const double eps = std::ldexp(1.0, -52);
  // the largest order, as numpy's min(S - 1, int(10 log10 S))
  const long long Ss[] = {2, 3, 4, 5, 10, 37, 64, 100, 300, 1000, 9999};
  const int Ps[] = {0, 0, 3, 4, 9, 15, 18, 20, 24, 30, 39};
  for (int i = 0; i < 11; ++i)
    EXPECT(nngp::field_diag_max_order(Ss[i]) == Ps[i], "max_order(%lld) = %d", Ss[i], nngp::field_diag_max_order(Ss[i]));

  std::mt19937_64 gen(12345);
  std::normal_distribution<double> N01;
  double worst = 0.0;
  for (long long S : {4LL, 5LL, 37LL, 300LL, 1000LL})
    for (double rho : {0.0, 0.5, 0.9, 0.99})
      for (int rep = 0; rep < 25; ++rep) {
        std::vector<double> x((size_t)S);
        x[0] = N01(gen) / std::sqrt(1 - rho * rho);
        for (long long t = 1; t < S; ++t) x[t] = rho * x[t - 1] + N01(gen);
        for (double& v : x) v += 3.0;
        const int P = nngp::field_diag_max_order(S);
        double sum = 0;
        long double suml = 0;
        for (double v : x) sum += v, suml += v;
        const double mu = sum / (double)S;
        const long double mul = suml / (long double)S;
        std::vector<double> acf((size_t)P + 1);
        std::vector<long double> acfl((size_t)P + 1);
        for (int l = 0; l <= P; ++l) {
          double a = 0;
          long double al = 0;
          for (long long t = 0; t + l < S; ++t) {
            a += (x[t] - mu) * (x[t + l] - mu);
            al += ((long double)x[t] - mul) * ((long double)x[t + l] - mul);
          }
          acf[l] = a / (double)S;
          acfl[l] = al / (long double)S;
        }
        const Ref r = ref_ess(acfl, S, P);
        int order = -1;
        const double got = run_header(acf, S, P, &order);
        EXPECT(r.gap >= 1e-6, "S=%lld rho=%g rep %d: reference AIC gap %g below 1e-6", S, rho, rep, r.gap);
        EXPECT(order == r.order, "S=%lld rho=%g rep %d: order %d want %d", S, rho, rep, order, r.order);
        const long double d2 = r.d * r.d < 1 ? r.d * r.d : 1.0L;
        const double tol = 8.0 * (double)(S + P) * eps / (double)d2;
        const double err = (double)(std::fabs((long double)got - r.ess) / r.ess);
        if (err / tol > worst) worst = err / tol;
        EXPECT(err <= tol, "S=%lld rho=%g rep %d: ess %.17g want %.17Lg (rel %g > %g)", S, rho, rep, got, r.ess, err, tol);
      }

  int order = -1;
  // v = 0 at order 1: the recursion is left there, order 0, spec0 = acf[0], ess = S
  EXPECT(run_header({1.0, 1.0, 1.0}, 300, 2, &order) == 300.0 && order == 0, "acf {1,1,1}: order %d", order);
  // a constant column
  EXPECT(run_header({0.0, 0.0, 0.0}, 300, 2, &order) == 300.0 && order == 0, "acf[0] = 0: order %d", order);
  // white noise: no order pays its 2 l, ess = S acf[0] / acf[0]
  EXPECT(run_header({2.0, 0.02, -0.02, 0.01}, 300, 3, &order) == 300.0 && order == 0, "white noise: order %d", order);
  // fewer than four rows: no fit
  EXPECT(run_header({1.0}, 3, 0, &order) == 3.0 && order == 0, "S = 3: order %d", order);
  // an AR(1) acf rho^l: order 1, phi = rho, v = 1 - rho^2, ess = S (1 - rho) / (1 + rho)
  {
    const double got = run_header({1.0, 0.5, 0.25, 0.125}, 300, 3, &order);
    EXPECT(order == 1 && std::fabs(got - 100.0) <= 100.0 * 8 * eps, "AR(1) acf: ess %.17g order %d", got, order);
  }

  // the combination: two chains, S = 4
  {
    const double mean[2] = {1.0, 3.0}, var[2] = {2.0, 4.0}, ess[2] = {5.0, 3.0};
    double out[5];
    nngp::field_diag_combine(mean, var, ess, 2, 4, false, out);
    // W = 3, Bv = 2, R = 1.5 * 0.75 * (2 / 3) + 1.25 = 2
    EXPECT(std::fabs(out[0] - 2.0) <= 4 * eps && out[1] == 8.0 && out[2] == 3.0 && out[3] == 3.0 && out[4] == 2.0,
           "combine: %g %g %g %g %g", out[0], out[1], out[2], out[3], out[4]);
    nngp::field_diag_combine(mean, var, ess, 1, 4, false, out);
    EXPECT(std::isnan(out[0]) && std::isnan(out[4]) && out[1] == 5.0 && out[3] == 2.0, "one chain");
    const double zero[2] = {0.0, 0.0}, same[2] = {0.5, 0.5};
    nngp::field_diag_combine(same, zero, ess, 2, 4, false, out);
    EXPECT(std::isnan(out[0]) && out[3] == 0.0 && out[4] == 0.0, "constant: R %g", out[0]);
    nngp::field_diag_combine(mean, zero, ess, 2, 4, false, out);
    EXPECT(std::isinf(out[0]) && out[3] == 0.0, "constant per chain: R %g", out[0]);
    nngp::field_diag_combine(mean, var, ess, 2, 4, true, out);
    for (int q = 0; q < 5; ++q) EXPECT(std::isnan(out[q]), "NaN column: out[%d] = %g", q, out[q]);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok (ess: largest fraction of the bound used %.3g)\n", worst);
  return 0;
}
