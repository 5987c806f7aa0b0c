// Per-location convergence diagnostics of the field samples: the effective
// sample size of one chain's column (the AR(p)-spectral estimate of
// diagnose._ess_1d, Scripts/mcmc_nngp_diagnose.R:107-118) and the
// Gelman-Rubin combination of the chains (Individual_PSRF,
// Scripts/mcmc_nngp_diagnose.R:1-24, with n := S saved rows).
// __host__ __device__, no HIP types: field_diag.hip runs it with one lane per
// column, tests/cpp/field_diag_check.cpp compiles the same text for the CPU.
#pragma once
#include <cmath>
#include <limits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NNGP_FD_HD __host__ __device__ __forceinline__
#else
#define NNGP_FD_HD inline
#endif

namespace nngp {

constexpr int kFieldDiagCols = 5;       // R_hat, ess, ess_min, W, Bv
constexpr int kFieldDiagMaxOrder = 39;  // int(10 log10 S) for S <= 9999
constexpr int kFieldDiagMaxRows = 9999;
constexpr int kFieldDiagMaxChains = 16;

// The largest AR order tried for S rows: min(S - 1, int(10 log10 S)), 0 below
// four rows (no fit).  The logarithm is taken as numpy takes it, in double;
// 10 log10 S is no integer near any S <= 9999 but the exact powers of ten.
NNGP_FD_HD int field_diag_max_order(long long S) {
  if (S < 4) return 0;
  const int p = (int)(10.0 * log10((double)S));
  return (long long)p < S - 1 ? p : (int)(S - 1);
}

// ess and the selected order from acf[0..P] (acf[l] = sum_t xc[t] xc[t+l] / S).
// Levinson-Durbin up to order P with AIC = S log v + 2 l, the first minimum
// (strict <, l upward from 0), the recursion left at the first v <= 0;
// spec0 = v / (1 - sum phi)^2 at the selected order, ess = S acf[0] / spec0 if
// spec0 > 0, else S.  acf[0] == 0 (a constant column) gives S and order 0.
// phi: storage of P values addressed phi[j] (a plain array on the host, a
// strided view of LDS on the device); only sum phi and v of the best order are
// kept, the coefficients themselves are updated in place.
template <class Phi>
NNGP_FD_HD double field_diag_ess(const double* acf, long long S, int P, Phi phi, int* order) {
  const double n = (double)S;
  *order = 0;
  if (P < 1 || acf[0] == 0.0) return n;
  double v = acf[0];
  double best_aic = n * log(v), best_v = v, best_sum = 0.0;
  for (int k = 1; k <= P; ++k) {
    double s = 0.0;
    for (int j = 0; j + 1 < k; ++j) s += phi[j] * acf[k - 1 - j];
    const double kk = (acf[k] - s) / v;
    // phi <- phi - kk rev(phi), in place by pairs from both ends
    for (int lo = 0, hi = k - 2; lo <= hi; ++lo, --hi) {
      const double a = phi[lo], b = phi[hi];
      phi[lo] = a - kk * b;
      if (hi != lo) phi[hi] = b - kk * a;
    }
    phi[k - 1] = kk;
    v = v * (1.0 - kk * kk);
    if (v <= 0.0) break;
    const double aic = n * log(v) + 2.0 * (double)k;
    if (aic < best_aic) {
      double sum = 0.0;
      for (int j = 0; j < k; ++j) sum += phi[j];
      best_aic = aic;
      best_v = v;
      best_sum = sum;
      *order = k;
    }
  }
  const double d = 1.0 - best_sum;
  const double spec0 = best_v / (d * d);
  return spec0 > 0.0 ? n * acf[0] / spec0 : n;
}

// The five numbers of one location from its m chains' means, variances
// (divisor S - 1) and ess values: W = mean of the variances, Bv = variance of
// the means with divisor m - 1 (0 / 0 = NaN for one chain, as np.cov gives),
// R_hat = ((m+1)/m) ((S-1)/S) (Bv/W) + (S+1)/S in plain IEEE division,
// ess = sum, ess_min = min.  nan: some chain's column held a NaN.
NNGP_FD_HD void field_diag_combine(const double* mean, const double* var, const double* ess, int m, long long S,
                                   bool nan, double* out) {
#pragma clang fp contract(off)
  const double dm = (double)m, n = (double)S;
  double sv = 0.0, sm = 0.0, se = 0.0, emin = ess[0];
  for (int k = 0; k < m; ++k) {
    sv += var[k];
    sm += mean[k];
    se += ess[k];
    emin = ess[k] < emin ? ess[k] : emin;
  }
  const double W = sv / dm, M = sm / dm;
  double sb = 0.0;
  for (int k = 0; k < m; ++k) {
    const double d = mean[k] - M;
    sb += d * d;
  }
  const double Bv = sb / (double)(m - 1);
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  out[0] = nan ? qnan : ((dm + 1.0) / dm) * ((n - 1.0) / n) * (Bv / W) + (n + 1.0) / n;
  out[1] = nan ? qnan : se;
  out[2] = nan ? qnan : emin;
  out[3] = nan ? qnan : W;
  out[4] = nan ? qnan : Bv;
}

}  // namespace nngp
