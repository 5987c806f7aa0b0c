// Per-column posterior summary (get_summary, Scripts/mcmc_nngp_estimate.R:1-6):
// mean, the type-7 quantiles 0.025 / 0.5 / 0.975 and sd of S values that are
// only ever streamed -- nothing here holds a column, so S is bounded by the
// 32-bit counters (S < 2^31), not by registers or LDS.  summary_column_probs
// is the same with the quantiles chosen by the caller and exceedance
// fractions.  __host__ __device__: summary.hip runs it with one lane per
// column, tests/cpp/summary_select_check.cpp and summary_probs_check.cpp
// compile the same text for the CPU.
//
// A column is a functor `double load(long long s)`, s = 0..S-1; every pass
// calls it for all s in increasing order.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NNGP_HD __host__ __device__ __forceinline__
#else
#define NNGP_HD inline
#endif

namespace nngp {

constexpr int kSummaryQ = 3;  // wanted quantiles
constexpr int kSummaryCols = 5;  // mean, q0.025, median, q0.975, sd

// Order-preserving key of a double: k(x) < k(y) <=> x < y for non-NaN x, y,
// refined by -0.0 < +0.0.  Negative values have all bits flipped, the others
// the sign bit.
NNGP_HD uint64_t summary_key(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  return (u >> 63) ? ~u : (u ^ 0x8000000000000000ull);
}
NNGP_HD double summary_unkey(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k);
}

// numpy's 'linear' (R type 7) position of quantile q among S sorted values:
// h = q (S - 1), j = floor(h), g = h - j.
NNGP_HD void summary_rank(double q, long long S, long long* j, double* g) {
  const double h = q * (double)(S - 1);
  const double f = floor(h);
  *j = (long long)f;
  *g = h - f;
}

// numpy's _lerp of a = x_(j), b = x_(j+1); g == 0 returns a itself.  Not
// contracted: the products round as numpy's do.
NNGP_HD double summary_lerp(double a, double b, double g) {
#pragma clang fp contract(off)
  if (g == 0.0) return a;
  const double d = b - a;
  return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

// Radix select of kSummaryQ ranks at once, BITS bits of the key per pass
// (64 / BITS passes over the column, most significant digit first).  Per rank
// only the key prefix found so far, the rank left inside it and 2^BITS
// counters live in registers; the counter loops are fully unrolled
// compare-and-adds, so nothing is indexed dynamically.  lo[r] = x_(j[r]);
// hi[r] = x_(j[r]+1) (= lo[r] for the last rank): lo[r] again while the run
// of values equal to it reaches past rank j[r], else the minimum of the
// values above it, found by one more pass (skipped unless want_hi).
template <int BITS, class Load>
NNGP_HD void summary_select(Load load, long long S, const long long* j, bool want_hi, double* lo, double* hi) {
  static_assert(BITS == 1 || BITS == 2 || BITS == 4, "digit width");
  constexpr int NB = 1 << BITS;
  uint64_t prefix[kSummaryQ];
  uint32_t left[kSummaryQ], run[kSummaryQ];
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r) {
    prefix[r] = 0;
    left[r] = (uint32_t)j[r];
    run[r] = 0;
  }
  for (int shift = 64 - BITS; shift >= 0; shift -= BITS) {
    // bits above this pass's digit (none in the first pass)
    const uint64_t above = shift + BITS == 64 ? 0ull : ~0ull << (shift + BITS);
    uint32_t cnt[kSummaryQ][NB];
#pragma unroll
    for (int r = 0; r < kSummaryQ; ++r)
#pragma unroll
      for (int d = 0; d < NB; ++d) cnt[r][d] = 0;
#pragma unroll 4
    for (long long s = 0; s < S; ++s) {
      const uint64_t k = summary_key(load(s));
      const uint32_t digit = (uint32_t)(k >> shift) & (NB - 1);
#pragma unroll
      for (int r = 0; r < kSummaryQ; ++r) {
        const uint32_t dr = ((k ^ prefix[r]) & above) == 0 ? digit : (uint32_t)NB;
#pragma unroll
        for (int d = 0; d < NB; ++d) cnt[r][d] += dr == (uint32_t)d;
      }
    }
#pragma unroll
    for (int r = 0; r < kSummaryQ; ++r) {
      uint32_t k = left[r], dsel = 0, csel = 0;
      bool found = false;
#pragma unroll
      for (int d = 0; d < NB; ++d) {
        const uint32_t c = cnt[r][d];
        const bool here = !found && k < c;
        dsel = here ? (uint32_t)d : dsel;
        csel = here ? c : csel;
        found = found || here;
        k = found ? k : k - c;
      }
      prefix[r] |= (uint64_t)dsel << shift;
      left[r] = k;
      run[r] = csel;  // after the last pass: the values equal to x_(j[r])
    }
  }
  bool again[kSummaryQ];
  bool any = false;
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r) {
    lo[r] = summary_unkey(prefix[r]);
    hi[r] = lo[r];
    again[r] = left[r] + 1 >= run[r];  // x_(j) is the last of its run
    any = any || again[r];
  }
  if (!want_hi || !any) return;
  uint64_t up[kSummaryQ];
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r) up[r] = ~0ull;
#pragma unroll 4
  for (long long s = 0; s < S; ++s) {
    const uint64_t k = summary_key(load(s));
#pragma unroll
    for (int r = 0; r < kSummaryQ; ++r) up[r] = (k > prefix[r] && k < up[r]) ? k : up[r];
  }
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r)
    if (again[r] && j[r] + 1 < S) hi[r] = summary_unkey(up[r]);
}

// The five numbers of one column: out[0] = mean (sum in row order / S),
// out[1..3] = the quantiles, out[4] = sd (two-pass, divisor S - 1; NaN for
// S = 1).  A column that holds a NaN gives five NaNs.
template <int BITS, class Load>
NNGP_HD void summary_column(Load load, long long S, double* out) {
#pragma clang fp contract(off)
  const double q[kSummaryQ] = {0.025, 0.5, 0.975};
  double sum = 0.0;
  bool nan = false;
#pragma unroll 4
  for (long long s = 0; s < S; ++s) {
    const double x = load(s);
    nan = nan || x != x;
    sum += x;
  }
  const double mean = sum / (double)S;
  double ss = 0.0;
#pragma unroll 4
  for (long long s = 0; s < S; ++s) {
    const double d = load(s) - mean;
    ss += d * d;
  }
  long long j[kSummaryQ];
  double g[kSummaryQ], lo[kSummaryQ], hi[kSummaryQ];
  bool want_hi = false;
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r) {
    summary_rank(q[r], S, &j[r], &g[r]);
    want_hi = want_hi || g[r] != 0.0;
  }
  summary_select<BITS>(load, S, j, want_hi, lo, hi);
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  out[0] = nan ? qnan : mean;
#pragma unroll
  for (int r = 0; r < kSummaryQ; ++r) out[1 + r] = nan ? qnan : summary_lerp(lo[r], hi[r], g[r]);
  out[4] = (nan || S < 2) ? qnan : sqrt(ss / (double)(S - 1));
}

constexpr int kSummaryProbsMax = 16;  // quantiles per request
constexpr int kSummaryThrMax = 8;     // exceedance thresholds per request

// The general column summary: out[0] = mean, out[(1 + i) stride] = the type-7
// quantile probs[i] (i < n_probs <= kSummaryProbsMax, in [0, 1], any order,
// repeats allowed; 0 and 1 are the exact minimum and maximum),
// out[(1 + n_probs) stride] = sd, out[(2 + n_probs + k) stride] =
// count(x > thr[k]) / S (k < n_thr <= kSummaryThrMax; strict compare, integer
// count, one division).  Mean, sd, ranks and interpolation are
// summary_column's, so probs = (0.025, 0.5, 0.975) without thresholds gives
// its five numbers bit for bit.  A column that holds a NaN gives NaNs only.
//
// The ranks go through summary_select in rounds of kSummaryQ (a short last
// round repeats its first rank): the counters of a round are the existing
// 3 x 2^BITS registers, and the select is exact, so a quantile's bits depend
// on its column and its own q only -- not on the round it fell into, the
// other probabilities or the thresholds.  The exceedance counts ride on the
// mean pass: kSummaryThrMax statically indexed counters, the unused ones
// compared against +inf (never exceeded).  Results are stored as they are
// found; nothing here is indexed by a run-time value except probs and thr,
// which the kernel holds in scalar memory.
template <int BITS, class Load>
NNGP_HD void summary_column_probs(Load load, long long S, const double* probs, int n_probs, const double* thr,
                                  int n_thr, double* out, long long stride) {
#pragma clang fp contract(off)
  double sum = 0.0;
  bool nan = false;
  uint32_t above[kSummaryThrMax];
#pragma unroll
  for (int k = 0; k < kSummaryThrMax; ++k) above[k] = 0;
  if (n_thr > 0) {
    double t[kSummaryThrMax];
#pragma unroll
    for (int k = 0; k < kSummaryThrMax; ++k) t[k] = k < n_thr ? thr[k] : std::numeric_limits<double>::infinity();
#pragma unroll 4
    for (long long s = 0; s < S; ++s) {
      const double x = load(s);
      nan = nan || x != x;
      sum += x;
#pragma unroll
      for (int k = 0; k < kSummaryThrMax; ++k) above[k] += x > t[k];
    }
  } else {
#pragma unroll 4
    for (long long s = 0; s < S; ++s) {
      const double x = load(s);
      nan = nan || x != x;
      sum += x;
    }
  }
  const double mean = sum / (double)S;
  double ss = 0.0;
#pragma unroll 4
  for (long long s = 0; s < S; ++s) {
    const double d = load(s) - mean;
    ss += d * d;
  }
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  out[0] = nan ? qnan : mean;
  out[(1 + n_probs) * stride] = (nan || S < 2) ? qnan : sqrt(ss / (double)(S - 1));
#pragma unroll
  for (int k = 0; k < kSummaryThrMax; ++k)
    if (k < n_thr) out[(2 + n_probs + k) * stride] = nan ? qnan : (double)above[k] / (double)S;
  for (int q0 = 0; q0 < n_probs; q0 += kSummaryQ) {
    long long j[kSummaryQ];
    double g[kSummaryQ], lo[kSummaryQ], hi[kSummaryQ];
    bool want_hi = false;
#pragma unroll
    for (int r = 0; r < kSummaryQ; ++r) {
      summary_rank(probs[q0 + r < n_probs ? q0 + r : q0], S, &j[r], &g[r]);
      want_hi = want_hi || g[r] != 0.0;
    }
    summary_select<BITS>(load, S, j, want_hi, lo, hi);
#pragma unroll
    for (int r = 0; r < kSummaryQ; ++r)
      if (q0 + r < n_probs) out[(1 + q0 + r) * stride] = nan ? qnan : summary_lerp(lo[r], hi[r], g[r]);
  }
}

}  // namespace nngp
