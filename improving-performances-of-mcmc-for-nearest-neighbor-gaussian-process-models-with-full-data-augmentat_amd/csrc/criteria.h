// Host interface of criteria.hip (the pointwise Gaussian log-likelihood of the
// saved samples reduced per observation on the device;
// nngp_pointwise_loglik of include/nngp.h).
#pragma once
#include <string>

namespace nngp {

constexpr int kCriteriaQMax = 1024;
constexpr int kCriteriaCols = 6;  // fit_mean, ll_mean, ll_var, lppd, log_cpo, pit

struct CriteriaStats {
  double copy_ms = 0.0;    // host-to-device copies of the field chunks (HIP events, summed over the chunks)
  double kernel_ms = 0.0;  // reduction kernels (HIP events, summed over the chunks)
  long long staged_bytes = 0;
  int chunk_cols = 0;
  int n_chunks = 0;
};

struct CriteriaArgs {
  int device;
  const double* y;  // n_obs
  long long n_obs;
  const int* obs_loc;  // n_obs, 1-based, non-decreasing
  const double* coef;  // n_samples x q column-major, or nullptr with q == 0
  long long n_samples;
  int q;
  const double* X;                     // n_obs x q column-major, or nullptr with q == 0
  const double* const* field_blocks;   // row-major blocks, pitch n
  const long long* block_rows;
  int n_blocks;
  long long n;
  const double* log_noise_var;  // n_samples
  int chunk_cols;
  double* out;  // n_obs x kCriteriaCols column-major
};

// Checks, uploads, the staging loop and one kernel launch per chunk; returns an
// nngp_status and, on failure, the message in err.  Every argument check is
// made before the first HIP call.
int criteria_run(const CriteriaArgs& a, CriteriaStats* stats, std::string& err);

}  // namespace nngp
