// Host interface of predict.hip (batched posterior prediction at new
// locations; nngp_predict_field of include/nngp.h).
#pragma once
#include <cstdint>
#include <string>

namespace nngp {

// Automatic sample batch: the device buffers of one batch (the factor rows of
// the batch's distinct factors, the values, the staging buffer and the output
// block) stay at or below this, but a batch never has fewer than 64 samples
// (one wavefront of lanes) unless the call has fewer.
constexpr size_t kPredictBudget = size_t(1) << 30;
constexpr int kPredictBMax = 32;  // launch_factor's limit on b

struct PredictStats {
  double plan_ms = 0.0;    // host: support set, compact table, level schedule
  double factor_ms = 0.0;  // HIP events: scaled coordinates + factor rows, summed over the batches
  double solve_ms = 0.0;   // HIP events: staging copies, transposes, level solve, output copy
  long long staged_bytes = 0;  // host-to-device bytes of support values and normals
  int sample_batch = 0;
  int n_batches = 0;
};

// one distinct covariance parameter set of the call (checked by the caller)
struct PredictFactor {
  double cp[8];
  int ncp;
  int family;  // launch_factor's
  double var, nugget, nu;
};

struct PredictArgs {
  int device;
  const double* locs;  // N x d column-major
  int n, n_pred, d;
  const int* NNarray;  // N x b column-major, 1-based
  int b;
  int covfun;
  const PredictFactor* factors;
  int n_factors;
  int n_samples;
  const int* factor_of;
  const double* fields;
  long long field_pitch;
  const long long* field_row;
  const double* beta0;
  const double* log_scale;
  const double* z;  // n_samples x n_pred row-major, or nullptr: Philox
  uint64_t seed;
  const uint64_t* counter;
  int sample_batch;
  double* out;
  int* fail_row;
};

// Plan, factor rows and the batched level solve behind nngp_predict_field;
// returns an nngp_status and, on failure, the message in err.  No HIP call is
// made before the plan is built (a bad table is NNGP_ERR_ARG on any host).
int predict_run(const PredictArgs& a, PredictStats* stats, std::string& err);

}  // namespace nngp
