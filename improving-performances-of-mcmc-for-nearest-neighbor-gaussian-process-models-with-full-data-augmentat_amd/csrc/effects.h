// Host interface of effects.hip (fixed-effect / response samples generated on
// the device and summarised there; nngp_effects_summary of include/nngp.h).
#pragma once
#include <cstdint>
#include <string>

namespace nngp {

constexpr int kEffectsQMax = 1024;

struct EffectsStats {
  double copy_ms = 0.0;      // host-to-device copies of the addend (HIP events, summed over the chunks)
  double generate_ms = 0.0;  // generator kernels (HIP events, summed over the chunks)
  double kernel_ms = 0.0;    // summary kernels (HIP events, summed over the chunks)
  long long staged_bytes = 0;  // addend bytes staged; 0 without an addend
  int chunk_cols = 0;
  int n_chunks = 0;
};

struct EffectsArgs {
  int device;
  const double* coef;  // n_samples x q column-major
  long long n_samples;
  int q;
  const double* X;  // n x q column-major
  long long n;
  const double* const* addend_blocks;  // row-major blocks, pitch n; n_blocks == 0: none
  const long long* block_rows;
  int n_blocks;
  const double* noise_sd;  // n_samples, or nullptr: no noise
  uint64_t seed;
  const uint64_t* counter;  // n_samples (with noise)
  int chunk_cols;
  const double* probs;
  int n_probs;
  const double* thresholds;
  int n_thresholds;
  double* out;          // n x (2 + n_probs + n_thresholds) column-major
  double* samples_out;  // n_samples x n row-major, or nullptr
};

// Checks, uploads, the generator + summary launches per chunk; returns an
// nngp_status and, on failure, the message in err.  Every argument check is
// made before the first HIP call.
int effects_run(const EffectsArgs& a, EffectsStats* stats, std::string& err);

}  // namespace nngp
