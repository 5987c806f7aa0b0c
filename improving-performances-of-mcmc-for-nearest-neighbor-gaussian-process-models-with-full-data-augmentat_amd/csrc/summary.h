// Host interface of summary.hip (posterior summaries per column; nngp_summary
// and nngp_summary_probs of include/nngp.h).
#pragma once
#include <string>

namespace nngp {

// Automatic chunk width: both staging buffers together stay at or below this.
constexpr size_t kSummaryStageBudget = size_t(1) << 30;

struct SummaryStats {
  double copy_ms = 0.0;    // host-to-device staging copies (HIP events, summed over the chunks)
  double kernel_ms = 0.0;  // summary kernels (HIP events, summed over the chunks)
  long long staged_bytes = 0;
  int chunk_cols = 0;
  int n_chunks = 0;
};

// The staging loop and kernel launches behind nngp_summary; returns an
// nngp_status and, on failure, the message in err.
int summary_run(int device, const double* const* blocks, const long long* block_rows, int n_blocks, long long n,
                const double* row_offset, int chunk_cols, double* out, SummaryStats* stats, std::string& err);

// The same staging loop behind nngp_summary_probs: mean, the n_probs type-7
// quantiles, sd and the n_thresholds exceedance fractions; out is
// n x (2 + n_probs + n_thresholds).  The request is checked before any HIP call.
int summary_run_probs(int device, const double* const* blocks, const long long* block_rows, int n_blocks, long long n,
                      const double* row_offset, int chunk_cols, const double* probs, int n_probs,
                      const double* thresholds, int n_thresholds, double* out, SummaryStats* stats, std::string& err);

}  // namespace nngp
