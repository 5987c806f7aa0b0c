// Host interface of field_diag.hip (per-location R-hat and effective sample
// size of the field samples; nngp_field_diag of include/nngp.h).
#pragma once
#include <string>

namespace nngp {

// Automatic chunk width: both staging buffers together stay at or below this.
constexpr size_t kFieldDiagStageBudget = size_t(1) << 30;

struct FieldDiagStats {
  double copy_ms = 0.0;    // host-to-device staging copies (HIP events, summed over the chunks)
  double kernel_ms = 0.0;  // diagnostics kernels (HIP events, summed over the chunks)
  long long staged_bytes = 0;
  int chunk_cols = 0;
  int n_chunks = 0;
};

// The staging loop and kernel launches behind nngp_field_diag; returns an
// nngp_status and, on failure, the message in err.
int field_diag_run(int device, const double* const* blocks, int n_chains, long long rows, long long n,
                   const double* row_offset, int chunk_cols, double* out, int* order, FieldDiagStats* stats,
                   std::string& err);

}  // namespace nngp
