// What another translation unit needs to run summary.hip's kernels on a chunk
// it has staged or generated itself (effects.hip): the checked request, the
// automatic chunk width, the digit width and the launch.  The kernels and the
// select code stay in summary.hip / summary_select.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "summary_select.h"

namespace nngp {

// The request of nngp_summary_probs, a kernel argument: the same for every
// lane, so the probabilities and thresholds are scalar loads.
struct SummaryRequest {
  double probs[kSummaryProbsMax];
  double thr[kSummaryThrMax];
  int n_probs, n_thr;
};

// nngp_summary_probs's checks of probs and thresholds (no HIP call); fills
// req, or returns NNGP_ERR_ARG with the message in err.
int summary_make_request(const double* probs, int n_probs, const double* thresholds, int n_thresholds,
                         SummaryRequest* req, std::string& err);

// Chunk width W (columns per launch) for S rows x n columns.  chunk_cols > 0
// is taken as given; 0 is automatic: the two staging buffers stay within
// kSummaryStageBudget (but never below one wavefront of columns); a matrix
// that would fit one chunk is still cut into about four, so that copies and
// kernels overlap, unless that leaves fewer than 64 Ki columns (4 waves on
// each of 256 CUs) per launch.  Never more than n.
long long summary_chunk_width(long long S, long long n, int chunk_cols);

// Radix digit width (NNGP_SUMMARY_BITS, default 4): 2 or 4, else
// NNGP_ERR_ARG with the message in err.
int summary_digit_bits(int* bits, std::string& err);

// One summary launch on a chunk of S rows x w columns, row-major with pitch
// `pitch`; off (S row offsets, device) or nullptr; req == nullptr: the five
// fixed columns of nngp_summary.  Writes rows c0 .. c0 + w - 1 of out (n x
// columns, column-major, device).
hipError_t summary_launch(int bits, hipStream_t st, const double* x, const double* off, long long S, int w,
                          long long pitch, const SummaryRequest* req, double* out, long long n, long long c0);

}  // namespace nngp
