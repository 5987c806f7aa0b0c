// get_summary on the device (Scripts/mcmc_nngp_estimate.R:1-6): mean, three
// type-7 quantiles and sd of every column of a samples x locations matrix
// (nngp_summary), or mean, the quantiles asked for, sd and the exceedance
// fractions P(x > t) (nngp_summary_probs).
//
// One lane owns one column of a staged chunk (S rows x w columns, row-major,
// pitch W): in every pass a wavefront reads 64 neighbouring columns of a row,
// 512 contiguous bytes, and the row's offset is one scalar load.  The
// selection is the radix select of summary_select.h; a lane's five numbers
// depend on its own column only (no cross-lane operation, no LDS), so they do
// not change with the chunk width, the column's position or its neighbours.
#include "summary.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/nngp.h"
#include "summary_launch.h"
#include "summary_select.h"

namespace nngp {
namespace {

constexpr int kSummaryBlock = 256;

struct ColumnLoad {
  const double* x;  // the lane's column: x[s * pitch]
  const double* off;
  long long pitch;
  __device__ __forceinline__ double operator()(long long s) const { return x[s * pitch] - off[s]; }
};
struct ColumnLoadPlain {
  const double* x;
  long long pitch;
  __device__ __forceinline__ double operator()(long long s) const { return x[s * pitch]; }
};

// out: n x 5 column-major; this launch writes columns c0 .. c0 + w - 1
template <int BITS, bool OFF>
__global__ __launch_bounds__(kSummaryBlock) void summary_kernel(const double* __restrict__ x, const double* __restrict__ off,
                                                                long long S, int w, long long pitch,
                                                                double* __restrict__ out, long long n, long long c0) {
  const int c = blockIdx.x * kSummaryBlock + threadIdx.x;
  if (c >= w) return;
  double r[kSummaryCols];
  if constexpr (OFF)
    summary_column<BITS>(ColumnLoad{x + c, off, pitch}, S, r);
  else
    summary_column<BITS>(ColumnLoadPlain{x + c, pitch}, S, r);
#pragma unroll
  for (int q = 0; q < kSummaryCols; ++q) out[q * n + c0 + c] = r[q];
}

// out: n x (2 + n_probs + n_thr) column-major; columns c0 .. c0 + w - 1.
// With row offsets the kernel is held to 4 waves per SIMD (110 VGPRs instead
// of 132 at 4-bit digits, no scratch; measured ahead); without
// them that bound would spill, so it is left to the compiler (144 VGPRs).
template <int BITS, bool OFF>
__global__ __launch_bounds__(kSummaryBlock, OFF ? 4 : 1) void summary_probs_kernel(const double* __restrict__ x,
                                                                      const double* __restrict__ off, long long S, int w,
                                                                      long long pitch, const SummaryRequest req,
                                                                      double* __restrict__ out, long long n, long long c0) {
  const int c = blockIdx.x * kSummaryBlock + threadIdx.x;
  if (c >= w) return;
  if constexpr (OFF)
    summary_column_probs<BITS>(ColumnLoad{x + c, off, pitch}, S, req.probs, req.n_probs, req.thr, req.n_thr,
                               out + c0 + c, n);
  else
    summary_column_probs<BITS>(ColumnLoadPlain{x + c, pitch}, S, req.probs, req.n_probs, req.thr, req.n_thr,
                               out + c0 + c, n);
}

// req == nullptr: the five fixed columns of nngp_summary
template <int BITS>
hipError_t launch_summary(hipStream_t st, const double* x, const double* off, long long S, int w, long long pitch,
                          const SummaryRequest* req, double* out, long long n, long long c0) {
  const dim3 grid((w + kSummaryBlock - 1) / kSummaryBlock), block(kSummaryBlock);
  if (req && off)
    hipLaunchKernelGGL((summary_probs_kernel<BITS, true>), grid, block, 0, st, x, off, S, w, pitch, *req, out, n, c0);
  else if (req)
    hipLaunchKernelGGL((summary_probs_kernel<BITS, false>), grid, block, 0, st, x, off, S, w, pitch, *req, out, n, c0);
  else if (off)
    hipLaunchKernelGGL((summary_kernel<BITS, true>), grid, block, 0, st, x, off, S, w, pitch, out, n, c0);
  else
    hipLaunchKernelGGL((summary_kernel<BITS, false>), grid, block, 0, st, x, off, S, w, pitch, out, n, c0);
  return hipGetLastError();
}

// every device object of a call; freed on every exit path
struct SummaryDev {
  double* buf[2] = {nullptr, nullptr};
  double* off = nullptr;
  double* out = nullptr;
  hipStream_t copy_st = nullptr, run_st = nullptr;
  hipEvent_t copy0[2] = {}, copy1[2] = {}, run0[2] = {}, run1[2] = {};
  ~SummaryDev() {
    for (int b = 0; b < 2; ++b) {
      if (buf[b]) (void)hipFree(buf[b]);
      for (hipEvent_t e : {copy0[b], copy1[b], run0[b], run1[b]})
        if (e) (void)hipEventDestroy(e);
    }
    if (off) (void)hipFree(off);
    if (out) (void)hipFree(out);
    if (copy_st) (void)hipStreamDestroy(copy_st);
    if (run_st) (void)hipStreamDestroy(run_st);
  }
};

// The one staging loop of both entry points; out: n x ncols column-major.
int summary_stage(int device, const double* const* blocks, const long long* block_rows, int n_blocks, long long n,
                  const double* row_offset, int chunk_cols, const SummaryRequest* req, int ncols, double* out,
                  SummaryStats* stats, std::string& err) {
  if (!blocks || !block_rows || !out || n_blocks < 1 || n < 1 || chunk_cols < 0) {
    err = "summary: bad args";
    return NNGP_ERR_ARG;
  }
  long long S = 0;
  for (int k = 0; k < n_blocks; ++k) {
    if (!blocks[k] || block_rows[k] < 0) {
      err = "summary: null block or negative row count";
      return NNGP_ERR_ARG;
    }
    S += block_rows[k];
  }
  if (S < 1 || S > 0x7fffffffLL) {
    err = S < 1 ? "summary: no rows" : "summary: more than 2^31 - 1 rows";
    return NNGP_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    err = "no HIP device";
    return NNGP_ERR_NODEV;
  }
  if (device >= ndev) {
    err = "device ordinal out of range";
    return NNGP_ERR_ARG;
  }
  // the calling thread's current device is put back on every exit path
  // (declared before the device objects, so they are released first)
  struct RestoreDevice {
    int prev = -1;
    ~RestoreDevice() {
      if (prev >= 0) (void)hipSetDevice(prev);
    }
  } restore;
  if (device >= 0 && (hipGetDevice(&restore.prev) != hipSuccess || restore.prev == device)) restore.prev = -1;
  hipError_t e = device < 0 ? hipSuccess : hipSetDevice(device);
  auto hip_fail = [&](const char* what) {
    err = std::string("summary: ") + what + ": " + hipGetErrorString(e);
    return NNGP_ERR_HIP;
  };
  if (e != hipSuccess) return hip_fail("hipSetDevice");

  const long long W = summary_chunk_width(S, n, chunk_cols);
  int bits = 0;
  if (const int rc = summary_digit_bits(&bits, err)) return rc;

  SummaryDev D;
  const size_t chunk_bytes = sizeof(double) * (size_t)S * (size_t)W;
  for (int b = 0; b < 2; ++b)
    if (hipMalloc((void**)&D.buf[b], chunk_bytes) != hipSuccess) {
      (void)hipGetLastError();
      err = "summary: staging buffers do not fit the device (smaller chunk_cols?)";
      return NNGP_ERR_NOMEM;
    }
  if (hipMalloc((void**)&D.out, sizeof(double) * (size_t)ncols * (size_t)n) != hipSuccess ||
      (row_offset && hipMalloc((void**)&D.off, sizeof(double) * (size_t)S) != hipSuccess)) {
    (void)hipGetLastError();
    err = "summary: device allocation failed";
    return NNGP_ERR_NOMEM;
  }
#define SUMMARY_HIP(x)                        \
  do {                                        \
    e = (x);                                  \
    if (e != hipSuccess) return hip_fail(#x); \
  } while (0)
  SUMMARY_HIP(hipStreamCreateWithFlags(&D.copy_st, hipStreamNonBlocking));
  SUMMARY_HIP(hipStreamCreateWithFlags(&D.run_st, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    SUMMARY_HIP(hipEventCreate(&D.copy0[b]));
    SUMMARY_HIP(hipEventCreate(&D.copy1[b]));
    SUMMARY_HIP(hipEventCreate(&D.run0[b]));
    SUMMARY_HIP(hipEventCreate(&D.run1[b]));
  }
  if (row_offset) SUMMARY_HIP(hipMemcpyAsync(D.off, row_offset, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, D.run_st));

  SummaryStats st;
  st.chunk_cols = (int)W;
  // the times of the chunk that used slot b last; called once its kernel is done
  auto collect = [&](int b) -> hipError_t {
    float ms = 0.f;
    hipError_t r = hipEventElapsedTime(&ms, D.copy0[b], D.copy1[b]);
    if (r != hipSuccess) return r;
    st.copy_ms += ms;
    r = hipEventElapsedTime(&ms, D.run0[b], D.run1[b]);
    st.kernel_ms += ms;
    return r;
  };
  long long k = 0;
  for (long long c0 = 0; c0 < n; c0 += W, ++k) {
    const int b = (int)(k & 1);
    const int w = (int)std::min(W, n - c0);
    if (k >= 2) {  // slot b: the kernel of chunk k - 2 has read it
      SUMMARY_HIP(hipEventSynchronize(D.run1[b]));
      SUMMARY_HIP(collect(b));
    }
    SUMMARY_HIP(hipEventRecord(D.copy0[b], D.copy_st));
    long long row = 0;
    for (int q = 0; q < n_blocks; ++q) {
      if (block_rows[q] == 0) continue;
      SUMMARY_HIP(hipMemcpy2DAsync(D.buf[b] + (size_t)row * (size_t)W, sizeof(double) * (size_t)W, blocks[q] + c0,
                                   sizeof(double) * (size_t)n, sizeof(double) * (size_t)w, (size_t)block_rows[q],
                                   hipMemcpyHostToDevice, D.copy_st));
      row += block_rows[q];
    }
    SUMMARY_HIP(hipEventRecord(D.copy1[b], D.copy_st));
    st.staged_bytes += (long long)sizeof(double) * S * w;
    SUMMARY_HIP(hipStreamWaitEvent(D.run_st, D.copy1[b], 0));
    SUMMARY_HIP(hipEventRecord(D.run0[b], D.run_st));
    SUMMARY_HIP(summary_launch(bits, D.run_st, D.buf[b], D.off, S, w, W, req, D.out, n, c0));
    SUMMARY_HIP(hipEventRecord(D.run1[b], D.run_st));
  }
  st.n_chunks = (int)k;
  SUMMARY_HIP(hipMemcpyAsync(out, D.out, sizeof(double) * (size_t)ncols * (size_t)n, hipMemcpyDeviceToHost, D.run_st));
  SUMMARY_HIP(hipStreamSynchronize(D.run_st));
  for (long long q = std::max(0LL, k - 2); q < k; ++q) SUMMARY_HIP(collect((int)(q & 1)));
#undef SUMMARY_HIP
  if (stats) *stats = st;
  return NNGP_OK;
}

}  // namespace

long long summary_chunk_width(long long S, long long n, int chunk_cols) {
  long long W = chunk_cols;
  if (W == 0) {
    W = (long long)(kSummaryStageBudget / 2 / sizeof(double)) / S / kSummaryBlock * kSummaryBlock;
    const long long quarter = (n / 4 + kSummaryBlock - 1) / kSummaryBlock * kSummaryBlock;
    W = std::min(W, std::max(65536LL, quarter));
    W = std::max(W, 64LL);
  }
  return std::min(W, n);
}

int summary_digit_bits(int* bits, std::string& err) {
  const char* s = std::getenv("NNGP_SUMMARY_BITS");
  *bits = s ? std::atoi(s) : 4;  // 4-bit digits: 16 passes; measured ahead of 2 bits x 32
  if (*bits != 2 && *bits != 4) {
    err = "NNGP_SUMMARY_BITS must be 2 or 4";
    return NNGP_ERR_ARG;
  }
  return NNGP_OK;
}

hipError_t summary_launch(int bits, hipStream_t st, const double* x, const double* off, long long S, int w,
                          long long pitch, const SummaryRequest* req, double* out, long long n, long long c0) {
  return bits == 4 ? launch_summary<4>(st, x, off, S, w, pitch, req, out, n, c0)
                   : launch_summary<2>(st, x, off, S, w, pitch, req, out, n, c0);
}

int summary_make_request(const double* probs, int n_probs, const double* thresholds, int n_thresholds,
                         SummaryRequest* req, std::string& err) {
  if (n_probs < 0 || n_probs > kSummaryProbsMax || n_thresholds < 0 || n_thresholds > kSummaryThrMax) {
    err = "summary: n_probs must be 0..16 and n_thresholds 0..8";
    return NNGP_ERR_ARG;
  }
  if ((n_probs > 0 && !probs) || (n_thresholds > 0 && !thresholds)) {
    err = "summary: null probs or thresholds with a positive count";
    return NNGP_ERR_ARG;
  }
  *req = {};
  req->n_probs = n_probs;
  req->n_thr = n_thresholds;
  for (int i = 0; i < n_probs; ++i) {
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) {  // a NaN fails both compares
      err = "summary: a probability is NaN or outside [0, 1]";
      return NNGP_ERR_ARG;
    }
    req->probs[i] = probs[i];
  }
  for (int k = 0; k < n_thresholds; ++k) {
    if (thresholds[k] != thresholds[k]) {
      err = "summary: a threshold is NaN";
      return NNGP_ERR_ARG;
    }
    req->thr[k] = thresholds[k];
  }
  return NNGP_OK;
}

int summary_run(int device, const double* const* blocks, const long long* block_rows, int n_blocks, long long n,
                const double* row_offset, int chunk_cols, double* out, SummaryStats* stats, std::string& err) {
  return summary_stage(device, blocks, block_rows, n_blocks, n, row_offset, chunk_cols, nullptr, kSummaryCols, out, stats,
                       err);
}

int summary_run_probs(int device, const double* const* blocks, const long long* block_rows, int n_blocks, long long n,
                      const double* row_offset, int chunk_cols, const double* probs, int n_probs,
                      const double* thresholds, int n_thresholds, double* out, SummaryStats* stats, std::string& err) {
  SummaryRequest req;
  if (const int rc = summary_make_request(probs, n_probs, thresholds, n_thresholds, &req, err)) return rc;
  return summary_stage(device, blocks, block_rows, n_blocks, n, row_offset, chunk_cols, &req, 2 + n_probs + n_thresholds,
                       out, stats, err);
}

}  // namespace nngp
