// Pointwise Gaussian log-likelihood of the saved samples, reduced per
// observation on the device (the dnorm terms of update_Gaussian.R:130-131,281
// behind WAIC, LPML, DIC and the held-out log score / PIT).
//
// Per sample s and observation i at location c = obs_loc[i] - 1, the value is
// defined by its arithmetic (include/nngp.h, nngp_pointwise_loglik):
//
//   acc  = coef[s,0] * X[i,0]
//   acc  = fma(coef[s,k], X[i,k], acc)          k = 1 .. q-1, in column order
//   mean = field[s,c] + acc                     (field[s,c] alone when q == 0)
//   r    = y[i] - mean
//   ll   = fma(-(h_s * r), r, a_s)              a_s, h_s, g_s = sqrt(2 h_s): host, fp64
//   p    = 0.5 * erfc(-((r * g_s) * (1 / sqrt 2)))
//
// and the six outputs are sequential fp64 reductions over s in row order, in
// two passes (the second needs the first's mean and maxima):
//
//   pass 1: sum mean, sum ll, M = max ll, M' = max -ll, sum p
//   pass 2: ss = fma(d, d, ss) with d = ll - ll_mean; e = sum exp(ll - M);
//           e' = sum exp(-ll - M')
//
// Layout.  A chunk of w locations is staged as S rows x w columns (pitch W),
// as summary.hip stages it.  Observations are sorted by location, so the ones
// of a chunk are one contiguous run; one lane owns one observation of the run
// and carries every sum of it through all samples: no split sums, no atomics,
// no cross-lane operation, so an observation's numbers depend on its inputs
// and its location's column only.  Neighbouring lanes read neighbouring (or
// the same) columns of a sample's row: the gathered field reads are as
// coalesced as the observation counts per location allow.
//
// Tiling.  A workgroup owns 256 observations and walks the samples in tiles of
// kCriteriaRows = 16: per tile and k one coalesced 8-byte load of X[i + k n_obs]
// per lane and 16 FMAs whose coefficients coef[s0 .. s0+15, k] are wave-uniform
// (the effects generator's scheme), then the tile's 16 field loads in flight at
// once.  The tile's means go to a per-lane LDS column (each lane reads back only
// what it wrote: no barrier) and a rolled loop makes the per-sample step, so
// the erfc / exp bodies exist once in the code, not once per accumulator.
// Pass 2 recomputes the means by the same code (bit for bit the same values)
// instead of keeping n_samples values per observation: a location may carry
// many observations, so the chunk buffer cannot hold them, and the second read
// of the chunk comes from HBM while the next chunk is still crossing the host
// link, which is what bounds the call (DESIGN.md "Model criteria").
#include "criteria.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/nngp.h"
#include "summary.h"
#include "summary_launch.h"

namespace nngp {
namespace {

constexpr int kCriteriaBlock = 256;
constexpr int kCriteriaRows = 16;  // samples per tile: accumulators per lane, LDS rows

// what a launch needs besides its pointers (separate __restrict__ kernel
// arguments, so the wave-uniform reads of coef and the constants can be scalar)
struct CriteriaGen {
  long long S, n_obs, o0, c0, pitch;
  double log_S;
  int q, count;  // observations o0 .. o0 + count - 1 read columns c0 .. of the chunk
};

// the sums one lane carries
struct CriteriaSums {
  double sum_mean = 0.0, sum_ll = 0.0, sum_pit = 0.0;
  double M = -std::numeric_limits<double>::infinity(), Mn = -std::numeric_limits<double>::infinity();
  double ll_mean = 0.0, ss = 0.0, e = 0.0, en = 0.0;
};

// The means of the tile's samples s0 .. s0 + rows - 1 for the lane's
// observation, into the lane's LDS column: xc = X + i, fc = chunk + column,
// cf = coef + s0.  FULL: rows == kCriteriaRows; else the surplus slots repeat
// the tile's last row and are not read back.
template <bool FULL, bool HASQ>
__device__ __forceinline__ void criteria_means(const CriteriaGen& g, long long s0, int rows,
                                               const double* __restrict__ cf, const double* __restrict__ xc,
                                               const double* __restrict__ fc, double* __restrict__ mine) {
// the arithmetic above is the contract: a product and a sum stay two roundings
#pragma clang fp contract(off)
  double f[kCriteriaRows];
#pragma unroll
  for (int i = 0; i < kCriteriaRows; ++i) f[i] = fc[(s0 + (FULL || i < rows ? i : rows - 1)) * g.pitch];
  if constexpr (HASQ) {
    double acc[kCriteriaRows];
    double x = xc[0];
#pragma unroll
    for (int i = 0; i < kCriteriaRows; ++i) acc[i] = cf[FULL || i < rows ? i : rows - 1] * x;
#pragma unroll 2
    for (int k = 1; k < g.q; ++k) {
      x = xc[(long long)k * g.n_obs];
      const double* __restrict__ ck = cf + (long long)k * g.S;
#pragma unroll
      for (int i = 0; i < kCriteriaRows; ++i) acc[i] = __builtin_fma(ck[FULL || i < rows ? i : rows - 1], x, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < kCriteriaRows; ++i) f[i] = f[i] + acc[i];
  }
#pragma unroll
  for (int i = 0; i < kCriteriaRows; ++i) mine[i * kCriteriaBlock] = f[i];
}

// One pass over all samples for the lane's observation.  cst: a_s at [s], h_s
// at [S + s], g_s at [2 S + s].
template <int PASS, bool HASQ>
__device__ __forceinline__ void criteria_pass(const CriteriaGen& g, const double* __restrict__ coef,
                                              const double* __restrict__ xc, const double* __restrict__ fc,
                                              const double* __restrict__ cst, double yv, double* __restrict__ mine,
                                              CriteriaSums& A) {
#pragma clang fp contract(off)
  for (long long s0 = 0; s0 < g.S; s0 += kCriteriaRows) {
    const int rows = (int)(g.S - s0 < kCriteriaRows ? g.S - s0 : kCriteriaRows);
    if (rows == kCriteriaRows)
      criteria_means<true, HASQ>(g, s0, rows, coef + s0, xc, fc, mine);
    else
      criteria_means<false, HASQ>(g, s0, rows, coef + s0, xc, fc, mine);
#pragma unroll 1
    for (int i = 0; i < rows; ++i) {
      const long long s = s0 + i;
      const double mean = mine[i * kCriteriaBlock];
      const double r = yv - mean;
      const double ll = __builtin_fma(-(cst[g.S + s] * r), r, cst[s]);
      if constexpr (PASS == 1) {
        A.sum_mean = A.sum_mean + mean;
        A.sum_ll = A.sum_ll + ll;
        A.M = ll > A.M ? ll : A.M;  // a NaN leaves the maxima alone and poisons the sums
        const double nl = -ll;
        A.Mn = nl > A.Mn ? nl : A.Mn;
        const double u = r * cst[2 * g.S + s];
        A.sum_pit = A.sum_pit + 0.5 * erfc(-(u * 0.70710678118654752440));
      } else {
        const double d = ll - A.ll_mean;
        A.ss = __builtin_fma(d, d, A.ss);
        A.e = A.e + exp(ll - A.M);
        A.en = A.en + exp(-ll - A.Mn);
      }
    }
  }
}

// y, obs_loc: n_obs; X: n_obs x q column-major; coef: S x q column-major; buf:
// the chunk, S rows of pitch g.pitch; out: n_obs x 6 column-major
template <bool HASQ>
__global__ __launch_bounds__(kCriteriaBlock) void criteria_kernel(const CriteriaGen g, const double* __restrict__ y,
                                                                  const int* __restrict__ obs_loc,
                                                                  const double* __restrict__ coef,
                                                                  const double* __restrict__ X,
                                                                  const double* __restrict__ buf,
                                                                  const double* __restrict__ cst,
                                                                  double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double stash[kCriteriaRows * kCriteriaBlock];
  const long long j = (long long)blockIdx.x * kCriteriaBlock + threadIdx.x;
  if (j >= g.count) return;
  const long long i = g.o0 + j;
  // the host cut the run so that every column lies in the chunk
  const double* __restrict__ fc = buf + ((long long)obs_loc[i] - 1 - g.c0);
  const double* __restrict__ xc = X + i;
  double* __restrict__ mine = stash + threadIdx.x;
  const double yv = y[i];
  const double Sd = (double)g.S;
  CriteriaSums A;
  criteria_pass<1, HASQ>(g, coef, xc, fc, cst, yv, mine, A);
  A.ll_mean = A.sum_ll / Sd;
  criteria_pass<2, HASQ>(g, coef, xc, fc, cst, yv, mine, A);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double o[kCriteriaCols];
  o[0] = A.sum_mean / Sd;
  o[1] = A.ll_mean;
  o[2] = g.S > 1 ? A.ss / (Sd - 1.0) : nan;
  o[3] = (A.M + log(A.e)) - g.log_S;
  o[4] = -((A.Mn + log(A.en)) - g.log_S);
  o[5] = A.sum_pit / Sd;
  // a NaN in y, X, coef or the column reaches every ll sum; y's does not reach
  // the sum of the means, so the six are set together
  const bool poisoned = A.ll_mean != A.ll_mean;
#pragma unroll
  for (int c = 0; c < kCriteriaCols; ++c) out[i + (long long)c * g.n_obs] = poisoned ? nan : o[c];
}

// every device object of a call; freed on every exit path
struct CriteriaDev {
  double* buf[2] = {nullptr, nullptr};
  double *y = nullptr, *coef = nullptr, *X = nullptr, *cst = nullptr, *out = nullptr;
  int* obs_loc = nullptr;
  hipStream_t copy_st = nullptr, run_st = nullptr;
  hipEvent_t copy0[2] = {}, copy1[2] = {}, run0[2] = {}, run1[2] = {};
  ~CriteriaDev() {
    for (int b = 0; b < 2; ++b) {
      if (buf[b]) (void)hipFree(buf[b]);
      for (hipEvent_t e : {copy0[b], copy1[b], run0[b], run1[b]})
        if (e) (void)hipEventDestroy(e);
    }
    for (void* p : {(void*)y, (void*)coef, (void*)X, (void*)cst, (void*)out, (void*)obs_loc})
      if (p) (void)hipFree(p);
    if (copy_st) (void)hipStreamDestroy(copy_st);
    if (run_st) (void)hipStreamDestroy(run_st);
  }
};

}  // namespace

int criteria_run(const CriteriaArgs& a, CriteriaStats* stats, std::string& err) {
  auto bad = [&](const char* what) {
    err = std::string("pointwise_loglik: ") + what;
    return NNGP_ERR_ARG;
  };
  if (!a.y || !a.obs_loc || !a.out || !a.log_noise_var) return bad("null y, obs_loc, out or log_noise_var");
  if (a.n_obs < 1) return bad("n_obs < 1");
  if (a.n < 1) return bad("n < 1");
  if (a.n_samples < 1 || a.n_samples > 0x7fffffffLL) return bad("n_samples must be 1 .. 2^31 - 1");
  if (a.q < 0 || a.q > kCriteriaQMax) return bad("q must be 0 .. 1024");
  if (a.q > 0 && (!a.coef || !a.X)) return bad("q > 0 needs coef and X");
  if (a.chunk_cols < 0) return bad("chunk_cols < 0");
  if (a.n_blocks < 1 || !a.field_blocks || !a.block_rows) return bad("no field blocks");
  {
    long long rows = 0;
    for (int k = 0; k < a.n_blocks; ++k) {
      if (!a.field_blocks[k] || a.block_rows[k] < 0 || a.block_rows[k] > a.n_samples)
        return bad("a null field block or a row count outside 0 .. n_samples");
      rows += a.block_rows[k];
    }
    if (rows != a.n_samples) return bad("the field blocks' rows do not sum to n_samples");
  }
  for (long long i = 0; i < a.n_obs; ++i) {
    if (a.obs_loc[i] < 1 || a.obs_loc[i] > a.n) return bad("an obs_loc outside 1 .. n");
    if (i > 0 && a.obs_loc[i] < a.obs_loc[i - 1]) return bad("obs_loc decreases");
  }
  const long long S = a.n_samples, n = a.n, n_obs = a.n_obs;
  // the per-sample constants, once per call in fp64: a_s, h_s, g_s
  std::vector<double> cst(3 * (size_t)S);
  const double log_2pi = std::log(2.0 * 3.14159265358979323846);
  for (long long s = 0; s < S; ++s) {
    const double lnv = a.log_noise_var[s];
    if (!std::isfinite(lnv)) return bad("a log_noise_var is NaN or infinite");
    const double h = 0.5 * std::exp(-lnv);
    cst[s] = -0.5 * (log_2pi + lnv);
    cst[S + s] = h;
    cst[2 * S + s] = std::sqrt(2.0 * h);
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    err = "no HIP device";
    return NNGP_ERR_NODEV;
  }
  if (a.device >= ndev) return bad("device ordinal out of range");
  // the calling thread's current device is put back on every exit path
  // (declared before the device objects, so they are released first)
  struct RestoreDevice {
    int prev = -1;
    ~RestoreDevice() {
      if (prev >= 0) (void)hipSetDevice(prev);
    }
  } restore;
  if (a.device >= 0 && (hipGetDevice(&restore.prev) != hipSuccess || restore.prev == a.device)) restore.prev = -1;
  hipError_t e = a.device < 0 ? hipSuccess : hipSetDevice(a.device);
  auto hip_fail = [&](const char* what) {
    err = std::string("pointwise_loglik: ") + what + ": " + hipGetErrorString(e);
    return NNGP_ERR_HIP;
  };
  if (e != hipSuccess) return hip_fail("hipSetDevice");

  // the summary's chunk rule: both chunk buffers within kSummaryStageBudget
  const long long W = summary_chunk_width(S, n, a.chunk_cols);

  CriteriaDev D;
  const size_t chunk_bytes = sizeof(double) * (size_t)S * (size_t)W;
  for (int b = 0; b < 2; ++b)
    if (hipMalloc((void**)&D.buf[b], chunk_bytes) != hipSuccess) {
      (void)hipGetLastError();
      err = "pointwise_loglik: chunk buffers do not fit the device (smaller chunk_cols?)";
      return NNGP_ERR_NOMEM;
    }
  const size_t coef_bytes = sizeof(double) * (size_t)S * (size_t)a.q, x_bytes = sizeof(double) * (size_t)n_obs * (size_t)a.q;
  const size_t out_bytes = sizeof(double) * (size_t)kCriteriaCols * (size_t)n_obs;
  if (hipMalloc((void**)&D.out, out_bytes) != hipSuccess ||
      hipMalloc((void**)&D.y, sizeof(double) * (size_t)n_obs) != hipSuccess ||
      hipMalloc((void**)&D.obs_loc, sizeof(int) * (size_t)n_obs) != hipSuccess ||
      hipMalloc((void**)&D.cst, sizeof(double) * cst.size()) != hipSuccess ||
      (a.q > 0 && (hipMalloc((void**)&D.coef, coef_bytes) != hipSuccess || hipMalloc((void**)&D.X, x_bytes) != hipSuccess))) {
    (void)hipGetLastError();
    err = "pointwise_loglik: device allocation failed";
    return NNGP_ERR_NOMEM;
  }
#define CRITERIA_HIP(x)                       \
  do {                                        \
    e = (x);                                  \
    if (e != hipSuccess) return hip_fail(#x); \
  } while (0)
  CRITERIA_HIP(hipStreamCreateWithFlags(&D.copy_st, hipStreamNonBlocking));
  CRITERIA_HIP(hipStreamCreateWithFlags(&D.run_st, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b)
    for (hipEvent_t* ev : {&D.copy0[b], &D.copy1[b], &D.run0[b], &D.run1[b]}) CRITERIA_HIP(hipEventCreate(ev));
  // everything but the field goes up once, ahead of the first kernel on the run stream
  CRITERIA_HIP(hipMemcpyAsync(D.y, a.y, sizeof(double) * (size_t)n_obs, hipMemcpyHostToDevice, D.run_st));
  CRITERIA_HIP(hipMemcpyAsync(D.obs_loc, a.obs_loc, sizeof(int) * (size_t)n_obs, hipMemcpyHostToDevice, D.run_st));
  CRITERIA_HIP(hipMemcpyAsync(D.cst, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice, D.run_st));
  if (a.q > 0) {
    CRITERIA_HIP(hipMemcpyAsync(D.coef, a.coef, coef_bytes, hipMemcpyHostToDevice, D.run_st));
    CRITERIA_HIP(hipMemcpyAsync(D.X, a.X, x_bytes, hipMemcpyHostToDevice, D.run_st));
  }

  CriteriaStats st;
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
  CriteriaGen g{S, n_obs, 0, 0, W, std::log((double)S), a.q, 0};
  long long k = 0, o1 = 0;
  for (long long c0 = 0; c0 < n; c0 += W, ++k) {
    const int b = (int)(k & 1);
    const int w = (int)std::min(W, n - c0);
    // the chunk's observations: the run o0 .. o1 - 1 of the sorted obs_loc
    const long long o0 = o1;
    while (o1 < n_obs && (long long)a.obs_loc[o1] - 1 < c0 + w) ++o1;
    if (k >= 2) {  // slot b: the kernel of chunk k - 2 has read it
      CRITERIA_HIP(hipEventSynchronize(D.run1[b]));
      CRITERIA_HIP(collect(b));
    }
    CRITERIA_HIP(hipEventRecord(D.copy0[b], D.copy_st));
    if (o1 > o0) {  // a chunk no observation reads is not staged
      long long row = 0;
      for (int j = 0; j < a.n_blocks; ++j) {
        if (a.block_rows[j] == 0) continue;
        CRITERIA_HIP(hipMemcpy2DAsync(D.buf[b] + (size_t)row * (size_t)W, sizeof(double) * (size_t)W,
                                      a.field_blocks[j] + c0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)w,
                                      (size_t)a.block_rows[j], hipMemcpyHostToDevice, D.copy_st));
        row += a.block_rows[j];
      }
      st.staged_bytes += (long long)sizeof(double) * S * w;
    }
    CRITERIA_HIP(hipEventRecord(D.copy1[b], D.copy_st));
    CRITERIA_HIP(hipStreamWaitEvent(D.run_st, D.copy1[b], 0));
    CRITERIA_HIP(hipEventRecord(D.run0[b], D.run_st));
    if (o1 > o0) {
      g.c0 = c0;
      // a run of more than 2^30 observations is cut into launches of that many
      for (g.o0 = o0; g.o0 < o1; g.o0 += g.count) {
        g.count = (int)std::min<long long>(o1 - g.o0, 0x40000000LL);
        const dim3 grid((unsigned)((g.count + kCriteriaBlock - 1) / kCriteriaBlock)), block(kCriteriaBlock);
        if (a.q > 0)
          hipLaunchKernelGGL(criteria_kernel<true>, grid, block, 0, D.run_st, g, D.y, D.obs_loc, D.coef, D.X, D.buf[b],
                             D.cst, D.out);
        else
          hipLaunchKernelGGL(criteria_kernel<false>, grid, block, 0, D.run_st, g, D.y, D.obs_loc, D.coef, D.X, D.buf[b],
                             D.cst, D.out);
        CRITERIA_HIP(hipGetLastError());
      }
    }
    CRITERIA_HIP(hipEventRecord(D.run1[b], D.run_st));
  }
  st.n_chunks = (int)k;
  CRITERIA_HIP(hipMemcpyAsync(a.out, D.out, out_bytes, hipMemcpyDeviceToHost, D.run_st));
  CRITERIA_HIP(hipStreamSynchronize(D.run_st));
  for (long long j = std::max(0LL, k - 2); j < k; ++j) CRITERIA_HIP(collect((int)(j & 1)));
#undef CRITERIA_HIP
  if (stats) *stats = st;
  return NNGP_OK;
}

}  // namespace nngp
