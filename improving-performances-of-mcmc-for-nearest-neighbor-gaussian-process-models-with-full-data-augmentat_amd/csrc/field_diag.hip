// Per-location convergence diagnostics of the field samples on the device
// (Scripts/mcmc_nngp_diagnose.R:1-24 Individual_PSRF, :107-118 ESS): R_hat,
// ess, ess_min, W and Bv of every column of m chains' S x n sample blocks.
//
// One lane owns one column of a staged chunk (m S rows x w columns, row-major,
// pitch W; chain k is rows k S .. (k + 1) S - 1): in every pass a wavefront
// reads 64 neighbouring columns of a row, 512 contiguous bytes, and the row's
// offset is one scalar load.  Per chain a lane makes two passes over its
// column: the mean (sum in row order), then the centred lagged products
// sum_t xc[t] xc[t - l], l = 0..P, with the sums in registers (CAP + 1 of
// them, CAP >= P the instantiation's bound; the lag loop is unrolled CAP times
// without a branch) and the lane's last P centred values in an
// LDS ring laid out [slot][lane] (one global load, one LDS write and CAP LDS
// reads per row).  A workgroup is one
// wavefront and a lane touches only its own LDS words, so there is no barrier
// and no cross-lane operation: a lane's numbers depend on its own column
// only, not on the chunk width, the column's position or its neighbours.
// After the lag pass the ring is dead and holds phi of the Levinson-Durbin
// recursion (field_diag.h).
#include "field_diag_run.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/nngp.h"
#include "field_diag.h"

namespace nngp {
namespace {

constexpr int kDiagBlock = 64;  // one wavefront per workgroup

struct LdsPhi {
  double* p;  // the lane's word of slot 0
  __device__ __forceinline__ double& operator[](int j) const { return p[j * kDiagBlock]; }
};

// x: the staged chunk; off: m S row offsets (OFF) or unused; P: the largest
// order, <= CAP (the register bound of this instantiation); dynamic LDS:
// max(P, 1) slots of 64 doubles.  out: n x 5 column-major, order: m x n or
// null; this launch writes columns c0 .. c0 + w - 1.
template <int CAP, bool OFF>
__global__ __launch_bounds__(kDiagBlock) void field_diag_kernel(const double* __restrict__ x,
                                                                const double* __restrict__ off, int m, int S, int P,
                                                                int w, long long pitch, double* __restrict__ out,
                                                                int* __restrict__ order, long long n, long long c0) {
  extern __shared__ double ring_all[];
  const int c = blockIdx.x * kDiagBlock + threadIdx.x;
  if (c >= w) return;
  double* const ring = ring_all + threadIdx.x;  // slot s of this lane: ring[s * kDiagBlock]
  const int Pw = P > 0 ? P : 1;
  double mean[kFieldDiagMaxChains], var[kFieldDiagMaxChains], ess[kFieldDiagMaxChains];
  bool nan = false;
  for (int k = 0; k < m; ++k) {
    const double* col = x + (size_t)k * (size_t)S * (size_t)pitch + c;
    const double* o = OFF ? off + (size_t)k * S : nullptr;
    auto load = [&](int s) -> double {
      const double v = col[(size_t)s * (size_t)pitch];
      return OFF ? v - o[s] : v;
    };
    double mu;
    {
#pragma clang fp contract(off)
      double sum = 0.0;
#pragma unroll 4
      for (int s = 0; s < S; ++s) {
        const double v = load(s);
        nan = nan || v != v;
        sum += v;
      }
      mu = sum / (double)S;
    }
    for (int l = 0; l < Pw; ++l) ring[l * kDiagBlock] = 0.0;
    double acc[CAP + 1];
#pragma unroll
    for (int l = 0; l <= CAP; ++l) acc[l] = 0.0;
    int ws = 0;  // the slot row t goes to: ws(t) = -t mod P, so row t - l lies at ws + l mod P
    // the next row's value and offset are fetched raw, one row ahead, and
    // combined only when used, so the load runs beside this row's lags
    double next = col[0], next_off = OFF ? o[0] : 0.0;
    for (int t = 0; t < S; ++t) {
      const double xc = (OFF ? next - next_off : next) - mu;
      if (t + 1 < S) {
        next = col[(size_t)(t + 1) * (size_t)pitch];
        if (OFF) next_off = o[t + 1];
      }
      acc[0] = fma(xc, xc, acc[0]);
#pragma unroll
      for (int l = 1; l <= CAP; ++l) {
        // No branch on l <= P: every acc index is a constant and the CAP LDS
        // reads of a row are independent, so they are all in flight together.
        // A lag beyond P reads a valid slot into a sum that nothing uses.
        int s = ws + l;
        s = s >= P ? s - P : s;
        s = s < Pw ? s : Pw - 1;
        acc[l] = fma(xc, ring[s * kDiagBlock], acc[l]);
      }
      ring[ws * kDiagBlock] = xc;
      ws = ws == 0 ? Pw - 1 : ws - 1;
    }
    double acf[CAP + 1];
#pragma unroll
    for (int l = 0; l <= CAP; ++l) acf[l] = acc[l] / (double)S;
    int ord = 0;
    mean[k] = mu;
    var[k] = acc[0] / (double)(S - 1);
    ess[k] = field_diag_ess(acf, (long long)S, P, LdsPhi{ring}, &ord);
    if (order) order[(size_t)k * (size_t)n + (size_t)(c0 + c)] = ord;
  }
  double r[kFieldDiagCols];
  field_diag_combine(mean, var, ess, m, (long long)S, nan, r);
#pragma unroll
  for (int q = 0; q < kFieldDiagCols; ++q) out[q * n + c0 + c] = r[q];
  if (order && nan)
    for (int k = 0; k < m; ++k) order[(size_t)k * (size_t)n + (size_t)(c0 + c)] = 0;
}

template <int CAP>
hipError_t launch_cap(hipStream_t st, const double* x, const double* off, int m, int S, int P, int w, long long pitch,
                      double* out, int* order, long long n, long long c0) {
  const dim3 grid((w + kDiagBlock - 1) / kDiagBlock), block(kDiagBlock);
  const size_t lds = sizeof(double) * kDiagBlock * (size_t)std::max(P, 1);
  if (off)
    hipLaunchKernelGGL((field_diag_kernel<CAP, true>), grid, block, lds, st, x, off, m, S, P, w, pitch, out, order, n, c0);
  else
    hipLaunchKernelGGL((field_diag_kernel<CAP, false>), grid, block, lds, st, x, off, m, S, P, w, pitch, out, order, n, c0);
  return hipGetLastError();
}

// the instantiation with the fewest accumulators that holds P + 1 of them
hipError_t launch_field_diag(hipStream_t st, const double* x, const double* off, int m, int S, int P, int w,
                             long long pitch, double* out, int* order, long long n, long long c0) {
  if (P <= 8) return launch_cap<8>(st, x, off, m, S, P, w, pitch, out, order, n, c0);
  if (P <= 24) return launch_cap<24>(st, x, off, m, S, P, w, pitch, out, order, n, c0);
  return launch_cap<kFieldDiagMaxOrder>(st, x, off, m, S, P, w, pitch, out, order, n, c0);
}

// every device object of a call; freed on every exit path
struct DiagDev {
  double* buf[2] = {nullptr, nullptr};
  double* off = nullptr;
  double* out = nullptr;
  int* order = nullptr;
  hipStream_t copy_st = nullptr, run_st = nullptr;
  hipEvent_t copy0[2] = {}, copy1[2] = {}, run0[2] = {}, run1[2] = {};
  ~DiagDev() {
    for (int b = 0; b < 2; ++b) {
      if (buf[b]) (void)hipFree(buf[b]);
      for (hipEvent_t e : {copy0[b], copy1[b], run0[b], run1[b]})
        if (e) (void)hipEventDestroy(e);
    }
    if (off) (void)hipFree(off);
    if (out) (void)hipFree(out);
    if (order) (void)hipFree(order);
    if (copy_st) (void)hipStreamDestroy(copy_st);
    if (run_st) (void)hipStreamDestroy(run_st);
  }
};

}  // namespace

int field_diag_run(int device, const double* const* blocks, int n_chains, long long rows, long long n,
                   const double* row_offset, int chunk_cols, double* out, int* order, FieldDiagStats* stats,
                   std::string& err) {
  if (!blocks || !out || n < 1 || n_chains < 1 || n_chains > kFieldDiagMaxChains || rows < 2 ||
      rows > kFieldDiagMaxRows || chunk_cols < 0) {
    err = "field_diag: bad args (n >= 1, 1..16 chains, 2..9999 rows, chunk_cols >= 0)";
    return NNGP_ERR_ARG;
  }
  for (int k = 0; k < n_chains; ++k)
    if (!blocks[k]) {
      err = "field_diag: null block";
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
    err = std::string("field_diag: ") + what + ": " + hipGetErrorString(e);
    return NNGP_ERR_HIP;
  };
  if (e != hipSuccess) return hip_fail("hipSetDevice");

  const int S = (int)rows, m = n_chains;
  const long long R = rows * m;  // staged rows
  const int P = field_diag_max_order(rows);
  // chunk width W (columns per launch), as nngp_summary chooses it: the two
  // staging buffers stay within kFieldDiagStageBudget (never below one
  // wavefront of columns); a matrix that would fit one chunk is still cut into
  // about four, so that copies and kernels overlap, unless that leaves fewer
  // than 64 Ki columns per launch.
  long long W = chunk_cols;
  if (W == 0) {
    W = (long long)(kFieldDiagStageBudget / 2 / sizeof(double)) / R / 256 * 256;
    const long long quarter = (n / 4 + 255) / 256 * 256;
    W = std::min(W, std::max(65536LL, quarter));
    W = std::max(W, 64LL);
  }
  W = std::min(W, n);

  DiagDev D;
  const size_t chunk_bytes = sizeof(double) * (size_t)R * (size_t)W;
  for (int b = 0; b < 2; ++b)
    if (hipMalloc((void**)&D.buf[b], chunk_bytes) != hipSuccess) {
      (void)hipGetLastError();
      err = "field_diag: staging buffers do not fit the device (smaller chunk_cols?)";
      return NNGP_ERR_NOMEM;
    }
  if (hipMalloc((void**)&D.out, sizeof(double) * kFieldDiagCols * (size_t)n) != hipSuccess ||
      (order && hipMalloc((void**)&D.order, sizeof(int) * (size_t)m * (size_t)n) != hipSuccess) ||
      (row_offset && hipMalloc((void**)&D.off, sizeof(double) * (size_t)R) != hipSuccess)) {
    (void)hipGetLastError();
    err = "field_diag: device allocation failed";
    return NNGP_ERR_NOMEM;
  }
#define DIAG_HIP(x)                           \
  do {                                        \
    e = (x);                                  \
    if (e != hipSuccess) return hip_fail(#x); \
  } while (0)
  DIAG_HIP(hipStreamCreateWithFlags(&D.copy_st, hipStreamNonBlocking));
  DIAG_HIP(hipStreamCreateWithFlags(&D.run_st, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    DIAG_HIP(hipEventCreate(&D.copy0[b]));
    DIAG_HIP(hipEventCreate(&D.copy1[b]));
    DIAG_HIP(hipEventCreate(&D.run0[b]));
    DIAG_HIP(hipEventCreate(&D.run1[b]));
  }
  if (row_offset) DIAG_HIP(hipMemcpyAsync(D.off, row_offset, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, D.run_st));

  FieldDiagStats st;
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
      DIAG_HIP(hipEventSynchronize(D.run1[b]));
      DIAG_HIP(collect(b));
    }
    DIAG_HIP(hipEventRecord(D.copy0[b], D.copy_st));
    for (int q = 0; q < m; ++q)
      DIAG_HIP(hipMemcpy2DAsync(D.buf[b] + (size_t)q * (size_t)rows * (size_t)W, sizeof(double) * (size_t)W,
                                blocks[q] + c0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)w, (size_t)rows,
                                hipMemcpyHostToDevice, D.copy_st));
    DIAG_HIP(hipEventRecord(D.copy1[b], D.copy_st));
    st.staged_bytes += (long long)sizeof(double) * R * w;
    DIAG_HIP(hipStreamWaitEvent(D.run_st, D.copy1[b], 0));
    DIAG_HIP(hipEventRecord(D.run0[b], D.run_st));
    DIAG_HIP(launch_field_diag(D.run_st, D.buf[b], D.off, m, S, P, w, W, D.out, D.order, n, c0));
    DIAG_HIP(hipEventRecord(D.run1[b], D.run_st));
  }
  st.n_chunks = (int)k;
  DIAG_HIP(hipMemcpyAsync(out, D.out, sizeof(double) * kFieldDiagCols * (size_t)n, hipMemcpyDeviceToHost, D.run_st));
  if (order) DIAG_HIP(hipMemcpyAsync(order, D.order, sizeof(int) * (size_t)m * (size_t)n, hipMemcpyDeviceToHost, D.run_st));
  DIAG_HIP(hipStreamSynchronize(D.run_st));
  for (long long q = std::max(0LL, k - 2); q < k; ++q) DIAG_HIP(collect((int)(q & 1)));
#undef DIAG_HIP
  if (stats) *stats = st;
  return NNGP_OK;
}

}  // namespace nngp
