// Fixed-effect and response prediction summarised on the device
// (mcmc_nngp_predict_fixed_effects, Scripts/mcmc_nngp_predict.R:92-102: the
// samples beta_matrix[, subset] %*% t(X_pred) and their get_summary).
//
// The n_samples x n matrix of samples is never formed on the host: a generator
// kernel fills a chunk of S rows x w columns (row-major, pitch W), the layout
// summary.hip's kernels read, and the summary launch follows it on the same
// stream.  The value of sample s at location c is defined by its arithmetic:
//
//   acc = coef[s,0] * X[c,0]
//   acc = fma(coef[s,k], X[c,k], acc)            k = 1 .. q-1, in column order
//   acc = addend[s,c] + acc                      with an addend
//   acc = fma(noise_sd[s], z(seed, counter[s], c), acc)   with noise
//
// (z = normal_loc of device_common.h, what nngp_device_normals returns at c.)
// One lane owns one column and carries the one accumulator of each sample
// through all k: no split sums, no atomics, no cross-lane operation, so a
// value depends on (s, c) and its inputs only.
//
// Tiling: a workgroup owns 256 columns and a tile of kEffectsRows = 32 samples
// (32 accumulators = 64 VGPRs per lane) and walks k = 0 .. q-1 once per tile:
// per k one coalesced 8-byte load of X[c + k n] per lane (512 B per
// wavefront) and 32 FMAs whose coefficient operands coef[s0 .. s0+31, k] are
// wave-uniform, 256 contiguous bytes of the column-major coef: scalar loads.
// Sample tiles are spread over blockIdx.y, so a chunk launches
// ceil(w / 256) x min(ceil(S / 32), 64) workgroups.  X is re-read once per
// sample tile (from L2: a workgroup's slice is 256 q doubles); the chunk is
// written once.  DESIGN.md "Effects summary" has the bytes and flops.
#include "effects.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/nngp.h"
#include "device_common.h"
#include "summary.h"
#include "summary_launch.h"

namespace nngp {
namespace {

constexpr int kEffectsBlock = 256;
constexpr int kEffectsRows = 32;    // samples per tile: accumulators per lane
constexpr int kEffectsTilesY = 64;  // at most this many workgroups share a column block's sample tiles

// what a launch needs besides its pointers (those are separate __restrict__
// kernel arguments: the chunk's stores then provably leave coef, noise_sd and
// counter alone, and their wave-uniform reads become scalar loads)
struct EffectsGen {
  uint64_t seed;
  long long S, n, c0, pitch;
  int q, w;
};

// One tile of `rows` samples from s0 for the lane's column: xc = X + column,
// bc = chunk + column, cf = coef + s0.  FULL: rows == kEffectsRows, the
// coefficient reads of a k are one contiguous run; else the surplus
// accumulators repeat the tile's last row and are not stored.
template <bool FULL, bool ADD>
__device__ __forceinline__ void effects_tile(const EffectsGen& g, long long s0, int rows, const double* __restrict__ cf,
                                             const double* __restrict__ xc, double* __restrict__ bc) {
// the arithmetic above is the contract: a product and a sum stay two roundings
#pragma clang fp contract(off)
  double acc[kEffectsRows];
  double x = xc[0];
#pragma unroll
  for (int i = 0; i < kEffectsRows; ++i) acc[i] = cf[FULL || i < rows ? i : rows - 1] * x;
#pragma unroll 2
  for (int k = 1; k < g.q; ++k) {
    x = xc[(long long)k * g.n];
    const double* __restrict__ ck = cf + (long long)k * g.S;
#pragma unroll
    for (int i = 0; i < kEffectsRows; ++i) acc[i] = __builtin_fma(ck[FULL || i < rows ? i : rows - 1], x, acc[i]);
  }
#pragma unroll
  for (int i = 0; i < kEffectsRows; ++i) {
    if (FULL || i < rows) {
      double* p = bc + (s0 + i) * g.pitch;
      double v = acc[i];
      if constexpr (ADD) v = *p + v;
      *p = v;
    }
  }
}

// coef: S x q column-major; X: n x q column-major; buf: the chunk, S rows of pitch g.pitch
template <bool ADD, bool NOISE>
__global__ __launch_bounds__(kEffectsBlock) void effects_kernel(const EffectsGen g, const double* __restrict__ coef,
                                                                const double* __restrict__ X, double* __restrict__ buf,
                                                                const double* __restrict__ noise_sd,
                                                                const uint64_t* __restrict__ counter) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * kEffectsBlock + threadIdx.x;
  if (c >= g.w) return;
  const double* __restrict__ xc = X + g.c0 + c;
  double* __restrict__ bc = buf + c;
  const uint32_t loc = (uint32_t)(g.c0 + c);
  const long long ntiles = (g.S + kEffectsRows - 1) / kEffectsRows;
  for (long long t = blockIdx.y; t < ntiles; t += gridDim.y) {
    const long long s0 = t * kEffectsRows;
    const int rows = (int)(g.S - s0 < kEffectsRows ? g.S - s0 : kEffectsRows);
    if (rows == kEffectsRows)
      effects_tile<true, ADD>(g, s0, rows, coef + s0, xc, bc);
    else
      effects_tile<false, ADD>(g, s0, rows, coef + s0, xc, bc);
    if constexpr (NOISE) {
      // the lane's own stores of this tile, in program order: one more fma each
      // (a rolled loop: the Philox / AS241 body is not repeated per accumulator)
#pragma unroll 1
      for (int i = 0; i < rows; ++i) {
        double* p = bc + (s0 + i) * g.pitch;
        *p = __builtin_fma(noise_sd[s0 + i], normal_loc(g.seed, counter[s0 + i], loc), *p);
      }
    }
  }
}

struct EffectsPtrs {
  const double *coef, *X;
  double* buf;
  const double* noise_sd;
  const uint64_t* counter;
};

hipError_t launch_effects(hipStream_t st, const EffectsGen& g, const EffectsPtrs& p, bool add) {
  const long long ntiles = (g.S + kEffectsRows - 1) / kEffectsRows;
  const dim3 grid((g.w + kEffectsBlock - 1) / kEffectsBlock, (unsigned)std::min<long long>(ntiles, kEffectsTilesY));
  const dim3 block(kEffectsBlock);
  const bool noise = p.noise_sd != nullptr;
  if (add && noise)
    hipLaunchKernelGGL((effects_kernel<true, true>), grid, block, 0, st, g, p.coef, p.X, p.buf, p.noise_sd, p.counter);
  else if (add)
    hipLaunchKernelGGL((effects_kernel<true, false>), grid, block, 0, st, g, p.coef, p.X, p.buf, p.noise_sd, p.counter);
  else if (noise)
    hipLaunchKernelGGL((effects_kernel<false, true>), grid, block, 0, st, g, p.coef, p.X, p.buf, p.noise_sd, p.counter);
  else
    hipLaunchKernelGGL((effects_kernel<false, false>), grid, block, 0, st, g, p.coef, p.X, p.buf, p.noise_sd, p.counter);
  return hipGetLastError();
}

// every device object of a call; freed on every exit path
struct EffectsDev {
  double* buf[2] = {nullptr, nullptr};
  double *coef = nullptr, *X = nullptr, *noise_sd = nullptr, *out = nullptr;
  uint64_t* counter = nullptr;
  hipStream_t copy_st = nullptr, run_st = nullptr;
  // per slot: addend copy, generator, summary kernel, and the slot free again
  // (behind the samples' copy out, when there is one)
  hipEvent_t copy0[2] = {}, copy1[2] = {}, gen0[2] = {}, run0[2] = {}, run1[2] = {}, done[2] = {};
  ~EffectsDev() {
    for (int b = 0; b < 2; ++b) {
      if (buf[b]) (void)hipFree(buf[b]);
      for (hipEvent_t e : {copy0[b], copy1[b], gen0[b], run0[b], run1[b], done[b]})
        if (e) (void)hipEventDestroy(e);
    }
    for (void* p : {(void*)coef, (void*)X, (void*)noise_sd, (void*)out, (void*)counter})
      if (p) (void)hipFree(p);
    if (copy_st) (void)hipStreamDestroy(copy_st);
    if (run_st) (void)hipStreamDestroy(run_st);
  }
};

}  // namespace

int effects_run(const EffectsArgs& a, EffectsStats* stats, std::string& err) {
  SummaryRequest req;
  if (const int rc = summary_make_request(a.probs, a.n_probs, a.thresholds, a.n_thresholds, &req, err)) return rc;
  auto bad = [&](const char* what) {
    err = std::string("effects_summary: ") + what;
    return NNGP_ERR_ARG;
  };
  if (!a.coef || !a.X || !a.out) return bad("null coef, X or out");
  if (a.n < 1) return bad("n < 1");
  if (a.n_samples < 1 || a.n_samples > 0x7fffffffLL) return bad("n_samples must be 1 .. 2^31 - 1");
  if (a.q < 1 || a.q > kEffectsQMax) return bad("q must be 1 .. 1024");
  if (a.chunk_cols < 0) return bad("chunk_cols < 0");
  if (a.n_blocks < 0 || (a.n_blocks > 0 && (!a.addend_blocks || !a.block_rows)))
    return bad("n_blocks < 0, or addend blocks without their arrays");
  const bool add = a.n_blocks > 0;
  if (add) {
    long long rows = 0;
    for (int k = 0; k < a.n_blocks; ++k) {
      if (!a.addend_blocks[k] || a.block_rows[k] < 0 || a.block_rows[k] > a.n_samples)
        return bad("a null addend block or a row count outside 0 .. n_samples");
      rows += a.block_rows[k];
    }
    if (rows != a.n_samples) return bad("the addend blocks' rows do not sum to n_samples");
  }
  if (a.noise_sd) {
    if (!a.counter) return bad("noise_sd needs counter");
    // z is nngp_device_normals' value at index c, an int there
    if (a.n > 0x7fffffffLL) return bad("noise needs n <= 2^31 - 1");
    for (long long s = 0; s < a.n_samples; ++s)
      if (!(a.noise_sd[s] >= 0.0)) return bad("a noise_sd is NaN or negative");  // a NaN fails the compare
  }
  const long long S = a.n_samples, n = a.n;
  const int ncols = 2 + a.n_probs + a.n_thresholds;

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
    err = std::string("effects_summary: ") + what + ": " + hipGetErrorString(e);
    return NNGP_ERR_HIP;
  };
  if (e != hipSuccess) return hip_fail("hipSetDevice");

  // the summary's chunk rule: both chunk buffers within kSummaryStageBudget
  const long long W = summary_chunk_width(S, n, a.chunk_cols);
  int bits = 0;
  if (const int rc = summary_digit_bits(&bits, err)) return rc;

  EffectsDev D;
  const size_t chunk_bytes = sizeof(double) * (size_t)S * (size_t)W;
  for (int b = 0; b < 2; ++b)
    if (hipMalloc((void**)&D.buf[b], chunk_bytes) != hipSuccess) {
      (void)hipGetLastError();
      err = "effects_summary: chunk buffers do not fit the device (smaller chunk_cols?)";
      return NNGP_ERR_NOMEM;
    }
  const size_t coef_bytes = sizeof(double) * (size_t)S * (size_t)a.q, x_bytes = sizeof(double) * (size_t)n * (size_t)a.q;
  if (hipMalloc((void**)&D.out, sizeof(double) * (size_t)ncols * (size_t)n) != hipSuccess ||
      hipMalloc((void**)&D.coef, coef_bytes) != hipSuccess || hipMalloc((void**)&D.X, x_bytes) != hipSuccess ||
      (a.noise_sd && (hipMalloc((void**)&D.noise_sd, sizeof(double) * (size_t)S) != hipSuccess ||
                      hipMalloc((void**)&D.counter, sizeof(uint64_t) * (size_t)S) != hipSuccess))) {
    (void)hipGetLastError();
    err = "effects_summary: device allocation failed";
    return NNGP_ERR_NOMEM;
  }
#define EFFECTS_HIP(x)                        \
  do {                                        \
    e = (x);                                  \
    if (e != hipSuccess) return hip_fail(#x); \
  } while (0)
  EFFECTS_HIP(hipStreamCreateWithFlags(&D.copy_st, hipStreamNonBlocking));
  EFFECTS_HIP(hipStreamCreateWithFlags(&D.run_st, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b)
    for (hipEvent_t* ev : {&D.copy0[b], &D.copy1[b], &D.gen0[b], &D.run0[b], &D.run1[b], &D.done[b]})
      EFFECTS_HIP(hipEventCreate(ev));
  // coef and X go up once, ahead of the first generator on the run stream
  EFFECTS_HIP(hipMemcpyAsync(D.coef, a.coef, coef_bytes, hipMemcpyHostToDevice, D.run_st));
  EFFECTS_HIP(hipMemcpyAsync(D.X, a.X, x_bytes, hipMemcpyHostToDevice, D.run_st));
  if (a.noise_sd) {
    EFFECTS_HIP(hipMemcpyAsync(D.noise_sd, a.noise_sd, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, D.run_st));
    EFFECTS_HIP(hipMemcpyAsync(D.counter, a.counter, sizeof(uint64_t) * (size_t)S, hipMemcpyHostToDevice, D.run_st));
  }

  EffectsStats st;
  st.chunk_cols = (int)W;
  // the times of the chunk that used slot b last; called once the slot is free
  auto collect = [&](int b) -> hipError_t {
    float ms = 0.f;
    hipError_t r = hipSuccess;
    if (add) {
      r = hipEventElapsedTime(&ms, D.copy0[b], D.copy1[b]);
      if (r != hipSuccess) return r;
      st.copy_ms += ms;
    }
    r = hipEventElapsedTime(&ms, D.gen0[b], D.run0[b]);
    if (r != hipSuccess) return r;
    st.generate_ms += ms;
    r = hipEventElapsedTime(&ms, D.run0[b], D.run1[b]);
    st.kernel_ms += ms;
    return r;
  };
  EffectsGen g{a.seed, S, n, 0, W, a.q, 0};
  EffectsPtrs ptrs{D.coef, D.X, nullptr, D.noise_sd, D.counter};
  long long k = 0;
  for (long long c0 = 0; c0 < n; c0 += W, ++k) {
    const int b = (int)(k & 1);
    const int w = (int)std::min(W, n - c0);
    if (k >= 2) {  // slot b: chunk k - 2 has been summarised (and copied out)
      EFFECTS_HIP(hipEventSynchronize(D.done[b]));
      EFFECTS_HIP(collect(b));
    }
    if (add) {
      EFFECTS_HIP(hipEventRecord(D.copy0[b], D.copy_st));
      long long row = 0;
      for (int j = 0; j < a.n_blocks; ++j) {
        if (a.block_rows[j] == 0) continue;
        EFFECTS_HIP(hipMemcpy2DAsync(D.buf[b] + (size_t)row * (size_t)W, sizeof(double) * (size_t)W,
                                     a.addend_blocks[j] + c0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)w,
                                     (size_t)a.block_rows[j], hipMemcpyHostToDevice, D.copy_st));
        row += a.block_rows[j];
      }
      EFFECTS_HIP(hipEventRecord(D.copy1[b], D.copy_st));
      st.staged_bytes += (long long)sizeof(double) * S * w;
      EFFECTS_HIP(hipStreamWaitEvent(D.run_st, D.copy1[b], 0));
    }
    ptrs.buf = D.buf[b];
    g.c0 = c0;
    g.w = w;
    EFFECTS_HIP(hipEventRecord(D.gen0[b], D.run_st));
    EFFECTS_HIP(launch_effects(D.run_st, g, ptrs, add));
    EFFECTS_HIP(hipEventRecord(D.run0[b], D.run_st));
    EFFECTS_HIP(summary_launch(bits, D.run_st, D.buf[b], nullptr, S, w, W, &req, D.out, n, c0));
    EFFECTS_HIP(hipEventRecord(D.run1[b], D.run_st));
    if (a.samples_out)
      EFFECTS_HIP(hipMemcpy2DAsync(a.samples_out + c0, sizeof(double) * (size_t)n, D.buf[b], sizeof(double) * (size_t)W,
                                   sizeof(double) * (size_t)w, (size_t)S, hipMemcpyDeviceToHost, D.run_st));
    EFFECTS_HIP(hipEventRecord(D.done[b], D.run_st));
  }
  st.n_chunks = (int)k;
  EFFECTS_HIP(hipMemcpyAsync(a.out, D.out, sizeof(double) * (size_t)ncols * (size_t)n, hipMemcpyDeviceToHost, D.run_st));
  EFFECTS_HIP(hipStreamSynchronize(D.run_st));
  for (long long j = std::max(0LL, k - 2); j < k; ++j) EFFECTS_HIP(collect((int)(j & 1)));
#undef EFFECTS_HIP
  if (stats) *stats = st;
  return NNGP_OK;
}

}  // namespace nngp
