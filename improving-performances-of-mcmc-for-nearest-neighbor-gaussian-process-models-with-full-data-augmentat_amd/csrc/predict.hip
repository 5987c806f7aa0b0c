// Batched posterior prediction at new locations (Scripts/mcmc_nngp_predict.R:39-53)
// without the stacked context.
//
// The stacked factor B of the n observed and n_pred new locations is lower
// triangular and its rows < n name columns < n only, so the top block of
// B^{-1} c(B11 (w / sd), z) is w / sd itself: neither the SpMV nor the first n
// rows of the solve are needed.  With y = w on the observed locations, a new
// location p = n .. N-1 (in order) has
//   y[p] = (sd z[p-n] - sum_{j=1..b-1} Linv[p,j] y[NN[p,j]]) / Linv[p,0]
// and the predicted sample is y[n..N-1].  Only the factor rows of the new
// locations and the observed values those rows name (the support) are used.
//
// Layout: the values of a batch of S samples are stored [compact row][sample]
// with row pitch SP (S rounded up to 64): one lane per sample, so a
// neighbour's values of 64 samples are one coalesced 512-byte line and the
// row's NNarray entries are wave-uniform (scalar loads).  Every sample carries
// the slot of its factor among the batch's factor buffers; lanes of equal slot
// read the same Linv address (one broadcast request).  A lane's arithmetic --
// the fma chain over j in table order, one fma with sd z, one division -- reads
// its own sample's values only, so a sample's bytes do not depend on the
// batch, on its lane or on the other samples.
//
// Scheduling: the dependency levels among the new rows (graph_prep.h
// PredictPlan) are the same for every sample.  A level of more than
// kPredictSmallRows rows is one launch (a wave per row and 64 samples); a run
// of consecutive smaller levels is ONE launch of a workgroup per 64 samples
// that walks the levels with a workgroup barrier in between (sample chunks are
// independent of each other, so no workgroup ever waits for another one: no
// flags, no spinning, nothing persistent).  A line of n_pred new points, one
// row per level, is one launch.
#include "predict.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/nngp.h"
#include "device_common.h"
#include "graph_prep.h"
#include "kernels.h"

namespace nngp {
namespace {

constexpr int kPredictSmallRows = 128;  // levels up to this many rows are walked inside one workgroup
constexpr int kPredictBlockWaves = 16;  // waves of that workgroup

struct SolveDev {
  const int* nn;            // n_pred x b, compact numbering
  const double* linv;       // slots x n_pred x b
  const int* fslot;         // S: factor slot of each sample
  const double* sd;         // S: exp(log_scale / 2)
  const uint64_t* counter;  // S (Philox) or null: the normals are in V
  uint64_t seed;
  double* V;                // (n_support + n_pred) x SP
  int SP, S, n_support, n_pred, b;
};

// row r of sample s: V[n_support + r][s] holds z (injected normals) and receives y
__device__ __forceinline__ void predict_row(const SolveDev& a, int r, int s) {
  const int* nr = a.nn + (size_t)r * a.b;
  const double* lr = a.linv + ((size_t)a.fslot[s] * a.n_pred + r) * a.b;
  double acc = 0.0;
  for (int j = 1; j < a.b; ++j) {
    const int idx = nr[j];
    if (idx >= 0) acc = __builtin_fma(lr[j], a.V[(size_t)idx * a.SP + s], acc);
  }
  double* yp = a.V + (size_t)(a.n_support + r) * a.SP + s;
  const double z = a.counter ? normal_loc(a.seed, a.counter[s], (uint32_t)r) : *yp;
  *yp = __builtin_fma(a.sd[s], z, -acc) / lr[0];
}

// one level: wave w of the grid takes row rows[w / chunks] and samples
// 64 (w % chunks) + lane
__global__ __launch_bounds__(256) void predict_level_kernel(SolveDev a, const int* __restrict__ rows, int nrows,
                                                            int chunks) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)nrows * chunks) return;
  const int r = __builtin_amdgcn_readfirstlane(rows[w / chunks]);
  const int s = (int)(w % chunks) * 64 + (threadIdx.x & 63);
  if (s < a.S) predict_row(a, r, s);
}

// levels [lv0, lv1) (rows of level lv: rows[lptr[lv] .. lptr[lv+1])) for the
// 64 samples of chunk blockIdx.x: the waves of the workgroup share a level's
// rows, the barrier between levels replaces a launch
__global__ __launch_bounds__(64 * kPredictBlockWaves) void predict_levels_block_kernel(SolveDev a,
                                                                                     const int* __restrict__ rows,
                                                                                     const int* __restrict__ lptr,
                                                                                     int lv0, int lv1) {
  const int wave = threadIdx.x >> 6, s = blockIdx.x * 64 + (threadIdx.x & 63);
  for (int lv = lv0; lv < lv1; ++lv) {
    const int r0 = lptr[lv], cnt = lptr[lv + 1] - r0;
    if (s < a.S)
      for (int it = wave; it < cnt; it += kPredictBlockWaves)
        predict_row(a, __builtin_amdgcn_readfirstlane(rows[r0 + it]), s);
    __syncthreads();
  }
}

// dst[c * dst_pitch + r] = src[r * src_pitch + c] - (sub ? sub[r] : 0) for
// r < rows, c < cols: 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void predict_transpose_kernel(const double* __restrict__ src, long long src_pitch,
                                                                int rows, int cols, double* __restrict__ dst,
                                                                long long dst_pitch, const double* __restrict__ sub) {
  __shared__ double t[32][33];
  const int tiles_c = (cols + 31) / 32;
  const int r0 = (int)(blockIdx.x / tiles_c) * 32, c0 = (int)(blockIdx.x % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int q = ty; q < 32; q += 8) {
    const int r = r0 + q, c = c0 + tx;
    if (r < rows && c < cols) t[q][tx] = src[(size_t)r * src_pitch + c] - (sub ? sub[r] : 0.0);
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const int c = c0 + q, r = r0 + tx;
    if (r < rows && c < cols) dst[(size_t)c * dst_pitch + r] = t[tx][q];
  }
}

hipError_t launch_transpose(hipStream_t st, const double* src, long long src_pitch, int rows, int cols, double* dst,
                            long long dst_pitch, const double* sub) {
  const long long tiles = (long long)((rows + 31) / 32) * ((cols + 31) / 32);
  if (tiles < 1) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predict_transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, st, src, src_pitch, rows, cols,
                     dst, dst_pitch, sub);
  return hipGetLastError();
}

// every device object of a call; freed on every exit path
struct PredictDev {
  std::vector<void*> mem;
  void* pinned = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[3] = {};
  template <typename T>
  bool alloc(T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    mem.push_back(q);
    *p = static_cast<T*>(q);
    return true;
  }
  ~PredictDev() {
    for (void* q : mem) (void)hipFree(q);
    if (pinned) (void)hipHostFree(pinned);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};

}  // namespace

int predict_run(const PredictArgs& a, PredictStats* stats, std::string& err) {
  PredictStats ps;
  const auto t0 = std::chrono::steady_clock::now();
  PredictPlan P;
  if (!build_predict_plan(a.NNarray, a.n, a.n_pred, a.b, P, err)) return NNGP_ERR_ARG;
  const int n = a.n, n_pred = a.n_pred, b = a.b, d = a.d, ns = P.n_support;
  const size_t N = (size_t)n + n_pred, M = (size_t)ns + n_pred;
  // compact coordinates (row-major M x d): the support, then the new locations
  std::vector<double> locs_c(M * d);
  for (size_t c = 0; c < M; ++c) {
    const size_t src = c < (size_t)ns ? (size_t)P.support[c] : (size_t)n + (c - ns);
    for (int k = 0; k < d; ++k) locs_c[c * d + k] = a.locs[src + (size_t)k * N];
  }
  std::vector<int> row_loc(n_pred);
  for (int r = 0; r < n_pred; ++r) row_loc[r] = n + r;  // failures are reported as stacked rows
  // launches of the level schedule: runs of small levels [lv0, lv1) for the block kernel, or one large level
  struct Seg { int lv0, lv1; bool block; };
  std::vector<Seg> segs;
  for (int lv = 0; lv < P.n_levels;) {
    if (P.level_ptr[lv + 1] - P.level_ptr[lv] > kPredictSmallRows) {
      segs.push_back({lv, lv + 1, false});
      ++lv;
      continue;
    }
    int e = lv;
    while (e < P.n_levels && P.level_ptr[e + 1] - P.level_ptr[e] <= kPredictSmallRows) ++e;
    segs.push_back({lv, e, true});
    lv = e;
  }
  ps.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    err = "no HIP device";
    return NNGP_ERR_NODEV;
  }
  if (a.device >= ndev) {
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
  if (a.device >= 0 && (hipGetDevice(&restore.prev) != hipSuccess || restore.prev == a.device)) restore.prev = -1;
  hipError_t e = a.device < 0 ? hipSuccess : hipSetDevice(a.device);
  auto hip_fail = [&](const char* what) {
    err = std::string("predict_field: ") + what + ": " + hipGetErrorString(e);
    return NNGP_ERR_HIP;
  };
  if (e != hipSuccess) return hip_fail("hipSetDevice");

  const bool sphere = a.covfun == NNGP_EXPONENTIAL_SPHERE || a.covfun == NNGP_MATERN_SPHERE;
  const int ds = sphere ? 3 : (d <= 2 ? 2 : (d == 3 ? 3 : 4));
  // batch size (predict.h kPredictBudget): per sample the values (M), the
  // staged support values (ns) and the normals / output block (n_pred); per
  // distinct factor of a batch n_pred x b factor entries
  const size_t per_sample = sizeof(double) * (M + ns + n_pred), per_factor = sizeof(double) * (size_t)n_pred * b;
  const size_t fixed = sizeof(double) * M * (d + (size_t)kMaxChains * ds) + sizeof(int) * (size_t)n_pred * (b + 2);
  long long SB = a.sample_batch;
  if (SB == 0) {
    SB = 64;
    while (SB < a.n_samples) {
      const size_t nxt = (size_t)SB + 64;
      if (fixed + nxt * per_sample + std::min<size_t>(nxt, a.n_factors) * per_factor > kPredictBudget) break;
      SB = (long long)nxt;
    }
  }
  SB = std::min<long long>(SB, a.n_samples);
  const int SP = (int)((SB + 63) / 64 * 64);
  const int FC = (int)std::min<long long>(SB, a.n_factors);  // factor slots of a batch
  ps.sample_batch = (int)SB;

  PredictDev D;
  double *locs_d, *sc_d, *linv_d, *V_d, *w_d, *zo_d, *sd_d, *b0_d;
  int *nn_d, *rows_d, *lptr_d, *rloc_d, *fail_d, *fslot_d;
  uint64_t* ctr_d;
  if (!D.alloc(&locs_d, M * d) || !D.alloc(&sc_d, M * ds * kMaxChains) || !D.alloc(&linv_d, (size_t)FC * n_pred * b) ||
      !D.alloc(&V_d, M * SP) || !D.alloc(&w_d, (size_t)SB * ns) || !D.alloc(&zo_d, (size_t)SB * n_pred) ||
      !D.alloc(&sd_d, (size_t)SB) || !D.alloc(&b0_d, (size_t)SB) || !D.alloc(&nn_d, (size_t)n_pred * b) ||
      !D.alloc(&rows_d, (size_t)n_pred) || !D.alloc(&lptr_d, (size_t)P.n_levels + 1) ||
      !D.alloc(&rloc_d, (size_t)n_pred) || !D.alloc(&fail_d, (size_t)FC) || !D.alloc(&fslot_d, (size_t)SB) ||
      !D.alloc(&ctr_d, (size_t)SB)) {
    err = "predict_field: device allocation failed (smaller sample_batch?)";
    return NNGP_ERR_NOMEM;
  }
  if (hipHostMalloc(&D.pinned, sizeof(double) * std::max<size_t>((size_t)SB * ns, 1), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    D.pinned = nullptr;
    err = "predict_field: host staging allocation failed";
    return NNGP_ERR_NOMEM;
  }
  double* w_h = static_cast<double*>(D.pinned);
#define PREDICT_HIP(x)                        \
  do {                                        \
    e = (x);                                  \
    if (e != hipSuccess) return hip_fail(#x); \
  } while (0)
  PREDICT_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
  for (hipEvent_t& ev : D.ev) PREDICT_HIP(hipEventCreate(&ev));
  hipStream_t st = D.st;
  PREDICT_HIP(hipMemcpyAsync(locs_d, locs_c.data(), sizeof(double) * M * d, hipMemcpyHostToDevice, st));
  PREDICT_HIP(hipMemcpyAsync(nn_d, P.nn.data(), sizeof(int) * (size_t)n_pred * b, hipMemcpyHostToDevice, st));
  PREDICT_HIP(hipMemcpyAsync(rows_d, P.level_rows.data(), sizeof(int) * (size_t)n_pred, hipMemcpyHostToDevice, st));
  PREDICT_HIP(hipMemcpyAsync(lptr_d, P.level_ptr.data(), sizeof(int) * ((size_t)P.n_levels + 1), hipMemcpyHostToDevice, st));
  PREDICT_HIP(hipMemcpyAsync(rloc_d, row_loc.data(), sizeof(int) * (size_t)n_pred, hipMemcpyHostToDevice, st));
  PREDICT_HIP(hipStreamSynchronize(st));  // the host vectors above may go; batches reuse their own

  std::vector<int> slot_of(a.n_factors), slot_factor, fslot(SB), fail_h(FC);
  std::vector<double> sd(SB), b0(SB);
  std::vector<uint64_t> ctr(SB);
  for (long long s0 = 0; s0 < a.n_samples; s0 += SB) {
    const int S = (int)std::min<long long>(SB, a.n_samples - s0);
    // factor slots of the batch, in order of first use
    std::fill(slot_of.begin(), slot_of.end(), -1);
    slot_factor.clear();
    for (int si = 0; si < S; ++si) {
      const long long s = s0 + si;
      const int f = a.factor_of[s];
      if (slot_of[f] < 0) {
        slot_of[f] = (int)slot_factor.size();
        slot_factor.push_back(f);
      }
      fslot[si] = slot_of[f];
      sd[si] = std::exp(0.5 * a.log_scale[s]);
      b0[si] = a.beta0[s];
      if (!a.z) ctr[si] = a.counter[s];
      const double* row = a.fields + a.field_row[s] * a.field_pitch;
      double* dst = w_h + (size_t)si * ns;
      for (int c = 0; c < ns; ++c) dst[c] = row[P.support[c]];
    }
    const int F = (int)slot_factor.size();
    PREDICT_HIP(hipEventRecord(D.ev[0], st));
    PREDICT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fail_d), INT_MAX, F, st));
    for (int q = 0; q < F;) {
      const PredictFactor& f0 = a.factors[slot_factor[q]];
      if (sphere) {  // three scaled coordinates from d = 2: job by job, as nngp_factor
        PREDICT_HIP(launch_scale_coords(st, a.covfun, f0.cp, f0.ncp, locs_d, (int)M, d, sc_d, ds));
        PREDICT_HIP(launch_factor(st, f0.family, f0.var, f0.nugget, f0.nu, sc_d, ds, nn_d, n_pred, b,
                                  linv_d + (size_t)q * n_pred * b, fail_d + q, rloc_d));
        ++q;
        continue;
      }
      FactorJobs J;  // up to kMaxChains consecutive slots of one smoothness in one launch
      while (q + J.n_jobs < F && J.n_jobs < kMaxChains) {
        const PredictFactor& f = a.factors[slot_factor[q + J.n_jobs]];
        if (!(f.nu == f0.nu)) break;
        const int j = J.n_jobs++;
        for (int k = 0; k < 8; ++k) J.sa[j].c[k] = k < f.ncp ? f.cp[k] : 0.0;
        J.sa[j].covfun = a.covfun;
        J.var[j] = f.var;
        J.nugget[j] = f.nugget;
        J.sc[j] = sc_d + (size_t)j * M * ds;
        J.linv[j] = linv_d + (size_t)(q + j) * n_pred * b;
        J.fail[j] = fail_d + q + j;
      }
      J.row_loc = rloc_d;
      PREDICT_HIP(launch_factor_jobs(st, f0.family, f0.nu, J, locs_d, n_pred, d, ds, nn_d, b, (int)M));
      q += J.n_jobs;
    }
    PREDICT_HIP(hipEventRecord(D.ev[1], st));
    PREDICT_HIP(hipMemcpyAsync(fail_h.data(), fail_d, sizeof(int) * F, hipMemcpyDeviceToHost, st));
    PREDICT_HIP(hipMemcpyAsync(fslot_d, fslot.data(), sizeof(int) * S, hipMemcpyHostToDevice, st));
    PREDICT_HIP(hipMemcpyAsync(sd_d, sd.data(), sizeof(double) * S, hipMemcpyHostToDevice, st));
    PREDICT_HIP(hipMemcpyAsync(b0_d, b0.data(), sizeof(double) * S, hipMemcpyHostToDevice, st));
    if (!a.z) PREDICT_HIP(hipMemcpyAsync(ctr_d, ctr.data(), sizeof(uint64_t) * S, hipMemcpyHostToDevice, st));
    // y = field - beta_0 on the support, [support entry][sample]
    if (ns > 0) {
      PREDICT_HIP(hipMemcpyAsync(w_d, w_h, sizeof(double) * (size_t)S * ns, hipMemcpyHostToDevice, st));
      PREDICT_HIP(launch_transpose(st, w_d, ns, S, ns, V_d, SP, b0_d));
    }
    ps.staged_bytes += (long long)sizeof(double) * S * ns;
    if (a.z) {  // the normals into the new rows' values, which the solve replaces by y
      PREDICT_HIP(hipMemcpyAsync(zo_d, a.z + (size_t)s0 * n_pred, sizeof(double) * (size_t)S * n_pred,
                                 hipMemcpyHostToDevice, st));
      PREDICT_HIP(launch_transpose(st, zo_d, n_pred, S, n_pred, V_d + (size_t)ns * SP, SP, nullptr));
      ps.staged_bytes += (long long)sizeof(double) * S * n_pred;
    }
    SolveDev sv{nn_d, linv_d, fslot_d, sd_d, a.z ? nullptr : ctr_d, a.seed, V_d, SP, S, ns, n_pred, b};
    const int chunks = (S + 63) / 64;
    for (const Seg& g : segs) {
      if (g.block) {
        hipLaunchKernelGGL(predict_levels_block_kernel, dim3(chunks), dim3(64 * kPredictBlockWaves), 0, st, sv, rows_d,
                           lptr_d, g.lv0, g.lv1);
      } else {
        const int r0 = P.level_ptr[g.lv0], cnt = P.level_ptr[g.lv1] - r0;
        const long long waves = (long long)cnt * chunks;
        hipLaunchKernelGGL(predict_level_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, sv, rows_d + r0,
                           cnt, chunks);
      }
      PREDICT_HIP(hipGetLastError());
    }
    PREDICT_HIP(launch_transpose(st, V_d + (size_t)ns * SP, SP, n_pred, S, zo_d, n_pred, nullptr));
    PREDICT_HIP(hipMemcpyAsync(a.out + (size_t)s0 * n_pred, zo_d, sizeof(double) * (size_t)S * n_pred,
                               hipMemcpyDeviceToHost, st));
    PREDICT_HIP(hipEventRecord(D.ev[2], st));
    PREDICT_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    PREDICT_HIP(hipEventElapsedTime(&ms, D.ev[0], D.ev[1]));
    ps.factor_ms += ms;
    PREDICT_HIP(hipEventElapsedTime(&ms, D.ev[1], D.ev[2]));
    ps.solve_ms += ms;
    ++ps.n_batches;
    for (int si = 0; si < S; ++si)
      if (fail_h[fslot[si]] != INT_MAX) {
        if (a.fail_row) *a.fail_row = fail_h[fslot[si]];
        err = "predict_field: local covariance of stacked row " + std::to_string(fail_h[fslot[si]]) +
              " is not positive definite";
        return NNGP_ERR_CHOL;
      }
  }
#undef PREDICT_HIP
  if (stats) *stats = ps;
  return NNGP_OK;
}

}  // namespace nngp
