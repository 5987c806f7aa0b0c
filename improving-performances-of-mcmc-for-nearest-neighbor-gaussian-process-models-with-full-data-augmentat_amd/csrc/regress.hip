// Regression block of mcmc_nngp_update_Gaussian on the device
// (update_Gaussian.R:77-83,145-151,226-250): crossprod(residual, cbind(1, X)),
// the interweaved statistics crossprod(B other, B Xl1) with their Gram matrix,
// and the field / mu updates that follow the host's draws.  Bandwidth-bound
// fp64 passes: lanes run across observations or rows and the columns are the
// outer loop, so the column-major X, Xl1 and SX are read coalesced; X is read
// once for all chains of a call, the NNarray once for all columns.
#include "regress.h"

namespace nngp {
namespace {

__device__ __forceinline__ double reg_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// the wave's partial of one value: tile sums added in tile order
__device__ __forceinline__ void reg_put(double* p, double s, bool first) { *p = first ? s : *p + s; }

__global__ __launch_bounds__(256) void design_gather_kernel(int n, int n_obs, int q, const int* __restrict__ dpos,
                                                            const int* __restrict__ first_obs,
                                                            const int* __restrict__ cols,
                                                            const double* __restrict__ X, double* __restrict__ Xl1) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int row = dpos[i], o = first_obs[i];
    Xl1[row] = 1.0;
    for (int j = 1; j < q; ++j) Xl1[(size_t)j * n + row] = X[(size_t)cols[j - 1] * n_obs + o];
  }
}

__global__ __launch_bounds__(256) void design_mean_stats_kernel(int n_obs, int p, const double* __restrict__ y,
                                                                const int* __restrict__ lm,
                                                                const double* __restrict__ X, RegJobs J,
                                                                double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int nparts = gridDim.x * (kBlock / kWave);
  const int gw = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  bool first = true;
  for (long long base = (long long)blockIdx.x * kRegTile; base < n_obs; base += (long long)gridDim.x * kRegTile) {
    double res[kMaxChains][kRegRows];
    long long obs[kRegRows];
    bool ok[kRegRows];
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) {
      obs[r] = base + r * kBlock + threadIdx.x;
      ok[r] = obs[r] < n_obs;
      const int loc = ok[r] ? lm[obs[r]] : 0;
      const double yv = ok[r] ? y[obs[r]] : 0.0;
#pragma unroll
      for (int m = 0; m < kMaxChains; ++m)
        res[m][r] = (m < J.M && ok[r]) ? (yv - J.field[m][loc]) + J.a[m] : 0.0;
    }
    for (int j = 0; j <= p; ++j) {
      double xv[kRegRows];
#pragma unroll
      for (int r = 0; r < kRegRows; ++r)
        xv[r] = j == 0 ? 1.0 : (ok[r] ? X[(size_t)(j - 1) * n_obs + obs[r]] : 0.0);
#pragma unroll
      for (int m = 0; m < kMaxChains; ++m) {
        if (m >= J.M) continue;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < kRegRows; ++r) s += res[m][r] * xv[r];
        s = reg_wave_sum(s);
        if (lane == 0) reg_put(partials + ((size_t)m * (p + 1) + j) * nparts + gw, s, first);
      }
    }
    first = false;
  }
}

__global__ __launch_bounds__(256) void reg_reduce_kernel(const double* __restrict__ partials, int nparts, int nvals,
                                                         RegSlots S, int res_stride, int res_off,
                                                         double* __restrict__ res) {
  __shared__ double sm[kBlock / kWave];
  const int m = blockIdx.x / nvals, v = blockIdx.x % nvals;
  const double* pv = partials + (size_t)blockIdx.x * nparts;
  double acc = 0.0;
  for (int q = threadIdx.x; q < nparts; q += blockDim.x) acc += pv[q];
  acc = reg_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) res[(size_t)S.slot[m] * res_stride + res_off + v] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// G lanes per row (G >= b): lane g holds entry g of the row, as row_stats_kernel
template <int G>
__global__ __launch_bounds__(256) void design_sx_kernel(const int* __restrict__ nn, int n, int b, int q,
                                                        const double* __restrict__ Xl1, RegJobs J) {
  const int g = threadIdx.x & (G - 1);
  const int rows_per_grid = gridDim.x * (blockDim.x / G);
  for (int k = blockIdx.x * (blockDim.x / G) + threadIdx.x / G; k < n; k += rows_per_grid) {
    const int idx = g < b ? nn[(size_t)k * b + g] : -1;
    double l[kMaxChains];
#pragma unroll
    for (int m = 0; m < kMaxChains; ++m) l[m] = (m < J.M && idx >= 0) ? J.linv[m][(size_t)k * b + g] : 0.0;
    for (int j = 0; j < q; ++j) {
      const double xv = idx >= 0 ? (j == 0 ? 1.0 : Xl1[(size_t)j * n + idx]) : 0.0;
#pragma unroll
      for (int m = 0; m < kMaxChains; ++m) {
        if (m >= J.M) continue;
        double u = l[m] * xv;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) u += __shfl_xor(u, off, 64);
        if (g == 0) J.sx[m][(size_t)j * n + k] = u;
      }
    }
  }
}

template <int G>
__global__ __launch_bounds__(256) void design_spmv_kernel(const int* __restrict__ nn, int n, int b, RegJobs J,
                                                          const double* __restrict__ oth, double* __restrict__ bo) {
  const int g = threadIdx.x & (G - 1);
  const int rows_per_grid = gridDim.x * (blockDim.x / G);
  for (int k = blockIdx.x * (blockDim.x / G) + threadIdx.x / G; k < n; k += rows_per_grid) {
    const int idx = g < b ? nn[(size_t)k * b + g] : -1;
#pragma unroll
    for (int m = 0; m < kMaxChains; ++m) {
      if (m >= J.M) continue;
      double u = idx >= 0 ? J.linv[m][(size_t)k * b + g] * oth[(size_t)m * n + idx] : 0.0;
#pragma unroll
      for (int off = 1; off < G; off <<= 1) u += __shfl_xor(u, off, 64);
      if (g == 0) bo[(size_t)m * n + k] = u;
    }
  }
}

// blockIdx.y = job.  Column a of a tile stays in registers while the columns
// b >= a stream past it (a tile's columns come back from the L2)
__global__ __launch_bounds__(256) void design_gram_kernel(int n, int q, RegJobs J, double* __restrict__ partials) {
  const int lane = threadIdx.x & 63, m = blockIdx.y;
  const int nparts = gridDim.x * (kBlock / kWave);
  const int gw = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const int npairs = q * (q + 1) / 2;
  const double* __restrict__ sx = J.sx[m];
  bool first = true;
  for (long long base = (long long)blockIdx.x * kRegTile; base < n; base += (long long)gridDim.x * kRegTile) {
    long long row[kRegRows];
    bool ok[kRegRows];
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) {
      row[r] = base + r * kBlock + threadIdx.x;
      ok[r] = row[r] < n;
    }
    int pair = 0;
    for (int a = 0; a < q; ++a) {
      double va[kRegRows];
#pragma unroll
      for (int r = 0; r < kRegRows; ++r) va[r] = ok[r] ? sx[(size_t)a * n + row[r]] : 0.0;
      for (int c = a; c < q; ++c, ++pair) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < kRegRows; ++r) s += va[r] * (ok[r] ? sx[(size_t)c * n + row[r]] : 0.0);
        s = reg_wave_sum(s);
        if (lane == 0) reg_put(partials + ((size_t)m * npairs + pair) * nparts + gw, s, first);
      }
    }
    first = false;
  }
}

__global__ __launch_bounds__(256) void design_tstats_kernel(int n, int q, RegJobs J, const double* __restrict__ bo,
                                                            double* __restrict__ partials) {
  const int lane = threadIdx.x & 63, m = blockIdx.y;
  const int nparts = gridDim.x * (kBlock / kWave);
  const int gw = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const double* __restrict__ sx = J.sx[m];
  bool first = true;
  for (long long base = (long long)blockIdx.x * kRegTile; base < n; base += (long long)gridDim.x * kRegTile) {
    long long row[kRegRows];
    bool ok[kRegRows];
    double u[kRegRows];
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) {
      row[r] = base + r * kBlock + threadIdx.x;
      ok[r] = row[r] < n;
      u[r] = ok[r] ? bo[(size_t)m * n + row[r]] : 0.0;
    }
    for (int j = 0; j < q; ++j) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < kRegRows; ++r) s += u[r] * (ok[r] ? sx[(size_t)j * n + row[r]] : 0.0);
      s = reg_wave_sum(s);
      if (lane == 0) reg_put(partials + ((size_t)m * q + j) * nparts + gw, s, first);
    }
    first = false;
  }
}

// (field + shift) + Xl bl, the column sum in column order (update_Gaussian.R:233,240)
__device__ __forceinline__ double design_other(const double* __restrict__ Xl1, int n, int q, int row, double f,
                                               double shift, const double* __restrict__ bl) {
  double s = 0.0;
  for (int j = 1; j < q; ++j) s += Xl1[(size_t)j * n + row] * bl[j - 1];
  return (f + shift) + s;
}

__global__ __launch_bounds__(256) void design_other_kernel(int n, int q, const double* __restrict__ Xl1, RegJobs J,
                                                           const double* __restrict__ bl, double* __restrict__ oth) {
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gridDim.x * blockDim.x)
#pragma unroll
    for (int m = 0; m < kMaxChains; ++m) {
      if (m >= J.M) continue;
      oth[(size_t)m * n + row] =
          design_other(Xl1, n, q, row, J.field[m][row], J.a[m], bl + (size_t)J.chain[m] * (q - 1));
    }
}

__global__ __launch_bounds__(256) void design_field_kernel(int n, int q, const double* __restrict__ Xl1, RegJobs J,
                                                           const double* __restrict__ bl_old,
                                                           const double* __restrict__ bl_new) {
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gridDim.x * blockDim.x)
#pragma unroll
    for (int m = 0; m < kMaxChains; ++m) {
      if (m >= J.M) continue;
      const size_t off = (size_t)J.chain[m] * (q - 1);
      const double other = design_other(Xl1, n, q, row, J.field[m][row], J.a[m], bl_old + off);
      double s = 0.0;
      for (int j = 1; j < q; ++j) s += Xl1[(size_t)j * n + row] * bl_new[off + j - 1];
      J.field[m][row] = other - s;
    }
}

__global__ __launch_bounds__(256) void design_mu_kernel(int n_obs, int p, const double* __restrict__ X, RegJobs J,
                                                        const double* __restrict__ beta) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_obs; i += gridDim.x * blockDim.x) {
    double acc[kMaxChains] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < p; ++j) {
      const double xv = X[(size_t)j * n_obs + i];
#pragma unroll
      for (int m = 0; m < kMaxChains; ++m)
        if (m < J.M) acc[m] += xv * beta[(size_t)J.chain[m] * p + j];
    }
#pragma unroll
    for (int m = 0; m < kMaxChains; ++m)
      if (m < J.M) J.mu[m][i] = J.b[m] + acc[m];
  }
}

int elementwise_blocks(long long rows) {
  long long g = (rows + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

int row_group(int b) { return b <= 4 ? 4 : b <= 8 ? 8 : b <= 16 ? 16 : 32; }

int row_group_blocks(int n, int G) {
  const long long rows_per_block = kBlock / G;
  long long g = (n + rows_per_block - 1) / rows_per_block;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

hipError_t launch_design_gather(hipStream_t st, int n, int n_obs, int q, const int* dpos, const int* first_obs,
                                const int* cols, const double* X, double* Xl1) {
  hipLaunchKernelGGL(design_gather_kernel, dim3(elementwise_blocks(n)), dim3(kBlock), 0, st, n, n_obs, q, dpos,
                     first_obs, cols, X, Xl1);
  return hipGetLastError();
}

hipError_t launch_design_mean_stats(hipStream_t st, int n_obs, int p, const double* y, const int* lm,
                                    const double* X, const RegJobs& J, double* partials) {
  hipLaunchKernelGGL(design_mean_stats_kernel, dim3(reg_blocks(n_obs)), dim3(kBlock), 0, st, n_obs, p, y, lm, X, J,
                     partials);
  return hipGetLastError();
}

hipError_t launch_reg_reduce(hipStream_t st, const double* partials, int nparts, int M, int nvals,
                             const RegSlots& s, int res_stride, int res_off, double* res) {
  hipLaunchKernelGGL(reg_reduce_kernel, dim3(M * nvals), dim3(kBlock), 0, st, partials, nparts, nvals, s, res_stride,
                     res_off, res);
  return hipGetLastError();
}

hipError_t launch_design_sx(hipStream_t st, const int* nn, int n, int b, int q, const double* Xl1,
                            const RegJobs& J) {
  const int G = row_group(b), g = row_group_blocks(n, G);
  switch (G) {
    case 4: hipLaunchKernelGGL(design_sx_kernel<4>, dim3(g), dim3(kBlock), 0, st, nn, n, b, q, Xl1, J); break;
    case 8: hipLaunchKernelGGL(design_sx_kernel<8>, dim3(g), dim3(kBlock), 0, st, nn, n, b, q, Xl1, J); break;
    case 16: hipLaunchKernelGGL(design_sx_kernel<16>, dim3(g), dim3(kBlock), 0, st, nn, n, b, q, Xl1, J); break;
    default: hipLaunchKernelGGL(design_sx_kernel<32>, dim3(g), dim3(kBlock), 0, st, nn, n, b, q, Xl1, J); break;
  }
  return hipGetLastError();
}

hipError_t launch_design_gram(hipStream_t st, int n, int q, const RegJobs& J, double* partials) {
  hipLaunchKernelGGL(design_gram_kernel, dim3(reg_blocks(n), J.M), dim3(kBlock), 0, st, n, q, J, partials);
  return hipGetLastError();
}

hipError_t launch_design_other(hipStream_t st, int n, int q, const double* Xl1, const RegJobs& J, const double* bl,
                               double* oth) {
  hipLaunchKernelGGL(design_other_kernel, dim3(elementwise_blocks(n)), dim3(kBlock), 0, st, n, q, Xl1, J, bl, oth);
  return hipGetLastError();
}

hipError_t launch_design_spmv(hipStream_t st, const int* nn, int n, int b, const RegJobs& J, const double* oth,
                              double* bo) {
  const int G = row_group(b), g = row_group_blocks(n, G);
  switch (G) {
    case 4: hipLaunchKernelGGL(design_spmv_kernel<4>, dim3(g), dim3(kBlock), 0, st, nn, n, b, J, oth, bo); break;
    case 8: hipLaunchKernelGGL(design_spmv_kernel<8>, dim3(g), dim3(kBlock), 0, st, nn, n, b, J, oth, bo); break;
    case 16: hipLaunchKernelGGL(design_spmv_kernel<16>, dim3(g), dim3(kBlock), 0, st, nn, n, b, J, oth, bo); break;
    default: hipLaunchKernelGGL(design_spmv_kernel<32>, dim3(g), dim3(kBlock), 0, st, nn, n, b, J, oth, bo); break;
  }
  return hipGetLastError();
}

hipError_t launch_design_tstats(hipStream_t st, int n, int q, const RegJobs& J, const double* bo, double* partials) {
  hipLaunchKernelGGL(design_tstats_kernel, dim3(reg_blocks(n), J.M), dim3(kBlock), 0, st, n, q, J, bo, partials);
  return hipGetLastError();
}

hipError_t launch_design_field(hipStream_t st, int n, int q, const double* Xl1, const RegJobs& J,
                               const double* bl_old, const double* bl_new) {
  hipLaunchKernelGGL(design_field_kernel, dim3(elementwise_blocks(n)), dim3(kBlock), 0, st, n, q, Xl1, J, bl_old,
                     bl_new);
  return hipGetLastError();
}

hipError_t launch_design_mu(hipStream_t st, int n_obs, int p, const double* X, const RegJobs& J, const double* beta) {
  hipLaunchKernelGGL(design_mu_kernel, dim3(elementwise_blocks(n_obs)), dim3(kBlock), 0, st, n_obs, p, X, J, beta);
  return hipGetLastError();
}

}  // namespace nngp
