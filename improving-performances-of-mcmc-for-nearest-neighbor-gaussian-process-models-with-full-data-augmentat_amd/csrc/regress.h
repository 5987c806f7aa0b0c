// Launch wrappers of regress.hip: the array operations of the regression block
// (update_Gaussian.R:77-83,145-151,226-250) on a design matrix resident in the
// context (nngp_design_* of include/nngp.h).  Internal C++ header.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace nngp {

constexpr int kDesignLocsMax = 31;             // p_locs (interweaved columns)
constexpr int kDesignQMax = kDesignLocsMax + 1;  // columns of Xl1 = cbind(1, X[first_obs, locs])
constexpr int kRegRows = 4;                    // rows (observations) per thread and tile of a reduction pass
constexpr int kRegTile = kBlock * kRegRows;    // rows of one tile
constexpr int kRegBlocksMax = 1024;            // blocks of a reduction pass (tiles beyond: grid stride)

// Every reduction here is a fixed tree: a lane sums its kRegRows rows of a tile
// in row order, the wave's 64 lanes by shuffles, a wave adds its tiles in tile
// order into its own partial; reg_reduce then sums the partials of one value
// in a fixed order.  The grid depends on the row count only, and a chain's
// sums never meet another chain's: bitwise the same for every chain mask.
inline int reg_blocks(long long rows) {
  long long g = (rows + kRegTile - 1) / kRegTile;
  return (int)(g < 1 ? 1 : (g > kRegBlocksMax ? kRegBlocksMax : g));
}
inline int reg_parts(long long rows) { return reg_blocks(rows) * (kBlock / kWave); }

// the chains of one call (job m = chain J.chain[m])
struct RegJobs {
  int M = 0;
  int chain[kMaxChains] = {};
  double* field[kMaxChains] = {};       // device rows
  const double* linv[kMaxChains] = {};  // current factor
  double* sx[kMaxChains] = {};          // SX = B_cur Xl1: n x q column-major, device rows
  double* mu[kMaxChains] = {};
  double a[kMaxChains] = {};            // beta_0 (mean statistics, mu) or the shift (field passes)
  double b[kMaxChains] = {};            // beta_0 of mu in a commit
};

// Xl1[j*n + dpos[i]] = j == 0 ? 1 : X[cols[j-1]*n_obs + first_obs[i]] (0-based tables)
hipError_t launch_design_gather(hipStream_t st, int n, int n_obs, int q, const int* dpos, const int* first_obs,
                                const int* cols, const double* X, double* Xl1);
// partials of sum_i ((y[i] - field_m[lm[i]]) + a[m]) * cbind(1, X)[i, j], j = 0..p: value m*(p+1)+j
hipError_t launch_design_mean_stats(hipStream_t st, int n_obs, int p, const double* y, const int* lm,
                                    const double* X, const RegJobs& J, double* partials);
// res[slot[m]*res_stride + res_off + v] = the sum of the nparts partials of value m*nvals + v
struct RegSlots { int slot[kMaxChains]; };
hipError_t launch_reg_reduce(hipStream_t st, const double* partials, int nparts, int M, int nvals,
                             const RegSlots& s, int res_stride, int res_off, double* res);
// SX_m = B_m Xl1 for the jobs, every column in one pass over the rows (NNarray read once)
hipError_t launch_design_sx(hipStream_t st, const int* nn, int n, int b, int q, const double* Xl1, const RegJobs& J);
// partials of crossprod(SX_m): pairs (a, b >= a) in row-major order of the upper triangle, value m*npairs + pair
hipError_t launch_design_gram(hipStream_t st, int n, int q, const RegJobs& J, double* partials);
// other_m = (field_m + a[m]) + Xl bl_m  (columns in order; bl_m = coef + chain*(q-1)); oth: job m at oth + m*n
hipError_t launch_design_other(hipStream_t st, int n, int q, const double* Xl1, const RegJobs& J, const double* bl,
                               double* oth);
// bo_m = B_m other_m (job m at bo + m*n)
hipError_t launch_design_spmv(hipStream_t st, const int* nn, int n, int b, const RegJobs& J, const double* oth,
                              double* bo);
// partials of crossprod(bo_m, SX_m): value m*q + j
hipError_t launch_design_tstats(hipStream_t st, int n, int q, const RegJobs& J, const double* bo, double* partials);
// field_m = ((field_m + a[m]) + Xl bl_old_m) - Xl bl_new_m
hipError_t launch_design_field(hipStream_t st, int n, int q, const double* Xl1, const RegJobs& J,
                               const double* bl_old, const double* bl_new);
// mu_m = b[m] + X beta_m  (beta_m = beta + chain*p; X read once for all jobs)
hipError_t launch_design_mu(hipStream_t st, int n_obs, int p, const double* X, const RegJobs& J, const double* beta);

}  // namespace nngp
