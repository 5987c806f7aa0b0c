/*
 * nngp.h -- C ABI of the MI355X-native NNGP chromatic-Gibbs hot path.
 *
 * Drop-in boundary for the reference's L1/L0 calls on the hot path (SURVEY.md
 * §8b).  Plain pointers and sizes only; no torch / C++ types cross it.  All
 * host arrays use R's conventions: matrices column-major, indices 1-based,
 * NA_integer_ == INT_MIN.  Every entry point returns 0 (NNGP_OK) or an
 * nngp_status; a context keeps the message of its last error
 * (nngp_ctx_last_error).  Host inputs are read-only for the call; outputs are
 * caller-allocated.  Device state is owned by the context and freed only by
 * nngp_ctx_destroy.  Calls on one context are serialised by the caller;
 * distinct contexts may live on distinct devices.  HIP is initialised lazily
 * by nngp_ctx_create: never fork() after it.  A context holds 1..4 MCMC chains
 * over the same locations / NNarray / colouring (replaces the per-chain
 * workers of parallel::mclapply, Scripts/mcmc_nngp_update_Gaussian.R:25-26):
 * per-chain entry points act on the chain chosen by nngp_set_chain, and
 * nngp_sweep_chains sweeps all chains of the context in the same kernels.
 *
 * Reference interface each entry point replaces (path:line under the
 * reference tree):
 *   nngp_order_maxmin ........ GpGp::order_maxmin, Scripts/mcmc_nngp_initialize.R:29
 *   nngp_find_ordered_nn ..... GpGp::find_ordered_nn, Scripts/mcmc_nngp_initialize.R:93
 *   nngp_greedy_coloring ..... moral graph Scripts/mcmc_nngp_initialize.R:97-109 +
 *                              naive_greedy_coloring Scripts/Coloring.R:2-20
 *   nngp_factor .............. GpGp::vecchia_Linv + Matrix::sparseMatrix,
 *                              Scripts/mcmc_nngp_update_Gaussian.R:72-73,123-124,179-180
 *   nngp_accept_factor ....... precision_diag refresh, update_Gaussian.R:140-142,195-197
 *   nngp_loglik .............. ll_compressed_sparse_chol (+GpGp::Linv_mult),
 *                              Scripts/mcmc_nngp_update_Gaussian.R:8-12,184-186
 *   nngp_set_mu .............. mu + residuals_sum, update_Gaussian.R:85-90,249-250,260
 *   nngp_sweep ............... chromatic sampling, update_Gaussian.R:257-275
 *   nngp_sweep_chains ........ the same for every chain (mclapply over chains,
 *                              update_Gaussian.R:25-26, around :257-275)
 *   nngp_ancillary_propose ... new_field, update_Gaussian.R:127 (SpMV + sparse
 *                              triangular solve); _chains: every chain at once
 *   nngp_field_response_ratio  dnorm ratio, update_Gaussian.R:129-131
 *   nngp_beta0_stats ......... beta_0 Gibbs block, update_Gaussian.R:221-222
 *   nngp_sum_squared_residuals update_Gaussian.R:281
 *   nngp_record_field ........ records$field[i, ] = field, update_Gaussian.R:305-311
 *   nngp_records_stream ...... records$field in host memory while the chain runs (same lines)
 *   nngp_summary ............. get_summary, Scripts/mcmc_nngp_estimate.R:1-6 (res$field,
 *                              estimate.R:88-94; predicted_field_summary, predict.R:57-58)
 *   nngp_summary_probs ....... the same with chosen quantiles and exceedance probabilities
 *   nngp_effects_summary ..... beta_matrix[, subset] %*% t(X_pred) and its get_summary,
 *                              Scripts/mcmc_nngp_predict.R:92-102, the samples generated on the device
 *   nngp_pointwise_loglik .... the dnorm terms of update_Gaussian.R:130-131,281 per saved sample
 *                              and observation, reduced to WAIC / LPML / DIC / PIT ingredients
 *   nngp_field_diag .......... Individual_PSRF of Gelman_Rubin_Brooks and ESS,
 *                              Scripts/mcmc_nngp_diagnose.R:1-24,107-118, per field location
 *   nngp_predict_field ....... the per-sample body of mcmc_nngp_predict_field,
 *                              Scripts/mcmc_nngp_predict.R:39-53, for all samples of a chain
 *   nngp_design_set .......... X, X$locs and beta_interweaved_* kept for the call,
 *                              Scripts/mcmc_nngp_update_Gaussian.R:77-83,145-151
 *   nngp_design_mean_stats_chains      crossprod(y - field[locs_match] + beta_0, cbind(1, X)),
 *                              update_Gaussian.R:230
 *   nngp_design_interweave_stats_chains  crossprod(sparse_chol %*% other, sparse_chol_X) and
 *                              beta_interweaved_precision, update_Gaussian.R:79,240-241
 *   nngp_design_commit_chains  the field and mu updates, update_Gaussian.R:233,240,245,249
 *   nngp_spmv / nngp_tri_solve sparse_chol %*% X (update_Gaussian.R:79,147) /
 *                              Matrix::solve (initialize.R:208, predict.R:46)
 */
#ifndef NNGP_H_
#define NNGP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_ABI_VERSION 14  /* 14: nngp_tri_rescues (+ nngp_summary, nngp_summary_probs, nngp_summary_stats, nngp_effects_summary, nngp_effects_stats, nngp_field_diag, nngp_field_diag_stats, nngp_predict_field, nngp_predict_stats, nngp_design_set, nngp_design_mean_stats_chains, nngp_design_interweave_stats_chains, nngp_design_commit_chains, nngp_get_mu, nngp_pointwise_loglik, nngp_pointwise_loglik_stats: additive, same version); 13: nngp_records_stream; 12: nngp_info gained tile_rows_needed, device_lds */
#define NNGP_SHARD_ID_BYTES 128 /* RCCL unique id */
#define NNGP_IPC_HANDLE_BYTES 192 /* HIP IPC handles of a tile shard's granule buffer, w replica, flags */

typedef enum {
  NNGP_OK = 0,
  NNGP_ERR_ARG = 1,     /* invalid argument / shape */
  NNGP_ERR_HIP = 2,     /* HIP runtime error (message in the context) */
  NNGP_ERR_CHOL = 3,    /* local covariance not positive definite */
  NNGP_ERR_STATE = 4,   /* call out of order (e.g. sweep before factor) */
  NNGP_ERR_NOMEM = 5,   /* host or device allocation failed */
  NNGP_ERR_NODEV = 6,   /* no HIP device available */
  NNGP_ERR_COMM = 7     /* RCCL error */
} nngp_status;

/* Covariance functions (GpGp names; covparms = c(variance, shape..., nugget)). */
typedef enum {
  NNGP_EXPONENTIAL_ISOTROPIC = 0, /* (var, range, nugget)                */
  NNGP_EXPONENTIAL_SPHERE = 1,    /* (var, range[Earth radii], nugget)   */
  NNGP_EXPONENTIAL_SCALEDIM = 2,  /* (var, range_1..range_d, nugget)     */
  NNGP_EXPONENTIAL_SPACETIME = 3, /* (var, range_space, range_time, nug) */
  NNGP_MATERN_ISOTROPIC = 4,      /* (var, range, smoothness, nugget)    */
  NNGP_MATERN_SPHERE = 5,         /* (var, range, smoothness, nugget)    */
  NNGP_MATERN_SCALEDIM = 6,       /* (var, range_1..range_d, smooth, nug)*/
  NNGP_MATERN_SPACETIME = 7,      /* (var, r_space, r_time, smooth, nug) */
  NNGP_MATERN15_ISOTROPIC = 8     /* (var, range, nugget); extension     */
} nngp_covfun;

typedef struct nngp_ctx nngp_ctx;

typedef struct {
  int n;           /* locations */
  int b;           /* m + 1 */
  int d;           /* coordinate dimension */
  int n_obs;       /* observations */
  int n_colors;    /* K */
  int n_levels;    /* depth of the Vecchia DAG (triangular solve) */
  long long nnz;   /* nonzeros of B */
  long long n_entries; /* sliced-ELL entries incl. padding */
  int max_collen;  /* longest column of B */
  int device;      /* HIP device ordinal */
  int n_chains;    /* chains held by the context */
  int lanes_per_chain; /* sweep lanes of one chain in a wavefront (64/32/16) */
  int n_chunks;    /* sweep chunks (wavefront tasks per chain and sweep) */
  int sweep_engine;  /* 0: one launch per colour, 1: tile-resident persistent sweep */
  int n_tiles;       /* tiles (persistent workgroups) of the tile engine */
  int tile_rows_max; /* max local rows (own + foreign) of a tile: its resident r */
  long long n_ghost_cells; /* foreign-member cells the tiles (or shard ranks) apply after a hand-off */
  int n_ranks;       /* shard contexts: ranks of the sharded sweep (0: not sharded);
                        sweep_engine 0: colour shard, 1: tile shard */
  int rank;          /* shard contexts: this context's rank */
  long long shard_owned;          /* locations swept by this rank */
  long long shard_needed_rows;    /* rows of B its columns touch (its r halo included) */
  long long shard_exchange_slots; /* colour shard: slots of all colours' exchange regions (padded);
                                     tile shard: locations whose draws other ranks read */
  int tile_ghost_pass;       /* tile engine: ghost cells a (tile, colour) applies per register pass */
  int tile_ghost_cells_max;  /* tile engine: most ghost cells of one (tile, colour) */
  int tile_r_global;         /* tile engine: 1 = the tiles' r in global memory (layout beyond the LDS) */
  int tile_chain_split;      /* always 0: the chain-split tile launches were removed (the field keeps the layout) */
  int tile_resident_per_cu;  /* tile engine: workgroups of its kernel resident per CU at once (occupancy query);
                                the persistent launch needs tiles <= this x CUs, else the colour engine runs */
  int engine_fallback;       /* why not the tile engine: 0 = it runs, 1 = layout unsuitable (LDS, shape),
                                2 = residency (more tile workgroups than fit the device at once),
                                3 = NNGP_ENGINE=colors / more ranks than the tile shard takes */
  int tile_exchange_wave;    /* tile engine: 1 = the last wave of each tile polls the hand-offs (NT - 64 cell threads) */
  int device_cus;            /* compute units of the context's device */
  int tile_rows_needed;      /* largest local-row count of a tile in the tile layout built for this context
                                (also when the tile engine was not used or keeps r in global memory; 0: none built) */
  int device_lds;            /* LDS bytes per CU of the context's device */
} nngp_info;

/* ---------- library ---------- */
int nngp_abi_version(void);
const char* nngp_status_string(int status);

/* ---------- host-side graph preparation (init-time, C++) ---------- */
/* locs: n x d column-major.  order: 1-based permutation (length n). */
int nngp_order_maxmin(const double* locs, int n, int d, int* order);
/* NNarray: n x (m+1) column-major, 1-based, NA = INT_MIN. Exact NN on the raw
 * coordinates, ties broken by the smaller index. */
int nngp_find_ordered_nn(const double* locs, int n, int d, int m, int* NNarray);
/* coloring: length n, 1-based colours; *n_colors = K. */
int nngp_greedy_coloring(const int* NNarray, int n, int b, int* coloring, int* n_colors);

/* ---------- device context ---------- */
/* locs n x d col-major (ordered); NNarray n x b col-major 1-based (NA=INT_MIN);
 * coloring 1-based (length n); locs_match 1-based (length n_obs);
 * observed_field length n_obs; n_chains 1..4 (chain 0 selected).
 * device: HIP ordinal (-1: current). */
int nngp_ctx_create(const double* locs, int n, int d, const int* NNarray, int b,
                    const int* coloring, const int* locs_match,
                    const double* observed_field, int n_obs, int n_chains, int device,
                    nngp_ctx** out);
/* select the chain (0-based) the per-chain entry points below act on */
int nngp_set_chain(nngp_ctx* ctx, int chain);
void nngp_ctx_destroy(nngp_ctx* ctx);
const char* nngp_ctx_last_error(const nngp_ctx* ctx);
int nngp_ctx_info(const nngp_ctx* ctx, nngp_info* info);
/* one line: the sweep engine chosen at creation and why (e.g. the residency
 * or LDS reason the tile engine was not used); owned by the context */
const char* nngp_ctx_engine_note(const nngp_ctx* ctx);

/* Vecchia factor (A4).  which: 0 = current factor, 1 = proposal. */
int nngp_factor(nngp_ctx* ctx, int which, int covfun, const double* covparms, int ncovparms);
/* copy a factor out as GpGp's Linv (n x b column-major, unfilled entries 0) */
int nngp_get_linv(nngp_ctx* ctx, int which, double* Linv);
/* upload an externally computed Linv (n x b col-major) into `which` */
int nngp_set_linv(nngp_ctx* ctx, int which, const double* Linv);
/* proposal factor becomes current; refreshes the sweep values + precision_diag (A5) */
int nngp_accept_factor(nngp_ctx* ctx);
/* precision_diag = colSums(B o B) of the current factor (length n) */
int nngp_get_precision_diag(nngp_ctx* ctx, double* D);

/* latent field (length n, location order) */
int nngp_set_field(nngp_ctx* ctx, const double* field);
int nngp_get_field(nngp_ctx* ctx, double* field);
/* mu (length n_obs): beta_0 + X beta; recomputes residuals_sum (A7).
 * mu == NULL means mu = beta0 for every observation. */
int nngp_set_mu(nngp_ctx* ctx, const double* mu, double beta0);

/* On-device field records (records$field, update_Gaussian.R:56,305-311 with
 * field_thinning): the selected chain's device buffer of n_rows
 * x n (location order); record_field copies the current field into row `row`
 * without a host round trip; get_records copies rows [row0, row0+n_rows) out
 * (row-major n_rows x n).  reserve(0) frees the buffer. */
int nngp_records_reserve(nngp_ctx* ctx, int n_rows);
int nngp_record_field(nngp_ctx* ctx, int row);
int nngp_get_records(nngp_ctx* ctx, int row0, int n_rows, double* out);
/* Streams the selected chain's recorded rows into a caller-owned host array
 * (n_rows x n row-major, n_rows = the reserved rows) as they are recorded: a
 * worker thread copies each row behind the stream while the chain runs, and
 * nngp_get_records(ctx, row0, k, host + row0 * n) only waits for them (rows
 * not recorded since the binding are copied from the device there).  The
 * array must stay valid until that get_records, the next records_reserve,
 * nngp_records_stream(ctx, NULL, 0) or nngp_ctx_destroy, which all end the
 * binding (after the rows in flight have landed).  A call that fails leaves
 * an existing binding in place. */
int nngp_records_stream(nngp_ctx* ctx, double* host, int n_rows);

/* Vecchia log-likelihood (A6) of z = field - beta0 under factor `which` */
int nngp_loglik(nngp_ctx* ctx, int which, double beta0, double log_scale, double* ll);

/* n_sweeps chromatic sweeps (A1).  Normals: Philox4x32-10 with key = seed,
 * counter = (location, counter_base + sweep, 0x5EED) unless z != NULL, in which
 * case z (n_sweeps x n row-major, z[s*n + i]) supplies them.  Stream-ordered:
 * the call may return before the sweeps have run (the only tile context of a
 * device; NNGP_SWEEP_SYNC=1 waits); every entry point that hands results to
 * the host waits for them, and reports a tile timeout of an earlier sweep. */
int nngp_sweep(nngp_ctx* ctx, int n_sweeps, double beta0, double log_scale,
               double log_noise_variance, uint64_t seed, uint64_t counter_base,
               const double* z);

/* n_sweeps sweeps of EVERY chain of the context in the same kernels; arrays
 * of length n_chains.  Chain k's result is bitwise identical to nngp_sweep on
 * chain k alone with the same arguments. */
int nngp_sweep_chains(nngp_ctx* ctx, int n_sweeps, const double* beta0, const double* log_scale,
                      const double* log_noise_variance, const uint64_t* seed,
                      const uint64_t* counter_base);

/* Ancillary proposal: proposal field = beta0 + exp(0.5*dlog_scale) *
 * B_prop^{-1} (B_cur (field - beta0)) (update_Gaussian.R:127). */
int nngp_ancillary_propose(nngp_ctx* ctx, double beta0, double dlog_scale);
/* nngp_ancillary_propose for the chains in chain_mask (bit k = chain k) in
 * the same kernels (one triangular-solve schedule for all of them); beta0 and
 * dlog_scale have n_chains entries (others ignored).  Chain k's proposal is
 * bitwise identical to nngp_ancillary_propose on chain k alone. */
int nngp_ancillary_propose_chains(nngp_ctx* ctx, int chain_mask, const double* beta0,
                                  const double* dlog_scale);
/* sum dnorm(y | proposal) - sum dnorm(y | field), sd = exp(lnv/2) (A8) */
int nngp_field_response_ratio(nngp_ctx* ctx, double beta0, double log_noise_variance,
                              double* ratio);
/* proposal field becomes current */
int nngp_accept_field(nngp_ctx* ctx);
/* 1'B'B1 and 1'B'B field (current factor) -- beta_0 Gibbs (update_Gaussian.R:221-222) */
int nngp_beta0_stats(nngp_ctx* ctx, double* ones_Q_ones, double* ones_Q_field);
/* sum (y - field[loc] - mu + beta0)^2 (update_Gaussian.R:281) */
int nngp_sum_squared_residuals(nngp_ctx* ctx, double beta0, double* ssr);
/* Batched forms for the chains in chain_mask (bit k = chain k), one host
 * synchronisation per call: parameter and result arrays have n_chains
 * entries (entries of other chains ignored).  factor_chains: covparms is
 * n_chains x ncovparms (row k = chain k); status[k] = NNGP_OK or
 * NNGP_ERR_CHOL per chain (the call itself returns NNGP_OK then).  Each
 * chain's result is bitwise the single-chain entry point's. */
int nngp_factor_chains(nngp_ctx* ctx, int which, int chain_mask, int covfun, const double* covparms,
                       int ncovparms, int* status);
int nngp_loglik_chains(nngp_ctx* ctx, int which, int chain_mask, const double* beta0,
                       const double* log_scale, double* ll);
int nngp_field_response_ratio_chains(nngp_ctx* ctx, int chain_mask, const double* beta0,
                                     const double* log_noise_variance, double* ratio);
int nngp_sum_squared_residuals_chains(nngp_ctx* ctx, int chain_mask, const double* beta0, double* ssr);
/* The sufficient MH step's two log-likelihoods (update_Gaussian.R:184-186:
 * ll_compressed_sparse_chol of the proposal minus that of the current factor)
 * for the chains in chain_mask in ONE pass over the rows: ll_prop[k] =
 * nngp_loglik_chains(1, ...) with log_scale_prop, ll_cur[k] =
 * nngp_loglik_chains(0, ...) with log_scale_cur, bitwise. */
int nngp_loglik_pair_chains(nngp_ctx* ctx, int chain_mask, const double* beta0, const double* log_scale_prop,
                            const double* log_scale_cur, double* ll_prop, double* ll_cur);
/* One Metropolis-Hastings covariance step behind ONE host sync (the separate
 * calls take two or three).  covparms, status as nngp_factor_chains (factor 1
 * = the proposal of each chain in chain_mask); then, enqueued before any
 * factor's outcome is known:
 *   ancillary_step_chains  (update_Gaussian.R:123-131): nngp_ancillary_propose_chains
 *     with beta0 / dlog_scale and nngp_field_response_ratio_chains with beta0 / lnv
 *     -> ratio[k];
 *   sufficient_step_chains (update_Gaussian.R:179-186): nngp_loglik_pair_chains
 *     -> ll_prop[k], ll_cur[k].
 * A chain whose proposal factor is not positive definite reports
 * status NNGP_ERR_CHOL and NaN results; every other chain's results are
 * bitwise those of the separate calls. */
int nngp_ancillary_step_chains(nngp_ctx* ctx, int chain_mask, int covfun, const double* covparms, int ncovparms,
                               const double* beta0, const double* dlog_scale, const double* log_noise_variance,
                               int* status, double* ratio);
int nngp_sufficient_step_chains(nngp_ctx* ctx, int chain_mask, int covfun, const double* covparms, int ncovparms,
                                const double* beta0, const double* log_scale_prop, const double* log_scale_cur,
                                int* status, double* ll_prop, double* ll_cur);
/* Y = B X for X n x ncols column-major (host buffers) */
int nngp_spmv(nngp_ctx* ctx, int which, const double* X, int ncols, double* Y);
/* x = B^{-1} u (host buffers, length n) */
int nngp_tri_solve(nngp_ctx* ctx, int which, const double* u, double* x);
/* Diagnostics of the sync-free solve (update_Gaussian.R:127): the solves of
 * this context so far whose static order stalled (a wave waited 20 ms on one
 * group, e.g. its inputs' waves were not resident) and finished in the
 * ticket order of the rescue; forced ticket orders (NNGP_TRI_RESCUE=1) do not
 * count.  Waits for the context's stream. */
int nngp_tri_rescues(nngp_ctx* ctx, long long* out);

/* ---------- regression coefficients (update_Gaussian.R:77-83,145-151,226-250) ----------
 * The design matrix resident in the context and the three array operations
 * of the regression block, batched over the chains in chain_mask (bit k =
 * chain k; per-chain arrays have n_chains rows, rows of other chains are
 * neither read nor written).  The small dense algebra -- the (p+1) and
 * (p_locs+1) square solves, Choleskys and the normal draws -- stays with the
 * caller.  Chain k's results are bitwise the same whatever other chains are in
 * the mask and from run to run (fixed reduction trees, no floating-point
 * atomics).  The entries that read the field refuse a tile-shard replica that
 * is behind (nngp_shard_sync), like the other readers.
 *
 * nngp_design_set uploads X (n_obs x p column-major, centred by the caller)
 * once for all chains and builds Xl1 = cbind(1, X[first_obs, locs_cols]),
 * n x (p_locs+1), on the device.  first_obs: length n, 1-based, the first
 * observation of each location (hctam_scol_1); locs_cols: p_locs distinct
 * 1-based columns of X (X$locs), p_locs may be 0.  X == NULL frees the design.
 * NNGP_ERR_ARG (checked before any HIP call): p < 1, p_locs outside
 * 0..min(p, 31), a column out of range or repeated, a first_obs entry outside
 * 1..n_obs.  NNGP_ERR_NOMEM: the design does not fit (no design is left).
 * NNGP_ERR_STATE: a shard context. */
int nngp_design_set(nngp_ctx* ctx, const double* X, int p, const int* first_obs, const int* locs_cols,
                    int p_locs);
/* out (n_chains x (p+1), row k = chain k) = crossprod(y - field_k[locs_match]
 * + beta0[k], cbind(1, X)) (update_Gaussian.R:230).  X is read once for all
 * chains of the mask; one host sync. */
int nngp_design_mean_stats_chains(nngp_ctx* ctx, int chain_mask, const double* beta0, double* out);
/* Per chain: other = field + shift[k] + Xl beta_locs[k,] (Xl = Xl1 without its
 * first column; beta_locs n_chains x p_locs), t[k,] = crossprod(B_cur other,
 * SX_k) (t: n_chains x (p_locs+1)), SX_k = B_cur Xl1 (update_Gaussian.R:240-241).
 * SX_k stays on the device and is formed again inside this call when chain
 * k's current factor changed since (all columns in one pass over the rows);
 * refreshed[k] = 1 then, else 0.  gram[k,,] = crossprod(SX_k)
 * (beta_interweaved_precision, :79; n_chains x (p_locs+1) x (p_locs+1)) is
 * always returned, from the call that formed SX_k when refreshed[k] = 0.
 * The field is not modified.  One host sync.  NNGP_ERR_STATE: p_locs == 0, no
 * design, factor or field. */
int nngp_design_interweave_stats_chains(nngp_ctx* ctx, int chain_mask, const double* shift,
                                        const double* beta_locs, double* t, double* gram, int* refreshed);
/* field_k = (field_k + shift[k] + Xl beta_locs_old[k,]) - Xl beta_locs_new[k,]
 * (update_Gaussian.R:233,240,245; column sums in column order; the two
 * beta_locs may be NULL when p_locs == 0: the shift alone) and mu_k = beta0[k]
 * + X beta[k,] (beta n_chains x p; :249) on the device.  Stream-ordered, no
 * host sync.  Leaves the context as nngp_set_field(new field) followed by
 * nngp_set_mu(mu, beta0[k]) would. */
int nngp_design_commit_chains(nngp_ctx* ctx, int chain_mask, const double* shift, const double* beta_locs_old,
                              const double* beta_locs_new, const double* beta0, const double* beta);
/* the selected chain's current mu (n_obs doubles); test hook like nngp_get_sweep_r */
int nngp_get_mu(nngp_ctx* ctx, double* mu);

/* ---------- colour-sharded sweep (multi-GPU) ----------
 * The chromatic sweep of ONE set of chains split over n_ranks contexts (one
 * per GPU, one process per GPU): rank g sweeps its spatial block of every
 * colour class, and after each colour the ranks all-gather {dw, w_new} of the
 * colour's locations (RCCL over xGMI) and apply the updates that cross their
 * block boundary.  Results are bitwise identical to n_ranks = 1.  A shard
 * context supports every entry point above (factor, loglik, field, ... are
 * computed redundantly on every rank) except nngp_sweep with injected
 * normals and nngp_sweep_timed; nngp_sweep / nngp_sweep_chains run the sharded
 * sweep (n_ranks > 1: after nngp_shard_comm_init).  Replaces the per-colour
 * masked update of update_Gaussian.R:261-275 across devices. */
int nngp_ctx_create_shard(const double* locs, int n, int d, const int* NNarray, int b,
                          const int* coloring, const int* locs_match,
                          const double* observed_field, int n_obs, int n_chains, int device,
                          int n_ranks, int rank, nngp_ctx** out);
/* rank 0 creates the id (len >= NNGP_SHARD_ID_BYTES) and sends it to the
 * other ranks out of band (e.g. torch.distributed broadcast) */
int nngp_shard_unique_id(unsigned char* id, int len);
/* collective over the n_ranks contexts: RCCL communicator of the shard */
int nngp_shard_comm_init(nngp_ctx* ctx, const unsigned char* id, int len);
/* all n_ranks shard contexts in ONE process (ctxs[g] = rank g; any devices):
 * nngp_sweep_chains with the exchange done by device copies between them.
 * Tile shards: the ranks of one device run in one launch (their tiles must fit
 * the device's CUs together), ranks on one device contiguous. */
int nngp_sweep_chains_group(nngp_ctx** ctxs, int n_ranks, int n_sweeps, const double* beta0,
                            const double* log_scale, const double* log_noise_variance,
                            const uint64_t* seed, const uint64_t* counter_base);

/* Tile shard (sweep_engine 1 on a shard context, the default when the tile
 * layout fits): the tile-resident sweep with its tiles split over the ranks
 * (rank g runs tiles [g*T/G, (g+1)*T/G) on its GPU).  A draw read by a tile
 * of another rank is written into that rank's granule buffer (peer memory
 * over xGMI) by the producing tile, so the hand-offs stay inside the one
 * persistent launch per call.  After the launch the ranks' replicas of the
 * field are brought up to date: with a communicator (nngp_shard_comm_init),
 * one grouped RCCL broadcast of every rank's slots; without one (the
 * default), each rank stores only its halo -- its slots that other ranks'
 * rows contain -- into the peers' replicas (peer stores + device flags), and
 * the other foreign slots of each replica fall behind until nngp_shard_sync.
 * Setup, every rank: export this rank's handles (nngp_shard_ipc_handle),
 * exchange them out of band (all-gather), open the others'
 * (nngp_shard_ipc_open).  NNGP_ENGINE=colors at creation selects the colour
 * shard instead. */
int nngp_shard_ipc_handle(nngp_ctx* ctx, unsigned char* handle, int len);
/* handles: n_ranks x len_each bytes, rank order (this rank's entry ignored).
 * Without a communicator (no nngp_shard_comm_init) a call exchanges w by
 * peer copies into the mapped replicas and device flags instead of RCCL. */
int nngp_shard_ipc_open(nngp_ctx* ctx, const unsigned char* handles, int len_each);
/* Collective over the ranks of a tile shard without a communicator (every
 * rank calls it, in the same order relative to its sweeps): the full
 * exchange of the field replicas.  After sweeps without it, the entry points
 * that read the field (nngp_get_field, nngp_record_field, nngp_loglik*,
 * nngp_beta0_stats, nngp_field_response_ratio*, nngp_sum_squared_residuals*,
 * nngp_ancillary_propose*, nngp_accept_field) return NNGP_ERR_STATE -- a
 * reader never performs a hidden collective.  A no-op on every other
 * context and on an up-to-date replica. */
int nngp_shard_sync(nngp_ctx* ctx);

/* ---------- posterior summaries (no context) ---------- */
/* get_summary (Scripts/mcmc_nngp_estimate.R:1-6; its uses at estimate.R:88-94 and
 * predict.R:57-58) of the row-wise stack of n_blocks host blocks; block k is
 * block_rows[k] x n row-major with row pitch n.  row_offset (total rows, or NULL)
 * is subtracted from each row.  out: n x 5 column-major (R matrix; columns mean,
 * q0.025, median, q0.975, sd).  chunk_cols: 0 = automatic, else the number of
 * columns staged per kernel launch.
 * The quantiles are R's type 7 (numpy 'linear') on exactly selected order
 * statistics, the mean is the sum in row order / rows, sd the two-pass one
 * with divisor rows - 1 (NaN for one row); a column holding a NaN gives five
 * NaNs.  A column's five numbers depend on that column alone: not on n, the
 * chunking or the column's position.  At most 2^31 - 1 rows in total.
 * The blocks are read where they lie (no stacked host copy): column chunks
 * are staged into two device buffers, the copy of one chunk running beside
 * the kernel of the chunk before.  Automatic chunk_cols keeps both buffers
 * together within 1 GiB (never below 64 columns), and cuts a matrix that
 * would fit one chunk into about four while a chunk keeps >= 65536 columns.
 * The n x 5 result is held on the device as well and copied out once.
 * device: HIP ordinal (-1: current); the calling thread's current device is
 * the same after the call as before it.  NNGP_ERR_ARG: no rows, n < 1,
 * n_blocks < 1, a null block. */
int nngp_summary(int device, const double* const* blocks, const long long* block_rows,
                 int n_blocks, long long n, const double* row_offset, int chunk_cols,
                 double* out);
/* The same summary with the quantiles chosen by the caller and exceedance
 * probabilities, the usual product of a pollution map (the reference's last
 * step, Heavy_metals/Results_analysis.R, maps the field's summary): blocks,
 * block_rows, n, row_offset, chunk_cols, device, staging and the row limit are
 * nngp_summary's.  probs: n_probs (0..16) probabilities in [0, 1], in any
 * order, repeats allowed; thresholds: n_thresholds (0..8) values, +-inf
 * allowed; either array may be NULL when its count is 0.
 * out: n x (2 + n_probs + n_thresholds) column-major: mean, the type-7
 * quantiles in the order of probs (0 and 1 are the exact minimum and
 * maximum), sd, then P(x > thresholds[k]) = count(x > t) / rows -- a strict
 * compare of the values summarised (after row_offset), an integer count and
 * one division.  probs = (0.025, 0.5, 0.975) without thresholds gives
 * nngp_summary's matrix bit for bit.  A quantile's bits depend on its column
 * and its own probability only, an exceedance column on its threshold only:
 * not on what else was asked, nor on n, the chunking or the column's
 * position.  A column holding a NaN gives NaNs in every output.
 * NNGP_ERR_ARG (before any HIP call): what nngp_summary rejects; n_probs
 * outside 0..16, n_thresholds outside 0..8, a null array with a positive
 * count, a probability that is NaN or outside [0, 1], a NaN threshold. */
int nngp_summary_probs(int device, const double* const* blocks, const long long* block_rows,
                       int n_blocks, long long n, const double* row_offset, int chunk_cols,
                       const double* probs, int n_probs, const double* thresholds, int n_thresholds,
                       double* out);
/* Measurement: the calling thread's last successful summary (nngp_summary or
 * nngp_summary_probs, whichever ran last) -- HIP-event times
 * of its staging copies and of its kernels (each summed over the chunks; they
 * overlap, so the sum can exceed the call's wall time), the bytes staged and
 * the chunk width used.  Any pointer may be NULL.  NNGP_ERR_STATE: none yet.
 * A separate entry, like the sweep's timed form, so that the summary's own
 * signature carries no measurement arguments: the times exist only inside the
 * call (its streams and events are gone when it returns), and
 * scripts/summary_time.py, the R wrapper and a C client all read them here. */
int nngp_summary_stats(double* copy_ms, double* kernel_ms, long long* staged_bytes, int* chunk_cols);

/* ---------- fixed-effect / response samples generated and summarised on the device (no context) ---------- */
/* mcmc_nngp_predict_fixed_effects (Scripts/mcmc_nngp_predict.R:92-102) without the
 * n_samples x n matrix beta_matrix[, subset] %*% t(X_pred) on the host: the samples
 * are generated chunk by chunk in the device buffer that the kernels of
 * nngp_summary_probs read, and summarised there.
 * coef: n_samples x q column-major (R's beta_matrix[, beta_subset]); X: n x q
 * column-major (the design rows of the n new locations).  Optional addend: the
 * row-wise stack of n_blocks host blocks (nngp_summary's convention: block k is
 * block_rows[k] x n row-major, pitch n, read where it lies); n_blocks == 0 with
 * NULL arrays: none.  Optional noise: noise_sd (n_samples) and counter
 * (n_samples); noise_sd == NULL: none.
 * The value of sample s at location c is defined by its arithmetic, in this order:
 *   acc = coef[s,0] * X[c,0]
 *   acc = fma(coef[s,k], X[c,k], acc)      k = 1 .. q-1, in column order
 *   acc = addend[s,c] + acc                with an addend
 *   acc = fma(noise_sd[s], z, acc)         with noise; z = the Philox / AS241 normal
 *                                          of (seed, counter[s], c), the value
 *                                          nngp_device_normals returns at [c] for
 *                                          sweep = counter[s]
 * so it depends on (s, c) and its inputs alone: not on n, the chunking, the
 * column's position or the other samples.  NaN and inf in coef, X or the addend
 * propagate by IEEE rules (a NaN among a location's samples gives NaNs in that
 * location's outputs, as nngp_summary_probs documents).
 * out: n x (2 + n_probs + n_thresholds) column-major, the columns of
 * nngp_summary_probs of these samples (bit for bit what it returns for them);
 * probs and thresholds as there.  samples_out: n_samples x n row-major, or NULL;
 * when given, every chunk's values are copied there, otherwise no sample leaves
 * the device.
 * Staging: coef and X are copied to the device once; per chunk of chunk_cols
 * columns (0 = automatic, nngp_summary's rule: both chunk buffers within 1 GiB,
 * never below 64 columns) only the addend's columns are copied, the copy of one
 * chunk running beside the kernels of the chunk before; without an addend
 * nothing is copied per chunk.  Device footprint: the two chunk buffers, X,
 * coef and out.  device: HIP ordinal (-1: current); the calling thread's
 * current device is the same after the call as before it.
 * NNGP_ERR_ARG (before any HIP call): what nngp_summary_probs rejects for probs
 * and thresholds; a null coef, X or out; n < 1; n_samples outside 1..2^31-1;
 * q outside 1..1024; chunk_cols < 0; a null addend block, or addend rows that
 * do not sum to n_samples; a NaN or negative noise_sd; noise_sd without
 * counter; noise with n > 2^31-1 (z is indexed by an int). */
int nngp_effects_summary(int device, const double* coef, long long n_samples, int q,
                         const double* X, long long n,
                         const double* const* addend_blocks, const long long* block_rows, int n_blocks,
                         const double* noise_sd, uint64_t seed, const uint64_t* counter,
                         int chunk_cols, const double* probs, int n_probs,
                         const double* thresholds, int n_thresholds,
                         double* out, double* samples_out);
/* Measurement, as nngp_summary_stats: the calling thread's last successful
 * nngp_effects_summary -- HIP-event times of the addend copies, the generator
 * kernels and the summary kernels (each summed over the chunks), the addend
 * bytes staged (0 without an addend) and the chunk width used.  Any pointer may
 * be NULL.  NNGP_ERR_STATE: none yet. */
int nngp_effects_stats(double* copy_ms, double* generate_ms, double* kernel_ms,
                       long long* staged_bytes, int* chunk_cols);

/* ---------- pointwise log-likelihood of the saved samples, reduced per observation (no context) ---------- */
/* The Gaussian log density of every observation under every saved sample (the
 * dnorm terms of Scripts/mcmc_nngp_update_Gaussian.R:130-131,281), reduced over
 * the samples on the device: what WAIC, LPML, DIC and the log score / PIT of
 * held-out observations are sums of.  The n_samples x n_obs matrix exists nowhere.
 * y (n_obs) and obs_loc (n_obs: the 1-based location of each observation,
 * non-decreasing -- the order of vecchia_approx$hctam_scol; a location may carry
 * 0, 1 or many observations).  coef: n_samples x q column-major; X: n_obs x q
 * column-major, rows in the order of y; q == 0 with both NULL: no regression
 * term.  field_blocks: the row-wise stack of n_blocks host blocks (nngp_summary's
 * convention: block k is block_rows[k] x n row-major, pitch n, read where it
 * lies).  log_noise_var: n_samples.
 * Per sample s, a_s = -0.5 (log(2 pi) + lnv_s), h_s = 0.5 exp(-lnv_s) and
 * g_s = sqrt(2 h_s) are computed once on the host in fp64.  The value of sample
 * s at observation i (c = obs_loc[i] - 1) is defined by its arithmetic, in this
 * order:
 *   acc  = coef[s,0] * X[i,0]
 *   acc  = fma(coef[s,k], X[i,k], acc)     k = 1 .. q-1, in column order
 *   mean = field[s,c] + acc                (field[s,c] alone when q == 0)
 *   r    = y[i] - mean
 *   ll   = fma(-(h_s * r), r, a_s)
 *   p    = 0.5 * erfc(-((r * g_s) * C))    C = the double nearest 1 / sqrt(2)
 * out: n_obs x 6 column-major; every sum below runs over s in row order, in
 * fp64, one addition per sample (D = (double)n_samples):
 *   1 fit_mean = (sum mean) / D
 *   2 ll_mean  = (sum ll) / D
 *   3 ll_var   = (sum by ss = fma(d, d, ss), d = ll - ll_mean) / (D - 1); NaN for n_samples == 1
 *   4 lppd     = (M + log(sum exp(ll - M))) - log(D),       M  = max_s ll
 *   5 log_cpo  = -((M' + log(sum exp(-ll - M'))) - log(D)), M' = max_s (-ll)
 *   6 pit      = (sum p) / D
 * (log(D) from the host).  The maxima shift the sums, so lppd and log_cpo are
 * finite whenever every ll is.  An observation's six numbers depend on its own
 * y, X row, and its location's column alone: not on n, n_obs, the chunking, its
 * position or the other observations.  A NaN in y[i], X[i, ] or the location's
 * column gives six NaNs for observation i and for no other (a NaN coef poisons
 * every observation).
 * Staging as nngp_summary: column chunks of chunk_cols locations (0 = automatic:
 * both chunk buffers within 1 GiB, never below 64 columns) go through two device
 * buffers, the copy of one chunk running beside the kernel of the chunk before;
 * a chunk no observation reads is not staged.  y, obs_loc, coef, X and the
 * per-sample constants are copied once, out is held on the device and copied
 * out once.  device: HIP ordinal (-1: current); the calling thread's current
 * device is the same after the call as before it.
 * NNGP_ERR_ARG (before any HIP call): a null y, obs_loc, out or log_noise_var;
 * n_obs < 1; n < 1; n_samples outside 1..2^31-1; q outside 0..1024; q > 0 with a
 * null coef or X; an obs_loc that decreases or lies outside 1..n; no blocks, a
 * null block, or block rows that do not sum to n_samples; a NaN or infinite
 * log_noise_var; chunk_cols < 0. */
int nngp_pointwise_loglik(int device,
                          const double* y, long long n_obs, const int* obs_loc,
                          const double* coef, long long n_samples, int q,
                          const double* X,
                          const double* const* field_blocks, const long long* block_rows, int n_blocks, long long n,
                          const double* log_noise_var,
                          int chunk_cols, double* out);
/* Measurement, as nngp_summary_stats: the calling thread's last successful
 * nngp_pointwise_loglik -- HIP-event times of the field copies and of the
 * kernels (each summed over the chunks), the bytes staged and the chunk width
 * used.  Any pointer may be NULL.  NNGP_ERR_STATE: none yet. */
int nngp_pointwise_loglik_stats(double* copy_ms, double* kernel_ms, long long* staged_bytes, int* chunk_cols);

/* ---------- convergence diagnostics per field location (no context) ---------- */
/* Individual_PSRF of Gelman_Rubin_Brooks and ESS (Scripts/mcmc_nngp_diagnose.R:1-24,
 * 107-118) of every column of n_chains host blocks; block k is chain k, rows x n
 * row-major with row pitch n (the saved field rows after burn-in).  row_offset
 * (n_chains x rows entries in stack order, or NULL) is subtracted from each row.
 * out: n x 5 column-major (columns R_hat, ess, ess_min, W, Bv); order (n_chains x
 * n, order[k * n + j], or NULL): the AR order selected for chain k at location j.
 * Per chain and column (S = rows values x): mean = sum in row order / S; var =
 * two-pass variance with divisor S - 1; for S < 4 or a centred sum of squares
 * of exactly 0, ess_k = S and order 0; otherwise P = min(S - 1, int(10 log10 S)),
 * acf[l] = sum_t xc[t] xc[t+l] / S (l = 0..P), Levinson-Durbin (left at the
 * first v <= 0), AIC = S log v + 2 l, the first minimum from l = 0 upward,
 * spec0 = v / (1 - sum phi)^2 and ess_k = S acf[0] / spec0 (S unless spec0 > 0).
 * Per location: W = mean of the chains' var, Bv = variance of their means with
 * divisor n_chains - 1 (NaN for one chain),
 *   R_hat = ((m+1)/m) ((S-1)/S) (Bv/W) + (S+1)/S     (m = n_chains)
 * in plain IEEE division (0/0 = NaN, x/0 = inf), ess = sum of ess_k, ess_min
 * their minimum.  A column holding a NaN in any chain gives five NaNs and
 * order 0.  A location's numbers depend on its column alone: not on n, the
 * chunking or the column's position.
 * Staging as nngp_summary: the blocks are read where they lie, column chunks go
 * through two device buffers, the copy of one chunk running beside the kernel
 * of the chunk before; chunk_cols: 0 = automatic (both buffers within 1 GiB,
 * never below 64 columns), else the columns staged per launch.  device: HIP
 * ordinal (-1: current); the calling thread's current device is the same after
 * the call as before it.  NNGP_ERR_ARG (before any HIP call): a null block,
 * n < 1, n_chains outside 1..16, rows outside 2..9999, chunk_cols < 0. */
int nngp_field_diag(int device, const double* const* blocks, int n_chains, long long rows,
                    long long n, const double* row_offset, int chunk_cols,
                    double* out, int* order);
/* Measurement, as nngp_summary_stats: the calling thread's last successful
 * nngp_field_diag.  Any pointer may be NULL.  NNGP_ERR_STATE: none yet. */
int nngp_field_diag_stats(double* copy_ms, double* kernel_ms, long long* staged_bytes, int* chunk_cols);

/* ---------- posterior prediction at new locations (no context) ---------- */
/* The samples of mcmc_nngp_predict_field (Scripts/mcmc_nngp_predict.R:39-53) for
 * n_samples saved samples of one chain in one call.  The stacked factor is lower
 * triangular and its observed rows name observed columns only, so
 * sd B^{-1} c(B11 (w/sd), z) equals w on the observed locations and, for the new
 * locations p = n .. N-1 in order (y = w on the observed ones, w = field - beta0),
 *   y[p] = (sd z[p-n] - sum_{j>=1} Linv[p,j] y[NN[p,j]]) / Linv[p,0],
 * out[s, p-n] = y[p]: only the factor rows of the new locations (the arithmetic
 * of nngp_factor on the stacked problem) and the observed values they name are
 * computed or moved.
 * locs: N x d column-major, N = n + n_pred: the n ordered observed locations,
 * then the new ones.  NNarray: N x b column-major, 1-based, NA = INT_MIN; only
 * rows n+1..N are read (column 1 the row itself, later columns earlier rows).
 * covparms: n_factors x ncovparms, row k = the parameters of factor k (one
 * covfun); factor_of[s] = the 0-based factor sample s uses.  Sample s reads
 * its field at fields + field_row[s] * field_pitch (n doubles, where they lie;
 * field_pitch in doubles), beta0[s] and log_scale[s] (sd = exp(log_scale / 2)).
 * Normals: z (n_samples x n_pred row-major), or z == NULL: new location i
 * (0-based) of sample s draws the Philox / AS241 normal of (seed, counter[s], i),
 * the value nngp_device_normals returns at [i] for sweep = counter[s].
 * out: n_samples x n_pred row-major.  A sample's output row depends on that
 * sample's inputs alone: not on sample_batch, the other samples or its position.
 * Samples are processed in batches of sample_batch (0 = automatic: the largest
 * multiple of 64 whose device buffers -- the factor rows of the batch's distinct
 * factors, the values [support + new rows] x batch, the staged support values
 * and the normals / output block -- stay within 1 GiB, never below 64, at most
 * n_samples).  NNGP_ERR_CHOL: a factor row is not positive definite; *fail_row
 * (may be NULL) = its stacked 1-based row (the first one of the first failing
 * sample's factor), else 0.  NNGP_ERR_ARG (checked before any HIP call):
 * a null pointer (z and counter both NULL included), n, n_pred, n_factors or
 * n_samples < 1, d outside 1..4, b outside 1..32, factor_of out of range, bad
 * covparms, a table whose new rows name themselves or later rows.
 * device: HIP ordinal (-1: current); the calling thread's current device is
 * the same after the call as before it. */
int nngp_predict_field(int device, const double* locs, int n, int n_pred, int d,
                       const int* NNarray, int b, int covfun, const double* covparms, int ncovparms,
                       int n_factors, int n_samples, const int* factor_of, const double* fields,
                       long long field_pitch, const long long* field_row, const double* beta0,
                       const double* log_scale, const double* z, uint64_t seed, const uint64_t* counter,
                       int sample_batch, double* out, int* fail_row);
/* Measurement: the calling thread's last successful prediction -- host time of
 * the plan (support set, compact table, level schedule), HIP-event times of
 * the factor launches and of the staging + solve + output copy (each summed
 * over the batches), the bytes staged and the batch size used.  Any pointer
 * may be NULL.  NNGP_ERR_STATE: none yet. */
int nngp_predict_stats(double* plan_ms, double* factor_ms, double* solve_ms, long long* staged_bytes,
                       int* sample_batch);

/* ---------- measurement ---------- */
/* nngp_sweep_chains bracketed by HIP events on the context's stream;
 * *ms = elapsed for the whole call; *kernel_ms (if not NULL) = elapsed for the
 * n_sweeps x n_colors sweep-kernel launches alone (a graph of only those
 * launches between two events: mean launch time = kernel_ms / launches). */
int nngp_sweep_timed(nngp_ctx* ctx, int n_sweeps, const double* beta0, const double* log_scale,
                     const double* log_noise_variance, const uint64_t* seed,
                     const uint64_t* counter_base, double* ms, double* kernel_ms);
/* Philox normals generated by the device code path (test hook). */
int nngp_device_normals(int device, uint64_t seed, uint64_t sweep, int n, double* z);
/* r = B (field - beta0) of the selected chain as the last sweep call left it
 * (location order, length n): the state a warm tile call starts from (the
 * tile kernel writes its r back).  Introspection for the
 * warm-call drift tests -- nngp_spmv gives the fresh product to compare. */
int nngp_get_sweep_r(nngp_ctx* ctx, double* r);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_H_ */
