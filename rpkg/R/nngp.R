# Thin R wrappers of the .Call entry points of src/nngp_shim.c (one per
# function of include/nngp.h).  Arrays follow R's own conventions
# (column-major, 1-based, NA_integer_), so GpGp / Matrix outputs of the
# reference pass through unchanged.

.covfun_ids <- c(exponential_isotropic = 0L, exponential_sphere = 1L, exponential_scaledim = 2L,
                 exponential_spacetime = 3L, matern_isotropic = 4L, matern_sphere = 5L,
                 matern_scaledim = 6L, matern_spacetime = 7L, matern15_isotropic = 8L)

nngp_covfun_id <- function(covfun_name) {
  id <- .covfun_ids[covfun_name]
  if (is.na(id)) stop("nngp: unknown covariance function ", covfun_name)
  unname(id)
}

# c(1, shape, 0) with the MCMC's transforms (update_Gaussian.R:67-72):
# exp() for log_* parameters, lo + span * plogis() for qlogis_* ones
nngp_covparms <- function(shape_params, shape, lo = .5, span = .5) {
  tr <- vapply(seq_along(shape_params), function(j) {
    if (substr(shape_params[j], 1, 3) == "log") exp(shape[j])
    else lo + span * stats::plogis(shape[j])
  }, 0)
  c(1, tr, 0)
}

nngp_abi_version <- function() .Call(C_nngp_abi_version)
nngp_status_string <- function(status) .Call(C_nngp_status_string, as.integer(status))
nngp_last_error <- function(ctx) .Call(C_nngp_ctx_last_error, ctx)
nngp_order_maxmin <- function(locs) .Call(C_nngp_order_maxmin, as.matrix(locs) + 0)
nngp_find_ordered_nn <- function(locs, m) .Call(C_nngp_find_ordered_nn, as.matrix(locs) + 0, as.integer(m))
nngp_greedy_coloring <- function(NNarray) .Call(C_nngp_greedy_coloring, NNarray)

nngp_context <- function(locs, NNarray, coloring, locs_match, observed_field, n_chains = 1L, device = -1L) {
  storage.mode(NNarray) <- "integer"
  .Call(C_nngp_ctx_create, as.matrix(locs) + 0, NNarray, as.integer(coloring), as.integer(locs_match),
        as.double(observed_field), as.integer(n_chains), as.integer(device))
}
nngp_context_shard <- function(locs, NNarray, coloring, locs_match, observed_field, n_ranks, rank,
                               n_chains = 1L, device = -1L) {
  storage.mode(NNarray) <- "integer"
  .Call(C_nngp_ctx_create_shard, as.matrix(locs) + 0, NNarray, as.integer(coloring), as.integer(locs_match),
        as.double(observed_field), as.integer(n_chains), as.integer(device), as.integer(n_ranks),
        as.integer(rank))
}
nngp_destroy <- function(ctx) invisible(.Call(C_nngp_ctx_destroy, ctx))
nngp_info <- function(ctx) .Call(C_nngp_ctx_info, ctx)
# the sweep engine chosen at creation and why (tile residency / LDS fallbacks)
nngp_engine_note <- function(ctx) .Call(C_nngp_ctx_engine_note, ctx)
nngp_set_chain <- function(ctx, chain) invisible(.Call(C_nngp_set_chain, ctx, as.integer(chain)))

nngp_factor <- function(ctx, which, covfun_name, covparms)
  invisible(.Call(C_nngp_factor, ctx, as.integer(which), nngp_covfun_id(covfun_name), as.double(covparms)))
nngp_get_linv <- function(ctx, which = 0L) .Call(C_nngp_get_linv, ctx, as.integer(which))
nngp_set_linv <- function(ctx, which, Linv) invisible(.Call(C_nngp_set_linv, ctx, as.integer(which), Linv + 0))
nngp_accept_factor <- function(ctx) invisible(.Call(C_nngp_accept_factor, ctx))
nngp_precision_diag <- function(ctx) .Call(C_nngp_get_precision_diag, ctx)

nngp_set_field <- function(ctx, field) invisible(.Call(C_nngp_set_field, ctx, as.double(field)))
nngp_get_field <- function(ctx) .Call(C_nngp_get_field, ctx)
nngp_set_mu <- function(ctx, mu, beta_0)
  invisible(.Call(C_nngp_set_mu, ctx, if (is.null(mu)) NULL else as.double(mu), as.double(beta_0)))
nngp_records_reserve <- function(ctx, n_rows) invisible(.Call(C_nngp_records_reserve, ctx, as.integer(n_rows)))
nngp_record_field <- function(ctx, row) invisible(.Call(C_nngp_record_field, ctx, as.integer(row)))
nngp_get_records <- function(ctx, row0, n_rows, buf = NULL) .Call(C_nngp_get_records, ctx, as.integer(row0), as.integer(n_rows), buf)
# rows x n numeric vector the selected chain's records stream into while it runs (NULL: release)
nngp_records_stream <- function(ctx, buf) invisible(.Call(C_nngp_records_stream, ctx, buf))

nngp_loglik <- function(ctx, which, beta_0, log_scale)
  .Call(C_nngp_loglik, ctx, as.integer(which), as.double(beta_0), as.double(log_scale))
# ll_compressed_sparse_chol (update_Gaussian.R:8-12) on the device factor `which`
ll_compressed_sparse_chol <- function(ctx, which, beta_0, log_scale) nngp_loglik(ctx, which, beta_0, log_scale)

nngp_sweep <- function(ctx, n_sweeps, beta_0, log_scale, log_noise_variance, seed, counter_base, z = NULL)
  invisible(.Call(C_nngp_sweep, ctx, as.integer(n_sweeps), as.double(beta_0), as.double(log_scale),
                  as.double(log_noise_variance), as.double(seed), as.double(counter_base),
                  if (is.null(z)) NULL else as.double(z)))
nngp_sweep_chains <- function(ctx, n_sweeps, beta_0, log_scale, log_noise_variance, seed, counter_base)
  invisible(.Call(C_nngp_sweep_chains, ctx, as.integer(n_sweeps), as.double(beta_0), as.double(log_scale),
                  as.double(log_noise_variance), as.double(seed), as.double(counter_base)))
nngp_sweep_timed <- function(ctx, n_sweeps, beta_0, log_scale, log_noise_variance, seed, counter_base)
  .Call(C_nngp_sweep_timed, ctx, as.integer(n_sweeps), as.double(beta_0), as.double(log_scale),
        as.double(log_noise_variance), as.double(seed), as.double(counter_base))
nngp_ancillary_propose <- function(ctx, beta_0, dlog_scale)
  invisible(.Call(C_nngp_ancillary_propose, ctx, as.double(beta_0), as.double(dlog_scale)))
nngp_ancillary_propose_chains <- function(ctx, chain_mask, beta_0, dlog_scale)
  invisible(.Call(C_nngp_ancillary_propose_chains, ctx, as.integer(chain_mask), as.double(beta_0),
                  as.double(dlog_scale)))
nngp_field_response_ratio <- function(ctx, beta_0, log_noise_variance)
  .Call(C_nngp_field_response_ratio, ctx, as.double(beta_0), as.double(log_noise_variance))
nngp_accept_field <- function(ctx) invisible(.Call(C_nngp_accept_field, ctx))
nngp_beta0_stats <- function(ctx) .Call(C_nngp_beta0_stats, ctx)
nngp_sum_squared_residuals <- function(ctx, beta_0) .Call(C_nngp_sum_squared_residuals, ctx, as.double(beta_0))
nngp_spmv <- function(ctx, which, X) .Call(C_nngp_spmv, ctx, as.integer(which), X + 0)
nngp_tri_solve <- function(ctx, which, u) .Call(C_nngp_tri_solve, ctx, as.integer(which), as.double(u))
# solves that finished in the rescue's ticket order (diagnostic)
nngp_tri_rescues <- function(ctx) .Call(C_nngp_tri_rescues, ctx)
nngp_device_normals <- function(device, seed, sweep, n)
  .Call(C_nngp_device_normals, as.integer(device), as.double(seed), as.double(sweep), as.integer(n))
# get_summary (Scripts/mcmc_nngp_estimate.R:1-6) of a samples x locations matrix on the device:
# n x 5 with columns mean, q0.025, median, q0.975, sd (type-7 quantiles, as quantile()'s default)
# With probs (up to 16 probabilities in [0, 1], any order) or thresholds (up to 8 values) given:
# n x (2 + Q + K) with columns mean, q<p>..., sd, p_gt_<t>... -- the type-7 quantiles in the order of probs
# (NULL: 0.025, 0.5, 0.975) and the exceedance fractions mean(x > t) per location.  Both NULL: the call above.
nngp_get_summary <- function(samples, device = -1L, probs = NULL, thresholds = NULL) {
  if (!is.matrix(samples)) samples <- matrix(samples, ncol = 1)
  storage.mode(samples) <- "double"
  if (is.null(probs) && is.null(thresholds)) return(.Call(C_nngp_summary, as.integer(device), samples))
  probs <- if (is.null(probs)) c(0.025, 0.5, 0.975) else as.double(probs)
  thresholds <- as.double(thresholds)
  out <- .Call(C_nngp_summary_probs, as.integer(device), samples, probs, thresholds)
  colnames(out) <- c("mean", sprintf("q%g", probs), "sd", sprintf("p_gt_%g", thresholds))
  out
}
# HIP-event times (ms), staged bytes and chunk width of the last nngp_get_summary
nngp_summary_stats <- function() .Call(C_nngp_summary_stats)
# The summary of coef %*% t(X) (+ addend) (+ noise_sd * normals) per location, the samples generated and summarised
# on the device (Scripts/mcmc_nngp_predict.R:92-102 without the n_samples x n matrix in R's memory): coef S x q
# (beta_matrix[, beta_subset]), X n x q (the design rows of the new locations), addend NULL or S x n (the predicted
# field's samples), noise_sd NULL or S values with seed and counter (default 0 .. S-1: the Philox / AS241 normals of
# nngp_device_normals(device, seed, counter[s], n)).  -> n x (2 + Q + K) with nngp_get_summary's columns
# (probs NULL: 0.025, 0.5, 0.975)
nngp_effects_summary <- function(coef, X, addend = NULL, noise_sd = NULL, seed = 0, counter = NULL, probs = NULL,
                                 thresholds = NULL, device = -1L) {
  coef <- as.matrix(coef) + 0
  X <- as.matrix(X) + 0
  probs <- if (is.null(probs)) c(0.025, 0.5, 0.975) else as.double(probs)
  thresholds <- as.double(thresholds)
  if (!is.null(noise_sd) && is.null(counter)) counter <- seq_len(nrow(coef)) - 1
  out <- .Call(C_nngp_effects_summary, as.integer(device), coef, X, if (is.null(addend)) NULL else t(addend) + 0,
               if (is.null(noise_sd)) NULL else as.double(noise_sd), as.double(seed),
               if (is.null(counter)) NULL else as.double(counter), probs, thresholds)
  colnames(out) <- c("mean", sprintf("q%g", probs), "sd", sprintf("p_gt_%g", thresholds))
  out
}
# HIP-event times (ms), staged bytes and chunk width of the last nngp_effects_summary
nngp_effects_stats <- function() .Call(C_nngp_effects_stats)
# The Gaussian log density of every observation under every saved sample (the dnorm terms of
# Scripts/mcmc_nngp_update_Gaussian.R:130-131,281), reduced over the samples on the device: y (n_obs), obs_loc
# (n_obs, the 1-based location of each observation, any order: vecchia_approx$locs_match), field S x n (the saved
# field rows, beta_0 included), log_noise_var (S), coef NULL or S x q with X n_obs x q.  -> n_obs x 6 with columns
# fit_mean, ll_mean, ll_var, lppd, log_cpo, pit, rows in the caller's order (WAIC = -2 (sum(lppd) - sum(ll_var)),
# LPML = sum(log_cpo))
nngp_pointwise_loglik <- function(y, obs_loc, field, log_noise_var, coef = NULL, X = NULL, device = -1L) {
  ord <- order(obs_loc)  # stable: ties keep the caller's order
  if (!is.null(coef)) {
    coef <- as.matrix(coef) + 0
    X <- (as.matrix(X) + 0)[ord, , drop = FALSE]
  }
  out <- .Call(C_nngp_pointwise_loglik, as.integer(device), as.double(y)[ord], as.integer(obs_loc)[ord], coef,
               if (is.null(coef)) NULL else X, t(field) + 0, as.double(log_noise_var))
  out[ord, ] <- out
  colnames(out) <- c("fit_mean", "ll_mean", "ll_var", "lppd", "log_cpo", "pit")
  out
}
# HIP-event times (ms), staged bytes and chunk width of the last nngp_pointwise_loglik
nngp_pointwise_loglik_stats <- function() .Call(C_nngp_pointwise_loglik_stats)
# R-hat (Individual_PSRF of Gelman_Rubin_Brooks, n := saved rows) and effective sample size (ESS) of every
# field location (Scripts/mcmc_nngp_diagnose.R:1-24,107-118) on the device.  chains: a list with one
# samples x locations matrix per chain (the saved field rows after burn-in, centred); -> n x 5 with
# columns R_hat, ess, ess_min, W, Bv
nngp_field_diagnostics <- function(chains, device = -1L) {
  if (is.matrix(chains)) chains <- list(chains)
  chains_t <- lapply(chains, function(x) { x <- t(x); storage.mode(x) <- "double"; x })
  .Call(C_nngp_field_diag, as.integer(device), chains_t)
}
# HIP-event times (ms), staged bytes and chunk width of the last nngp_field_diagnostics
nngp_field_diag_stats <- function() .Call(C_nngp_field_diag_stats)
# The predicted samples (n_samples x n_pred) of one chain in one call (Scripts/mcmc_nngp_predict.R:39-53):
# locs / NNarray of the stacked locations (the n observed first), covparms one row per distinct factor,
# factor_of (1-based row of covparms per sample), fields n_samples x n (the chain's saved fields of the
# samples), z n_samples x n_pred normals or NULL (Philox normals of (seed, counter[s]) drawn on the device).
# The shim takes the per-sample matrices transposed (R's column-major = the C ABI's row-major).
nngp_predict_field <- function(locs, n, NNarray, covfun, covparms, factor_of, fields, beta_0, log_scale, z = NULL,
                               seed = 0, counter = NULL, sample_batch = 0L, device = -1L) {
  storage.mode(NNarray) <- "integer"
  t(.Call(C_nngp_predict_field, as.integer(device), as.matrix(locs) + 0, as.integer(n), NNarray,
          nngp_covfun_id(covfun), t(as.matrix(covparms)) + 0, as.integer(factor_of) - 1L, t(fields) + 0,
          as.double(beta_0), as.double(log_scale), if (is.null(z)) NULL else t(z) + 0, as.double(seed),
          if (is.null(counter)) NULL else as.double(counter), as.integer(sample_batch)))
}
# plan / factor / solve times (ms), staged bytes and batch size of the last nngp_predict_field
nngp_predict_stats <- function() .Call(C_nngp_predict_stats)
# r = B (field - beta0) of the selected chain as the last sweep call left it (warm-call state)
nngp_get_sweep_r <- function(ctx) .Call(C_nngp_get_sweep_r, ctx)

nngp_shard_unique_id <- function() .Call(C_nngp_shard_unique_id)
nngp_shard_comm_init <- function(ctx, id) invisible(.Call(C_nngp_shard_comm_init, ctx, id))
nngp_factor_chains <- function(ctx, which, chain_mask, covfun, covparms)
  .Call(C_nngp_factor_chains, ctx, as.integer(which), as.integer(chain_mask), nngp_covfun_id(covfun),
        as.matrix(covparms) + 0)
nngp_loglik_chains <- function(ctx, which, chain_mask, beta_0, log_scale)
  .Call(C_nngp_loglik_chains, ctx, as.integer(which), as.integer(chain_mask), as.double(beta_0), as.double(log_scale))
# list(proposal = loglik_chains(1, ...), current = loglik_chains(0, ...)) in one pass over the rows
nngp_loglik_pair_chains <- function(ctx, chain_mask, beta_0, log_scale_prop, log_scale_cur)
  .Call(C_nngp_loglik_pair_chains, ctx, as.integer(chain_mask), as.double(beta_0), as.double(log_scale_prop),
        as.double(log_scale_cur))
# one host sync for a proposal's factor and its MH step (update_Gaussian.R:123-131 / :179-186):
# list(status, ratio) / list(status, proposal, current); a failed factor (status 3): NaN values
nngp_ancillary_step_chains <- function(ctx, chain_mask, covfun, covparms, beta_0, dlog_scale, log_noise_variance)
  .Call(C_nngp_ancillary_step_chains, ctx, as.integer(chain_mask), nngp_covfun_id(covfun), as.matrix(covparms) + 0,
        as.double(beta_0), as.double(dlog_scale), as.double(log_noise_variance))
nngp_sufficient_step_chains <- function(ctx, chain_mask, covfun, covparms, beta_0, log_scale_prop, log_scale_cur)
  .Call(C_nngp_sufficient_step_chains, ctx, as.integer(chain_mask), nngp_covfun_id(covfun), as.matrix(covparms) + 0,
        as.double(beta_0), as.double(log_scale_prop), as.double(log_scale_cur))
nngp_field_response_ratio_chains <- function(ctx, chain_mask, beta_0, log_noise_variance)
  .Call(C_nngp_field_response_ratio_chains, ctx, as.integer(chain_mask), as.double(beta_0),
        as.double(log_noise_variance))
nngp_sum_squared_residuals_chains <- function(ctx, chain_mask, beta_0)
  .Call(C_nngp_sum_squared_residuals_chains, ctx, as.integer(chain_mask), as.double(beta_0))
# Regression block on the device (update_Gaussian.R:77-83,145-151,226-250).  Per-chain matrices
# have one column per chain.  nngp_design_set: X (n_obs x p, centred), first_obs =
# vecchia_approx$hctam_scol_1, locs_cols = X$locs (1-based); X = NULL frees the design.
nngp_design_set <- function(ctx, X, first_obs = NULL, locs_cols = integer(0))
  invisible(.Call(C_nngp_design_set, ctx, if (is.null(X)) NULL else as.matrix(X) + 0, as.integer(first_obs),
                  as.integer(locs_cols)))
# (p+1) x n_chains: crossprod(cbind(1, X), y - field[locs_match] + beta_0) per chain
nngp_design_mean_stats_chains <- function(ctx, chain_mask, beta_0, ncol_X)
  .Call(C_nngp_design_mean_stats_chains, ctx, as.integer(chain_mask), as.double(beta_0), as.integer(ncol_X))
# list(t = (p_locs+1) x n_chains, gram = (p_locs+1)^2 x n_chains, refreshed); beta_locs: p_locs x n_chains
nngp_design_interweave_stats_chains <- function(ctx, chain_mask, shift, beta_locs)
  .Call(C_nngp_design_interweave_stats_chains, ctx, as.integer(chain_mask), as.double(shift), as.matrix(beta_locs) + 0)
# field and mu updates of the chains in the mask (no host sync); beta: ncol(X) x n_chains
nngp_design_commit_chains <- function(ctx, chain_mask, shift, beta_locs_old, beta_locs_new, beta_0, beta)
  invisible(.Call(C_nngp_design_commit_chains, ctx, as.integer(chain_mask), as.double(shift),
                  if (is.null(beta_locs_old)) NULL else as.matrix(beta_locs_old) + 0,
                  if (is.null(beta_locs_new)) NULL else as.matrix(beta_locs_new) + 0, as.double(beta_0),
                  as.matrix(beta) + 0))
nngp_get_mu <- function(ctx) .Call(C_nngp_get_mu, ctx)
nngp_shard_ipc_handle <- function(ctx) .Call(C_nngp_shard_ipc_handle, ctx)
nngp_shard_ipc_open <- function(ctx, handles) invisible(.Call(C_nngp_shard_ipc_open, ctx, handles))
# collective over the ranks of a tile shard: full exchange of the replicas
# (the readers of the field refuse a stale replica)
nngp_shard_sync <- function(ctx) invisible(.Call(C_nngp_shard_sync, ctx))
nngp_sweep_chains_group <- function(ctxs, n_sweeps, beta_0, log_scale, log_noise_variance, seed, counter_base)
  invisible(.Call(C_nngp_sweep_chains_group, ctxs, as.integer(n_sweeps), as.double(beta_0), as.double(log_scale),
                  as.double(log_noise_variance), as.double(seed), as.double(counter_base)))
