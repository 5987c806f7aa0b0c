/*
 * nngp_shim.c -- R .Call shim over the C ABI of include/nngp.h.
 *
 * One .Call entry point per nngp.h function (R_registerRoutines below), so
 * the R host code of the reference (Scripts/mcmc_nngp_*.R) can drive the
 * MI355X hot path.  Conventions:
 *  - a context is an external pointer with a finalizer (nngp_ctx_destroy);
 *  - R's own arrays cross unchanged (column-major, 1-based, NA_integer_ ==
 *    INT_MIN), integers as INTSXP, reals as REALSXP; uint64 seeds / counters
 *    arrive as doubles (exact below 2^53);
 *  - a non-zero nngp_status becomes Rf_error with the context's message.
 *    The library is C/C++ behind a C ABI and has returned before Rf_error
 *    runs, so no longjmp crosses a C++ frame; temporaries are R-allocated.
 *  - HIP must not be initialised before a fork(): the R side replaces
 *    parallel::mclapply over chains (update_Gaussian.R:25-26) by contexts
 *    holding up to 4 chains each.
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <stdint.h>
#include <string.h>

#include "nngp.h"
#include "nngp_rows.h"

static SEXP ctx_tag(void) { return Rf_install("nngp_ctx"); }

/* The external pointer's protected slot: a list of kKeep + 1 entries, [k] =
 * the numeric vector bound to chain k by C_nngp_records_stream (kept alive
 * while the library may stream rows into it, whatever happens to the R
 * variables that referenced it), [kKeep] = the selected chain (INTSXP). */
#define kKeep 4

static void ctx_finalizer(SEXP p) {
  nngp_ctx* c = (nngp_ctx*)R_ExternalPtrAddr(p);
  if (c) {
    nngp_ctx_destroy(c);
    R_ClearExternalPtr(p);
  }
}

static SEXP wrap_ctx(nngp_ctx* c) {
  SEXP keep = PROTECT(Rf_allocVector(VECSXP, kKeep + 1));
  SET_VECTOR_ELT(keep, kKeep, Rf_ScalarInteger(0));  /* a new context selects chain 0 */
  SEXP p = PROTECT(R_MakeExternalPtr(c, ctx_tag(), keep));
  R_RegisterCFinalizerEx(p, ctx_finalizer, TRUE);
  UNPROTECT(2);
  return p;
}

/* the bound records vector of the selected chain (R_NilValue: none) */
static void keep_bound(SEXP p, SEXP buf) {
  SEXP keep = R_ExternalPtrProtected(p);
  if (TYPEOF(keep) != VECSXP) return;
  const int k = INTEGER(VECTOR_ELT(keep, kKeep))[0];
  if (k >= 0 && k < kKeep) SET_VECTOR_ELT(keep, k, buf);
}

static nngp_ctx* get_ctx(SEXP p) {
  if (TYPEOF(p) != EXTPTRSXP || R_ExternalPtrTag(p) != ctx_tag()) Rf_error("nngp: not a context");
  nngp_ctx* c = (nngp_ctx*)R_ExternalPtrAddr(p);
  if (!c) Rf_error("nngp: the context was destroyed");
  return c;
}

/* status -> R error (message copied first: the context may be gone after) */
static void check(int st, const nngp_ctx* c) {
  if (st == NNGP_OK) return;
  char msg[512];
  const char* m = c ? nngp_ctx_last_error(c) : NULL;
  snprintf(msg, sizeof msg, "nngp: %s%s%s", nngp_status_string(st), (m && m[0]) ? ": " : "", m ? m : "");
  Rf_error("%s (status %d)", msg, st);
}

static int as_int(SEXP x) { return Rf_asInteger(x); }
static double as_real(SEXP x) { return Rf_asReal(x); }
static const double* rptr(SEXP x) { return TYPEOF(x) == NILSXP ? NULL : REAL(x); }

static void to_u64(SEXP x, uint64_t* out, int n) {
  if (TYPEOF(x) != REALSXP || XLENGTH(x) != n) Rf_error("nngp: need %d seeds / counters (double)", n);
  for (int k = 0; k < n; ++k) out[k] = (uint64_t)REAL(x)[k];
}

/* chains of the context */
static int ctx_chains(nngp_ctx* c) {
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  return inf.n_chains;
}

/* a per-chain argument: a double vector with one entry per chain of the
 * context (the library reads every chain's entry; R's recycling does not
 * apply across the boundary) */
static const double* per_chain(SEXP x, int k, const char* what) {
  if (TYPEOF(x) != REALSXP || XLENGTH(x) != k)
    Rf_error("nngp: %s must be a double vector with one entry per chain (%d)", what, k);
  return REAL(x);
}

/* ---------- library ---------- */
SEXP C_nngp_abi_version(void) { return Rf_ScalarInteger(nngp_abi_version()); }
SEXP C_nngp_status_string(SEXP st) { return Rf_mkString(nngp_status_string(as_int(st))); }

/* ---------- graph preparation ---------- */
SEXP C_nngp_order_maxmin(SEXP locs) {
  int n = Rf_nrows(locs), d = Rf_ncols(locs);
  SEXP o = PROTECT(Rf_allocVector(INTSXP, n));
  check(nngp_order_maxmin(REAL(locs), n, d, INTEGER(o)), NULL);
  UNPROTECT(1);
  return o;
}

SEXP C_nngp_find_ordered_nn(SEXP locs, SEXP m) {
  int n = Rf_nrows(locs), d = Rf_ncols(locs), mm = as_int(m);
  SEXP nn = PROTECT(Rf_allocMatrix(INTSXP, n, mm + 1));
  check(nngp_find_ordered_nn(REAL(locs), n, d, mm, INTEGER(nn)), NULL);
  UNPROTECT(1);
  return nn;
}

SEXP C_nngp_greedy_coloring(SEXP NNarray) {
  int n = Rf_nrows(NNarray), b = Rf_ncols(NNarray), K = 0;
  SEXP col = PROTECT(Rf_allocVector(INTSXP, n));
  check(nngp_greedy_coloring(INTEGER(NNarray), n, b, INTEGER(col), &K), NULL);
  UNPROTECT(1);
  return col;
}

/* ---------- contexts ---------- */
SEXP C_nngp_ctx_create(SEXP locs, SEXP NNarray, SEXP coloring, SEXP locs_match, SEXP y, SEXP n_chains,
                       SEXP device) {
  nngp_ctx* c = NULL;
  check(nngp_ctx_create(REAL(locs), Rf_nrows(locs), Rf_ncols(locs), INTEGER(NNarray), Rf_ncols(NNarray),
                        INTEGER(coloring), INTEGER(locs_match), REAL(y), (int)XLENGTH(y), as_int(n_chains),
                        as_int(device), &c),
        NULL);
  return wrap_ctx(c);
}

SEXP C_nngp_ctx_create_shard(SEXP locs, SEXP NNarray, SEXP coloring, SEXP locs_match, SEXP y, SEXP n_chains,
                             SEXP device, SEXP n_ranks, SEXP rank) {
  nngp_ctx* c = NULL;
  check(nngp_ctx_create_shard(REAL(locs), Rf_nrows(locs), Rf_ncols(locs), INTEGER(NNarray), Rf_ncols(NNarray),
                              INTEGER(coloring), INTEGER(locs_match), REAL(y), (int)XLENGTH(y),
                              as_int(n_chains), as_int(device), as_int(n_ranks), as_int(rank), &c),
        NULL);
  return wrap_ctx(c);
}

SEXP C_nngp_ctx_destroy(SEXP p) {
  ctx_finalizer(p);
  return R_NilValue;
}

SEXP C_nngp_ctx_last_error(SEXP p) { return Rf_mkString(nngp_ctx_last_error(get_ctx(p))); }

SEXP C_nngp_set_chain(SEXP p, SEXP chain) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_set_chain(c, as_int(chain)), c);
  SEXP keep = R_ExternalPtrProtected(p);
  if (TYPEOF(keep) == VECSXP) INTEGER(VECTOR_ELT(keep, kKeep))[0] = as_int(chain);
  return R_NilValue;
}

SEXP C_nngp_ctx_engine_note(SEXP p) { return Rf_mkString(nngp_ctx_engine_note(get_ctx(p))); }

SEXP C_nngp_ctx_info(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  const char* nm[] = {"n", "b", "d", "n_obs", "n_colors", "n_levels", "nnz", "n_entries", "max_collen", "device",
                      "n_chains", "lanes_per_chain", "n_chunks", "sweep_engine", "n_tiles", "tile_rows_max",
                      "n_ghost_cells", "n_ranks", "rank", "shard_owned", "shard_needed_rows",
                      "shard_exchange_slots", "tile_ghost_pass", "tile_ghost_cells_max", "tile_r_global",
                      "tile_chain_split", "tile_resident_per_cu", "engine_fallback", "tile_exchange_wave",
                      "device_cus"};
  const double v[] = {inf.n, inf.b, inf.d, inf.n_obs, inf.n_colors, inf.n_levels, (double)inf.nnz,
                      (double)inf.n_entries, inf.max_collen, inf.device, inf.n_chains, inf.lanes_per_chain,
                      inf.n_chunks, inf.sweep_engine, inf.n_tiles, inf.tile_rows_max, (double)inf.n_ghost_cells,
                      inf.n_ranks, inf.rank, (double)inf.shard_owned, (double)inf.shard_needed_rows,
                      (double)inf.shard_exchange_slots, inf.tile_ghost_pass, inf.tile_ghost_cells_max,
                      inf.tile_r_global, inf.tile_chain_split, inf.tile_resident_per_cu, inf.engine_fallback,
                      inf.tile_exchange_wave, inf.device_cus};
  const int k = (int)(sizeof v / sizeof v[0]);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, k)), names = PROTECT(Rf_allocVector(STRSXP, k));
  for (int i = 0; i < k; ++i) {
    REAL(out)[i] = v[i];
    SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
  }
  Rf_setAttrib(out, R_NamesSymbol, names);
  UNPROTECT(2);
  return out;
}

/* ---------- factor (A4/A5) ---------- */
SEXP C_nngp_factor(SEXP p, SEXP which, SEXP covfun, SEXP covparms) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_factor(c, as_int(which), as_int(covfun), REAL(covparms), (int)XLENGTH(covparms)), c);
  return R_NilValue;
}

SEXP C_nngp_get_linv(SEXP p, SEXP which) {
  nngp_ctx* c = get_ctx(p);
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  SEXP L = PROTECT(Rf_allocMatrix(REALSXP, inf.n, inf.b));
  check(nngp_get_linv(c, as_int(which), REAL(L)), c);
  UNPROTECT(1);
  return L;
}

SEXP C_nngp_set_linv(SEXP p, SEXP which, SEXP Linv) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_set_linv(c, as_int(which), REAL(Linv)), c);
  return R_NilValue;
}

SEXP C_nngp_accept_factor(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_accept_factor(c), c);
  return R_NilValue;
}

static int ctx_n(nngp_ctx* c) {
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  return inf.n;
}

SEXP C_nngp_get_precision_diag(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  SEXP D = PROTECT(Rf_allocVector(REALSXP, ctx_n(c)));
  check(nngp_get_precision_diag(c, REAL(D)), c);
  UNPROTECT(1);
  return D;
}

/* ---------- state ---------- */
SEXP C_nngp_set_field(SEXP p, SEXP field) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_set_field(c, REAL(field)), c);
  return R_NilValue;
}

SEXP C_nngp_get_field(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  SEXP f = PROTECT(Rf_allocVector(REALSXP, ctx_n(c)));
  check(nngp_get_field(c, REAL(f)), c);
  UNPROTECT(1);
  return f;
}

SEXP C_nngp_set_mu(SEXP p, SEXP mu, SEXP beta0) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_set_mu(c, rptr(mu), as_real(beta0)), c);
  return R_NilValue;
}

SEXP C_nngp_records_reserve(SEXP p, SEXP n_rows) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_records_reserve(c, as_int(n_rows)), c);
  keep_bound(p, R_NilValue);  /* a reserve ends the binding */
  return R_NilValue;
}

SEXP C_nngp_record_field(SEXP p, SEXP row) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_record_field(c, as_int(row)), c);
  return R_NilValue;
}

/* binds (or, for NULL, releases) a numeric vector of rows x n as the
 * selected chain's streamed records (row-major); the context keeps the vector
 * alive until the binding ends (R objects do not move).  A failed call
 * leaves the binding as it was (nngp.h), so does the kept reference. */
SEXP C_nngp_records_stream(SEXP p, SEXP buf) {
  nngp_ctx* c = get_ctx(p);
  if (buf == R_NilValue) {
    check(nngp_records_stream(c, NULL, 0), c);
    keep_bound(p, R_NilValue);
    return R_NilValue;
  }
  if (TYPEOF(buf) != REALSXP || XLENGTH(buf) % ctx_n(c) != 0) Rf_error("nngp: records buffer must be a numeric vector of rows x n");
  check(nngp_records_stream(c, REAL(buf), (int)(XLENGTH(buf) / ctx_n(c))), c);
  keep_bound(p, buf);
  return R_NilValue;
}

/* rows [row0, row0 + n_rows) as an n_rows x n matrix (records$field layout).
 * buf: the vector bound by C_nngp_records_stream -- the rows are already
 * there (the call waits for them and ends the binding) and are transposed
 * straight out of it; NULL: the rows come from the device in blocks of
 * kRowBlock into one small temporary, each block transposed in turn. */
#define kRowBlock 16
SEXP C_nngp_get_records(SEXP p, SEXP row0, SEXP n_rows, SEXP buf) {
  nngp_ctx* c = get_ctx(p);
  const int n = ctx_n(c), r = as_int(n_rows), r0 = as_int(row0);
  if (r < 0 || r0 < 0) Rf_error("nngp: negative record rows");
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, r, n));
  if (buf != R_NilValue) {
    if (TYPEOF(buf) != REALSXP || XLENGTH(buf) < (R_xlen_t)(r0 + r) * n) Rf_error("nngp: records buffer too short");
    check(nngp_get_records(c, r0, r, REAL(buf) + (R_xlen_t)r0 * n), c);
    keep_bound(p, R_NilValue);
    nngp_rows_to_colmajor(REAL(buf) + (R_xlen_t)r0 * n, REAL(out), r, r, n);
  } else {
    const int blk = r < kRowBlock ? r : kRowBlock;
    SEXP tmp = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)blk * n));
    for (int i = 0; i < r; i += blk) {
      const int k = r - i < blk ? r - i : blk;
      check(nngp_get_records(c, r0 + i, k, REAL(tmp)), c);
      nngp_rows_to_colmajor(REAL(tmp), REAL(out) + i, r, k, n);
    }
    UNPROTECT(1);
  }
  UNPROTECT(1);
  return out;
}

/* ---------- kernels ---------- */
SEXP C_nngp_loglik(SEXP p, SEXP which, SEXP beta0, SEXP log_scale) {
  nngp_ctx* c = get_ctx(p);
  double ll = 0;
  check(nngp_loglik(c, as_int(which), as_real(beta0), as_real(log_scale), &ll), c);
  return Rf_ScalarReal(ll);
}

SEXP C_nngp_sweep(SEXP p, SEXP n_sweeps, SEXP beta0, SEXP log_scale, SEXP lnv, SEXP seed, SEXP counter_base,
                  SEXP z) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_sweep(c, as_int(n_sweeps), as_real(beta0), as_real(log_scale), as_real(lnv),
                   (uint64_t)as_real(seed), (uint64_t)as_real(counter_base), rptr(z)),
        c);
  return R_NilValue;
}

SEXP C_nngp_sweep_chains(SEXP p, SEXP n_sweeps, SEXP beta0, SEXP log_scale, SEXP lnv, SEXP seed,
                         SEXP counter_base) {
  nngp_ctx* c = get_ctx(p);
  uint64_t s[4], cb[4];
  const int k = ctx_chains(c);
  const double *b0 = per_chain(beta0, k, "beta0"), *ls = per_chain(log_scale, k, "log_scale"),
               *nv = per_chain(lnv, k, "log_noise_variance");
  to_u64(seed, s, k);
  to_u64(counter_base, cb, k);
  check(nngp_sweep_chains(c, as_int(n_sweeps), b0, ls, nv, s, cb), c);
  return R_NilValue;
}

SEXP C_nngp_sweep_timed(SEXP p, SEXP n_sweeps, SEXP beta0, SEXP log_scale, SEXP lnv, SEXP seed,
                        SEXP counter_base) {
  nngp_ctx* c = get_ctx(p);
  uint64_t s[4], cb[4];
  const int k = ctx_chains(c);
  const double *b0 = per_chain(beta0, k, "beta0"), *ls = per_chain(log_scale, k, "log_scale"),
               *nv = per_chain(lnv, k, "log_noise_variance");
  to_u64(seed, s, k);
  to_u64(counter_base, cb, k);
  double ms = 0, kms = 0;
  check(nngp_sweep_timed(c, as_int(n_sweeps), b0, ls, nv, s, cb, &ms, &kms), c);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 2));
  REAL(out)[0] = ms;
  REAL(out)[1] = kms;
  UNPROTECT(1);
  return out;
}

SEXP C_nngp_ancillary_propose(SEXP p, SEXP beta0, SEXP dlog_scale) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_ancillary_propose(c, as_real(beta0), as_real(dlog_scale)), c);
  return R_NilValue;
}

SEXP C_nngp_ancillary_propose_chains(SEXP p, SEXP chain_mask, SEXP beta0, SEXP dlog_scale) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  check(nngp_ancillary_propose_chains(c, as_int(chain_mask), per_chain(beta0, k, "beta0"),
                                      per_chain(dlog_scale, k, "dlog_scale")),
        c);
  return R_NilValue;
}

SEXP C_nngp_field_response_ratio(SEXP p, SEXP beta0, SEXP lnv) {
  nngp_ctx* c = get_ctx(p);
  double r = 0;
  check(nngp_field_response_ratio(c, as_real(beta0), as_real(lnv), &r), c);
  return Rf_ScalarReal(r);
}

SEXP C_nngp_accept_field(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_accept_field(c), c);
  return R_NilValue;
}

SEXP C_nngp_beta0_stats(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 2));
  check(nngp_beta0_stats(c, REAL(out), REAL(out) + 1), c);
  UNPROTECT(1);
  return out;
}

SEXP C_nngp_sum_squared_residuals(SEXP p, SEXP beta0) {
  nngp_ctx* c = get_ctx(p);
  double ssr = 0;
  check(nngp_sum_squared_residuals(c, as_real(beta0), &ssr), c);
  return Rf_ScalarReal(ssr);
}

SEXP C_nngp_spmv(SEXP p, SEXP which, SEXP X) {
  nngp_ctx* c = get_ctx(p);
  const int n = ctx_n(c);
  const int ncols = Rf_isMatrix(X) ? Rf_ncols(X) : 1;
  if ((Rf_isMatrix(X) ? Rf_nrows(X) : (int)XLENGTH(X)) != n) Rf_error("nngp_spmv: X must have n rows");
  SEXP Y = PROTECT(Rf_isMatrix(X) ? Rf_allocMatrix(REALSXP, n, ncols) : Rf_allocVector(REALSXP, n));
  check(nngp_spmv(c, as_int(which), REAL(X), ncols, REAL(Y)), c);
  UNPROTECT(1);
  return Y;
}

SEXP C_nngp_tri_solve(SEXP p, SEXP which, SEXP u) {
  nngp_ctx* c = get_ctx(p);
  SEXP x = PROTECT(Rf_allocVector(REALSXP, ctx_n(c)));
  check(nngp_tri_solve(c, as_int(which), REAL(u), REAL(x)), c);
  UNPROTECT(1);
  return x;
}

SEXP C_nngp_tri_rescues(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  long long k = 0;
  check(nngp_tri_rescues(c, &k), c);
  return Rf_ScalarReal((double)k);
}

SEXP C_nngp_device_normals(SEXP device, SEXP seed, SEXP sweep, SEXP n) {
  SEXP z = PROTECT(Rf_allocVector(REALSXP, as_int(n)));
  check(nngp_device_normals(as_int(device), (uint64_t)as_real(seed), (uint64_t)as_real(sweep), as_int(n), REAL(z)),
        NULL);
  UNPROTECT(1);
  return z;
}

/* get_summary (estimate.R:1-6) of an S x n matrix of samples on the device:
 * the column-major R matrix is brought to S row-major rows of n (the blocked
 * transpose of nngp_rows.h, reading it as n row-major rows of S) and passed
 * as one block; -> n x 5 with the reference's column names. */
SEXP C_nngp_summary(SEXP device, SEXP samples) {
  if (TYPEOF(samples) != REALSXP || !Rf_isMatrix(samples)) Rf_error("nngp: samples must be a numeric matrix");
  const int S = Rf_nrows(samples), n = Rf_ncols(samples);
  static const char* names[5] = {"mean", "q0.025", "median", "q0.975", "sd"};
  SEXP rows = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)S * n));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, 5));
  nngp_rows_to_colmajor(REAL(samples), REAL(rows), n, n, S);
  const double* block = REAL(rows);
  const long long block_rows = S;
  check(nngp_summary(as_int(device), &block, &block_rows, 1, n, NULL, 0, REAL(out)), NULL);
  SEXP cn = PROTECT(Rf_allocVector(STRSXP, 5));
  for (int i = 0; i < 5; ++i) SET_STRING_ELT(cn, i, Rf_mkChar(names[i]));
  SEXP dn = PROTECT(Rf_allocVector(VECSXP, 2));
  SET_VECTOR_ELT(dn, 1, cn);
  Rf_setAttrib(out, Rf_install("dimnames"), dn);
  UNPROTECT(4);
  return out;
}

/* The same with chosen quantiles and exceedance probabilities
 * (nngp_summary_probs): probs and thresholds are numeric vectors (length 0
 * allowed); -> n x (2 + length(probs) + length(thresholds)): mean, the
 * quantiles in the order of probs, sd, P(x > thresholds[k]).  The R wrapper
 * names the columns. */
SEXP C_nngp_summary_probs(SEXP device, SEXP samples, SEXP probs, SEXP thresholds) {
  if (TYPEOF(samples) != REALSXP || !Rf_isMatrix(samples)) Rf_error("nngp: samples must be a numeric matrix");
  if (TYPEOF(probs) != REALSXP || TYPEOF(thresholds) != REALSXP) Rf_error("nngp: probs and thresholds must be numeric");
  const int S = Rf_nrows(samples), n = Rf_ncols(samples);
  const int n_probs = (int)XLENGTH(probs), n_thr = (int)XLENGTH(thresholds);
  if (n_probs > 16 || n_thr > 8) Rf_error("nngp: at most 16 probs and 8 thresholds");
  SEXP rows = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)S * n));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, 2 + n_probs + n_thr));
  nngp_rows_to_colmajor(REAL(samples), REAL(rows), n, n, S);
  const double* block = REAL(rows);
  const long long block_rows = S;
  check(nngp_summary_probs(as_int(device), &block, &block_rows, 1, n, NULL, 0, n_probs ? REAL(probs) : NULL, n_probs,
                           n_thr ? REAL(thresholds) : NULL, n_thr, REAL(out)),
        NULL);
  UNPROTECT(2);
  return out;
}

/* the last summary's HIP-event times (ms), staged bytes and chunk width */
SEXP C_nngp_summary_stats(void) {
  static const char* names[4] = {"copy_ms", "kernel_ms", "staged_bytes", "chunk_cols"};
  double copy_ms = 0, kernel_ms = 0;
  long long bytes = 0;
  int cols = 0;
  check(nngp_summary_stats(&copy_ms, &kernel_ms, &bytes, &cols), NULL);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 4));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 4));
  REAL(out)[0] = copy_ms;
  REAL(out)[1] = kernel_ms;
  REAL(out)[2] = (double)bytes;
  REAL(out)[3] = (double)cols;
  for (int i = 0; i < 4; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

/* The summary of coef %*% t(X) (+ addend) (+ noise) per location with the
 * samples generated on the device (nngp_effects_summary; predict.R:92-102):
 * coef S x q and X n x q as R holds them; addend_t NULL or n x S, the TRANSPOSE
 * of the S x n addend, so that R's column-major storage is the S row-major
 * rows of n the library reads where they lie; noise_sd NULL or S values with
 * seed and counter (S doubles); probs and thresholds numeric vectors (length 0
 * allowed).  -> n x (2 + length(probs) + length(thresholds)); the R wrapper
 * names the columns. */
SEXP C_nngp_effects_summary(SEXP device, SEXP coef, SEXP X, SEXP addend_t, SEXP noise_sd, SEXP seed, SEXP counter,
                            SEXP probs, SEXP thresholds) {
  if (TYPEOF(coef) != REALSXP || !Rf_isMatrix(coef) || TYPEOF(X) != REALSXP || !Rf_isMatrix(X))
    Rf_error("nngp: effects_summary: coef and X must be numeric matrices");
  if (TYPEOF(probs) != REALSXP || TYPEOF(thresholds) != REALSXP) Rf_error("nngp: probs and thresholds must be numeric");
  const int S = Rf_nrows(coef), q = Rf_ncols(coef), n = Rf_nrows(X);
  const int n_probs = (int)XLENGTH(probs), n_thr = (int)XLENGTH(thresholds);
  if (Rf_ncols(X) != q) Rf_error("nngp: effects_summary: coef and X differ in columns");
  if (n_probs > 16 || n_thr > 8) Rf_error("nngp: at most 16 probs and 8 thresholds");
  const int has_add = TYPEOF(addend_t) != NILSXP, has_noise = TYPEOF(noise_sd) != NILSXP;
  if (has_add && (TYPEOF(addend_t) != REALSXP || !Rf_isMatrix(addend_t) || Rf_nrows(addend_t) != n ||
                  Rf_ncols(addend_t) != S))
    Rf_error("nngp: effects_summary: the addend must be S x n");
  if (has_noise && (TYPEOF(noise_sd) != REALSXP || XLENGTH(noise_sd) != S))
    Rf_error("nngp: effects_summary: noise_sd needs one value per sample");
  /* 8-byte scratch in an R vector (released with the call, also on an R error) */
  SEXP ctr_s = PROTECT(Rf_allocVector(REALSXP, has_noise ? S : 1));
  uint64_t* ctr = NULL;
  if (has_noise) {
    ctr = (uint64_t*)(void*)REAL(ctr_s);
    to_u64(counter, ctr, S);
  }
  const double* block = has_add ? REAL(addend_t) : NULL;
  const long long block_rows = S;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, 2 + n_probs + n_thr));
  check(nngp_effects_summary(as_int(device), REAL(coef), S, q, REAL(X), n, has_add ? &block : NULL,
                             has_add ? &block_rows : NULL, has_add ? 1 : 0, has_noise ? REAL(noise_sd) : NULL,
                             has_noise ? (uint64_t)as_real(seed) : 0, ctr, 0, n_probs ? REAL(probs) : NULL, n_probs,
                             n_thr ? REAL(thresholds) : NULL, n_thr, REAL(out), NULL),
        NULL);
  UNPROTECT(2);
  return out;
}

/* the last effects summary's HIP-event times (ms), staged bytes and chunk width */
SEXP C_nngp_effects_stats(void) {
  static const char* names[5] = {"copy_ms", "generate_ms", "kernel_ms", "staged_bytes", "chunk_cols"};
  double v[3] = {0, 0, 0};
  long long bytes = 0;
  int cols = 0;
  check(nngp_effects_stats(&v[0], &v[1], &v[2], &bytes, &cols), NULL);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 5));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 5));
  for (int i = 0; i < 3; ++i) REAL(out)[i] = v[i];
  REAL(out)[3] = (double)bytes;
  REAL(out)[4] = (double)cols;
  for (int i = 0; i < 5; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

/* The pointwise Gaussian log-likelihood of the saved samples reduced per
 * observation (nngp_pointwise_loglik; the dnorm terms of
 * update_Gaussian.R:130-131,281): y (n_obs) and obs_loc (n_obs integers,
 * 1-based, non-decreasing: the R wrapper sorts); coef NULL or S x q with X
 * n_obs x q as R holds them; field_t n x S, the TRANSPOSE of the S x n field
 * samples, so that R's column-major storage is the S row-major rows of n the
 * library reads where they lie; log_noise_var S values.  -> n_obs x 6; the R
 * wrapper names the columns and restores the caller's order. */
SEXP C_nngp_pointwise_loglik(SEXP device, SEXP y, SEXP obs_loc, SEXP coef, SEXP X, SEXP field_t, SEXP log_noise_var) {
  if (TYPEOF(y) != REALSXP || TYPEOF(obs_loc) != INTSXP || XLENGTH(y) != XLENGTH(obs_loc) || XLENGTH(y) < 1)
    Rf_error("nngp: pointwise_loglik: y must be numeric and obs_loc integer, of one length");
  if (TYPEOF(field_t) != REALSXP || !Rf_isMatrix(field_t) || TYPEOF(log_noise_var) != REALSXP)
    Rf_error("nngp: pointwise_loglik: the field must be a numeric matrix and log_noise_var numeric");
  const long long n_obs = (long long)XLENGTH(y);
  const int n = Rf_nrows(field_t), S = Rf_ncols(field_t);
  if (XLENGTH(log_noise_var) != S) Rf_error("nngp: pointwise_loglik: log_noise_var needs one value per sample");
  const int has_q = TYPEOF(coef) != NILSXP;
  int q = 0;
  if (has_q) {
    if (TYPEOF(coef) != REALSXP || !Rf_isMatrix(coef) || TYPEOF(X) != REALSXP || !Rf_isMatrix(X))
      Rf_error("nngp: pointwise_loglik: coef and X must be numeric matrices");
    q = Rf_ncols(coef);
    if (Rf_nrows(coef) != S || Rf_ncols(X) != q || Rf_nrows(X) != n_obs)
      Rf_error("nngp: pointwise_loglik: coef must be S x q and X n_obs x q");
  }
  const double* block = REAL(field_t);
  const long long block_rows = S;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)n_obs, 6));
  check(nngp_pointwise_loglik(as_int(device), REAL(y), n_obs, INTEGER(obs_loc), q ? REAL(coef) : NULL, S, q,
                              q ? REAL(X) : NULL, &block, &block_rows, 1, n, REAL(log_noise_var), 0, REAL(out)),
        NULL);
  UNPROTECT(1);
  return out;
}

/* the last pointwise log-likelihood's HIP-event times (ms), staged bytes and chunk width */
SEXP C_nngp_pointwise_loglik_stats(void) {
  static const char* names[4] = {"copy_ms", "kernel_ms", "staged_bytes", "chunk_cols"};
  double v[2] = {0, 0};
  long long bytes = 0;
  int cols = 0;
  check(nngp_pointwise_loglik_stats(&v[0], &v[1], &bytes, &cols), NULL);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 4));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 4));
  REAL(out)[0] = v[0];
  REAL(out)[1] = v[1];
  REAL(out)[2] = (double)bytes;
  REAL(out)[3] = (double)cols;
  for (int i = 0; i < 4; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

/* Per-location R-hat and effective sample size of the field samples
 * (Scripts/mcmc_nngp_diagnose.R:1-24,107-118).  chains_t: a list with one
 * n x S numeric matrix per chain, the TRANSPOSE of its S saved rows x n
 * locations, so that R's column-major storage is the S row-major rows of n the
 * library reads where they lie; -> n x 5 with named columns. */
SEXP C_nngp_field_diag(SEXP device, SEXP chains_t) {
  if (TYPEOF(chains_t) != VECSXP || XLENGTH(chains_t) < 1 || XLENGTH(chains_t) > 16)
    Rf_error("nngp: chains must be a list of 1 to 16 numeric matrices");
  const int m = (int)XLENGTH(chains_t);
  const double* blocks[16];
  int n = 0, S = 0;
  for (int k = 0; k < m; ++k) {
    SEXP x = VECTOR_ELT(chains_t, k);
    if (TYPEOF(x) != REALSXP || !Rf_isMatrix(x)) Rf_error("nngp: every chain must be a numeric matrix");
    if (k == 0) {
      n = Rf_nrows(x);
      S = Rf_ncols(x);
    } else if (Rf_nrows(x) != n || Rf_ncols(x) != S) {
      Rf_error("nngp: the chains' matrices must have one shape");
    }
    blocks[k] = REAL(x);
  }
  static const char* names[5] = {"R_hat", "ess", "ess_min", "W", "Bv"};
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, 5));
  check(nngp_field_diag(as_int(device), blocks, m, S, n, NULL, 0, REAL(out), NULL), NULL);
  SEXP cn = PROTECT(Rf_allocVector(STRSXP, 5));
  for (int i = 0; i < 5; ++i) SET_STRING_ELT(cn, i, Rf_mkChar(names[i]));
  SEXP dn = PROTECT(Rf_allocVector(VECSXP, 2));
  SET_VECTOR_ELT(dn, 1, cn);
  Rf_setAttrib(out, Rf_install("dimnames"), dn);
  UNPROTECT(3);
  return out;
}

/* the last field diagnostics' HIP-event times (ms), staged bytes and chunk width */
SEXP C_nngp_field_diag_stats(void) {
  static const char* names[4] = {"copy_ms", "kernel_ms", "staged_bytes", "chunk_cols"};
  double copy_ms = 0, kernel_ms = 0;
  long long bytes = 0;
  int cols = 0;
  check(nngp_field_diag_stats(&copy_ms, &kernel_ms, &bytes, &cols), NULL);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 4));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 4));
  REAL(out)[0] = copy_ms;
  REAL(out)[1] = kernel_ms;
  REAL(out)[2] = (double)bytes;
  REAL(out)[3] = (double)cols;
  for (int i = 0; i < 4; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

/* nngp_predict_field for one chain (Scripts/mcmc_nngp_predict.R:39-53 for all of
 * its saved samples).  locs N x d and NNarray N x b as R holds them.  The
 * per-sample matrices come TRANSPOSED from the R side, so that R's column-major
 * storage is the row-major layout of the C ABI with no copy here:
 * covparms_t ncovparms x n_factors, fields_t n x n_samples (column s = the field
 * of sample s: the wrapper gathers the chain's saved rows with
 * t(field[rows, ])), z_t n_pred x n_samples or NULL (Philox: seed, counter).
 * -> n_pred x n_samples (the wrapper transposes back). */
SEXP C_nngp_predict_field(SEXP device, SEXP locs, SEXP n, SEXP NNarray, SEXP covfun, SEXP covparms_t, SEXP factor_of,
                          SEXP fields_t, SEXP beta0, SEXP log_scale, SEXP z_t, SEXP seed, SEXP counter,
                          SEXP sample_batch) {
  if (TYPEOF(locs) != REALSXP || !Rf_isMatrix(locs) || TYPEOF(NNarray) != INTSXP || !Rf_isMatrix(NNarray) ||
      TYPEOF(covparms_t) != REALSXP || !Rf_isMatrix(covparms_t) || TYPEOF(fields_t) != REALSXP ||
      !Rf_isMatrix(fields_t) || TYPEOF(factor_of) != INTSXP || TYPEOF(beta0) != REALSXP || TYPEOF(log_scale) != REALSXP)
    Rf_error("nngp: predict_field: wrong argument types");
  const int N = Rf_nrows(locs), d = Rf_ncols(locs), nobs = as_int(n), n_pred = N - nobs;
  const int S = Rf_ncols(fields_t);
  if (Rf_nrows(NNarray) != N || Rf_nrows(fields_t) != nobs || XLENGTH(factor_of) != S || XLENGTH(beta0) != S ||
      XLENGTH(log_scale) != S || n_pred < 1 || S < 1)
    Rf_error("nngp: predict_field: sizes do not match");
  const int philox = TYPEOF(z_t) == NILSXP;
  if (!philox && (TYPEOF(z_t) != REALSXP || !Rf_isMatrix(z_t) || Rf_nrows(z_t) != n_pred || Rf_ncols(z_t) != S))
    Rf_error("nngp: predict_field: z must be n_pred x n_samples");
  /* 8-byte scratch in R vectors (released with the call, also on an R error) */
  SEXP rows_s = PROTECT(Rf_allocVector(REALSXP, S));
  SEXP ctr_s = PROTECT(Rf_allocVector(REALSXP, S));
  long long* rows = (long long*)(void*)REAL(rows_s);
  uint64_t* ctr = NULL;
  for (int s = 0; s < S; ++s) rows[s] = s;
  if (philox) {
    ctr = (uint64_t*)(void*)REAL(ctr_s);
    to_u64(counter, ctr, S);
  }
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n_pred, S));
  int fail_row = 0;
  const int st = nngp_predict_field(as_int(device), REAL(locs), nobs, n_pred, d, INTEGER(NNarray), Rf_ncols(NNarray),
                                    as_int(covfun), REAL(covparms_t), Rf_nrows(covparms_t), Rf_ncols(covparms_t), S,
                                    INTEGER(factor_of), REAL(fields_t), nobs, rows, REAL(beta0), REAL(log_scale),
                                    philox ? NULL : REAL(z_t), (uint64_t)as_real(seed), ctr, as_int(sample_batch),
                                    REAL(out), &fail_row);
  if (st == NNGP_ERR_CHOL)
    Rf_error("nngp: local covariance of stacked row %d is not positive definite (status %d)", fail_row, st);
  check(st, NULL);
  UNPROTECT(3);
  return out;
}

/* the last prediction's plan / factor / solve times (ms), staged bytes and batch size */
SEXP C_nngp_predict_stats(void) {
  static const char* names[5] = {"plan_ms", "factor_ms", "solve_ms", "staged_bytes", "sample_batch"};
  double v[3] = {0, 0, 0};
  long long bytes = 0;
  int batch = 0;
  check(nngp_predict_stats(&v[0], &v[1], &v[2], &bytes, &batch), NULL);
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 5));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 5));
  for (int i = 0; i < 3; ++i) REAL(out)[i] = v[i];
  REAL(out)[3] = (double)bytes;
  REAL(out)[4] = (double)batch;
  for (int i = 0; i < 5; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

SEXP C_nngp_get_sweep_r(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  SEXP r = PROTECT(Rf_allocVector(REALSXP, ctx_n(c)));
  check(nngp_get_sweep_r(c, REAL(r)), c);
  UNPROTECT(1);
  return r;
}

/* ---------- sharded sweep (colour shard / tile shard) ---------- */
SEXP C_nngp_shard_unique_id(void) {
  SEXP id = PROTECT(Rf_allocVector(RAWSXP, NNGP_SHARD_ID_BYTES));
  check(nngp_shard_unique_id(RAW(id), NNGP_SHARD_ID_BYTES), NULL);
  UNPROTECT(1);
  return id;
}

SEXP C_nngp_shard_comm_init(SEXP p, SEXP id) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_shard_comm_init(c, RAW(id), (int)XLENGTH(id)), c);
  return R_NilValue;
}

SEXP C_nngp_sweep_chains_group(SEXP ctxs, SEXP n_sweeps, SEXP beta0, SEXP log_scale, SEXP lnv, SEXP seed,
                               SEXP counter_base) {
  const int G = (int)XLENGTH(ctxs);
  if (G < 1 || G > 64) Rf_error("nngp: 1..64 ranks");
  nngp_ctx* cs[64];
  for (int g = 0; g < G; ++g) cs[g] = get_ctx(VECTOR_ELT(ctxs, g));
  uint64_t s[4], cb[4];
  const int k = ctx_chains(cs[0]);
  const double *b0 = per_chain(beta0, k, "beta0"), *ls = per_chain(log_scale, k, "log_scale"),
               *nv = per_chain(lnv, k, "log_noise_variance");
  to_u64(seed, s, k);
  to_u64(counter_base, cb, k);
  check(nngp_sweep_chains_group(cs, G, as_int(n_sweeps), b0, ls, nv, s, cb), cs[0]);
  return R_NilValue;
}

/* tile shard: HIP IPC handle of this rank's granule buffer (a raw vector the
   ranks exchange out of band), and the mapping of the others' (list of raws) */
SEXP C_nngp_shard_ipc_handle(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  SEXP h = PROTECT(Rf_allocVector(RAWSXP, NNGP_IPC_HANDLE_BYTES));
  check(nngp_shard_ipc_handle(c, RAW(h), NNGP_IPC_HANDLE_BYTES), c);
  UNPROTECT(1);
  return h;
}

SEXP C_nngp_shard_sync(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  check(nngp_shard_sync(c), c);
  return R_NilValue;
}

SEXP C_nngp_shard_ipc_open(SEXP p, SEXP handles) {
  nngp_ctx* c = get_ctx(p);
  const int G = (int)XLENGTH(handles);
  if (G < 1 || G > 16) Rf_error("nngp: 1..16 ranks in a tile shard");
  unsigned char buf[16 * NNGP_IPC_HANDLE_BYTES];
  for (int g = 0; g < G; ++g) {
    SEXP h = VECTOR_ELT(handles, g);
    if (TYPEOF(h) != RAWSXP || XLENGTH(h) != NNGP_IPC_HANDLE_BYTES) Rf_error("nngp: IPC handles must be raw(%d)", NNGP_IPC_HANDLE_BYTES);
    memcpy(buf + (size_t)g * NNGP_IPC_HANDLE_BYTES, RAW(h), NNGP_IPC_HANDLE_BYTES);
  }
  check(nngp_shard_ipc_open(c, buf, NNGP_IPC_HANDLE_BYTES), c);
  return R_NilValue;
}

/* ---------- batched per-chain forms (one host sync for all chains) ---------- */
SEXP C_nngp_factor_chains(SEXP p, SEXP which, SEXP mask, SEXP covfun, SEXP covparms) {
  nngp_ctx* c = get_ctx(p);
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  /* covparms: n_chains x ncovparms matrix (row k = chain k), column-major in R */
  const int k = inf.n_chains, ncp = Rf_ncols(covparms);
  if (Rf_nrows(covparms) != k) Rf_error("nngp: covparms needs one row per chain");
  double rm[4 * 16];
  if (ncp > 16) Rf_error("nngp: at most 16 covariance parameters");
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < ncp; ++j) rm[i * ncp + j] = REAL(covparms)[i + (size_t)j * k];
  SEXP st = PROTECT(Rf_allocVector(INTSXP, k));
  for (int i = 0; i < k; ++i) INTEGER(st)[i] = 0;
  const int rc = nngp_factor_chains(c, as_int(which), as_int(mask), as_int(covfun), rm, ncp, INTEGER(st));
  UNPROTECT(1);
  check(rc, c);
  return st;
}

/* covparms: n_chains x ncovparms matrix (row k = chain k) -> row-major rm */
static int covparms_rows(nngp_ctx* c, SEXP covparms, double* rm) {
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  const int k = inf.n_chains, ncp = Rf_ncols(covparms);
  if (Rf_nrows(covparms) != k) Rf_error("nngp: covparms needs one row per chain");
  if (ncp > 16) Rf_error("nngp: at most 16 covariance parameters");
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < ncp; ++j) rm[i * ncp + j] = REAL(covparms)[i + (size_t)j * k];
  return ncp;
}

static SEXP named_list(int n, SEXP* v, const char** names) {
  SEXP out = PROTECT(Rf_allocVector(VECSXP, n));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, n));
  for (int i = 0; i < n; ++i) {
    SET_VECTOR_ELT(out, i, v[i]);
    SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  }
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

static SEXP chains_out(nngp_ctx* c) {
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  return Rf_allocVector(REALSXP, inf.n_chains);
}

SEXP C_nngp_loglik_chains(SEXP p, SEXP which, SEXP mask, SEXP beta0, SEXP log_scale) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  const double *b0 = per_chain(beta0, k, "beta0"), *ls = per_chain(log_scale, k, "log_scale");
  SEXP out = PROTECT(chains_out(c));
  const int rc = nngp_loglik_chains(c, as_int(which), as_int(mask), b0, ls, REAL(out));
  UNPROTECT(1);
  check(rc, c);
  return out;
}

SEXP C_nngp_loglik_pair_chains(SEXP p, SEXP mask, SEXP beta0, SEXP ls_prop, SEXP ls_cur) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  const double *b0 = per_chain(beta0, k, "beta0"), *lp = per_chain(ls_prop, k, "log_scale_prop"),
               *lc = per_chain(ls_cur, k, "log_scale_cur");
  SEXP prop = PROTECT(chains_out(c));
  SEXP cur = PROTECT(chains_out(c));
  const int rc = nngp_loglik_pair_chains(c, as_int(mask), b0, lp, lc, REAL(prop), REAL(cur));
  if (rc) {
    UNPROTECT(2);
    check(rc, c);
  }
  SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 2));
  SET_VECTOR_ELT(out, 0, prop);
  SET_VECTOR_ELT(out, 1, cur);
  SET_STRING_ELT(nm, 0, Rf_mkChar("proposal"));
  SET_STRING_ELT(nm, 1, Rf_mkChar("current"));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(4);
  return out;
}

SEXP C_nngp_field_response_ratio_chains(SEXP p, SEXP mask, SEXP beta0, SEXP lnv) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  const double *b0 = per_chain(beta0, k, "beta0"), *nv = per_chain(lnv, k, "log_noise_variance");
  SEXP out = PROTECT(chains_out(c));
  const int rc = nngp_field_response_ratio_chains(c, as_int(mask), b0, nv, REAL(out));
  UNPROTECT(1);
  check(rc, c);
  return out;
}

SEXP C_nngp_sum_squared_residuals_chains(SEXP p, SEXP mask, SEXP beta0) {
  nngp_ctx* c = get_ctx(p);
  const double* b0 = per_chain(beta0, ctx_chains(c), "beta0");
  SEXP out = PROTECT(chains_out(c));
  const int rc = nngp_sum_squared_residuals_chains(c, as_int(mask), b0, REAL(out));
  UNPROTECT(1);
  check(rc, c);
  return out;
}

/* ---------- regression block (nngp_design_*) ----------
 * Per-chain matrix arguments and results have one COLUMN per chain: a
 * column-major width x n_chains R matrix is the ABI's n_chains x width rows. */
static const double* chain_cols(SEXP x, int width, int k, const char* what) {
  if (TYPEOF(x) != REALSXP || XLENGTH(x) != (R_xlen_t)width * k)
    Rf_error("nngp: %s must be a double matrix of %d rows with one column per chain (%d)", what, width, k);
  return REAL(x);
}

SEXP C_nngp_design_set(SEXP p, SEXP X, SEXP first_obs, SEXP locs_cols) {
  nngp_ctx* c = get_ctx(p);
  if (TYPEOF(X) == NILSXP) {
    check(nngp_design_set(c, NULL, 0, NULL, NULL, 0), c);
    return R_NilValue;
  }
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  if (TYPEOF(X) != REALSXP || !Rf_isMatrix(X) || Rf_nrows(X) != inf.n_obs)
    Rf_error("nngp: X must be a double matrix with one row per observation (%d)", inf.n_obs);
  if (TYPEOF(first_obs) != INTSXP || XLENGTH(first_obs) != inf.n || TYPEOF(locs_cols) != INTSXP)
    Rf_error("nngp: first_obs must be an integer vector with one entry per location (%d), locs_cols integer", inf.n);
  const int pl = (int)XLENGTH(locs_cols);
  check(nngp_design_set(c, REAL(X), Rf_ncols(X), INTEGER(first_obs), pl ? INTEGER(locs_cols) : NULL, pl), c);
  return R_NilValue;
}

SEXP C_nngp_design_mean_stats_chains(SEXP p, SEXP mask, SEXP beta0, SEXP ncol_X) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c), nv = as_int(ncol_X) + 1;
  const double* b0 = per_chain(beta0, k, "beta0");
  if (nv < 2) Rf_error("nngp: ncol(X) >= 1");
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, nv, k));
  memset(REAL(out), 0, sizeof(double) * (size_t)nv * k);
  const int rc = nngp_design_mean_stats_chains(c, as_int(mask), b0, REAL(out));
  UNPROTECT(1);
  check(rc, c);
  return out;
}

SEXP C_nngp_design_interweave_stats_chains(SEXP p, SEXP mask, SEXP shift, SEXP beta_locs) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  if (!Rf_isMatrix(beta_locs) || Rf_nrows(beta_locs) < 1) Rf_error("nngp: beta_locs must be a p_locs x n_chains matrix");
  const int q = Rf_nrows(beta_locs) + 1;
  const double *sh = per_chain(shift, k, "shift"), *bl = chain_cols(beta_locs, q - 1, k, "beta_locs");
  SEXP t = PROTECT(Rf_allocMatrix(REALSXP, q, k));
  SEXP gram = PROTECT(Rf_allocMatrix(REALSXP, q * q, k));
  SEXP refreshed = PROTECT(Rf_allocVector(INTSXP, k));
  memset(REAL(t), 0, sizeof(double) * (size_t)q * k);
  memset(REAL(gram), 0, sizeof(double) * (size_t)q * q * k);
  for (int i = 0; i < k; ++i) INTEGER(refreshed)[i] = 0;
  const int rc = nngp_design_interweave_stats_chains(c, as_int(mask), sh, bl, REAL(t), REAL(gram), INTEGER(refreshed));
  if (rc) {
    UNPROTECT(3);
    check(rc, c);
  }
  SEXP v[3] = {t, gram, refreshed};
  const char* nm[3] = {"t", "gram", "refreshed"};
  SEXP out = named_list(3, v, nm);
  UNPROTECT(3);
  return out;
}

SEXP C_nngp_design_commit_chains(SEXP p, SEXP mask, SEXP shift, SEXP beta_locs_old, SEXP beta_locs_new, SEXP beta0,
                                 SEXP beta) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  if (!Rf_isMatrix(beta)) Rf_error("nngp: beta must be a ncol(X) x n_chains matrix");
  const int pl = TYPEOF(beta_locs_old) == NILSXP ? 0 : Rf_nrows(beta_locs_old);
  const double *sh = per_chain(shift, k, "shift"), *b0 = per_chain(beta0, k, "beta0");
  const double* bo = pl ? chain_cols(beta_locs_old, pl, k, "beta_locs_old") : NULL;
  const double* bn = pl ? chain_cols(beta_locs_new, pl, k, "beta_locs_new") : NULL;
  const double* b = chain_cols(beta, Rf_nrows(beta), k, "beta");
  check(nngp_design_commit_chains(c, as_int(mask), sh, bo, bn, b0, b), c);
  return R_NilValue;
}

SEXP C_nngp_get_mu(SEXP p) {
  nngp_ctx* c = get_ctx(p);
  nngp_info inf;
  check(nngp_ctx_info(c, &inf), c);
  SEXP mu = PROTECT(Rf_allocVector(REALSXP, inf.n_obs));
  const int rc = nngp_get_mu(c, REAL(mu));
  UNPROTECT(1);
  check(rc, c);
  return mu;
}

/* ---------- registration ---------- */
#define E(name, n) {#name, (DL_FUNC)&name, n}
SEXP C_nngp_ancillary_step_chains(SEXP p, SEXP mask, SEXP covfun, SEXP covparms, SEXP beta0, SEXP dls, SEXP lnv) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  double rm[4 * 16];
  const int ncp = covparms_rows(c, covparms, rm);
  const double *b0 = per_chain(beta0, k, "beta0"), *dl = per_chain(dls, k, "dlog_scale"),
               *lv = per_chain(lnv, k, "log_noise_variance");
  SEXP st = PROTECT(Rf_allocVector(INTSXP, k));
  SEXP ratio = PROTECT(chains_out(c));
  for (int i = 0; i < k; ++i) INTEGER(st)[i] = 0;
  const int rc = nngp_ancillary_step_chains(c, as_int(mask), as_int(covfun), rm, ncp, b0, dl, lv, INTEGER(st),
                                            REAL(ratio));
  if (rc) {
    UNPROTECT(2);
    check(rc, c);
  }
  SEXP v[2] = {st, ratio};
  const char* nm[2] = {"status", "ratio"};
  SEXP out = named_list(2, v, nm);
  UNPROTECT(2);
  return out;
}

SEXP C_nngp_sufficient_step_chains(SEXP p, SEXP mask, SEXP covfun, SEXP covparms, SEXP beta0, SEXP ls_prop,
                                   SEXP ls_cur) {
  nngp_ctx* c = get_ctx(p);
  const int k = ctx_chains(c);
  double rm[4 * 16];
  const int ncp = covparms_rows(c, covparms, rm);
  const double *b0 = per_chain(beta0, k, "beta0"), *lp = per_chain(ls_prop, k, "log_scale_prop"),
               *lc = per_chain(ls_cur, k, "log_scale_cur");
  SEXP st = PROTECT(Rf_allocVector(INTSXP, k));
  SEXP prop = PROTECT(chains_out(c));
  SEXP cur = PROTECT(chains_out(c));
  for (int i = 0; i < k; ++i) INTEGER(st)[i] = 0;
  const int rc = nngp_sufficient_step_chains(c, as_int(mask), as_int(covfun), rm, ncp, b0, lp, lc, INTEGER(st),
                                             REAL(prop), REAL(cur));
  if (rc) {
    UNPROTECT(3);
    check(rc, c);
  }
  SEXP v[3] = {st, prop, cur};
  const char* nm[3] = {"status", "proposal", "current"};
  SEXP out = named_list(3, v, nm);
  UNPROTECT(3);
  return out;
}

static const R_CallMethodDef call_methods[] = {
    E(C_nngp_abi_version, 0),
    E(C_nngp_status_string, 1),
    E(C_nngp_order_maxmin, 1),
    E(C_nngp_find_ordered_nn, 2),
    E(C_nngp_greedy_coloring, 1),
    E(C_nngp_ctx_create, 7),
    E(C_nngp_ctx_create_shard, 9),
    E(C_nngp_ctx_destroy, 1),
    E(C_nngp_ctx_last_error, 1),
    E(C_nngp_set_chain, 2),
    E(C_nngp_ctx_info, 1),
    E(C_nngp_ctx_engine_note, 1),
    E(C_nngp_shard_sync, 1),
    E(C_nngp_factor, 4),
    E(C_nngp_get_linv, 2),
    E(C_nngp_set_linv, 3),
    E(C_nngp_accept_factor, 1),
    E(C_nngp_get_precision_diag, 1),
    E(C_nngp_set_field, 2),
    E(C_nngp_get_field, 1),
    E(C_nngp_set_mu, 3),
    E(C_nngp_records_reserve, 2),
    E(C_nngp_record_field, 2),
    E(C_nngp_get_records, 4),
    E(C_nngp_records_stream, 2),
    E(C_nngp_loglik, 4),
    E(C_nngp_sweep, 8),
    E(C_nngp_sweep_chains, 7),
    E(C_nngp_sweep_timed, 7),
    E(C_nngp_ancillary_propose, 3),
    E(C_nngp_ancillary_propose_chains, 4),
    E(C_nngp_field_response_ratio, 3),
    E(C_nngp_accept_field, 1),
    E(C_nngp_beta0_stats, 1),
    E(C_nngp_sum_squared_residuals, 2),
    E(C_nngp_spmv, 3),
    E(C_nngp_tri_solve, 3),
    E(C_nngp_tri_rescues, 1),
    E(C_nngp_device_normals, 4),
    E(C_nngp_summary, 2),
    E(C_nngp_summary_probs, 4),
    E(C_nngp_summary_stats, 0),
    E(C_nngp_effects_summary, 9),
    E(C_nngp_effects_stats, 0),
    E(C_nngp_pointwise_loglik, 7),
    E(C_nngp_pointwise_loglik_stats, 0),
    E(C_nngp_field_diag, 2),
    E(C_nngp_field_diag_stats, 0),
    E(C_nngp_predict_field, 14),
    E(C_nngp_predict_stats, 0),
    E(C_nngp_get_sweep_r, 1),
    E(C_nngp_shard_unique_id, 0),
    E(C_nngp_shard_comm_init, 2),
    E(C_nngp_sweep_chains_group, 7),
    E(C_nngp_shard_ipc_handle, 1),
    E(C_nngp_shard_ipc_open, 2),
    E(C_nngp_factor_chains, 5),
    E(C_nngp_loglik_chains, 5),
    E(C_nngp_loglik_pair_chains, 5),
    E(C_nngp_ancillary_step_chains, 7),
    E(C_nngp_sufficient_step_chains, 7),
    E(C_nngp_field_response_ratio_chains, 4),
    E(C_nngp_sum_squared_residuals_chains, 3),
    E(C_nngp_design_set, 4),
    E(C_nngp_design_mean_stats_chains, 4),
    E(C_nngp_design_interweave_stats_chains, 4),
    E(C_nngp_design_commit_chains, 7),
    E(C_nngp_get_mu, 1),
    {NULL, NULL, 0}};
#undef E

void R_init_nngpamd(DllInfo* dll) {
  R_registerRoutines(dll, NULL, call_methods, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}
