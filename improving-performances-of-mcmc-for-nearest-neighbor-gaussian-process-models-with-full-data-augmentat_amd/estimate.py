"""mcmc_nngp_estimate -- host mirror of Scripts/mcmc_nngp_estimate.R:1-96
(posterior summaries; out of the kernel scope, kept for statistical parity)."""
from __future__ import annotations

import numpy as np

SUMMARY_COLS = ["mean", "q0.025", "median", "q0.975", "sd"]


def _quantile7(x, q):
    return np.quantile(x, q, axis=0)  # numpy 'linear' == R type 7


DEFAULT_PROBS = (0.025, 0.5, 0.975)
MAX_PROBS, MAX_THRESHOLDS = 16, 8  # kSummaryProbsMax, kSummaryThrMax (csrc/summary_select.h)


def _summary_request(probs, thresholds):
    """The checked request of a widened summary: (probs, thresholds) as float64
    vectors, ``probs=None`` being the default three.  One wording for both
    backends; the library checks the same again."""
    p = np.asarray(DEFAULT_PROBS if probs is None else probs, np.float64)
    t = np.asarray(() if thresholds is None else thresholds, np.float64)
    if p.ndim > 1 or t.ndim > 1:
        raise ValueError("get_summary: probs and thresholds must be scalars or 1-D")
    p, t = np.ascontiguousarray(p.reshape(-1)), np.ascontiguousarray(t.reshape(-1))
    if p.size > MAX_PROBS:
        raise ValueError(f"get_summary: at most {MAX_PROBS} probs, not {p.size}")
    if t.size > MAX_THRESHOLDS:
        raise ValueError(f"get_summary: at most {MAX_THRESHOLDS} thresholds, not {t.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):  # a NaN fails both compares
        raise ValueError("get_summary: probs must lie in [0, 1]")
    if np.any(np.isnan(t)):
        raise ValueError("get_summary: thresholds must not be NaN")
    return p, t


def summary_columns(probs=None, thresholds=None):
    """The column names of get_summary(..., probs, thresholds): SUMMARY_COLS
    for the defaults, else mean, q<p>..., sd, p_gt_<t>..."""
    if probs is None and thresholds is None:
        return list(SUMMARY_COLS)
    p, t = _summary_request(probs, thresholds)
    return ["mean"] + [f"q{v:g}" for v in p] + ["sd"] + [f"p_gt_{v:g}" for v in t]


def get_summary(samples, backend="host", device=-1, row_offset=None, chunk_cols=0, probs=None, thresholds=None):
    """estimate.R:1-6: mean, q0.025, median, q0.975, sd per column.

    ``samples``: a 2-D array (rows = samples) or a list of 2-D arrays with equal
    column counts, summarised as their row-wise stack; ``row_offset`` (one
    value per row of the stack) is subtracted from its row first.
    ``backend="host"`` (default) is numpy; ``backend="hip"`` runs the selection
    kernel of libnngp.so (nngp_summary) on ``device``: float64 row-contiguous
    blocks are passed where they lie, any other block is copied (only that
    block), and ``chunk_cols`` columns are staged per launch (0: automatic).
    Returns an (n, 5) array.

    ``probs`` (up to 16 probabilities in [0, 1], any order, repeats allowed)
    and ``thresholds`` (up to 8 values, +-inf allowed) widen it: with either
    given the result is (n, 2 + Q + K) with the columns of
    ``summary_columns(probs, thresholds)`` -- mean, the type-7 quantiles in
    the order of ``probs`` (None: the default three), sd, then the exceedance
    fractions P(x > t) = count(x > t) / rows of the values summarised (after
    ``row_offset``).  The device backend calls nngp_summary_probs; a column
    holding a NaN gives NaNs on both."""
    req = None if probs is None and thresholds is None else _summary_request(probs, thresholds)
    if backend == "hip":
        return _summary_hip(samples, device, row_offset, chunk_cols, req)
    if backend != "host":
        raise ValueError(f"get_summary: backend must be 'host' or 'hip', not {backend!r}")
    if isinstance(samples, (list, tuple)) and len(samples) and np.ndim(samples[0]) == 2:
        samples = np.vstack([np.asarray(b, np.float64) for b in samples])
    if row_offset is not None:
        samples = np.asarray(samples, np.float64) - np.asarray(row_offset, np.float64).reshape(-1, 1)
    s = np.atleast_2d(np.asarray(samples, np.float64))
    if s.shape[0] == 1 and s.ndim == 2 and s.shape[1] > 1 and np.asarray(samples).ndim == 1:
        s = s.T
    if req is not None:
        p, t = req
        bad = np.isnan(s).any(0)
        above = [np.where(bad, np.nan, (s > v).sum(0) / s.shape[0]) for v in t]
        return np.column_stack([s.mean(0), *_quantile7(s, p), s.std(0, ddof=1), *above])
    return np.column_stack([s.mean(0), _quantile7(s, 0.025), _quantile7(s, 0.5), _quantile7(s, 0.975),
                            s.std(0, ddof=1)])


def _summary_hip(samples, device, row_offset, chunk_cols, req=None):
    import ctypes as C

    from . import _lib

    if not (isinstance(samples, (list, tuple)) and len(samples) and np.ndim(samples[0]) == 2):
        a = np.asarray(samples)
        samples = [a.reshape(-1, 1) if a.ndim == 1 else a]
    blocks = []
    for b in samples:
        b = np.asarray(b)
        if b.ndim != 2:
            raise ValueError("get_summary: every block must be 2-D")
        if b.dtype != np.float64 or not b.flags.c_contiguous:
            b = np.ascontiguousarray(b, np.float64)
        blocks.append(b)
    n = blocks[0].shape[1]
    if any(b.shape[1] != n for b in blocks):
        raise ValueError("get_summary: the blocks' column counts differ")
    rows = (C.c_longlong * len(blocks))(*[b.shape[0] for b in blocks])
    ptrs = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    off = None
    if row_offset is not None:
        off = _lib.f64(np.asarray(row_offset).reshape(-1))
        if off.size != sum(b.shape[0] for b in blocks):
            raise ValueError("get_summary: row_offset needs one entry per row")
    if req is not None:
        p, t = req
        out = np.empty((2 + p.size + t.size, max(n, 1)))  # n x (2 + Q + K) column-major
        _lib.check(_lib.lib.nngp_summary_probs(int(device), ptrs, rows, len(blocks), n,
                                               None if off is None else off.ctypes.data, int(chunk_cols),
                                               p.ctypes.data if p.size else None, p.size,
                                               t.ctypes.data if t.size else None, t.size, out))
        return np.ascontiguousarray(out.T)
    out = np.empty((5, max(n, 1)))  # n x 5 column-major
    _lib.check(_lib.lib.nngp_summary(int(device), ptrs, rows, len(blocks), n, None if off is None else off.ctypes.data,
                                     int(chunk_cols), out))
    return np.ascontiguousarray(out.T)


def summary_stats():
    """HIP-event times and staging size of this thread's last device summary
    (nngp_summary_stats)."""
    import ctypes as C

    from . import _lib

    cp, kn, by, w = C.c_double(), C.c_double(), C.c_longlong(), C.c_int()
    _lib.check(_lib.lib.nngp_summary_stats(C.byref(cp), C.byref(kn), C.byref(by), C.byref(w)))
    return {"copy_ms": cp.value, "kernel_ms": kn.value, "staged_bytes": by.value, "chunk_cols": w.value}


def _row_blocks(blocks, what):
    """A 2-D array or a list of 2-D arrays as float64 row-contiguous blocks
    (a block that is one already is passed where it lies)."""
    if not (isinstance(blocks, (list, tuple)) and len(blocks) and np.ndim(blocks[0]) == 2):
        blocks = [np.asarray(blocks)]
    out = []
    for b in blocks:
        b = np.asarray(b)
        if b.ndim != 2:
            raise ValueError(f"{what}: every block must be 2-D")
        if b.dtype != np.float64 or not b.flags.c_contiguous:
            b = np.ascontiguousarray(b, np.float64)
        out.append(b)
    return out


def effects_summary(coef, X, addend=None, noise_sd=None, seed=0, counter=None, probs=None, thresholds=None,
                    backend="host", device=-1, chunk_cols=0, return_samples=False):
    """The summary of the samples ``coef @ X.T (+ addend) (+ noise)`` per
    location (predict.R:92-102: beta_matrix[, subset] %*% t(X_pred) and its
    get_summary), without the samples on the host when ``backend="hip"``.

    ``coef``: S x q coefficient samples; ``X``: n x q design rows of the new
    locations (an array whose transpose is C-contiguous float64 is passed where
    it lies); ``addend``: an S x n array or a list of blocks stacking to S rows
    (the predicted field's per-chain samples); ``noise_sd`` (S): sample s gets
    noise_sd[s] * z with z the Philox / AS241 normals of
    (``seed``, ``counter[s]``) -- nngp_device_normals -- ``counter`` defaulting
    to 0 .. S-1.  ``probs`` / ``thresholds`` are get_summary's.

    ``backend="host"`` is numpy (the product, the sums, the host get_summary);
    its normals still come from the library, so noise needs a device.
    ``backend="hip"`` is nngp_effects_summary: the samples are generated chunk
    by chunk on ``device`` by the arithmetic include/nngp.h states and
    summarised there; ``chunk_cols`` as for get_summary.  Returns the (n,
    columns) summary, or (summary, samples) with ``return_samples=True``
    (hip: the device's own values)."""
    if backend not in ("host", "hip"):
        raise ValueError(f"effects_summary: backend must be 'host' or 'hip', not {backend!r}")
    req = _summary_request(probs, thresholds)
    coef = np.asarray(coef, np.float64)
    X = np.asarray(X, np.float64)
    if coef.ndim != 2 or X.ndim != 2 or coef.shape[1] != X.shape[1]:
        raise ValueError("effects_summary: coef must be S x q and X n x q")
    S, n = coef.shape[0], X.shape[0]
    blocks = None if addend is None else _row_blocks(addend, "effects_summary")
    if blocks is not None and (any(b.shape[1] != n for b in blocks) or sum(b.shape[0] for b in blocks) != S):
        raise ValueError("effects_summary: the addend must stack to S x n")
    sd = cnt = None
    if noise_sd is not None:
        sd = np.ascontiguousarray(np.asarray(noise_sd, np.float64).reshape(-1))
        cnt = np.arange(S, dtype=np.uint64) if counter is None else np.ascontiguousarray(counter, np.uint64).reshape(-1)
        if sd.size != S or cnt.size != S:
            raise ValueError("effects_summary: noise_sd and counter need one entry per sample")
    seed = int(seed) & (2 ** 64 - 1)
    if backend == "hip":
        return _effects_hip(coef, X, blocks, sd, seed, cnt, req, device, chunk_cols, return_samples)
    samples = coef @ X.T
    if blocks is not None:
        samples = samples + np.vstack(blocks)
    if sd is not None:
        from . import _lib

        z = np.empty((S, n))
        for s in range(S):
            _lib.check(_lib.lib.nngp_device_normals(int(device), seed, int(cnt[s]), n, z[s]))
        samples = samples + sd[:, None] * z
    widen = {} if probs is None and thresholds is None else {"probs": probs, "thresholds": thresholds}
    summary = get_summary(samples, **widen)
    return (summary, samples) if return_samples else summary


def _effects_hip(coef, X, blocks, sd, seed, cnt, req, device, chunk_cols, return_samples):
    import ctypes as C

    from . import _lib

    p, t = req
    (S, q), n = coef.shape, X.shape[0]
    coef_cm, X_cm = _lib.colmajor(coef, np.float64), _lib.colmajor(X, np.float64)
    nb = 0 if blocks is None else len(blocks)
    rows = (C.c_longlong * max(nb, 1))(*[b.shape[0] for b in blocks or ()])
    ptrs = (C.c_void_p * max(nb, 1))(*[b.ctypes.data for b in blocks or ()])
    out = np.empty((2 + p.size + t.size, max(n, 1)))  # n x (2 + Q + K) column-major
    samples = np.empty((S, n)) if return_samples else None
    _lib.check(_lib.lib.nngp_effects_summary(
        int(device), coef_cm.ctypes.data, S, q, X_cm.ctypes.data, n, ptrs if nb else None, rows if nb else None, nb,
        None if sd is None else sd.ctypes.data, seed, None if cnt is None else cnt.ctypes.data, int(chunk_cols),
        p.ctypes.data if p.size else None, p.size, t.ctypes.data if t.size else None, t.size,
        out.ctypes.data, None if samples is None else samples.ctypes.data))
    summary = np.ascontiguousarray(out.T)
    return (summary, samples) if return_samples else summary


def effects_stats():
    """HIP-event times and staging size of this thread's last device
    effects_summary (nngp_effects_stats)."""
    import ctypes as C

    from . import _lib

    cp, gn, kn, by, w = C.c_double(), C.c_double(), C.c_double(), C.c_longlong(), C.c_int()
    _lib.check(_lib.lib.nngp_effects_stats(C.byref(cp), C.byref(gn), C.byref(kn), C.byref(by), C.byref(w)))
    return {"copy_ms": cp.value, "generate_ms": gn.value, "kernel_ms": kn.value, "staged_bytes": by.value,
            "chunk_cols": w.value}


POINTWISE_COLUMNS = ["fit_mean", "ll_mean", "ll_var", "lppd", "log_cpo", "pit"]
_HOST_SLAB = 4096  # observations per slab of the host backend's S x slab temporaries


def pointwise_loglik(y, obs_loc, field_blocks, log_noise_var, coef=None, X=None, backend="host", device=-1,
                     chunk_cols=0):
    """The Gaussian log density of every observation under every saved sample,
    ll[s, i] = log N(y[i] | field[s, obs_loc[i]] + X[i] . coef[s], exp(log_noise_var[s])),
    reduced over the samples: an (n_obs, 6) array with POINTWISE_COLUMNS --
    fit_mean (mean of the means), ll_mean, ll_var (divisor S - 1; NaN for one
    sample), lppd = log mean exp(ll), log_cpo = -log mean exp(-ll) (both with
    the maximum taken out first) and pit = mean of Phi((y - mean) / sd).

    ``y`` (n_obs); ``obs_loc`` (n_obs): the 1-based location of each
    observation, in any order; ``field_blocks``: an S x n array or a list of
    blocks stacking to S rows (float64 row-contiguous blocks, tail slices of the
    records included, are passed where they lie); ``log_noise_var`` (S);
    ``coef`` (S x q) and ``X`` (n_obs x q, rows in the order of ``y``), or
    neither.  ``backend="host"`` (default) is numpy; ``backend="hip"`` sorts the
    observations by location (a stable sort), calls nngp_pointwise_loglik on
    ``device`` (``chunk_cols`` locations staged per launch, 0: automatic) and
    returns the rows in the caller's order.  A NaN in y[i], X[i] or the
    location's column gives six NaNs in row i."""
    if backend not in ("host", "hip"):
        raise ValueError(f"pointwise_loglik: backend must be 'host' or 'hip', not {backend!r}")
    y = np.ascontiguousarray(np.asarray(y, np.float64).reshape(-1))
    loc = np.asarray(obs_loc).reshape(-1)
    blocks = _row_blocks(field_blocks, "pointwise_loglik")
    n = blocks[0].shape[1]
    S = sum(b.shape[0] for b in blocks)
    lnv = np.ascontiguousarray(np.asarray(log_noise_var, np.float64).reshape(-1))
    if any(b.shape[1] != n for b in blocks) or lnv.size != S or S < 1:
        raise ValueError("pointwise_loglik: the field blocks must stack to S x n with one log_noise_var per row")
    if loc.size != y.size or y.size < 1:
        raise ValueError("pointwise_loglik: y and obs_loc need one entry per observation")
    if loc.min() < 1 or loc.max() > n:
        raise ValueError("pointwise_loglik: obs_loc must lie in 1 .. n")
    if (coef is None) != (X is None):
        raise ValueError("pointwise_loglik: coef and X go together")
    if coef is not None:
        coef, X = np.asarray(coef, np.float64), np.asarray(X, np.float64)
        if coef.ndim != 2 or X.ndim != 2 or coef.shape != (S, X.shape[1]) or X.shape[0] != y.size:
            raise ValueError("pointwise_loglik: coef must be S x q and X n_obs x q")
        if coef.shape[1] == 0:
            coef = X = None
    if not np.all(np.isfinite(lnv)):
        raise ValueError("pointwise_loglik: log_noise_var must be finite")
    if backend == "hip":
        return _pointwise_hip(y, loc, blocks, lnv, coef, X, device, chunk_cols)
    a = -0.5 * (np.log(2.0 * np.pi) + lnv)[:, None]
    h = (0.5 * np.exp(-lnv))[:, None]
    g = np.sqrt(2.0 * h)
    from scipy.special import erfc

    out = np.empty((y.size, 6))
    col = loc.astype(np.int64) - 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i0 in range(0, y.size, _HOST_SLAB):
            sl = slice(i0, i0 + _HOST_SLAB)
            mean = np.vstack([b[:, col[sl]] for b in blocks])
            if coef is not None:
                # column by column, the order of the device's chain (a BLAS product
                # may round equal rows differently)
                acc = coef[:, :1] * X[sl, 0]
                for k in range(1, coef.shape[1]):
                    acc += coef[:, k:k + 1] * X[sl, k]
                mean = mean + acc
            r = y[sl] - mean
            ll = a - h * r * r
            M, Mn = np.fmax.reduce(ll, axis=0), np.fmax.reduce(-ll, axis=0)
            o = out[sl]
            o[:, 0] = mean.sum(0) / S
            o[:, 1] = ll.sum(0) / S
            o[:, 2] = ((ll - o[:, 1]) ** 2).sum(0) / (S - 1) if S > 1 else np.nan
            o[:, 3] = M + np.log(np.exp(ll - M).sum(0)) - np.log(S)
            o[:, 4] = -(Mn + np.log(np.exp(-ll - Mn).sum(0)) - np.log(S))
            o[:, 5] = (0.5 * erfc(-(r * g) * np.sqrt(0.5))).sum(0) / S
            o[np.isnan(o[:, 1])] = np.nan
    return out


def _pointwise_hip(y, loc, blocks, lnv, coef, X, device, chunk_cols):
    import ctypes as C

    from . import _lib

    # observations that come sorted already are passed as they are (an X whose
    # transpose is C-contiguous where it lies: no n_obs x q gather or copy)
    is_sorted = bool(np.all(loc[1:] >= loc[:-1]))
    order = slice(None) if is_sorted else np.argsort(loc, kind="stable")
    ys, ls = np.ascontiguousarray(y[order]), np.ascontiguousarray(loc[order], np.int32)
    q = 0 if coef is None else coef.shape[1]
    coef_cm = None if q == 0 else _lib.colmajor(coef, np.float64)
    X_cm = None if q == 0 else _lib.colmajor(X if is_sorted else X[order], np.float64)
    rows = (C.c_longlong * len(blocks))(*[b.shape[0] for b in blocks])
    ptrs = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    out = np.empty((6, y.size))  # n_obs x 6 column-major
    _lib.check(_lib.lib.nngp_pointwise_loglik(
        int(device), ys.ctypes.data, y.size, ls.ctypes.data, None if q == 0 else coef_cm.ctypes.data, lnv.size, q,
        None if q == 0 else X_cm.ctypes.data, ptrs, rows, len(blocks), blocks[0].shape[1], lnv.ctypes.data,
        int(chunk_cols), out.ctypes.data))
    res = np.empty((y.size, 6))
    res[order] = out.T
    return res


def pointwise_loglik_stats():
    """HIP-event times and staging size of this thread's last device
    pointwise_loglik (nngp_pointwise_loglik_stats)."""
    import ctypes as C

    from . import _lib

    cp, kn, by, w = C.c_double(), C.c_double(), C.c_longlong(), C.c_int()
    _lib.check(_lib.lib.nngp_pointwise_loglik_stats(C.byref(cp), C.byref(kn), C.byref(by), C.byref(w)))
    return {"copy_ms": cp.value, "kernel_ms": kn.value, "staged_bytes": by.value, "chunk_cols": w.value}


def mcmc_nngp_criteria(mcmc_nngp_list, burn_in=0.5, backend="host", device=-1):
    """WAIC, LPML and DIC of a fit from the pointwise log-likelihood of its
    stored field samples (pointwise_loglik over the chains' stack).

    The stored iterations are predict.py's: saved_field > burn_in * max.  Per
    chain the tail of params["field"] is one block, read where it lies; the
    field holds beta_0, so the mean of observation i is
    field[locs_match[i]] + X[i] . beta with the centred X["X"] (no regression
    term without covariates).  Returns ``pointwise`` (n_obs x 6, ``columns``),
    ``lppd`` and ``p_waic`` (the sums of lppd and ll_var), ``waic`` =
    -2 (lppd - p_waic), ``lpml`` (the sum of log_cpo), ``dbar`` =
    -2 sum ll_mean, ``dhat`` = -2 sum log N(y | fit_mean, exp(mean
    log_noise_var)), ``p_dic`` = dbar - dhat, ``dic`` = dbar + p_dic and
    ``n_samples``."""
    L = mcmc_nngp_list
    recs = list(L["records"].values())
    saved = np.asarray(recs[0]["saved_field"])
    sel = saved > burn_in * saved.max()
    idx = np.nonzero(sel)[0]
    if idx.size == 0:
        raise ValueError("mcmc_nngp_criteria: no stored field sample after burn-in")
    stored = saved[sel].astype(int)
    suffix = idx[0] + idx.size == sel.size
    blocks, coef, lnv = [], [], []
    has_beta = L["X"].get("X") is not None and all("beta" in c["params"] for c in recs)
    for c in recs:
        f = c["params"]["field"]
        blocks.append(f[idx[0]:] if suffix and f.shape[0] == sel.size else f[sel])
        lnv.append(np.asarray(c["params"]["log_noise_variance"], np.float64).reshape(-1)[stored - 1])
        if has_beta:
            coef.append(np.asarray(c["params"]["beta"], np.float64)[stored - 1])
    lnv = np.concatenate(lnv)
    y = np.asarray(L["observed_field"], np.float64)
    pw = pointwise_loglik(y, L["vecchia_approx"]["locs_match"], blocks, lnv,
                          coef=np.vstack(coef) if has_beta else None, X=L["X"]["X"] if has_beta else None,
                          backend=backend, device=device)
    lppd, p_waic, lpml = pw[:, 3].sum(), pw[:, 2].sum(), pw[:, 4].sum()
    dbar = -2.0 * pw[:, 1].sum()
    lnv_bar = lnv.mean()
    dhat = -2.0 * (-0.5 * (np.log(2.0 * np.pi) + lnv_bar) - 0.5 * np.exp(-lnv_bar) * (y - pw[:, 0]) ** 2).sum()
    p_dic = dbar - dhat
    return {"pointwise": pw, "columns": list(POINTWISE_COLUMNS), "lppd": lppd, "p_waic": p_waic,
            "waic": -2.0 * (lppd - p_waic), "lpml": lpml, "dbar": dbar, "dhat": dhat, "p_dic": p_dic,
            "dic": dbar + p_dic, "n_samples": int(lnv.size)}


def _plogis(x):
    return 1 / (1 + np.exp(-x))


def mcmc_nngp_estimate(mcmc_nngp_list, burn_in=0.5, field_backend="host", device=-1, field_probs=None,
                       field_thresholds=None):
    """estimate.R:9-96.  ``field_backend="hip"`` takes res["field"] (the one
    summary as wide as the field) from the device get_summary on ``device``;
    the covariance and fixed-effect summaries are a handful of columns and
    stay on the host.  A burn_in that leaves no saved field row raises
    NNGPError (status 1: no rows) there, where the host path returns NaNs.
    ``field_probs`` / ``field_thresholds`` are get_summary's ``probs`` /
    ``thresholds`` for res["field"] (both backends); with either given,
    res["field_columns"] names its columns."""
    if field_backend not in ("host", "hip"):
        raise ValueError(f"mcmc_nngp_estimate: field_backend must be 'host' or 'hip', not {field_backend!r}")
    L = mcmc_nngp_list
    recs = L["records"]
    first = next(iter(recs.values()))
    it = int(first["iterations"][-1, 0])
    lo = int(burn_in * it) - 1
    res = {"covariance_params": {}}
    widen = {}
    if field_probs is not None or field_thresholds is not None:
        widen = {"probs": field_probs, "thresholds": field_thresholds}
        res["field_columns"] = summary_columns(field_probs, field_thresholds)
    sp = L["space_time_model"]["covfun"]["shape_params"]
    names = ["log_scale", "log_noise_variance"] + list(sp)
    samples = np.vstack([np.column_stack([c["params"]["log_scale"], c["params"]["log_noise_variance"],
                                          c["params"]["shape"]])[lo:it] for c in recs.values()])
    res["covariance_params"]["sampled_covparams"] = {"names": names, "summary": get_summary(samples)}
    g = samples.copy()
    gnames = []
    for j, nm in enumerate(names):
        if nm.startswith("log_"):
            g[:, j] = np.exp(g[:, j])
            gnames.append(nm[4:])
        elif nm.startswith("qlogis_"):
            g[:, j] = 1.5 * _plogis(g[:, j])
            gnames.append(nm[7:])
        else:
            gnames.append(nm)
    res["covariance_params"]["GpGp_covparams"] = {"names": gnames, "summary": get_summary(g)}
    inla = g.copy()
    inames = list(gnames)
    covfun = L["space_time_model"]["covfun"]["stationary_covfun"]
    keep = np.ones(len(inames), bool)
    if "exponential" in covfun:
        for j, nm in enumerate(inames):
            if "range" in nm:
                inla[:, j] *= 2
    if "matern" in covfun and covfun != "matern15_isotropic":
        sm = [j for j, nm in enumerate(inames) if "smoothness" in nm][0]
        for j, nm in enumerate(inames):
            if "range" in nm:
                inla[:, j] *= np.sqrt(8 * inla[:, sm])
        keep[sm] = False
    for j, nm in enumerate(inames):
        if "noise" in nm:
            inla[:, j] = 1 / inla[:, j]
            inames[j] = "precision_of_Gaussian_obs"
        elif "scale" in nm:
            inla[:, j] = np.sqrt(inla[:, j])
            inames[j] = "sd_for_spatial"
    res["covariance_params"]["INLA_covparams"] = {"names": [n for n, k in zip(inames, keep) if k],
                                                  "summary": get_summary(inla[:, keep])}
    # fixed effects (estimate.R:76-87)
    fx = []
    for c in recs.values():
        b = [c["params"]["beta_0"]]
        if "beta" in c["params"]:
            b.append(c["params"]["beta"])
        out = np.column_stack(b)[lo:it].copy()
        if out.shape[1] > 1:
            out[:, 0] = out[:, 0] - out[:, 1:] @ L["X"]["X_mean"]
        fx.append(out)
    fx = np.vstack(fx)
    fe = get_summary(fx)
    zero_out = (np.sign(fe[:, 1]) * np.sign(fe[:, 3])) > 0
    res["fixed_effects"] = {"names": ["beta_0"] + list(L["X"].get("names", [])),
                            "summary": np.column_stack([fe, zero_out])}
    # field (estimate.R:89-96): centered field samples after burn-in
    fs = []
    saved = first["saved_field"]
    sel = saved > it * burn_in
    if field_backend == "hip":
        # saved_field increases, so the rows after burn-in are a suffix: each
        # chain's block is a view of its records, the centring is the kernel's
        # row offset (a mask that is no suffix falls back to a copy)
        idx = np.nonzero(sel)[0]
        suffix = idx.size > 0 and idx[0] + idx.size == sel.size
        b0_rows = saved[sel].astype(int) - 1
        for c in recs.values():
            f = c["params"]["field"]
            fs.append(f[idx[0]:] if suffix and f.shape[0] == sel.size else f[sel])
        offs = np.concatenate([c["params"]["beta_0"][b0_rows, 0] for c in recs.values()])
        res["field"] = get_summary(fs, backend="hip", device=device, row_offset=offs, **widen)
        return res
    for c in recs.values():
        f = c["params"]["field"][sel]
        b0 = c["params"]["beta_0"][saved[sel].astype(int) - 1, 0]
        fs.append(f - b0[:, None])
    res["field"] = get_summary(np.vstack(fs), **widen)
    return res
