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
