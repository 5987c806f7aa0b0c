"""mcmc_nngp_predict_field / mcmc_nngp_predict_fixed_effects -- host mirror of
Scripts/mcmc_nngp_predict.R:1-104 ("next"), and
mcmc_nngp_predict_response, the sum of the two per stored iteration.

Per saved sample the field is predicted with the device factor build on the
stacked locations and the device sparse triangular solve
(predict.R:39-53): sd * B^{-1} c(B11 (w/sd), z).

Two engines compute the same samples: ``engine="context"`` builds a
ChainContext on the stacked locations and runs factor, SpMV and triangular
solve per sample; ``engine="batched"`` makes one nngp_predict_field call per
chain (include/nngp.h): the factor rows of the new locations only, and a
level solve with the samples in the lanes (DESIGN.md "Batched prediction").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .context import ChainContext
from .estimate import POINTWISE_COLUMNS, effects_summary, get_summary, pointwise_loglik, summary_columns
from .graph import find_ordered_nn, naive_greedy_coloring
from .model import covparms


def mcmc_nngp_predict_field(mcmc_nngp_list, predicted_locs, burn_in=0.5, n_cores=1, m=10, seed=1,
                            device=-1, z_new=None, summary_backend="host", engine="context", rng="numpy",
                            sample_batch=0, summary_probs=None, summary_thresholds=None):
    """predict.R:1-60.  ``z_new`` (optional) replaces the rnorm draws of the
    new locations (predict.R:50): z_new[k][i] = the normals of chain k's i-th
    prediction; by default they come from numpy's generator seeded ``seed``.
    ``summary_backend="hip"`` summarises the per-chain sample arrays on the
    device (get_summary, no stacked copy); the samples are the same.
    ``summary_probs`` / ``summary_thresholds`` are get_summary's ``probs`` /
    ``thresholds`` for predicted_field_summary (both backends, both engines);
    with either given, predicted_field_summary_columns names its columns.

    ``engine="batched"``: one nngp_predict_field call per chain, reading
    chain["params"]["field"] where it lies; no colouring and no ChainContext.
    Same arguments, same samples up to rounding.  ``rng="philox"`` (batched
    engine only) draws the normals on the device instead: sample k of a chain
    (its ordinal among the chain's predicted samples, 0-based) uses Philox
    counter k, and chain c (0-based) the key
    (seed + (c + 1) * 0x9E3779B97F4A7C15) mod 2^64 -- the 64-bit golden-ratio
    increment, so chains with one ``seed`` get distinct streams.
    ``sample_batch`` (batched engine; 0 = automatic) is nngp_predict_field's."""
    if summary_backend not in ("host", "hip"):
        raise ValueError(f"mcmc_nngp_predict_field: summary_backend must be 'host' or 'hip', not {summary_backend!r}")
    if engine not in ("context", "batched"):
        raise ValueError(f"mcmc_nngp_predict_field: engine must be 'context' or 'batched', not {engine!r}")
    if rng not in ("numpy", "philox"):
        raise ValueError(f"mcmc_nngp_predict_field: rng must be 'numpy' or 'philox', not {rng!r}")
    if rng == "philox" and engine != "batched":
        raise ValueError("mcmc_nngp_predict_field: rng='philox' needs engine='batched'")
    if engine == "batched":
        return _predict_field_batched(mcmc_nngp_list, predicted_locs, burn_in, m, seed, device, z_new,
                                      summary_backend, rng, sample_batch, summary_probs, summary_thresholds)
    L = mcmc_nngp_list
    locs = L["locs"]
    predicted_locs = np.asarray(predicted_locs, np.float64)
    allloc = np.vstack([locs, predicted_locs])
    NN = find_ordered_nn(allloc, m)
    N, n = allloc.shape[0], locs.shape[0]
    ctx = ChainContext(allloc, NN, naive_greedy_coloring(NN), np.arange(1, N + 1, dtype=np.int32),
                       np.zeros(N), device=device)
    covfun = L["space_time_model"]["covfun"]["stationary_covfun"]
    sp = L["space_time_model"]["covfun"]["shape_params"]
    first = next(iter(L["records"].values()))
    stored = first["saved_field"]
    stored = stored[stored > burn_in * stored.max()].astype(int)
    rng = np.random.default_rng(seed)
    out = []
    for kc, chain in enumerate(L["records"].values()):
        shapes = chain["params"]["shape"][stored - 1]
        _, first_idx = np.unique(shapes, axis=0, return_index=True)
        need = np.zeros(len(stored), bool)
        need[first_idx] = True  # !duplicated(shape[stored_idx, ])
        samples = np.zeros((len(stored), predicted_locs.shape[0]))
        for k, i_chain in enumerate(stored):
            i_field = int(np.nonzero(chain["saved_field"] == i_chain)[0][0]) if "saved_field" in chain \
                else int(np.nonzero(first["saved_field"] == i_chain)[0][0])
            if need[k] or k == 0:
                ctx.factor(0, covfun, covparms(sp, chain["params"]["shape"][i_chain - 1], 0.0, 1.5))
            sd = np.exp(0.5 * chain["params"]["log_scale"][i_chain - 1, 0])
            w = chain["params"]["field"][i_field] - chain["params"]["beta_0"][i_chain - 1, 0]
            u = ctx.spmv(0, np.concatenate([w, np.zeros(N - n)]))[:n]
            z = rng.normal(size=N - n) if z_new is None else np.asarray(z_new[kc][k], np.float64)
            x = ctx.tri_solve(0, np.concatenate([u / sd, z]))
            samples[k] = sd * x[n:]
        out.append(samples)
    ctx.close()
    return {"predicted_locs": predicted_locs, "predicted_field_samples": out,
            **_field_summary(out, summary_backend, device, summary_probs, summary_thresholds)}


def predict_field_call(locs, NN, n, covfun, covparms_rows, factor_of, fields, field_row, beta0, log_scale,
                       z=None, seed=0, counter=None, sample_batch=0, device=-1):
    """nngp_predict_field (include/nngp.h) on numpy arrays: ``locs`` (N x d) and
    ``NN`` (N x b, 1-based, NA = INT_MIN) of the stacked locations, the first
    ``n`` observed; ``fields`` a C-contiguous (rows x >= n) float64 array read
    in place.  Returns the n_samples x n_pred samples; NNGPError carries the
    status (``fail_row``: the stacked 1-based row of a failed factor)."""
    N, d = locs.shape
    n_pred = N - n
    cp = _lib.f64(np.atleast_2d(covparms_rows))
    factor_of = _lib.i32(factor_of)
    n_samples = len(factor_of)
    if not (isinstance(fields, np.ndarray) and fields.dtype == np.float64 and fields.ndim == 2
            and fields.flags.c_contiguous):
        fields = np.ascontiguousarray(fields, np.float64)
    field_row = np.ascontiguousarray(field_row, np.int64)
    beta0, log_scale = _lib.f64(beta0), _lib.f64(log_scale)
    if len(field_row) != n_samples or len(beta0) != n_samples or len(log_scale) != n_samples:
        raise ValueError("predict_field_call: per-sample arrays differ in length")
    if len(field_row) and (field_row.min() < 0 or field_row.max() >= fields.shape[0]):
        raise ValueError("predict_field_call: field_row out of range")
    zp = cnt = None
    if z is not None:
        z = _lib.f64(z)
        if z.shape != (n_samples, n_pred):
            raise ValueError(f"predict_field_call: z must be {n_samples} x {n_pred}")
        zp = z.ctypes.data
    else:
        cnt = np.ascontiguousarray(counter, np.uint64)
        if len(cnt) != n_samples:
            raise ValueError("predict_field_call: counter needs one entry per sample")
    out = np.empty((max(n_samples, 0), max(n_pred, 0)))
    fail = C.c_int(0)
    locs_cm, nn_cm = _lib.colmajor(locs, np.float64), _lib.colmajor(NN, np.int32)
    st = _lib.lib.nngp_predict_field(device, locs_cm, n, n_pred, d, nn_cm, NN.shape[1], _lib.COVFUNS[covfun], cp,
                                     cp.shape[1], cp.shape[0], n_samples, factor_of.ctypes.data, fields.ctypes.data,
                                     fields.shape[1], field_row.ctypes.data, beta0.ctypes.data, log_scale.ctypes.data,
                                     zp, int(seed) & (2 ** 64 - 1), None if cnt is None else cnt.ctypes.data,
                                     int(sample_batch), out.ctypes.data, C.byref(fail))
    if st != 0:
        try:
            _lib.check(st)
        except _lib.NNGPError as e:
            e.fail_row = fail.value
            raise
    return out


def predict_stats():
    """nngp_predict_stats: the calling thread's last successful prediction."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    by, sb = C.c_longlong(), C.c_int()
    _lib.check(_lib.lib.nngp_predict_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(by), C.byref(sb)))
    return {"plan_ms": a.value, "factor_ms": b.value, "solve_ms": c.value, "staged_bytes": by.value,
            "sample_batch": sb.value}


PHILOX_CHAIN_MIX = 0x9E3779B97F4A7C15


def _field_summary(out, summary_backend, device, probs, thresholds):
    """predicted_field_summary (and its column names when it is widened)."""
    widen = {} if probs is None and thresholds is None else {"probs": probs, "thresholds": thresholds}
    summary = get_summary(out, backend="hip", device=device, **widen) if summary_backend == "hip" \
        else get_summary(np.vstack(out), **widen)
    res = {"predicted_field_summary": summary}
    if widen:
        res["predicted_field_summary_columns"] = summary_columns(probs, thresholds)
    return res


def _predict_field_batched(L, predicted_locs, burn_in, m, seed, device, z_new, summary_backend, rng, sample_batch,
                           summary_probs=None, summary_thresholds=None):
    locs = L["locs"]
    predicted_locs = np.asarray(predicted_locs, np.float64)
    allloc = np.vstack([locs, predicted_locs])
    NN = find_ordered_nn(allloc, m)
    n, n_pred = locs.shape[0], predicted_locs.shape[0]
    covfun = L["space_time_model"]["covfun"]["stationary_covfun"]
    sp = L["space_time_model"]["covfun"]["shape_params"]
    first = next(iter(L["records"].values()))
    stored = first["saved_field"]
    stored = stored[stored > burn_in * stored.max()].astype(int)
    gen = np.random.default_rng(seed)
    out = []
    for kc, chain in enumerate(L["records"].values()):
        saved = chain["saved_field"] if "saved_field" in chain else first["saved_field"]
        field_row = np.array([int(np.nonzero(saved == i)[0][0]) for i in stored], np.int64)
        shapes = chain["params"]["shape"][stored - 1]
        # predict.R:23,32: a factor is built where !duplicated(shape) marks the
        # sample; every other sample uses the LAST factor built, also when its
        # own shape was seen earlier and another one came in between
        _, first_idx = np.unique(shapes, axis=0, return_index=True)
        need = np.zeros(len(stored), bool)
        need[first_idx] = True
        need[:1] = True
        factor_of = np.cumsum(need) - 1
        rows = np.array([covparms(sp, chain["params"]["shape"][i - 1], 0.0, 1.5) for i in stored[need]], np.float64)
        kw = {}
        if rng == "philox":
            kw = {"seed": (int(seed) + (kc + 1) * PHILOX_CHAIN_MIX) % 2 ** 64,
                  "counter": np.arange(len(stored), dtype=np.uint64)}
        elif z_new is None:
            kw = {"z": gen.normal(size=(len(stored), n_pred))}
        else:
            kw = {"z": np.asarray(z_new[kc], np.float64)[:len(stored)]}
        out.append(predict_field_call(allloc, NN, n, covfun, rows, factor_of, chain["params"]["field"], field_row,
                                      chain["params"]["beta_0"][stored - 1, 0],
                                      chain["params"]["log_scale"][stored - 1, 0],
                                      sample_batch=sample_batch, device=device, **kw))
    return {"predicted_locs": predicted_locs, "predicted_field_samples": out,
            **_field_summary(out, summary_backend, device, summary_probs, summary_thresholds)}


def _stored_coef(L, X_predicted, burn_in, match_field_thinning, add_intercept):
    """predict.R:67-91: the design rows of the new locations (n_pred x q) and,
    per chain, the de-centred cbind(beta_0, beta)[stored, subset] rows."""
    from .initialize import _model_matrix

    first = next(iter(L["records"].values()))
    stored = first["saved_field"] if match_field_thinning else np.arange(1, int(first["iterations"][-1, 0]) + 1)
    stored = stored[stored > burn_in * stored.max()].astype(int)
    mm, names = _model_matrix(X_predicted)
    mm = np.column_stack([np.ones(len(mm)), mm])
    names = ["beta_0"] + names
    if not add_intercept:
        mm, names = mm[:, 1:], names[1:]
    allnames = ["beta_0"] + list(L["X"].get("names", []))
    subset = [allnames.index(nm) for nm in names]
    coef = []
    for chain in L["records"].values():
        bm = np.column_stack([chain["params"]["beta_0"]] + ([chain["params"]["beta"]] if "beta" in chain["params"] else []))
        bm = bm[stored - 1].copy()
        if bm.shape[1] > 1:
            bm[:, 0] = bm[:, 0] - bm[:, 1:] @ L["X"]["X_mean"]
        coef.append(bm[:, subset])
    return mm, coef, stored


def mcmc_nngp_predict_fixed_effects(mcmc_nngp_list, X_predicted, burn_in=0.5, n_cores=1,
                                    match_field_thinning=True, add_intercept=False, summary_backend="host",
                                    device=-1, summary_probs=None, summary_thresholds=None, keep_samples=True):
    """predict.R:62-104.  ``summary_backend="hip"``: the samples are generated
    and summarised on ``device`` by one effects_summary call over the chains'
    stacked coefficient rows (nngp_effects_summary); with ``keep_samples=False``
    predicted_fixed_effects_samples is None and no n_samples x n_pred array
    exists on the host, with ``keep_samples=True`` the per-chain arrays are the
    device's own values.  ``summary_probs`` / ``summary_thresholds`` are
    get_summary's ``probs`` / ``thresholds`` (both backends); with either
    given, predicted_fixed_effects_summary_columns names the columns."""
    if summary_backend not in ("host", "hip"):
        raise ValueError(f"mcmc_nngp_predict_fixed_effects: summary_backend must be 'host' or 'hip', "
                         f"not {summary_backend!r}")
    mm, coef, _ = _stored_coef(mcmc_nngp_list, X_predicted, burn_in, match_field_thinning, add_intercept)
    widen = {} if summary_probs is None and summary_thresholds is None \
        else {"probs": summary_probs, "thresholds": summary_thresholds}
    if summary_backend == "hip":
        got = effects_summary(np.vstack(coef), mm, backend="hip", device=device, return_samples=keep_samples, **widen)
        summary, out = got if keep_samples else (got, None)
        if keep_samples:
            out = np.split(out, np.cumsum([len(c) for c in coef])[:-1])
    else:
        out = [c @ mm.T for c in coef]
        summary = get_summary(np.vstack(out), **widen)
        if not keep_samples:
            out = None
    res = {"X_predicted": X_predicted, "predicted_fixed_effects_samples": out,
           "predicted_fixed_effects_summary": summary}
    if widen:
        res["predicted_fixed_effects_summary_columns"] = summary_columns(summary_probs, summary_thresholds)
    return res


PHILOX_RESPONSE_MIX = 0xD1B54A32D192ED03


def mcmc_nngp_predict_response(mcmc_nngp_list, predicted_locs, X_predicted, burn_in=0.5, m=10, seed=1, noise=False,
                               summary_backend="hip", device=-1, summary_probs=None, summary_thresholds=None,
                               **predict_field_kw):
    """The map the reference's pieces add up to: intercept + fixed effects +
    predicted field (+ observation noise) at new locations, summarised per
    location with quantiles and P(value > t).

    The field samples come from mcmc_nngp_predict_field(engine="batched")
    (``m``, ``seed``, ``device`` and ``predict_field_kw`` go there); they are
    field - beta_0.  One effects_summary call then adds, per stored iteration
    (the field's thinning), the de-centred cbind(beta_0, beta) row times
    cbind(1, X_predicted) -- the beta_0 column alone when the model has no
    covariates (``X_predicted=None``) -- to that iteration's field sample, the
    per-chain field arrays being its addend blocks, read where they lie.
    ``noise=True`` adds exp(log_noise_variance / 2) times a Philox / AS241
    normal: key (seed + 0xD1B54A32D192ED03) mod 2^64, counter = the sample's
    ordinal in the chains' stack.  ``summary_backend="host"`` does the same
    through numpy.  Returns predicted_locs, predicted_response_summary, its
    column names and the field prediction's own dict."""
    if summary_backend not in ("host", "hip"):
        raise ValueError(f"mcmc_nngp_predict_response: summary_backend must be 'host' or 'hip', "
                         f"not {summary_backend!r}")
    L = mcmc_nngp_list
    predict_field_kw.setdefault("summary_backend", summary_backend)
    field = mcmc_nngp_predict_field(L, predicted_locs, burn_in=burn_in, m=m, seed=seed, device=device,
                                    engine="batched", **predict_field_kw)
    n_pred = field["predicted_locs"].shape[0]
    if X_predicted is None:
        X_predicted = np.zeros((n_pred, 0))
    mm, coef, stored = _stored_coef(L, X_predicted, burn_in, True, True)
    kw = {}
    if noise:
        kw = {"noise_sd": np.concatenate([np.exp(0.5 * c["params"]["log_noise_variance"][stored - 1, 0])
                                          for c in L["records"].values()]),
              "seed": (int(seed) + PHILOX_RESPONSE_MIX) % 2 ** 64,
              "counter": np.arange(sum(len(c) for c in coef), dtype=np.uint64)}
    summary = effects_summary(np.vstack(coef), mm, addend=field["predicted_field_samples"], probs=summary_probs,
                              thresholds=summary_thresholds, backend=summary_backend, device=device, **kw)
    return {"predicted_locs": field["predicted_locs"], "predicted_response_summary": summary,
            "predicted_response_summary_columns": summary_columns(summary_probs, summary_thresholds),
            "field_prediction": field}


def mcmc_nngp_score_response(mcmc_nngp_list, predicted_locs, X_predicted, y_new, burn_in=0.5, m=10, seed=1,
                             backend="hip", device=-1, **predict_field_kw):
    """Scores of held-out observations ``y_new`` at ``predicted_locs`` (one per
    location): the held-out counterpart of mcmc_nngp_criteria.

    The field samples come from mcmc_nngp_predict_field(engine="batched") as in
    mcmc_nngp_predict_response (field - beta_0; ``m``, ``seed``, ``device`` and
    ``predict_field_kw`` go there), the regression term is the de-centred
    cbind(beta_0, beta) row against cbind(1, X_predicted), the noise variance
    that iteration's exp(log_noise_variance); pointwise_loglik(``backend``)
    reduces them with the per-chain field arrays as its blocks, read where they
    lie.  Returns ``pointwise`` (n_pred x 6, ``columns``), ``log_score`` (the
    mean of lppd), ``rmse`` of fit_mean, ``pit``, ``coverage_95`` (the share of
    pit in [0.025, 0.975]) and the field prediction's own dict."""
    if backend not in ("host", "hip"):
        raise ValueError(f"mcmc_nngp_score_response: backend must be 'host' or 'hip', not {backend!r}")
    L = mcmc_nngp_list
    predict_field_kw.setdefault("summary_backend", backend)
    field = mcmc_nngp_predict_field(L, predicted_locs, burn_in=burn_in, m=m, seed=seed, device=device,
                                    engine="batched", **predict_field_kw)
    n_pred = field["predicted_locs"].shape[0]
    y_new = np.asarray(y_new, np.float64).reshape(-1)
    if y_new.size != n_pred:
        raise ValueError("mcmc_nngp_score_response: y_new needs one value per predicted location")
    if X_predicted is None:
        X_predicted = np.zeros((n_pred, 0))
    mm, coef, stored = _stored_coef(L, X_predicted, burn_in, True, True)
    lnv = np.concatenate([np.asarray(c["params"]["log_noise_variance"], np.float64).reshape(-1)[stored - 1]
                          for c in L["records"].values()])
    pw = pointwise_loglik(y_new, np.arange(1, n_pred + 1), field["predicted_field_samples"], lnv,
                          coef=np.vstack(coef), X=mm, backend=backend, device=device)
    pit = pw[:, 5]
    return {"predicted_locs": field["predicted_locs"], "pointwise": pw, "columns": list(POINTWISE_COLUMNS),
            "log_score": float(pw[:, 3].mean()), "rmse": float(np.sqrt(np.mean((y_new - pw[:, 0]) ** 2))),
            "pit": pit, "coverage_95": float(np.mean((pit >= 0.025) & (pit <= 0.975))), "field_prediction": field}
