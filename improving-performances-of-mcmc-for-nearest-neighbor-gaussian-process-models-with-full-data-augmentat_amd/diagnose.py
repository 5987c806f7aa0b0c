"""Convergence diagnostics used by the run loop's stop rule
(Scripts/mcmc_nngp_diagnose.R:1-24 Gelman_Rubin_Brooks, :107-118 ESS).

Out of the hot-path scope; restated here only so that
``mcmc_nngp_run``'s early-stop logic (run.R:38-46) behaves like the
reference.  ESS uses an AR(p)-spectral estimate at frequency 0 in the spirit
of coda::effectiveSize (coda is not available: not parity-checked).
"""
from __future__ import annotations

import numpy as np


def _samples(records, burn_in, n=None):
    out = []
    for chain in records.values():
        p = chain["params"]
        nn = n if n is not None else p["beta_0"].shape[0]
        start = max(int(burn_in * nn) - 1, 0)
        cols, names = [], []
        for k, v in p.items():
            if k == "field":
                continue
            v = np.asarray(v)
            v = v[:, None] if v.ndim == 1 else v
            cols.append(v[start:nn])
            names += [k] if v.shape[1] == 1 else [f"{k}{j + 1}" for j in range(v.shape[1])]
        out.append(np.column_stack(cols))
    return out, names


def Gelman_Rubin_Brooks(records, burn_in=0.5, n=None):
    samples, names = _samples(records, burn_in, n)
    n = n if n is not None else next(iter(records.values()))["params"]["beta_0"].shape[0]
    m = len(samples)
    W = sum(np.atleast_2d(np.cov(s, rowvar=False)) for s in samples) / m
    means = np.array([s.mean(0) for s in samples])
    Bv = np.atleast_2d(np.cov(means, rowvar=False))
    try:
        ev = np.linalg.svd(np.linalg.solve(W, Bv), compute_uv=False)[0]
    except np.linalg.LinAlgError:
        ev = np.inf
    mpsrf = (n - 1) / n + (m + 1) / m * ev
    ind = ((m + 1) / m) * ((n - 1) / n) * (np.diag(Bv) / np.diag(W)) + (n + 1) / n
    return {"R_hat": np.concatenate([[mpsrf], ind]), "names": ["Multivariate"] + names,
            "within_variance": W}


def _ess_1d(x, max_order=None):
    x = np.asarray(x, np.float64)
    n = len(x)
    if n < 4 or np.var(x) == 0:
        return float(n)
    x = x - x.mean()
    max_order = max_order or min(n - 1, int(10 * np.log10(n)))
    acf = np.array([x[: n - k] @ x[k:] / n for k in range(max_order + 1)])
    best = (np.inf, 0, acf[0])
    # Levinson-Durbin, AIC order selection (as stats::ar.yw)
    phi = np.zeros(0)
    v = acf[0]
    aic0 = n * np.log(v)
    best = (aic0, phi.copy(), v)
    for k in range(1, max_order + 1):
        kk = (acf[k] - (phi @ acf[1:k][::-1] if k > 1 else 0.0)) / v
        phi = np.concatenate([phi - kk * phi[::-1], [kk]])
        v = v * (1 - kk * kk)
        if v <= 0:
            break
        aic = n * np.log(v) + 2 * k
        if aic < best[0]:
            best = (aic, phi.copy(), v)
    _, phi, v = best
    spec0 = v / (1 - phi.sum()) ** 2
    return float(n * acf[0] / spec0) if spec0 > 0 else float(n)


def ESS(records, burn_in=0.5):
    samples, names = _samples(records, burn_in)
    E = np.array([[_ess_1d(s[:, j]) for j in range(s.shape[1])] for s in samples])
    return np.vstack([E, E.sum(0)]), names


FIELD_DIAG_COLS = ["R_hat", "ess", "ess_min", "W", "Bv"]
_HOST_COLS = 16384  # columns per pass of the host backend (bounds its temporaries)


def _ess_columns(xc):
    """_ess_1d for every column of the centred S x n matrix ``xc`` at once
    (loops over lags and orders only) -> (ess (n,), order (n,) int32)."""
    S, n = xc.shape
    if S < 4:
        return np.full(n, float(S)), np.zeros(n, np.int32)
    P = min(S - 1, int(10 * np.log10(S)))
    acf = np.stack([(xc[: S - l] * xc[l:]).sum(0) / S for l in range(P + 1)])
    zero = acf[0] == 0
    with np.errstate(all="ignore"):
        v = acf[0].copy()
        best_aic, best_v, best_sum = S * np.log(v), v.copy(), np.zeros(n)
        order = np.zeros(n, np.int32)
        phi = np.zeros((P, n))
        live = ~zero  # the recursion of a column ends at its first v <= 0
        for k in range(1, P + 1):
            s = (phi[: k - 1] * acf[k - 1:0:-1]).sum(0) if k > 1 else 0.0
            kk = (acf[k] - s) / v
            phi[: k - 1] = phi[: k - 1] - kk * phi[: k - 1][::-1]
            phi[k - 1] = kk
            v = v * (1 - kk * kk)
            live &= ~(v <= 0)
            better = live & (S * np.log(v) + 2 * k < best_aic)
            best_aic = np.where(better, S * np.log(v) + 2 * k, best_aic)
            best_v = np.where(better, v, best_v)
            best_sum = np.where(better, phi[:k].sum(0), best_sum)
            order[better] = k
        spec0 = best_v / (1 - best_sum) ** 2
        ess = np.where(spec0 > 0, S * acf[0] / spec0, float(S))
    ess[zero] = float(S)
    return ess, order


def _field_diag_host(blocks, off):
    m, (S, n) = len(blocks), blocks[0].shape
    out = np.empty((n, 5))
    order = np.zeros((m, n), np.int32)
    for c0 in range(0, n, _HOST_COLS):
        c1 = min(n, c0 + _HOST_COLS)
        mean, var, ess = (np.empty((m, c1 - c0)) for _ in range(3))
        nan = np.zeros(c1 - c0, bool)
        for k, b in enumerate(blocks):
            x = np.array(b[:, c0:c1], np.float64)
            if off is not None:
                x -= off[k * S:(k + 1) * S, None]
            nan |= np.isnan(x).any(0)
            mean[k] = x.sum(0) / S
            xc = x - mean[k]
            var[k] = (xc * xc).sum(0) / (S - 1)
            ess[k], order[k, c0:c1] = _ess_columns(xc)
        with np.errstate(all="ignore"):
            W = var.sum(0) / m
            d = mean - mean.sum(0) / m
            Bv = (d * d).sum(0) / np.float64(m - 1)
            r = ((m + 1) / m) * ((S - 1) / S) * (Bv / W) + (S + 1) / S
        o = np.column_stack([r, ess.sum(0), ess.min(0), W, Bv])
        o[nan] = np.nan
        order[:, c0:c1][:, nan] = 0
        out[c0:c1] = o
    return out, order


def field_diagnostics(blocks, row_offset=None, backend="host", device=-1, chunk_cols=0, return_order=False):
    """R-hat and effective sample size of every field location
    (Scripts/mcmc_nngp_diagnose.R:1-24 Individual_PSRF with n := S, :107-118 ESS).

    ``blocks``: one (S, n) array per chain, the saved rows after burn-in;
    ``row_offset`` (chains x S values in stack order) is subtracted from each
    row first.  Per chain and column the algorithm of ``_ess_1d`` gives ess_k
    and the AR order; per location W = mean of the chains' variances, Bv =
    variance of the chain means, R_hat = ((m+1)/m) ((S-1)/S) (Bv/W) + (S+1)/S,
    ess = sum of ess_k, ess_min their minimum.  Returns an (n, 5) array with
    the columns ``FIELD_DIAG_COLS`` (and the (chains, n) orders with
    ``return_order``).  ``backend="host"`` is numpy; ``backend="hip"`` runs
    nngp_field_diag of libnngp.so on ``device``: float64 row-contiguous blocks
    are passed where they lie, any other block is copied, ``chunk_cols``
    columns are staged per launch (0: automatic).  No fallback: without a GPU
    the hip backend raises NNGPError (status 6)."""
    if backend not in ("host", "hip"):
        raise ValueError(f"field_diagnostics: backend must be 'host' or 'hip', not {backend!r}")
    if isinstance(blocks, np.ndarray) and blocks.ndim == 2:
        blocks = [blocks]
    bs = []
    for b in blocks:
        b = np.asarray(b)
        if b.ndim != 2:
            raise ValueError("field_diagnostics: every block must be 2-D (saved rows x locations)")
        if backend == "hip" and (b.dtype != np.float64 or not b.flags.c_contiguous):
            b = np.ascontiguousarray(b, np.float64)
        bs.append(b)
    if not bs or any(b.shape != bs[0].shape for b in bs):
        raise ValueError("field_diagnostics: the chains' blocks must have one shape")
    m, (S, n) = len(bs), bs[0].shape
    off = None
    if row_offset is not None:
        off = np.ascontiguousarray(np.asarray(row_offset, np.float64).reshape(-1))
        if off.size != m * S:
            raise ValueError("field_diagnostics: row_offset needs one entry per chain and row")
    if backend == "hip":
        import ctypes as C

        from . import _lib

        ptrs = (C.c_void_p * m)(*[b.ctypes.data for b in bs])
        out = np.empty((5, max(n, 1)))  # n x 5 column-major
        order = np.zeros((m, max(n, 1)), np.int32) if return_order else None
        _lib.check(_lib.lib.nngp_field_diag(int(device), ptrs, m, S, n, None if off is None else off.ctypes.data,
                                            int(chunk_cols), out, None if order is None else order.ctypes.data))
        out = np.ascontiguousarray(out.T)
    else:
        if n < 1 or not 2 <= S:
            raise ValueError("field_diagnostics: needs at least two rows and one location")
        out, order = _field_diag_host(bs, off)
    return (out, order) if return_order else out


def field_diagnostics_stats():
    """HIP-event times and staging size of this thread's last device
    field_diagnostics (nngp_field_diag_stats)."""
    import ctypes as C

    from . import _lib

    cp, kn, by, w = C.c_double(), C.c_double(), C.c_longlong(), C.c_int()
    _lib.check(_lib.lib.nngp_field_diag_stats(C.byref(cp), C.byref(kn), C.byref(by), C.byref(w)))
    return {"copy_ms": cp.value, "kernel_ms": kn.value, "staged_bytes": by.value, "chunk_cols": w.value}


def field_digest(diag):
    """The few numbers of an (n, 5) field_diagnostics result worth printing.
    The R_hat quantiles and the share above 1.1 are taken over the locations
    with a finite R_hat (``n_finite_R_hat`` of ``n_locations``; a constant
    column has none), ess_min and ess_median over the non-NaN ess values."""
    r, ess = diag[:, 0], diag[:, 1]
    ok = np.isfinite(r)
    q = np.quantile(r[ok], [0.5, 0.9, 0.99]) if ok.any() else np.full(3, np.nan)
    worst = int(np.argmax(np.where(np.isnan(r), -np.inf, r)))
    e = ess[~np.isnan(ess)]
    return {"R_hat_max": float(r[worst]), "R_hat_argmax": worst,
            "R_hat_q0.5": float(q[0]), "R_hat_q0.9": float(q[1]), "R_hat_q0.99": float(q[2]),
            "ess_min": float(e.min()) if e.size else float("nan"),
            "ess_median": float(np.median(e)) if e.size else float("nan"),
            "share_R_hat_above_1.1": float(np.mean(r[ok] > 1.1)) if ok.any() else float("nan"),
            "n_finite_R_hat": int(ok.sum()), "n_locations": int(r.size)}


def Field_diagnostics(mcmc_nngp_list, burn_in=0.5, backend="host", device=-1):
    """field_diagnostics of the saved field rows of a run, selected as
    mcmc_nngp_estimate selects them for res["field"] (saved_field > it *
    burn_in; each chain's block a suffix view of its records where the
    selection is one; beta_0 of the saved iterations as row offsets).
    Returns the five arrays by name and ``digest`` (field_digest)."""
    recs = mcmc_nngp_list["records"]
    first = next(iter(recs.values()))
    it = int(first["iterations"][-1, 0])
    saved = first["saved_field"]
    sel = saved > it * burn_in
    idx = np.nonzero(sel)[0]
    suffix = idx.size > 0 and idx[0] + idx.size == sel.size
    b0_rows = saved[sel].astype(int) - 1
    fs = []
    for c in recs.values():
        f = c["params"]["field"]
        fs.append(f[idx[0]:] if suffix and f.shape[0] == sel.size else f[sel])
    offs = np.concatenate([c["params"]["beta_0"][b0_rows, 0] for c in recs.values()])
    d = field_diagnostics(fs, row_offset=offs, backend=backend, device=device)
    out = {nm: d[:, j].copy() for j, nm in enumerate(FIELD_DIAG_COLS)}
    out["digest"] = field_digest(d)
    return out
