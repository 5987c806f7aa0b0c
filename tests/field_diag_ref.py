"""Long-double reference of the per-location field diagnostics (plain helpers,
no fixtures; see tests/highprec.py for the practice): the algorithm of
diagnose._ess_1d and the Gelman-Rubin combination in np.longdouble (x87
extended, 64-bit significand), vectorised over columns.  Inputs are the
centred fp64 samples, taken exactly."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not extended precision here: no high-precision reference"

RHOS = (0.0, 0.5, 0.9, 0.99)


def ar1_blocks(S, n, m, seed, shift=True):
    """m chains of S x n AR(1) columns, mean 3, rho of column j = RHOS[j % 4];
    the last chain is shifted by +2 on every third column."""
    rng = np.random.default_rng(seed)
    rho = np.array([RHOS[j % 4] for j in range(n)])
    out = []
    for k in range(m):
        e = rng.standard_normal((S, n))
        x = np.empty((S, n))
        x[0] = e[0] / np.sqrt(1 - rho * rho)
        for t in range(1, S):
            x[t] = rho * x[t - 1] + e[t]
        x += 3.0
        if shift and k == m - 1:
            x[:, ::3] += 2.0
        out.append(x)
    return out


def ess_ld(x):
    """One chain's S x n block -> (mean, var, ess, order, aic_gap, d), mean, var
    and ess in longdouble; aic_gap = second lowest minus lowest AIC among the
    orders the recursion reached (inf where there is one order only); d =
    1 - sum phi at the selected order (float64)."""
    x = np.asarray(x, np.float64).astype(LD)
    S, n = x.shape
    mean = x.sum(0) / LD(S)
    xc = x - mean
    ss = (xc * xc).sum(0)
    var = ss / LD(S - 1)
    ess = np.full(n, LD(S))
    order = np.zeros(n, np.int32)
    gap = np.full(n, np.inf)
    if S < 4:
        return mean, var, ess, order, gap, np.ones(n)
    P = min(S - 1, int(10 * np.log10(S)))
    acf = np.stack([(xc[: S - l] * xc[l:]).sum(0) / LD(S) for l in range(P + 1)])
    zero = acf[0] == 0
    with np.errstate(all="ignore"):
        v = acf[0].copy()
        aics = np.full((P + 1, n), np.inf, LD)
        aics[0] = LD(S) * np.log(v)
        best_aic, best_v, best_sum = aics[0].copy(), v.copy(), np.zeros(n, LD)
        phi = np.zeros((P, n), LD)
        live = ~zero
        for k in range(1, P + 1):
            s = (phi[: k - 1] * acf[k - 1:0:-1]).sum(0) if k > 1 else LD(0)
            kk = (acf[k] - s) / v
            phi[: k - 1] = phi[: k - 1] - kk * phi[: k - 1][::-1]
            phi[k - 1] = kk
            v = v * (1 - kk * kk)
            live &= ~(v <= 0)
            aic = LD(S) * np.log(v) + LD(2 * k)
            aics[k] = np.where(live, aic, np.inf)
            better = live & (aic < best_aic)
            best_aic = np.where(better, aic, best_aic)
            best_v = np.where(better, v, best_v)
            best_sum = np.where(better, phi[:k].sum(0), best_sum)
            order[better] = k
        spec0 = best_v / (1 - best_sum) ** 2
        e = np.where(spec0 > 0, LD(S) * acf[0] / spec0, LD(S))
    ess = np.where(zero, LD(S), e)
    srt = np.sort(np.where(np.isnan(aics), np.inf, aics), axis=0)
    with np.errstate(all="ignore"):
        gap = np.where(zero, np.inf, (srt[1] - srt[0]).astype(np.float64))
    return mean, var, ess, order, gap, np.where(zero, 1.0, (1 - best_sum).astype(np.float64))


def field_diag_ld(blocks):
    """-> dict: out (n, 5) longdouble [R_hat, ess, ess_min, W, Bv], order and
    aic_gap (m, n), means, ess_k (m, n) longdouble, d (m, n)."""
    m = len(blocks)
    S = blocks[0].shape[0]
    parts = [ess_ld(b) for b in blocks]
    mean = np.stack([p[0] for p in parts])
    var = np.stack([p[1] for p in parts])
    ess = np.stack([p[2] for p in parts])
    with np.errstate(all="ignore"):
        W = var.sum(0) / LD(m)
        d = mean - mean.sum(0) / LD(m)
        Bv = (d * d).sum(0) / LD(m - 1)
        r = (LD(m + 1) / LD(m)) * (LD(S - 1) / LD(S)) * (Bv / W) + LD(S + 1) / LD(S)
    return {"out": np.column_stack([r, ess.sum(0), ess.min(0), W, Bv]),
            "order": np.stack([p[3] for p in parts]), "aic_gap": np.stack([p[4] for p in parts]), "means": mean,
            "ess_k": ess, "d": np.stack([p[5] for p in parts])}
