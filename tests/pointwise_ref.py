"""High-precision reference and error bound for pointwise_loglik (plain
helpers, no fixtures): the six reductions of include/nngp.h's
nngp_pointwise_loglik with mpmath at 50 digits on the same doubles, and a
bound on what an fp64 evaluation of the stated arithmetic can differ from
them by.  tests/test_pointwise_loglik.py (host backend) and
tests/test_gpu_pointwise_loglik.py (device) share both.

The bound, per observation (u = 2^-53, gamma(k) = k u / (1 - k u); U_exp,
U_log, U_erfc = the ulp errors granted to exp, log and erfc, 1 ulp = 2 u
relative), follows the operations in order:

  mean  q products and sums (q - 1 fma, 1 product, 1 sum): E_m = gamma(q + 1)
        (sum_k |coef X| + |field|); 0 for q = 0.
  r     E_r = E_m + u (|r| + E_m).
  h, g  host exp and sqrt: relative 2 u each.  a: E_a = u (3.5 + |lnv| / 2)
        (log(2 pi) from libm, one sum).
  ll    Q = h r^2 by two or three products: E_Q = h (2 |r| E_r + E_r^2) +
        4.01 u h (|r| + E_r)^2; E_ll = (E_Q + E_a)(1 + u) + u |ll|.
  fit_mean, ll_mean   S - 1 sums and a division: (gamma(S) sum |x_s| +
        (1 + gamma(S)) sum E_s) / S.
  ll_var  d = ll - ll_mean: E_d = E_ll + E_llmean + u (|d| + E_ll + E_llmean);
        [(1 + gamma) sum (2 |d| E_d + E_d^2) + gamma(S + 2) sum d^2] / (S - 1).
  lppd  M + log sum exp(ll_hat - M) = log sum exp(ll_hat) exactly, within
        max E_ll of the true value; rounding x = ll - M scales exp(x) by
        (1 + |x| u): rho_x = u sum w |x| / sum w (w = exp(x), |x| widened by
        2 max E_ll); rho = rho_x + 2 u U_exp + gamma(S - 1) is the relative
        error of the sum, an absolute one of its log; log: 2 u U_log (log sum
        + rho); the two roundings of (M + log) - log S: u |lppd + log S| +
        u |lppd|; log S from the host: 2 u log S.
  log_cpo  the same on -ll.
  pit   t = (r g) C: E_t = (g E_r + 3 u |r g|) C (1 + 2 u) + 2 u |t|; the slope
        of 0.5 erfc(-t) is exp(-t^2) / sqrt(pi), taken at the end of
        [|t| - E_t, |t|] nearer 0; E_p = slope E_t + 2 u U_erfc p; then as
        fit_mean.

Everything is multiplied by 1 + 1e-9 for the second-order terms left out."""
import mpmath
import numpy as np

_MP = mpmath.mp.clone()
_MP.dps = 50
U = 2.0 ** -53
COLS = ["fit_mean", "ll_mean", "ll_var", "lppd", "log_cpo", "pit"]


def _gamma(k):
    return k * U / (1 - k * U)


def ulps(got, ref_mp):
    """|got - ref| in ulps of the double nearest ref (ref: an mpf)."""
    ref = float(ref_mp)
    if ref == 0.0:
        return 0.0 if got == 0.0 else np.inf
    return float(abs(_MP.mpf(float(got)) - ref_mp) / _MP.mpf(float(np.spacing(abs(ref)))))


def reference(y, obs_loc, field, lnv, coef=None, X=None, u_exp=1.0, u_log=1.0, u_erfc=1.0):
    """-> (ref, bound, extra): ref and bound (n_obs, 6) float64 (a NaN input
    gives NaN rows in both); extra["mp"]: the six mpf values per observation
    (None for a NaN row), extra["ll_min"], extra["ll_max"] per observation."""
    mp = _MP
    y = np.asarray(y, np.float64)
    loc = np.asarray(obs_loc).astype(np.int64) - 1
    field = np.asarray(field, np.float64)
    lnv = np.asarray(lnv, np.float64)
    S = field.shape[0]
    q = 0 if coef is None else np.asarray(coef).shape[1]
    two_pi = 2 * mp.pi
    a = [-(mp.log(two_pi) + mp.mpf(float(v))) / 2 for v in lnv]
    h = [mp.exp(-mp.mpf(float(v))) / 2 for v in lnv]
    g = [mp.sqrt(2 * v) for v in h]
    e_a = [U * (3.5 + abs(float(v)) / 2) for v in lnv]
    C = mp.sqrt(mp.mpf(1) / 2)
    inv_sqrt_pi = 1 / mp.sqrt(mp.pi)
    log_S = mp.log(S)
    gq, gS = _gamma(q + 1), _gamma(S)
    ref = np.full((y.size, 6), np.nan)
    bound = np.full((y.size, 6), np.nan)
    mps, ll_min, ll_max = [], np.full(y.size, np.nan), np.full(y.size, np.nan)
    for i in range(y.size):
        row_nan = np.isnan(y[i]) or np.isnan(field[:, loc[i]]).any() or (q and np.isnan(X[i]).any())
        if row_nan:
            mps.append(None)
            continue
        yi = mp.mpf(float(y[i]))
        mean, ll, p, e_m, e_ll, e_p = [], [], [], [], [], []
        for s in range(S):
            f = mp.mpf(float(field[s, loc[i]]))
            acc, mag = mp.mpf(0), abs(f)
            for k in range(q):
                t = mp.mpf(float(coef[s, k])) * mp.mpf(float(X[i, k]))
                acc += t
                mag += abs(t)
            m = f + acc
            em = gq * mag if q else mp.mpf(0)
            r = yi - m
            er = em + U * (abs(r) + em)
            l = a[s] - h[s] * r * r
            eq = h[s] * (2 * abs(r) * er + er * er) + 4.01 * U * h[s] * (abs(r) + er) ** 2
            el = (eq + e_a[s]) * (1 + U) + U * abs(l)
            t = r * g[s] * C
            et = (g[s] * er + 3 * U * abs(r * g[s])) * C * (1 + 2 * U) + 2 * U * abs(t)
            ps = mp.erfc(-t) / 2
            near = max(abs(t) - et, mp.mpf(0))
            ep = mp.exp(-near * near) * inv_sqrt_pi * et + 2 * U * u_erfc * ps
            mean.append(m), ll.append(l), p.append(ps), e_m.append(em), e_ll.append(el), e_p.append(ep)
        fit, llm, pit = sum(mean) / S, sum(ll) / S, sum(p) / S
        b_fit = (gS * sum(abs(v) for v in mean) + (1 + gS) * sum(e_m)) / S
        b_llm = (gS * sum(abs(v) for v in ll) + (1 + gS) * sum(e_ll)) / S
        b_pit = (gS * sum(p) + (1 + gS) * sum(e_p)) / S
        if S > 1:
            d = [v - llm for v in ll]
            ed = [e + b_llm + U * (abs(dv) + e + b_llm) for e, dv in zip(e_ll, d)]
            var = sum(dv * dv for dv in d) / (S - 1)
            b_var = ((1 + gS) * sum(2 * abs(dv) * e + e * e for dv, e in zip(d, ed))
                     + _gamma(S + 2) * sum(dv * dv for dv in d)) / (S - 1)
        else:
            var = b_var = mp.nan
        e_max = max(e_ll)

        def lse(vals):
            M = max(vals)
            x = [v - M for v in vals]
            w = [mp.exp(v) for v in x]
            tot = sum(w)
            val = M + mp.log(tot) - log_S
            rho = U * sum(wv * (abs(xv) + 2 * e_max) for wv, xv in zip(w, x)) / tot + 2 * U * u_exp + _gamma(S - 1)
            b = (e_max + rho + 2 * U * u_log * (mp.log(tot) + rho) + U * (abs(val + log_S) + e_max + rho)
                 + U * (abs(val) + e_max + rho) + 2 * U * log_S)
            return val, b

        lppd, b_lppd = lse(ll)
        ncpo, b_cpo = lse([-v for v in ll])
        vals = [fit, llm, var, lppd, -ncpo, pit]
        bs = [b_fit, b_llm, b_var, b_lppd, b_cpo, b_pit]
        mps.append(vals)
        ref[i] = [float(v) for v in vals]
        bound[i] = [float(b * (1 + 1e-9)) for b in bs]
        ll_min[i], ll_max[i] = float(min(ll)), float(max(ll))
    return ref, bound, {"mp": mps, "ll_min": ll_min, "ll_max": ll_max}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries with a finite reference; the
    NaN pattern must agree (ll_var of one sample, poisoned rows)."""
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the reference's"
    ok = ~np.isnan(ref)
    assert np.all(np.isfinite(got[ok])), "a non-finite output where the reference is finite"
    return float(np.max(np.abs(got[ok] - ref[ok]) / bound[ok])) if ok.any() else 0.0


def problem(S, n, q, seed, per_loc=(0, 1, 3), empty=()):
    """A random problem: observations per location drawn from ``per_loc``
    (locations in ``empty``, 0-based, get none); rows come sorted by location.
    -> dict(y, obs_loc, field, lnv, coef, X)."""
    rng = np.random.default_rng(seed)
    counts = rng.choice(per_loc, size=n)
    counts[list(empty)] = 0
    if counts.sum() == 0:
        counts[0] = 1
    loc = np.repeat(np.arange(1, n + 1), counts).astype(np.int32)
    n_obs = loc.size
    field = 1.0 + rng.normal(size=(S, n))
    lnv = rng.normal(size=S) * 0.7 - 0.5
    coef = rng.normal(size=(S, q)) if q else None
    X = rng.normal(size=(n_obs, q)) if q else None
    y = 1.0 + rng.normal(size=n_obs) * 1.5
    return {"y": y, "obs_loc": loc, "field": field, "lnv": lnv, "coef": coef, "X": X}


def extreme_problem(S=9, odd=4):
    """One observation whose residual is about 40 noise sd in every sample
    but sample ``odd`` (about 1 sd there): ll spans about -800 .. -1."""
    rng = np.random.default_rng(5)
    lnv = rng.normal(size=S) * 0.01
    field = rng.normal(size=(S, 3)) * 0.01
    field[odd, 1] = 39.0
    return {"y": np.array([40.0]), "obs_loc": np.array([2], np.int32), "field": field, "lnv": lnv,
            "coef": None, "X": None}


def run_list(rng, chains=2, iters=40, thin=2, n=15, p=2, extra_obs=6):
    """A small synthetic mcmc_nngp_list: what mcmc_nngp_criteria reads."""
    saved = np.arange(thin, iters + 1, thin, dtype=np.float64)
    lm = np.concatenate([np.arange(1, n + 1), rng.integers(1, n + 1, size=extra_obs)]).astype(np.int32)
    recs = {}
    for k in range(chains):
        par = {"beta_0": rng.normal(size=(iters, 1)), "log_noise_variance": rng.normal(size=(iters, 1)) * 0.3,
               "field": 1.0 + rng.normal(size=(len(saved), n))}
        if p:
            par["beta"] = rng.normal(size=(iters, p)) * 0.5
        recs[f"chain_{k + 1}"] = {"iterations": np.column_stack([np.arange(1, iters + 1), np.zeros(iters)]),
                                  "saved_field": saved, "params": par}
    X = {"X": None}
    if p:
        XX = rng.normal(size=(len(lm), p))
        X = {"X": XX - XX.mean(0), "X_mean": XX.mean(0), "names": [f"V{j + 1}" for j in range(p)]}
    return {"records": recs, "X": X, "observed_field": 1.0 + rng.normal(size=len(lm)),
            "vecchia_approx": {"locs_match": lm}}
