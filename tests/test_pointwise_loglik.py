"""pointwise_loglik / mcmc_nngp_criteria / nngp_pointwise_loglik without a GPU:
the host backend against the 50-digit reference of tests/pointwise_ref.py
within that module's bound, the hand-checkable identities, the totals of
mcmc_nngp_criteria against a direct numpy evaluation, and the argument checks
of the C entry, which are made before any HIP call.

The host backend's bound grants numpy's exp and log 4 ulp (the limit numpy's
own accuracy tests hold its SIMD loops to) and scipy's erfc 8 ulp (cephes
documents a peak relative error of 1.3e-15, about 6 ulp, over 0 .. 26.6)."""
import ctypes as C

import numpy as np
import pytest

import pointwise_ref as R

HOST_ULP = dict(u_exp=4.0, u_log=4.0, u_erfc=8.0)
CASES = [(1, 7, 0, 1), (2, 33, 1, 2), (3, 64, 5, 3), (65, 100, 5, 4), (65, 40, 0, 5), (3, 9, 1, 6)]


@pytest.mark.parametrize("S,n,q,seed", CASES)
def test_host_backend_against_high_precision(P, S, n, q, seed):
    pr = R.problem(S, n, q, seed)
    if (S, q) == (65, 5):
        assert pr["y"].size <= 259
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"])
    ref, bound, _ = R.reference(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], pr["coef"], pr["X"], **HOST_ULP)
    assert got.shape == (pr["y"].size, 6) and P.POINTWISE_COLUMNS == R.COLS
    ratio = R.worst_ratio(got, ref, bound)
    print(f"[pointwise host S={S} n={n} q={q}] n_obs {pr['y'].size}  max err / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_n_obs_259_blocks_and_default_backend(P):
    """The largest shape (259 observations, one per location), the field given
    as three blocks (one empty), q = 1."""
    pr = R.problem(3, 259, 1, 11, per_loc=(1,))
    f = pr["field"]
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], [f[:1], f[1:1], f[1:]], pr["lnv"], coef=pr["coef"], X=pr["X"],
                             backend="host")
    ref, bound, _ = R.reference(pr["y"], pr["obs_loc"], f, pr["lnv"], pr["coef"], pr["X"], **HOST_ULP)
    assert got.shape == (259, 6) and R.worst_ratio(got, ref, bound) <= 1.0


def test_rows_come_back_in_the_callers_order(P):
    pr = R.problem(5, 30, 2, 7)
    base = P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"])
    perm = np.random.default_rng(0).permutation(pr["y"].size)
    got = P.pointwise_loglik(pr["y"][perm], pr["obs_loc"][perm], pr["field"], pr["lnv"], coef=pr["coef"],
                             X=pr["X"][perm])
    np.testing.assert_array_equal(got, base[perm])


def test_bad_python_arguments(P):
    pr = R.problem(4, 6, 2, 1)
    y, loc, f, lnv, coef, X = (pr[k] for k in ("y", "obs_loc", "field", "lnv", "coef", "X"))
    with pytest.raises(ValueError):
        P.pointwise_loglik(y, loc, f, lnv, backend="cuda")
    with pytest.raises(ValueError):
        P.pointwise_loglik(y, loc, f, lnv[:-1])
    with pytest.raises(ValueError):
        P.pointwise_loglik(y, loc + 6, f, lnv)
    with pytest.raises(ValueError):
        P.pointwise_loglik(y, loc, f, lnv, coef=coef)
    with pytest.raises(ValueError):
        P.pointwise_loglik(y, loc, f, lnv, coef=coef[:, :1], X=X)
    with pytest.raises(ValueError):
        P.pointwise_loglik(y[:-1], loc, f, lnv)


def test_one_sample_identities(P):
    pr = R.problem(1, 12, 2, 8)
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"])
    np.testing.assert_array_equal(got[:, 3], got[:, 1])
    np.testing.assert_array_equal(got[:, 4], got[:, 1])
    assert np.isnan(got[:, 2]).all() and np.isfinite(got[:, [0, 1, 5]]).all()


def test_identical_samples_identities(P):
    pr = R.problem(1, 12, 2, 9)
    rep = lambda a, S: np.repeat(a, S, axis=0)  # noqa: E731
    # two samples: x + x and its half are exact, so the variance is 0 to the bit
    # ((M + log 2) - log 2 rounds: lppd and log_cpo are held to the bound below)
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], rep(pr["field"], 2), rep(pr["lnv"], 2), coef=rep(pr["coef"], 2),
                             X=pr["X"])
    np.testing.assert_array_equal(got[:, 2], 0.0)
    # seven: the running sum rounds too, so all three hold within the bound
    args = (pr["y"], pr["obs_loc"], rep(pr["field"], 7), rep(pr["lnv"], 7))
    got = P.pointwise_loglik(*args, coef=rep(pr["coef"], 7), X=pr["X"])
    _, bound, _ = R.reference(*args, rep(pr["coef"], 7), pr["X"], **HOST_ULP)
    assert np.all(np.abs(got[:, 2]) <= bound[:, 2])
    assert np.all(np.abs(got[:, 3] - got[:, 1]) <= bound[:, 3] + bound[:, 1])
    assert np.all(np.abs(got[:, 4] - got[:, 1]) <= bound[:, 4] + bound[:, 1])


def test_jensen_ordering(P):
    pr = R.problem(65, 60, 3, 10)
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"])
    slack = 1e-12 * (1 + np.abs(got[:, 1]))  # rounding only: the inequalities are strict here
    assert np.all(got[:, 4] <= got[:, 1] + slack) and np.all(got[:, 1] <= got[:, 3] + slack)
    assert np.all(got[:, 2] > 0) and np.all((got[:, 5] > 0) & (got[:, 5] < 1))


def test_nan_poisons_its_own_rows_only(P):
    pr = R.problem(4, 10, 2, 12, per_loc=(1, 2))
    y, X, f = pr["y"].copy(), pr["X"].copy(), pr["field"].copy()
    y[0] = np.nan
    X[3, 1] = np.nan
    col = int(pr["obs_loc"][-1]) - 1
    f[2, col] = np.nan
    got = P.pointwise_loglik(y, pr["obs_loc"], f, pr["lnv"], coef=pr["coef"], X=X)
    bad = np.zeros(y.size, bool)
    bad[[0, 3]] = True
    bad |= pr["obs_loc"] == col + 1
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    ref, bound, _ = R.reference(y, pr["obs_loc"], f, pr["lnv"], pr["coef"], X, **HOST_ULP)
    assert R.worst_ratio(got, ref, bound) <= 1.0


def test_extreme_spread_stays_finite(P):
    """ll from about -800 to about -1: the naive log(mean(exp(ll))) is -inf
    (asserted, so the case is known to bite); the max shift keeps lppd and
    log_cpo finite and within the bound."""
    pr = R.extreme_problem()
    ref, bound, extra = R.reference(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], **HOST_ULP)
    assert extra["ll_min"][0] < -780 and extra["ll_max"][0] > -2
    r = pr["y"][0] - pr["field"][:, 1]
    ll = -0.5 * (np.log(2 * np.pi) + pr["lnv"]) - 0.5 * np.exp(-pr["lnv"]) * r * r
    with np.errstate(divide="ignore", over="ignore"):
        naive_cpo = -np.log(np.mean(np.exp(-ll)))
        naive_lppd_all_far = np.log(np.mean(np.exp(np.delete(ll, 4))))
    assert naive_cpo == -np.inf and naive_lppd_all_far == -np.inf
    got = P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"])
    assert np.isfinite(got).all()
    ratio = R.worst_ratio(got, ref, bound)
    print(f"[pointwise host extreme] lppd {got[0, 3]:.6f} log_cpo {got[0, 4]:.6f}  max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    # every sample far: lppd itself would underflow without the shift
    far = {k: (v[np.arange(9) != 4] if k in ("field", "lnv") else v) for k, v in pr.items()}
    got = P.pointwise_loglik(far["y"], far["obs_loc"], far["field"], far["lnv"])
    ref, bound, _ = R.reference(far["y"], far["obs_loc"], far["field"], far["lnv"], **HOST_ULP)
    assert np.isfinite(got).all() and got[0, 3] < -700 and R.worst_ratio(got, ref, bound) <= 1.0


# ---------------------------------------------------------------- mcmc_nngp_criteria
@pytest.mark.parametrize("p,burn_in", [(2, 0.5), (0, 0.25)])
def test_criteria_totals_are_the_definitions(P, p, burn_in):
    rng = np.random.default_rng(21)
    L = R.run_list(rng, p=p)
    got = P.mcmc_nngp_criteria(L, burn_in=burn_in)
    # predict.py's selection: saved_field > burn_in * max, rows of params[...] at stored - 1
    saved = L["records"]["chain_1"]["saved_field"]
    stored = saved[saved > burn_in * saved.max()].astype(int)
    assert got["n_samples"] == 2 * len(stored) == 2 * (20 - int(burn_in * 20))
    y, lm = L["observed_field"], L["vecchia_approx"]["locs_match"]
    mean, lnv = [], []
    for c in L["records"].values():
        f = c["params"]["field"][np.isin(saved, stored)][:, lm - 1]
        if p:
            f = f + c["params"]["beta"][stored - 1] @ L["X"]["X"].T
        mean.append(f)
        lnv.append(c["params"]["log_noise_variance"][stored - 1, 0])
    mean, lnv = np.vstack(mean), np.concatenate(lnv)
    ll = -0.5 * (np.log(2 * np.pi) + lnv[:, None]) - 0.5 * np.exp(-lnv[:, None]) * (y - mean) ** 2
    S = ll.shape[0]
    lppd = np.log(np.exp(ll).mean(0)).sum()
    p_waic = ll.var(0, ddof=1).sum()
    lpml = -np.log(np.exp(-ll).mean(0)).sum()
    dbar = -2 * ll.mean(0).sum()
    v = np.exp(lnv.mean())
    dhat = -2 * (-0.5 * np.log(2 * np.pi * v) - 0.5 * (y - mean.mean(0)) ** 2 / v).sum()
    want = {"lppd": lppd, "p_waic": p_waic, "waic": -2 * (lppd - p_waic), "lpml": lpml, "dbar": dbar, "dhat": dhat,
            "p_dic": dbar - dhat, "dic": 2 * dbar - dhat}
    for k, w in want.items():
        assert abs(got[k] - w) <= 1e-11 * (abs(w) + abs(dbar)), (k, got[k], w)
    assert got["columns"] == P.POINTWISE_COLUMNS and got["pointwise"].shape == (len(y), 6) and S == got["n_samples"]
    np.testing.assert_allclose(got["pointwise"][:, 0], mean.mean(0), rtol=1e-13, atol=1e-14)
    with pytest.raises(ValueError):
        P.mcmc_nngp_criteria(L, burn_in=1.0)


def test_criteria_blocks_are_views_of_the_records(P, monkeypatch):
    """Per chain the tail slice of params["field"] is one block, never copied."""
    import nngp_amd.estimate as E

    L = R.run_list(np.random.default_rng(22))
    seen = {}
    real = E.pointwise_loglik

    def spy(y, obs_loc, field_blocks, lnv, **kw):
        seen["blocks"] = field_blocks
        return real(y, obs_loc, field_blocks, lnv, **kw)

    monkeypatch.setattr(E, "pointwise_loglik", spy)
    E.mcmc_nngp_criteria(L, burn_in=0.5)
    for b, c in zip(seen["blocks"], L["records"].values()):
        f = c["params"]["field"]
        assert b.base is f and b.shape == (10, f.shape[1]) and b.flags.c_contiguous
        assert b.ctypes.data == f[10:].ctypes.data


# ---------------------------------------------------------------- the C entry's argument checks
def test_abi_lists_the_new_symbols(P):
    from nngp_amd import _lib

    for s in ("nngp_pointwise_loglik", "nngp_pointwise_loglik_stats"):
        assert s in _lib.ABI_SYMBOLS and getattr(_lib.lib, s).argtypes is not None
    assert _lib.lib.nngp_abi_version() == 14
    assert P.pointwise_loglik_stats and P.mcmc_nngp_criteria and P.mcmc_nngp_score_response


def _call(lib, **over):
    """nngp_pointwise_loglik on a valid problem (S = 5, n = 4, n_obs = 3, q = 2)
    with some arguments replaced."""
    S, n, n_obs, q = (int(over.get(k, d)) for k, d in (("S", 5), ("n", 4), ("n_obs", 3), ("q", 2)))
    keep = {"y": np.ones(3), "loc": np.array([1, 3, 3], np.int32), "coef": np.ones((2, 5)), "X": np.ones((2, 3)),
            "lnv": np.zeros(5), "out": np.empty((6, 3)), "blocks": [np.ones((5, 4))], "rows": [5]}
    a = {k: keep[k] for k in ("y", "loc", "coef", "X", "lnv", "out", "blocks", "rows")}
    a["chunk_cols"] = 0
    a.update({k: v for k, v in over.items() if k not in ("S", "n", "n_obs", "q")})
    ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    bl = a["blocks"]
    blocks = None if bl is None else (C.c_void_p * len(bl))(*[ptr(b) for b in bl])
    rows = None if bl is None else (C.c_longlong * len(bl))(*a["rows"])
    return lib.nngp_pointwise_loglik(-1, ptr(a["y"]), n_obs, ptr(a["loc"]), ptr(a["coef"]), S, q, ptr(a["X"]), blocks,
                                     rows, 0 if bl is None else len(bl), n, ptr(a["lnv"]), a["chunk_cols"], ptr(a["out"]))


BAD = {
    "null y": dict(y=None),
    "null obs_loc": dict(loc=None),
    "null out": dict(out=None),
    "null log_noise_var": dict(lnv=None),
    "n_obs 0": dict(n_obs=0),
    "n 0": dict(n=0),
    "n_samples 0": dict(S=0),
    "n_samples 2^31": dict(S=2 ** 31),
    "q -1": dict(q=-1),
    "q 1025": dict(q=1025),
    "q > 0, null coef": dict(coef=None),
    "q > 0, null X": dict(X=None),
    "obs_loc decreasing": dict(loc=np.array([2, 1, 3], np.int32)),
    "obs_loc 0": dict(loc=np.array([0, 1, 3], np.int32)),
    "obs_loc above n": dict(loc=np.array([1, 3, 5], np.int32)),
    "null block": dict(blocks=[np.ones((2, 4)), None], rows=[2, 3]),
    "no blocks": dict(blocks=None),
    "block rows short": dict(blocks=[np.ones((4, 4))], rows=[4]),
    "block rows long": dict(blocks=[np.ones((3, 4)), np.ones((3, 4))], rows=[3, 3]),
    "NaN log_noise_var": dict(lnv=np.array([0.0, np.nan, 0.0, 0.0, 0.0])),
    "infinite log_noise_var": dict(lnv=np.array([0.0, 0.0, -np.inf, 0.0, 0.0])),
    "chunk_cols -1": dict(chunk_cols=-1),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_err_arg_before_any_hip_call(P, case):
    from nngp_amd import _lib

    assert _call(_lib.lib, **BAD[case]) == _lib.NNGP_ERR_ARG, case
    assert _lib.lib.nngp_ctx_last_error(None)


def test_good_arguments_pass_the_checks(P):
    """The calls the bad cases are one change away from: past the argument
    checks (no device here: NNGP_ERR_NODEV; with one they succeed)."""
    from nngp_amd import _lib

    good = [dict(), dict(q=0, coef=None, X=None), dict(blocks=[np.ones((2, 4)), np.ones((0, 4)), np.ones((3, 4))], rows=[2, 0, 3]),
            dict(loc=np.array([4, 4, 4], np.int32)), dict(chunk_cols=64)]
    for kw in good:
        assert _call(_lib.lib, **kw) in (_lib.NNGP_OK, _lib.NNGP_ERR_NODEV), kw
