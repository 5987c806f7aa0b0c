"""regression="host" / "device" in update_gaussian._chain_program, driven with
a recording numpy stand-in for the device context (no GPU): which calls and
requests each mode issues, when the Gram matrix is inverted again, and that
the host's draws come in the same order with the same numbers.

The stand-in reads every field-sized input through a rounding to 6 decimals:
the two modes form the shifted field with differently associated additions
(field - beta_0 + innov against field + (innov - beta_0)), an ulp apart, and
the rounding makes the statistics -- and with them every draw -- identical."""
import numpy as np
import pytest


def _r(a):
    return np.round(np.asarray(a, np.float64), 6)


class _NumpyCtx:
    n_chains = 1

    def __init__(self, n, lm, y, X=None, first_obs=None):
        self.n, self.lm0, self.y = n, np.asarray(lm) - 1, np.asarray(y, np.float64)
        self.calls, self.B, self.gen, self.sx_gen = [], [None, None], [0, 0], -1
        self.field = self.prop = self.mu = None
        self.step = 0

    def _log(self, name, *info):
        self.calls.append((name,) + info)

    # ---- the calls of the host path
    def factor(self, which, covfun, cp):
        self._log("factor", which)
        i, j = np.indices((self.n, self.n))
        self.B[which] = np.eye(self.n) + np.where(i > j, 0.1 * np.exp(-abs(float(cp[1])) * (i - j)), 0.0)
        self.gen[which] = max(self.gen) + 1

    def accept_factor(self):
        self._log("accept_factor")
        self.B.reverse()
        self.gen.reverse()

    def accept_field(self):
        self._log("accept_field")

    def ancillary_propose(self, b0, dls):
        self._log("ancillary_propose")

    def field_response_ratio(self, b0, lnv):
        self.step += 1
        return 1e9 if self.step % 3 == 1 else -1e9  # accepted in iterations 1, 4, ...

    def loglik(self, which, b0, ls):
        return (1e9 if self.step % 2 == 0 else -1e9) if which == 1 else 0.0  # accepted in even iterations

    def set_field(self, f):
        self._log("set_field")
        self.field = np.array(f, np.float64)

    def get_field(self):
        self._log("get_field")
        return _r(self.field)

    def set_mu(self, mu, b0):
        self._log("set_mu", mu is not None)
        self.mu = None if mu is None else np.array(mu)

    def spmv(self, which, M):
        self._log("spmv")
        return self.B[which] @ _r(M)

    def beta0_stats(self):
        self._log("beta0_stats")
        one = self.B[0] @ np.ones(self.n)
        return float(one @ one), float(one @ (self.B[0] @ _r(self.field)))

    def sum_squared_residuals(self, b0):
        return 3.0

    def sweep(self, *a):
        self._log("sweep")
        self.sweeps = getattr(self, "sweeps", 0) + 1
        self.field = _r(self.field) + 0.01 * np.sin(np.arange(self.n) + self.sweeps)


class _DesignCtx(_NumpyCtx):
    """... with the design entry points, in the host path's numpy expressions."""

    def design_set(self, X, first_obs, locs_cols):
        self._log("design_set")
        self.X, self.cols = np.asarray(X, np.float64), list(locs_cols)
        self.Xl = self.X[np.asarray(first_obs) - 1][:, self.cols]

    def design_mean_stats_chains(self, mask, b0):
        self._log("design_mean_stats_chains", mask)
        X1 = np.column_stack([np.ones(len(self.y)), self.X])
        return ((self.y - _r(self.field)[self.lm0] + b0[0]) @ X1)[None, :]

    def design_interweave_stats_chains(self, mask, shift, bl):
        self._log("design_interweave_stats_chains", mask)
        SX = self.B[0] @ _r(np.column_stack([np.ones(self.n), self.Xl]))
        refreshed = int(self.sx_gen != self.gen[0])
        self.sx_gen = self.gen[0]
        other = _r(self.field) + shift[0] + self.Xl @ bl[0]
        return ((self.B[0] @ _r(other)) @ SX)[None, :], (SX.T @ SX)[None, :, :], np.array([refreshed], np.int32)

    def design_commit_chains(self, mask, shift, bl_old, bl_new, b0, beta):
        self._log("design_commit_chains", mask)
        f = _r(self.field) + shift[0]
        if bl_old is not None:
            f = (f + self.Xl @ bl_old[0]) - self.Xl @ bl_new[0]
        self.field = f
        self.mu = b0[0] + self.X @ beta[0]


def _problem(with_locs=True):
    rng = np.random.default_rng(4)
    n = 12
    lm = np.concatenate([np.arange(1, n + 1), [3, 7, 7]])
    y = rng.normal(size=len(lm)) + 1.0
    X = rng.normal(size=(len(lm), 4))
    cols = [1, 3] if with_locs else []
    for c in cols:
        X[:, c] = rng.normal(size=n)[lm - 1]
    X = X - X.mean(0)
    X1 = np.column_stack([np.ones(len(lm)), X])
    Xd = {"X": X, "locs": np.array(cols, np.int64), "solve_1XT1X": np.linalg.inv(X1.T @ X1)}
    Xd["chol_solve_1XT1X"] = np.linalg.cholesky(Xd["solve_1XT1X"]).T
    va = {"n_obs": len(lm), "n_locs": n, "locs_match": lm, "hctam_scol_1": np.arange(1, n + 1)}
    stm = {"covfun": {"stationary_covfun": "exponential_isotropic", "shape_params": ["log_range"]}}
    state = {"params": {"beta_0": 1.0, "beta": np.zeros(4), "log_scale": -3.0, "shape": np.array([0.0]),
                        "log_noise_variance": 0.0, "field": 1.0 + rng.normal(size=n)},
             "transition_kernels": {"covariance_params_sufficient": {"logvar": -2.0},
                                    "covariance_params_ancillary": {"logvar": -2.0},
                                    "log_noise_variance": {"logvar": -1.0}}}
    return n, lm, y, Xd, va, stm, state


def _run(ctx, prob, regression, iters=6):
    """-> (result, request kinds, index into ctx.calls of the first call inside the loop)"""
    from nngp_amd.update_gaussian import _chain_program, _serve_one

    n, lm, y, Xd, va, stm, state = prob
    g = _chain_program(0, state, ctx, Xd, y, stm, va, iters, 0.0, True, 1, 0, 1, regression=regression)
    kinds, mark = [], None
    try:
        req = next(g)
        mark = len(ctx.calls)
        while True:
            kinds.append(req[0])
            req = g.send(_serve_one(ctx, req))
    except StopIteration as stop:
        return stop.value, kinds, mark


NEW = ("design_set", "design_mean_stats_chains", "design_interweave_stats_chains", "design_commit_chains", "get_mu")


def test_host_mode_is_todays_path(P):
    prob = _problem()
    ctx = _DesignCtx(prob[0], prob[1], prob[2])
    res, kinds, _ = _run(ctx, prob, "host")
    assert kinds == ["astep", "sstep", "sweep", "ssr"] * 6
    assert not [c for c in ctx.calls if c[0] in NEW]
    assert {"get_field", "spmv", "set_field", "set_mu"} <= {c[0] for c in ctx.calls}
    # the default is the host path
    from nngp_amd.update_gaussian import _chain_program
    import inspect

    assert inspect.signature(_chain_program).parameters["regression"].default == "host"


@pytest.mark.parametrize("with_locs", [True, False])
def test_device_mode_requests_calls_and_draws(P, with_locs, monkeypatch):
    import nngp_amd.update_gaussian as UG

    prob = _problem(with_locs)
    host_ctx = _NumpyCtx(prob[0], prob[1], prob[2])
    host, _, _ = _run(host_ctx, prob, "host")
    inv_calls = []
    real_inv = np.linalg.inv
    monkeypatch.setattr(UG.np.linalg, "inv", lambda a: (inv_calls.append(1), real_inv(a))[1])
    ctx = _DesignCtx(prob[0], prob[1], prob[2])
    refreshed = []
    inter = ctx.design_interweave_stats_chains

    def spy(mask, shift, bl):
        out = inter(mask, shift, bl)
        refreshed.append(int(out[2][0]))
        return out

    ctx.design_interweave_stats_chains = spy
    dev, kinds, mark = _run(ctx, prob, "device")
    monkeypatch.undo()
    per_it = ["astep", "sstep", "dmean"] + (["dinter"] if with_locs else []) + ["dcommit", "sweep", "ssr"]
    assert kinds == per_it * 6
    names = [c[0] for c in ctx.calls]
    assert names.count("design_set") == 1 and names.index("design_set") < mark
    assert names.count("design_mean_stats_chains") == 6 and names.count("design_commit_chains") == 6
    assert names.count("design_interweave_stats_chains") == (6 if with_locs else 0)
    loop = ctx.calls[mark:]
    assert not [c for c in loop if c[0] in ("spmv", "set_field") or c == ("set_mu", True)]
    assert [i for i, c in enumerate(loop) if c[0] == "get_field"] == [len(loop) - 1]  # only the final state's copy
    assert "spmv" not in names  # no interweave preparation on the host either
    if with_locs:
        # accepted proposals: iterations 1, 4 (ancillary) and 2, 4, 6 (sufficient)
        assert refreshed == [1, 1, 0, 1, 0, 1] and len(inv_calls) == sum(refreshed)
        assert host["acceptance"]["covariance_acceptance_ancillary"].tolist() == [1, 0, 0, 1, 0, 0]
    else:
        assert not inv_calls and names.count("beta0_stats") == 6
    # same draws in the same order on the same numbers: the records are equal
    for key in ("beta", "beta_0", "log_scale", "log_noise_variance", "shape"):
        np.testing.assert_array_equal(dev["records"][key], host["records"][key], err_msg=key)
    for key in ("covariance_acceptance_ancillary", "covariance_acceptance_sufficient"):
        np.testing.assert_array_equal(dev["acceptance"][key], host["acceptance"][key])
    assert np.ptp(dev["records"]["beta"], axis=0).min() > 0


def test_device_mode_needs_the_entry_points_and_a_known_value(P):
    from nngp_amd._lib import NNGPError
    from nngp_amd.update_gaussian import mcmc_nngp_update_Gaussian

    prob = _problem()
    with pytest.raises(NNGPError):
        _run(_NumpyCtx(prob[0], prob[1], prob[2]), prob, "device")  # no design_* methods: no fallback
    with pytest.raises(ValueError):
        _run(_DesignCtx(prob[0], prob[1], prob[2]), prob, "gpu")
    n, lm, y, Xd, va, stm, state = prob
    with pytest.raises(ValueError):
        mcmc_nngp_update_Gaussian(None, Xd, y, stm, va, [state], 1, contexts=[None], regression="gpu")
