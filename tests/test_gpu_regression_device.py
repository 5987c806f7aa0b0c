"""The regression block on the device (nngp_design_*; update_Gaussian.R:77-83,
145-151,226-250): the three array operations against numpy with a-priori
rounding bounds, their bitwise rules (chain mask, run to run), the state a
commit leaves, the refreshed bookkeeping, and full Gibbs iterations with
regression="device" against the CPU oracle.  The primitives here run at one
shape (500 locations, 550 observations, m = 6, 3 chains);
tests/test_gpu_regression_shapes.py takes the same checks over the launch
shapes and limits.

Bounds: a sum of k floating-point operations on its longest path differs from
the exact value by at most gamma_k x the sum of the absolute values of the
products, gamma_k = k 2^-53, for any summation order; the reference side is
accumulated in 80-bit long double (2^-64 per operation: three decades below)."""
import copy

import numpy as np
import pytest

import highprec as H
from conftest import make_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
EPS = np.finfo(np.float64).eps
COV = "exponential_isotropic"
CPS = [[1.0, 0.10, 0.0], [1.2, 0.07, 0.05], [0.8, 0.15, 0.0], [0.9, 0.12, 0.02]]


def _synthetic(P, p, locs_cols0, n=500, m=6, seed=3, n_obs=None):
    """make_problem(n=500, m=6, dup_frac=0.1): 550 observations in shuffled
    order (first_obs is not the identity), p centred columns, the columns
    locs_cols0 constant within a location.  With n_obs: every location once,
    then n_obs - n random repeats.  The NNarray keeps m + 1 columns (all NA
    beyond n - 1 neighbours), so b = m + 1 also where n <= m."""
    assert np.finfo(LD).eps < 2.0 ** -60
    if n_obs is None:
        locs, NN, col, lm, y = make_problem(P, n, m, seed=seed, dup_frac=0.1)
    else:
        locs, NN, col, lm, _ = make_problem(P, n, m, seed=seed)
        rep = np.random.default_rng(seed + 200)
        lm = np.concatenate([lm, rep.integers(1, n + 1, n_obs - n).astype(np.int32)])
        y = rep.normal(size=n_obs)
    NN = H.pad_na(NN, m + 1)
    rng = np.random.default_rng(seed + 100)
    perm = rng.permutation(len(lm))
    lm, y = lm[perm], y[perm] + 2.0
    X = rng.normal(size=(len(lm), p))
    for c in locs_cols0:
        X[:, c] = rng.normal(size=n)[lm - 1]
    X = X - X.mean(0)
    first_obs = (np.unique(lm, return_index=True)[1] + 1).astype(np.int32)  # all of 1..n occur
    return {"locs": locs, "NN": NN, "col": col, "lm": lm, "y": y, "X": X, "first_obs": first_obs,
            "locs_cols": list(locs_cols0), "n": n, "m": m}


@pytest.fixture(scope="module")
def prob(P):
    return _synthetic(P, 70, [2, 0, 69])  # locs_cols = [3, 1, 70], 1-based


def _chain_inputs(pr, C=3):
    rng = np.random.default_rng(17)
    n, p, ql = pr["n"], pr["X"].shape[1], len(pr["locs_cols"])
    return {"fields": [2.0 + rng.normal(size=n) for _ in range(C)], "b0": rng.normal(size=C) + 2.0,
            "shift": rng.normal(size=C) * 0.3, "bl_old": rng.normal(size=(C, ql)), "bl_new": rng.normal(size=(C, ql)),
            "b0_new": rng.normal(size=C) + 2.0, "beta": rng.normal(size=(C, p))}


def _open(P, pr, C=3, design=True):
    ctx = P.ChainContext(pr["locs"], pr["NN"], pr["col"], pr["lm"], pr["y"], device=0, n_chains=C)
    if design:
        ctx.design_set(pr["X"], pr["first_obs"], pr["locs_cols"])
    return ctx


def _primitives_on(ctx, pr, inp, masks):
    """Every primitive for the chain masks `masks` (together they cover all
    chains) on the context `ctx`, which holds the design -> per-chain results."""
    C = len(inp["fields"])
    ql = len(pr["locs_cols"])
    out = {k: [None] * C for k in ("mean", "t", "gram", "refreshed", "field", "mu", "linv")}
    for k in range(C):
        ctx.select(k).factor(0, COV, CPS[k])
        ctx.set_field(inp["fields"][k])
        out["linv"][k] = ctx.get_linv(0)
    for mask in masks:
        ks = [k for k in range(C) if (mask >> k) & 1]
        mean = ctx.design_mean_stats_chains(mask, inp["b0"])
        if ql:
            t, gram, refreshed = ctx.design_interweave_stats_chains(mask, inp["shift"], inp["bl_old"])
        ctx.design_commit_chains(mask, inp["shift"], inp["bl_old"], inp["bl_new"], inp["b0_new"], inp["beta"])
        for k in ks:
            out["mean"][k] = mean[k].copy()
            if ql:
                out["t"][k], out["gram"][k], out["refreshed"][k] = t[k].copy(), gram[k].copy(), int(refreshed[k])
            out["field"][k] = ctx.select(k).get_field()
            out["mu"][k] = ctx.get_mu()
    return out


def _primitives(P, pr, inp, masks):
    """_primitives_on a fresh context"""
    with _open(P, pr, len(inp["fields"])) as ctx:
        return _primitives_on(ctx, pr, inp, masks)


def _reference(O, pr, inp, linv, k):
    """Chain k in long double, with the sums of absolute values the bounds use;
    B stays sparse (highprec.sparse_B_times), so n is not limited by an n x n matrix."""
    lm0 = pr["lm"] - 1
    X, y, f = pr["X"].astype(LD), pr["y"].astype(LD), inp["fields"][k].astype(LD)
    X1 = np.column_stack([np.ones(len(y), LD), X])
    resid = y - f[lm0] + LD(inp["b0"][k])
    ref = {"mean": resid @ X1, "mean_abs": (np.abs(y) + np.abs(f[lm0]) + abs(inp["b0"][k])) @ np.abs(X1)}
    Xl = X[pr["first_obs"] - 1][:, pr["locs_cols"]]
    Xl1 = np.column_stack([np.ones(pr["n"], LD), Xl])
    bo, bn, sh = inp["bl_old"][k].astype(LD), inp["bl_new"][k].astype(LD), LD(inp["shift"][k])
    other = f + sh + Xl @ bo
    other_abs = np.abs(f) + abs(sh) + np.abs(Xl) @ np.abs(bo)
    SX, SX_abs = H.sparse_B_times(linv, pr["NN"], Xl1)
    Bo, Bo_abs = H.sparse_B_times(linv, pr["NN"], other, other_abs)
    ref.update({"t": Bo @ SX, "t_abs": Bo_abs @ SX_abs,
                "gram": SX.T @ SX, "gram_abs": SX_abs.T @ SX_abs,
                "field": other - Xl @ bn, "field_abs": other_abs + np.abs(Xl) @ np.abs(bn),
                "mu": LD(inp["b0_new"][k]) + X @ inp["beta"][k].astype(LD),
                "mu_abs": abs(inp["b0_new"][k]) + np.abs(X) @ np.abs(inp["beta"][k].astype(LD))})
    return ref


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got).astype(LD) - ref)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: max error / bound = {worst:.3g}")
    assert np.all(err <= bound), (what, worst)


def _check_against_numpy(O, pr, inp, out):
    n, b, n_obs, p = pr["n"], pr["m"] + 1, len(pr["y"]), pr["X"].shape[1]
    ql = len(pr["locs_cols"])
    q = ql + 1
    for k in range(len(inp["fields"])):
        ref = _reference(O, pr, inp, out["linv"][k], k)
        # residual: 2 operations, the product, n_obs - 1 additions
        _within(out["mean"][k], ref["mean"], (n_obs + 2) * U * ref["mean_abs"], f"mean stats chain {k}")
        if ql:
            # a term of t is (B other)_i (B Xl1)_ij: other takes 2 ql + 1 operations, each SpMV row
            # b products and b - 1 additions (2b - 1), then the product and n - 1 additions;
            # a term of the Gram matrix has two SpMV rows as factors
            _within(out["t"][k], ref["t"], (n + 4 * b + 2 * ql) * U * ref["t_abs"], f"t chain {k}")
            _within(out["gram"][k], ref["gram"], (n + 4 * b) * U * ref["gram_abs"], f"gram chain {k}")
            assert out["refreshed"][k] == 1
            assert np.array_equal(out["gram"][k], out["gram"][k].T)
        _within(out["field"][k], ref["field"], (ql + 3) * EPS * ref["field_abs"], f"field chain {k}")
        _within(out["mu"][k], ref["mu"], (p + 1) * EPS * ref["mu_abs"], f"mu chain {k}")


def _assert_same(a, b):
    for key in a:
        for x, y in zip(a[key], b[key]):
            np.testing.assert_array_equal(x, y, err_msg=key)


@pytest.mark.usefixtures("engine")
def test_primitives_match_numpy_and_are_bitwise_reproducible(P, O, prob):
    """p = 70, locs_cols = [3, 1, 70], 550 observations, 3 chains: mean
    statistics, t, Gram matrix, committed field and mu within their bounds;
    one chain at a time == batched, bitwise; a second run == the first."""
    inp = _chain_inputs(prob)
    batched = _primitives(P, prob, inp, [0b111])
    _check_against_numpy(O, prob, inp, batched)
    _assert_same(batched, _primitives(P, prob, inp, [0b001, 0b010, 0b100]))
    _assert_same(batched, _primitives(P, prob, inp, [0b111]))


def test_shift_only_commit_and_all_columns_interweaved(P, O):
    """p = 1 with p_locs = 0: the commit applies the shift alone and the
    interweave statistics report NNGP_ERR_STATE; p_locs = p = 2."""
    from nngp_amd._lib import NNGP_ERR_STATE

    pr = _synthetic(P, 1, [])
    inp = _chain_inputs(pr)
    out = _primitives(P, pr, inp, [0b111])
    _check_against_numpy(O, pr, inp, out)
    for k in range(3):
        np.testing.assert_array_equal(out["field"][k], inp["fields"][k] + inp["shift"][k])
    with _open(P, pr) as ctx:
        ctx.factor(0, COV, CPS[0])
        ctx.set_field(inp["fields"][0])
        with pytest.raises(P.NNGPError) as e:
            ctx.design_interweave_stats_chains(1, np.zeros(3), np.zeros((3, 0)))
        assert e.value.status == NNGP_ERR_STATE
        assert ctx.design_mean_stats_chains(1, inp["b0"]).shape == (3, 2)
    pr = _synthetic(P, 2, [1, 0])
    inp = _chain_inputs(pr)
    _check_against_numpy(O, pr, inp, _primitives(P, pr, inp, [0b111]))


def test_state_after_commit_equals_set_field_and_set_mu(P, prob, engine):
    """Context A commits; context B gets set_field(A's field) and set_mu(A's
    mu, beta_0): the same sweep_chains call then gives bitwise equal fields --
    after a sweep call that left warm tile state in both."""
    inp = _chain_inputs(prob)
    C = 3
    ls, lnv = [0.1, -0.2, 0.0], [-0.5, -0.3, -0.7]
    fields = []
    ctxs = [_open(P, prob, C, design=(j == 0)) for j in range(2)]
    try:
        for ctx in ctxs:
            for k in range(C):
                ctx.select(k).factor(0, COV, CPS[k])
                ctx.set_field(inp["fields"][k])
                ctx.set_mu(None, inp["b0"][k])
            ctx.sweep_chains(2, inp["b0"], ls, lnv, [11, 12, 13], [0, 0, 0])  # warm tile state before the commit
        A, B = ctxs
        A.design_commit_chains(0b111, inp["shift"], inp["bl_old"], inp["bl_new"], inp["b0_new"], inp["beta"])
        for k in range(C):
            B.select(k).set_field(A.select(k).get_field())
            B.set_mu(A.get_mu(), inp["b0_new"][k])
        for ctx in ctxs:
            ctx.sweep_chains(2, inp["b0_new"], ls, lnv, [11, 12, 13], [2, 2, 2])
            fields.append([ctx.select(k).get_field() for k in range(C)])
    finally:
        for ctx in ctxs:
            ctx.close()
    for k in range(C):
        assert not np.array_equal(fields[0][k], inp["fields"][k])
        np.testing.assert_array_equal(fields[0][k], fields[1][k], err_msg=f"{engine} chain {k}")


def test_refreshed_follows_the_factor_generation(P, O, prob):
    inp = _chain_inputs(prob)
    n, b = prob["n"], prob["m"] + 1
    with _open(P, prob, 1) as ctx:
        ctx.factor(0, COV, CPS[0])
        ctx.set_field(inp["fields"][0])
        args = (1, inp["shift"][:1], inp["bl_old"][:1])
        _, g1, r1 = ctx.design_interweave_stats_chains(*args)
        _, g2, r2 = ctx.design_interweave_stats_chains(*args)
        assert (int(r1[0]), int(r2[0])) == (1, 0)
        np.testing.assert_array_equal(g1, g2)
        ctx.factor(1, COV, CPS[1])
        ctx.accept_factor()
        _, g3, r3 = ctx.design_interweave_stats_chains(*args)
        assert int(r3[0]) == 1
        ref = _reference(O, prob, {**inp, "fields": inp["fields"][:1]}, ctx.get_linv(0), 0)
        _within(g3[0], ref["gram"], (n + 4 * b) * U * ref["gram_abs"], "gram after accept_factor")
        assert not np.array_equal(g3, g1)


# ---------------------------------------------------------------- full iterations
def _compare(res, ref):
    """The tolerances of tests/test_gpu_mcmc.py::_compare: identical acceptance
    vectors, rtol 1e-7 on the scalar records, 1e-6 on beta and the field."""
    rec = res["records"]
    for key in ("beta_0", "log_scale", "log_noise_variance"):
        np.testing.assert_allclose(rec[key][:, 0], ref["records"][key], rtol=1e-7, atol=1e-9, err_msg=key)
    np.testing.assert_allclose(rec["shape"], np.array(ref["records"]["shape"]), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(rec["beta"], np.array(ref["records"]["beta"]), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(res["state"]["params"]["field"], ref["params"]["field"], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(res["acceptance"]["covariance_acceptance_ancillary"], ref["acceptance"]["ancillary"])
    np.testing.assert_array_equal(res["acceptance"]["covariance_acceptance_sufficient"], ref["acceptance"]["sufficient"])


@pytest.mark.usefixtures("engine")
def test_iterations_match_oracle_vignette_X_locs(P, O, toy):
    """The vignette toy as test_update_iterations_match_oracle_vignette_X_locs, regression="device"."""
    import mcmc_oracle as MO
    from nngp_amd.update_gaussian import _philox_key, _run_chain

    L = P.mcmc_nngp_initialize(toy["locs"], toy["observed_field"], X_locs=toy["X"],
                               stationary_covfun=COV, m=5, n_chains=1, seed=1)
    st, va = L["states"]["chain_1"], L["vecchia_approx"]
    iters, nc = 30, 5
    try:
        res = _run_chain(0, st, L["_contexts"][0], L["X"], L["observed_field"], L["space_time_model"], va,
                         iters, 1.0, True, nc, 0, 1, regression="device")
    finally:
        for c in L["_contexts"]:
            c.close()
    ref = MO.run_chain(0, st, L["locs"], va["NNarray"], va["coloring"], L["X"], L["observed_field"],
                       L["space_time_model"], va, iters, 1.0, nc, 0, _philox_key(0, 1, 1))
    _compare(res, ref)


def _synthetic_run(P, pr, iters=10, nc=3, n_chains=1):
    """Chain i of n_chains against the oracle's chain i.  One chain runs alone
    (_run_chain); several run in lockstep on one context, so the regression
    calls are batched over the chains."""
    import mcmc_oracle as MO
    from nngp_amd.update_gaussian import _philox_key, _run_chain, mcmc_nngp_update_Gaussian

    n, p = pr["n"], pr["X"].shape[1]
    X1 = np.column_stack([np.ones(len(pr["y"])), pr["X"]])
    X = {"X": pr["X"], "locs": np.array(pr["locs_cols"], np.int64), "solve_1XT1X": np.linalg.inv(X1.T @ X1)}
    X["chol_solve_1XT1X"] = np.linalg.cholesky(X["solve_1XT1X"]).T  # initialize.py:142-143
    va = {"n_locs": n, "n_obs": len(pr["lm"]), "locs_match": pr["lm"], "NNarray": pr["NN"], "coloring": pr["col"],
          "obs_per_loc": np.bincount(pr["lm"] - 1, minlength=n).astype(np.int32), "hctam_scol_1": pr["first_obs"]}
    stm = {"covfun": {"stationary_covfun": COV, "shape_params": ["log_range"]}}
    rng = np.random.default_rng(0)
    states = [{"params": {"beta_0": 2.0, "beta": np.zeros(p), "log_scale": 0.0, "shape": np.array([np.log(0.1)]),
                          "log_noise_variance": np.log(0.5), "field": 2.0 + rng.normal(size=n)},
               "transition_kernels": {"covariance_params_sufficient": {"logvar": -2.0},
                                      "covariance_params_ancillary": {"logvar": -2.0},
                                      "log_noise_variance": {"logvar": -1.0}}} for _ in range(n_chains)]
    with P.ChainContext(pr["locs"], pr["NN"], pr["col"], pr["lm"], pr["y"], device=0, n_chains=n_chains) as ctx:
        if n_chains == 1:
            res = [_run_chain(0, copy.deepcopy(states[0]), ctx, X, pr["y"], stm, va, iters, 1.0, True, nc, 0, 1,
                              regression="device")]
        else:
            out = mcmc_nngp_update_Gaussian(pr["locs"], X, pr["y"], stm, va, copy.deepcopy(states), iters,
                                            field_thinning=1.0, n_chromatic=nc, seed=1, regression="device",
                                            contexts=[ctx.view(i) for i in range(n_chains)])
            res = list(out.values())
    for i, state in enumerate(states):
        ref = MO.run_chain(i, state, pr["locs"], pr["NN"], pr["col"], X, pr["y"], stm, va, iters, 1.0, nc, 0,
                           _philox_key(0, i + 1, 1))
        _compare(res[i], ref)


def test_iterations_match_oracle_synthetic_design(P, O, prob):
    """p = 70 with three interweaved columns, 10 iterations."""
    _synthetic_run(P, prob)


def test_iterations_match_oracle_row_group_32(P, O):
    """m = 16 (b = 17: the 32-lane row group), n = 600, p = 3 with one
    interweaved column, two chains in lockstep on one context, 10 iterations."""
    _synthetic_run(P, _synthetic(P, 3, [1], n=600, m=16, seed=7), n_chains=2)


def test_iterations_match_oracle_X_obs_only(P, O):
    """p_locs = 0: the beta_0 Gibbs draw and the regression draw both run."""
    _synthetic_run(P, _synthetic(P, 3, [], seed=5))


@pytest.mark.usefixtures("engine")
def test_lockstep_batched_chains_equal_sequential_chains(P, toy):
    """3 chains of one context, regression="device", batched in lockstep ==
    the chains one after another (_run_chain), bitwise."""
    from nngp_amd.context import make_chain_views
    from nngp_amd.update_gaussian import _run_chain, mcmc_nngp_update_Gaussian

    L = P.mcmc_nngp_initialize(toy["locs"], toy["observed_field"], X_locs=toy["X"],
                               stationary_covfun=COV, m=5, n_chains=3, seed=2)
    va = L["vecchia_approx"]
    assert len({id(v.ctx) for v in L["_contexts"]}) == 1
    states0 = copy.deepcopy(L["states"])
    views = make_chain_views(L["locs"], va["NNarray"], va["coloring"], va["locs_match"], L["observed_field"], 3)
    try:
        out = mcmc_nngp_update_Gaussian(L["locs"], L["X"], L["observed_field"], L["space_time_model"], va,
                                        L["states"], 20, field_thinning=0.1, n_chromatic=3,
                                        contexts=L["_contexts"], seed=1, regression="device")
        y = np.asarray(L["observed_field"], np.float64)
        for i, (nm, st) in enumerate(states0.items()):
            ref = _run_chain(i, st, views[i], L["X"], y, L["space_time_model"], va, 20, 0.1, True, 3, 0, 1,
                             regression="device")
            for key in ("beta_0", "log_scale", "log_noise_variance", "shape", "beta", "field"):
                np.testing.assert_array_equal(out[nm]["records"][key], ref["records"][key], err_msg=f"{nm} {key}")
    finally:
        views[0].ctx.close()
        L["_contexts"][0].close()


def test_heavy_metals_matches_oracle(P, O, heavy):
    """p = 156, p_locs = 14, m = 5, 3 iterations, compared as
    test_heavy_metals_device_path_matches_oracle compares (its tolerances)."""
    import mcmc_oracle as MO
    from nngp_amd.model import covparms
    from nngp_amd.update_gaussian import _philox_key, _run_chain

    L = P.mcmc_nngp_initialize(heavy["observed_locs"], heavy["observed_field"], X_locs=heavy["X_locs"],
                               stationary_covfun="exponential_sphere", m=5, n_chains=1, seed=1)
    va, st, ctx = L["vecchia_approx"], L["states"]["chain_1"], L["_contexts"][0]
    assert L["X"]["X"].shape[1] == 156 and len(L["X"]["locs"]) == 14
    try:
        cp = covparms(L["space_time_model"]["covfun"]["shape_params"], st["params"]["shape"])
        ctx.factor(0, "exponential_sphere", cp)
        Ld = ctx.get_linv(0)
        Lo = O.vecchia_linv("exponential_sphere", cp, L["locs"], va["NNarray"])
        err, scale, kmax = np.abs(Ld - Lo).max(1), np.abs(Lo).max(1), 1.0
        for i in np.nonzero(err > 1e-10 * scale)[0]:
            NN = va["NNarray"]
            idx = NN[i][NN[i] != O.NA] - 1
            kmax = max(kmax, np.linalg.cond(O.covmat("exponential_sphere", cp, L["locs"][idx])))
        iters, nc = 3, 3
        res = _run_chain(0, st, ctx, L["X"], L["observed_field"], L["space_time_model"], va, iters, 1.0, True, nc, 0, 1,
                         regression="device")
    finally:
        ctx.close()
    ref = MO.run_chain(0, st, L["locs"], va["NNarray"], va["coloring"], L["X"], L["observed_field"],
                       L["space_time_model"], va, iters, 1.0, nc, 0, _philox_key(0, 1, 1))
    np.testing.assert_array_equal(res["acceptance"]["covariance_acceptance_sufficient"], ref["acceptance"]["sufficient"])
    np.testing.assert_array_equal(res["acceptance"]["covariance_acceptance_ancillary"], ref["acceptance"]["ancillary"])
    np.testing.assert_allclose(res["records"]["log_scale"][:, 0], ref["records"]["log_scale"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(res["records"]["beta_0"][:, 0], ref["records"]["beta_0"], rtol=1e-5, atol=1e-7)
    ftol = min(1e-4, max(1e-8, 100 * 1e-14 * kmax))  # the conditioning-derived tolerance of that test
    fd, fr = res["state"]["params"]["field"], ref["params"]["field"]
    rel = np.abs(fd - fr).max() / np.abs(fr).max()
    print(f"heavy metals, regression on the device: cond max {kmax:.3g}, field max rel diff {rel:.3g}, tol {ftol:.3g}")
    assert rel <= ftol, (rel, ftol, kmax)
    assert np.all(np.isfinite(res["records"]["beta"]))


# ---------------------------------------------------------------- argument checks
def test_argument_and_state_errors_leave_the_context_usable(P, prob):
    from nngp_amd._lib import NNGP_ERR_ARG, NNGP_ERR_STATE, colmajor, i32, lib

    n, n_obs = prob["n"], len(prob["y"])
    Xc = colmajor(prob["X"], np.float64)
    fo = i32(prob["first_obs"])

    def raw(ctx, p, first_obs, cols):
        c = i32(cols)
        return lib.nngp_design_set(ctx._h, Xc.ctypes.data, p, first_obs.ctypes.data, c.ctypes.data if len(c) else None,
                                   len(c))

    inp = _chain_inputs(prob)
    with _open(P, prob, 3, design=False) as ctx:
        bad0, badn = fo.copy(), fo.copy()
        bad0[7], badn[n - 1] = 0, n_obs + 1
        for p, f, cols in ((0, fo, []), (2, fo, [1, 2, 1]), (40, fo, list(range(1, 33))), (70, fo, [0]),
                           (70, fo, [71]), (70, fo, [3, 3]), (70, bad0, [1]), (70, badn, [1])):
            assert raw(ctx, p, f, cols) == NNGP_ERR_ARG, (p, cols)
        assert lib.nngp_design_set(ctx._h, Xc.ctypes.data, 70, fo.ctypes.data, None, -1) == NNGP_ERR_ARG
        # no design yet
        for call in (lambda: ctx.design_mean_stats_chains(1, inp["b0"]),
                     lambda: ctx.design_commit_chains(1, inp["shift"], None, None, inp["b0"], np.zeros((3, 0)))):
            with pytest.raises(P.NNGPError) as e:
                call()
            assert e.value.status == NNGP_ERR_STATE
        ctx.design_p_locs = 3
        with pytest.raises(P.NNGPError) as e:
            ctx.design_interweave_stats_chains(1, inp["shift"], inp["bl_old"])
        assert e.value.status == NNGP_ERR_STATE
        ctx.design_set(prob["X"], prob["first_obs"], prob["locs_cols"])
        for call in (lambda: ctx.design_mean_stats_chains(1, inp["b0"]),  # no field
                     lambda: ctx.design_interweave_stats_chains(1, inp["shift"], inp["bl_old"])):  # no factor, no field
            with pytest.raises(P.NNGPError) as e:
                call()
            assert e.value.status == NNGP_ERR_STATE
        ctx.set_field(inp["fields"][0])
        with pytest.raises(P.NNGPError) as e:
            ctx.design_interweave_stats_chains(1, inp["shift"], inp["bl_old"])  # no factor
        assert e.value.status == NNGP_ERR_STATE
        for mask in (0, 8):
            with pytest.raises(P.NNGPError) as e:
                ctx.design_mean_stats_chains(mask, inp["b0"])
            assert e.value.status == NNGP_ERR_ARG
        # the context is usable: valid calls succeed
        ctx.factor(0, COV, CPS[0])
        assert np.all(np.isfinite(ctx.design_mean_stats_chains(1, inp["b0"])[0]))
        t, gram, refreshed = ctx.design_interweave_stats_chains(1, inp["shift"], inp["bl_old"])
        assert refreshed[0] == 1 and np.all(np.isfinite(t[0])) and np.all(np.isfinite(gram[0]))
        ctx.design_commit_chains(1, inp["shift"], inp["bl_old"], inp["bl_new"], inp["b0_new"], inp["beta"])
        assert np.all(np.isfinite(ctx.get_mu()))
        ctx.design_set(None)  # frees the design
        with pytest.raises(P.NNGPError) as e:
            ctx.design_mean_stats_chains(1, inp["b0"])
        assert e.value.status == NNGP_ERR_STATE
    with P.ChainContext(prob["locs"], prob["NN"], prob["col"], prob["lm"], prob["y"], device=0, _shard=(2, 0)) as sh:
        with pytest.raises(P.NNGPError) as e:
            sh.design_set(prob["X"], prob["first_obs"], prob["locs_cols"])
        assert e.value.status == NNGP_ERR_STATE
        sh.factor(0, COV, CPS[0])  # still usable
