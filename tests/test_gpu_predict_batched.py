"""Batched posterior prediction (nngp_predict_field; engine="batched" of
mcmc_nngp_predict_field): the factor rows of the new locations only and a
level solve with the samples in the lanes, against the oracle's restatement
of Scripts/mcmc_nngp_predict.R with the same normals for the new locations.

Bound: the one the context-engine tests (test_gpu_predict.py) state for the
same comparison, 1e-9 max|ref| for the exponential covariance and 1e-8
max|ref| for Matern.  The recursion itself agrees with the oracle to 1e-15
on the CPU, so the budget is the device factor's, as for the context engine;
every comparison prints both engines' errors before it asserts.

Measured on an MI355X (2026-10-20), error / max|ref|, batched | context:
shape 1 3.7e-14 | 3.7e-14, shape 2 (Matern) 1.4e-11 | 1.4e-11, shape 3 m = 5
4.6e-15 | 4.6e-15, shape 3 m = 15 (Matern) 8.3e-12 | 8.3e-12, the line
6.5e-15 | 6.1e-15, n = 3 1.7e-16 | 3.5e-16, m = 20 / 24 1.1e-14 / 9.2e-15 (both
engines).  The context engine meets the stated bound at every shape, so the
bound is the stated one everywhere; the engines differ by 4e-16 max|ref|.
The Matern case of shape 3 spends about ten seconds in the CPU oracle (seven
factors of 1800 rows x 16 neighbours through its Bessel function)."""
import re

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

EXP, MAT = "exponential_isotropic", "matern_isotropic"
REL = {EXP: 1e-9, MAT: 1e-8}


def _chain(shapes, log_scales, beta0s, fields):
    k = len(shapes)
    return {"saved_field": np.arange(1, k + 1, dtype=np.float64),
            "params": {"shape": np.asarray(shapes, np.float64).reshape(k, -1),
                       "log_scale": np.asarray(log_scales, np.float64).reshape(k, 1),
                       "beta_0": np.asarray(beta0s, np.float64).reshape(k, 1),
                       "field": np.ascontiguousarray(fields, np.float64)}}


def _list(locs, covfun, chains):
    sp = ["log_range"] if covfun == EXP else ["log_range", "qlogis_smoothness"]
    return {"locs": locs, "records": {f"chain_{k + 1}": c for k, c in enumerate(chains)},
            "space_time_model": {"covfun": {"stationary_covfun": covfun, "shape_params": sp}}}


def _random_chain(rng, n, shapes):
    k = len(shapes)
    return _chain(shapes, rng.normal(size=k) * 0.2, 1.0 + rng.normal(size=k) * 0.1, 1.0 + rng.normal(size=(k, n)))


def _z(L, n_pred, seed=99):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(len(c["saved_field"]), n_pred)) for c in L["records"].values()]


def _errors(got, ref):
    return max(np.abs(g - r).max() / np.abs(r).max() for g, r in zip(got, ref))


def _both_engines(P, O, L, pred, m, label, context=True, **kw):
    """Errors of both engines against the oracle, relative to max|ref| per
    chain; asserts the batched engine's against the stated bound."""
    covfun = L["space_time_model"]["covfun"]["stationary_covfun"]
    z = _z(L, len(pred))
    ref = O.predict_field(L, pred, z, burn_in=0.0, m=m)
    got = P.mcmc_nngp_predict_field(L, pred, burn_in=0.0, m=m, z_new=z, device=0, engine="batched", **kw)
    eb = _errors(got["predicted_field_samples"], ref)
    ctx = None
    if context:
        ctx = P.mcmc_nngp_predict_field(L, pred, burn_in=0.0, m=m, z_new=z, device=0, engine="context")
        ec = _errors(ctx["predicted_field_samples"], ref)
        print(f"[predict {label}] batched err {eb:.3e}  context err {ec:.3e}  bound {REL[covfun]:.0e} (x max|ref|)")
    else:
        print(f"[predict {label}] batched err {eb:.3e}  bound {REL[covfun]:.0e} (x max|ref|)")
    for g, r in zip(got["predicted_field_samples"], ref):
        assert g.shape == r.shape
    assert eb <= REL[covfun], (label, eb)
    return got, ctx, ref


def _shapes(covfun, k, rng):
    """k distinct shape rows."""
    lr = np.log(0.05 + 0.1 * rng.uniform(size=k))
    return lr.reshape(k, 1) if covfun == EXP else np.column_stack([lr, rng.normal(size=k) * 0.7])


# ---- shapes 1 and 2: n = 3000, m = 8, 400 new locations, two chains [a, a, b, a]
@pytest.fixture(scope="module")
def shape1(P, O):
    n, m = 3000, 8
    locs, *_ = make_problem(P, n, m, seed=4)
    rng = np.random.default_rng(1)
    a, b = [np.log(0.1)], [np.log(0.05)]
    L = _list(locs, EXP, [_random_chain(rng, n, [a, a, b, a]) for _ in range(2)])
    pred = rng.uniform(size=(400, 2))
    return (L, pred, m) + _both_engines(P, O, L, pred, m, "shape 1")


def test_shape1_two_chains_reused_factor(shape1):
    """Shapes [a, a, b, a]: the fourth sample uses b's factor (the last one
    built, predict.R:23,32), which the oracle restates; both chains within
    1e-9 max|ref|."""
    L, pred, m, got, ctx, ref = shape1
    assert len(got["predicted_field_samples"]) == 2 and got["predicted_field_samples"][0].shape == (4, 400)


def test_shape2_matern_transform(P, O):
    """matern_isotropic with predict.R:37's 1.5 * plogis smoothness."""
    n, m = 3000, 8
    locs, *_ = make_problem(P, n, m, seed=4)
    rng = np.random.default_rng(2)
    s1, s2 = [np.log(0.1), 0.3], [np.log(0.08), -0.5]
    L = _list(locs, MAT, [_random_chain(rng, n, [s1, s1, s2, s1]) for _ in range(2)])
    _both_engines(P, O, L, rng.uniform(size=(400, 2)), m, "shape 2")


# ---- shape 3: n = 300, 1500 uniform new locations (new rows depend on new rows)
def _shape3(P, m, covfun, k, seed):
    locs, *_ = make_problem(P, 300, m, seed=seed)
    rng = np.random.default_rng(seed + 1)
    sh = _shapes(covfun, 7, rng)
    L = _list(locs, covfun, [_random_chain(rng, 300, [sh[i % 7] for i in range(k)])])
    return L, rng.uniform(size=(1500, 2))


@pytest.fixture(scope="module")
def shape3(P, O):
    """m = 5, exponential, 130 samples cycling through 7 shapes (after the
    first 7 every sample reuses the seventh factor: the reference's rule)."""
    L, pred = _shape3(P, 5, EXP, 130, 30)
    z = _z(L, 1500)
    return L, pred, z, O.predict_field(L, pred, z, burn_in=0.0, m=5)[0]


def _prefix(L, k):
    c = L["records"]["chain_1"]
    q = {"saved_field": c["saved_field"][:k], "params": {key: v[:k] for key, v in c["params"].items()}}
    return _list(L["locs"], L["space_time_model"]["covfun"]["stationary_covfun"], [q])


@pytest.mark.parametrize("m,covfun", [(5, EXP), (15, MAT)])
def test_shape3_dense_new_points_seven_factors(P, O, m, covfun):
    """Depth about 19 (m = 5) and 50 (m = 15) among the new rows; seven
    distinct shapes in one chain: more than one FactorJobs launch."""
    L, pred = _shape3(P, m, covfun, 8, 40 + m)
    _both_engines(P, O, L, pred, m, f"shape 3 m={m}")


@pytest.mark.parametrize("k", [1, 65, 130])
def test_shape3_sample_counts(P, shape3, k):
    """1, 65 and 130 samples (a lane tail, two waves of samples, and three
    batches at sample_batch = 64) against the oracle's rows."""
    L, pred, z, ref = shape3
    got = P.mcmc_nngp_predict_field(_prefix(L, k), pred, burn_in=0.0, m=5, z_new=[z[0][:k]], device=0,
                                    engine="batched", sample_batch=64,
                                    summary_backend="hip")["predicted_field_samples"][0]
    e = _errors([got], [ref[:k]])
    print(f"[predict shape 3, {k} samples] batched err {e:.3e}")
    assert got.shape == (k, 1500) and e <= REL[EXP]


def _direct_args(P, L, pred, m, z):
    """The arguments of one nngp_predict_field call for chain_1 of L."""
    from nngp_amd.model import covparms

    c = L["records"]["chain_1"]
    allloc = np.vstack([L["locs"], pred])
    NN = P.find_ordered_nn(allloc, m)
    sh = c["params"]["shape"]
    uniq, inv = np.unique(sh, axis=0, return_inverse=True)
    sp = L["space_time_model"]["covfun"]["shape_params"]
    rows = np.array([covparms(sp, u, 0.0, 1.5) for u in uniq])
    k = len(sh)
    return dict(locs=allloc, NN=NN, n=len(L["locs"]), covfun=L["space_time_model"]["covfun"]["stationary_covfun"],
                covparms_rows=rows, factor_of=np.asarray(inv).ravel().astype(np.int32), fields=c["params"]["field"],
                field_row=np.arange(k), beta0=c["params"]["beta_0"][:, 0].copy(),
                log_scale=c["params"]["log_scale"][:, 0].copy(), z=z)


def _subset(a, idx):
    b = dict(a)
    for key in ("factor_of", "field_row", "beta0", "log_scale", "z"):
        b[key] = np.ascontiguousarray(a[key][idx])
    return b


def test_sample_independence_bitwise(P, shape3):
    """A sample's output bytes depend on its own inputs only: the batch size
    (1, 7, 64, automatic), a permutation of the samples, and unrelated
    samples appended after it change nothing."""
    from nngp_amd import predict as PR

    L, pred, z, _ = shape3
    a = _direct_args(P, L, pred, 5, z[0])
    base = PR.predict_field_call(**a, device=0)
    assert np.isfinite(base).all()
    for sb in (1, 7, 64):
        assert np.array_equal(PR.predict_field_call(**a, sample_batch=sb, device=0), base), sb
    perm = np.random.default_rng(0).permutation(len(base))
    assert np.array_equal(PR.predict_field_call(**_subset(a, perm), device=0), base[perm])
    assert np.array_equal(PR.predict_field_call(**_subset(a, np.arange(40)), sample_batch=7, device=0), base[:40])


def test_philox_equals_injected_device_normals(P, shape3):
    """z == NULL with (seed, counter) == the run with z[s] =
    nngp_device_normals(device, seed, counter[s], n_pred), bitwise."""
    from nngp_amd import predict as PR

    L, pred, z, _ = shape3
    a = _subset(_direct_args(P, L, pred, 5, z[0]), np.arange(70))
    seed = 0xC0FFEE1234567
    counter = (np.arange(70, dtype=np.uint64) * np.uint64(7919) + np.uint64(2 ** 33 + 5))
    zi = np.stack([P.context.device_normals(seed, int(c), 1500, device=0) for c in counter])
    inj = PR.predict_field_call(**{**a, "z": zi}, device=0)
    phi = PR.predict_field_call(**{**a, "z": None}, seed=seed, counter=counter, sample_batch=64, device=0)
    assert np.array_equal(inj, phi)
    L70 = _prefix(L, 70)
    s1 = P.mcmc_nngp_predict_field(L70, pred, burn_in=0.0, m=5, device=0, engine="batched", rng="philox", seed=5)
    s2 = P.mcmc_nngp_predict_field(L70, pred, burn_in=0.0, m=5, device=0, engine="batched", rng="philox", seed=6)
    x1, x2 = s1["predicted_field_samples"][0], s2["predicted_field_samples"][0]
    assert np.isfinite(x1).all() and not np.array_equal(x1, x2)
    zc = np.stack([P.context.device_normals((5 + PR.PHILOX_CHAIN_MIX) % 2 ** 64, k, 1500, device=0) for k in range(70)])
    s3 = P.mcmc_nngp_predict_field(L70, pred, burn_in=0.0, m=5, device=0, engine="batched", z_new=[zc])
    assert np.array_equal(s3["predicted_field_samples"][0], x1)


def test_shape4_line_of_new_points(P, O):
    """600 new points on a line over 500 observed ones (m = 5): every new row
    names the one before it, depth = n_pred, one row per level -- the
    in-workgroup multi-level path."""
    locs, *_ = make_problem(P, 500, 5, seed=8)
    rng = np.random.default_rng(9)
    pred = np.column_stack([np.linspace(0.1, 0.9, 600), np.full(600, 0.5)])
    L = _list(locs, EXP, [_random_chain(rng, 500, _shapes(EXP, 3, rng))])
    _both_engines(P, O, L, pred, 5, "shape 4 line")


@pytest.mark.parametrize("n_pred", [10, 1])
def test_shape5_na_padding_and_single_location(P, O, n_pred):
    """n = 3, m = 5: the first new rows have fewer than m neighbours (NA)."""
    locs, *_ = make_problem(P, 3, 5, seed=3)
    rng = np.random.default_rng(10)
    L = _list(locs, EXP, [_random_chain(rng, 3, _shapes(EXP, 2, rng))])
    _both_engines(P, O, L, rng.uniform(size=(n_pred, 2)), 5, f"shape 5 n_pred={n_pred}")


@pytest.mark.parametrize("m", [20, 24])
def test_shape6_wide_neighbourhoods(P, O, m):
    """b = 21 (the widest register-resident factor kernel) and b = 25 (the
    run-time-b factor kernel) at n = 400, 200 new locations."""
    locs, *_ = make_problem(P, 400, m, seed=11)
    rng = np.random.default_rng(12)
    L = _list(locs, EXP, [_random_chain(rng, 400, _shapes(EXP, 2, rng))])
    _both_engines(P, O, L, rng.uniform(size=(200, 2)), m, f"shape 6 m={m}")


def test_engines_agree_and_device_summary(P, O, shape1):
    """Batched and context engine within twice the bound at shapes 1 and 3;
    summary_backend="hip" summarises exactly those samples."""
    L, pred, m, got, ctx, ref = shape1
    e1 = _errors(got["predicted_field_samples"], ctx["predicted_field_samples"])
    L3, pred3 = _shape3(P, 5, EXP, 8, 45)
    g3, c3, _ = _both_engines(P, O, L3, pred3, 5, "shape 3 (engines)", summary_backend="hip")
    e3 = _errors(g3["predicted_field_samples"], c3["predicted_field_samples"])
    print(f"[predict engines] batched vs context: shape 1 {e1:.3e}  shape 3 {e3:.3e}")
    assert e1 <= 2 * REL[EXP] and e3 <= 2 * REL[EXP]
    host = P.get_summary(np.vstack(g3["predicted_field_samples"]))
    np.testing.assert_allclose(g3["predicted_field_summary"], host, rtol=1e-12,
                               atol=1e-12 * np.abs(host).max())


# make_problem seed of the failing problem below.  Seeds 0..5 were tried once on
# the device (2026-10-20): ChainContext.factor on the stacked problem reports
# NNGP_ERR_CHOL for seeds 0 (row 408) and 3 (row 410); for 1, 2, 4 and 5 the
# rounding leaves the coinciding row's pivot barely positive and the factor passes.
CHOL_SEED = 0


def test_non_positive_definite_row_is_reported(P, O):
    """A new location coinciding with its nearest observed neighbour, no
    nugget (the construction of test_gpu_mcmc.py's failing chain): the
    context engine's factor on the stacked problem and the batched engine
    report NNGP_ERR_CHOL for the same 1-based stacked row; a following valid
    call on the same device is exact."""
    from nngp_amd import predict as PR
    from nngp_amd._lib import NNGP_ERR_CHOL, NNGPError

    n, m = 400, 8
    locs, *_ = make_problem(P, n, m, seed=CHOL_SEED)
    rng = np.random.default_rng(13)
    pred = rng.uniform(size=(50, 2))
    pred[7] = locs[np.argmin(((locs - pred[7]) ** 2).sum(1))]
    allloc = np.vstack([locs, pred])
    NN = P.find_ordered_nn(allloc, m)
    cp = [1.0, 0.1, 0.0]
    N = len(allloc)
    with P.ChainContext(allloc, NN, P.naive_greedy_coloring(NN), np.arange(1, N + 1, dtype=np.int32), np.zeros(N),
                        device=0) as ctx:
        with pytest.raises(NNGPError) as e0:
            ctx.factor(0, EXP, cp)
    assert e0.value.status == NNGP_ERR_CHOL
    row = int(re.search(r"row (\d+)", str(e0.value)).group(1))
    assert row == n + 8
    L = _list(locs, EXP, [_random_chain(rng, n, [[np.log(0.1)]] * 3)])
    z = _z(L, 50)
    with pytest.raises(NNGPError) as e1:
        P.mcmc_nngp_predict_field(L, pred, burn_in=0.0, m=m, z_new=z, device=0, engine="batched")
    assert e1.value.status == NNGP_ERR_CHOL and e1.value.fail_row == row
    pred[7] = [0.123, 0.456]
    _both_engines(P, O, L, pred, m, "after a failed call", context=False)
