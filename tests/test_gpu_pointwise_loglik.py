"""nngp_pointwise_loglik on the device (pointwise_loglik(backend="hip"),
mcmc_nngp_criteria, mcmc_nngp_score_response) against the 50-digit reference
of tests/pointwise_ref.py, and the bitwise properties include/nngp.h states.

Bound.  The derivation is the docstring of tests/pointwise_ref.py, operation
by operation: (q + 1) eps sum |terms| for the mean, carried through r and ll,
the sequential sums over S, and the ulp errors of the device's exp, log and
erfc.  Those ulp figures are measured once (fixture ``ulp``) on the S = 1
cases, where pit is one erfc value and lppd / log_cpo are one exp and one log:
the device's pit against 0.5 erfc of the device's own argument (rebuilt from
its fit_mean, which is the mean itself for S = 1, with the host's constants),
and lppd, log_cpo against its ll_mean.  For S = 1 the exp and log arguments
are 0 and 1, where both functions are exact, so that measurement cannot speak
for other arguments: each figure is floored at 1 ulp (no library promises
better than faithful rounding), and the bound uses twice the figure, because
the arguments of larger cases differ.

Measured on an MI355X (2026-10-21): erfc worst 2.59 ulp, exp / log 0 ulp at
their S = 1 arguments, so the bound grants 5.19 ulp to erfc and 2 ulp to exp
and log; worst max err / bound 0.52 (S = 1, n = 65, q = 1), 0.34 chunked at
n = 259, 0.21 for the extreme spread, 0.21 for the toy fit's held-out scores.
Every case prints its max err / bound."""
import ctypes as C
import math

import numpy as np
import pytest

import pointwise_ref as R

pytestmark = pytest.mark.gpu

TILE = 16  # kCriteriaRows of csrc/criteria.hip: samples per register tile


def _hip(P, pr, **kw):
    return P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"],
                              backend="hip", device=0, **kw)


def _ref(pr, ulp):
    return R.reference(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], pr["coef"], pr["X"], **ulp)


@pytest.fixture(scope="module")
def ulp(P):
    """The measured ulp errors of the device's erfc and of its exp / log, from
    S = 1 cases; -> the figures the bound grants (twice the measured ones,
    each floored at 1 ulp first)."""
    mp = R._MP
    worst = {"erfc": 0.0, "exp_log": 0.0}
    for n, q, seed in ((259, 2, 31), (65, 0, 32), (63, 17, 33)):
        pr = R.problem(1, n, q, seed)
        got = _hip(P, pr)
        g = math.sqrt(2.0 * (0.5 * math.exp(-float(pr["lnv"][0]))))
        for i in range(pr["y"].size):
            t = ((float(pr["y"][i]) - got[i, 0]) * g) * 0.70710678118654752440
            worst["erfc"] = max(worst["erfc"], R.ulps(got[i, 5], mp.erfc(-mp.mpf(t)) / 2))
            worst["exp_log"] = max(worst["exp_log"], R.ulps(got[i, 3], mp.mpf(float(got[i, 1]))),
                                   R.ulps(got[i, 4], mp.mpf(float(got[i, 1]))))
    print(f"[pointwise ulp] device erfc: worst {worst['erfc']:.3f} ulp over the S = 1 cases; "
          f"exp/log at their S = 1 arguments: worst {worst['exp_log']:.3f} ulp")
    e, c = 2.0 * max(worst["exp_log"], 1.0), 2.0 * max(worst["erfc"], 1.0)
    return {"u_exp": e, "u_log": e, "u_erfc": c}


# S: 1, 2, one more than the sample tile, 65; n: 1, 63, 65, 259; q: 0, 1, 2, 17
ACCURACY = [(1, 65, 1, 41), (2, 1, 1, 42), (2, 63, 0, 43), (TILE + 1, 63, 17, 44), (65, 65, 0, 45), (65, 1, 2, 46),
            (TILE + 1, 259, 2, 47), (TILE, 65, 1, 48)]


@pytest.mark.parametrize("S,n,q,seed", ACCURACY)
def test_against_high_precision(P, ulp, S, n, q, seed):
    pr = R.problem(S, n, q, seed)
    got = _hip(P, pr)
    ref, bound, _ = _ref(pr, ulp)
    ratio = R.worst_ratio(got, ref, bound)
    print(f"[pointwise hip S={S} n={n} q={q}] n_obs {pr['y'].size}  max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    np.testing.assert_array_equal(_hip(P, pr), got)  # two runs agree


@pytest.fixture(scope="module")
def chunked(P):
    """n = 259, observations per location from {0, 1, 3}, no observation at the
    first and last location of a chunk for chunk_cols 64 and 100; one call per
    chunk_cols, shared."""
    pr = R.problem(TILE + 3, 259, 2, 51, empty=(0, 63, 64, 99, 100, 127, 128, 199, 200, 258))
    counts = np.bincount(pr["obs_loc"], minlength=260)[1:]
    assert set(counts) == {0, 1, 3} and counts[62] + counts[65] > 0
    return pr, {w: _hip(P, pr, chunk_cols=w) for w in (0, 64, 100)}


def test_chunking_leaves_the_bits_alone(P, ulp, chunked):
    from nngp_amd import estimate

    pr, got = chunked
    np.testing.assert_array_equal(got[64], got[0])
    np.testing.assert_array_equal(got[100], got[0])
    ref, bound, _ = _ref(pr, ulp)
    ratio = R.worst_ratio(got[0], ref, bound)
    print(f"[pointwise hip chunked n=259 q=2] n_obs {pr['y'].size}  max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    _hip(P, pr, chunk_cols=100)
    st = estimate.pointwise_loglik_stats()
    assert st["chunk_cols"] == 100 and st["staged_bytes"] == 8 * (TILE + 3) * 259 and st["kernel_ms"] > 0


def test_embedded_in_a_larger_problem(P, chunked):
    """The same observations at other positions, among other locations and
    observations, with another n and n_obs: the same bits."""
    pr, got = chunked
    rng = np.random.default_rng(52)
    S, n, off = pr["field"].shape[0], 259, 70
    field = rng.normal(size=(S, n + 200))
    field[:, off:off + n] = pr["field"]
    before, after = 45, 80
    loc = np.concatenate([rng.integers(1, off + 1, before), pr["obs_loc"] + off, rng.integers(off + n + 1, n + 201, after)])
    y = np.concatenate([rng.normal(size=before), pr["y"], rng.normal(size=after)])
    X = np.vstack([rng.normal(size=(before, 2)), pr["X"], rng.normal(size=(after, 2))])
    big = P.pointwise_loglik(y, loc, field, pr["lnv"], coef=pr["coef"], X=X, backend="hip", device=0, chunk_cols=64)
    np.testing.assert_array_equal(big[before:before + pr["y"].size], got[0])
    # the others' inputs altered: the embedded rows do not move
    y[:before] += 1.0
    X[-after:] *= 2.0
    field[:, :off] -= 3.0
    again = P.pointwise_loglik(y, loc, field, pr["lnv"], coef=pr["coef"], X=X, backend="hip", device=0)
    np.testing.assert_array_equal(again[before:before + pr["y"].size], got[0])
    assert not np.array_equal(again[:before], big[:before])


def test_shuffled_observations_come_back_in_order(P, chunked):
    pr, got = chunked
    perm = np.random.default_rng(53).permutation(pr["y"].size)
    sh = P.pointwise_loglik(pr["y"][perm], pr["obs_loc"][perm], pr["field"], pr["lnv"], coef=pr["coef"],
                            X=pr["X"][perm], backend="hip", device=0)
    np.testing.assert_array_equal(sh, got[0][perm])


def test_nan_isolation(P, ulp):
    pr = R.problem(TILE + 1, 65, 2, 54, per_loc=(1, 3))
    y, X, f = pr["y"].copy(), pr["X"].copy(), pr["field"].copy()
    y[5] = np.nan
    X[17, 1] = np.nan
    f[TILE, 40] = np.nan  # a column three or one observations read, in the partial tile
    bad = np.zeros(y.size, bool)
    bad[[5, 17]] = True
    bad |= pr["obs_loc"] == 41
    got = P.pointwise_loglik(y, pr["obs_loc"], f, pr["lnv"], coef=pr["coef"], X=X, backend="hip", device=0)
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all() and bad.sum() >= 3
    clean = _hip(P, pr)
    np.testing.assert_array_equal(got[~bad], clean[~bad])


def test_extreme_spread_on_the_device(P, ulp):
    pr = R.extreme_problem()
    got = _hip(P, pr)
    ref, bound, extra = _ref(pr, ulp)
    assert extra["ll_min"][0] < -780 and extra["ll_max"][0] > -2 and np.isfinite(got).all()
    ratio = R.worst_ratio(got, ref, bound)
    print(f"[pointwise hip extreme] lppd {got[0, 3]:.6f} log_cpo {got[0, 4]:.6f}  max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    far = dict(pr, field=pr["field"][np.arange(9) != 4], lnv=pr["lnv"][np.arange(9) != 4])
    got = _hip(P, far)
    ref, bound, _ = _ref(far, ulp)
    assert np.isfinite(got).all() and got[0, 3] < -700 and R.worst_ratio(got, ref, bound) <= 1.0


def test_identities_on_the_device(P, ulp):
    pr = R.problem(1, 40, 2, 55)
    one = _hip(P, pr)
    np.testing.assert_array_equal(one[:, 3], one[:, 1])
    np.testing.assert_array_equal(one[:, 4], one[:, 1])
    assert np.isnan(one[:, 2]).all()
    two = dict(pr, field=np.repeat(pr["field"], 2, 0), lnv=np.repeat(pr["lnv"], 2), coef=np.repeat(pr["coef"], 2, 0))
    got = _hip(P, two)
    np.testing.assert_array_equal(got[:, 2], 0.0)
    np.testing.assert_array_equal(got[:, [0, 1, 5]], one[:, [0, 1, 5]])  # x + x and its half are exact
    _, bound, _ = _ref(two, ulp)  # (M + log 2) - log 2 rounds
    assert np.all(np.abs(got[:, 3] - got[:, 1]) <= bound[:, 3] + bound[:, 1])
    assert np.all(np.abs(got[:, 4] - got[:, 1]) <= bound[:, 4] + bound[:, 1])


def test_blocks_are_read_where_they_lie(P):
    """A block given as the tail slice of a larger array gives the bits of a
    contiguous copy; the stack of several blocks those of the whole."""
    pr = R.problem(TILE + 5, 65, 1, 56)
    whole = _hip(P, pr)
    big = np.vstack([np.full((7, 65), np.nan), pr["field"]])
    view = big[7:]
    assert view.base is big and view.flags.c_contiguous
    np.testing.assert_array_equal(_hip(P, dict(pr, field=view)), whole)
    f = pr["field"]
    np.testing.assert_array_equal(_hip(P, dict(pr, field=[f[:3], f[3:3], big[10:]])), whole)


def test_current_device_is_unchanged(P):
    hip = C.CDLL("libamdhip64.so")
    pr = R.problem(2, 5, 1, 57)
    for dev in (0, -1):
        before, after = C.c_int(-7), C.c_int(-8)
        assert hip.hipGetDevice(C.byref(before)) == 0
        P.pointwise_loglik(pr["y"], pr["obs_loc"], pr["field"], pr["lnv"], coef=pr["coef"], X=pr["X"], backend="hip",
                           device=dev)
        assert hip.hipGetDevice(C.byref(after)) == 0 and after.value == before.value


def test_criteria_hip_is_the_direct_call(P):
    L = R.run_list(np.random.default_rng(58), n=70, extra_obs=30)
    got = P.mcmc_nngp_criteria(L, burn_in=0.5, backend="hip", device=0)
    host = P.mcmc_nngp_criteria(L, burn_in=0.5)
    recs = list(L["records"].values())
    direct = P.pointwise_loglik(
        L["observed_field"], L["vecchia_approx"]["locs_match"], [c["params"]["field"][10:] for c in recs],
        np.concatenate([c["params"]["log_noise_variance"][np.arange(22, 41, 2) - 1, 0] for c in recs]),
        coef=np.vstack([c["params"]["beta"][np.arange(22, 41, 2) - 1] for c in recs]), X=L["X"]["X"], backend="hip",
        device=0)
    np.testing.assert_array_equal(got["pointwise"], direct)
    assert got["n_samples"] == 20
    for k in ("lppd", "p_waic", "waic", "lpml", "dbar", "dhat", "p_dic", "dic"):
        assert abs(got[k] - host[k]) <= 1e-11 * (abs(host[k]) + abs(host["dbar"])), k


@pytest.fixture(scope="module")
def toy_fit(P, toy):
    """300 of the vignette toy's locations, 2 chains, 12 iterations with
    field_thinning = .5."""
    keep = np.random.default_rng(59).choice(len(toy["locs"]), 300, replace=False)
    L = P.mcmc_nngp_initialize(toy["locs"][keep], toy["observed_field"][keep], X_locs=toy["X"][keep],
                               stationary_covfun="exponential_isotropic", m=5, n_chains=2, seed=3)
    L = P.mcmc_nngp_run(L, n_cycles=1, n_iterations_update=12, n_chromatic=3, field_thinning=0.5,
                        Gelman_Rubin_Brooks_stop=(1.0, 1.0), verbose=False)
    yield L
    for c in L["_contexts"]:
        c.close()


def test_score_response_on_a_toy_fit(P, toy, toy_fit, ulp):
    from nngp_amd.predict import _stored_coef

    L = toy_fit
    rng = np.random.default_rng(60)
    lo, hi = L["locs"].min(0), L["locs"].max(0)
    pred = lo + (hi - lo) * rng.uniform(size=(65, L["locs"].shape[1]))
    Xp = rng.normal(size=(65, toy["X"].shape[1]))
    y_new = rng.normal(size=65) + float(np.mean(L["observed_field"]))
    kw = dict(m=5, seed=4, device=0)
    hip = P.mcmc_nngp_score_response(L, pred, Xp, y_new, **kw)
    samples = hip["field_prediction"]["predicted_field_samples"]
    mm, coef, stored = _stored_coef(L, Xp, 0.5, True, True)
    lnv = np.concatenate([c["params"]["log_noise_variance"][stored - 1, 0] for c in L["records"].values()])
    args = (y_new, np.arange(1, 66), np.vstack(samples), lnv, np.vstack(coef), mm)
    ref, bound, _ = R.reference(*args, **ulp)
    _, bound_host, _ = R.reference(*args, u_exp=4.0, u_log=4.0, u_erfc=8.0)
    ratio = R.worst_ratio(hip["pointwise"], ref, bound)
    # the host backend on the same predicted samples
    host = P.pointwise_loglik(y_new, np.arange(1, 66), samples, lnv, coef=np.vstack(coef), X=mm)
    both = float(np.max(np.abs(hip["pointwise"] - host) / (bound + bound_host)))
    again = P.mcmc_nngp_score_response(L, pred, Xp, y_new, backend="host", **kw)
    np.testing.assert_allclose(again["pointwise"], host, rtol=1e-9, atol=1e-9)  # its own prediction run
    print(f"[pointwise hip score_response S={len(lnv)}] max err / bound {ratio:.3f}; hip - host / bounds {both:.3f}")
    assert ratio <= 1.0 and both <= 1.0 and len(lnv) >= 4
    pit = hip["pointwise"][:, 5]
    np.testing.assert_array_equal(hip["pit"], pit)
    assert hip["coverage_95"] == np.mean((pit >= 0.025) & (pit <= 0.975))
    assert hip["log_score"] == hip["pointwise"][:, 3].mean() and hip["columns"] == P.POINTWISE_COLUMNS
    assert abs(hip["rmse"] - np.sqrt(np.mean((y_new - hip["pointwise"][:, 0]) ** 2))) <= 1e-15 * hip["rmse"]
