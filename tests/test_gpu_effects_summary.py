"""Fixed-effect / response samples generated and summarised on the device
(nngp_effects_summary, csrc/effects.hip).

Sample accuracy.  The value of sample s at location c is a length-q fma chain
followed by at most two more rounded operations (the addend's sum, the noise's
fma), so with eps = 2^-52

  |dev - exact| <= (q + 2) eps (sum_k |coef_sk X_ck| + |addend_sc| + |noise_sd_s z_sc|),

exact being the sum of the q + 2 products of the same doubles.  The reference
here carries every product as an error-free pair (Dekker's two-product) and
sums the pairs in compensated double-double arithmetic: its own error is below
2^-100 of the bound's sum, and a few entries of every case are held against
fractions.Fraction, which is exact.  z is nngp_device_normals(seed, counter[s]).

Shapes: S in {1, 2, 65} (the kernel's sample tile is 32 rows: 65 is two full
tiles and a tail of one), n in {1, 63, 65, 259} (259 = one 256-column
workgroup and three columns), q in {1, 2, 5, 17} (the k loop is unrolled by
two and starts at k = 1: 2 and 5 leave a remainder, 17 runs it eight times;
there is no other k-block), chunk_cols in {0, 64, 100} (at n = 259: one chunk;
five, the slots reused, the last of 3 columns; three, a chunk ending inside a
workgroup).

Everything else is bitwise: the summary is nngp_summary_probs' of the samples
returned, and a value depends on (s, c) and its inputs alone."""
import threading
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
WIDE_P, WIDE_T = (0.9, 0.0, 0.25, 1.0, 0.25, 0.5), (0.0, -np.inf, np.inf, 1.5)
SEED = 0x1234ABCD5678


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; no overflow at these magnitudes)."""
    p = a * b
    f = 134217729.0  # 2^27 + 1

    def split(x):
        t = f * x
        hi = t - (t - x)
        return hi, x - hi

    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _exact(coef, X, addend=None, sd=None, z=None):
    """(hi, lo, mag): hi + lo = the exact sample values (to ~2^-100 of mag),
    mag = the bound's sum of absolute terms; all S x n."""
    S, n = coef.shape[0], X.shape[0]
    terms = [(np.broadcast_to(coef[:, k][:, None], (S, n)), np.broadcast_to(X[:, k][None, :], (S, n)))
             for k in range(coef.shape[1])]
    if addend is not None:
        terms.append((np.ones((S, n)), addend))
    if sd is not None:
        terms.append((np.broadcast_to(sd[:, None], (S, n)), z))
    hi, lo, mag = np.zeros((S, n)), np.zeros((S, n)), np.zeros((S, n))
    for a, b in terms:
        p, e = _two_prod(a, b)
        hi, r = _two_sum(hi, p)
        lo = lo + (r + e)
        mag = mag + np.abs(p)
    return hi, lo, mag


def _normals(S, n, counter):
    from nngp_amd import _lib

    z = np.empty((S, n))
    for s in range(S):
        _lib.check(_lib.lib.nngp_device_normals(0, SEED, int(counter[s]), n, z[s]))
    return z


def _problem(S, n, q, seed=0):
    rng = np.random.default_rng([S, n, q, seed])
    coef = rng.normal(size=(S, q))
    # a row of mixed signs and magnitudes spread over 1e-8 .. 1e8
    coef[S // 2] = rng.choice([-1.0, 1.0], size=q) * 10.0 ** rng.uniform(-8, 8, size=q)
    X = rng.normal(size=(n, q)) * 10.0 ** rng.integers(-2, 3, size=(n, q))
    addend = 3.0 * rng.normal(size=(S, n))
    sd = rng.uniform(0.1, 2.0, size=S)
    counter = (np.arange(S)[::-1] + 5).astype(np.uint64)  # not the row's ordinal
    return coef, X, addend, sd, counter


def _dev(P, coef, X, **kw):
    return P.effects_summary(coef, X, backend="hip", device=0, seed=kw.pop("seed", SEED), return_samples=True, **kw)


def _assert_within_bound(samples, coef, X, addend=None, sd=None, z=None, what=""):
    hi, lo, mag = _exact(coef, X, addend, sd, z)
    q = coef.shape[1]
    err = np.abs((samples - hi) - lo)
    bound = (q + 2) * EPS * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[effects {what}] max err / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)
    # the reference itself against exact rational arithmetic, a few entries
    S, n = samples.shape
    for s, c in {(0, 0), (S // 2, n // 2), (S - 1, n - 1)}:
        ex = sum(Fraction(float(coef[s, k])) * Fraction(float(X[c, k])) for k in range(q))
        if addend is not None:
            ex += Fraction(float(addend[s, c]))
        if sd is not None:
            ex += Fraction(float(sd[s])) * Fraction(float(z[s, c]))
        ref_err = abs(Fraction(float(hi[s, c])) + Fraction(float(lo[s, c])) - ex)
        assert ref_err <= Fraction(float(mag[s, c])) * Fraction(1, 2 ** 90), (what, s, c)
        assert abs(Fraction(float(samples[s, c])) - ex) <= Fraction(float(bound[s, c])), (what, s, c)


@pytest.mark.parametrize("n", [1, 63, 64 + 1, 256 + 3])
@pytest.mark.parametrize("S", [1, 2, 65])
def test_samples_within_the_fma_chain_bound_and_summary_is_of_the_samples(P, S, n):
    z = _normals(S, n, _problem(S, n, 1)[4])
    for q in (1, 2, 5, 17):
        coef, X, addend, sd, counter = _problem(S, n, q)
        # plain for the default columns, addend + noise for the wide request
        summ, x = _dev(P, coef, X)
        _assert_within_bound(x, coef, X, what=f"S={S} n={n} q={q} plain")
        np.testing.assert_array_equal(summ, P.get_summary(x, backend="hip", device=0))
        summ, x = _dev(P, coef, X, addend=addend, noise_sd=sd, counter=counter, probs=WIDE_P, thresholds=WIDE_T)
        _assert_within_bound(x, coef, X, addend, sd, z, what=f"S={S} n={n} q={q} addend+noise")
        np.testing.assert_array_equal(summ, P.get_summary(x, backend="hip", device=0, probs=WIDE_P, thresholds=WIDE_T))
        assert summ.shape == (n, 2 + len(WIDE_P) + len(WIDE_T))
        if q == 5:  # each piece alone
            _, xa = _dev(P, coef, X, addend=addend)
            _assert_within_bound(xa, coef, X, addend, what=f"S={S} n={n} q={q} addend")
            _, xn = _dev(P, coef, X, noise_sd=sd, counter=counter)
            _assert_within_bound(xn, coef, X, None, sd, z, what=f"S={S} n={n} q={q} noise")


@pytest.fixture(scope="module")
def base(P):
    """S = 65, n = 259, q = 17: the problem and its results at chunk_cols = 0,
    plain / with the addend / with addend and noise."""
    coef, X, addend, sd, counter = _problem(65, 259, 17, seed=1)
    kw = dict(probs=WIDE_P, thresholds=WIDE_T)
    return {"coef": coef, "X": X, "addend": addend, "sd": sd, "counter": counter, "kw": kw,
            "plain": _dev(P, coef, X, **kw), "add": _dev(P, coef, X, addend=addend, **kw),
            "full": _dev(P, coef, X, addend=addend, noise_sd=sd, counter=counter, **kw)}


def _same(got, ref, cols=slice(None), what=""):
    np.testing.assert_array_equal(got[0], ref[0][cols], err_msg=f"{what}: summary")
    np.testing.assert_array_equal(got[1], ref[1][:, cols], err_msg=f"{what}: samples")


@pytest.mark.parametrize("chunk_cols", [64, 100])
def test_chunk_width_changes_no_bit(P, base, chunk_cols):
    b = base
    _same(_dev(P, b["coef"], b["X"], chunk_cols=chunk_cols, **b["kw"]), b["plain"], what="plain")
    _same(_dev(P, b["coef"], b["X"], addend=b["addend"], noise_sd=b["sd"], counter=b["counter"],
               chunk_cols=chunk_cols, **b["kw"]), b["full"], what="addend + noise")
    from nngp_amd import estimate

    st = estimate.effects_stats()
    assert st["chunk_cols"] == chunk_cols and st["staged_bytes"] == 8 * 65 * 259


def test_a_location_alone_and_reversed_columns(P, base):
    b = base
    for j in (0, 100, 258):
        _same(_dev(P, b["coef"], b["X"][j:j + 1], addend=b["addend"][:, j:j + 1], **b["kw"]), b["add"],
              cols=slice(j, j + 1), what=f"location {j} alone")
    # the noise of a location is z at its index: location 0 alone keeps it
    _same(_dev(P, b["coef"], b["X"][:1], addend=b["addend"][:, :1], noise_sd=b["sd"], counter=b["counter"],
               **b["kw"]), b["full"], cols=slice(0, 1), what="location 0 alone, noise")
    rev = _dev(P, b["coef"], b["X"][::-1], addend=b["addend"][:, ::-1], chunk_cols=100, **b["kw"])
    _same((rev[0][::-1], rev[1][:, ::-1]), b["add"], what="reversed columns")


def test_a_sample_row_alone(P, base):
    """S = 1 gives the bits the row has within S = 65 (first tile, second
    tile, the one-row tail)."""
    b = base
    for s in (0, 40, 64):
        _, x = _dev(P, b["coef"][s:s + 1], b["X"], addend=b["addend"][s:s + 1], noise_sd=b["sd"][s:s + 1],
                    counter=b["counter"][s:s + 1])
        np.testing.assert_array_equal(x[0], b["full"][1][s], err_msg=f"row {s}")
        _, x = _dev(P, b["coef"][s:s + 1], b["X"])
        np.testing.assert_array_equal(x[0], b["plain"][1][s], err_msg=f"row {s} plain")


def test_addend_blocks(P, base):
    b = base
    a = b["addend"]
    blocks = [a[:20].copy(), a[20:20].copy(), a[20:]]
    _same(_dev(P, b["coef"], b["X"], addend=blocks, **b["kw"]), b["add"], what="three blocks, one empty")
    _same(_dev(P, b["coef"], b["X"], addend=blocks, chunk_cols=64, **b["kw"]), b["add"], what="blocks, 64 columns")


def test_noise(P, base):
    b = base
    zero = _dev(P, b["coef"], b["X"], addend=b["addend"], noise_sd=np.zeros(65), counter=b["counter"], **b["kw"])
    assert np.all(zero[1] == b["add"][1]) and np.all(zero[0] == b["add"][0])  # ==: -0.0 may have become +0.0
    again = _dev(P, b["coef"], b["X"], addend=b["addend"], noise_sd=b["sd"], counter=b["counter"], **b["kw"])
    _same(again, b["full"], what="second call")
    # (where a value is 1e10 a small draw is below half an ulp: nearly all differ, and every row does)
    differs = b["full"][1] != b["add"][1]
    assert differs.mean() > 0.99 and np.all(differs.any(1))
    other = _dev(P, b["coef"], b["X"], addend=b["addend"], noise_sd=b["sd"], counter=b["counter"], seed=SEED + 1,
                 **b["kw"])
    assert (other[1] != b["full"][1]).mean() > 0.99
    # default counter: 0 .. S-1
    dflt = _dev(P, b["coef"], b["X"], noise_sd=b["sd"])
    np.testing.assert_array_equal(dflt[1], _dev(P, b["coef"], b["X"], noise_sd=b["sd"], counter=np.arange(65))[1])


def test_nan_and_inf_follow_ieee(P, base):
    b = base
    X = b["X"].copy()
    X[77, 3] = np.nan
    summ, x = _dev(P, b["coef"], X, addend=b["addend"], **b["kw"])
    keep = np.arange(259) != 77
    assert np.all(np.isnan(x[:, 77])) and np.all(np.isnan(summ[77]))
    np.testing.assert_array_equal(x[:, keep], b["add"][1][:, keep])
    np.testing.assert_array_equal(summ[keep], b["add"][0][keep])
    coef = np.array([[1.0, np.inf, 2.0], [np.inf, np.inf, 0.5], [-np.inf, 3.0, np.inf], [1.0, 2.0, 3.0]])
    Xs = np.array([[1.0, 2.0, 3.0], [1.0, -1.0, 1.0], [-2.0, 0.5, 0.25], [3.0, 1.0, -1.0], [0.0, 1.0, 1.0]])
    _, x = _dev(P, coef, Xs)
    with np.errstate(invalid="ignore"):
        ref = coef[:, :1] * Xs[:, 0][None, :]
        for k in (1, 2):
            ref = coef[:, k][:, None] * Xs[:, k][None, :] + ref
    assert np.isnan(ref).any() and np.isinf(ref).any()
    np.testing.assert_array_equal(x[:3], ref[:3])  # inf / NaN by IEEE (equal NaNs compare equal here)
    np.testing.assert_array_equal(np.isfinite(x[3]), np.ones(5, bool))


def test_stats_state(P, base):
    from nngp_amd import _lib, estimate

    b = base
    _dev(P, b["coef"], b["X"], chunk_cols=100)
    st = estimate.effects_stats()
    assert st["staged_bytes"] == 0 and st["chunk_cols"] == 100 and st["copy_ms"] == 0.0
    assert st["generate_ms"] > 0.0 and st["kernel_ms"] > 0.0
    _dev(P, b["coef"], b["X"])
    assert estimate.effects_stats()["chunk_cols"] == 259 and estimate.effects_stats()["staged_bytes"] == 0
    seen = []

    def fresh():
        try:
            estimate.effects_stats()
        except _lib.NNGPError as e:
            seen.append(e.status)

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen == [_lib.NNGP_ERR_STATE]


# ---- through the public functions
def _summary_close(got, dev_x, host_x, delta, probs, thr, what):
    """got: the device summary of dev_x (bitwise, checked by the caller's
    consistency assert) against numpy on host_x, whose entries differ from
    dev_x by at most delta per column: the bounds of
    tests/test_gpu_summary_probs.py on host_x, widened by delta (a quantile
    and a mean move by at most max|d|, an sd by at most 2 max|d|)."""
    S, n = host_x.shape
    assert np.all(np.abs(dev_x - host_x) <= delta[None, :]), what
    xs = np.sort(host_x, 0)
    for k, p in enumerate(probs):
        j = int(np.floor(p * (S - 1)))
        a, c = xs[j], xs[min(j + 1, S - 1)]
        d = np.abs(got[:, 1 + k] - np.quantile(host_x, p, axis=0))
        assert np.all(d <= 8 * EPS * np.maximum(np.abs(a), np.abs(c)) + delta), (what, p)
    assert np.all(np.abs(got[:, 0] - host_x.mean(0)) <= S * EPS * np.abs(host_x).mean(0) + delta), (what, "mean")
    ref = host_x.std(0, ddof=1)
    assert np.all(np.abs(got[:, 1 + len(probs)] - ref) <= (S + 4) * EPS * ref + 2 * delta), (what, "sd")
    for k, t in enumerate(thr):
        clear = np.abs(host_x - t).min(0) > delta  # no sample within delta of the threshold
        np.testing.assert_array_equal(got[clear, 2 + len(probs) + k], ((host_x > t).sum(0) / S)[clear])


def test_predict_fixed_effects_hip_agrees_with_host(P):
    from test_effects_summary import _run_list

    rng = np.random.default_rng(11)
    L = _run_list(rng, chains=2, iters=40, p=3, thin=2)
    Xp = rng.normal(size=(40, 3))
    probs, thr = (0.05, 0.5, 0.95), (0.0, 1.0)
    kw = dict(add_intercept=True, summary_probs=probs, summary_thresholds=thr)
    host = P.mcmc_nngp_predict_fixed_effects(L, Xp, **kw)
    got = P.mcmc_nngp_predict_fixed_effects(L, Xp, summary_backend="hip", device=0, **kw)
    assert got.keys() == host.keys()
    assert got["predicted_fixed_effects_summary_columns"] == host["predicted_fixed_effects_summary_columns"]
    assert [a.shape for a in got["predicted_fixed_effects_samples"]] == [(10, 40), (10, 40)]
    hx, dx = np.vstack(host["predicted_fixed_effects_samples"]), np.vstack(got["predicted_fixed_effects_samples"])
    np.testing.assert_array_equal(got["predicted_fixed_effects_summary"],
                                  P.get_summary(dx, backend="hip", device=0, probs=probs, thresholds=thr))
    # device and host samples are each within the sample bound of the exact value
    from nngp_amd.predict import _stored_coef

    mm, coef, _ = _stored_coef(L, Xp, 0.5, True, True)
    coef = np.vstack(coef)
    _assert_within_bound(dx, coef, mm, what="fixed effects")
    mag = np.abs(coef) @ np.abs(mm).T
    delta = (2 * (4 + 2) * EPS * mag).max(0)
    _summary_close(got["predicted_fixed_effects_summary"], dx, hx, delta, probs, thr, "fixed effects")
    lean = P.mcmc_nngp_predict_fixed_effects(L, Xp, summary_backend="hip", device=0, keep_samples=False, **kw)
    assert lean["predicted_fixed_effects_samples"] is None
    np.testing.assert_array_equal(lean["predicted_fixed_effects_summary"], got["predicted_fixed_effects_summary"])


@pytest.fixture(scope="module")
def toy_run(P, toy):
    """Vignette toy (n = 2000, m = 5), 2 chains, 30 iterations with
    field_thinning = .5, as tests/test_gpu_summary.py sets it up."""
    L = P.mcmc_nngp_initialize(toy["locs"], toy["observed_field"], X_locs=toy["X"],
                               stationary_covfun="exponential_isotropic", m=5, n_chains=2, seed=3)
    L = P.mcmc_nngp_run(L, n_cycles=1, n_iterations_update=30, n_chromatic=3, field_thinning=0.5,
                        Gelman_Rubin_Brooks_stop=(1.0, 1.0), verbose=False)
    yield L
    for c in L["_contexts"]:
        c.close()


def test_predict_response_on_the_vignette_toy(P, toy, toy_run):
    from nngp_amd.predict import PHILOX_RESPONSE_MIX, _stored_coef

    L = toy_run
    rng = np.random.default_rng(5)
    lo, hi = L["locs"].min(0), L["locs"].max(0)
    pred = lo + (hi - lo) * rng.uniform(size=(30, L["locs"].shape[1]))
    Xp = rng.normal(size=(30, toy["X"].shape[1]))
    probs, thr = (0.05, 0.5, 0.95), (0.0,)
    r = P.mcmc_nngp_predict_response(L, pred, Xp, m=5, seed=4, device=0, summary_probs=probs, summary_thresholds=thr)
    assert r["predicted_response_summary_columns"] == ["mean", "q0.05", "q0.5", "q0.95", "sd", "p_gt_0"]
    assert r["predicted_response_summary"].shape == (30, 6)
    field = P.mcmc_nngp_predict_field(L, pred, m=5, seed=4, device=0, engine="batched")
    fs = field["predicted_field_samples"]
    for a, b in zip(fs, r["field_prediction"]["predicted_field_samples"]):
        np.testing.assert_array_equal(a, b)
    mm, coef, stored = _stored_coef(L, Xp, 0.5, True, True)
    coef = np.vstack(coef)
    assert coef.shape[0] == sum(len(a) for a in fs) >= 4 and mm.shape == (30, 1 + Xp.shape[1])
    by_hand, x = P.effects_summary(coef, mm, addend=fs, probs=probs, thresholds=thr, backend="hip", device=0,
                                   return_samples=True)
    np.testing.assert_array_equal(r["predicted_response_summary"], by_hand)
    # mean of the sum against the sum of the means: three means of S values
    # (each within S eps mean|x| of its exact mean) and one rounded sum per sample
    S = coef.shape[0]
    f, fe = np.vstack(fs), coef @ mm.T
    mag = np.abs(coef) @ np.abs(mm).T + np.abs(f)
    bound = S * EPS * (np.abs(x).mean(0) + np.abs(f).mean(0) + np.abs(fe).mean(0)) \
        + ((mm.shape[1] + 2) * EPS * mag).mean(0) * 2
    d = np.abs(by_hand[:, 0] - (f.mean(0) + fe.mean(0)))
    print(f"[response] max mean err / bound = {(d / bound).max():.3f}")
    assert np.all(d <= bound)
    host = P.mcmc_nngp_predict_response(L, pred, Xp, m=5, seed=4, device=0, summary_backend="host",
                                        summary_probs=probs, summary_thresholds=thr)
    np.testing.assert_allclose(host["predicted_response_summary"][:, :5], by_hand[:, :5], rtol=1e-10, atol=1e-12)
    # noise: the same call with noise_sd, the response key and the stack ordinals
    noisy = P.mcmc_nngp_predict_response(L, pred, Xp, m=5, seed=4, device=0, noise=True, summary_probs=probs,
                                         summary_thresholds=thr)
    sd = np.concatenate([np.exp(0.5 * c["params"]["log_noise_variance"][stored - 1, 0])
                         for c in L["records"].values()])
    hand = P.effects_summary(coef, mm, addend=fs, noise_sd=sd, seed=(4 + PHILOX_RESPONSE_MIX) % 2 ** 64,
                             counter=np.arange(S), probs=probs, thresholds=thr, backend="hip", device=0)
    np.testing.assert_array_equal(noisy["predicted_response_summary"], hand)
    assert np.all(noisy["predicted_response_summary"][:, 0] != by_hand[:, 0])
